// wav2vec 2.0 front end of the UnitExtractor (reference models/unit_extractor/unit_extractor.py:91-98 and the fairseq2
// Wav2Vec2Frontend it calls): utterance normalisation, the first feature-extractor layer, the grouped convolutional position
// encoder, and the operand packers of the k-means arg-max.  The remaining extractor layers are implicit-convolution products
// (k_gemm*.hip), the Transformer layers the usual LayerNorm / product / attention launches.
//
// All arithmetic here is plain fp32 FMA (utterance statistics in double): the first layer has one input channel - 10
// multiplies per output - and is bound by writing its [frames][512] result once; the position convolution carries fp32
// weights (weight-norm folded, not representable in fp16) and is 2 * 80 * 128 flops per output element.
#include <algorithm>

#include "device_util.h"

namespace sc {

namespace {

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// block-wide sum of a double (1024 threads = 16 waves), result to every thread
__device__ __forceinline__ double block_sum_d(double v, double* sh) {
    v = wave_sum_d(v);
    __syncthreads();  // sh may still be read from the previous reduction
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += sh[w];
    return t;
}

// sample i of an item with ns real samples: the waveform, one 1.0 behind an odd length, zeros further out
__device__ __forceinline__ float wave_at(const float* w, int ns, int i) { return i < ns ? w[i] : (i == ns && (ns & 1)) ? 1.0f : 0.0f; }

__global__ __launch_bounds__(1024) void wave_stats_kernel(const float* __restrict__ wav, int64_t wav_stride, const int* __restrict__ num_samples,
                                                          float* __restrict__ stats) {
    __shared__ double sh[16];
    const int b = blockIdx.x;
    const int ns = num_samples[b], nsp = ns + (ns & 1);
    const float* w = wav + (int64_t)b * wav_stride;
    double acc = 0.0;
    for (int i = threadIdx.x; i < nsp; i += blockDim.x) acc += (double)wave_at(w, ns, i);
    const double mean = block_sum_d(acc, sh) / (double)nsp;
    acc = 0.0;
    for (int i = threadIdx.x; i < nsp; i += blockDim.x) {
        const double d = (double)wave_at(w, ns, i) - mean;
        acc += d * d;
    }
    const double var = block_sum_d(acc, sh) / (double)nsp;
    if (threadIdx.x == 0) {
        stats[2 * b] = (float)mean;
        stats[2 * b + 1] = (float)(1.0 / sqrt(var + 1e-5));
    }
}

constexpr int C0_FR = 8;      // frames per workgroup
constexpr int C0_MAXK = 16;   // taps
constexpr int C0_MAXC = 1024;

// 256 threads: phase 1 every thread owns channels tid, tid + 256, ... and computes them for the workgroup's 8 frames into LDS;
// phase 2 every wave owns two frames: mean, centred variance, affine, GELU, 16-byte stores.
__global__ __launch_bounds__(256) void conv0_kernel(const float* __restrict__ wav, int64_t wav_stride, const int* __restrict__ num_samples,
                                                    const float* __restrict__ stats, const float* __restrict__ w, const float* __restrict__ bias,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta, int C, int k, int stride,
                                                    float* __restrict__ out, int t_rows) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* sx = sm;                                // [(C0_FR - 1) * stride + k] normalised samples
    float* sy = sm + ((C0_FR - 1) * stride + k + 3) / 4 * 4;  // [C0_FR][C]
    const int b = blockIdx.y, t0 = blockIdx.x * C0_FR, tid = threadIdx.x;
    const int ns = num_samples[b];
    const float* wv = wav + (int64_t)b * wav_stride;
    const float mean = stats[2 * b], rstd = stats[2 * b + 1];
    const int nx = (C0_FR - 1) * stride + k, nsp = ns + (ns & 1);
    for (int i = tid; i < nx; i += 256) {
        const int si = t0 * stride + i;
        sx[i] = si < nsp ? (wave_at(wv, ns, si) - mean) * rstd : 0.f;
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        float wr[C0_MAXK];
#pragma unroll
        for (int j = 0; j < C0_MAXK; ++j) wr[j] = j < k ? w[c * k + j] : 0.f;
        const float bc = bias[c];
#pragma unroll
        for (int f = 0; f < C0_FR; ++f) {
            float acc = bc;
#pragma unroll
            for (int j = 0; j < C0_MAXK; ++j)
                if (j < k) acc = fmaf(wr[j], sx[f * stride + j], acc);
            sy[f * C + c] = acc;
        }
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    for (int f = wave; f < C0_FR; f += 4) {
        const int t = t0 + f;
        if (t >= t_rows) break;
        const float* yr = sy + f * C;
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s += yr[c];
        const float mu = wave_sum(s) / (float)C;
        float q = 0.f;
        for (int c = lane; c < C; c += 64) {
            const float d = yr[c] - mu;
            q += d * d;
        }
        const float rs = 1.0f / sqrtf(wave_sum(q) / (float)C + 1e-5f);
        float* orow = out + ((int64_t)b * t_rows + t) * C;
        for (int c4 = lane; c4 < C / 4; c4 += 64) {
            const float4 y = *reinterpret_cast<const float4*>(yr + 4 * c4);
            const float4 g = *reinterpret_cast<const float4*>(gamma + 4 * c4);
            const float4 be = *reinterpret_cast<const float4*>(beta + 4 * c4);
            float4 o;
            o.x = gelu_erf((y.x - mu) * rs * g.x + be.x);
            o.y = gelu_erf((y.y - mu) * rs * g.y + be.y);
            o.z = gelu_erf((y.z - mu) * rs * g.z + be.z);
            o.w = gelu_erf((y.w - mu) * rs * g.w + be.w);
            *reinterpret_cast<float4*>(orow + 4 * c4) = o;
        }
    }
}

// [C][cg][k] -> [group][tap][c_in][c_out]
__global__ void pack_pos_weight_kernel(const float* __restrict__ w, float* __restrict__ dst, int C, int cg, int k) {
    const int64_t total = (int64_t)C * cg * k;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int co_l = (int)(i % cg);
        const int ci = (int)((i / cg) % cg);
        const int tap = (int)((i / ((int64_t)cg * cg)) % k);
        const int g = (int)(i / ((int64_t)cg * cg * k));
        dst[i] = w[((int64_t)(g * cg + co_l) * cg + ci) * k + tap];
    }
}

constexpr int PC_TT = 32;  // output rows per workgroup
constexpr int PC_TY = 4;   // thread rows; a thread owns PC_TT / PC_TY output rows of one output channel

// grid (time tiles, groups, items), block (cg, 4): the input window [32 + k - 1][cg] of the group sits in LDS (rows outside
// [0, len) as zeros); thread (c, ty) accumulates output channel c of rows ty, ty + 4, ... - the weight read is coalesced over
// c and shared by the four thread rows through the cache, the input read is an LDS broadcast.
__global__ __launch_bounds__(512) void pos_conv_kernel(const float* __restrict__ x, const float* __restrict__ wp, const float* __restrict__ bias,
                                                       float* __restrict__ y, int T, int C, int cg, int k, const int* __restrict__ lens) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int g = blockIdx.y, b = blockIdx.z, t0 = blockIdx.x * PC_TT;
    const int c = threadIdx.x, ty = threadIdx.y, tid = ty * cg + c, nthr = cg * PC_TY;
    const int len = lens ? min(lens[b], T) : T;
    const int pad = k / 2, win = PC_TT + k - 1;
    const float* xb = x + (int64_t)b * T * C + g * cg;
    for (int i = tid; i < win * cg; i += nthr) {
        const int r = i / cg, ci = i - r * cg;
        const int t = t0 - pad + r;
        sm[i] = (t >= 0 && t < len) ? xb[(int64_t)t * C + ci] : 0.f;
    }
    __syncthreads();
    constexpr int NR = PC_TT / PC_TY;
    float acc[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = 0.f;
    const float* wg = wp + (int64_t)g * k * cg * cg + c;
    for (int tap = 0; tap < k; ++tap) {
        const float* wt = wg + (int64_t)tap * cg * cg;
        const float* xs = sm + (tap + ty) * cg;
        for (int ci = 0; ci < cg; ++ci) {
            const float wv = wt[ci * cg];
#pragma unroll
            for (int r = 0; r < NR; ++r) acc[r] = fmaf(wv, xs[(r * PC_TY) * cg + ci], acc[r]);
        }
    }
    const float bc = bias[g * cg + c];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int t = t0 + ty + r * PC_TY;
        if (t < T) {
            const int64_t o = ((int64_t)b * T + t) * C + g * cg + c;
            y[o] = x[o] + gelu_erf(acc[r] + bc);
        }
    }
}

__global__ void dup_split_kernel(const float* __restrict__ x, int64_t ldx, int rows, int C, __half* __restrict__ hi, __half* __restrict__ lo) {
    const int64_t total = (int64_t)rows * C;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / C;
        const int c = (int)(i - r * C);
        const float v = x[r * ldx + c];
        const __half h = __float2half_rn(v);
        const __half l = __float2half_rn(v - __half2float(h));
        const int64_t o = r * 2 * C + c;
        hi[o] = h;
        hi[o + C] = h;
        lo[o] = l;
        lo[o + C] = l;
    }
}

// one wave per centroid
__global__ __launch_bounds__(256) void pack_centroids_kernel(const float* __restrict__ cent, int C, int K, __half* __restrict__ W,
                                                             float* __restrict__ bias) {
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= K) return;
    float q = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float v = cent[(int64_t)c * K + j];
        const __half h = __float2half_rn(v);
        const __half l = __float2half_rn(v - __half2float(h));
        W[(int64_t)j * 2 * C + c] = h;
        W[(int64_t)j * 2 * C + C + c] = l;
        const float s = __half2float(h) + __half2float(l);
        q = fmaf(s, s, q);
    }
    q = wave_sum(q);
    if (lane == 0) bias[j] = -0.5f * q;
}

}  // namespace

void launch_w2v2_wave_stats(const float* wav, int64_t wav_stride, const int* num_samples, int nb, float* stats, hipStream_t s) {
    SC_CHECK(wav && num_samples && stats && nb > 0, "w2v2_wave_stats: bad argument");
    prof::Scope scope("w2v2_wave_stats", 0, 0, s);
    hipLaunchKernelGGL(wave_stats_kernel, dim3(nb), dim3(1024), 0, s, wav, wav_stride, num_samples, stats);
    SC_LAUNCH_CHECK();
}

void launch_w2v2_conv0(const float* wav, int64_t wav_stride, const int* num_samples, const float* stats, int nb, const float* w,
                       const float* bias, const float* gamma, const float* beta, int C, int k, int stride, float* out, int t_rows,
                       hipStream_t s) {
    SC_CHECK(wav && num_samples && stats && w && bias && gamma && beta && out, "w2v2_conv0: null argument");
    SC_CHECK(nb > 0 && nb <= 65535 && t_rows > 0, "w2v2_conv0: nb=%d t_rows=%d", nb, t_rows);
    SC_CHECK(C > 0 && C % 4 == 0 && C <= C0_MAXC && k >= 1 && k <= C0_MAXK && stride >= 1 && stride <= 64,
             "w2v2_conv0: C=%d (multiple of 4, <= %d) k=%d (<= %d) stride=%d", C, C0_MAXC, k, C0_MAXK, stride);
    SC_CHECK((reinterpret_cast<uintptr_t>(out) & 15) == 0 && (reinterpret_cast<uintptr_t>(gamma) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(beta) & 15) == 0,
             "w2v2_conv0: out / gamma / beta must be 16-byte aligned");
    const size_t lds = ((size_t)((C0_FR - 1) * stride + k + 3) / 4 * 4 + (size_t)C0_FR * C) * 4;
    prof::Scope scope("w2v2_conv0", 2.0 * nb * t_rows * (double)C * k, 4.0 * nb * t_rows * (double)C, s);
    hipLaunchKernelGGL(conv0_kernel, dim3(cdiv(t_rows, C0_FR), nb), dim3(256), lds, s, wav, wav_stride, num_samples, stats, w, bias, gamma, beta,
                       C, k, stride, out, t_rows);
    SC_LAUNCH_CHECK();
}

void launch_w2v2_pack_pos_weight(const float* w, float* dst, int C, int groups, int k, hipStream_t s) {
    SC_CHECK(w && dst && C > 0 && groups > 0 && C % groups == 0 && k > 0, "w2v2_pack_pos_weight: C=%d groups=%d k=%d", C, groups, k);
    const int cg = C / groups;
    const int64_t total = (int64_t)C * cg * k;
    hipLaunchKernelGGL(pack_pos_weight_kernel, dim3((unsigned)std::min<int64_t>(cdiv64(total, 256), 4096)), dim3(256), 0, s, w, dst, C, cg, k);
    SC_LAUNCH_CHECK();
}

void launch_w2v2_pos_conv(const float* x, const float* w_packed, const float* bias, float* y, int nb, int T, int C, int groups, int k,
                          const int* lens, hipStream_t s) {
    SC_CHECK(x && w_packed && bias && y && x != y, "w2v2_pos_conv: null or aliased argument");
    SC_CHECK(nb > 0 && nb <= 65535 && T > 0 && C > 0 && groups > 0 && groups <= 65535 && C % groups == 0 && k >= 2 && k % 2 == 0 && k <= 256,
             "w2v2_pos_conv: nb=%d T=%d C=%d groups=%d k=%d (k even, <= 256)", nb, T, C, groups, k);
    const int cg = C / groups;
    SC_CHECK(cg <= 128, "w2v2_pos_conv: %d channels per group > 128", cg);
    const size_t lds = (size_t)(PC_TT + k - 1) * cg * 4;  // at most 287 * 128 * 4 = 146 944 B
    // the default limit holds up to 64 KB (XLS-R: 159 * 80 * 4 = 50 880 B); wider groups raise it (idempotent, per device)
    if (lds > 64 * 1024)
        SC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&pos_conv_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
    prof::Scope scope("w2v2_pos_conv", 2.0 * nb * T * (double)C * cg * k, 8.0 * nb * T * (double)C + 4.0 * C * (double)cg * k, s);
    hipLaunchKernelGGL(pos_conv_kernel, dim3(cdiv(T, PC_TT), groups, nb), dim3(cg, PC_TY), lds, s, x, w_packed, bias, y, T, C, cg, k, lens);
    SC_LAUNCH_CHECK();
}

void launch_w2v2_dup_split(const float* x, int64_t ldx, int rows, int C, __half* hi, __half* lo, hipStream_t s) {
    SC_CHECK(x && hi && lo && rows > 0 && C > 0, "w2v2_dup_split: bad argument");
    const int64_t total = (int64_t)rows * C;
    hipLaunchKernelGGL(dup_split_kernel, dim3((unsigned)std::min<int64_t>(cdiv64(total, 256), 8192)), dim3(256), 0, s, x, ldx, rows, C, hi, lo);
    SC_LAUNCH_CHECK();
}

void launch_w2v2_pack_centroids(const float* cent, int C, int K, __half* W, float* bias, hipStream_t s) {
    SC_CHECK(cent && W && bias && C > 0 && K > 0, "w2v2_pack_centroids: bad argument");
    hipLaunchKernelGGL(pack_centroids_kernel, dim3(cdiv(K, 4)), dim3(256), 0, s, cent, C, K, W, bias);
    SC_LAUNCH_CHECK();
}

}  // namespace sc
