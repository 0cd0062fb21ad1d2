// ECAPA-TDNN prosody encoder (reference models/pretssel/ecapa_tdnn.py, arch `base`): the kernels between its products.
//
//   ecapa_chain_kernel    Res2NetBlock.forward (:250-263): the scale - 1 dependent TDNN stages of one SE-Res2Net block
//                         (Conv1d(w -> w, k = 3, dilation d) + ReLU + LayerNorm(w), input x_i + y_{i-1}) and the pass-through
//                         chunk in ONE launch.  A workgroup of 8 waves owns EC_ROWS = 256 consecutive frames of one item, of
//                         which the middle 256 - 2 (scale - 1) d are stored: rows are addressed in place (tile row j is frame
//                         t_first + j at every stage) and every stage makes d more rows per side meaningless, as in the
//                         vocoder's fused MRF kernel (k_resblock.hip).  The running chunk y lives in the accumulator layout in
//                         registers (lane = column, 16 rows per lane); only the hi/lo fp16 planes of x_i + y_{i-1} are in LDS,
//                         where the three taps read them as MFMA A fragments; a stage's w x 3w fp16 weights are staged in LDS
//                         in front of its product.  Frames outside [0, T) are zeros at the input of EVERY stage (the zero
//                         padding each Conv1d of the reference sees), T being the padded batch length: TDNN blocks ignore the
//                         item lengths.  The LayerNorm of a row is a reduction over the 32 lanes of a half wave.
//   ecapa_relu_ln_kernel  the epilogue of every other TDNN block: ReLU + LayerNorm over the channels (eps 1e-12) in one pass,
//                         optionally with a per-item bias in front (the time-constant part of the pooling's 3C-wide product)
//                         and tanh behind.
//   ecapa_se_gate_kernel  SEBlock.forward (:296-309) up to the gate: masked time mean, both 1 x 1 products, sigmoid; one
//                         workgroup per item.  ecapa_se_apply_kernel: gate * y + residual into the block's slice of the
//                         [B][T][3C] concat buffer.
//   ecapa_gstats_kernel / ecapa_item_bias_kernel / ecapa_pool_kernel   AttentiveStatisticsPooling.forward (:341-394): masked
//                         mean / std per (item, channel); W[:, C:3C] . [mean | std] + b per item; masked softmax over time per
//                         channel with the weighted mean and the std AROUND that mean (as the reference forms it).
//   ecapa_tail_kernel     asp_norm + fc + F.normalize (:137-143), one workgroup per item.
//   ecapa_gcmvn_kernel    (x - mean) / std on the frames in front of an item's length, zeros behind.
#include <algorithm>

#include "device_util.h"

namespace sc {

namespace {

constexpr int EC_ROWS = 256;     // frames a workgroup computes per stage: 8 waves x one 32-row MFMA fragment
constexpr int EC_G = 8;          // zero guard rows on both sides of the planes = the largest dilation
constexpr int EC_THREADS = 512;
constexpr float EC_EPS = 1e-12f;

__device__ __forceinline__ float half_wave_sum(float v) {  // over the 32 lanes that share lane >> 5
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

template <int CW>
__global__ __launch_bounds__(EC_THREADS) void ecapa_chain_kernel(EcapaChainArgs p, int tiles) {
    constexpr int CS = CW + 8;   // halfs per plane row: 16-byte fragment reads of consecutive rows hit distinct banks
    constexpr int NF = CW / 32;  // 32-column output fragments
    constexpr int CPT = CW / 16; // 16-wide K chunks per tap
    constexpr int PR = EC_ROWS + 2 * EC_G;
    constexpr int LDB = 3 * CW + 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char ec_smem[];
    _Float16* const ph = reinterpret_cast<_Float16*>(ec_smem);
    _Float16* const pl = ph + PR * CS;
    _Float16* const sW = pl + PR * CS;  // [CW][LDB]: the packed (tap-major) weight rows of the running stage

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
    const int T = p.T, dil = p.dil;
    const int halo = (p.scale - 1) * dil, TT = EC_ROWS - 2 * halo;
    const int t_first = tile * TT - halo;  // frame of tile row 0
    const float* __restrict__ xn = p.x + (int64_t)n * T * p.ldx;
    float* __restrict__ on = p.out + (int64_t)n * T * p.ldo;

    {   // planes start as zeros; the guard rows stay zero
        const half8_t z = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = tid; i < 2 * PR * CS / 8; i += EC_THREADS) reinterpret_cast<half8_t*>(ph)[i] = z;
    }
    // chunk 0 passes through untouched
    for (int i = tid; i < TT * (CW / 4); i += EC_THREADS) {
        const int r = i / (CW / 4), c4 = i - r * (CW / 4);
        const int t = tile * TT + r;
        if (t < T) *reinterpret_cast<f32x4_t*>(on + (int64_t)t * p.ldo + c4 * 4) = *reinterpret_cast<const f32x4_t*>(xn + (int64_t)t * p.ldx + c4 * 4);
    }
    __syncthreads();

    const int col0 = lane & 31, koff = (lane >> 5) * 8;
    const int jbase = 32 * wave + 4 * (lane >> 5);  // tile row of accumulator register r: jbase + (r & 3) + 8 * (r >> 2)
    float y[NF][16];
#pragma unroll
    for (int nf = 0; nf < NF; ++nf)
#pragma unroll
        for (int r = 0; r < 16; ++r) y[nf][r] = 0.f;

    for (int s = 1; s < p.scale; ++s) {
        // ---- hi/lo planes of x_s + y_{s-1}, zeros outside [0, T); this stage's weights ------------------------------
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) {
            const int col = nf * 32 + col0;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = jbase + (r & 3) + 8 * (r >> 2);
                const int t = t_first + j;
                float v = 0.f;
                if (t >= 0 && t < T) v = xn[(int64_t)t * p.ldx + s * CW + col] + y[nf][r];
                split1(v, ph[(EC_G + j) * CS + col], pl[(EC_G + j) * CS + col]);
            }
        }
        {
            const __half* __restrict__ W = p.w[s - 1];
            constexpr int VPR = 3 * CW / 8;
            for (int i = tid; i < CW * VPR; i += EC_THREADS) {
                const int c = i / VPR, v = i - c * VPR;
                *reinterpret_cast<half8_t*>(sW + c * LDB + v * 8) = *reinterpret_cast<const half8_t*>(W + (int64_t)c * p.ldw + v * 8);
            }
        }
        __syncthreads();
        // ---- product: output row j reads plane rows j - dil, j, j + dil ---------------------------------------------
        float16_t acc[NF];
#pragma unroll
        for (int nf = 0; nf < NF; ++nf)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nf][r] = 0.f;
        const int a_base = (EC_G + 32 * wave + col0 - dil) * CS + koff;
        for (int tap = 0; tap < 3; ++tap) {
#pragma unroll
            for (int cc = 0; cc < CPT; ++cc) {
                const int a_off = a_base + tap * dil * CS + cc * 16;
                const half8_t ah = *reinterpret_cast<const half8_t*>(ph + a_off);
                const half8_t al = *reinterpret_cast<const half8_t*>(pl + a_off);
#pragma unroll
                for (int nf = 0; nf < NF; ++nf) {
                    const half8_t b = *reinterpret_cast<const half8_t*>(sW + (nf * 32 + col0) * LDB + koff + (tap * CPT + cc) * 16);
                    acc[nf] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, b, acc[nf], 0, 0, 0);
                    acc[nf] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, b, acc[nf], 0, 0, 0);
                }
            }
        }
        __syncthreads();  // every wave is done with the planes and the weights: the next stage may overwrite them
        // ---- bias, ReLU, LayerNorm over the CW columns of each row; store the rows this tile owns -------------------
        float bs[NF], ga[NF], be[NF];
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) {
            bs[nf] = p.bias[s - 1][nf * 32 + col0];
            ga[nf] = p.gamma[s - 1][nf * 32 + col0];
            be[nf] = p.beta[s - 1][nf * 32 + col0];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v[NF], sum = 0.f;
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) {
                v[nf] = relu_keep_nan(acc[nf][r] + bs[nf]);
                sum += v[nf];
            }
            const float mean = half_wave_sum(sum) * (1.0f / CW);
            float sq = 0.f;
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) {
                v[nf] -= mean;
                sq += v[nf] * v[nf];
            }
            const float inv = 1.0f / sqrtf(half_wave_sum(sq) * (1.0f / CW) + EC_EPS);
            const int j = jbase + (r & 3) + 8 * (r >> 2);
            const int t = t_first + j;
            const bool store = j >= halo && j < halo + TT && t < T;
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) {
                const float o = v[nf] * inv * ga[nf] + be[nf];
                y[nf][r] = o;
                if (store) on[(int64_t)t * p.ldo + s * CW + nf * 32 + col0] = o;
            }
        }
    }
}

// one wave per row: y = act(LayerNorm(relu(x + item_bias)))
__global__ __launch_bounds__(256) void ecapa_relu_ln_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ item_bias, int t_per_item,
                                                            const float* __restrict__ g, const float* __restrict__ b, float* y, int64_t ldy, int rows,
                                                            int C, int act) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* xr = x + (int64_t)row * ldx;
    const float* ib = item_bias ? item_bias + (int64_t)(row / t_per_item) * C : nullptr;
    float sum = 0.f;
    for (int c = lane; c < C; c += 64) sum += relu_keep_nan(xr[c] + (ib ? ib[c] : 0.f));
    const float mean = wave_sum(sum) / (float)C;
    float sq = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float d = relu_keep_nan(xr[c] + (ib ? ib[c] : 0.f)) - mean;
        sq += d * d;
    }
    const float inv = 1.0f / sqrtf(wave_sum(sq) / (float)C + EC_EPS);
    float* yr = y + (int64_t)row * ldy;
    for (int c = lane; c < C; c += 64) {  // y may be x: a lane reads an element before it writes the same element
        float o = (relu_keep_nan(xr[c] + (ib ? ib[c] : 0.f)) - mean) * inv * g[c] + b[c];
        if (act == ACT_TANH) o = tanhf(o);
        yr[c] = o;
    }
}

// one workgroup per item: s = masked time mean [C]; h = relu(W1 s + b1) [S]; gate = sigmoid(W2 h + b2) [C]
__global__ __launch_bounds__(1024) void ecapa_se_gate_kernel(const float* __restrict__ x, int64_t ldx, int T, const int* __restrict__ lens, int C, int S,
                                                             const __half* __restrict__ w1, const float* __restrict__ b1, const __half* __restrict__ w2,
                                                             const float* __restrict__ b2, float* __restrict__ gate) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ec_smem[];
    float* part = reinterpret_cast<float*>(ec_smem);  // [groups][C]
    float* sm = part + 4096;                          // [C]
    float* hh = sm + C;                               // [S]
    const int n = blockIdx.x, tid = threadIdx.x;
    const int len = lens ? lens[n] : T;
    const int vpr = C / 4, groups = 1024 / vpr;
    const float* xn = x + (int64_t)n * T * ldx;
    if (tid < groups * vpr) {
        const int tg = tid / vpr, c4 = tid - tg * vpr;
        f32x4_t a = {0.f, 0.f, 0.f, 0.f};
        for (int t = tg; t < len; t += groups) a += *reinterpret_cast<const f32x4_t*>(xn + (int64_t)t * ldx + c4 * 4);
        *reinterpret_cast<f32x4_t*>(part + tg * C + c4 * 4) = a;
    }
    __syncthreads();
    for (int c = tid; c < C; c += 1024) {
        float a = 0.f;
        for (int gidx = 0; gidx < groups; ++gidx) a += part[gidx * C + c];
        sm[c] = a / (float)len;
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    for (int j = wave; j < S; j += 16) {
        float a = 0.f;
        for (int c = lane; c < C; c += 64) a += __half2float(w1[(int64_t)j * C + c]) * sm[c];
        a = wave_sum(a);
        if (lane == 0) hh[j] = relu_keep_nan(a + b1[j]);
    }
    __syncthreads();
    for (int c = tid; c < C; c += 1024) {
        float a = 0.f;
        for (int j = 0; j < S; ++j) a += __half2float(w2[(int64_t)c * S + j]) * hh[j];
        gate[(int64_t)n * C + c] = 1.0f / (1.0f + expf(-(a + b2[c])));
    }
}

__global__ __launch_bounds__(256) void ecapa_se_apply_kernel(const float* __restrict__ yv, int64_t ldy, const float* __restrict__ gate,
                                                             const float* __restrict__ res, int64_t ldr, float* __restrict__ out, int64_t ldo, int T,
                                                             int C, int64_t total4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int vpr = C / 4;
    const int64_t row = i / vpr;
    const int c = (int)(i - row * vpr) * 4;
    const int n = (int)(row / T);
    const f32x4_t v = *reinterpret_cast<const f32x4_t*>(yv + row * ldy + c) * *reinterpret_cast<const f32x4_t*>(gate + (int64_t)n * C + c) +
                      *reinterpret_cast<const f32x4_t*>(res + row * ldr + c);
    *reinterpret_cast<f32x4_t*>(out + row * ldo + c) = v;
}

// Column kernels: a workgroup owns 64 channels of one item, 4 time groups x 64 lanes; frames behind the length are never read.
__device__ __forceinline__ float col_reduce_sum(float v, float* red, int tg, int cl) {
    __syncthreads();
    red[tg * 64 + cl] = v;
    __syncthreads();
    return (red[cl] + red[64 + cl]) + (red[128 + cl] + red[192 + cl]);
}
__device__ __forceinline__ float col_reduce_max(float v, float* red, int tg, int cl) {
    __syncthreads();
    red[tg * 64 + cl] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[cl], red[64 + cl]), fmaxf(red[128 + cl], red[192 + cl]));
}

// gstats[n][c] = mean, gstats[n][C + c] = sqrt(max(sum((x - mean)^2) / len, 1e-12)) over the frames t < len
__global__ __launch_bounds__(256) void ecapa_gstats_kernel(const float* __restrict__ x, int T, int C, const int* __restrict__ lens,
                                                           float* __restrict__ gstats) {
    __shared__ float red[256];
    const int n = blockIdx.y, cl = threadIdx.x & 63, tg = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const bool ok = c < C;
    const int len = lens ? lens[n] : T;
    const float* xc = x + (int64_t)n * T * C + (ok ? c : 0);
    float a = 0.f;
    for (int t = tg; t < len; t += 4) a += xc[(int64_t)t * C];
    const float mean = col_reduce_sum(a, red, tg, cl) / (float)len;
    float q = 0.f;
    for (int t = tg; t < len; t += 4) {
        const float d = xc[(int64_t)t * C] - mean;
        q += d * d;
    }
    const float var = col_reduce_sum(q, red, tg, cl) / (float)len;
    if (ok && tg == 0) {
        gstats[(int64_t)n * 2 * C + c] = mean;
        gstats[(int64_t)n * 2 * C + C + c] = sqrtf(fmaxf(var, EC_EPS));
    }
}

// out[n][j] = W[j][k0 .. k0 + K) . v[n] + bias[j]; one wave per (item, j)
__global__ __launch_bounds__(256) void ecapa_item_bias_kernel(const __half* __restrict__ W, int64_t ldw, int k0, const float* __restrict__ bias,
                                                              const float* __restrict__ v, int K, int N, float* __restrict__ out) {
    const int n = blockIdx.y, j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= N) return;
    const __half* w = W + (int64_t)j * ldw + k0;
    const float* vn = v + (int64_t)n * K;
    float a = 0.f;
    for (int k = lane; k < K; k += 64) a += __half2float(w[k]) * vn[k];
    a = wave_sum(a);
    if (lane == 0) out[(int64_t)n * N + j] = a + bias[j];
}

// pooled[n][c] = sum_t a_t x_t, pooled[n][C + c] = sqrt(max(sum_t a_t (x_t - mean)^2, 1e-12)), a = softmax over t < len of the logits
__global__ __launch_bounds__(256) void ecapa_pool_kernel(const float* __restrict__ x, const float* __restrict__ logits, int T, int C,
                                                         const int* __restrict__ lens, float* __restrict__ pooled) {
    __shared__ float red[256];
    const int n = blockIdx.y, cl = threadIdx.x & 63, tg = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const bool ok = c < C;
    const int len = lens ? lens[n] : T;
    const int64_t base = (int64_t)n * T * C + (ok ? c : 0);
    const float* xc = x + base;
    const float* lc = logits + base;
    float mx = -INFINITY;
    for (int t = tg; t < len; t += 4) mx = fmaxf(mx, lc[(int64_t)t * C]);
    mx = col_reduce_max(mx, red, tg, cl);
    float se = 0.f, sx = 0.f;
    for (int t = tg; t < len; t += 4) {
        const float e = expf(lc[(int64_t)t * C] - mx);
        se += e;
        sx += e * xc[(int64_t)t * C];
    }
    se = col_reduce_sum(se, red, tg, cl);
    const float mean = col_reduce_sum(sx, red, tg, cl) / se;
    float q = 0.f;
    for (int t = tg; t < len; t += 4) {
        const float d = xc[(int64_t)t * C] - mean;
        q += expf(lc[(int64_t)t * C] - mx) * (d * d);
    }
    const float var = col_reduce_sum(q, red, tg, cl) / se;
    if (ok && tg == 0) {
        pooled[(int64_t)n * 2 * C + c] = mean;
        pooled[(int64_t)n * 2 * C + C + c] = sqrtf(fmaxf(var, EC_EPS));
    }
}

__device__ __forceinline__ float block_sum_1024(float v, float* red, int tid) {
    v = wave_sum(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) a += red[i];
    return a;
}

// out[n] = normalize(W . LayerNorm(pooled[n]) + b); one workgroup per item; LDS: C2 + E floats
__global__ __launch_bounds__(1024) void ecapa_tail_kernel(const float* __restrict__ pooled, int C2, const float* __restrict__ g, const float* __restrict__ b,
                                                          const __half* __restrict__ W, int64_t ldw, const float* __restrict__ bias, int E,
                                                          float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ec_smem[];
    __shared__ float red[16];
    float* ln = reinterpret_cast<float*>(ec_smem);  // [C2]
    float* ov = ln + C2;                            // [E]
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* pn = pooled + (int64_t)n * C2;
    float a = 0.f;
    for (int c = tid; c < C2; c += 1024) a += pn[c];
    const float mean = block_sum_1024(a, red, tid) / (float)C2;
    float q = 0.f;
    for (int c = tid; c < C2; c += 1024) {
        const float d = pn[c] - mean;
        q += d * d;
    }
    const float inv = 1.0f / sqrtf(block_sum_1024(q, red, tid) / (float)C2 + EC_EPS);
    for (int c = tid; c < C2; c += 1024) ln[c] = (pn[c] - mean) * inv * g[c] + b[c];
    __syncthreads();
    for (int o = wave; o < E; o += 16) {
        const __half* w = W + (int64_t)o * ldw;
        float d = 0.f;
        for (int c = lane; c < C2; c += 64) d += __half2float(w[c]) * ln[c];
        d = wave_sum(d);
        if (lane == 0) ov[o] = d + bias[o];
    }
    __syncthreads();
    float s2 = 0.f;
    for (int o = tid; o < E; o += 1024) s2 += ov[o] * ov[o];
    const float norm = fmaxf(sqrtf(block_sum_1024(s2, red, tid)), EC_EPS);
    for (int o = tid; o < E; o += 1024) out[(int64_t)n * E + o] = ov[o] / norm;
}

__global__ __launch_bounds__(256) void ecapa_gcmvn_kernel(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ stdv,
                                                          const int* __restrict__ lens, int T, int D, int64_t total, float* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t row = i / D;
    const int d = (int)(i - row * D);
    const int n = (int)(row / T), t = (int)(row - (int64_t)n * T);
    y[i] = (!lens || t < lens[n]) ? (x[i] - mean[d]) / stdv[d] : 0.f;
}

template <int CW>
void launch_chain_cfg(const EcapaChainArgs& a, hipStream_t s) {
    constexpr size_t LDS = ((size_t)2 * (EC_ROWS + 2 * EC_G) * (CW + 8) + (size_t)CW * (3 * CW + 8)) * sizeof(_Float16);
    static_assert(LDS <= 160 * 1024, "planes + one stage's weights must fit in the CU's LDS");
    static bool attr_set = false;
    if (!attr_set) {
        SC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&ecapa_chain_kernel<CW>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS));
        attr_set = true;
    }
    const int tiles = cdiv(a.T, ecapa_chain_tile_rows(a.scale, a.dil));
    const double rows = (double)a.nb * a.T;
    prof::Scope scope(CW == 64 ? "ecapa_chain_c64" : "ecapa_chain_c32", 2.0 * rows * (a.scale - 1) * 3.0 * CW * CW,
                      4.0 * rows * a.scale * CW * 2.0 + 2.0 * (a.scale - 1) * 3.0 * CW * CW, s);
    hipLaunchKernelGGL((ecapa_chain_kernel<CW>), dim3((unsigned)(a.nb * tiles)), dim3(EC_THREADS), LDS, s, a, tiles);
}

}  // namespace

bool ecapa_chain_supported(int chunk, int scale, int k, int dil) {
    return (chunk == 32 || chunk == 64) && k == 3 && scale >= 2 && scale <= ECAPA_MAX_SCALE && dil >= 1 && dil <= EC_G &&
           EC_ROWS - 2 * (scale - 1) * dil >= 32;
}

int ecapa_chain_tile_rows(int scale, int dil) { return EC_ROWS - 2 * (scale - 1) * dil; }

void launch_ecapa_chain(const EcapaChainArgs& a, hipStream_t s) {
    SC_CHECK(ecapa_chain_supported(a.CW, a.scale, 3, a.dil), "ecapa chain: unsupported chunk width %d (32 or 64), scale %d or dilation %d (1..%d)", a.CW,
             a.scale, a.dil, EC_G);
    SC_CHECK(a.nb > 0 && a.T > 0 && a.x && a.out && a.x != a.out, "ecapa chain: empty problem or in-place call");
    SC_CHECK(a.ldx % 4 == 0 && a.ldo % 4 == 0 && a.ldx >= a.scale * a.CW && a.ldo >= a.scale * a.CW && a.ldw % 8 == 0 && a.ldw >= 3 * a.CW,
             "ecapa chain: row strides (x %lld, out %lld, w %lld) too short or misaligned", (long long)a.ldx, (long long)a.ldo, (long long)a.ldw);
    SC_CHECK(((reinterpret_cast<uintptr_t>(a.x) | reinterpret_cast<uintptr_t>(a.out)) & 15) == 0, "ecapa chain: x / out must be 16-byte aligned");
    for (int i = 0; i + 1 < a.scale; ++i) SC_CHECK(a.w[i] && a.bias[i] && a.gamma[i] && a.beta[i], "ecapa chain: stage %d has no weights", i);
    SC_CHECK((int64_t)a.nb * cdiv(a.T, ecapa_chain_tile_rows(a.scale, a.dil)) < (1ll << 31), "ecapa chain: grid too large");
    if (a.CW == 64) launch_chain_cfg<64>(a, s);
    else launch_chain_cfg<32>(a, s);
    SC_LAUNCH_CHECK();
}

void launch_ecapa_relu_ln(const float* x, int64_t ldx, const float* item_bias, int t_per_item, const float* g, const float* b, float* y, int64_t ldy,
                          int rows, int C, int act, hipStream_t s) {
    SC_CHECK(rows > 0 && C > 0 && (act == ACT_NONE || act == ACT_TANH) && (!item_bias || t_per_item > 0), "ecapa relu_ln: bad argument");
    prof::Scope scope("ecapa_relu_ln", 8.0 * rows * C, 8.0 * rows * C, s);
    hipLaunchKernelGGL(ecapa_relu_ln_kernel, dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, s, x, ldx, item_bias, t_per_item, g, b, y, ldy, rows, C, act);
    SC_LAUNCH_CHECK();
}

void launch_ecapa_se_gate(const float* x, int64_t ldx, int nb, int T, const int* d_lens, int C, int S, const __half* w1, const float* b1,
                          const __half* w2, const float* b2, float* gate, hipStream_t s) {
    SC_CHECK(nb > 0 && T > 0 && C > 0 && C % 4 == 0 && C <= 4096 && S > 0 && S <= 1024 && ldx % 4 == 0, "ecapa se gate: C=%d (multiple of 4, <= 4096) S=%d (<= 1024)",
             C, S);
    prof::Scope scope("ecapa_se_gate", 2.0 * nb * ((double)T * C + 2.0 * C * S), 4.0 * nb * (double)T * C, s);
    hipLaunchKernelGGL(ecapa_se_gate_kernel, dim3((unsigned)nb), dim3(1024), (size_t)(4096 + C + S) * 4, s, x, ldx, T, d_lens, C, S, w1, b1, w2, b2, gate);
    SC_LAUNCH_CHECK();
}

void launch_ecapa_se_apply(const float* y, int64_t ldy, const float* gate, const float* res, int64_t ldr, float* out, int64_t ldo, int nb, int T, int C,
                           hipStream_t s) {
    SC_CHECK(C % 4 == 0 && ldy % 4 == 0 && ldr % 4 == 0 && ldo % 4 == 0 && nb > 0 && T > 0, "ecapa se apply: C and the row strides must be multiples of 4");
    const int64_t total4 = (int64_t)nb * T * (C / 4);
    SC_CHECK(cdiv64(total4, 256) < (1ll << 31), "ecapa se apply: grid too large");
    prof::Scope scope("ecapa_se_apply", 2.0 * total4 * 4, 12.0 * total4 * 4, s);
    hipLaunchKernelGGL(ecapa_se_apply_kernel, dim3((unsigned)cdiv64(total4, 256)), dim3(256), 0, s, y, ldy, gate, res, ldr, out, ldo, T, C, total4);
    SC_LAUNCH_CHECK();
}

void launch_ecapa_gstats(const float* x, int nb, int T, int C, const int* d_lens, float* gstats, hipStream_t s) {
    SC_CHECK(nb > 0 && nb < 65536 && T > 0 && C > 0, "ecapa gstats: bad geometry");
    prof::Scope scope("ecapa_gstats", 4.0 * nb * (double)T * C, 8.0 * nb * (double)T * C, s);
    hipLaunchKernelGGL(ecapa_gstats_kernel, dim3((unsigned)cdiv(C, 64), (unsigned)nb), dim3(256), 0, s, x, T, C, d_lens, gstats);
    SC_LAUNCH_CHECK();
}

void launch_ecapa_item_bias(const __half* W, int64_t ldw, int k0, const float* bias, const float* v, int nb, int K, int N, float* out, hipStream_t s) {
    SC_CHECK(nb > 0 && nb < 65536 && K > 0 && N > 0 && k0 >= 0 && k0 + K <= ldw, "ecapa item bias: bad geometry");
    prof::Scope scope("ecapa_item_bias", 2.0 * nb * (double)K * N, 2.0 * (double)K * N, s);
    hipLaunchKernelGGL(ecapa_item_bias_kernel, dim3((unsigned)cdiv(N, 4), (unsigned)nb), dim3(256), 0, s, W, ldw, k0, bias, v, K, N, out);
    SC_LAUNCH_CHECK();
}

void launch_ecapa_pool(const float* x, const float* logits, int nb, int T, int C, const int* d_lens, float* pooled, hipStream_t s) {
    SC_CHECK(nb > 0 && nb < 65536 && T > 0 && C > 0, "ecapa pool: bad geometry");
    prof::Scope scope("ecapa_pool", 10.0 * nb * (double)T * C, 20.0 * nb * (double)T * C, s);
    hipLaunchKernelGGL(ecapa_pool_kernel, dim3((unsigned)cdiv(C, 64), (unsigned)nb), dim3(256), 0, s, x, logits, T, C, d_lens, pooled);
    SC_LAUNCH_CHECK();
}

void launch_ecapa_tail(const float* pooled, int nb, int C2, const float* g, const float* b, const __half* W, int64_t ldw, const float* bias, int E,
                       float* out, hipStream_t s) {
    SC_CHECK(nb > 0 && C2 > 0 && E > 0 && (size_t)(C2 + E) * 4 <= 60 * 1024 && ldw >= C2, "ecapa tail: %d + %d values do not fit in LDS", C2, E);
    prof::Scope scope("ecapa_tail", 2.0 * nb * (double)C2 * E, 2.0 * nb * (double)C2 * E, s);
    hipLaunchKernelGGL(ecapa_tail_kernel, dim3((unsigned)nb), dim3(1024), (size_t)(C2 + E) * 4, s, pooled, C2, g, b, W, ldw, bias, E, out);
    SC_LAUNCH_CHECK();
}

void launch_ecapa_gcmvn(const float* x, const float* mean, const float* stdv, const int* d_lens, int nb, int T, int D, float* y, hipStream_t s) {
    const int64_t total = (int64_t)nb * T * D;
    SC_CHECK(total > 0 && cdiv64(total, 256) < (1ll << 31), "ecapa gcmvn: bad geometry");
    prof::Scope scope("ecapa_gcmvn", 2.0 * total, 8.0 * total, s);
    hipLaunchKernelGGL(ecapa_gcmvn_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, s, x, mean, stdv, d_lens, T, D, total, y);
    SC_LAUNCH_CHECK();
}

}  // namespace sc
