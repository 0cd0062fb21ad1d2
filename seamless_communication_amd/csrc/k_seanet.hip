// Kernels of the PRETSSEL waveform generator's SEANet half (reference models/generator/streamable.py, vocoder.py:556-572):
// the 2-layer LSTM step, the fused ELU residual block, the "streamable" strided / transposed convolutions and the tail.
//
// Activations are fp32 rows [time][C]; the items of a call lie back to back and every kernel takes the items' first rows from
// a small table ([n + 1] ints on the device), one table per length the layer sees.  Every output element is computed by one
// thread (convolutions) or one wave (LSTM) in a fixed order from its own item's rows only, tiles are counted from the item's
// first row: an item's bits do not depend on its companions.  Weights are fp16, accumulation and state fp32.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "device_util.h"

namespace sc {

namespace {

__device__ __forceinline__ float elu1(float v) { return v > 0.f ? v : expm1f(v); }
__device__ __forceinline__ float sigmoid1(float v) { return 1.f / (1.f + expf(-v)); }
__device__ __forceinline__ float in_act1(float v, int act) { return act == SEANET_IN_ELU ? elu1(v) : act == SEANET_IN_TANH ? tanhf(v) : v; }

// ---- LSTM ------------------------------------------------------------------------------------------------------------------
// One launch per time step t = 0 .. max steps: layer 0 at t, layer 1 at t - 1 (both read what the launch before wrote).
// grid (2 * H / 4, n): blockIdx.x < H / 4 is layer 0.  A wave owns one hidden unit of one item: its four gate rows (i, f, g,
// o) are reduced over K in lane order, then lane 0 updates the cell.  Items whose steps are done leave at once.
constexpr int LSTM_WAVES = 4;

__global__ __launch_bounds__(LSTM_WAVES * 64) void lstm2_step_kernel(LstmStepArgs a, int t) {
    const int H = a.H, item = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int units_blocks = H / LSTM_WAVES;
    const int layer = blockIdx.x >= units_blocks ? 1 : 0;
    const int j = (blockIdx.x - layer * units_blocks) * LSTM_WAVES + wave;
    const int row0 = a.row_off[item], steps = a.row_off[item + 1] - row0;
    const int s = t - layer;  // the step this layer computes
    if (s < 0 || s >= steps) return;
    const int64_t row = row0 + s;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    // operand: layer 0 h0[s - 1] (K = H); layer 1 [h0[s] ; h1[s - 1]] (K = 2H).  A missing previous step is zero.
    const int K = layer ? 2 * H : H;
    const __half* W = layer ? a.w1 : a.whh0;
    for (int k = lane * 8; k < K; k += 64 * 8) {
        const float* src;
        if (layer == 0) src = s > 0 ? a.h0 + (row - 1) * H + k : nullptr;
        else src = k < H ? a.h0 + row * H + k : (s > 0 ? a.h1 + (row - 1) * H + (k - H) : nullptr);
        if (!src) continue;
        const float4 v0 = *reinterpret_cast<const float4*>(src), v1 = *reinterpret_cast<const float4*>(src + 4);
        const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const uint4 wq = *reinterpret_cast<const uint4*>(W + (int64_t)(g * H + j) * K + k);
            const __half2* wh = reinterpret_cast<const __half2*>(&wq);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float2 wf = __half22float2(wh[q]);
                acc[g] = fmaf(wf.x, v[2 * q], acc[g]);
                acc[g] = fmaf(wf.y, v[2 * q + 1], acc[g]);
            }
        }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = wave_sum(acc[g]);
    if (lane != 0) return;
    const float* bi = layer ? a.b_ih1 : a.b_ih0;
    const float* bh = layer ? a.b_hh1 : a.b_hh0;
    float pre[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        pre[g] = acc[g] + bi[g * H + j] + bh[g * H + j];
        if (layer == 0) pre[g] += a.xproj[row * 4 * H + g * H + j];
    }
    float* cst = (layer ? a.c1 : a.c0) + (int64_t)item * H + j;
    const float c = sigmoid1(pre[1]) * *cst + sigmoid1(pre[0]) * tanhf(pre[2]);
    const float h = sigmoid1(pre[3]) * tanhf(c);
    *cst = c;
    if (layer == 0) {
        a.h0[row * H + j] = h;
    } else {
        a.h1[row * H + j] = h;
        a.y[row * H + j] = h + a.x[row * H + j];
    }
    if (a.max_pre) {  // largest gate pre-activation seen (tests and the liveness conditions of the synthetic weights)
        float m = 0.f;
#pragma unroll
        for (int g = 0; g < 4; ++g) m = fmaxf(m, fabsf(pre[g]));
        atomicMax(reinterpret_cast<int*>(a.max_pre), __float_as_int(m));  // non-negative floats order like ints
    }
}

// ---- fused residual block: y = x + conv_k1(ELU(conv_k3(ELU(x)))) at C in {32, 64}, hidden C / 2 ---------------------------
// One workgroup per tile of SEANET_RES_TILE rows of one item.  LDS: ELU(x) on tile + 2 rows, the hidden rows, both weight
// matrices transposed (adjacent threads = adjacent output channels read adjacent words, the activation is a broadcast).
// y must not alias x: a tile reads the rows of x next to it, which another workgroup would be overwriting.
__global__ __launch_bounds__(256) void seanet_resblock_kernel(SeanetResArgs a) {
    extern __shared__ __align__(16) float lds[];
    const int C = a.C, Hd = C / 2, item = blockIdx.y, tid = threadIdx.x;
    const int row0 = a.row_off[item], len = a.row_off[item + 1] - row0;
    const int t0 = blockIdx.x * SEANET_RES_TILE;
    if (t0 >= len) return;
    float* xs = lds;                                  // [TILE + 2][C]   ELU(x), rows t0 - 1 ..
    float* hs = xs + (SEANET_RES_TILE + 2) * C;       // [TILE][Hd]      ELU(hidden)
    float* w1 = hs + SEANET_RES_TILE * Hd;            // [3 * C][Hd]
    float* w2 = w1 + 3 * C * Hd;                      // [Hd][C]
    for (int i = tid; i < (SEANET_RES_TILE + 2) * C; i += 256) {
        const int t = t0 - 1 + i / C;
        xs[i] = (t >= 0 && t < len) ? elu1(a.x[(int64_t)(row0 + t) * C + i % C]) : 0.f;
    }
    for (int i = tid; i < 3 * C * Hd; i += 256) w1[i] = __half2float(a.w1[(int64_t)(i % Hd) * 3 * C + i / Hd]);
    for (int i = tid; i < Hd * C; i += 256) w2[i] = __half2float(a.w2[(int64_t)(i % C) * Hd + i / C]);
    __syncthreads();
    {
        const int h = tid % Hd;
        const float b = a.b1[h];
        for (int r = tid / Hd; r < SEANET_RES_TILE; r += 256 / Hd) {
            float acc = 0.f;
            const float* xr = xs + r * C;  // the window of row r: rows r .. r + 2 of xs, contiguous
            for (int kk = 0; kk < 3 * C; ++kk) acc = fmaf(w1[kk * Hd + h], xr[kk], acc);
            hs[r * Hd + h] = elu1(acc + b);
        }
    }
    __syncthreads();
    {
        const int c = tid % C;
        const float b = a.b2[c];
        for (int r = tid / C; r < SEANET_RES_TILE; r += 256 / C) {
            if (t0 + r >= len) break;
            float acc = 0.f;
            for (int h = 0; h < Hd; ++h) acc = fmaf(w2[h * C + c], hs[r * Hd + h], acc);
            const int64_t o = (int64_t)(row0 + t0 + r) * C + c;
            a.y[o] = a.x[o] + (acc + b);
        }
    }
}

// ---- streamable convolution (direct): stride r, kernel k, zero padding `left` in front and whatever the last window needs ----
// grid (tiles of SCONV_ROWS output rows, cout / 64, n), block (64, SCONV_ROWS): a wave per output row, a lane per output
// channel.  The activated input window of the tile lies in LDS; the weights are [k * cin][cout], so a wave reads them coalesced.
constexpr int SCONV_ROWS = 4;
// input rows SCONV_ROWS consecutive outputs of the transposed convolution can read: (p0 + left) / r - 1 .. (p0 + left + 3) / r
constexpr int SCONVTR_IN_ROWS = SCONV_ROWS + 1;

__global__ __launch_bounds__(64 * SCONV_ROWS) void sconv_kernel(SconvArgs a) {
    extern __shared__ __align__(16) float lds[];
    const int item = blockIdx.z, cin = a.cin;
    const int in0 = a.in_off[item], in_len = a.in_off[item + 1] - in0;
    const int out0 = a.out_off[item], out_len = a.out_off[item + 1] - out0;
    const int q0 = blockIdx.x * SCONV_ROWS;
    if (q0 >= out_len) return;
    const int win_rows = (SCONV_ROWS - 1) * a.stride + a.k;
    const int tfirst = q0 * a.stride - a.left;
    const int tid = threadIdx.y * 64 + threadIdx.x;
    for (int i = tid; i < win_rows * cin; i += 64 * SCONV_ROWS) {
        const int t = tfirst + i / cin;
        lds[i] = (t >= 0 && t < in_len) ? in_act1(a.x[(int64_t)(in0 + t) * cin + i % cin], a.in_act) : 0.f;
    }
    __syncthreads();
    const int co = blockIdx.y * 64 + threadIdx.x, q = q0 + threadIdx.y;
    if (co >= a.cout || q >= out_len) return;
    const float* win = lds + threadIdx.y * a.stride * cin;
    const __half* w = a.wt + co;
    // eight partial sums in a fixed order: shorter dependency chains, and a rounding error that grows with K / 8
    float part[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int K = a.k * cin;
    int kk = 0;
    for (; kk + 8 <= K; kk += 8) {
#pragma unroll
        for (int u = 0; u < 8; ++u) part[u] = fmaf(__half2float(w[(int64_t)(kk + u) * a.cout]), win[kk + u], part[u]);
    }
    for (; kk < K; ++kk) part[kk & 7] = fmaf(__half2float(w[(int64_t)kk * a.cout]), win[kk], part[kk & 7]);
    float acc = ((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7]));
    const int64_t o = (int64_t)(out0 + q) * a.cout + co;
    acc += a.bias[co];
    a.y[o] = a.res ? a.res[o] + acc : acc;
}

// ---- transposed streamable convolution, k = 2 * stride: output p takes the taps (p + trim) % r and that + r ----------------
__global__ __launch_bounds__(64 * SCONV_ROWS) void sconvtr_kernel(SconvArgs a) {
    extern __shared__ __align__(16) float lds[];  // the activated input rows the tile's outputs read: at most SCONVTR_IN_ROWS
    const int item = blockIdx.z, cin = a.cin, r = a.stride;
    const int in0 = a.in_off[item], in_len = a.in_off[item + 1] - in0;
    const int out0 = a.out_off[item], out_len = a.out_off[item + 1] - out0;
    const int p0 = blockIdx.x * SCONV_ROWS;
    if (p0 >= out_len) return;
    const int ifirst = (p0 + a.left) / r - 1;  // the oldest input row any output of the tile reads
    const int tid = threadIdx.y * 64 + threadIdx.x;
    for (int i = tid; i < SCONVTR_IN_ROWS * cin; i += 64 * SCONV_ROWS) {
        const int t = ifirst + i / cin;
        lds[i] = (t >= 0 && t < in_len) ? in_act1(a.x[(int64_t)(in0 + t) * cin + i % cin], a.in_act) : 0.f;
    }
    __syncthreads();
    const int p = p0 + threadIdx.y, co = blockIdx.y * 64 + threadIdx.x;
    if (p >= out_len || co >= a.cout) return;
    const int j = p + a.left;  // position in the untrimmed output
    float acc = 0.f;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int i = j / r - u, tap = j % r + u * r;
        if (i < 0 || i >= in_len) continue;
        const float* xr = lds + (i - ifirst) * cin;
        const __half* w = a.wt + (int64_t)tap * cin * a.cout + co;
        float part[4] = {0.f, 0.f, 0.f, 0.f};
        int c = 0;
        for (; c + 4 <= cin; c += 4) {
#pragma unroll
            for (int v = 0; v < 4; ++v) part[v] = fmaf(__half2float(w[(int64_t)(c + v) * a.cout]), xr[c + v], part[v]);
        }
        for (; c < cin; ++c) part[c & 3] = fmaf(__half2float(w[(int64_t)c * a.cout]), xr[c], part[c & 3]);
        acc += (part[0] + part[1]) + (part[2] + part[3]);
    }
    a.y[(int64_t)(out0 + p) * a.cout + co] = acc + a.bias[co];
}

// ---- tail: wav[t] = 0.8 * (conv_k(ELU(h)))[t] + tanh(skip[t]) for t < L, h given on the decoder's rounded-up length ----------
__global__ __launch_bounds__(256) void seanet_tail_kernel(SeanetTailArgs a) {
    extern __shared__ __align__(16) float lds[];  // [k * cin] weights, then ELU(h) on the tile's 256 + k - 1 rows, row stride cin + 1
    const int item = blockIdx.y, cin = a.cin, K = a.k * cin, ld = cin + 1;  // the odd stride keeps a wave's rows off one bank
    float* hs = lds + K;
    const int in0 = a.in_off[item], in_len = a.in_off[item + 1] - in0;
    const int out0 = a.out_off[item], out_len = a.out_off[item + 1] - out0;
    const int t0 = blockIdx.x * 256;
    if (t0 >= out_len) return;
    const int left = (a.k - 1) - (a.k - 1) / 2;
    for (int i = threadIdx.x; i < K; i += 256) lds[i] = __half2float(a.w[i]);
    for (int i = threadIdx.x; i < (256 + a.k - 1) * cin; i += 256) {
        const int ti = t0 - left + i / cin;
        hs[(i / cin) * ld + i % cin] = (ti >= 0 && ti < in_len) ? elu1(a.h[(int64_t)(in0 + ti) * cin + i % cin]) : 0.f;
    }
    __syncthreads();
    const int t = t0 + threadIdx.x;
    if (t >= out_len) return;
    float acc = 0.f;
    for (int tap = 0; tap < a.k; ++tap) {
        const float* hr = hs + (threadIdx.x + tap) * ld;
        for (int c = 0; c < cin; ++c) acc = fmaf(lds[tap * cin + c], hr[c], acc);
    }
    const float v = 0.8f * (acc + a.bias[0]) + tanhf(a.skip[out0 + t]);
    if (a.wav_stride) a.wav[(int64_t)item * a.wav_stride + t] = v;
    else a.wav[out0 + t] = v;
}

// mel rows [n][t_cap][dim] -> packed (x - mean) / scale rows [off[n]][dim]
__global__ __launch_bounds__(256) void mel_norm_pack_kernel(const float* __restrict__ mel, const float* __restrict__ mean, const float* __restrict__ scale,
                                                            const int* __restrict__ off, int t_cap, int dim, float* __restrict__ out) {
    const int item = blockIdx.y, row0 = off[item], len = off[item + 1] - row0;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)len * dim) return;
    const int d = i % dim;
    out[(int64_t)row0 * dim + i] = (mel[(int64_t)item * t_cap * dim + i] - mean[d]) / scale[d];
}

// weights [d0][d1][k] (Conv1d: d0 = cout, d1 = cin; ConvTranspose1d: d0 = cin, d1 = cout) -> [k * cin][cout] fp16
__global__ void pack_sconv_weight_kernel(const float* __restrict__ w, __half* __restrict__ dst, int cin, int cout, int k, int transposed) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)k * cin * cout) return;
    const int co = i % cout, c = (i / cout) % cin, tap = i / ((int64_t)cout * cin);
    const int64_t src = transposed ? ((int64_t)c * cout + co) * k + tap : ((int64_t)co * cin + c) * k + tap;
    dst[i] = __float2half(w[src]);
}

}  // namespace

bool lstm2_supported(int H) { return H >= 32 && H % 32 == 0 && H <= 2048; }

void launch_lstm2_step(const LstmStepArgs& a, int n, int t, hipStream_t s) {
    SC_CHECK(lstm2_supported(a.H) && n >= 1 && n <= 65535 && t >= 0, "launch_lstm2_step: H=%d n=%d t=%d", a.H, n, t);
    hipLaunchKernelGGL(lstm2_step_kernel, dim3(2 * a.H / LSTM_WAVES, n), dim3(LSTM_WAVES * 64), 0, s, a, t);
    SC_LAUNCH_CHECK();
}

bool seanet_resblock_supported(int C) { return C == 32 || C == 64; }

void launch_seanet_resblock(const SeanetResArgs& a, hipStream_t s) {
    SC_CHECK(seanet_resblock_supported(a.C) && a.n >= 1 && a.n <= 65535 && a.longest >= 1, "launch_seanet_resblock: C=%d n=%d longest=%d", a.C, a.n, a.longest);
    SC_CHECK(a.x != a.y, "launch_seanet_resblock: y must not alias x (a tile reads its neighbours' rows of x)");
    const int C = a.C, Hd = C / 2;
    const size_t bytes = ((size_t)(SEANET_RES_TILE + 2) * C + (size_t)SEANET_RES_TILE * Hd + (size_t)3 * C * Hd + (size_t)Hd * C) * 4;
    hipLaunchKernelGGL(seanet_resblock_kernel, dim3(cdiv(a.longest, SEANET_RES_TILE), a.n), dim3(256), bytes, s, a);
    SC_LAUNCH_CHECK();
}

bool sconv_supported(int cin, int cout, int k, int stride) {
    if (cin < 1 || cout < 1 || k < 1 || stride < 1 || k < stride || cout > 65535 * 64) return false;
    return ((size_t)(SCONV_ROWS - 1) * stride + k) * cin * 4 <= 48 * 1024;
}

void launch_sconv(const SconvArgs& a, hipStream_t s) {
    SC_CHECK(sconv_supported(a.cin, a.cout, a.k, a.stride) && a.left >= 0 && a.left <= a.k - a.stride && a.n >= 1 && a.n <= 65535 && a.longest_out >= 1,
             "launch_sconv: cin=%d cout=%d k=%d stride=%d left=%d n=%d", a.cin, a.cout, a.k, a.stride, a.left, a.n);
    const size_t bytes = ((size_t)(SCONV_ROWS - 1) * a.stride + a.k) * a.cin * 4;
    hipLaunchKernelGGL(sconv_kernel, dim3(cdiv(a.longest_out, SCONV_ROWS), cdiv(a.cout, 64), a.n), dim3(64, SCONV_ROWS), bytes, s, a);
    SC_LAUNCH_CHECK();
}

void launch_sconvtr(const SconvArgs& a, hipStream_t s) {
    SC_CHECK(a.cin >= 1 && a.cout >= 1 && a.stride >= 1 && a.k == 2 * a.stride && a.left >= 0 && a.left <= a.stride && a.res == nullptr && a.n >= 1 &&
                 a.n <= 65535 && a.longest_out >= 1,
             "launch_sconvtr: cin=%d cout=%d k=%d stride=%d left=%d n=%d", a.cin, a.cout, a.k, a.stride, a.left, a.n);
    SC_CHECK((size_t)SCONVTR_IN_ROWS * a.cin * 4 <= 48 * 1024, "launch_sconvtr: cin=%d", a.cin);
    hipLaunchKernelGGL(sconvtr_kernel, dim3(cdiv(a.longest_out, SCONV_ROWS), cdiv(a.cout, 64), a.n), dim3(64, SCONV_ROWS), (size_t)SCONVTR_IN_ROWS * a.cin * 4, s, a);
    SC_LAUNCH_CHECK();
}

void launch_seanet_tail(const SeanetTailArgs& a, hipStream_t s) {
    const size_t bytes = ((size_t)a.k * a.cin + (size_t)(256 + a.k - 1) * (a.cin + 1)) * 4;
    SC_CHECK(a.cin >= 1 && a.k >= 1 && bytes <= 48 * 1024 && a.n >= 1 && a.n <= 65535 && a.longest_out >= 1, "launch_seanet_tail: cin=%d k=%d n=%d", a.cin, a.k,
             a.n);
    hipLaunchKernelGGL(seanet_tail_kernel, dim3(cdiv(a.longest_out, 256), a.n), dim3(256), bytes, s, a);
    SC_LAUNCH_CHECK();
}

bool seanet_tail_supported(int cin, int k) {
    return cin >= 1 && k >= 1 && k % 2 == 1 && ((size_t)k * cin + (size_t)(256 + k - 1) * (cin + 1)) * 4 <= 48 * 1024;
}

void launch_mel_norm_pack(const float* mel, const float* mean, const float* scale, const int* off, int n, int longest, int t_cap, int dim, float* out,
                          hipStream_t s) {
    SC_CHECK(n >= 1 && n <= 65535 && longest >= 1 && longest <= t_cap && dim >= 1, "launch_mel_norm_pack: n=%d longest=%d t_cap=%d dim=%d", n, longest, t_cap, dim);
    hipLaunchKernelGGL(mel_norm_pack_kernel, dim3((unsigned)cdiv64((int64_t)longest * dim, 256), n), dim3(256), 0, s, mel, mean, scale, off, t_cap, dim, out);
    SC_LAUNCH_CHECK();
}

void launch_pack_sconv_weight(const float* w, __half* dst, int cin, int cout, int k, bool transposed, hipStream_t s) {
    const int64_t total = (int64_t)k * cin * cout;
    SC_CHECK(total >= 1 && total < (1ll << 31), "launch_pack_sconv_weight: %lld elements", (long long)total);
    hipLaunchKernelGGL(pack_sconv_weight_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, s, w, dst, cin, cout, k, transposed ? 1 : 0);
    SC_LAUNCH_CHECK();
}

}  // namespace sc
