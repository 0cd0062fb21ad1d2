// Time-scale modification of finished waveforms: a waveform-similarity overlap-add (WSOLA) that turns a row
// of L samples into Lo samples at the same pitch.  An extension of this project; the reference has no counterpart.
// sc_time_stretch, sc_op_tsm_centres.
//
// N = frame (even, 64..2048), Hs = N / 2, D = radius (0..Hs); x[0, L) the item, +0 outside; Lo the wanted length.
//
// ---- 1. Peak (tsm_peak_kernel) ---------------------------------------------------------------------------------------------------
// peak = max |x[i]| over the finite samples, as the unsigned maximum of their bit patterns without the sign (exact, any order).
// No finite sample, or peak < 2^-100: q == 0.  Otherwise e = floor(log2 peak) is the peak's exponent field and
//     q[i] = clamp(rintf(x[i] * 2^(14 - e)), -32767, 32767)     (the product by a power of two is exact; ties to even)
// with q[i] = 0 for a sample that is not finite and outside [0, L).  q is used by the search only.
//
// ---- 2. Search (tsm_search_kernel) -----------------------------------------------------------------------------------------------
// M = ceil(Lo / Hs) + 1 frames; frame m has the centre c_m and reads x[c_m - Hs, c_m + Hs).
//     a_m = floor(m * Hs * L / Lo)                                    (int64; below 2^63 for L <= 2^30, Lo <= 4 L)
//     c_0 = 0;  c_m = a_m + d_m  (m >= 1)
//     d_m = the d in [-D, D] with the smallest SAD(d) = sum_{k < N} | q[c_{m-1} + k] - q[a_m + d - Hs + k] |      (int32: < 2^31)
//           ties: the smallest |d|, then the negative one
// The first term is the natural continuation of frame m - 1 (centre c_{m-1} + Hs).  Integers only: no order of summation and no
// rounding can change a result.  Lo == L gives d == 0 (SAD(0) = 0) and q == 0 gives d == 0 (every SAD is 0): both are written
// without the walk, c_m = a_m.
// One workgroup per item walks its frames; the items of a call run side by side.  Per frame: the template q[c_{m-1} + k] (N
// samples) and the region q[a_m - D - Hs + j] (N + 2 D samples) are quantised into LDS as int16 (at most 4 + 8 KB); barrier; lane
// j takes the lags j, j + threads, ... and sums its N differences (the template is a broadcast read, the region a read of
// consecutive int16 over the lanes); the key SAD << 12 | |d| << 1 | (d > 0) is reduced to its minimum with an xor butterfly over
// the wavefront and one LDS exchange between the waves; barrier; every thread holds c_m.  The workgroup has one lane per lag where
// 1024 threads allow it (2 D + 1 rounded up to whole waves).
//
// ---- 3. Overlap-add (tsm_ola_kernel) ---------------------------------------------------------------------------------------------
// w[k] = (float)(0.5 - 0.5 cos(2 pi k / N)), k < N: built on the host in double, rounded to fp32 once.  For t in [0, Lo), m = t / Hs,
// k = t - m * Hs, every operation a single correctly rounded fp32 one (no contraction):
//     y[t] = (w[k + Hs] * x[c_m + k]) + (w[k] * x[c_{m+1} - Hs + k])
// Lo == L: y[t] = x[t], the bits.  One thread per output sample of every item, 256 per workgroup; nothing is written behind Lo.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <list>
#include <mutex>
#include <vector>

#include "handle.h"

namespace sc {

static constexpr int TSM_THREADS = 256;  // peak and overlap-add
static constexpr int TSM_MIN_FRAME = 64, TSM_MAX_FRAME = 2048;
static constexpr int TSM_DEFAULT_FRAME = 512, TSM_DEFAULT_RADIUS = 160;
static constexpr int TSM_MAX_SEARCH_THREADS = 1024;
static constexpr int64_t TSM_MAX_LEN = (int64_t)1 << 30;
static constexpr unsigned TSM_QUIET_BITS = (127u - 100u) << 23;  // 2^-100

struct TsmItem {
    long long L, Lo;
};

__global__ __launch_bounds__(TSM_THREADS) void tsm_peak_kernel(const float* __restrict__ in, int64_t in_stride, const TsmItem* __restrict__ items,
                                                               unsigned* __restrict__ peak_bits) {
    const int b = blockIdx.y;
    const long long L = items[b].L;
    if (items[b].Lo == L) return;  // a copy: no search
    const float* x = in + (int64_t)b * in_stride;
    unsigned m = 0;
    for (long long i = (long long)blockIdx.x * TSM_THREADS + threadIdx.x; i < L; i += (long long)gridDim.x * TSM_THREADS) {
        const unsigned u = __float_as_uint(x[i]) & 0x7fffffffu;
        if (u < 0x7f800000u && u > m) m = u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned v = __shfl_xor(m, o);
        m = v > m ? v : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(peak_bits + b, m);
}

__device__ __forceinline__ short tsm_quant(const float* __restrict__ x, long long L, long long i, float scale) {
    if (i < 0 || i >= L) return 0;
    const float v = x[i];
    if ((__float_as_uint(v) & 0x7fffffffu) >= 0x7f800000u) return 0;  // inf, NaN
    const float r = fminf(fmaxf(rintf(__fmul_rn(v, scale)), -32767.f), 32767.f);
    return (short)(int)r;
}

__global__ __launch_bounds__(TSM_MAX_SEARCH_THREADS) void tsm_search_kernel(const float* __restrict__ in, int64_t in_stride,
                                                                            const TsmItem* __restrict__ items,
                                                                            const unsigned* __restrict__ peak_bits, int N, int D,
                                                                            int* __restrict__ centres, int64_t m_stride) {
    __shared__ short s_t[TSM_MAX_FRAME];      // q[c_{m-1} + k]
    __shared__ short s_r[2 * TSM_MAX_FRAME];  // q[a_m - D - Hs + j], j < N + 2 D
    __shared__ unsigned long long s_min[TSM_MAX_SEARCH_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const long long L = items[b].L, Lo = items[b].Lo;
    const int Hs = N >> 1;
    const long long M = (Lo + Hs - 1) / Hs + 1;
    int* c = centres + (int64_t)b * m_stride;
    const float* x = in + (int64_t)b * in_stride;
    const unsigned pb = Lo == L ? 0u : peak_bits[b];
    if (Lo == L || pb < TSM_QUIET_BITS) {  // d == 0 in every frame (uniform over the workgroup)
        for (long long m = tid; m < M; m += nt) c[m] = Lo > 0 ? (int)(m * Hs * L / Lo) : 0;
        return;
    }
    const float scale = __uint_as_float((268u - (pb >> 23)) << 23);  // 2^(14 - e), e = (pb >> 23) - 127
    const int nl = 2 * D + 1, nw = nt >> 6;
    int cprev = 0;
    if (tid == 0) c[0] = 0;
    for (long long m = 1; m < M; ++m) {
        const long long am = m * Hs * L / Lo;
        const long long r0 = am - D - Hs;
        for (int i = tid; i < N; i += nt) s_t[i] = tsm_quant(x, L, (long long)cprev + i, scale);
        for (int i = tid; i < N + 2 * D; i += nt) s_r[i] = tsm_quant(x, L, r0 + i, scale);
        __syncthreads();
        unsigned long long best = ~0ull;
        for (int j = tid; j < nl; j += nt) {
            const short* r = s_r + j;
            int sad = 0;
#pragma unroll 8
            for (int k = 0; k < N; ++k) {
                const int diff = (int)s_t[k] - (int)r[k];
                sad += diff < 0 ? -diff : diff;
            }
            const int d = j - D;
            const unsigned long long key = ((unsigned long long)(unsigned)sad << 12) | (unsigned)((d < 0 ? -d : d) << 1) | (d > 0 ? 1u : 0u);
            best = key < best ? key : best;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long v = __shfl_xor(best, o);
            best = v < best ? v : best;
        }
        if ((tid & 63) == 0) s_min[tid >> 6] = best;
        __syncthreads();  // also: s_t and s_r are read, the next frame may overwrite them
        best = s_min[0];
        for (int w = 1; w < nw; ++w) best = s_min[w] < best ? s_min[w] : best;
        const int ad = (int)((best & 0xfffu) >> 1);
        cprev = (int)am + ((best & 1u) ? ad : -ad);
        if (tid == 0) c[m] = cprev;
        // s_min is written again behind the next frame's first barrier, which no wave passes before all have read it here
    }
}

__global__ __launch_bounds__(TSM_THREADS) void tsm_ola_kernel(const float* __restrict__ in, int64_t in_stride, const TsmItem* __restrict__ items,
                                                              const int* __restrict__ centres, int64_t m_stride, const float* __restrict__ w,
                                                              int Hs, float* __restrict__ out, int64_t out_stride) {
    const int b = blockIdx.y;
    const long long L = items[b].L, Lo = items[b].Lo;
    const long long t = (long long)blockIdx.x * TSM_THREADS + threadIdx.x;
    if (t >= Lo) return;
    const float* x = in + (int64_t)b * in_stride;
    float* y = out + (int64_t)b * out_stride;
    if (Lo == L) {
        y[t] = x[t];
        return;
    }
    const long long m = t / Hs;
    const int k = (int)(t - m * Hs);
    const int* c = centres + (int64_t)b * m_stride;
    const long long i0 = (long long)c[m] + k, i1 = (long long)c[m + 1] - Hs + k;
    const float x0 = i0 >= 0 && i0 < L ? x[i0] : 0.f;
    const float x1 = i1 >= 0 && i1 < L ? x[i1] : 0.f;
    y[t] = __fadd_rn(__fmul_rn(w[k + Hs], x0), __fmul_rn(w[k], x1));
}

// ---- per device: the item table, the peaks, the centres and the window of the last frame size ------------------------------------

struct TsmDevice {
    int device;
    TsmItem* d_items = nullptr;
    unsigned* d_peak = nullptr;
    size_t item_cap = 0;
    int* d_c = nullptr;
    size_t c_cap = 0;
    float* d_w = nullptr;  // [TSM_MAX_FRAME]
    int w_frame = 0;
};
static std::mutex g_tsm_mutex;
static std::list<TsmDevice> g_tsm_devices;

// g_tsm_mutex held
static TsmDevice& tsm_device_state(int device, size_t n, size_t centres, int N) {
    TsmDevice* l = nullptr;
    for (auto& x : g_tsm_devices)
        if (x.device == device) l = &x;
    if (!l) {
        g_tsm_devices.push_back(TsmDevice{device});
        l = &g_tsm_devices.back();
    }
    if (l->item_cap < n) {
        if (l->d_items) (void)hipFree(l->d_items);
        if (l->d_peak) (void)hipFree(l->d_peak);
        l->d_items = nullptr, l->d_peak = nullptr, l->item_cap = 0;
        const size_t cap = std::max<size_t>(n, 64);
        SC_HIP(hipMalloc(reinterpret_cast<void**>(&l->d_items), cap * sizeof(TsmItem)));
        SC_HIP(hipMalloc(reinterpret_cast<void**>(&l->d_peak), cap * sizeof(unsigned)));
        l->item_cap = cap;
    }
    if (l->c_cap < centres) {
        if (l->d_c) (void)hipFree(l->d_c);
        l->d_c = nullptr, l->c_cap = 0;
        const size_t cap = std::max<size_t>(centres, 4096);
        SC_HIP(hipMalloc(reinterpret_cast<void**>(&l->d_c), cap * sizeof(int)));
        l->c_cap = cap;
    }
    if (!l->d_w) SC_HIP(hipMalloc(reinterpret_cast<void**>(&l->d_w), TSM_MAX_FRAME * sizeof(float)));
    if (l->w_frame != N) {
        std::vector<float> w((size_t)N);
        for (int k = 0; k < N; ++k) w[k] = (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (double)k / (double)N));
        l->w_frame = 0;
        SC_HIP(hipMemcpy(l->d_w, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
        l->w_frame = N;
    }
    return *l;
}

void run_time_stretch(const char* who, const float* d_in, int n, int64_t in_stride, const int64_t* h_in_len, const int64_t* h_out_len,
                      const ::sc_tsm_opts* opts, bool with_out, float* d_out, int64_t out_stride, int32_t* h_centres, int64_t m_stride) {
    // every argument check comes before the first device call
    int N = TSM_DEFAULT_FRAME, D = TSM_DEFAULT_RADIUS;
    static const ::sc_tsm_opts zero{};
    if (opts && std::memcmp(opts, &zero, sizeof(zero)) != 0) {
        SC_CHECK(opts->abi_version == SC_ABI_VERSION, "%s: options ABI version %d != library %d", who, opts->abi_version, SC_ABI_VERSION);
        if (opts->frame != 0) N = opts->frame;
        if (opts->radius != 0) D = opts->radius == -1 ? 0 : opts->radius;
    }
    SC_CHECK(d_in && h_in_len && h_out_len && (with_out ? d_out != nullptr : h_centres != nullptr), "%s: null argument", who);
    SC_CHECK(n >= 1 && n <= 65535, "%s: %d rows, the limit is 1..65535", who, n);
    SC_CHECK(N >= TSM_MIN_FRAME && N <= TSM_MAX_FRAME && N % 2 == 0, "%s: frame %d must be even and lie in %d..%d", who, N, TSM_MIN_FRAME,
             TSM_MAX_FRAME);
    SC_CHECK(D >= 0 && D <= N / 2, "%s: radius %d is outside 0..frame / 2 = %d (-1 in the options: none)", who, D, N / 2);
    SC_CHECK(in_stride >= 0 && (!with_out || out_stride >= 0), "%s: negative stride", who);
    const int Hs = N / 2;
    std::vector<TsmItem> items((size_t)n);
    int64_t max_l = 0, max_lo = 0, max_m = 1;
    bool any_search = false;
    for (int i = 0; i < n; ++i) {
        const int64_t L = h_in_len[i], Lo = h_out_len[i];
        SC_CHECK(L >= 0 && L <= in_stride, "%s: row %d has %lld samples, in_stride is %lld", who, i, (long long)L, (long long)in_stride);
        SC_CHECK(L <= TSM_MAX_LEN, "%s: row %d has %lld samples, above the limit of 2^30", who, i, (long long)L);
        SC_CHECK(Lo >= 0 && (!with_out || Lo <= out_stride), "%s: row %d has the out_len %lld, out_stride is %lld", who, i, (long long)Lo,
                 (long long)out_stride);
        SC_CHECK(L > 0 || Lo == 0, "%s: row %d is empty and cannot become %lld samples", who, i, (long long)Lo);
        SC_CHECK(L == 0 || (Lo >= 1 && Lo <= 4 * L && L <= 4 * Lo), "%s: row %d: %lld -> %lld samples is outside the ratio limit (out_len >= 1, 1/4 .. 4)",
                 who, i, (long long)L, (long long)Lo);
        items[i] = TsmItem{L, Lo};
        max_l = std::max(max_l, L), max_lo = std::max(max_lo, Lo);
        max_m = std::max(max_m, cdiv64(Lo, Hs) + 1);
        any_search = any_search || Lo != L;
    }
    if (with_out) {
        const char* ib = reinterpret_cast<const char*>(d_in);
        const char* ob = reinterpret_cast<const char*>(d_out);
        const int64_t in_bytes = (int64_t)n * in_stride * 4, out_bytes = (int64_t)n * out_stride * 4;
        SC_CHECK(ob + out_bytes <= ib || ib + in_bytes <= ob, "%s: d_out overlaps d_in", who);
        if (max_lo == 0) return;
    } else {
        SC_CHECK(m_stride >= max_m, "%s: m_stride %lld is below the %lld centres of the longest row", who, (long long)m_stride, (long long)max_m);
    }
    int device = 0;
    SC_HIP(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(g_tsm_mutex);
    TsmDevice& dv = tsm_device_state(device, (size_t)n, (size_t)n * (size_t)max_m, N);
    hipStream_t stream = nullptr;  // the default stream, like sc_resample: ordered behind the caller's work on it
    SC_HIP(hipMemcpyAsync(dv.d_items, items.data(), (size_t)n * sizeof(TsmItem), hipMemcpyHostToDevice, stream));
    if (any_search) {
        SC_HIP(hipMemsetAsync(dv.d_peak, 0, (size_t)n * sizeof(unsigned), stream));
        const unsigned chunks = (unsigned)std::min<int64_t>(std::max<int64_t>(cdiv64(max_l, TSM_THREADS * 8), 1), 1024);
        hipLaunchKernelGGL(tsm_peak_kernel, dim3(chunks, n), dim3(TSM_THREADS), 0, stream, d_in, in_stride, dv.d_items, dv.d_peak);
        SC_LAUNCH_CHECK();
    }
    const int threads = (int)std::min<int64_t>(align_up(2 * D + 1, 64), TSM_MAX_SEARCH_THREADS);
    hipLaunchKernelGGL(tsm_search_kernel, dim3(n), dim3(threads), 0, stream, d_in, in_stride, dv.d_items, dv.d_peak, N, D, dv.d_c, max_m);
    SC_LAUNCH_CHECK();
    if (with_out) {
        hipLaunchKernelGGL(tsm_ola_kernel, dim3((unsigned)cdiv64(max_lo, TSM_THREADS), n), dim3(TSM_THREADS), 0, stream, d_in, in_stride, dv.d_items,
                           dv.d_c, max_m, dv.d_w, Hs, d_out, out_stride);
        SC_LAUNCH_CHECK();
    }
    SC_HIP(hipStreamSynchronize(stream));  // items stays alive until the copy has run
    if (h_centres) {
        std::vector<int32_t> all((size_t)n * (size_t)max_m);
        SC_HIP(hipMemcpy(all.data(), dv.d_c, all.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i)
            std::copy_n(all.begin() + (size_t)i * max_m, (size_t)(cdiv64(items[i].Lo, Hs) + 1), h_centres + (int64_t)i * m_stride);
    }
}

}  // namespace sc

using namespace sc;

extern "C" {

int sc_time_stretch(const float* d_in, int32_t n, int64_t in_stride, const int64_t* h_in_len, const sc_tsm_opts* opts, float* d_out,
                    int64_t out_stride, const int64_t* h_out_len) {
    SC_API_BEGIN
    run_time_stretch("sc_time_stretch", d_in, n, in_stride, h_in_len, h_out_len, opts, true, d_out, out_stride, nullptr, 0);
    SC_API_END
}

}  // extern "C"
