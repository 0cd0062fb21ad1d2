// Long-form speech translation: the two kernels a dubbed track needs that the short-utterance chain
// does not have.  An extension of this project; the reference has no counterpart.
//
// ---- 1. Duration fit (fit_durations_kernel; sc_t2u_nar_fit, sc_op_fit_durations) ------------------------------------------------
// Item b has C_b characters.  e_k = expf(x_k) - 1.0f with x_k = h_k . w + b, the duration predictor's output: the operations
// of durations_kernel (k_misc.hip), in its order (lane l sums the columns l, l + 64, ... with fmaf, xor butterfly, + b[0]).
// For a factor f
//     dur_k(f) = clamp((long long)rintf(e_k * f), min_dur, 1000000)        (one fp32 product, ties to even)
//     U_b(f)   = sum_k dur_k(f)                                            (64-bit integers)
// U_b is non-decreasing in f >= 0 (min_dur >= 0): e_k * f is monotone in f for e_k >= 0, and a negative e_k rounds to at most 0
// and falls under the clamp.  The caller gives a target T_b in units (0: none) and bounds 0 < lo_b <= hi_b.  Candidates lie on
// a fixed grid, J = 65536:
//     f_J = hi_b;   f_j = fminf(hi_b, __fadd_rn(lo_b, __fmul_rn(__fsub_rn(hi_b, lo_b), j * 2^-16)))   for j < J
// (non-decreasing in j; f_0 = lo_b).  The result is the largest j with U_b(f_j) <= T_b: j = J is tested first (T_b = 0 takes
// it untested), then j = 0 - if even lo_b does not fit, the result is lo_b with flag bit 0 (FIT_OVER) - then at most 16
// bisection steps between a j that fits and one that does not.  Outputs: the factor, U_b at it, the flags, and
// durations[b][k] = dur_k(factor), 0 on the rows behind C_b.
//
// One workgroup of 256 threads per item.  Stage 1 (skipped when the e values are given): wave w takes the rows w, w + 4, ...;
// lane 0 writes e_k to the scratch row in global memory and, for k < FIT_LDS_ROWS, to LDS.  Stage 2: a candidate is one pass
// - thread t takes k = t, t + 256, ..., reads e_k from LDS (k < FIT_LDS_ROWS) or from the scratch row (char_max_seq_len goes to
// 10 000), rounds, clamps and adds in int64; the 64 lanes are reduced with an xor butterfly, the 4 waves through one LDS
// exchange (part[0] + part[1] + part[2] + part[3]).  The order is fixed and the additions are integer, so U_b does not depend
// on it; every thread holds the same total and the search is uniform over the workgroup.  The last pass writes the durations.
//
// ---- 2. Timeline mix (mix_timeline_kernel; sc_mix_timeline) ------------------------------------------------------------------
// n segments seg_i [L_i] placed at ascending sample offsets p_i in a track of T samples, over an optional bed [T].  All fp32,
// every operation below a single correctly rounded one (no contraction):
//     w_i(k) = fminf(1, fminf((float)(k + 1), (float)(L_i - k)) * inv_fade)       inv_fade = 1.0f / (float)(fade + 1), host
//     c_i(t) = fmaxf(0, 1.0f - (float)dist_i(t) / (float)(ramp + 1))              dist_i(t): samples from t to [p_i, p_i + L_i),
//                                                                                 0 inside; an empty segment covers nothing
//     c(t)   = max_i c_i(t)                                                       (0 without a segment within ramp)
//     term_i = (g_i * w_i(t - p_i)) * seg_i[t - p_i]                              for the segments that cover t
//     bedterm = bed[t] * (1.0f - a * c(t))                                        a = 1.0f - duck, host
//     out[t] = ((term_i1 + term_i2) + ...) + bedterm
// - the covering segments in ascending i, the bed term last; a list with one entry is that entry's bits (a lone segment with
// fade = 0 and gain = 1 is a copy, bed[t] passes where c(t) = 0), an empty list is +0.0f.
//
// One thread per output sample, 256 per workgroup, coalesced stores; every sample of out[0, T) is written.  The segment table
// {p_i, prefix maximum of the ends p_j + L_j (j <= i, host-built), L_i, g_i} lies in global memory; a workgroup finds the part
// that can reach its 256 samples with two binary searches (first i whose prefix-maximum end + ramp lies behind its first sample;
// first i with p_i - ramp behind its last) and stages it into LDS 256 entries at a time.  In a staged chunk every thread finds
// its first candidate by a binary search over the prefix maximum of the ends and scans forward while p_i - ramp <= t.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <list>
#include <mutex>
#include <vector>

#include "device_util.h"
#include "handle.h"

namespace sc {

static constexpr int FIT_THREADS = 256, FIT_WAVES = FIT_THREADS / 64;
static constexpr int FIT_LDS_ROWS = 2048;  // e values of an item kept in LDS (8 KB); rows behind are re-read from the scratch row
static constexpr int FIT_J = 65536;
static constexpr int FIT_OVER = 1;

__device__ __forceinline__ float fit_grid(float lo, float hi, int j) {
    if (j >= FIT_J) return hi;
    return fminf(hi, __fadd_rn(lo, __fmul_rn(__fsub_rn(hi, lo), (float)j * (1.0f / 65536.0f))));
}

// U(f) of the item in every thread; dur_out != null: the durations are written on the way
__device__ __forceinline__ long long fit_total(const float* e_lds, const float* e_row, int C, float f, int min_dur, long long* part,
                                               int* dur_out) {
    long long s = 0;
    for (int k = threadIdx.x; k < C; k += FIT_THREADS) {
        const float e = k < FIT_LDS_ROWS ? e_lds[k] : e_row[k];
        const float r = rintf(__fmul_rn(e, f));
        long long dl = (long long)r;
        if (dl < (long long)min_dur) dl = min_dur;
        if (dl > 1000000) dl = 1000000;
        if (dur_out) dur_out[k] = (int)dl;
        s += dl;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    const long long total = ((part[0] + part[1]) + part[2]) + part[3];
    __syncthreads();  // part is written again by the next candidate
    return total;
}

__global__ __launch_bounds__(FIT_THREADS) void fit_durations_kernel(FitArgs a) {
    __shared__ float e_lds[FIT_LDS_ROWS];
    __shared__ long long part[FIT_WAVES];
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C = min(max(a.lens[b], 0), a.s_char);
    float* e_row = a.e + (int64_t)b * a.s_char;
    int* dur_row = a.durations + (int64_t)b * a.s_char;
    if (a.h) {  // stage 1: durations_kernel's dot product and exponential, one wave per row
        for (int k = wave; k < C; k += FIT_WAVES) {
            const float* hr = a.h + ((int64_t)b * a.s_char + k) * a.ld;
            float acc = 0.f;
            for (int c = lane; c < a.H; c += 64) acc = fmaf(hr[c], a.w[c], acc);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
            if (lane == 0) {
                const float x = acc + a.b[0];
                const float e = expf(x) - 1.0f;
                e_row[k] = e;
                if (k < FIT_LDS_ROWS) e_lds[k] = e;
            }
        }
    } else {
        for (int k = threadIdx.x; k < C && k < FIT_LDS_ROWS; k += FIT_THREADS) e_lds[k] = e_row[k];
    }
    for (int k = C + threadIdx.x; k < a.s_char; k += FIT_THREADS) dur_row[k] = 0;
    __syncthreads();  // e_lds, and the workgroup's own writes to e_row, are visible to all of its threads

    const int T = a.target[b];
    const float lo = a.lo[b], hi = a.hi[b];
    int j = FIT_J, flags = 0;
    if (T > 0 && fit_total(e_lds, e_row, C, hi, a.min_dur, part, nullptr) > (long long)T) {
        if (fit_total(e_lds, e_row, C, fit_grid(lo, hi, 0), a.min_dur, part, nullptr) > (long long)T) {
            j = 0;
            flags = FIT_OVER;
        } else {
            int ok = 0, bad = FIT_J;  // U(f_ok) <= T < U(f_bad)
            while (bad - ok > 1) {
                const int mid = (ok + bad) >> 1;
                if (fit_total(e_lds, e_row, C, fit_grid(lo, hi, mid), a.min_dur, part, nullptr) <= (long long)T) ok = mid;
                else bad = mid;
            }
            j = ok;
        }
    }
    const float f = fit_grid(lo, hi, j);
    const long long total = fit_total(e_lds, e_row, C, f, a.min_dur, part, dur_row);
    if (threadIdx.x == 0) {
        a.factor[b] = f;
        a.total[b] = total;
        a.flags[b] = flags;
    }
}

void launch_fit_durations(const FitArgs& a, int n, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(fit_durations_kernel, dim3(n), dim3(FIT_THREADS), 0, s, a);
    SC_LAUNCH_CHECK();
}

// the checks of the fit's per-item arguments, shared by sc_t2u_nar_fit and the test hook: before any device work
void check_fit_items(const char* who, int n, const int32_t* h_target, const float* h_lo, const float* h_hi) {
    for (int b = 0; b < n; ++b) {
        SC_CHECK(h_target[b] >= 0, "%s: item %d has the negative target %d", who, b, h_target[b]);
        SC_CHECK(std::isfinite(h_lo[b]) && std::isfinite(h_hi[b]), "%s: item %d has a bound that is not finite (lo %g, hi %g)", who, b,
                 (double)h_lo[b], (double)h_hi[b]);
        SC_CHECK(h_lo[b] > 0.f, "%s: item %d has the lower bound %g, it must be above 0", who, b, (double)h_lo[b]);
        SC_CHECK(h_lo[b] <= h_hi[b], "%s: item %d has lo %g above hi %g", who, b, (double)h_lo[b], (double)h_hi[b]);
    }
}

// ---- timeline mix ---------------------------------------------------------------------------------------------------------

static constexpr int MIX_THREADS = 256, MIX_CHUNK = 256;
static constexpr int MIX_MAX_EDGE = 1 << 20;  // fade and ramp, samples: (float)dist stays exact

struct MixSeg {
    long long start;     // p_i
    long long pmax_end;  // max over j <= i of p_j + L_j
    int len;             // L_i
    float gain;          // g_i
};

__global__ __launch_bounds__(MIX_THREADS) void mix_timeline_kernel(const float* __restrict__ seg, int64_t seg_stride, const MixSeg* __restrict__ tab,
                                                                  int n, float inv_fade, const float* __restrict__ bed, float a, int ramp,
                                                                  float ramp1, float* __restrict__ out, int64_t T) {
    __shared__ MixSeg s[MIX_CHUNK];
    const int64_t t0 = (int64_t)blockIdx.x * MIX_THREADS;
    const int64_t t = t0 + threadIdx.x;
    const int64_t t_last = (t0 + MIX_THREADS < T ? t0 + MIX_THREADS : T) - 1;
    // the workgroup's part of the table (uniform): [i0, i1)
    int i0 = 0, i1 = n;
    for (int hi = n; i0 < hi;) {  // first i with pmax_end + ramp > t0
        const int mid = (i0 + hi) >> 1;
        if (tab[mid].pmax_end + ramp > t0) hi = mid;
        else i0 = mid + 1;
    }
    for (int lo = i0; lo < i1;) {  // first i with start - ramp > t_last
        const int mid = (lo + i1) >> 1;
        if (tab[mid].start - ramp > t_last) i1 = mid;
        else lo = mid + 1;
    }
    float sum = 0.f, c = 0.f;
    int covering = 0;
    for (int base = i0; base < i1; base += MIX_CHUNK) {
        const int m = i1 - base < MIX_CHUNK ? i1 - base : MIX_CHUNK;
        if (base != i0) __syncthreads();  // the chunk before is read
        if ((int)threadIdx.x < m) s[threadIdx.x] = tab[base + threadIdx.x];
        __syncthreads();
        if (t >= T) continue;
        int first = 0;
        for (int hi = m; first < hi;) {  // first entry whose prefix-maximum end + ramp lies behind t
            const int mid = (first + hi) >> 1;
            if (s[mid].pmax_end + ramp > t) hi = mid;
            else first = mid + 1;
        }
        for (int i = first; i < m && s[i].start - ramp <= t; ++i) {
            const int L = s[i].len;
            if (L <= 0) continue;
            const int64_t k = t - s[i].start;
            if (k >= 0 && k < L) {
                c = 1.0f;
                const float w = fminf(1.0f, __fmul_rn(fminf((float)(k + 1), (float)(L - k)), inv_fade));
                const float term = __fmul_rn(__fmul_rn(s[i].gain, w), seg[(int64_t)(base + i) * seg_stride + k]);
                sum = covering ? __fadd_rn(sum, term) : term;
                ++covering;
            } else {
                const int64_t dist = k < 0 ? -k : k - L + 1;
                if (dist <= ramp) c = fmaxf(c, fmaxf(0.f, __fsub_rn(1.0f, __fdiv_rn((float)dist, ramp1))));
            }
        }
    }
    if (t >= T) return;
    if (bed) {
        const float bedterm = __fmul_rn(bed[t], __fsub_rn(1.0f, __fmul_rn(a, c)));
        sum = covering ? __fadd_rn(sum, bedterm) : bedterm;
    }
    out[t] = sum;
}

struct MixDevice {
    int device;
    MixSeg* d_tab = nullptr;
    size_t cap = 0;
};
static std::mutex g_mix_mutex;
static std::list<MixDevice> g_mix_devices;

// g_mix_mutex held
static MixDevice& mix_device_state(int device, size_t n) {
    MixDevice* l = nullptr;
    for (auto& x : g_mix_devices)
        if (x.device == device) l = &x;
    if (!l) {
        g_mix_devices.push_back(MixDevice{device});
        l = &g_mix_devices.back();
    }
    if (l->cap < n) {
        if (l->d_tab) (void)hipFree(l->d_tab);
        l->d_tab = nullptr, l->cap = 0;
        const size_t cap = std::max<size_t>(n, 256);
        SC_HIP(hipMalloc(reinterpret_cast<void**>(&l->d_tab), cap * sizeof(MixSeg)));
        l->cap = cap;
    }
    return *l;
}

}  // namespace sc

using namespace sc;

extern "C" {

int sc_op_fit_durations(const float* d_e, int32_t n, int32_t s_char, const int32_t* h_char_lens, const int32_t* h_target, const float* h_lo,
                        const float* h_hi, int32_t min_dur, int32_t* h_durations, float* h_factor, int64_t* h_total, int32_t* h_flags) {
    SC_API_BEGIN
    SC_CHECK(d_e && h_char_lens && h_target && h_lo && h_hi && h_durations && h_factor && h_total && h_flags, "sc_op_fit_durations: null argument");
    SC_CHECK(n >= 1 && n <= 65535 && s_char >= 1, "sc_op_fit_durations: n %d (1..65535), s_char %d (>= 1)", n, s_char);
    SC_CHECK(min_dur >= 0 && min_dur <= 1000000, "sc_op_fit_durations: min_dur %d is outside 0..1000000", min_dur);
    for (int b = 0; b < n; ++b)
        SC_CHECK(h_char_lens[b] >= 0 && h_char_lens[b] <= s_char, "sc_op_fit_durations: item %d has %d characters, s_char is %d", b, h_char_lens[b], s_char);
    check_fit_items("sc_op_fit_durations", n, h_target, h_lo, h_hi);
    OpScratch sc;
    const size_t rows = (size_t)n * s_char;
    FitArgs a;
    a.e = sc.get<float>(rows);
    SC_HIP(hipMemcpy(a.e, d_e, rows * 4, hipMemcpyDeviceToDevice));  // the kernel's scratch row: the caller's values stay untouched
    a.s_char = s_char;
    a.lens = sc.put(std::vector<int>(h_char_lens, h_char_lens + n));
    a.target = sc.put(std::vector<int>(h_target, h_target + n));
    a.lo = sc.put(std::vector<float>(h_lo, h_lo + n));
    a.hi = sc.put(std::vector<float>(h_hi, h_hi + n));
    a.min_dur = min_dur;
    a.durations = sc.get<int>(rows);
    a.factor = sc.get<float>(n);
    a.total = sc.get<long long>(n);
    a.flags = sc.get<int>(n);
    launch_fit_durations(a, n, nullptr);
    static_assert(sizeof(long long) == sizeof(int64_t), "totals travel as int64");
    SC_HIP(hipMemcpy(h_durations, a.durations, rows * 4, hipMemcpyDeviceToHost));
    SC_HIP(hipMemcpy(h_factor, a.factor, (size_t)n * 4, hipMemcpyDeviceToHost));
    SC_HIP(hipMemcpy(h_total, a.total, (size_t)n * 8, hipMemcpyDeviceToHost));
    SC_HIP(hipMemcpy(h_flags, a.flags, (size_t)n * 4, hipMemcpyDeviceToHost));
    SC_API_END
}

int sc_mix_timeline(const float* d_seg, int32_t n, int64_t seg_stride, const int32_t* h_len, const int64_t* h_start, const float* h_gain,
                    int32_t fade, const float* d_bed, float duck, int32_t ramp, float* d_out, int64_t T) {
    SC_API_BEGIN
    // every argument check comes before the first device call
    SC_CHECK(n >= 0 && T >= 0 && seg_stride >= 0, "sc_mix_timeline: n %d, T %lld, seg_stride %lld: none may be negative", n, (long long)T,
             (long long)seg_stride);
    SC_CHECK(d_out || T == 0, "sc_mix_timeline: null argument (d_out)");
    SC_CHECK(n == 0 || (d_seg && h_len && h_start && h_gain), "sc_mix_timeline: null argument");
    SC_CHECK(fade >= 0 && fade <= MIX_MAX_EDGE, "sc_mix_timeline: fade %d is outside 0..%d samples", fade, MIX_MAX_EDGE);
    SC_CHECK(ramp >= 0 && ramp <= MIX_MAX_EDGE, "sc_mix_timeline: ramp %d is outside 0..%d samples", ramp, MIX_MAX_EDGE);
    SC_CHECK(duck >= 0.f && duck <= 1.f, "sc_mix_timeline: duck %g is outside [0, 1]", (double)duck);  // (a NaN fails both)
    SC_CHECK(cdiv64(T, MIX_THREADS) <= 0x7fffffff, "sc_mix_timeline: T %lld needs more workgroups than one launch has", (long long)T);
    std::vector<MixSeg> tab((size_t)n);
    long long pmax = 0;
    for (int i = 0; i < n; ++i) {
        SC_CHECK(h_len[i] >= 0 && (int64_t)h_len[i] <= seg_stride, "sc_mix_timeline: segment %d has %d samples, seg_stride is %lld", i, h_len[i],
                 (long long)seg_stride);
        SC_CHECK(h_start[i] >= 0, "sc_mix_timeline: segment %d starts at %lld, before the track", i, (long long)h_start[i]);
        SC_CHECK(i == 0 || h_start[i] >= h_start[i - 1], "sc_mix_timeline: segment %d starts at %lld, before segment %d at %lld (starts ascend)", i,
                 (long long)h_start[i], i - 1, (long long)h_start[i - 1]);
        SC_CHECK(h_start[i] <= T && h_len[i] <= T - h_start[i], "sc_mix_timeline: segment %d covers [%lld, %lld), the track has %lld samples", i,
                 (long long)h_start[i], (long long)h_start[i] + h_len[i], (long long)T);
        SC_CHECK(std::isfinite(h_gain[i]), "sc_mix_timeline: segment %d has a gain that is not finite", i);
        pmax = std::max<long long>(pmax, h_start[i] + h_len[i]);
        tab[i] = MixSeg{h_start[i], pmax, h_len[i], h_gain[i]};
    }
    if (T == 0) return SC_OK;
    int device = 0;
    SC_HIP(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(g_mix_mutex);
    MixDevice& dv = mix_device_state(device, (size_t)n);
    hipStream_t stream = nullptr;  // the default stream, like sc_resample: ordered behind the caller's work on it
    if (n > 0) SC_HIP(hipMemcpyAsync(dv.d_tab, tab.data(), (size_t)n * sizeof(MixSeg), hipMemcpyHostToDevice, stream));
    const float inv_fade = 1.0f / (float)(fade + 1), a = 1.0f - duck;
    hipLaunchKernelGGL(mix_timeline_kernel, dim3((unsigned)cdiv64(T, MIX_THREADS)), dim3(MIX_THREADS), 0, stream, d_seg, seg_stride, dv.d_tab, n,
                       inv_fade, d_bed, a, ramp, (float)(ramp + 1), d_out, T);
    SC_LAUNCH_CHECK();
    SC_HIP(hipStreamSynchronize(stream));  // tab stays alive until the copy has run
    SC_API_END
}

}  // extern "C"
