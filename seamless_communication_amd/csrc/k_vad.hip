// Speech probability per window (sc_vad_probs): the track the reference takes from Silero VAD in front of its
// segmentation of long input (segment/silero_vad.py get_speech_probs), here from an energy detector whose threshold adapts to the
// row.  No weights, no handle.
//
// Kernel 1, window energies: one wavefront per window, VAD_WAVES windows per workgroup.  The window's samples stay in registers
// between the two passes (mean, then the sum of squared deviations); lane l holds the samples 4 * (j * 64 + l) + {0, 1, 2, 3}, so a
// window whose first sample is 16-byte aligned is read with one float4 load per lane and step, and any other window (a row starts
// at i * wav_stride, a window at w * W: neither need be a multiple of 4 samples) with four scalar loads that touch the same cache
// lines.  Both paths put the same sample into the same register, the per-lane sums run in ascending order and the 64 lanes are
// reduced with an xor butterfly: a window's bits depend on its own samples only.
// Kernel 2, one workgroup per row: the count of finite windows, both order statistics from a radix select on the order-preserving
// integer image of the floats (sign flip, four 8-bit passes, one 256-bin LDS histogram per statistic), then the threshold, the
// hangover maximum and the logistic for every window of the row, and the zero tails.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <list>
#include <mutex>
#include <vector>

#include "device_util.h"
#include "handle.h"

namespace sc {

static constexpr int VAD_THREADS = 256;
static constexpr int VAD_WAVES = VAD_THREADS / 64;
static constexpr int VAD_MIN_WINDOW = 32, VAD_MAX_WINDOW = 8192;
static constexpr int64_t VAD_MAX_WINDOWS = (int64_t)1 << 20;
static constexpr int VAD_MAX_HANGOVER = 8;
static constexpr double VAD_FLOOR_QUANTILE = 0.10, VAD_PEAK_QUANTILE = 0.95;

struct VadParams {
    double floor_q = VAD_FLOOR_QUANTILE, peak_q = VAD_PEAK_QUANTILE;
    float ceiling_db = -45.f, margin_db = 6.f, range_fraction = 0.35f, slope_db = 1.5f;
    int hangover = 1;
};

// ---- kernel 1 -----------------------------------------------------------------------------------------------------------------

// NV: float4 steps per lane, NV * 256 >= W
template <int NV>
__global__ __launch_bounds__(VAD_THREADS) void vad_energy_kernel(const float* __restrict__ wav, int64_t wav_stride, const int64_t* __restrict__ len,
                                                                 int W, float* __restrict__ db, int64_t db_stride) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * VAD_WAVES + (threadIdx.x >> 6);
    const int64_t row = blockIdx.y;
    const int64_t L = len[row];
    if (w * W >= L) return;  // the whole wavefront: no window w in this row
    const float* x = wav + row * wav_stride + w * W;
    const int64_t left = L - w * W;
    const int valid = left < W ? (int)left : W;  // samples of the window inside the row; zeros behind them
    const bool aligned = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    float v[NV][4];
    bool bad = false;
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int q = (j * 64 + lane) * 4;
        if (aligned && q + 3 < valid) {
            const float4 t = *reinterpret_cast<const float4*>(x + q);
            v[j][0] = t.x, v[j][1] = t.y, v[j][2] = t.z, v[j][3] = t.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[j][e] = q + e < valid ? x[q + e] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            bad |= !__builtin_isfinite(v[j][e]);
            sum += v[j][e];
        }
    }
    const float inv_w = 1.f / (float)W;
    const float mean = wave_sum(sum) * inv_w;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int q = (j * 64 + lane) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float d = q + e < W ? v[j][e] - mean : 0.f;  // the zero padding up to W belongs to the window
            acc = fmaf(d, d, acc);
        }
    }
    const float energy = wave_sum(acc) * inv_w;
    const bool any_bad = __any(bad ? 1 : 0) != 0;
    float out = 10.f * log10f(fmaxf(energy, 1e-10f));
    if (any_bad || !__builtin_isfinite(energy)) out = __builtin_nanf("");
    if (lane == 0) db[row * db_stride + w] = out;
}

// ---- kernel 2 -----------------------------------------------------------------------------------------------------------------

// order-preserving image: a < b as floats <=> key(a) < key(b) as unsigned (-0 below +0)
__device__ __forceinline__ uint32_t vad_key(float f) {
    const uint32_t b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float vad_unkey(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

__global__ __launch_bounds__(VAD_THREADS) void vad_prob_kernel(float* __restrict__ db, int64_t db_stride, int db_tail, const int64_t* __restrict__ len, int W,
                                                               VadParams p, float* __restrict__ probs, int64_t probs_stride, float* __restrict__ stats) {
    __shared__ unsigned s_hist[2][256];
    __shared__ unsigned s_count;
    __shared__ unsigned s_rank[2], s_prefix[2];
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x;
    const int64_t L = len[row];
    const int nw = (int)((L + W - 1) / W);
    float* d = db + row * db_stride;
    float* pr = probs + row * probs_stride;
    if (tid == 0) s_count = 0;
    __syncthreads();
    unsigned mine = 0;
    for (int i = tid; i < nw; i += VAD_THREADS) mine += d[i] == d[i] ? 1u : 0u;
    if (mine) atomicAdd(&s_count, mine);
    __syncthreads();
    const unsigned k = s_count;
    // the zero tails
    for (int64_t i = nw + tid; i < probs_stride; i += VAD_THREADS) pr[i] = 0.f;
    if (db_tail)
        for (int64_t i = nw + tid; i < db_stride; i += VAD_THREADS) d[i] = 0.f;
    const float nan = __builtin_nanf("");
    if (k == 0) {  // the whole workgroup
        for (int i = tid; i < nw; i += VAD_THREADS) pr[i] = nan;
        if (tid == 0) stats[row * 4 + 0] = nan, stats[row * 4 + 1] = nan, stats[row * 4 + 2] = nan, stats[row * 4 + 3] = 0.f;
        return;
    }
    if (tid < 2) {
        const double q = tid == 0 ? p.floor_q : p.peak_q;
        unsigned r = (unsigned)floor(q * (double)(k - 1));
        s_rank[tid] = r < k ? r : k - 1;
        s_prefix[tid] = 0;
    }
    uint32_t mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        s_hist[0][tid] = 0;
        s_hist[1][tid] = 0;
        __syncthreads();  // also orders s_rank / s_prefix of the pass before
        const uint32_t pf0 = s_prefix[0], pf1 = s_prefix[1];
        for (int i = tid; i < nw; i += VAD_THREADS) {
            const float f = d[i];
            if (f != f) continue;
            const uint32_t key = vad_key(f);
            const unsigned bin = (key >> shift) & 255u;
            if ((key & mask) == pf0) atomicAdd(&s_hist[0][bin], 1u);
            if ((key & mask) == pf1) atomicAdd(&s_hist[1][bin], 1u);
        }
        __syncthreads();
        if (tid < 2) {  // the bin that holds the rank among the keys of this prefix
            unsigned r = s_rank[tid], below = 0;
            int b = 0;
            for (; b < 255; ++b) {
                const unsigned h = s_hist[tid][b];
                if (below + h > r) break;
                below += h;
            }
            s_rank[tid] = r - below;
            s_prefix[tid] |= (uint32_t)b << shift;
        }
        mask |= 0xffu << shift;
        __syncthreads();
    }
    const float Fq = vad_unkey(s_prefix[0]), P = vad_unkey(s_prefix[1]);
    const float F = fminf(Fq, p.ceiling_db);
    const float c = F + fmaxf(p.margin_db, p.range_fraction * (P - F));
    if (tid == 0) stats[row * 4 + 0] = F, stats[row * 4 + 1] = P, stats[row * 4 + 2] = c, stats[row * 4 + 3] = (float)k;
    for (int i = tid; i < nw; i += VAD_THREADS) {
        const float own = d[i];
        float out = nan;
        if (own == own) {
            float s = own;
            const int lo = i - p.hangover < 0 ? 0 : i - p.hangover;
            const int hi = i + p.hangover > nw - 1 ? nw - 1 : i + p.hangover;
            for (int j = lo; j <= hi; ++j) {
                const float t = d[j];
                if (t == t && t > s) s = t;
            }
            out = 1.f / (1.f + expf(-(s - c) / p.slope_db));
        }
        pr[i] = out;
    }
}

// ---- the streaming detector (sc_vad_stream_*) -------------------------------------------------------------
//
// State per lane: the levels of the last H windows as a ring (slot = window number mod H; NaN = no level: a slot not written since
// the reset, or a window that has none), the levels of the last VAD_STREAM_RECENT windows for the hangover (slot = window number
// mod 8: the hangover does not depend on H), the number of windows since the reset and F, P, c, k of the last window.
// A push is vad_energy_kernel over the whole windows of every named lane, then this kernel: one workgroup per named lane walks
// the lane's new windows in order - append, count, radix select of both order statistics over the ring in LDS (the 256 bins of a
// pass are scanned by one wavefront per statistic: four bins a lane, a shuffle prefix sum, a ballot for the bin that holds the
// rank - the walk of one thread over the bins that vad_prob_kernel makes once per row would cost about 30 us per window here),
// backwards maximum, logistic.  A window's result is a function of the lane's levels up to it: neither the cut into pushes nor the
// companions of a push enter.

static constexpr int VAD_STREAM_MAX_HISTORY = 1024, VAD_STREAM_DEFAULT_HISTORY = 312;
static constexpr int VAD_STREAM_RECENT = 8;  // >= VAD_MAX_HANGOVER, a power of two
static constexpr int VAD_STREAM_STATS = 5;   // F, P, c, k, windows handled
static_assert(VAD_STREAM_RECENT >= VAD_MAX_HANGOVER && (VAD_STREAM_RECENT & (VAD_STREAM_RECENT - 1)) == 0, "hangover ring");

struct VadStreamState {
    float* ring;     // [sessions][H]
    float* recent;   // [sessions][VAD_STREAM_RECENT]
    float* last;     // [sessions][4]: F, P, c, k of the lane's last window
    int64_t* count;  // [sessions]: windows since the reset
};

// lanes == nullptr: every lane, blockIdx.x is the lane
__global__ __launch_bounds__(VAD_THREADS) void vad_stream_reset_kernel(VadStreamState st, int H, const int32_t* __restrict__ lanes) {
    const int64_t sid = lanes ? lanes[blockIdx.x] : (int)blockIdx.x;
    const float nan = __builtin_nanf("");
    for (int i = threadIdx.x; i < H; i += VAD_THREADS) st.ring[sid * H + i] = nan;
    if (threadIdx.x < VAD_STREAM_RECENT) st.recent[sid * VAD_STREAM_RECENT + threadIdx.x] = nan;
    if (threadIdx.x < 4) st.last[sid * 4 + threadIdx.x] = threadIdx.x == 3 ? 0.f : nan;
    if (threadIdx.x == 0) st.count[sid] = 0;
}

// len[b]: samples of the whole windows of named lane b (a multiple of W); db [n][db_stride] from vad_energy_kernel
__global__ __launch_bounds__(VAD_THREADS) void vad_stream_kernel(const float* __restrict__ db, int64_t db_stride, const int64_t* __restrict__ len,
                                                                 const int32_t* __restrict__ lanes, int W, int H, VadParams p, VadStreamState st,
                                                                 float* __restrict__ probs, int64_t probs_stride, float* __restrict__ stats) {
    __shared__ float s_ring[VAD_STREAM_MAX_HISTORY];
    __shared__ float s_recent[VAD_STREAM_RECENT];
    __shared__ unsigned s_hist[2][256];
    __shared__ unsigned s_count;
    __shared__ unsigned s_rank[2], s_prefix[2];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t sid = lanes[b];
    const int nw = (int)(len[b] / W);
    float* ring = st.ring + sid * H;
    const float* d = db + b * db_stride;
    float* pr = probs + b * probs_stride;
    for (int i = tid; i < H; i += VAD_THREADS) s_ring[i] = ring[i];
    if (tid < VAD_STREAM_RECENT) s_recent[tid] = st.recent[sid * VAD_STREAM_RECENT + tid];
    const int64_t t0 = st.count[sid];
    float F = st.last[sid * 4 + 0], P = st.last[sid * 4 + 1], c = st.last[sid * 4 + 2];
    unsigned k = (unsigned)st.last[sid * 4 + 3];
    const float nan = __builtin_nanf("");
    for (int j = 0; j < nw; ++j) {
        const int64_t t = t0 + j;
        const float own = d[j];
        __syncthreads();  // the loads above; every read of s_count / s_prefix of the window before
        if (tid == 0) {
            const int slot = (int)(t % H);
            s_ring[slot] = own;
            ring[slot] = own;
            s_count = 0;
        }
        __syncthreads();
        unsigned mine = 0;
        for (int i = tid; i < H; i += VAD_THREADS) mine += s_ring[i] == s_ring[i] ? 1u : 0u;
        if (mine) atomicAdd(&s_count, mine);
        __syncthreads();
        k = s_count;
        if (k == 0) {  // the whole workgroup: no level in the history, so this window has none either
            F = P = c = nan;
            if (tid == 0) pr[j] = nan, s_recent[t & (VAD_STREAM_RECENT - 1)] = own;
            continue;
        }
        if (tid < 2) {
            const double q = tid == 0 ? p.floor_q : p.peak_q;
            unsigned r = (unsigned)floor(q * (double)(k - 1));
            s_rank[tid] = r < k ? r : k - 1;
            s_prefix[tid] = 0;
        }
        uint32_t mask = 0;
        for (int shift = 24; shift >= 0; shift -= 8) {
            s_hist[0][tid] = 0;
            s_hist[1][tid] = 0;
            __syncthreads();  // also orders s_rank / s_prefix of the pass before
            const uint32_t pf0 = s_prefix[0], pf1 = s_prefix[1];
            for (int i = tid; i < H; i += VAD_THREADS) {
                const float f = s_ring[i];
                if (f != f) continue;
                const uint32_t key = vad_key(f);
                const unsigned bin = (key >> shift) & 255u;
                if ((key & mask) == pf0) atomicAdd(&s_hist[0][bin], 1u);
                if ((key & mask) == pf1) atomicAdd(&s_hist[1][bin], 1u);
            }
            __syncthreads();
            if (tid < 128) {  // the bin that holds the rank among the keys of this prefix: wavefront 0 the floor's, wavefront 1 the peak's
                const int w = tid >> 6, l = tid & 63;
                const unsigned r = s_rank[w];
                const unsigned h0 = s_hist[w][4 * l], h1 = s_hist[w][4 * l + 1], h2 = s_hist[w][4 * l + 2], h3 = s_hist[w][4 * l + 3];
                const unsigned own4 = h0 + h1 + h2 + h3;
                unsigned incl = own4;  // keys in the bins 0 .. 4 l + 3
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const unsigned up = __shfl_up(incl, o);
                    if (l >= o) incl += up;
                }
                const unsigned long long holds = __ballot(incl > r);  // never empty: the rank is below the number of keys of the prefix
                if (holds && l == __ffsll((long long)holds) - 1) {
                    unsigned below = incl - own4;
                    int bin = 4 * l;
                    if (below + h0 <= r) {
                        below += h0, ++bin;
                        if (below + h1 <= r) {
                            below += h1, ++bin;
                            if (below + h2 <= r) below += h2, ++bin;
                        }
                    }
                    s_rank[w] = r - below;
                    s_prefix[w] |= (uint32_t)bin << shift;
                }
            }
            mask |= 0xffu << shift;
            __syncthreads();
        }
        P = vad_unkey(s_prefix[1]);
        F = fminf(vad_unkey(s_prefix[0]), p.ceiling_db);
        c = F + fmaxf(p.margin_db, p.range_fraction * (P - F));
        if (tid == 0) {
            float out = nan;
            if (own == own) {
                float s = own;
                for (int i = 1; i <= p.hangover && t - i >= 0; ++i) {  // backwards only, clipped at the reset
                    const float u = s_recent[(t - i) & (VAD_STREAM_RECENT - 1)];
                    if (u == u && u > s) s = u;
                }
                out = 1.f / (1.f + expf(-(s - c) / p.slope_db));
            }
            pr[j] = out;
            s_recent[t & (VAD_STREAM_RECENT - 1)] = own;
        }
    }
    __syncthreads();
    if (tid == 0) {
        st.count[sid] = t0 + nw;
        st.last[sid * 4 + 0] = F, st.last[sid * 4 + 1] = P, st.last[sid * 4 + 2] = c, st.last[sid * 4 + 3] = (float)k;
        for (int i = 0; i < VAD_STREAM_RECENT; ++i) st.recent[sid * VAD_STREAM_RECENT + i] = s_recent[i];
        float* o = stats + b * VAD_STREAM_STATS;
        o[0] = F, o[1] = P, o[2] = c, o[3] = (float)k, o[4] = (float)nw;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

static bool number(float v) { return std::isfinite(v); }

// every check of the options; a zero field stands for its default
static VadParams checked_vad_opts(const sc_vad_opts* o, const char* who = "sc_vad_probs") {
    VadParams r;
    static const sc_vad_opts zero{};
    if (!o || std::memcmp(o, &zero, sizeof(zero)) == 0) return r;
    SC_CHECK(o->abi_version == SC_ABI_VERSION, "%s: options ABI version %d != library %d", who, o->abi_version, SC_ABI_VERSION);
    SC_CHECK(o->hangover >= -1 && o->hangover <= VAD_MAX_HANGOVER, "%s: hangover %d is outside the limit -1..%d", who, o->hangover, VAD_MAX_HANGOVER);
    SC_CHECK(number(o->floor_quantile) && number(o->peak_quantile) && number(o->noise_ceiling_db) && number(o->min_margin_db) &&
                 number(o->range_fraction) && number(o->slope_db),
             "%s: an option is not a number", who);
    SC_CHECK(o->floor_quantile >= 0.f && o->floor_quantile <= 1.f, "%s: floor_quantile %g is outside [0, 1]", who, (double)o->floor_quantile);
    SC_CHECK(o->peak_quantile >= 0.f && o->peak_quantile <= 1.f, "%s: peak_quantile %g is outside [0, 1]", who, (double)o->peak_quantile);
    SC_CHECK(o->min_margin_db >= 0.f, "%s: min_margin_db %g is negative", who, (double)o->min_margin_db);
    SC_CHECK(o->range_fraction >= 0.f, "%s: range_fraction %g is negative", who, (double)o->range_fraction);
    SC_CHECK(o->slope_db >= 0.f, "%s: slope_db %g is negative (0 stands for the default)", who, (double)o->slope_db);
    if (o->hangover != 0) r.hangover = o->hangover < 0 ? 0 : o->hangover;
    // the struct carries the quantiles as fp32: a field that holds its default rounded to fp32 stands for the default itself
    if (o->floor_quantile != 0.f && o->floor_quantile != (float)VAD_FLOOR_QUANTILE) r.floor_q = (double)o->floor_quantile;
    if (o->peak_quantile != 0.f && o->peak_quantile != (float)VAD_PEAK_QUANTILE) r.peak_q = (double)o->peak_quantile;
    if (o->noise_ceiling_db != 0.f) r.ceiling_db = o->noise_ceiling_db;
    if (o->min_margin_db != 0.f) r.margin_db = o->min_margin_db;
    if (o->range_fraction != 0.f) r.range_fraction = o->range_fraction;
    if (o->slope_db != 0.f) r.slope_db = o->slope_db;
    return r;
}

// per device: the lengths, the statistics and the dB track of a call without d_db; grown on demand, never shrunk
struct VadDevice {
    int device;
    int64_t* d_len = nullptr;
    float* d_stats = nullptr;
    size_t rows = 0;
    float* d_db = nullptr;
    size_t db_floats = 0;
};
static std::mutex g_vad_mutex;
static std::list<VadDevice> g_vad_devices;

// g_vad_mutex held
static VadDevice& vad_device_state(int device, size_t n, size_t db_floats) {
    VadDevice* l = nullptr;
    for (auto& x : g_vad_devices)
        if (x.device == device) l = &x;
    if (!l) {
        g_vad_devices.push_back(VadDevice{device});
        l = &g_vad_devices.back();
    }
    if (l->rows < n) {
        if (l->d_len) (void)hipFree(l->d_len);
        if (l->d_stats) (void)hipFree(l->d_stats);
        l->d_len = nullptr, l->d_stats = nullptr, l->rows = 0;
        const size_t cap = std::max<size_t>(n, 64);
        SC_HIP(hipMalloc(reinterpret_cast<void**>(&l->d_len), cap * sizeof(int64_t)));
        SC_HIP(hipMalloc(reinterpret_cast<void**>(&l->d_stats), cap * 4 * sizeof(float)));
        l->rows = cap;
    }
    if (l->db_floats < db_floats) {
        if (l->d_db) (void)hipFree(l->d_db);
        l->d_db = nullptr, l->db_floats = 0;
        SC_HIP(hipMalloc(reinterpret_cast<void**>(&l->d_db), db_floats * sizeof(float)));
        l->db_floats = db_floats;
    }
    return *l;
}

template <int NV>
static void launch_energy(dim3 grid, hipStream_t stream, const float* d_wav, int64_t wav_stride, const int64_t* d_len, int W, float* d_db, int64_t db_stride) {
    hipLaunchKernelGGL(vad_energy_kernel<NV>, grid, dim3(VAD_THREADS), 0, stream, d_wav, wav_stride, d_len, W, d_db, db_stride);
}

static void launch_energy_for(int window, dim3 grid, hipStream_t stream, const float* d_wav, int64_t wav_stride, const int64_t* d_len, float* d_db,
                              int64_t db_stride) {
    if (window <= 512)
        launch_energy<2>(grid, stream, d_wav, wav_stride, d_len, window, d_db, db_stride);
    else if (window <= 2048)
        launch_energy<8>(grid, stream, d_wav, wav_stride, d_len, window, d_db, db_stride);
    else
        launch_energy<32>(grid, stream, d_wav, wav_stride, d_len, window, d_db, db_stride);
}

}  // namespace sc

// The streaming detector's handle.  Nothing of it lives on a device until the first reset or push: creation checks and records.
struct sc_vad_stream {
    int sessions = 0, window = 0, history = 0;
    sc::VadParams p;
    int device = -1;  // the device of the first reset / push; every later call must run on it
    sc::VadStreamState st{};
    int64_t* d_len = nullptr;  // [sessions] int64 lengths, then [sessions] int32 lanes: one copy per push
    float* d_stats = nullptr;  // [sessions][VAD_STREAM_STATS]
    float* d_db = nullptr;     // the levels of a push without d_db; grown on demand
    size_t db_floats = 0;
    std::vector<int64_t> h_meta;
    std::vector<char> named;
    std::mutex mutex;
};

namespace sc {

// mutex held; argument checks done
static void vad_stream_on_device(sc_vad_stream& h) {
    int device = 0;
    SC_HIP(hipGetDevice(&device));
    if (h.device >= 0) {
        SC_CHECK(device == h.device, "sc_vad_stream: the handle lives on device %d, the current device is %d", h.device, device);
        return;
    }
    const size_t n = (size_t)h.sessions;
    SC_HIP(hipMalloc(reinterpret_cast<void**>(&h.st.ring), n * h.history * sizeof(float)));
    SC_HIP(hipMalloc(reinterpret_cast<void**>(&h.st.recent), n * VAD_STREAM_RECENT * sizeof(float)));
    SC_HIP(hipMalloc(reinterpret_cast<void**>(&h.st.last), n * 4 * sizeof(float)));
    SC_HIP(hipMalloc(reinterpret_cast<void**>(&h.st.count), n * sizeof(int64_t)));
    SC_HIP(hipMalloc(reinterpret_cast<void**>(&h.d_len), n * (sizeof(int64_t) + sizeof(int32_t))));
    SC_HIP(hipMalloc(reinterpret_cast<void**>(&h.d_stats), n * VAD_STREAM_STATS * sizeof(float)));
    h.device = device;
    hipLaunchKernelGGL(vad_stream_reset_kernel, dim3((unsigned)n), dim3(VAD_THREADS), 0, nullptr, h.st, h.history, (const int32_t*)nullptr);
    SC_LAUNCH_CHECK();
}

// the named lanes: each inside 0..sessions-1, none twice
static void check_lanes(sc_vad_stream& h, const char* who, const int32_t* sids, int32_t n) {
    SC_CHECK(n >= 0 && n <= h.sessions, "%s: %d lanes named, the handle has %d", who, n, h.sessions);
    SC_CHECK(n == 0 || sids, "%s: null argument", who);
    h.named.assign((size_t)h.sessions, 0);
    for (int i = 0; i < n; ++i) {
        SC_CHECK(sids[i] >= 0 && sids[i] < h.sessions, "%s: lane %d is out of range 0..%d", who, sids[i], h.sessions - 1);
        SC_CHECK(!h.named[sids[i]], "%s: duplicate lane %d", who, sids[i]);
        h.named[sids[i]] = 1;
    }
}

}  // namespace sc

using namespace sc;

extern "C" {

int64_t sc_vad_windows(int64_t num_samples, int32_t window) {
    if (window <= 0 || num_samples < 0 || num_samples > ((int64_t)1 << 50)) return -1;
    return cdiv64(num_samples, window);
}

int sc_vad_probs(const float* d_wav, int32_t n, int64_t wav_stride, const int64_t* h_num_samples, int32_t window, const sc_vad_opts* opts,
                 float* d_probs, int64_t probs_stride, float* d_db, float* h_stats) {
    SC_API_BEGIN
    // every argument check comes before the first device call
    const VadParams p = checked_vad_opts(opts);
    SC_CHECK(d_wav && h_num_samples && d_probs, "sc_vad_probs: null argument");
    SC_CHECK(window >= VAD_MIN_WINDOW && window <= VAD_MAX_WINDOW, "sc_vad_probs: window %d is outside the limit %d..%d", window, VAD_MIN_WINDOW,
             VAD_MAX_WINDOW);
    SC_CHECK(n >= 1 && n <= 65535, "sc_vad_probs: %d rows, the limit is 1..65535", n);
    SC_CHECK(wav_stride >= 0 && probs_stride >= 0, "sc_vad_probs: negative stride");
    int64_t most = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t L = h_num_samples[i];
        SC_CHECK(L >= 0 && L <= wav_stride, "sc_vad_probs: row %d has %lld samples, wav_stride is %lld", i, (long long)L, (long long)wav_stride);
        const int64_t nw = cdiv64(L, window);
        SC_CHECK(nw <= VAD_MAX_WINDOWS, "sc_vad_probs: row %d has %lld windows, the limit is %lld", i, (long long)nw, (long long)VAD_MAX_WINDOWS);
        most = std::max(most, nw);
    }
    SC_CHECK(probs_stride >= most, "sc_vad_probs: probs_stride %lld is below the most windows of a row, %lld", (long long)probs_stride, (long long)most);
    if (probs_stride == 0) {  // no window anywhere and nothing to clear
        if (h_stats)
            for (int i = 0; i < n; ++i) h_stats[4 * i] = h_stats[4 * i + 1] = h_stats[4 * i + 2] = std::nanf(""), h_stats[4 * i + 3] = 0.f;
        return SC_OK;
    }
    int device = 0;
    SC_HIP(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(g_vad_mutex);
    const int64_t scratch_stride = std::max<int64_t>(most, 1);
    VadDevice& dv = vad_device_state(device, n, d_db ? 0 : (size_t)n * scratch_stride);
    float* db = d_db ? d_db : dv.d_db;
    const int64_t db_stride = d_db ? probs_stride : scratch_stride;
    hipStream_t stream = nullptr;  // the default stream, like sc_resample: ordered behind the caller's work on it
    SC_HIP(hipMemcpyAsync(dv.d_len, h_num_samples, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, stream));
    if (most > 0) {
        const dim3 grid((unsigned)cdiv64(most, VAD_WAVES), (unsigned)n);
        launch_energy_for(window, grid, stream, d_wav, wav_stride, dv.d_len, db, db_stride);
        SC_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(vad_prob_kernel, dim3((unsigned)n), dim3(VAD_THREADS), 0, stream, db, db_stride, d_db ? 1 : 0, dv.d_len, window, p, d_probs,
                       probs_stride, dv.d_stats);
    SC_LAUNCH_CHECK();
    if (h_stats) SC_HIP(hipMemcpyAsync(h_stats, dv.d_stats, (size_t)n * 4 * sizeof(float), hipMemcpyDeviceToHost, stream));
    SC_HIP(hipStreamSynchronize(stream));
    SC_API_END
}

int sc_vad_stream_create(int32_t sessions, int32_t window, const sc_vad_stream_opts* opts, sc_vad_stream** out) {
    SC_API_BEGIN
    SC_CHECK(out, "sc_vad_stream_create: null argument");
    *out = nullptr;
    SC_CHECK(sessions >= 1 && sessions <= 65535, "sc_vad_stream_create: %d sessions, the limit is 1..65535", sessions);
    SC_CHECK(window >= 1 && window <= VAD_MAX_WINDOW, "sc_vad_stream_create: window %d is outside the limit 1..%d", window, VAD_MAX_WINDOW);
    int history = VAD_STREAM_DEFAULT_HISTORY;
    VadParams p;
    static const sc_vad_stream_opts zero{};
    if (opts && std::memcmp(opts, &zero, sizeof(zero)) != 0) {
        SC_CHECK(opts->abi_version == SC_ABI_VERSION, "sc_vad_stream_create: options ABI version %d != library %d", opts->abi_version, SC_ABI_VERSION);
        const sc_vad_opts base{opts->abi_version, opts->hangover,      opts->floor_quantile, opts->peak_quantile, opts->noise_ceiling_db,
                               opts->min_margin_db, opts->range_fraction, opts->slope_db};
        p = checked_vad_opts(&base, "sc_vad_stream_create");
        SC_CHECK(opts->history_windows >= 0 && opts->history_windows <= VAD_STREAM_MAX_HISTORY,
                 "sc_vad_stream_create: history_windows %d is outside the limit 1..%d (0 stands for the default)", opts->history_windows,
                 VAD_STREAM_MAX_HISTORY);
        if (opts->history_windows != 0) history = opts->history_windows;
    }
    sc_vad_stream* h = new sc_vad_stream();
    h->sessions = sessions, h->window = window, h->history = history, h->p = p;
    *out = h;
    SC_API_END
}

void sc_vad_stream_destroy(sc_vad_stream* h) {
    if (!h) return;
    if (h->device >= 0) {
        int cur = 0;
        const bool swap = hipGetDevice(&cur) == hipSuccess && cur != h->device && hipSetDevice(h->device) == hipSuccess;
        for (void* p : {(void*)h->st.ring, (void*)h->st.recent, (void*)h->st.last, (void*)h->st.count, (void*)h->d_len, (void*)h->d_stats, (void*)h->d_db})
            if (p) (void)hipFree(p);
        if (swap) (void)hipSetDevice(cur);
    }
    delete h;
}

int sc_vad_stream_reset(sc_vad_stream* h, const int32_t* sids, int32_t n) {
    SC_API_BEGIN
    SC_CHECK(h, "sc_vad_stream_reset: null argument");
    std::lock_guard<std::mutex> lock(h->mutex);
    check_lanes(*h, "sc_vad_stream_reset", sids, n);
    if (n == 0) return SC_OK;
    const bool fresh = h->device < 0;
    vad_stream_on_device(*h);
    hipStream_t stream = nullptr;
    if (!fresh) {  // a handle that has just come to the device holds fresh lanes only
        int32_t* d_lanes = reinterpret_cast<int32_t*>(h->d_len + h->sessions);
        SC_HIP(hipMemcpyAsync(d_lanes, sids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(vad_stream_reset_kernel, dim3((unsigned)n), dim3(VAD_THREADS), 0, stream, h->st, h->history, (const int32_t*)d_lanes);
        SC_LAUNCH_CHECK();
    }
    SC_HIP(hipStreamSynchronize(stream));
    SC_API_END
}

int sc_vad_stream_push(sc_vad_stream* h, const int32_t* sids, int32_t n, const float* d_wav, int64_t wav_stride, const int64_t* h_num_samples,
                       float* d_probs, int64_t probs_stride, float* d_db, float* h_stats) {
    SC_API_BEGIN
    // every argument check comes before the first device call
    SC_CHECK(h, "sc_vad_stream_push: null argument");
    std::lock_guard<std::mutex> lock(h->mutex);
    check_lanes(*h, "sc_vad_stream_push", sids, n);
    if (n == 0) return SC_OK;
    SC_CHECK(h_num_samples, "sc_vad_stream_push: null argument");
    SC_CHECK(wav_stride >= 0 && probs_stride >= 0, "sc_vad_stream_push: negative stride");
    const int W = h->window;
    int64_t most = 0;
    h->h_meta.assign((size_t)n + ((size_t)n + 1) / 2, 0);
    for (int i = 0; i < n; ++i) {
        const int64_t L = h_num_samples[i];
        SC_CHECK(L >= 0, "sc_vad_stream_push: lane %d has a negative length %lld", sids[i], (long long)L);
        SC_CHECK(L <= wav_stride, "sc_vad_stream_push: lane %d has %lld samples, wav_stride is %lld", sids[i], (long long)L, (long long)wav_stride);
        const int64_t nw = L / W;  // the samples behind the last whole window are not heard
        SC_CHECK(nw <= VAD_MAX_WINDOWS, "sc_vad_stream_push: lane %d has %lld windows, the limit is %lld", sids[i], (long long)nw, (long long)VAD_MAX_WINDOWS);
        h->h_meta[i] = nw * W;
        most = std::max(most, nw);
    }
    SC_CHECK(probs_stride >= most, "sc_vad_stream_push: probs_stride %lld is below the most windows of a lane, %lld", (long long)probs_stride,
             (long long)most);
    SC_CHECK(most == 0 || (d_wav && d_probs), "sc_vad_stream_push: null argument");
    std::memcpy(reinterpret_cast<char*>(h->h_meta.data()) + (size_t)n * sizeof(int64_t), sids, (size_t)n * sizeof(int32_t));
    vad_stream_on_device(*h);
    hipStream_t stream = nullptr;  // the default stream, like sc_vad_probs
    const int64_t scratch_stride = std::max<int64_t>(most, 1);
    if (!d_db && h->db_floats < (size_t)n * scratch_stride) {
        if (h->d_db) (void)hipFree(h->d_db);
        h->d_db = nullptr, h->db_floats = 0;
        const size_t want = std::max<size_t>((size_t)n * scratch_stride, (size_t)h->sessions * 16);
        SC_HIP(hipMalloc(reinterpret_cast<void**>(&h->d_db), want * sizeof(float)));
        h->db_floats = want;
    }
    float* db = d_db ? d_db : h->d_db;
    const int64_t db_stride = d_db ? probs_stride : scratch_stride;
    // lengths and lanes in one copy: the lanes of this call sit right behind its n lengths
    SC_HIP(hipMemcpyAsync(h->d_len, h->h_meta.data(), (size_t)n * (sizeof(int64_t) + sizeof(int32_t)), hipMemcpyHostToDevice, stream));
    const int32_t* d_lanes = reinterpret_cast<const int32_t*>(h->d_len + n);
    if (most > 0) {
        launch_energy_for(W, dim3((unsigned)cdiv64(most, VAD_WAVES), (unsigned)n), stream, d_wav, wav_stride, h->d_len, db, db_stride);
        SC_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(vad_stream_kernel, dim3((unsigned)n), dim3(VAD_THREADS), 0, stream, db, db_stride, h->d_len, d_lanes, W, h->history, h->p, h->st,
                       d_probs, probs_stride, h->d_stats);
    SC_LAUNCH_CHECK();
    if (h_stats) SC_HIP(hipMemcpyAsync(h_stats, h->d_stats, (size_t)n * VAD_STREAM_STATS * sizeof(float), hipMemcpyDeviceToHost, stream));
    SC_HIP(hipStreamSynchronize(stream));
    SC_API_END
}

}  // extern "C"
