// Windowed-sinc polyphase resampler (the algorithm of torchaudio.functional.resample, restated: DESIGN.md section 7h), the
// step the reference runs on the host in front of every model that opens a file (cli/m4t/predict/predict.py:226-231,
// cli/expressivity/predict/predict.py:115, models/aligner/alignment_extractor.py:63-71).
//
// Host: the filter bank of a reduced rate pair orig:new, built in double and rounded to fp32; phase p keeps only its
// contiguous support [k0[p], k0[p] + cnt[p]) of the 2 * width + orig taps (the taps outside |t| < lpw are zero here).
// Device: one thread per output sample, fp32 fmaf in ascending tap order, so an output depends on its own row's samples only.
// A 256-thread workgroup owns F whole frames of one row (F * new consecutive outputs) and stages their input span
// (F * orig + 2 * width samples, zeros outside [0, L)) and the bank in LDS.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <list>
#include <mutex>
#include <numeric>
#include <vector>

#include "handle.h"

namespace sc {

static constexpr int RS_THREADS = 256;
static constexpr int RS_MAX_RATE = 1024;                // orig and new after reduction
static constexpr size_t RS_MAX_BANK_BYTES = 64 * 1024;  // new * S * 4
static constexpr size_t RS_LDS_TWO = 72 * 1024;         // LDS of a workgroup when two share a CU (160 KiB)
static constexpr size_t RS_LDS_ONE = 152 * 1024;        // one workgroup per CU
static constexpr int RS_TILE_OUTPUTS = 2048;            // outputs of a tile where the ratio and the LDS budget allow
static constexpr double RS_DEFAULT_BETA = 14.769656459379492;
static constexpr double RS_DEFAULT_ROLLOFF = 0.99;

struct ResampleOpts {
    int lpw = 6;
    double rolloff = RS_DEFAULT_ROLLOFF;
    int method = 0;  // 0 hann, 1 kaiser
    double beta = RS_DEFAULT_BETA;
};

struct ResampleBank {
    int orig = 0, nw = 0;  // reduced rates
    int width = 0, S = 0;
    std::vector<int32_t> k0, cnt;  // [new]
    std::vector<float> taps;       // [new][S], zero behind cnt[p]
    // the tile of the kernel
    int F = 0, span = 0;  // frames per workgroup, floats of the staged span (multiple of 4)
    size_t lds = 0;
};

// modified Bessel function of the first kind, order 0: sum_k ((x/2)^k / k!)^2, every term positive
static double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

// the checks of the rate pair and the options; `who` names the entry in the message
static ResampleOpts checked_opts(const char* who, int32_t orig_freq, int32_t new_freq, const sc_resample_opts* o) {
    SC_CHECK(orig_freq > 0 && new_freq > 0, "%s: sample rates must be positive (got %d -> %d)", who, orig_freq, new_freq);
    ResampleOpts r;
    static const sc_resample_opts zero{};
    if (!o || std::memcmp(o, &zero, sizeof(zero)) == 0) return r;
    SC_CHECK(o->abi_version == SC_ABI_VERSION, "%s: options ABI version %d != library %d", who, o->abi_version, SC_ABI_VERSION);
    SC_CHECK(o->lowpass_filter_width >= 1, "%s: lowpass_filter_width %d is below the limit of 1", who, o->lowpass_filter_width);
    SC_CHECK(o->rolloff > 0.f && o->rolloff <= 1.f, "%s: rolloff %g is outside the limit (0, 1]", who, (double)o->rolloff);
    SC_CHECK(o->method == 0 || o->method == 1, "%s: unknown method %d (0 hann, 1 kaiser)", who, o->method);
    SC_CHECK(o->beta >= 0.f && std::isfinite(o->beta), "%s: beta %g must be finite and not negative", who, (double)o->beta);
    r.lpw = o->lowpass_filter_width;
    // the struct carries rolloff and beta as fp32: a field that holds its default rounded to fp32 stands for the default itself
    r.rolloff = o->rolloff == (float)RS_DEFAULT_ROLLOFF ? RS_DEFAULT_ROLLOFF : (double)o->rolloff;
    r.method = o->method;
    if (o->beta > 0.f && o->beta != (float)RS_DEFAULT_BETA) r.beta = (double)o->beta;
    return r;
}

static void build_bank(const char* who, int32_t orig_freq, int32_t new_freq, const ResampleOpts& o, ResampleBank& b) {
    const int g = std::gcd(orig_freq, new_freq);
    const int orig = orig_freq / g, nw = new_freq / g;
    b.orig = orig;
    b.nw = nw;
    if (orig == nw) return;  // a copy: no bank
    SC_CHECK(orig <= RS_MAX_RATE && nw <= RS_MAX_RATE, "%s: %d -> %d reduces to %d:%d, above the limit of %d per side", who, orig_freq,
             new_freq, orig, nw, RS_MAX_RATE);
    const double lpw = (double)o.lpw;
    const double base = (double)std::min(orig, nw) * o.rolloff;
    const double wd = std::ceil(lpw * (double)orig / base);
    // every phase keeps about 2 * width taps: refuse before anything of that size is allocated
    SC_CHECK(wd * 2.0 * nw * 4.0 <= 4.0 * (double)RS_MAX_BANK_BYTES, "%s: the filter bank of %d:%d at width %d is above the limit of %zu bytes",
             who, orig, nw, o.lpw, RS_MAX_BANK_BYTES);
    const int width = (int)wd;
    const int K = 2 * width + orig;
    const double scale = base / (double)orig;
    const double i0_beta = o.method == 1 ? bessel_i0(o.beta) : 1.0;
    std::vector<float> full((size_t)nw * K);
    b.k0.assign(nw, 0);
    b.cnt.assign(nw, 0);
    int longest = 0;
    for (int p = 0; p < nw; ++p) {
        int first = -1, last = -1;
        for (int k = 0; k < K; ++k) {
            double t = (-(double)p / (double)nw + ((double)k - (double)width) / (double)orig) * base;
            const bool inside = std::fabs(t) < lpw;
            t = std::min(std::max(t, -lpw), lpw);
            double w;
            if (o.method == 0) {
                const double c = std::cos(t * M_PI / lpw / 2.0);
                w = c * c;
            } else {
                const double r = t / lpw;
                w = bessel_i0(o.beta * std::sqrt(1.0 - r * r)) / i0_beta;
            }
            const double x = t * M_PI;
            const double sinc = x == 0.0 ? 1.0 : std::sin(x) / x;
            full[(size_t)p * K + k] = inside ? (float)(sinc * w * scale) : 0.f;
            if (inside) {
                if (first < 0) first = k;
                last = k;
            }
        }
        SC_CHECK(first >= 0, "%s: phase %d of %d:%d has no tap", who, p, orig, nw);
        b.k0[p] = first;
        b.cnt[p] = last - first + 1;
        longest = std::max(longest, b.cnt[p]);
    }
    b.width = width;
    b.S = (longest + 3) / 4 * 4;
    const size_t bank_bytes = (size_t)nw * b.S * sizeof(float);
    SC_CHECK(bank_bytes <= RS_MAX_BANK_BYTES, "%s: the filter bank of %d:%d (%d phases x %d taps, %zu bytes) is above the limit of %zu bytes", who,
             orig, nw, nw, b.S, bank_bytes, RS_MAX_BANK_BYTES);
    b.taps.assign((size_t)nw * b.S, 0.f);
    for (int p = 0; p < nw; ++p)
        for (int s = 0; s < b.cnt[p]; ++s) b.taps[(size_t)p * b.S + s] = full[(size_t)p * K + b.k0[p] + s];
    // the tile: F whole frames, about RS_TILE_OUTPUTS outputs, span + bank inside the LDS share of two workgroups per CU where one
    // frame fits there, inside one workgroup's LDS otherwise
    const size_t fixed = bank_bytes + (size_t)nw * 2 * sizeof(int32_t);
    auto span_of = [&](int F) { return ((int64_t)F * orig + 2 * width + 3 + 3) / 4 * 4; };  // + 3: the shift to a 16-byte aligned source
    int F = std::max(1, RS_TILE_OUTPUTS / nw);
    while (F > 1 && fixed + (size_t)span_of(F) * sizeof(float) > RS_LDS_TWO) F = std::max(1, F / 2);
    b.F = F;
    b.span = (int)span_of(F);
    b.lds = fixed + (size_t)b.span * sizeof(float);
    SC_CHECK(b.lds <= RS_LDS_ONE, "%s: one frame of %d:%d needs %zu bytes of LDS, above the limit of %zu", who, orig, nw, b.lds, RS_LDS_ONE);
}

static int64_t resample_len(int64_t L, int orig, int nw) { return (L * nw + orig - 1) / orig; }

// ---- kernels ----------------------------------------------------------------------------------------------------------------

// d_bank: tapsT [S][new] floats (phase-adjacent lanes read adjacent LDS banks) | k0 [new] | cnt [new]
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const float* __restrict__ in, int64_t in_stride, const int64_t* __restrict__ in_len,
                                                              float* __restrict__ out, int64_t out_stride, const float* __restrict__ d_bank, int orig,
                                                              int nw, int width, int S, int F, int span) {
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    float* s_x = s_mem;                // [span]
    float* s_taps = s_mem + span;      // [S][new]
    int* s_k0 = reinterpret_cast<int*>(s_taps + (size_t)S * nw);
    int* s_cnt = s_k0 + nw;
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.y;
    const int64_t L = in_len[row];
    const int64_t out_len = (L * nw + orig - 1) / orig;
    const int tile_out = F * nw;
    const int64_t o0 = (int64_t)blockIdx.x * tile_out;
    float* orow = out + row * out_stride;
    const int64_t left = out_stride - o0;
    const int n_here = left < tile_out ? (int)left : tile_out;  // outputs of this tile inside the row's stride
    if (o0 >= out_len) {  // the row's zero tail
        for (int j = tid; j < n_here; j += RS_THREADS) orow[o0 + j] = 0.f;
        return;
    }
    const int bank_words = S * nw + 2 * nw;
    const int* bank_i = reinterpret_cast<const int*>(d_bank);
    int* s_bank_i = reinterpret_cast<int*>(s_taps);
    for (int i = tid; i < bank_words; i += RS_THREADS) s_bank_i[i] = bank_i[i];
    // span: s_x[shift + i] = x[g0 + i] for i in [0, F * orig + 2 * width), zero outside [0, L).  Staged from g0 - shift, where the
    // source is 16-byte aligned, in groups of four: a group inside [0, L) is one vector load, the others go sample by sample.
    const float* xrow = in + row * in_stride;
    const int64_t g0 = (int64_t)blockIdx.x * F * orig - width;
    const int shift = (int)(((reinterpret_cast<uintptr_t>(xrow) >> 2) + (uintptr_t)(g0 & 3)) & 3);
    const int64_t ga = g0 - shift;
    for (int q = tid; q < span / 4; q += RS_THREADS) {
        const int64_t g = ga + 4 * (int64_t)q;
        float4 v;
        if (g >= 0 && g + 3 < L) {
            v = *reinterpret_cast<const float4*>(xrow + g);
        } else {
            v.x = (g >= 0 && g < L) ? xrow[g] : 0.f;
            v.y = (g + 1 >= 0 && g + 1 < L) ? xrow[g + 1] : 0.f;
            v.z = (g + 2 >= 0 && g + 2 < L) ? xrow[g + 2] : 0.f;
            v.w = (g + 3 >= 0 && g + 3 < L) ? xrow[g + 3] : 0.f;
        }
        *reinterpret_cast<float4*>(s_x + 4 * q) = v;
    }
    __syncthreads();
    for (int j = tid; j < n_here; j += RS_THREADS) {
        float acc = 0.f;
        if (o0 + j < out_len) {
            const int f = j / nw;
            const int p = j - f * nw;
            const float* x = s_x + shift + f * orig + s_k0[p];
            const float* h = s_taps + p;
            const int c = s_cnt[p];
            for (int s = 0; s < c; ++s) acc = fmaf(h[(size_t)s * nw], x[s], acc);
        }
        orow[o0 + j] = acc;
    }
}

// orig == new: the row with its zero tail
__global__ __launch_bounds__(RS_THREADS) void resample_copy_kernel(const float* __restrict__ in, int64_t in_stride, const int64_t* __restrict__ in_len,
                                                                   float* __restrict__ out, int64_t out_stride) {
    const int64_t row = blockIdx.y;
    const int64_t L = in_len[row];
    const float* xrow = in + row * in_stride;
    float* orow = out + row * out_stride;
    for (int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x; i < out_stride; i += (int64_t)gridDim.x * RS_THREADS)
        orow[i] = i < L ? xrow[i] : 0.f;
}

// ---- the process-wide cache: banks per (orig, new, options) with their device copies, one length buffer per device -----------

struct ResampleEntry {
    int orig_freq, new_freq;
    ResampleOpts o;
    ResampleBank b;
    std::vector<std::pair<int, float*>> dev;  // (device, bank on it)
};
struct ResampleDevice {
    int device;
    int64_t* d_len = nullptr;
    size_t cap = 0;
    bool attr_set = false;
};
static std::mutex g_rs_mutex;
static std::list<ResampleEntry> g_rs_cache;  // most recently used first
static std::list<ResampleDevice> g_rs_devices;
static constexpr size_t RS_CACHE_ENTRIES = 16;

static bool same_opts(const ResampleOpts& a, const ResampleOpts& b) {
    return a.lpw == b.lpw && a.rolloff == b.rolloff && a.method == b.method && (a.method == 0 || a.beta == b.beta);
}

// g_rs_mutex held.  Host work only: the limits of the bank are checked here, before any device call.
static ResampleEntry& cached_bank(int32_t orig_freq, int32_t new_freq, const ResampleOpts& o) {
    for (auto it = g_rs_cache.begin(); it != g_rs_cache.end(); ++it)
        if (it->orig_freq == orig_freq && it->new_freq == new_freq && same_opts(it->o, o)) {
            g_rs_cache.splice(g_rs_cache.begin(), g_rs_cache, it);
            return g_rs_cache.front();
        }
    ResampleEntry e;
    e.orig_freq = orig_freq;
    e.new_freq = new_freq;
    e.o = o;
    build_bank("sc_resample", orig_freq, new_freq, o, e.b);
    if (g_rs_cache.size() >= RS_CACHE_ENTRIES) {  // nothing is in flight: every call synchronises under the mutex
        int cur = 0;
        const bool have_cur = !g_rs_cache.back().dev.empty() && hipGetDevice(&cur) == hipSuccess;
        for (auto& d : g_rs_cache.back().dev) {
            (void)hipSetDevice(d.first);
            (void)hipFree(d.second);
        }
        if (have_cur) (void)hipSetDevice(cur);
        g_rs_cache.pop_back();
    }
    g_rs_cache.push_front(std::move(e));
    return g_rs_cache.front();
}

// g_rs_mutex held: the bank on `device` (the current one) as tapsT [S][new] | k0 [new] | cnt [new]
static const float* device_bank(ResampleEntry& e, int device) {
    for (auto& d : e.dev)
        if (d.first == device) return d.second;
    const ResampleBank& b = e.b;
    std::vector<int32_t> words((size_t)b.S * b.nw + 2 * b.nw);
    for (int p = 0; p < b.nw; ++p)
        for (int s = 0; s < b.S; ++s) std::memcpy(&words[(size_t)s * b.nw + p], &b.taps[(size_t)p * b.S + s], 4);
    std::copy(b.k0.begin(), b.k0.end(), words.begin() + (size_t)b.S * b.nw);
    std::copy(b.cnt.begin(), b.cnt.end(), words.begin() + (size_t)b.S * b.nw + b.nw);
    float* d_bank = nullptr;
    SC_HIP(hipMalloc(reinterpret_cast<void**>(&d_bank), words.size() * 4));
    const hipError_t err = hipMemcpy(d_bank, words.data(), words.size() * 4, hipMemcpyHostToDevice);
    if (err != hipSuccess) {
        (void)hipFree(d_bank);
        SC_HIP(err);
    }
    e.dev.emplace_back(device, d_bank);
    return d_bank;
}

// g_rs_mutex held
static ResampleDevice& device_state(int device, size_t n) {
    ResampleDevice* l = nullptr;
    for (auto& x : g_rs_devices)
        if (x.device == device) l = &x;
    if (!l) {
        g_rs_devices.push_back(ResampleDevice{device});
        l = &g_rs_devices.back();
    }
    if (l->cap < n) {
        if (l->d_len) (void)hipFree(l->d_len);
        l->d_len = nullptr;
        l->cap = 0;
        const size_t cap = std::max<size_t>(n, 64);
        SC_HIP(hipMalloc(reinterpret_cast<void**>(&l->d_len), cap * sizeof(int64_t)));
        l->cap = cap;
    }
    return *l;
}

}  // namespace sc

using namespace sc;

extern "C" {

int64_t sc_resample_len(int64_t num_samples, int32_t orig_freq, int32_t new_freq) {
    if (orig_freq <= 0 || new_freq <= 0 || num_samples < 0 || num_samples > ((int64_t)1 << 50)) return -1;
    const int g = std::gcd(orig_freq, new_freq);
    return resample_len(num_samples, orig_freq / g, new_freq / g);
}

int sc_op_resample_bank(int32_t orig_freq, int32_t new_freq, const sc_resample_opts* opts, int32_t* width, int32_t* S, int32_t* h_k0,
                        float* h_taps, int64_t cap) {
    SC_API_BEGIN
    const ResampleOpts o = checked_opts("sc_op_resample_bank", orig_freq, new_freq, opts);
    ResampleBank b;
    build_bank("sc_op_resample_bank", orig_freq, new_freq, o, b);
    if (width) *width = b.width;
    if (S) *S = b.S;
    if (h_k0 || h_taps) {
        SC_CHECK(h_k0 && h_taps, "sc_op_resample_bank: h_k0 and h_taps go together");
        if (cap < (int64_t)b.nw * b.S) {
            set_error("sc_op_resample_bank: %d phases x %d taps need %lld floats, cap is %lld", b.nw, b.S, (long long)b.nw * b.S, (long long)cap);
            throw Error{SC_ERR_CAPACITY};
        }
        std::copy(b.k0.begin(), b.k0.end(), h_k0);
        std::copy(b.taps.begin(), b.taps.end(), h_taps);
    }
    SC_API_END
}

int sc_op_resample_plan(int32_t orig_freq, int32_t new_freq, const sc_resample_opts* opts, int32_t* h_plan6) {
    SC_API_BEGIN
    SC_CHECK(h_plan6, "sc_op_resample_plan: null argument");
    const ResampleOpts o = checked_opts("sc_op_resample_plan", orig_freq, new_freq, opts);
    ResampleBank b;
    build_bank("sc_op_resample_plan", orig_freq, new_freq, o, b);
    h_plan6[0] = b.orig;
    h_plan6[1] = b.nw;
    h_plan6[2] = b.F;
    h_plan6[3] = b.F * b.nw;
    h_plan6[4] = b.F * b.orig;
    h_plan6[5] = (int32_t)b.lds;
    SC_API_END
}

int sc_resample(const float* d_in, int32_t n, int64_t in_stride, const int64_t* h_in_len, int32_t orig_freq, int32_t new_freq,
                const sc_resample_opts* opts, float* d_out, int64_t out_stride, int64_t* h_out_len) {
    SC_API_BEGIN
    // every argument check comes before the first device call
    const ResampleOpts o = checked_opts("sc_resample", orig_freq, new_freq, opts);
    SC_CHECK(d_in && h_in_len && d_out && h_out_len, "sc_resample: null argument");
    std::lock_guard<std::mutex> lock(g_rs_mutex);
    ResampleEntry& e = cached_bank(orig_freq, new_freq, o);  // the limits of the bank: still no device call
    SC_CHECK(n >= 1 && n <= 65535, "sc_resample: %d rows, the limit is 1..65535", n);
    SC_CHECK(in_stride >= 0 && out_stride >= 0, "sc_resample: negative stride");
    const int g = std::gcd(orig_freq, new_freq);
    const int orig = orig_freq / g, nw = new_freq / g;
    std::vector<int64_t> out_len(n);
    int64_t longest = 0;
    for (int i = 0; i < n; ++i) {
        SC_CHECK(h_in_len[i] >= 0 && h_in_len[i] <= in_stride && h_in_len[i] <= ((int64_t)1 << 50),
                 "sc_resample: row %d has %lld samples, in_stride is %lld", i, (long long)h_in_len[i], (long long)in_stride);
        out_len[i] = resample_len(h_in_len[i], orig, nw);
        longest = std::max(longest, out_len[i]);
    }
    SC_CHECK(out_stride >= longest, "sc_resample: out_stride %lld is below the longest out_len %lld", (long long)out_stride, (long long)longest);
    {
        const char* ib = reinterpret_cast<const char*>(d_in);
        const char* ob = reinterpret_cast<const char*>(d_out);
        const int64_t in_bytes = ((int64_t)(n - 1) * in_stride + in_stride) * 4, out_bytes = (int64_t)n * out_stride * 4;
        SC_CHECK(ob + out_bytes <= ib || ib + in_bytes <= ob, "sc_resample: d_out overlaps d_in");
    }
    std::copy(out_len.begin(), out_len.end(), h_out_len);
    if (out_stride == 0) return SC_OK;
    int device = 0;
    SC_HIP(hipGetDevice(&device));
    ResampleDevice& dv = device_state(device, n);
    hipStream_t stream = nullptr;  // the default stream, like the sc_op_* entries: ordered behind the caller's work on it
    SC_HIP(hipMemcpyAsync(dv.d_len, h_in_len, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, stream));
    if (orig == nw) {
        const int64_t blocks = std::min<int64_t>(cdiv64(out_stride, RS_THREADS), 2048);
        hipLaunchKernelGGL(resample_copy_kernel, dim3((unsigned)blocks, n), dim3(RS_THREADS), 0, stream, d_in, in_stride, dv.d_len, d_out, out_stride);
    } else {
        const ResampleBank& b = e.b;
        const int64_t tiles = cdiv64(out_stride, (int64_t)b.F * b.nw);
        SC_CHECK(tiles <= 0x7fffffff, "sc_resample: out_stride %lld needs %lld tiles", (long long)out_stride, (long long)tiles);
        const float* d_bank = device_bank(e, device);
        if (!dv.attr_set) {
            SC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&resample_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)RS_LDS_ONE));
            dv.attr_set = true;
        }
        hipLaunchKernelGGL(resample_kernel, dim3((unsigned)tiles, n), dim3(RS_THREADS), b.lds, stream, d_in, in_stride, dv.d_len, d_out, out_stride,
                           d_bank, b.orig, b.nw, b.width, b.S, b.F, b.span);
    }
    SC_LAUNCH_CHECK();
    SC_HIP(hipStreamSynchronize(stream));
    SC_API_END
}

}  // extern "C"
