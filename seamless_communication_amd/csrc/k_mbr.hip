// Minimum-Bayes-risk selection over sampled hypotheses (sc_mbr_select): the token n-gram F-score of every
// pair of hypotheses of an utterance, the expected utility of each hypothesis and the arg-max.  No weights, no handle.
//
// An n-gram is compared as the tuple of its tokens, never as a packed or hashed key; the sorted-tuple counting is seq_match.h at
// tuple width 4 (sc_ngram_match of k_metrics.hip is the same code at width 6).
// Pass A, one workgroup per hypothesis: the tuples, a bitonic sort in LDS, and per sorted slot and order the number of times the
// n-gram occurs where the slot is the first of its run (0 elsewhere).  Both go to scratch, hypothesis after hypothesis.
// Pass B, one workgroup per (utterance, i): row i's tuples and counts in LDS, one wavefront per j; a lane takes a slot of i, finds
// the first slot of j that is not below it in the first n components (binary search) and adds min(count_i, count_j); integer
// sums over the lanes give m_1..m_4.
// Pass C, one workgroup per utterance, thread i: U(h_i, h_j) in double for ascending j, the weighted sum, E_i; thread 0 takes the
// first maximum.  Every sum has one order and the counts are integers: an utterance's bits depend on its own hypotheses only, and
// two equal hypotheses get equal rows.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <list>
#include <mutex>
#include <vector>

#include "device_util.h"
#include "handle.h"
#include "seq_match.h"

namespace sc {

static constexpr int MBR_THREADS = 256;
static constexpr int MBR_WAVES = MBR_THREADS / 64;
static constexpr int MBR_MAX_N = 4096, MBR_MAX_HYPS = 128, MBR_MAX_LEN = 1024, MBR_MAX_ORDER = 4;
// one launch set covers consecutive utterances up to these sums (an utterance is never split: at most 128 x 1024 tokens and
// 128 x 128 pairs), so scratch stays below 200 MB whatever the call holds
static constexpr int64_t MBR_CHUNK_TOKENS = (int64_t)1 << 22, MBR_CHUNK_PAIRS = (int64_t)1 << 21;
using MbrTuple = SeqTuple<MBR_MAX_ORDER>;
using MbrCounts = SeqCounts<MBR_MAX_ORDER, uint32_t>;

struct MbrHyp {  // one hypothesis of a chunk
    uint32_t off;  // first token / first sorted slot
    int32_t len;
    int32_t utt;   // utterance within the chunk
    int32_t idx;   // hypothesis within the utterance
};
struct MbrUtt {
    int32_t first;      // its first MbrHyp
    int32_t num;        // hypotheses
    uint32_t pair_off;  // its num x num block of the pair arrays
    int32_t reserved;
};

// ---- pass A -------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(MBR_THREADS) void mbr_sort_kernel(const int32_t* __restrict__ tok, const MbrHyp* __restrict__ hyps,
                                                               MbrTuple* __restrict__ keys, MbrCounts* __restrict__ counts) {
    __shared__ MbrTuple s_key[MBR_MAX_LEN];
    const MbrHyp h = hyps[blockIdx.x];
    if (h.len == 0) return;  // 0..MBR_MAX_LEN, checked on the host
    seq_sort_count<MBR_MAX_ORDER, uint32_t>(tok + h.off, h.len, s_key, keys + h.off, counts + h.off);
}

// ---- pass B -------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(MBR_THREADS) void mbr_match_kernel(const MbrHyp* __restrict__ hyps, const MbrUtt* __restrict__ utts,
                                                                const MbrTuple* __restrict__ keys, const MbrCounts* __restrict__ counts,
                                                                int max_order, i32x4_t* __restrict__ match) {
    extern __shared__ MbrTuple s_row[];  // row i: len_i tuples, then len_i counts (the launch sizes it by the longest hypothesis)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const MbrHyp me = hyps[blockIdx.x];
    const MbrUtt u = utts[me.utt];
    const int Li = me.len;
    MbrCounts* s_cnt = reinterpret_cast<MbrCounts*>(s_row + Li);
    for (int p = tid; p < Li; p += MBR_THREADS) {
        s_row[p] = keys[me.off + p];
        s_cnt[p] = counts[me.off + p];
    }
    __syncthreads();
    for (int j = wave; j < u.num; j += MBR_WAVES) {  // the whole wavefront takes the same j
        const MbrHyp hj = hyps[u.first + j];
        int m[MBR_MAX_ORDER];
        seq_match_wave<MBR_MAX_ORDER, uint32_t>(s_row, s_cnt, Li, keys + hj.off, counts + hj.off, hj.len, max_order, lane, m);
        if (lane == 0) match[u.pair_off + (uint32_t)me.idx * (uint32_t)u.num + (uint32_t)j] = i32x4_t{m[0], m[1], m[2], m[3]};
    }
}

// ---- pass C -------------------------------------------------------------------------------------------------------------------

// from here on a product and a sum stay two roundings, as the definition writes them
#pragma clang fp contract(off)
__device__ double mbr_utility(const i32x4_t m, int len_h, int len_r, int max_order, double b2) {
    double sp = 0.0, sr = 0.0;
    int eff = 0;
#pragma unroll
    for (int c = 0; c < MBR_MAX_ORDER; ++c) {
        const int H = len_h - c, R = len_r - c;  // |h| - n + 1
        if (c < max_order && H > 0 && R > 0) {
            sp += (double)m[c] / (double)H;
            sr += (double)m[c] / (double)R;
            ++eff;
        }
    }
    if (eff == 0) return 0.0;
    const double P = sp / (double)eff, R = sr / (double)eff;
    const double den = b2 * P + R;
    if (den == 0.0) return 0.0;
    return (1.0 + b2) * P * R / den;
}

__global__ __launch_bounds__(MBR_MAX_HYPS) void mbr_expect_kernel(const MbrHyp* __restrict__ hyps, const MbrUtt* __restrict__ utts,
                                                                  const i32x4_t* __restrict__ match, const float* __restrict__ weights,
                                                                  int max_order, double b2, double* __restrict__ utility,
                                                                  double* __restrict__ expected, int32_t* __restrict__ best) {
    __shared__ double s_e[MBR_MAX_HYPS];
    const MbrUtt u = utts[blockIdx.x];
    const int i = threadIdx.x;
    if (i < u.num) {
        const int len_i = hyps[u.first + i].len;
        double acc = 0.0, wsum = 0.0;
        for (int j = 0; j < u.num; ++j) {
            const uint32_t at = u.pair_off + (uint32_t)i * (uint32_t)u.num + (uint32_t)j;
            const double U = mbr_utility(match[at], len_i, hyps[u.first + j].len, max_order, b2);
            const double w = (double)weights[u.first + j];
            utility[at] = U;
            acc += w * U;
            wsum += w;
        }
        const double e = acc / wsum;  // wsum > 0, checked on the host
        s_e[i] = e;
        expected[u.first + i] = e;
    }
    __syncthreads();
    if (i == 0) {
        int arg = 0;
        for (int k = 1; k < u.num; ++k)
            if (s_e[k] > s_e[arg]) arg = k;
        best[blockIdx.x] = arg;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

struct MbrParams {
    int max_order = MBR_MAX_ORDER;
    double b2 = 1.0;
};

// every check of the options; a zero field stands for its default
static MbrParams checked_mbr_opts(const sc_mbr_opts* o) {
    MbrParams r;
    static const sc_mbr_opts zero{};
    if (!o || std::memcmp(o, &zero, sizeof(zero)) == 0) return r;
    SC_CHECK(o->abi_version == SC_ABI_VERSION, "sc_mbr_select: options ABI version %d != library %d", o->abi_version, SC_ABI_VERSION);
    SC_CHECK(o->max_order >= 0 && o->max_order <= MBR_MAX_ORDER, "sc_mbr_select: max_order %d is outside the limit 0..%d", o->max_order, MBR_MAX_ORDER);
    SC_CHECK(std::isfinite(o->beta) && o->beta >= 0.f, "sc_mbr_select: beta %g is negative or not a number", (double)o->beta);
    if (o->max_order != 0) r.max_order = o->max_order;
    if (o->beta != 0.f) r.b2 = (double)o->beta * (double)o->beta;
    return r;
}

// per device: the buffers of one chunk
struct MbrDevice {
    int device;
    ScratchBuffer tok, hyps, utts, weights, keys, counts, match, utility, expected, best;
};
static std::mutex g_mbr_mutex;
static std::list<MbrDevice> g_mbr_devices;

// g_mbr_mutex held
static MbrDevice& mbr_device_state(int device) {
    for (auto& x : g_mbr_devices)
        if (x.device == device) return x;
    g_mbr_devices.push_back(MbrDevice{device});
    return g_mbr_devices.back();
}

}  // namespace sc

using namespace sc;

extern "C" {

int sc_mbr_select(const int32_t* h_ids, int32_t n, int32_t hyp_stride, int32_t len_stride, const int32_t* h_num_hyps, const int32_t* h_lens,
                  const float* h_weights_or_null, const sc_mbr_opts* opts, double* h_expected, int32_t* h_best, double* h_utility_or_null,
                  int32_t* h_match_or_null) {
    SC_API_BEGIN
    // every argument check comes before the first device call
    const MbrParams prm = checked_mbr_opts(opts);
    SC_CHECK(h_ids && h_num_hyps && h_lens && h_expected && h_best, "sc_mbr_select: null argument");
    SC_CHECK(n >= 1 && n <= MBR_MAX_N, "sc_mbr_select: %d utterances, the limit is 1..%d", n, MBR_MAX_N);
    SC_CHECK(hyp_stride >= 1 && hyp_stride <= MBR_MAX_HYPS, "sc_mbr_select: hyp_stride %d is outside the limit 1..%d", hyp_stride, MBR_MAX_HYPS);
    SC_CHECK(len_stride >= 1 && len_stride <= MBR_MAX_LEN, "sc_mbr_select: len_stride %d is outside the limit 1..%d", len_stride, MBR_MAX_LEN);
    const int64_t hs = hyp_stride, ls = len_stride;
    int longest = 0;
    for (int64_t u = 0; u < n; ++u) {
        const int N = h_num_hyps[u];
        SC_CHECK(N >= 1 && N <= hyp_stride, "sc_mbr_select: utterance %d has %d hypotheses, hyp_stride is %d", (int)u, N, hyp_stride);
        double wsum = 0.0;
        for (int64_t i = 0; i < N; ++i) {
            const int L = h_lens[u * hs + i];
            SC_CHECK(L >= 0 && L <= len_stride, "sc_mbr_select: utterance %d, hypothesis %d has %d tokens, len_stride is %d", (int)u, (int)i, L, len_stride);
            const int32_t* t = h_ids + (u * hs + i) * ls;
            for (int p = 0; p < L; ++p)
                SC_CHECK(t[p] >= 0, "sc_mbr_select: utterance %d, hypothesis %d holds the negative token %d", (int)u, (int)i, t[p]);
            longest = std::max(longest, L);
            if (h_weights_or_null) {
                const float w = h_weights_or_null[u * hs + i];
                SC_CHECK(std::isfinite(w) && w >= 0.f, "sc_mbr_select: utterance %d, weight %d is negative or not a number", (int)u, (int)i);
                wsum += (double)w;
            }
        }
        SC_CHECK(!h_weights_or_null || wsum > 0.0, "sc_mbr_select: the weights of utterance %d sum to 0", (int)u);
    }
    // what lies behind num_hyps is 0
    std::fill(h_expected, h_expected + n * hs, 0.0);
    if (h_utility_or_null) std::fill(h_utility_or_null, h_utility_or_null + n * hs * hs, 0.0);
    if (h_match_or_null) std::fill(h_match_or_null, h_match_or_null + n * hs * hs * MBR_MAX_ORDER, 0);

    int device = 0;
    SC_HIP(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(g_mbr_mutex);
    MbrDevice& dv = mbr_device_state(device);
    hipStream_t stream = nullptr;  // the default stream, like sc_resample: ordered behind the caller's work on it
    const size_t row_lds = (size_t)std::max(longest, 1) * (sizeof(MbrTuple) + sizeof(MbrCounts));  // at most 32 KB

    std::vector<int32_t> tok;
    std::vector<MbrHyp> hyps;
    std::vector<MbrUtt> utts;
    std::vector<float> weights;
    std::vector<i32x4_t> match;
    std::vector<double> utility, expected;
    std::vector<int32_t> best;
    for (int64_t u0 = 0; u0 < n;) {
        // the chunk [u0, u1): packed tokens, one descriptor per hypothesis and per utterance
        tok.clear(), hyps.clear(), utts.clear(), weights.clear();
        int64_t u1 = u0, pairs = 0;
        while (u1 < n) {
            const int N = h_num_hyps[u1];
            int64_t t = 0;
            for (int64_t i = 0; i < N; ++i) t += h_lens[u1 * hs + i];
            if (u1 > u0 && ((int64_t)tok.size() + t > MBR_CHUNK_TOKENS || pairs + (int64_t)N * N > MBR_CHUNK_PAIRS)) break;
            utts.push_back(MbrUtt{(int32_t)hyps.size(), N, (uint32_t)pairs, 0});
            for (int64_t i = 0; i < N; ++i) {
                const int L = h_lens[u1 * hs + i];
                hyps.push_back(MbrHyp{(uint32_t)tok.size(), L, (int32_t)(u1 - u0), (int32_t)i});
                const int32_t* t_i = h_ids + (u1 * hs + i) * ls;
                tok.insert(tok.end(), t_i, t_i + L);
                weights.push_back(h_weights_or_null ? h_weights_or_null[u1 * hs + i] : 1.f);
            }
            pairs += (int64_t)N * N;
            ++u1;
        }
        const size_t T = tok.size(), H = hyps.size(), U = utts.size(), Q = (size_t)pairs;
        int32_t* d_tok = dv.tok.grow<int32_t>(T);
        MbrHyp* d_hyps = dv.hyps.grow<MbrHyp>(H);
        MbrUtt* d_utts = dv.utts.grow<MbrUtt>(U);
        float* d_w = dv.weights.grow<float>(H);
        MbrTuple* d_keys = dv.keys.grow<MbrTuple>(T);
        MbrCounts* d_counts = dv.counts.grow<MbrCounts>(T);
        i32x4_t* d_match = dv.match.grow<i32x4_t>(Q);
        double* d_utility = dv.utility.grow<double>(Q);
        double* d_expected = dv.expected.grow<double>(H);
        int32_t* d_best = dv.best.grow<int32_t>(U);
        if (T) SC_HIP(hipMemcpyAsync(d_tok, tok.data(), T * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        SC_HIP(hipMemcpyAsync(d_hyps, hyps.data(), H * sizeof(MbrHyp), hipMemcpyHostToDevice, stream));
        SC_HIP(hipMemcpyAsync(d_utts, utts.data(), U * sizeof(MbrUtt), hipMemcpyHostToDevice, stream));
        SC_HIP(hipMemcpyAsync(d_w, weights.data(), H * sizeof(float), hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(mbr_sort_kernel, dim3((unsigned)H), dim3(MBR_THREADS), 0, stream, d_tok, d_hyps, d_keys, d_counts);
        SC_LAUNCH_CHECK();
        hipLaunchKernelGGL(mbr_match_kernel, dim3((unsigned)H), dim3(MBR_THREADS), row_lds, stream, d_hyps, d_utts, d_keys, d_counts, prm.max_order,
                           d_match);
        SC_LAUNCH_CHECK();
        hipLaunchKernelGGL(mbr_expect_kernel, dim3((unsigned)U), dim3(MBR_MAX_HYPS), 0, stream, d_hyps, d_utts, d_match, d_w, prm.max_order, prm.b2,
                           d_utility, d_expected, d_best);
        SC_LAUNCH_CHECK();
        expected.resize(H), best.resize(U);
        SC_HIP(hipMemcpyAsync(expected.data(), d_expected, H * sizeof(double), hipMemcpyDeviceToHost, stream));
        SC_HIP(hipMemcpyAsync(best.data(), d_best, U * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        if (h_utility_or_null) {
            utility.resize(Q);
            SC_HIP(hipMemcpyAsync(utility.data(), d_utility, Q * sizeof(double), hipMemcpyDeviceToHost, stream));
        }
        if (h_match_or_null) {
            match.resize(Q);
            SC_HIP(hipMemcpyAsync(match.data(), d_match, Q * sizeof(i32x4_t), hipMemcpyDeviceToHost, stream));
        }
        SC_HIP(hipStreamSynchronize(stream));
        for (size_t k = 0; k < U; ++k) {  // packed -> the caller's strides
            const MbrUtt& ut = utts[k];
            const int64_t u = u0 + (int64_t)k;
            h_best[u] = best[k];
            for (int64_t i = 0; i < ut.num; ++i) {
                h_expected[u * hs + i] = expected[ut.first + i];
                const size_t row = ut.pair_off + (size_t)i * ut.num;
                if (h_utility_or_null) std::copy(utility.begin() + row, utility.begin() + row + ut.num, h_utility_or_null + (u * hs + i) * hs);
                if (h_match_or_null) std::memcpy(h_match_or_null + (u * hs + i) * hs * MBR_MAX_ORDER, &match[row], (size_t)ut.num * sizeof(i32x4_t));
            }
        }
        u0 = u1;
    }
    SC_API_END
}

}  // extern "C"
