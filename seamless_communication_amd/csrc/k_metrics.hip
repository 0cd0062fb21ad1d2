// The two device primitives of the quality metrics (seamless_communication_amd/metrics.py): clipped n-gram
// match counts up to order 6 (sc_ngram_match: BLEU, chrF / chrF++, chrF as an MBR utility) and unit-cost Levenshtein distances
// (sc_edit_distance: WER / CER).  Both take a pool of int32 symbol sequences (packed symbols + int64 offsets) and a pair list into
// it; no weights, no handle, all pointers host memory, the default stream of the current device.
//
// sc_ngram_match is the sorted-tuple method of seq_match.h at tuple width 6 (k_mbr.hip is the same code at width 4):
//   sort:  one workgroup per sequence that a pair of the launch set names - once, however many pairs name it.  4096 tuples of
//          6 x uint32 are 96 KiB of LDS; the launch sizes it by the longest sequence of the set.
//   match: the pairs are grouped by their first sequence; one workgroup per group (of at most 64 pairs) stages that row once -
//          tuples and the run lengths as uint16 (a run is at most 4096 long), 24 + 12 bytes per slot, 144 KiB at the limit, inside
//          the 160 KiB a workgroup may have - and each wavefront takes a pair of the group.
// sc_edit_distance: one workgroup per pair, an anti-diagonal wavefront.  With s the shorter side (m symbols) and l the longer one
//   (n symbols), diagonal d holds D(i, d - i), indexed by i = 0..m; D_d needs D_{d-1} and D_{d-2} only, so three rolling diagonals
//   of m + 1 int32 live in LDS beside s itself (4 (4 m + 3) bytes: 128 KiB at m = 8192); l is read from global memory (a diagonal
//   reads consecutive addresses); one barrier per diagonal, m + n diagonals.  The launch sizes the LDS by the longest short side of
//   its pairs, and pairs with a short side below 1024 run in launches of their own with 256 threads and at most 16 KiB.
#include <algorithm>
#include <cstring>
#include <list>
#include <mutex>
#include <vector>

#include "device_util.h"
#include "handle.h"
#include "seq_match.h"

namespace sc {

static constexpr int NGM_W = 6;                          // the largest order
static constexpr int NGM_MAX_LEN = 4096;                 // symbols per sequence
static constexpr int NGM_SORT_THREADS = 512, NGM_MATCH_THREADS = 256, NGM_MATCH_WAVES = NGM_MATCH_THREADS / 64;
static constexpr int NGM_GROUP_PAIRS = 64;               // pairs that share one staged row
static constexpr int ED_MAX_SHORT = 8192, ED_MAX_LONG = 1 << 20;
static constexpr int ED_SMALL = 1024;                    // short sides below it: the 256-thread launches
static constexpr int ED_THREADS_SMALL = 256, ED_THREADS_LARGE = 1024;
// one launch set covers consecutive pairs up to these sums (a pair is never split), so scratch stays bounded whatever the call
// holds: 2^21 symbols are 72 MiB of tuples and counts
static constexpr int64_t SEQ_CHUNK_SYMBOLS = (int64_t)1 << 21, SEQ_CHUNK_PAIRS = (int64_t)1 << 20;

using NgmTuple = SeqTuple<NGM_W>;
using NgmCounts = SeqCounts<NGM_W, uint16_t>;
static_assert(sizeof(NgmTuple) == 24 && sizeof(NgmCounts) == 12, "24 + 12 bytes per slot");
static_assert((size_t)NGM_MAX_LEN * (sizeof(NgmTuple) + sizeof(NgmCounts)) <= 160 * 1024, "a staged row fits the LDS of a workgroup");

struct SeqDesc {  // one sequence of a launch set
    uint32_t off;  // first symbol / first sorted slot
    int32_t len;
};
struct NgmGroup {  // pairs (a, b_k) that share a
    int32_t a;
    int32_t num;
    uint32_t first;  // its first NgmPair
    int32_t reserved;
};
struct NgmPair {
    int32_t b;
    int32_t out;  // the pair's index within the launch set
};
struct EdPair {
    int32_t s, l;  // the shorter and the longer sequence
    int32_t out;
    int32_t reserved;
};

__global__ __launch_bounds__(NGM_SORT_THREADS) void ngm_sort_kernel(const int32_t* __restrict__ sym, const SeqDesc* __restrict__ seqs,
                                                                    NgmTuple* __restrict__ keys, NgmCounts* __restrict__ counts) {
    extern __shared__ NgmTuple s_sort[];  // the next power of two >= the longest sequence of the launch
    const SeqDesc q = seqs[blockIdx.x];
    if (q.len == 0) return;  // 0..NGM_MAX_LEN, checked on the host
    seq_sort_count<NGM_W, uint16_t>(sym + q.off, q.len, s_sort, keys + q.off, counts + q.off);
}

__global__ __launch_bounds__(NGM_MATCH_THREADS) void ngm_match_kernel(const SeqDesc* __restrict__ seqs, const NgmGroup* __restrict__ groups,
                                                                      const NgmPair* __restrict__ pairs, const NgmTuple* __restrict__ keys,
                                                                      const NgmCounts* __restrict__ counts, int max_order,
                                                                      int32_t* __restrict__ match) {
    extern __shared__ NgmTuple s_row[];  // row a: len_a tuples, then len_a counts (the launch sizes it by the longest first sequence)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const NgmGroup g = groups[blockIdx.x];
    const SeqDesc a = seqs[g.a];
    NgmCounts* s_cnt = reinterpret_cast<NgmCounts*>(s_row + a.len);
    for (int p = tid; p < a.len; p += NGM_MATCH_THREADS) {
        s_row[p] = keys[a.off + p];
        s_cnt[p] = counts[a.off + p];
    }
    __syncthreads();
    for (int k = wave; k < g.num; k += NGM_MATCH_WAVES) {  // the whole wavefront takes the same pair
        const NgmPair pr = pairs[g.first + k];
        const SeqDesc b = seqs[pr.b];
        int m[NGM_W];
        seq_match_wave<NGM_W, uint16_t>(s_row, s_cnt, a.len, keys + b.off, counts + b.off, b.len, max_order, lane, m);
        if (lane == 0) {
            int32_t* o = match + (int64_t)pr.out * NGM_W;
#pragma unroll
            for (int c = 0; c < NGM_W; ++c) o[c] = m[c];
        }
    }
}

__global__ __launch_bounds__(ED_THREADS_LARGE) void edit_distance_kernel(const int32_t* __restrict__ sym, const SeqDesc* __restrict__ seqs,
                                                                         const EdPair* __restrict__ pairs, int32_t* __restrict__ dist) {
    extern __shared__ int32_t s_ed[];  // three diagonals of m + 1, then the m symbols of the short side
    const int tid = threadIdx.x, threads = blockDim.x;
    const EdPair pr = pairs[blockIdx.x];
    const SeqDesc qs = seqs[pr.s], ql = seqs[pr.l];
    const int m = qs.len, n = ql.len;  // m <= n, m <= ED_MAX_SHORT: the host arranged and checked it
    if (m == 0) {
        if (tid == 0) dist[pr.out] = n;
        return;
    }
    const int32_t* __restrict__ lg = sym + ql.off;
    int32_t* s_short = s_ed + 3 * (m + 1);
    for (int i = tid; i < m; i += threads) s_short[i] = sym[qs.off + i];
    // D_0 = {D(0, 0)} and D_1 = {D(0, 1), D(1, 0)}
    int32_t* prev2 = s_ed;                 // D_{d-2}
    int32_t* prev = s_ed + (m + 1);        // D_{d-1}
    int32_t* cur = s_ed + 2 * (m + 1);     // D_d
    if (tid == 0) prev2[0] = 0, prev[0] = 1, prev[1] = 1;
    __syncthreads();
    const int last = m + n;
    for (int d = 2; d <= last; ++d) {
        // the cells (i, j = d - i) of the diagonal: j <= n and i <= m; the borders D(0, j) = j and D(i, 0) = i are set apart
        const int lo = d - n > 1 ? d - n : 1, hi = d - 1 < m ? d - 1 : m;
        for (int i = lo + tid; i <= hi; i += threads) {
            const int j = d - i;
            const int sub = prev2[i - 1] + (s_short[i - 1] != lg[j - 1] ? 1 : 0);
            const int del = prev[i - 1] + 1;  // from (i - 1, j)
            const int ins = prev[i] + 1;      // from (i, j - 1)
            const int best = del < ins ? del : ins;
            cur[i] = sub < best ? sub : best;
        }
        if (tid == 0) {
            if (d <= n) cur[0] = d;
            if (d <= m) cur[d] = d;
        }
        __syncthreads();
        int32_t* t = prev2;
        prev2 = prev, prev = cur, cur = t;
    }
    if (tid == 0) dist[pr.out] = prev[m];  // D(m, n), on the last diagonal
}

// per device: the buffers of one launch set
struct MetricsDevice {
    int device;
    ScratchBuffer sym, seqs, groups, pairs, keys, counts, out;
};
static std::mutex g_metrics_mutex;
static std::list<MetricsDevice> g_metrics_devices;

// g_metrics_mutex held
static MetricsDevice& metrics_device_state(int device) {
    for (auto& x : g_metrics_devices)
        if (x.device == device) return x;
    g_metrics_devices.push_back(MetricsDevice{device});
    return g_metrics_devices.back();
}

// the checks both entries share; -> nothing, it throws
static void check_pool(const char* who, const int32_t* h_symbols, const int64_t* h_offsets, int32_t n_seq, const int32_t* h_pairs, int64_t n_pairs,
                       const void* h_out) {
    SC_CHECK(h_offsets && (h_pairs || n_pairs == 0) && (h_out || n_pairs == 0), "%s: null argument", who);
    SC_CHECK(n_seq >= 1, "%s: %d sequences, at least 1 is needed", who, n_seq);
    SC_CHECK(n_pairs >= 0 && n_pairs <= ((int64_t)1 << 31) - 1, "%s: %lld pairs, the limit is 0..2^31 - 1", who, (long long)n_pairs);
    SC_CHECK(h_offsets[0] == 0, "%s: offsets[0] is %lld, not 0", who, (long long)h_offsets[0]);
    for (int64_t i = 0; i < n_seq; ++i)
        SC_CHECK(h_offsets[i + 1] >= h_offsets[i], "%s: the offsets decrease at sequence %lld", who, (long long)i);
    const int64_t total = h_offsets[n_seq];
    SC_CHECK(total == 0 || h_symbols, "%s: null argument", who);
    for (int64_t p = 0; p < total; ++p) SC_CHECK(h_symbols[p] >= 0, "%s: the negative symbol %d at position %lld", who, h_symbols[p], (long long)p);
    for (int64_t k = 0; k < 2 * n_pairs; ++k)
        SC_CHECK(h_pairs[k] >= 0 && h_pairs[k] < n_seq, "%s: pair %lld names sequence %d of %d", who, (long long)(k / 2), h_pairs[k], n_seq);
}

// The sequences a launch set names, each once, in the order of their first mention: packed symbols and one descriptor each.
struct SeqSet {
    std::vector<int32_t> slot;  // pool index -> index within the set, -1: not in it
    std::vector<int32_t> members;
    std::vector<int32_t> sym;
    std::vector<SeqDesc> seqs;
    explicit SeqSet(int32_t n_seq) : slot((size_t)n_seq, -1) {}
    void clear() {
        for (int32_t s : members) slot[(size_t)s] = -1;
        members.clear(), sym.clear(), seqs.clear();
    }
    bool has(int32_t s) const { return slot[(size_t)s] >= 0; }
    int32_t add(int32_t s, const int32_t* h_symbols, const int64_t* h_offsets) {
        if (slot[(size_t)s] < 0) {
            slot[(size_t)s] = (int32_t)seqs.size();
            members.push_back(s);
            seqs.push_back(SeqDesc{(uint32_t)sym.size(), (int32_t)(h_offsets[s + 1] - h_offsets[s])});
            sym.insert(sym.end(), h_symbols + h_offsets[s], h_symbols + h_offsets[s + 1]);
        }
        return slot[(size_t)s];
    }
};

}  // namespace sc

using namespace sc;

extern "C" {

int sc_ngram_match(const int32_t* h_symbols, const int64_t* h_offsets, int32_t n_seq, const int32_t* h_pairs, int64_t n_pairs, int32_t max_order,
                   int32_t* h_match) {
    SC_API_BEGIN
    // every argument check comes before the first device call
    SC_CHECK(max_order >= 1 && max_order <= NGM_W, "sc_ngram_match: max_order %d is outside the limit 1..%d", max_order, NGM_W);
    check_pool("sc_ngram_match", h_symbols, h_offsets, n_seq, h_pairs, n_pairs, h_match);
    for (int64_t i = 0; i < n_seq; ++i) {
        const int64_t L = h_offsets[i + 1] - h_offsets[i];
        SC_CHECK(L <= NGM_MAX_LEN, "sc_ngram_match: sequence %lld has %lld symbols, the limit is %d", (long long)i, (long long)L, NGM_MAX_LEN);
    }
    if (n_pairs == 0) return SC_OK;

    int device = 0;
    SC_HIP(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(g_metrics_mutex);
    MetricsDevice& dv = metrics_device_state(device);
    hipStream_t stream = nullptr;  // the default stream, like sc_mbr_select: ordered behind the caller's work on it
    auto len_of = [&](int32_t s) { return h_offsets[s + 1] - h_offsets[s]; };

    SeqSet set(n_seq);
    std::vector<NgmGroup> groups;
    std::vector<NgmPair> pairs;
    std::vector<int32_t> order;  // the set's pairs, those with the same first sequence together
    for (int64_t p0 = 0; p0 < n_pairs;) {
        // the launch set [p0, p1)
        set.clear(), groups.clear(), pairs.clear(), order.clear();
        int64_t p1 = p0;
        while (p1 < n_pairs && p1 - p0 < SEQ_CHUNK_PAIRS) {
            const int32_t a = h_pairs[2 * p1], b = h_pairs[2 * p1 + 1];
            const int64_t extra = (set.has(a) ? 0 : len_of(a)) + (set.has(b) || b == a ? 0 : len_of(b));
            if (p1 > p0 && (int64_t)set.sym.size() + extra > SEQ_CHUNK_SYMBOLS) break;
            set.add(a, h_symbols, h_offsets), set.add(b, h_symbols, h_offsets);
            ++p1;
        }
        const size_t Q = (size_t)(p1 - p0), S = set.seqs.size(), T = set.sym.size();
        order.resize(Q);
        for (size_t k = 0; k < Q; ++k) order[k] = (int32_t)k;
        std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return h_pairs[2 * (p0 + x)] < h_pairs[2 * (p0 + y)]; });
        int longest = 1, longest_first = 1;
        for (const SeqDesc& q : set.seqs) longest = std::max(longest, q.len);
        for (size_t k = 0; k < Q; ++k) {
            const int32_t a = set.slot[(size_t)h_pairs[2 * (p0 + order[k])]], b = set.slot[(size_t)h_pairs[2 * (p0 + order[k]) + 1]];
            if (groups.empty() || groups.back().a != a || groups.back().num == NGM_GROUP_PAIRS) {
                groups.push_back(NgmGroup{a, 0, (uint32_t)pairs.size(), 0});
                longest_first = std::max(longest_first, set.seqs[(size_t)a].len);
            }
            ++groups.back().num;
            pairs.push_back(NgmPair{b, order[k]});
        }
        int P2 = 1;
        while (P2 < longest) P2 <<= 1;
        const size_t sort_lds = (size_t)P2 * sizeof(NgmTuple);                                    // at most 96 KiB
        const size_t row_lds = (size_t)longest_first * (sizeof(NgmTuple) + sizeof(NgmCounts));   // at most 144 KiB
        // the default limit holds up to 64 KiB; longer sequences raise it (idempotent, per device)
        if (sort_lds > 64 * 1024)
            SC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&ngm_sort_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
        if (row_lds > 64 * 1024)
            SC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&ngm_match_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024));

        int32_t* d_sym = dv.sym.grow<int32_t>(T);
        SeqDesc* d_seqs = dv.seqs.grow<SeqDesc>(S);
        NgmGroup* d_groups = dv.groups.grow<NgmGroup>(groups.size());
        NgmPair* d_pairs = dv.pairs.grow<NgmPair>(Q);
        NgmTuple* d_keys = dv.keys.grow<NgmTuple>(T);
        NgmCounts* d_counts = dv.counts.grow<NgmCounts>(T);
        int32_t* d_match = dv.out.grow<int32_t>(Q * NGM_W);
        if (T) SC_HIP(hipMemcpyAsync(d_sym, set.sym.data(), T * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        SC_HIP(hipMemcpyAsync(d_seqs, set.seqs.data(), S * sizeof(SeqDesc), hipMemcpyHostToDevice, stream));
        SC_HIP(hipMemcpyAsync(d_groups, groups.data(), groups.size() * sizeof(NgmGroup), hipMemcpyHostToDevice, stream));
        SC_HIP(hipMemcpyAsync(d_pairs, pairs.data(), Q * sizeof(NgmPair), hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(ngm_sort_kernel, dim3((unsigned)S), dim3(NGM_SORT_THREADS), sort_lds, stream, d_sym, d_seqs, d_keys, d_counts);
        SC_LAUNCH_CHECK();
        hipLaunchKernelGGL(ngm_match_kernel, dim3((unsigned)groups.size()), dim3(NGM_MATCH_THREADS), row_lds, stream, d_seqs, d_groups, d_pairs,
                           d_keys, d_counts, (int)max_order, d_match);
        SC_LAUNCH_CHECK();
        // the set's pairs are consecutive in the caller's array
        SC_HIP(hipMemcpyAsync(h_match + p0 * NGM_W, d_match, Q * NGM_W * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        SC_HIP(hipStreamSynchronize(stream));
        p0 = p1;
    }
    SC_API_END
}

int sc_edit_distance(const int32_t* h_symbols, const int64_t* h_offsets, int32_t n_seq, const int32_t* h_pairs, int64_t n_pairs, int32_t* h_dist) {
    SC_API_BEGIN
    // every argument check comes before the first device call
    check_pool("sc_edit_distance", h_symbols, h_offsets, n_seq, h_pairs, n_pairs, h_dist);
    auto len_of = [&](int32_t s) { return h_offsets[s + 1] - h_offsets[s]; };
    for (int64_t p = 0; p < n_pairs; ++p) {
        const int64_t la = len_of(h_pairs[2 * p]), lb = len_of(h_pairs[2 * p + 1]);
        SC_CHECK(std::min(la, lb) <= ED_MAX_SHORT, "sc_edit_distance: pair %lld has %lld and %lld symbols, the shorter side may have at most %d",
                 (long long)p, (long long)la, (long long)lb, ED_MAX_SHORT);
        SC_CHECK(std::max(la, lb) <= ED_MAX_LONG, "sc_edit_distance: pair %lld has %lld and %lld symbols, the longer side may have at most %d",
                 (long long)p, (long long)la, (long long)lb, ED_MAX_LONG);
    }
    if (n_pairs == 0) return SC_OK;

    int device = 0;
    SC_HIP(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(g_metrics_mutex);
    MetricsDevice& dv = metrics_device_state(device);
    hipStream_t stream = nullptr;

    SeqSet set(n_seq);
    std::vector<EdPair> pairs;
    std::vector<int64_t> where;  // the caller's index of each pair of the launch set
    std::vector<int32_t> dist;
    // two passes: the pairs with a short side below ED_SMALL, then the others - so that short pairs never pay a long pair's LDS
    for (int large = 0; large < 2; ++large) {
        auto mine = [&](int64_t p) { return (std::min(len_of(h_pairs[2 * p]), len_of(h_pairs[2 * p + 1])) >= ED_SMALL) == (large == 1); };
        for (int64_t p0 = 0; p0 < n_pairs;) {
            set.clear(), pairs.clear(), where.clear();
            int64_t p1 = p0;
            int longest_short = 0;
            for (; p1 < n_pairs && (int64_t)pairs.size() < SEQ_CHUNK_PAIRS; ++p1) {
                if (!mine(p1)) continue;
                const int32_t a = h_pairs[2 * p1], b = h_pairs[2 * p1 + 1];
                const int64_t extra = (set.has(a) ? 0 : len_of(a)) + (set.has(b) || b == a ? 0 : len_of(b));
                if (!pairs.empty() && (int64_t)set.sym.size() + extra > SEQ_CHUNK_SYMBOLS) break;
                const int32_t ia = set.add(a, h_symbols, h_offsets), ib = set.add(b, h_symbols, h_offsets);
                const bool a_short = len_of(a) <= len_of(b);
                pairs.push_back(EdPair{a_short ? ia : ib, a_short ? ib : ia, (int32_t)pairs.size(), 0});
                where.push_back(p1);
                longest_short = std::max<int>(longest_short, (int)std::min(len_of(a), len_of(b)));
            }
            p0 = p1;
            if (pairs.empty()) continue;
            const size_t Q = pairs.size(), S = set.seqs.size(), T = set.sym.size();
            const size_t lds = (size_t)(4 * longest_short + 3) * sizeof(int32_t);  // at most 131 084 B
            if (lds > 64 * 1024)
                SC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&edit_distance_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)((4 * ED_MAX_SHORT + 3) * sizeof(int32_t))));
            int32_t* d_sym = dv.sym.grow<int32_t>(T);
            SeqDesc* d_seqs = dv.seqs.grow<SeqDesc>(S);
            EdPair* d_pairs = dv.pairs.grow<EdPair>(Q);
            int32_t* d_dist = dv.out.grow<int32_t>(Q);
            if (T) SC_HIP(hipMemcpyAsync(d_sym, set.sym.data(), T * sizeof(int32_t), hipMemcpyHostToDevice, stream));
            SC_HIP(hipMemcpyAsync(d_seqs, set.seqs.data(), S * sizeof(SeqDesc), hipMemcpyHostToDevice, stream));
            SC_HIP(hipMemcpyAsync(d_pairs, pairs.data(), Q * sizeof(EdPair), hipMemcpyHostToDevice, stream));
            hipLaunchKernelGGL(edit_distance_kernel, dim3((unsigned)Q), dim3(large ? ED_THREADS_LARGE : ED_THREADS_SMALL), lds, stream, d_sym, d_seqs,
                               d_pairs, d_dist);
            SC_LAUNCH_CHECK();
            dist.resize(Q);
            SC_HIP(hipMemcpyAsync(dist.data(), d_dist, Q * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
            SC_HIP(hipStreamSynchronize(stream));
            for (size_t k = 0; k < Q; ++k) h_dist[where[k]] = dist[k];
        }
    }
    SC_API_END
}

}  // extern "C"
