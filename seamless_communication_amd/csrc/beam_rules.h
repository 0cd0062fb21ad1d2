// Device helpers of the generation step rules, shared by the beam search (k_beam.hip) and the sampler (k_sample.hip): the total
// order of candidate values, the value of a (row, token) candidate under the step rules, the banned-sequence processor and the
// phrase-boost processor.
#pragma once
#include "kernels.h"
#include "boost_list.h"

namespace sc {
namespace {

// Order-preserving map of an fp32 value to int32 (-0 and +0 map to the same key; -inf to the smallest key; a NaN of any sign
// and payload to ONE key above that of +inf - the order of torch.topk, which the reference's search uses) and back (a NaN
// comes back as the quiet NaN 0x7fc00000).  Every candidate path (plain, banned, chunked) orders by these keys.
// beam_candidates_kernel orders its per-thread lists by these keys: with fp32 comparisons in that insertion network, the
// compiled kernel dropped every -inf candidate of a thread whose list had not yet taken a finite value (a forced-EOS step:
// the list filled with another thread's -inf entries out of index order, or with the 0x7fffffff sentinel), although the
// source and its IR order them correctly.  Integer keys give a total order (NaN included) without float compares.
constexpr int KEY_NAN = 0x7fc00000;
__device__ __forceinline__ int order_key(float v) {
    const int k = __float_as_int(v + 0.f);  // -0 + 0 = +0
    if ((k & 0x7fffffff) > 0x7f800000) return KEY_NAN;
    return k >= 0 ? k : k ^ 0x7fffffff;
}
__device__ __forceinline__ float key_value(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }
__device__ __forceinline__ bool better_key(int v, int i, int w, int j) { return v > w || (v == w && i < j); }

// BannedSequenceProcessor for one row, by the whole workgroup.  seq: the row's S tokens so far (prompt included).  Banned
// sequence q = tokens[offsets[q] .. offsets[q+1]) of length L (1 <= L <= BANNED_MAX_LEN, checked by the launcher): when its
// first L-1 tokens equal the row's last L-1 tokens (right-aligned, over its own length only; L-1 > S never matches; L == 1
// always does) the logit of its last token becomes -inf.  The row's tail (min(S, max_len - 1) tokens) is staged once in LDS
// (s_tail: BANNED_MAX_LEN ints), threads stride over the sequences; several threads may store the same -inf to one address.
// Every thread of the workgroup must call it (barriers); the caller orders the stores before later reads of the row.
__device__ __forceinline__ void banned_block_row(float* row, int V, const int* __restrict__ seq, int S, const BannedList& bl, int* s_tail) {
    const int T = min(S, min(bl.max_len, BANNED_MAX_LEN) - 1);
    __syncthreads();  // s_tail may still be read for the previous row
    for (int i = threadIdx.x; i < T; i += 256) s_tail[i] = seq[S - T + i];
    __syncthreads();
    for (int q = threadIdx.x; q < bl.n; q += 256) {
        const int o = bl.offsets[q];
        const int P = bl.offsets[q + 1] - o - 1;  // prefix length
        if (P < 0 || P > T) continue;             // P > T: longer than the row's sequence (P <= max_len - 1 always)
        bool same = true;
        for (int e = 0; e < P; ++e) same = same && (bl.tokens[o + e] == s_tail[T - P + e]);
        const int t = bl.tokens[o + P];
        if (same && t >= 0 && t < V) row[t] = -INFINITY;
    }
}

// ---- PhraseBoostProcessor (the rule: boost_list.h) ----------------------------------------------------------------------------
// The kept candidates of a row are children of the trie nodes on the row's suffix chain (levels 0 .. 63), one per distinct
// token.  A trie with n leaves has sum(children - 1) = n - 1 over its inner nodes, so the chain's nodes have at most
// n - 1 + 64 children in all.
constexpr int BOOST_MAX_CAND = BOOST_MAX_PHRASES + BOOST_MAX_LEN;
struct BoostShared {
    int tail[BOOST_MAX_LEN];
    int lo[BOOST_MAX_LEN + 1];  // level P: the phrases [lo, hi) start with the row's last P tokens
    int hi[BOOST_MAX_LEN + 1];
    unsigned long long open;  // bit P: level P is not empty and its suffix is no whole phrase (it has children)
    int dp;
    int count;
    int c_tok[BOOST_MAX_CAND];
    float c_val[BOOST_MAX_CAND];
};

// phrase q against key[0 .. P): < 0 / > 0 as the sorted list orders them, 0 when q starts with the key (a phrase shorter than P
// that agrees with the key over its own length sorts in front of it)
__device__ __forceinline__ int boost_cmp(const BoostList& bo, int q, const int* key, int P) {
    const int o = bo.offsets[q], L = bo.offsets[q + 1] - o;
    const int m = min(L, P);
    for (int e = 0; e < m; ++e) {
        const int a = bo.tokens[o + e], b = key[e];
        if (a != b) return a < b ? -1 : 1;
    }
    return L < P ? -1 : 0;
}

// PhraseBoostProcessor for one row, by the whole workgroup: row[t] = fmaf(beta, k(y, t), row[t]) for every t < V with k != 0.
// 1. the row's tail (min(S, max_len) tokens) goes to LDS; 2. wavefront 0 takes one suffix length P = 1 .. 64 per lane and
// binary-searches the sorted list for the phrases that start with the row's last P tokens (level 0 is the whole list): the
// non-empty levels are the trie nodes on the row's suffix chain, the deepest is d(y), a level whose phrase has P tokens is a
// whole phrase; 3. the candidates of level P are the distinct entries of column P over its range (adjacent: the range is
// sorted); one that a deeper level offers too is dropped there, so d(y + t) is the maximum; the kept ones take their value from
// the UNMODIFIED logit into LDS; 4. when dp(y) > 0 the whole row moves by -beta * dp; 5. the candidates are stored.  Each token
// is kept once, so the result does not depend on the order of the LDS slots (an integer counter hands them out).
// Every thread of the workgroup must call it (barriers); the caller orders the stores before later reads of the row.
__device__ __forceinline__ void boost_row(float* row, int V, const int* __restrict__ seq, int S, const BoostList& bo, BoostShared& sh) {
    const int tid = threadIdx.x;
    const int T = min(S, min(bo.max_len, BOOST_MAX_LEN));
    __syncthreads();  // the LDS may still be read for the previous row; the other processors' stores to this row are done
    for (int i = tid; i < T; i += 256) sh.tail[i] = seq[S - T + i];
    if (tid == 0) sh.count = 0;
    __syncthreads();
    if (tid < 64) {  // wavefront 0
        const int P = tid + 1;
        int lo = 0, hi = 0;
        bool leaf = false;
        if (P <= T) {
            const int* key = sh.tail + (T - P);
            int a = 0, b = bo.n;
            while (a < b) {
                const int mid = (a + b) >> 1;
                if (boost_cmp(bo, mid, key, P) < 0) a = mid + 1; else b = mid;
            }
            lo = a;
            b = (a < bo.n && boost_cmp(bo, a, key, P) == 0) ? bo.n : a;  // most levels are empty: no second search then
            while (a < b) {
                const int mid = (a + b) >> 1;
                if (boost_cmp(bo, mid, key, P) <= 0) a = mid + 1; else b = mid;
            }
            hi = a;
            leaf = lo < hi && bo.offsets[lo + 1] - bo.offsets[lo] == P;
        }
        sh.lo[P] = lo;
        sh.hi[P] = hi;
        const unsigned long long full = __ballot(lo < hi);
        const unsigned long long open = __ballot(lo < hi && !leaf);  // (level 64 is a whole phrase when it is not empty)
        const int d = full ? 64 - __clzll((long long)full) : 0;
        if (P == d) sh.dp = leaf ? 0 : d;
        if (tid == 0) {
            sh.lo[0] = 0;
            sh.hi[0] = bo.n;
            sh.open = (open << 1) | 1ull;
            if (d == 0) sh.dp = 0;
        }
    }
    __syncthreads();
    const int dp = sh.dp;
    const float beta = bo.beta;
    for (unsigned long long m = sh.open; m; m &= m - 1) {
        const int P = __ffsll((long long)m) - 1;
        const int lo = sh.lo[P], hi = sh.hi[P];
        for (int q = lo + tid; q < hi; q += 256) {
            const int o = bo.offsets[q];
            if (bo.offsets[q + 1] - o <= P) continue;  // (never in a prefix-free list: an open level holds longer phrases only)
            const int t = bo.tokens[o + P];
            if (q > lo && bo.tokens[bo.offsets[q - 1] + P] == t) continue;  // not the first of its run
            bool deeper = false;
            for (unsigned long long m2 = m & (m - 1); m2 && !deeper; m2 &= m2 - 1) {
                const int P2 = __ffsll((long long)m2) - 1;
                const int end = sh.hi[P2];
                int a = sh.lo[P2], b = end;
                while (a < b) {
                    const int mid = (a + b) >> 1;
                    if (bo.tokens[bo.offsets[mid] + P2] < t) a = mid + 1; else b = mid;
                }
                deeper = a < end && bo.tokens[bo.offsets[a] + P2] == t;
            }
            if (deeper || t < 0 || t >= V) continue;
            const int k = P + 1 - dp;
            const float x = row[t];
            const int slot = atomicAdd(&sh.count, 1);
            if (slot < BOOST_MAX_CAND) {
                sh.c_tok[slot] = t;
                sh.c_val[slot] = k == 0 ? x : fmaf(beta, (float)k, x);
            }
        }
    }
    __syncthreads();
    if (dp > 0) {
        // one workgroup streams the whole row (1 MB at V = 256 102): 16-byte accesses, four in flight per thread, behind up to
        // three scalar elements that bring the pointer to 16 bytes and in front of a scalar tail (a row stride need not be a
        // multiple of four floats).  The same fmaf on every element whichever path takes it.
        const float back = -(float)dp;
        const int head = min(V, (int)((4 - ((reinterpret_cast<uintptr_t>(row) >> 2) & 3)) & 3));
        const int nvec = (V - head) >> 2;
        if (tid < head) row[tid] = fmaf(beta, back, row[tid]);
        float4* r4 = reinterpret_cast<float4*>(row + head);
        for (int i = tid; i < nvec; i += 256 * 4) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i + 256 * u < nvec) v[u] = r4[i + 256 * u];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i + 256 * u < nvec) {
                    v[u].x = fmaf(beta, back, v[u].x);
                    v[u].y = fmaf(beta, back, v[u].y);
                    v[u].z = fmaf(beta, back, v[u].z);
                    v[u].w = fmaf(beta, back, v[u].w);
                    r4[i + 256 * u] = v[u];
                }
        }
        for (int i = head + 4 * nvec + tid; i < V; i += 256) row[i] = fmaf(beta, back, row[i]);
    }
    __syncthreads();
    const int cnt = min(sh.count, BOOST_MAX_CAND);
    for (int c = tid; c < cnt; c += 256) row[sh.c_tok[c]] = sh.c_val[c];
}

// Value of the candidate (row, token t): log-softmax of the logit x (l: the row's log-sum-exp), the generation step rules, + the
// beam's cumulative score.  A token that a rule excludes (EOS before min_seq_len, everything but EOS at the length limit, PAD)
// is -inf whatever the row and the score hold: a beam that carries NaN still never emits PAD and still ends at the limit.
__device__ __forceinline__ float candidate_value(float x, float l, float base, int t, int no_eos, int force_eos, int pad_idx, int eos_idx,
                                                 int unk_idx, float unk_penalty) {
    float lp = x - l;
    if (t == unk_idx) lp -= unk_penalty;
    const bool excluded = (no_eos && t == eos_idx) || (force_eos && t != eos_idx) || t == pad_idx;
    return excluded ? -INFINITY : lp + base;
}

}  // namespace
}  // namespace sc
