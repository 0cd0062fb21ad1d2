// Device helpers of the generation step rules, shared by the beam search (k_beam.hip) and the sampler (k_sample.hip): the total
// order of candidate values, the value of a (row, token) candidate under the step rules, and the banned-sequence processor.
#pragma once
#include "kernels.h"

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
