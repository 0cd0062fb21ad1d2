// Clipped n-gram match counts between int32 symbol sequences by sorted tuples, templated on the tuple width W (the largest order):
// k_mbr.hip instantiates W = 4 on token ids (sc_mbr_select), k_metrics.hip W = 6 on characters and word ids (sc_ngram_match).
//
// An n-gram is compared as the tuple of its symbols, never as a packed or hashed key: a sequence's start positions p become the
// W-tuples (t[p], .., t[p+W-1]) of uint32 with a symbol t stored as t + 1 and 0 behind the end of the sequence.  Sorted
// lexicographically, the tuples are sorted by their first n components for every n <= W at once, the n-grams of order n are the
// tuples whose n-th component is not 0, and equal n-grams are neighbours.
//   seq_sort_count: one workgroup, one sequence: the tuples, a bitonic sort in LDS, and per sorted slot and order the number of
//     times the n-gram occurs where the slot is the first of its run (0 elsewhere).  Both go to global memory.
//   seq_match_wave: one wavefront, one pair: row a (tuples and counts, in LDS) against the sorted b in global memory; a lane takes
//     a slot of a, finds the first slot of b that is not below it in the first n components (binary search) and adds
//     min(count_a, count_b); integer sums over the lanes give m_1..m_W.
// CT is the type of a count: a run is at most the sequence's length, so uint16_t holds it up to 65535 symbols.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "common.h"

namespace sc {

static constexpr uint32_t SEQ_SORT_PAD = 0xffffffffu;  // above every stored symbol (at most 2^31)

template <int W>
struct alignas(W % 4 == 0 ? 16 : 8) SeqTuple {
    uint32_t v[W];
};
template <int W, typename CT>
struct alignas(sizeof(CT) * W % 16 == 0 ? 16 : sizeof(CT) * W % 8 == 0 ? 8 : 4) SeqCounts {
    CT v[W];
};

typedef unsigned int seq_u32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned int seq_u32x4_t __attribute__((ext_vector_type(4)));

// A whole tuple in as few loads as its alignment allows (16 bytes each at W = 4, 8 bytes each otherwise), all issued at once: read
// through the struct, the components are fetched one by one as a comparison gets to them, each load behind a branch on the last.
template <int W>
__device__ __forceinline__ SeqTuple<W> seq_load(const SeqTuple<W>* p) {
    static_assert(W % 2 == 0, "an even tuple width");
    SeqTuple<W> t;
    if constexpr (W % 4 == 0) {
#pragma unroll
        for (int k = 0; k < W / 4; ++k) {
            const seq_u32x4_t x = reinterpret_cast<const seq_u32x4_t*>(p)[k];
            t.v[4 * k] = x[0], t.v[4 * k + 1] = x[1], t.v[4 * k + 2] = x[2], t.v[4 * k + 3] = x[3];
        }
    } else {
#pragma unroll
        for (int k = 0; k < W / 2; ++k) {
            const seq_u32x2_t x = reinterpret_cast<const seq_u32x2_t*>(p)[k];
            t.v[2 * k] = x[0], t.v[2 * k + 1] = x[1];
        }
    }
    return t;
}

// -1 / 0 / 1: a against b in the first n components
template <int W>
__device__ __forceinline__ int seq_cmp(const SeqTuple<W>& a, const SeqTuple<W>& b, int n) {
#pragma unroll
    for (int c = 0; c < W; ++c) {
        if (c < n && a.v[c] != b.v[c]) return a.v[c] < b.v[c] ? -1 : 1;
    }
    return 0;
}

// The whole workgroup calls it with the same arguments.  t: the L >= 1 symbols; s_key: room for the next power of two >= L
// tuples in LDS; keys / counts: L slots each.
template <int W, typename CT>
__device__ __forceinline__ void seq_sort_count(const int32_t* __restrict__ t, int L, SeqTuple<W>* s_key, SeqTuple<W>* __restrict__ keys,
                                               SeqCounts<W, CT>* __restrict__ counts) {
    const int tid = threadIdx.x, threads = blockDim.x;
    int P2 = 1;
    while (P2 < L) P2 <<= 1;
    for (int p = tid; p < P2; p += threads) {
        SeqTuple<W> k;
#pragma unroll
        for (int c = 0; c < W; ++c) k.v[c] = p >= L ? SEQ_SORT_PAD : p + c < L ? (uint32_t)t[p + c] + 1u : 0u;
        s_key[p] = k;
    }
    __syncthreads();
    for (int k = 2; k <= P2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = tid; p < P2; p += threads) {
                const int q = p ^ j;
                if (q > p) {
                    const SeqTuple<W> a = seq_load<W>(s_key + p), b = seq_load<W>(s_key + q);
                    const bool ascending = (p & k) == 0;
                    if ((seq_cmp<W>(a, b, W) > 0) == ascending) s_key[p] = b, s_key[q] = a;
                }
            }
            __syncthreads();
        }
    }
    for (int p = tid; p < L; p += threads) {
        const SeqTuple<W> a = seq_load<W>(s_key + p);
        SeqCounts<W, CT> cnt;
#pragma unroll
        for (int c = 0; c < W; ++c) {
            const int n = c + 1;
            cnt.v[c] = 0;
            if (a.v[c] == 0u) continue;                                                // no n-gram starts here: the sequence ends first
            if (p > 0 && seq_cmp<W>(seq_load<W>(s_key + p - 1), a, n) == 0) continue;  // inside a run
            int lo = p + 1, hi = L;                                                    // the first slot behind the run
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (seq_cmp<W>(seq_load<W>(s_key + mid), a, n) == 0) lo = mid + 1; else hi = mid;
            }
            cnt.v[c] = (CT)(lo - p);
        }
        keys[p] = a;
        counts[p] = cnt;
    }
}

// The whole wavefront calls it with the same arguments; every lane returns m[0..W) = m_1..m_W (0 for orders above max_order).
template <int W, typename CT>
__device__ __forceinline__ void seq_match_wave(const SeqTuple<W>* s_row, const SeqCounts<W, CT>* s_cnt, int La, const SeqTuple<W>* __restrict__ kb,
                                               const SeqCounts<W, CT>* __restrict__ cb, int Lb, int max_order, int lane, int (&m)[W]) {
#pragma unroll
    for (int c = 0; c < W; ++c) m[c] = 0;
    for (int p = lane; p < La; p += 64) {
        const SeqTuple<W> a = seq_load<W>(s_row + p);
        const SeqCounts<W, CT> ca = s_cnt[p];
#pragma unroll
        for (int c = 0; c < W; ++c) {
            if (c >= max_order || ca.v[c] == 0) continue;
            const int n = c + 1;
            int lo = 0, hi = Lb;  // the first slot of b that is not below a
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (seq_cmp<W>(seq_load<W>(kb + mid), a, n) < 0) lo = mid + 1; else hi = mid;
            }
            if (lo < Lb && seq_cmp<W>(seq_load<W>(kb + lo), a, n) == 0) {  // the first slot of the run: it carries the run's length
                const uint32_t mine = ca.v[c], other = cb[lo].v[c];
                m[c] += (int)(mine < other ? mine : other);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < W; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m[c] += __shfl_xor(m[c], o);
    }
}

// per device: a scratch buffer of one launch set; grown on demand, never shrunk
struct ScratchBuffer {
    void* p = nullptr;
    size_t bytes = 0;
    template <typename T>
    T* grow(size_t n) {
        const size_t need = std::max<size_t>(n * sizeof(T), 256);
        if (bytes < need) {
            if (p) (void)hipFree(p);
            p = nullptr, bytes = 0;
            const size_t cap = need + need / 4;
            SC_HIP(hipMalloc(&p, cap));
            bytes = cap;
        }
        return static_cast<T*>(p);
    }
};

}  // namespace sc
