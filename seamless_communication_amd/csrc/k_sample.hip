// Sampled generation: one top-k / top-p draw per logit row (fairseq2 0.2 TopKSampler / TopPSampler restated).
//
// sample_rows_kernel: one workgroup of 1024 threads per live row.  With y = x / T (one rounded product per logit):
//   log-sum-exp of y (row max + sum of exp, two reads), the step processors (n-gram blocker, banned sequences: -inf into the
//   row AFTER the log-sum-exp is known, the helpers of the beam search), then for every token the value
//   v = candidate_value(y, lse, 0, ...) (step rules of beam_rules.h), its order key and its INTEGER mass
//   w = floor(exp(v) * 2^36).  Every sum below is a sum of these integers: exact, whatever the order of the additions.
//   Kept set: a prefix of the total order (key descending, index ascending), described by (tkey, ctie) = every token whose key
//   is above tkey and the first ctie tokens (index order) whose key is tkey.  Tokens of one key have one mass, so a prefix that
//   ends inside a run of equal keys needs no index scan to know its mass.
//     top-k: radix descent over the 32-bit keys by COUNT (four 8-bit levels, one read of the row each; 256 count + mass bins in
//            LDS, LDS integer atomics, a thread adds a run of equal bins once) -> key of the k-th token, mass Z_k of the k;
//     top-p: the same descent by MASS for the threshold floor(top_p * Z_k) -> the last token whose mass-before is <= it.
//   Draw: Philox4x32-10, key = seed, counter = (stream, gen, position); u24 = out[0] >> 8; R = (u24 * Z_kept) >> 24; the
//   token is the lowest index whose inclusive kept mass in INDEX order exceeds R: every wave owns a contiguous span of the row,
//   sums its kept mass (one read), the wave that holds R walks its span once more with a wave scan.  When the kept set ends
//   inside a run of equal keys, one more read counts the run's members per span first (their rank decides who is kept).
//   Z_kept == 0 (no kept token reaches 2^-36: a forced EOS of tiny probability, a row that is not a number): the first token
//   of the order.  Reads of the row: 2 + 4 per active filter + 2 (+ 1); nothing else leaves the CU.
// sample_prompt_lprob_kernel: the echoed prompt's log-probability under the same temperature.
#include "kernels.h"
#include "beam_rules.h"

namespace sc {

namespace {

constexpr int NT = 1024, NW = NT / 64, BINS = 256;

struct Rules {
    float inv, lse, unk_penalty;
    int no_eos, force_eos, pad_idx, eos_idx, unk_idx;
};

struct Lds {
    unsigned cnt[BINS];
    unsigned long long ms[BINS];
    unsigned scnt[BINS];  // inclusive sums over the bins, best bin first
    unsigned long long sms[BINS];
    float red[NW];
    unsigned wties[NW];
    unsigned long long wmass[NW];
    unsigned wkey[NW];
    int widx[NW];
    int tail[BANNED_MAX_LEN];
    int sel;
    int pick;
};

// the prefix of the order a descent stopped at: the key of its last token, count and mass of the better keys and of that key
struct Cut {
    unsigned key = 0, cnt_gt = 0, cnt_eq = 0;
    unsigned long long mass_gt = 0, mass_eq = 0, zk = 0, thr = 0;
    bool found = false;
};

__device__ __forceinline__ float token_value(float x, int t, const Rules& r) {
    return candidate_value(__fmul_rn(x, r.inv), r.lse, 0.f, t, r.no_eos, r.force_eos, r.pad_idx, r.eos_idx, r.unk_idx, r.unk_penalty);
}
// larger = better; NaN above +inf, -0 with +0 (order_key)
__device__ __forceinline__ unsigned ukey(float v) { return (unsigned)order_key(v) ^ 0x80000000u; }
__device__ __forceinline__ unsigned long long mass(float v) {
    return (v == v && v > -INFINITY) ? (unsigned long long)fminf(floorf(expf(v) * 0x1p36f), 0x1p62f) : 0ull;
}

__device__ __forceinline__ unsigned long long shfl_xor64(unsigned long long v, int o) {
    const unsigned lo = __shfl_xor((unsigned)v, o), hi = __shfl_xor((unsigned)(v >> 32), o);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long shfl_up64(unsigned long long v, int d) {
    const unsigned lo = __shfl_up((unsigned)v, d), hi = __shfl_up((unsigned)(v >> 32), d);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long shfl64(unsigned long long v, int l) {
    const unsigned lo = __shfl((unsigned)v, l), hi = __shfl((unsigned)(v >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}

// every thread calls f(t, x_t) for its tokens t = tid, tid + NT, ...; eight loads in flight
template <class F>
__device__ __forceinline__ void for_each_token(const float* row, int V, F f) {
    for (int i0 = threadIdx.x; i0 < V; i0 += NT * 8) {
        float x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = (i0 + NT * u < V) ? row[i0 + NT * u] : 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (i0 + NT * u < V) f(i0 + NT * u, x[u]);
    }
}

// a wave walks its tokens [w0, w1) in index order, 64 at a time, four loads in flight: every lane calls f(t, t < w1, x_t) in step,
// f returns true (the same in every lane) to end the walk
template <class F>
__device__ __forceinline__ void wave_walk(const float* row, int w0, int w1, F f) {
    const int lane = threadIdx.x & 63;
    for (int b0 = w0; b0 < w1; b0 += 256) {
        float x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = (b0 + 64 * u + lane < w1) ? row[b0 + 64 * u + lane] : 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (b0 + 64 * u >= w1) return;
            const int t = b0 + 64 * u + lane;
            if (f(t, t < w1, x[u])) return;
        }
    }
}

// log-sum-exp of y = x * inv over the row; every thread returns it.  fmaxf drops NaN, the exponentials do not: a row with a
// NaN, with +inf, or of -inf only has a NaN log-sum-exp.
__device__ __forceinline__ float row_lse(const float* row, int V, float inv, float* red) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float mx = -INFINITY;
    for_each_token(row, V, [&](int, float x) { mx = fmaxf(mx, __fmul_rn(x, inv)); });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    __syncthreads();
    if (lane == 0) red[wv] = mx;
    __syncthreads();
    mx = red[0];
    for (int w = 1; w < NW; ++w) mx = fmaxf(mx, red[w]);
    float sm = 0.f;
    for_each_token(row, V, [&](int, float x) { sm += expf(__fmul_rn(x, inv) - mx); });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sm += __shfl_xor(sm, o);
    __syncthreads();
    if (lane == 0) red[wv] = sm;
    __syncthreads();
    sm = red[0];
    for (int w = 1; w < NW; ++w) sm += red[w];
    return mx + logf(sm);
}

// Radix descent over the keys, best first, 8 bits per level.  BY_MASS = false: the token of rank top_k (1-based) in the order:
// found always (the caller has top_k < V).  BY_MASS = true: the token at which the inclusive mass first exceeds thr = floor(top_p
// * zk) (zk: the caller's, or the row's whole mass when have_zk is false); found = false when no mass exceeds it (zk == 0).
// Every thread of the workgroup calls it and returns the same Cut.
template <bool BY_MASS>
__device__ __forceinline__ Cut descend(const float* row, int V, const Rules& ru, Lds& L, unsigned top_k, float top_p, unsigned long long zk,
                                       bool have_zk) {
    const int tid = threadIdx.x;
    Cut c;
    c.zk = zk;
    unsigned prefix = 0;
    for (int level = 0; level < 4; ++level) {
        const int shift = 24 - 8 * level;
        __syncthreads();  // the previous level's bins are read no more
        if (tid < BINS) {
            L.cnt[tid] = 0;
            L.ms[tid] = 0;
        }
        if (tid == 0) L.sel = -1;
        __syncthreads();
        int cb = -1;  // a run of tokens of one bin is added once
        unsigned cc = 0;
        unsigned long long cm = 0;
        for_each_token(row, V, [&](int t, float x) {
            const float v = token_value(x, t, ru);
            const unsigned uk = ukey(v);
            if (level > 0 && (uk >> (shift + 8)) != prefix) return;
            const int b = (int)((uk >> shift) & 255u);
            if (b != cb) {
                if (cc) {
                    atomicAdd(&L.cnt[cb], cc);
                    if (cm) atomicAdd(&L.ms[cb], cm);
                }
                cb = b, cc = 0, cm = 0;
            }
            ++cc;
            cm += mass(v);
        });
        if (cc) {
            atomicAdd(&L.cnt[cb], cc);
            if (cm) atomicAdd(&L.ms[cb], cm);
        }
        __syncthreads();
        if (tid < BINS) {
            L.scnt[tid] = L.cnt[BINS - 1 - tid];
            L.sms[tid] = L.ms[BINS - 1 - tid];
        }
        __syncthreads();
        for (int o = 1; o < BINS; o <<= 1) {
            unsigned ac = 0;
            unsigned long long am = 0;
            if (tid < BINS && tid >= o) ac = L.scnt[tid - o], am = L.sms[tid - o];
            __syncthreads();
            if (tid < BINS) L.scnt[tid] += ac, L.sms[tid] += am;
            __syncthreads();
        }
        if (BY_MASS && level == 0) {
            if (!have_zk) c.zk = L.sms[BINS - 1];
            c.thr = (unsigned long long)floor((double)top_p * (double)c.zk);
        }
        if (tid < BINS) {
            bool here, before = false;
            if (BY_MASS) {
                here = c.mass_gt + L.sms[tid] > c.thr;
                if (tid > 0) before = c.mass_gt + L.sms[tid - 1] > c.thr;
            } else {
                here = c.cnt_gt + L.scnt[tid] >= top_k;
                if (tid > 0) before = c.cnt_gt + L.scnt[tid - 1] >= top_k;
            }
            if (here && !before) L.sel = tid;
        }
        __syncthreads();
        const int sel = L.sel;
        if (sel < 0) return c;  // (first level only: the deeper levels split a bin that crossed)
        const int b = BINS - 1 - sel;
        c.cnt_gt += L.scnt[sel] - L.cnt[b];
        c.mass_gt += L.sms[sel] - L.ms[b];
        c.cnt_eq = L.cnt[b];
        c.mass_eq = L.ms[b];
        prefix = (prefix << 8) | (unsigned)b;
    }
    c.key = prefix;
    c.found = true;
    return c;
}

// kept mass of token t (0 when it is not kept); every lane of the wave calls it in step (ballot).  tr: members of the boundary
// run in front of this wave iteration, advanced here.
__device__ __forceinline__ unsigned long long kept_mass(bool in, float v, bool filt, bool partial, unsigned tkey, unsigned ctie, unsigned& tr) {
    const unsigned uk = ukey(v);
    const bool tie = in && filt && uk == tkey;
    const unsigned long long bal = __ballot(tie);
    const unsigned rank = tr + (unsigned)__popcll(bal & ((1ull << (threadIdx.x & 63)) - 1ull));
    tr += (unsigned)__popcll(bal);
    const bool kept = in && (!filt || uk > tkey || (tie && (!partial || rank < ctie)));
    return kept ? mass(v) : 0ull;
}

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&out)[4]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        if (i > 0) k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0, c1 = lo1, c2 = n2, c3 = lo0;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

__global__ __launch_bounds__(NT) void sample_rows_kernel(SampleArgs a) {
    __shared__ Lds L;
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (a.finished && a.finished[r]) return;
    float* row = a.logits + (int64_t)r * a.ld;
    const int V = a.V;
    Rules ru;
    ru.inv = 1.0f / a.temperature, ru.unk_penalty = a.unk_penalty;
    ru.no_eos = a.no_eos, ru.force_eos = a.force_eos, ru.pad_idx = a.pad_idx, ru.eos_idx = a.eos_idx, ru.unk_idx = a.unk_idx;
    ru.lse = row_lse(row, V, ru.inv, L.red);
    // step processors: block, do not renormalise (every thread is past its reads for the log-sum-exp); not on the forced-EOS step
    if (a.seqs_in && !a.force_eos) {
        const int* seq = a.seqs_in + (int64_t)r * a.seq_ld;
        const int S = a.S, G = a.G;
        if (G > 0 && G < S) {  // NGramRepeatBlockProcessor(G), as beam_candidates_body
            const int* tail = seq + S - (G - 1);
            for (int j = tid; j + G <= S; j += NT) {
                bool same = true;
                for (int e = 0; e + 1 < G; ++e) same = same && (seq[j + e] == tail[e]);
                const int t = seq[j + G - 1];
                if (same && t >= 0 && t < V) row[t] = -INFINITY;
            }
        }
        if (a.banned.n > 0) banned_block_row(row, V, seq, S, a.banned, L.tail);  // (its strides of 256 cover the list several times: same stores)
        __syncthreads();
    }

    // ---- kept set: keys above tkey, and the first ctie tokens of key tkey ------------------------------------------------
    bool filt = false;
    unsigned tkey = 0, ctie = 0, cnt_gt = 0, cnt_eq = 0;
    unsigned long long zk = 0;
    const bool use_k = a.top_k > 0 && a.top_k < V;
    if (use_k) {
        const Cut c = descend<false>(row, V, ru, L, (unsigned)a.top_k, 1.f, 0, false);
        tkey = c.key, cnt_gt = c.cnt_gt, cnt_eq = c.cnt_eq, ctie = (unsigned)a.top_k - c.cnt_gt;
        zk = c.mass_gt + (unsigned long long)ctie * (c.mass_eq / c.cnt_eq);  // one key, one mass
        filt = true;
    }
    if (a.top_p < 1.f) {
        const Cut c = descend<true>(row, V, ru, L, 0, a.top_p, zk, use_k);
        if (c.found) {
            // token j of the boundary run stays iff mass_gt + j * w <= thr; the run's mass exceeds thr - mass_gt, so w > 0
            const unsigned long long w = c.mass_eq / c.cnt_eq, j = (c.thr - c.mass_gt) / w + 1;
            const unsigned cp = j < c.cnt_eq ? (unsigned)j : c.cnt_eq;
            if (!filt || c.key > tkey) {
                tkey = c.key, cnt_gt = c.cnt_gt, cnt_eq = c.cnt_eq, ctie = cp;
            } else if (c.key == tkey) {
                ctie = min(ctie, cp);
            }
            filt = true;
        }
    }
    const bool partial = filt && ctie < cnt_eq;
    const unsigned kept_count = filt ? cnt_gt + ctie : (unsigned)V;

    // ---- draw in index order: wave wv owns tokens [w0, w1) -----------------------------------------------------------------
    const int span = ((V + NW - 1) / NW + 63) & ~63;
    const int w0 = min(V, wv * span), w1 = min(V, w0 + span);
    unsigned tie_base = 0;
    if (partial) {  // members of the boundary run in front of this wave's span
        unsigned n = 0;
        wave_walk(row, w0, w1, [&](int t, bool in, float x) {
            n += (unsigned)__popcll(__ballot(in && ukey(token_value(x, t, ru)) == tkey));
            return false;
        });
        if (lane == 0) L.wties[wv] = n;
        __syncthreads();
        for (int w = 0; w < wv; ++w) tie_base += L.wties[w];
    }
    {
        unsigned long long acc = 0;
        unsigned tr = tie_base;
        wave_walk(row, w0, w1, [&](int t, bool in, float x) {
            acc += kept_mass(in, in ? token_value(x, t, ru) : -INFINITY, filt, partial, tkey, ctie, tr);
            return false;
        });
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += shfl_xor64(acc, o);
        if (lane == 0) L.wmass[wv] = acc;
        if (tid == 0) L.pick = -1;
        __syncthreads();
    }
    unsigned long long Z = 0;
    for (int w = 0; w < NW; ++w) Z += L.wmass[w];
    if (Z > 0) {
        const unsigned long long st = a.stream ? a.stream[r] : (unsigned long long)r;
        const int pos = a.position ? a.position[r] : a.pos;
        unsigned o[4];
        philox4x32_10((unsigned)st, (unsigned)(st >> 32), (unsigned)(a.gen ? a.gen[r] : 0), (unsigned)pos, (unsigned)a.seed,
                      (unsigned)(a.seed >> 32), o);
        const unsigned long long R = ((unsigned long long)(o[0] >> 8) * Z) >> 24;  // < Z <= 2^36 (1 + eps): the product fits
        unsigned long long before = 0;
        int wc = 0;
        while (wc < NW - 1 && before + L.wmass[wc] <= R) before += L.wmass[wc++];  // R < Z: ends inside the waves
        if (wv == wc) {
            const unsigned long long Rw = R - before;
            unsigned long long run = 0;
            unsigned tr = tie_base;
            wave_walk(row, w0, w1, [&](int t, bool in, float x) {
                unsigned long long inc = kept_mass(in, in ? token_value(x, t, ru) : -INFINITY, filt, partial, tkey, ctie, tr);
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const unsigned long long up = shfl_up64(inc, d);
                    if (lane >= d) inc += up;
                }
                const unsigned long long tot = shfl64(inc, 63);
                if (run + tot > Rw) {
                    const unsigned long long bal = __ballot(run + inc > Rw);
                    if (lane == __ffsll((long long)bal) - 1) L.pick = t;
                    return true;
                }
                run += tot;
                return false;
            });
        }
    } else {
        // no kept token has a mass: the first token of the order (highest key, lowest index)
        unsigned bk = 0;
        int bi = 0x7fffffff;
        for_each_token(row, V, [&](int t, float x) {
            const unsigned uk = ukey(token_value(x, t, ru));
            if (uk > bk || (uk == bk && t < bi)) bk = uk, bi = t;
        });
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned ok = __shfl_xor(bk, o);
            const int oi = __shfl_xor(bi, o);
            if (ok > bk || (ok == bk && oi < bi)) bk = ok, bi = oi;
        }
        if (lane == 0) L.wkey[wv] = bk, L.widx[wv] = bi;
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < NW; ++w)
                if (L.wkey[w] > bk || (L.wkey[w] == bk && L.widx[w] < bi)) bk = L.wkey[w], bi = L.widx[w];
            L.pick = bi;
        }
    }
    __syncthreads();
    if (tid == 0) {
        // a token of the row: every key is above the initial one, and R < Z ends the walk on a kept token (the next step's
        // embedding reads emb + tok * M: nothing outside the vocabulary leaves this kernel)
        const int tk = (unsigned)L.pick < (unsigned)V ? L.pick : a.eos_idx;
        const float v = token_value(row[tk], tk, ru);
        if (a.tok) a.tok[r] = tk;
        if (a.lprob) a.lprob[r] = v;
        if (a.kept) a.kept[r] = (int)kept_count;
        if (a.z_kept) a.z_kept[r] = Z;
        if (a.seqs) {
            const int pos = a.position ? a.position[r] : a.pos;
            a.seqs[(int64_t)r * a.seq_ld + pos] = tk;
            a.next_tok[r] = tk;
            a.cum[r] += v;
            a.step_lprob[(int64_t)r * a.seq_ld + pos] = v;
            if (tk == a.eos_idx) {
                a.finished[r] = 1;
                a.out_len[r] = pos + 1;
                atomicSub(a.remaining, 1);
            }
        }
    }
}

__global__ __launch_bounds__(NT) void sample_prompt_lprob_kernel(const float* __restrict__ logits, int64_t ld, int V, int row_stride, int token,
                                                                 float inv, float* __restrict__ out) {
    __shared__ float red[NW];
    const float* row = logits + (int64_t)blockIdx.x * row_stride * ld;
    const float lse = row_lse(row, V, inv, red);
    if (threadIdx.x == 0) out[blockIdx.x] += __fmul_rn(row[token], inv) - lse;
}

}  // namespace

void launch_sample_rows(const SampleArgs& a, hipStream_t s) {
    SC_CHECK(a.logits && a.rows >= 1 && a.V >= 1 && a.ld >= a.V, "sample: bad shape (rows=%d V=%d ld=%lld)", a.rows, a.V, (long long)a.ld);
    SC_CHECK(a.temperature > 0.f && std::isfinite(a.temperature), "sample: temperature %g (must be positive and finite)", (double)a.temperature);
    SC_CHECK(a.top_k >= 0, "sample: top_k %d", a.top_k);
    SC_CHECK(a.top_p > 0.f && a.top_p <= 1.f, "sample: top_p %g (0 < top_p <= 1)", (double)a.top_p);
    SC_CHECK(a.eos_idx >= 0 && a.eos_idx < a.V, "sample: eos_idx %d outside the vocabulary of %d", a.eos_idx, a.V);
    if (a.seqs_in) {
        SC_CHECK(a.G >= 0 && a.S >= 0 && a.S <= a.seq_ld, "sample: %d tokens in rows of %d (n-gram size %d)", a.S, a.seq_ld, a.G);
        if (a.banned.n > 0)
            SC_CHECK(a.banned.tokens && a.banned.offsets && a.banned.n <= BANNED_MAX_SEQS && a.banned.max_len >= 1 && a.banned.max_len <= BANNED_MAX_LEN,
                     "banned sequences: bad device list (n=%d max_len=%d)", a.banned.n, a.banned.max_len);
    }
    if (a.seqs)
        SC_CHECK(!a.position && a.pos >= 0 && a.pos < a.seq_ld && a.next_tok && a.cum && a.step_lprob && a.finished && a.out_len && a.remaining,
                 "sample: incomplete loop state (position %d in rows of %d)", a.pos, a.seq_ld);
    hipLaunchKernelGGL(sample_rows_kernel, dim3(a.rows), dim3(NT), 0, s, a);
    SC_LAUNCH_CHECK();
}

void launch_sample_prompt_lprob(const float* logits, int64_t ld, int rows, int V, int row_stride, int token, float temperature, float* out,
                                hipStream_t s) {
    SC_CHECK(token >= 0 && token < V, "sample_prompt_lprob: token %d out of range", token);
    hipLaunchKernelGGL(sample_prompt_lprob_kernel, dim3(rows), dim3(NT), 0, s, logits, ld, V, row_stride, token, 1.0f / temperature, out);
    SC_LAUNCH_CHECK();
}

}  // namespace sc
