// Cross-attention capture of the greedy decoder step (sc_generate_text_capture, the Transcriber's word timestamps).
// One extra launch after a step of the row-group chain: the last decoder layer's encoder-decoder attention probabilities of
// every live row, summed over the heads, and the log-probability of the token the step chose.  The step's own kernels are
// untouched: dattn_kernel<CROSS> never materialises normalised probabilities (online soft-max across 64-key trips), so
// this kernel recomputes the scores from the same inputs (the projected query rows the step left in StepCtx::qkvr and the
// encoder keys of the last layer) in the same arithmetic order.
//
// Cross-attention rows of a whole teacher-forced pass (sc_score_text_capture, Transcriber.align): the same quantity for KNOWN
// tokens, every position of every item in one launch - xattn_rows_kernel below.  One workgroup owns XROWS_QT query positions
// of one item; a key row staged in LDS serves the whole tile.  Arithmetic order, all fp32:
//   score(p, h, j) = (fmaf chain over the 64 head columns in column order, from 0) * 0.125
//   per (p, h): every lane l keeps a running max / sum over its own keys j = l, l + 64, ... in key order (online soft-max:
//     sum = sum * expf(max - new_max) + expf(score - new_max)); the 64 lanes combine as max by xor-butterfly, each sum
//     rescaled to the row max once (sum * expf(lane_max - row_max)), then added by xor-butterfly 32, 16, 8, 4, 2, 1
//   xattn[b][p][j] = ((0 + P_0) + P_1) + ... + P_{heads-1} with P_h = expf(score - row_max_h) / row_sum_h: one thread owns
//     the element and adds the heads in head order (no atomics).
// Nothing above depends on n, on the padded S1 / s_enc or on another item: the key loop of the statistics runs to the item's
// own encoder length.  Not bit-equal to the greedy capture: that one sums a score as 16 lanes x 4 columns + butterfly, and
// its queries come from the row-group products instead of the tiled ones.
#include "kernels.h"

namespace sc {

// key columns staged in LDS per pass of the head sum: XCAP_MAX_HEADS x XCAP_CHUNK floats (32 KB); a longer encoder
// output (a 40 s input is ~250 positions at full size) runs several chunks
constexpr int XCAP_CHUNK = 512;

// scores of the 64 keys j0 .. j0+63 of one (row, head) pair: 16 lanes hold one 64-wide key row as float4, the four
// 16-lane groups take keys j, j+1, j+2, j+3 (dattn_kernel's layout and summation order); keys at or behind kv_len -> -inf
__device__ __forceinline__ void xcap_trip(const float* __restrict__ kc, int64_t ld, int j0, int kv_len, int g, float4 q4,
                                          float (&sc)[16]) {
    float4 kreg[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) kreg[i] = *reinterpret_cast<const float4*>(kc + (int64_t)min(j0 + 4 * i + g, kv_len - 1) * ld);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float4 kv = kreg[i];
        float d = 0.f;
        d = fmaf(q4.x, kv.x, d);
        d = fmaf(q4.y, kv.y, d);
        d = fmaf(q4.z, kv.z, d);
        d = fmaf(q4.w, kv.w, d);
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) d += __shfl_xor(d, off);
        sc[i] = (j0 + 4 * i + g < kv_len) ? d * 0.125f : -INFINITY;
    }
}

// One workgroup per row slot, one wave per head (at least four waves: the arg-max records are combined by 256 threads in
// argmax_finalize_kernel's order).  Pass 1: running max and sum of the row's scores per head.  Pass 2, per chunk of keys:
// each wave writes its probabilities to LDS, then the heads are summed in head order (no atomics: deterministic).
__global__ __launch_bounds__(1024) void xattn_capture_kernel(XattnCapArgs p) {
    __shared__ float s_p[XCAP_MAX_HEADS * XCAP_CHUNK];
    __shared__ float s_v[4], s_m[4], s_s[4];
    __shared__ int s_i[4];
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, hd = tid >> 6;
    const int pos = *p.d_pos - 1;  // the step has advanced the position counter already
    if (pos < 0 || pos >= p.cap) return;
    if (p.d_rows && b >= *p.d_rows) return;                   // behind the live rows (compaction): nothing was computed
    if (p.finished[b] && p.out_len[b] != pos + 2) return;     // finished at an earlier step: this step fed it padding
    const int utt = p.slot_utt[b];
    const int M = p.heads * 64;
    const int64_t ld = 2 * (int64_t)M;
    const int kv_len = min(p.enc_lens[b], p.s_enc);
    const int c = lane & 15, g = lane >> 4;
    const bool head = hd < p.heads;
    float4 q4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const float* kc = p.kv + (int64_t)b * p.s_enc * ld + hd * 64 + 4 * c;
    float m_run = -INFINITY, l_run = 0.f;
    if (head) {
        q4 = *reinterpret_cast<const float4*>(p.q + (int64_t)b * M + hd * 64 + 4 * c);
        for (int j0 = 0; j0 < kv_len; j0 += 64) {
            float sc[16];
            xcap_trip(kc, ld, j0, kv_len, g, q4, sc);
            float mx = -INFINITY;
#pragma unroll
            for (int i = 0; i < 16; ++i) mx = fmaxf(mx, sc[i]);
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float m_new = fmaxf(m_run, mx);  // finite: every trip holds at least one valid key
            const float alpha = expf(m_run - m_new);
            float ls = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) ls += expf(sc[i] - m_new);
            l_run = l_run * alpha + ls;
            m_run = m_new;
        }
        l_run += __shfl_xor(l_run, 16);
        l_run += __shfl_xor(l_run, 32);
    }
    float* out = p.xattn + ((int64_t)utt * p.cap + pos) * p.s_enc;
    for (int cb = 0; cb < p.s_enc; cb += XCAP_CHUNK) {
        const int cend = min(cb + XCAP_CHUNK, p.s_enc);
        if (head) {
            for (int j0 = cb; j0 < cend; j0 += 64) {
                float sc[16];
                if (j0 < kv_len) xcap_trip(kc, ld, j0, kv_len, g, q4, sc);
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int j = j0 + 4 * i + g;
                    if (c == 0 && j < cend) s_p[hd * XCAP_CHUNK + (j - cb)] = j < kv_len ? expf(sc[i] - m_run) / l_run : 0.f;
                }
            }
        }
        __syncthreads();
        for (int j = cb + tid; j < cend; j += blockDim.x) {
            float s = 0.f;
            for (int h = 0; h < p.heads; ++h) s += s_p[h * XCAP_CHUNK + (j - cb)];
            out[j] = s;
        }
        __syncthreads();
    }

    // log-probability of the chosen token: argmax_finalize_kernel's combination of the step's arg-max records
    if (!p.am_part) {  // a step without vocabulary projection (prompt position): no token was chosen
        if (tid == 0) p.lprob[(int64_t)utt * p.cap + pos] = 0.f;
        return;
    }
    // every thread of the group reaches the barrier below; the first four waves hold the records
    float best = -INFINITY, m = -INFINITY, ssum = 0.f;
    int bidx = 0x7fffffff;
    if (tid < 256) {
        const int w = tid >> 6;
        for (int t = tid; t < p.am_tiles; t += 256) {
            const float4 r = p.am_part[(int64_t)t * p.nb + b];
            const int oi = __float_as_int(r.y);
            if (r.x > best || (r.x == best && oi < bidx)) {
                best = r.x;
                bidx = oi;
            }
            const float nm = fmaxf(m, r.z);
            const float a = (m == -INFINITY) ? 0.f : ssum * expf(m - nm);
            const float e = (r.z == -INFINITY) ? 0.f : r.w * expf(r.z - nm);
            ssum = a + e;
            m = nm;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o);
            const int oi = __shfl_xor(bidx, o);
            if (ob > best || (ob == best && oi < bidx)) {
                best = ob;
                bidx = oi;
            }
            const float om = __shfl_xor(m, o);
            const float os = __shfl_xor(ssum, o);
            const float nm = fmaxf(m, om);
            const float a = (m == -INFINITY) ? 0.f : ssum * expf(m - nm);
            const float e = (om == -INFINITY) ? 0.f : os * expf(om - nm);
            ssum = a + e;
            m = nm;
        }
        if (lane == 0) {
            s_v[w] = best;
            s_i[w] = bidx;
            s_m[w] = m;
            s_s[w] = ssum;
        }
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < 4; ++k) {
            if (s_v[k] > best || (s_v[k] == best && s_i[k] < bidx)) {
                best = s_v[k];
                bidx = s_i[k];
            }
            const float nm = fmaxf(m, s_m[k]);
            const float a = (m == -INFINITY) ? 0.f : ssum * expf(m - nm);
            const float e = (s_m[k] == -INFINITY) ? 0.f : s_s[k] * expf(s_m[k] - nm);
            ssum = a + e;
            m = nm;
        }
        if (p.force_eos_step >= 0 && pos == p.force_eos_step) best = p.eos_logit[b];
        p.lprob[(int64_t)utt * p.cap + pos] = best - (m + logf(ssum));
    }
}

void launch_xattn_capture(const XattnCapArgs& a, hipStream_t s) {
    SC_CHECK(a.q && a.kv && a.enc_lens && a.d_pos && a.finished && a.out_len && a.slot_utt && a.xattn && a.lprob,
             "xattn capture: null argument");
    SC_CHECK(a.nb > 0 && a.heads >= 1 && a.heads <= XCAP_MAX_HEADS && a.s_enc > 0 && a.cap > 1, "xattn capture: nb=%d heads=%d s_enc=%d cap=%d",
             a.nb, a.heads, a.s_enc, a.cap);
    SC_CHECK(!a.am_part || (a.am_tiles > 0 && a.eos_logit), "xattn capture: arg-max records without tiles / EOS logits");
    prof::Scope scope("xattn_capture", 0.0, 0.0, s);
    hipLaunchKernelGGL(xattn_capture_kernel, dim3(a.nb), dim3(64 * std::max(4, a.heads)), 0, s, a);
    SC_LAUNCH_CHECK();
}

// ---- the whole teacher-forced pass -------------------------------------------------------------------------------------
// LDS row stride of a staged key row: 64 columns + one float4, so that the 16 lanes of a ds_read_b128 group (one key row
// each) fall on 16 different 4-bank slots
constexpr int XROWS_LD = 68;

// the workgroup's tile of one head: XROWS_QT query rows (zeros behind the live ones) and the XROWS_KC key rows from j0
// (zeros behind the item's encoder length); 256 threads, one float4 per thread and 16 rows
__device__ __forceinline__ void xrows_stage(const XattnRowsArgs& p, const float* __restrict__ qb, const float* __restrict__ kb, int h, int j0,
                                            int live, int kv_len, bool with_q, float* s_q, float* s_k) {
    const int r = threadIdx.x >> 4, c4 = 4 * (threadIdx.x & 15);
    if (with_q) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < live) v = *reinterpret_cast<const float4*>(qb + (int64_t)r * p.ldq + h * 64 + c4);
        *reinterpret_cast<float4*>(s_q + r * 64 + c4) = v;
    }
    float4 kv[XROWS_KC / 16];
#pragma unroll
    for (int i = 0; i < XROWS_KC / 16; ++i) {  // the loads first, then the stores: four rows in flight per thread
        const int j = j0 + r + 16 * i;
        kv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < kv_len) kv[i] = *reinterpret_cast<const float4*>(kb + (int64_t)j * p.ldk + h * 64 + c4);
    }
#pragma unroll
    for (int i = 0; i < XROWS_KC / 16; ++i) *reinterpret_cast<float4*>(s_k + (r + 16 * i) * XROWS_LD + c4) = kv[i];
}

// scores of key j0 + lane against the wave's four query rows 4w .. 4w+3 (-inf at or behind kv_len)
__device__ __forceinline__ float4 xrows_scores(const float* s_q, const float* s_k, int j0, int kv_len) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float4 kreg[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) kreg[i] = *reinterpret_cast<const float4*>(s_k + lane * XROWS_LD + 4 * i);
    float sc[4];
#pragma unroll
    for (int qi = 0; qi < 4; ++qi) {
        const float* qr = s_q + (4 * w + qi) * 64;  // wave-uniform: a broadcast read
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float4 q4 = *reinterpret_cast<const float4*>(qr + 4 * i);
            d = fmaf(q4.x, kreg[i].x, d);
            d = fmaf(q4.y, kreg[i].y, d);
            d = fmaf(q4.z, kreg[i].z, d);
            d = fmaf(q4.w, kreg[i].w, d);
        }
        sc[qi] = (j0 + lane < kv_len) ? d * 0.125f : -INFINITY;
    }
    return make_float4(sc[0], sc[1], sc[2], sc[3]);
}

// grid (query tiles, items), 256 threads: wave w owns query rows 4w .. 4w+3 of the tile, lane l key j0 + l of a chunk.
// Pass 1, head by head: max and sum of every (row, head) over the item's keys.  Pass 2, key chunk by key chunk: every thread
// adds the heads' probabilities of its four elements in head order and stores them; zeros behind the live rows and keys.
__global__ __launch_bounds__(256) void xattn_rows_kernel(XattnRowsArgs p) {
    __shared__ __attribute__((aligned(16))) float s_k[XROWS_KC * XROWS_LD];
    __shared__ __attribute__((aligned(16))) float s_q[XROWS_QT * 64];
    __shared__ float s_m[XCAP_MAX_HEADS * XROWS_QT], s_l[XCAP_MAX_HEADS * XROWS_QT];
    const int b = blockIdx.y, p0 = blockIdx.x * XROWS_QT;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nq = min(XROWS_QT, p.S1 - p0);                  // rows of the tile inside the buffer
    const int live = min(p.tok_lens[b] - 1, p.S1) - p0;      // of them, rows that have a target (<= 0: none)
    const int kv_len = min(p.enc_lens[b], p.s_enc);
    float* out = p.xattn + ((int64_t)b * p.S1 + p0) * p.s_enc;
    if (live <= 0 || kv_len <= 0) {  // workgroup-uniform
        for (int64_t i = tid; i < (int64_t)nq * p.s_enc; i += 256) out[i] = 0.f;
        return;
    }
    const float* qb = p.q + ((int64_t)b * p.S1 + p0) * p.ldq;
    const float* kb = p.k + (int64_t)b * p.s_enc * p.ldk;
    for (int h = 0; h < p.heads; ++h) {
        float m_t[4], l_t[4];
#pragma unroll
        for (int qi = 0; qi < 4; ++qi) m_t[qi] = -INFINITY, l_t[qi] = 0.f;
        for (int j0 = 0; j0 < kv_len; j0 += XROWS_KC) {
            __syncthreads();  // the previous tile has been read
            xrows_stage(p, qb, kb, h, j0, live, kv_len, j0 == 0, s_q, s_k);
            __syncthreads();
            const float4 s4 = xrows_scores(s_q, s_k, j0, kv_len);
            const float sc[4] = {s4.x, s4.y, s4.z, s4.w};
            if (j0 + lane < kv_len) {
#pragma unroll
                for (int qi = 0; qi < 4; ++qi) {
                    const float m_new = fmaxf(m_t[qi], sc[qi]);  // finite: this key is a valid one
                    l_t[qi] = l_t[qi] * expf(m_t[qi] - m_new) + expf(sc[qi] - m_new);
                    m_t[qi] = m_new;
                }
            }
        }
#pragma unroll
        for (int qi = 0; qi < 4; ++qi) {
            float m = m_t[qi];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
            float l = l_t[qi] * expf(m_t[qi] - m);  // a lane without a key: 0 * expf(-inf)
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) l += __shfl_xor(l, off);
            if (lane == 0) s_m[h * XROWS_QT + 4 * w + qi] = m, s_l[h * XROWS_QT + 4 * w + qi] = l;
        }
    }
    for (int j0 = 0; j0 < p.s_enc; j0 += XROWS_KC) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if (j0 < kv_len) {
            for (int h = 0; h < p.heads; ++h) {
                __syncthreads();  // the previous tile has been read; pass 1's statistics are visible
                xrows_stage(p, qb, kb, h, j0, live, kv_len, true, s_q, s_k);
                __syncthreads();
                const float4 s4 = xrows_scores(s_q, s_k, j0, kv_len);
                const float sc[4] = {s4.x, s4.y, s4.z, s4.w};
                if (j0 + lane < kv_len) {
#pragma unroll
                    for (int qi = 0; qi < 4; ++qi) acc[qi] += expf(sc[qi] - s_m[h * XROWS_QT + 4 * w + qi]) / s_l[h * XROWS_QT + 4 * w + qi];
                }
            }
        }
        const int j = j0 + lane;
        if (j < p.s_enc) {
#pragma unroll
            for (int qi = 0; qi < 4; ++qi) {
                const int r = 4 * w + qi;
                if (r < nq) out[(int64_t)r * p.s_enc + j] = r < live ? acc[qi] : 0.f;
            }
        }
    }
}

void check_xattn_rows_geometry(int heads, int model_dim, const char* who) {
    SC_CHECK(heads >= 1 && heads <= XCAP_MAX_HEADS && model_dim == heads * 64,
             "%s: %d heads over model_dim=%d (the cross-attention rows need 1..%d heads of width 64)", who, heads, model_dim, XCAP_MAX_HEADS);
}

void launch_xattn_rows(const XattnRowsArgs& a, hipStream_t s) {
    SC_CHECK(a.q && a.k && a.enc_lens && a.tok_lens && a.xattn, "xattn rows: null argument");
    SC_CHECK(a.n > 0 && a.n <= 65535 && a.S1 > 0 && a.s_enc > 0, "xattn rows: n=%d S1=%d s_enc=%d", a.n, a.S1, a.s_enc);
    check_xattn_rows_geometry(a.heads, a.heads * 64, "xattn rows");
    SC_CHECK(a.ldq >= a.heads * 64 && a.ldk >= a.heads * 64 && a.ldq % 4 == 0 && a.ldk % 4 == 0, "xattn rows: ldq=%lld ldk=%lld for %d heads",
             (long long)a.ldq, (long long)a.ldk, a.heads);
    SC_CHECK(((uintptr_t)a.q | (uintptr_t)a.k) % 16 == 0, "xattn rows: q / k must be 16-byte aligned");
    prof::Scope scope("xattn_rows", 2.0 * a.n * a.S1 * (double)a.s_enc * a.heads * 64 * 2, 0.0, s);
    hipLaunchKernelGGL(xattn_rows_kernel, dim3((a.S1 + XROWS_QT - 1) / XROWS_QT, a.n), dim3(256), 0, s, a);
    SC_LAUNCH_CHECK();
}

}  // namespace sc
