// Cross-attention capture of the greedy decoder step (sc_generate_text_capture, the Transcriber's word timestamps).
// One extra launch after a step of the row-group chain: the last decoder layer's encoder-decoder attention probabilities of
// every live row, summed over the heads, and the log-probability of the token the step chose.  The step's own kernels are
// untouched: dattn_kernel<CROSS> never materialises normalised probabilities (online soft-max across 64-key trips), so
// this kernel recomputes the scores from the same inputs (the projected query rows the step left in StepCtx::qkvr and the
// encoder keys of the last layer) in the same arithmetic order.
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

}  // namespace sc
