// Streaming session pool: N concurrent sessions of the monotonic decoder (sc_mma_begin / sc_mma_step, model_decoder.hip)
// share every decoder step.  The step is the row-group chain (k_dstep3.hip) in the decode engine's slot mode over
// mma_stack(m): slot b of a step works on ROW STATE slot_rp[b].x - here a SESSION - at that session's own position, on the
// session's own self K / V lane and encoder K / V lane.  What the engine's chain does not have is added here:
//   * the closing launch of a pool step (pool_close_kernel, in engine_finalize_kernel's place: positions of the taking-part
//     rows + the decoder outputs into the caller's packed rows, no generation rule);
//   * the p_choose hook for rows: every layer's normed cross-attention input of the live slots (pool_capture_ln_kernel),
//     the query-side energy MLPs with each layer's weight read once per level for all rows (energy_level_rows_kernel), and
//     p_choose per (head, layer, row) (pchoose_rows_kernel);
//   * begin for k sessions: ONE row-independent product per layer over the packed encoder rows, scattered into the lanes,
//     the per-session pooled mean and the key-side energy MLPs batched over sessions;
//   * per-row blocked fill in front of the arg-max over k rows.
// A session's arithmetic depends on nothing but its own state and feed: every product is row-independent (the chain's
// own contract, tests/test_engine_gpu.py; linear(..., row_independent) for the vocabulary projection and the encoder K / V),
// every other kernel works on one row per workgroup or walks the rows one at a time in a fixed K order.
// Reference semantics per session: streaming/agents/online_text_decoder.py:205-243, :303-387 (see sc_mma_step).
#include <cmath>
#include <cstring>

#include "dstep.h"

namespace sc {

namespace {

constexpr int POOL_MAX_BLOCKED = 32;

template <typename T>
struct Pinned {  // page-locked host staging: the copies of a call are asynchronous, the call's closing synchronisation frees it
    T* p = nullptr;
    void alloc(size_t n) { SC_HIP(hipHostMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(n, 1) * sizeof(T), hipHostMallocDefault)); }
    ~Pinned() {
        if (p) (void)hipHostFree(p);
    }
};

// ---- step ---------------------------------------------------------------------------------------------------------------
// The slot table of one step: slot s < n_live holds session recs[s].x, which feeds token recs[s].y and whose decoder output
// goes to row recs[s].z of the caller's features.  Slots behind the live ones point at session 0 (their loads stay inside the
// buffers and are discarded, as in the decode engine).
__global__ __launch_bounds__(256) void pool_set_slots_kernel(const int4* __restrict__ recs, int n_live, int slots, int2* __restrict__ slot_rp,
                                                             int* __restrict__ slot_lane, int* __restrict__ tok, const int* __restrict__ pos_row,
                                                             int* __restrict__ feat_row, int* __restrict__ d_rows) {
    for (int s = threadIdx.x; s < slots; s += 256) {
        int2 v = make_int2(0, 0);
        int lane = 0, fr = 0;
        if (s < n_live) {
            const int4 rec = recs[s];
            v.x = rec.x;
            v.y = pos_row[rec.x];
            lane = rec.x;
            fr = rec.z;
            tok[rec.x] = rec.y;
        }
        slot_rp[s] = v;
        slot_lane[s] = lane;
        feat_row[s] = fr;
    }
    if (threadIdx.x == 0) *d_rows = n_live;
}

__global__ __launch_bounds__(256) void pool_close_kernel(const float* __restrict__ hN, const int2* __restrict__ slot_rp, const int* __restrict__ d_rows,
                                                         int* __restrict__ pos_row, const int* __restrict__ feat_row, float* __restrict__ features,
                                                         int M) {
    const int b = blockIdx.x;
    if (b >= *d_rows) return;
    const int2 rp = slot_rp[b];
    const float4* src = reinterpret_cast<const float4*>(hN + (int64_t)b * M);
    float4* dst = reinterpret_cast<float4*>(features + (int64_t)feat_row[b] * M);
    for (int c = threadIdx.x; c < (M >> 2); c += 256) dst[c] = src[c];
    if (threadIdx.x == 0) pos_row[rp.x] = rp.y + 1;
}

// LayerNorm of one row of the k-group-major residual stream as an fp32 row; ln3_kernel's arithmetic, expression by expression
__global__ __launch_bounds__(256) void pool_capture_ln_kernel(const float* __restrict__ xg, int XRB, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float* __restrict__ out, int C,
                                                              const int* __restrict__ d_rows) {
    __shared__ float red[8];
    const int row = blockIdx.x, tid = threadIdx.x;
    if (row >= *d_rows) return;  // block-uniform: nobody is left behind at the barriers below
    const bool on = tid < (C >> 2);
    const int t = on ? tid : 0;
    const float4 a = *reinterpret_cast<const float4*>(xg + ((int64_t)(t >> 1) * XRB + row) * 8 + (t & 1) * 4);
    const float4 g = reinterpret_cast<const float4*>(gamma)[t];
    const float4 be = reinterpret_cast<const float4*>(beta)[t];
    float s = on ? (a.x + a.y) + (a.z + a.w) : 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    const float mean = ((red[0] + red[1]) + (red[2] + red[3])) / (float)C;
    float q = 0.f;
    if (on) {
        const float d0 = a.x - mean, d1 = a.y - mean, d2 = a.z - mean, d3 = a.w - mean;
        q = (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    if ((tid & 63) == 0) red[4 + (tid >> 6)] = q;
    __syncthreads();
    const float rstd = 1.0f / sqrtf(((red[4] + red[5]) + (red[6] + red[7])) / (float)C + 1e-5f);
    if (!on) return;
    reinterpret_cast<float4*>(out + (int64_t)row * C)[tid] =
        make_float4((a.x - mean) * rstd * g.x + be.x, (a.y - mean) * rstd * g.y + be.y, (a.z - mean) * rstd * g.z + be.z,
                    (a.w - mean) * rstd * g.w + be.w);
}

// One level of the EnergyProjection of EVERY layer for `rows` rows in one launch:
//   out[l][map(r)][n] = relu(b[l][n] + W[l][n][:] . in[l][r][:])        fp16 weights, fp32 arithmetic.
// energy_level_kernel (model_dstep.hip) made weight-stationary: grid (M / 32, layers), a wave owns 8 output features and
// loads their 16 weight vectors (8 features x 2 K halves of 512) ONCE, then walks the rows - a layer's weight is read once per
// level whatever the row count.  Per row the sum is that kernel's: the same 16 products per lane in the same order, the same
// wave reduction by shuffles, so a row's bits depend on nothing but the row.
struct EnergyRowsArgs {
    const __half* const* Wt;
    const float* const* Bt;
    int ldw;
    const float* in;
    int64_t in_ls, in_rs;  // layer / row stride of `in` (in_ls = 0: every layer reads the same rows)
    float* out;
    int64_t out_ls, out_rs;
    const int* row_map;  // row r is written to row row_map[r] of `out` (null: r)
    int M, rows;
};
__global__ __launch_bounds__(256) void energy_level_rows_kernel(EnergyRowsArgs p) {
    typedef _Float16 h8_t __attribute__((ext_vector_type(8)));
    const int l = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = blockIdx.x * 32 + wave * 8, M = p.M;
    const __half* W = p.Wt[l];
    const float* bias = p.Bt[l];
    h8_t w[8][2];
    float bv[8];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int k = c * 512 + lane * 8;
#pragma unroll
        for (int f = 0; f < 8; ++f) {
            h8_t z;
#pragma unroll
            for (int e = 0; e < 8; ++e) z[e] = (_Float16)0.f;
            w[f][c] = (k < M && n0 + f < M) ? *reinterpret_cast<const h8_t*>(W + (int64_t)(n0 + f) * p.ldw + k) : z;
        }
    }
#pragma unroll
    for (int f = 0; f < 8; ++f) bv[f] = (bias && n0 + f < M) ? bias[n0 + f] : 0.f;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int r = 0; r < p.rows; ++r) {
        const float* x = p.in + (int64_t)l * p.in_ls + (int64_t)r * p.in_rs;
        float xv[2][8];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int k = c * 512 + lane * 8;  // M is a multiple of 8: k < M covers k + 7
            const float4 a = k < M ? *reinterpret_cast<const float4*>(x + k) : zero;
            const float4 b = k < M ? *reinterpret_cast<const float4*>(x + k + 4) : zero;
            xv[c][0] = a.x, xv[c][1] = a.y, xv[c][2] = a.z, xv[c][3] = a.w;
            xv[c][4] = b.x, xv[c][5] = b.y, xv[c][6] = b.z, xv[c][7] = b.w;
        }
        float* o = p.out + (int64_t)l * p.out_ls + (int64_t)(p.row_map ? p.row_map[r] : r) * p.out_rs;
#pragma unroll
        for (int f = 0; f < 8; ++f) {
            float acc = 0.f;
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int e = 0; e < 8; ++e) acc = fmaf((float)w[f][c][e], xv[c][e], acc);
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s);
            if (lane == 0 && n0 + f < M) {
                const float v = acc + bv[f];
                o[n0 + f] = !(v <= 0.f) ? v : 0.f;  // NaN stays NaN
            }
        }
    }
}

// p_choose of every (head, layer, row): pchoose_all_kernel's arithmetic; row r's key-side energies are its session's
__global__ void pchoose_rows_kernel(const float* __restrict__ q, int64_t q_ls, const float* __restrict__ kenergy, const int2* __restrict__ slot_rp,
                                    int M, int head_dim, const float* const* __restrict__ energy_bias, float temperature,
                                    float* __restrict__ out) {
    const int h = blockIdx.x, l = blockIdx.y, r = blockIdx.z, lane = threadIdx.x, H = gridDim.x, L = gridDim.y;
    const int sid = slot_rp[r].x;
    const float* ql = q + (int64_t)l * q_ls + (int64_t)r * M + h * head_dim;
    const float* kl = kenergy + ((int64_t)sid * L + l) * M + h * head_dim;
    float acc = 0.f;
    for (int c = lane; c < head_dim; c += 64) acc = fmaf(ql[c], kl[c], acc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) {
        float e = acc * rsqrtf((float)head_dim);
        if (energy_bias[l]) e += energy_bias[l][0];
        out[((int64_t)r * L + l) * H + h] = 1.f / (1.f + expf(-(e / temperature)));
    }
}

// logits[b][blocked[b][i]] = -inf for i < n_blocked[b] (online_text_decoder.py:226-229), one workgroup per row
__global__ void pool_fill_blocked_kernel(float* __restrict__ logits, int64_t ld, int V, const int* __restrict__ blocked,
                                         const int* __restrict__ n_blocked) {
    const int b = blockIdx.x, i = threadIdx.x;
    if (i >= min(n_blocked[b], POOL_MAX_BLOCKED)) return;
    const int idx = blocked[b * POOL_MAX_BLOCKED + i];
    if (idx >= 0 && idx < V) logits[(int64_t)b * ld + idx] = -INFINITY;
}

// ---- begin --------------------------------------------------------------------------------------------------------------
// Session j of the call (rows offs[j] .. + s_enc[j] of the packed encoder output): the mean of its LAST pooled source position -
// AvgPool1d(kernel = stride = ratio, ceil_mode=True), a clipped window divided by the positions it really covers
// (p_choose.py:114-118; mean_rows_kernel's sum) - and its row state: position 0, the new encoder length.
__global__ __launch_bounds__(256) void pool_begin_rows_kernel(const int* __restrict__ sids, const int* __restrict__ s_enc, const int* __restrict__ offs,
                                                              const float* __restrict__ enc, int ratio, int M, float* __restrict__ pooled,
                                                              int* __restrict__ pos_row, int* __restrict__ enc_lens) {
    const int j = blockIdx.x, se = s_enc[j];
    const int start = ((se + ratio - 1) / ratio - 1) * ratio, count = se - start;
    const float* rows = enc + (int64_t)(offs[j] + start) * M;
    for (int c = threadIdx.x; c < M; c += 256) {
        float acc = 0.f;
        for (int t = 0; t < count; ++t) acc += rows[(int64_t)t * M + c];
        pooled[(int64_t)j * M + c] = acc / (float)count;
    }
    if (threadIdx.x == 0) {
        pos_row[sids[j]] = 0;
        enc_lens[sids[j]] = se;
    }
}

// rows offs[j] + t (t < s_enc[j]) of the packed K | V product -> row t of session sids[j]'s lane; grid (longest s_enc, k)
__global__ __launch_bounds__(256) void pool_scatter_cross_kernel(const float* __restrict__ packed, const int* __restrict__ sids,
                                                                 const int* __restrict__ s_enc, const int* __restrict__ offs, int lane_rows,
                                                                 int W, float* __restrict__ lanes) {
    const int t = blockIdx.x, j = blockIdx.y;
    if (t >= s_enc[j]) return;
    const float4* src = reinterpret_cast<const float4*>(packed + (int64_t)(offs[j] + t) * W);
    float4* dst = reinterpret_cast<float4*>(lanes + ((int64_t)sids[j] * lane_rows + t) * W);
    for (int c = threadIdx.x; c < (W >> 2); c += 256) dst[c] = src[c];
}

}  // namespace

void launch_pool_close(const float* hN, const int2* slot_rp, const int* d_rows, int* pos_row, const int* feat_row, float* features,
                       int slots, int M, hipStream_t s) {
    SC_CHECK(hN && slot_rp && d_rows && pos_row && feat_row && features && slots > 0 && M % 4 == 0, "pool close: bad argument");
    hipLaunchKernelGGL(pool_close_kernel, dim3(slots), dim3(256), 0, s, hN, slot_rp, d_rows, pos_row, feat_row, features, M);
    SC_LAUNCH_CHECK();
}

void launch_pool_capture_ln(const float* xg, int XRB, const float* gamma, const float* beta, float* out, int slots, int M,
                            const int* d_rows, hipStream_t s) {
    SC_CHECK(xg && out && d_rows && slots > 0 && XRB >= slots && M % 8 == 0 && M <= 1024, "pool capture: slots=%d RB=%d M=%d", slots, XRB, M);
    hipLaunchKernelGGL(pool_capture_ln_kernel, dim3(slots), dim3(256), 0, s, xg, XRB, gamma, beta, out, M, d_rows);
    SC_LAUNCH_CHECK();
}

struct MmaPool {
    Model& m;
    int S = 0, cap = 0, se_cap = 0, L = 0, M = 0, H = 0, V = 0, E = 0;
    int64_t ldl = 0;  // row stride of the logits
    DecStack W;
    StepCtx c;
    PoolStep hook;
    StepScratch scratch;
    Buf<int> ints, blk;
    Buf<int4> table;
    Buf<float> kenergy, hq, qe0, qe1, pooled, logits, pch, xtmp;
    std::vector<Buf<float>> caches;
    // slices of `ints`
    int *d_rows = nullptr, *feat_row = nullptr, *out_idx = nullptr, *b_sids = nullptr, *b_senc = nullptr, *b_offs = nullptr, *n_blk = nullptr;
    Pinned<int4> h_table;
    Pinned<int> h_ints;  // begin: sids | s_enc | offs;  step: n_blocked | blocked | out_idx
    Pinned<float> h_pch;
    std::vector<int> pos, s_enc;  // host mirror of the row states; s_enc 0: the session never began
    sc_mma_pool_stats st{};
    explicit MmaPool(Model& mm) : m(mm) {}

    void energy_levels(const __half* const* Wt, const float* const* Bt, const float* in, int64_t in_ls, int rows, float* last, int64_t last_ls,
                       int64_t last_rs, const int* last_map);
};

// the E levels of an energy MLP of every layer for `rows` rows; the last level is written to `last`
void MmaPool::energy_levels(const __half* const* Wt, const float* const* Bt, const float* in, int64_t in_ls, int rows, float* last,
                            int64_t last_ls, int64_t last_rs, const int* last_map) {
    EnergyRowsArgs a{};
    a.ldw = m.mma_qe_ldw, a.M = M, a.rows = rows;
    a.in = in, a.in_ls = in_ls, a.in_rs = M;
    for (int e = 0; e < E; ++e) {
        const bool fin = e + 1 == E;
        a.Wt = Wt + (size_t)e * L, a.Bt = Bt + (size_t)e * L;
        a.out = fin ? last : ((e & 1) ? qe1.get() : qe0.get());
        a.out_ls = fin ? last_ls : (int64_t)S * M, a.out_rs = fin ? last_rs : M, a.row_map = fin ? last_map : nullptr;
        hipLaunchKernelGGL(energy_level_rows_kernel, dim3(cdiv(M, 32), L), dim3(256), 0, m.stream, a);
        SC_LAUNCH_CHECK();
        a.in = a.out, a.in_ls = (int64_t)S * M;
    }
}

MmaPool* mma_pool_create(Model& m, const sc_mma_pool_opts& o) {
    const sc_config& cfg = m.cfg;
    const int S = o.sessions, cap = o.max_len, se = o.s_enc_cap, M = cfg.model_dim, L = cfg.mma_layers;
    SC_CHECK(L > 0 && !m.mma_dec.empty(), "sc_mma_pool_create: the model was loaded without a monotonic decoder");
    SC_CHECK(S >= 1 && S <= 512, "sc_mma_pool_create: sessions=%d outside 1..512", S);
    SC_CHECK(cap >= 2 && cap <= cfg.text_max_seq_len && cap <= 4096, "sc_mma_pool_create: max_len=%d outside 2..min(%d, 4096)", cap,
             cfg.text_max_seq_len);
    SC_CHECK(se >= 1 && se <= 4096, "sc_mma_pool_create: s_enc_cap=%d outside 1..4096", se);
    std::unique_ptr<MmaPool> P(new MmaPool(m));
    P->W = mma_stack(m);
    const DecStack& W = P->W;
    const bool narrow = S <= 64 && step2_eligible(m, W, S) && step3_eligible(m, W, S);
    const bool wide = S > 64 && step3_wide_eligible(m, W, S);
    SC_CHECK((narrow || wide) && m.mma_qe_w && m.mma_ke_w && M <= 1024 && M % 8 == 0 && cfg.mma_energy_layers >= 1,
             "sc_mma_pool_create: the row-group step chain does not take this model at %d sessions", S);
    P->S = S, P->cap = cap, P->se_cap = se, P->L = L, P->M = M, P->H = cfg.num_heads, P->V = cfg.text_vocab_size, P->E = cfg.mma_energy_layers;
    P->ldl = align_up(P->V, 4);
    prof::set_tag("mma");
    StepCtx& c = P->c;
    c.nb = S, c.cap = cap, c.s_enc = se;
    c.stack = &P->W;
    c.pool = &P->hook;
    // ints: [0] unused scalar position | [1] live slots | [8 ..) slot_rp | slot_lane | feat_row | tok | pos | enc_lens | out_idx |
    //       begin: sids | s_enc | offs [S + 1] | n_blocked
    const size_t n_ints = 16 + (size_t)12 * S;
    P->ints = Buf<int>(m.pp(), n_ints);
    SC_HIP(hipMemsetAsync(P->ints.get(), 0, n_ints * 4, m.stream));
    int* p = P->ints.get();
    c.d_pos = p;
    P->d_rows = p + 1;
    c.d_rows = P->d_rows;
    p += 8;
    c.slot_rp = reinterpret_cast<int2*>(p), p += 2 * S;
    c.slot_lane = p, p += S;
    P->feat_row = p, p += S;
    c.d_tok = p, p += S;
    c.pos_row = p, p += S;
    c.d_enc_lens = p, p += S;
    P->out_idx = p, p += S;
    P->b_sids = p, p += S;
    P->b_senc = p, p += S;
    P->b_offs = p, p += S + 1;
    P->n_blk = p, p += S;
    P->hook.feat_row = P->feat_row;
    StepTuning tune;
    if (S > 128) tune.rg_small = 32;  // as the decode engine: same bits whatever the grouping (tests/test_dstep3_gpu.py)
    init_chain_scratch(m, P->scratch, c, W, S, S > 64 ? 4 : 3, tune);
    for (int li = 0; li < L; ++li) {
        P->caches.emplace_back(m.pp(), (size_t)S * cap * M);
        c.kcache.push_back(P->caches.back());
        P->caches.emplace_back(m.pp(), (size_t)S * cap * M);
        c.vcache.push_back(P->caches.back());
        // encoder K / V: the attention clamps its loads to the lane and masks by length, so the rows behind a session's length
        // only have to be finite
        P->caches.emplace_back(m.pp(), (size_t)S * se * 2 * M);
        SC_HIP(hipMemsetAsync(P->caches.back().get(), 0, (size_t)S * se * 2 * M * 4, m.stream));
        c.cross_kv.push_back(P->caches.back());
    }
    const size_t lsm = (size_t)L * S * M;
    P->kenergy = Buf<float>(m.pp(), lsm);
    P->hq = Buf<float>(m.pp(), lsm);
    P->qe0 = Buf<float>(m.pp(), lsm);
    P->qe1 = Buf<float>(m.pp(), lsm);
    P->pooled = Buf<float>(m.pp(), (size_t)S * M);
    P->logits = Buf<float>(m.pp(), (size_t)S * P->ldl);
    P->pch = Buf<float>(m.pp(), (size_t)S * L * P->H);
    P->xtmp = Buf<float>(m.pp(), (size_t)S * se * 2 * M);
    P->table = Buf<int4>(m.pp(), (size_t)cap * S);
    P->blk = Buf<int>(m.pp(), (size_t)S * POOL_MAX_BLOCKED);
    P->hook.hq = P->hq;
    P->h_table.alloc((size_t)cap * S);
    P->h_ints.alloc((size_t)S * (POOL_MAX_BLOCKED + 8) + 8);
    P->h_pch.alloc((size_t)S * L * P->H);
    P->pos.assign(S, 0);
    P->s_enc.assign(S, 0);
    P->st.self_kv_bytes = (int64_t)2 * L * S * cap * M * 4;
    P->st.cross_kv_bytes = (int64_t)L * S * se * 2 * M * 4;
    const int64_t rb = align_up(S, 32);
    const int64_t chain = (int64_t)S * M * 4 * 2 + (int64_t)std::max(1, std::max(M, W.ffn_dim) / 256) * S * 3 * M * 4 +
                          (int64_t)(4 * M + 2 * W.ffn_dim) * rb * 2 + (int64_t)M * rb * 4;
    P->st.work_bytes = chain + (int64_t)4 * lsm * 4 + (int64_t)S * M * 4 + (int64_t)S * P->ldl * 4 + (int64_t)S * L * P->H * 4 +
                       (int64_t)S * se * 2 * M * 4 + (int64_t)cap * S * 16 + (int64_t)S * POOL_MAX_BLOCKED * 4 + (int64_t)n_ints * 4;
    SC_HIP(hipStreamSynchronize(m.stream));
    return P.release();
}

void mma_pool_free(MmaPool* p) {
    if (!p) return;
    (void)hipStreamSynchronize(p->m.stream);
    delete p;
}

int mma_pool_device(const MmaPool& p) { return p.m.device; }

void mma_pool_stats(MmaPool& p, sc_mma_pool_stats* out, bool reset) {
    *out = p.st;
    if (reset) p.st.begins = p.st.steps = p.st.row_steps = 0;
}

namespace {
// the sessions a call names: k of them, in range, none twice
void check_sessions(const char* who, const MmaPool& P, const int32_t* h_sessions, int k) {
    SC_CHECK(k >= 1 && k <= P.S, "%s: k=%d outside 1..%d sessions", who, k, P.S);
    std::vector<char> seen(P.S, 0);
    for (int j = 0; j < k; ++j) {
        const int sid = h_sessions[j];
        SC_CHECK(sid >= 0 && sid < P.S, "%s: session %d outside 0..%d", who, sid, P.S - 1);
        SC_CHECK(!seen[sid], "%s: session %d is named twice", who, sid);
        seen[sid] = 1;
    }
}
}  // namespace

void mma_pool_begin(MmaPool& P, const int32_t* h_sessions, int k, const float* d_enc, const int32_t* h_s_enc) {
    Model& m = P.m;
    const int M = P.M, L = P.L, S = P.S;
    check_sessions("sc_mma_pool_begin", P, h_sessions, k);
    int64_t total = 0;
    int longest = 0;
    for (int j = 0; j < k; ++j) {
        SC_CHECK(h_s_enc[j] >= 1 && h_s_enc[j] <= P.se_cap, "sc_mma_pool_begin: session %d: encoder length %d outside 1..%d", h_sessions[j],
                 h_s_enc[j], P.se_cap);
        total += h_s_enc[j];
        longest = std::max(longest, (int)h_s_enc[j]);
    }
    prof::set_tag("mma");
    // sids | s_enc | offs: one copy (b_sids, b_senc, b_offs are consecutive slices of S, S and S + 1 ints)
    int* h = P.h_ints.p;
    int off = 0;
    for (int j = 0; j < k; ++j) {
        h[j] = h_sessions[j];
        h[S + j] = h_s_enc[j];
        h[2 * S + j] = off;
        off += h_s_enc[j];
    }
    h[2 * S + k] = off;
    SC_HIP(hipMemcpyAsync(P.b_sids, h, (size_t)(3 * S + 1) * 4, hipMemcpyHostToDevice, m.stream));
    hipLaunchKernelGGL(pool_begin_rows_kernel, dim3(k), dim3(256), 0, m.stream, P.b_sids, P.b_senc, P.b_offs, d_enc,
                       m.cfg.mma_pre_decision_ratio, M, P.pooled.get(), P.c.pos_row, P.c.d_enc_lens);
    SC_LAUNCH_CHECK();
    // encoder-decoder K / V of every layer: ONE row-independent product over the packed rows of all k sessions, scattered
    // into the sessions' lanes
    for (int li = 0; li < L; ++li) {
        project_cross_kv(m, d_enc, m.mma_dec[li].cross_kv, P.xtmp.get(), (int)total);
        hipLaunchKernelGGL(pool_scatter_cross_kernel, dim3(longest, k), dim3(256), 0, m.stream, P.xtmp.get(), P.b_sids, P.b_senc, P.b_offs,
                           P.se_cap, 2 * M, P.c.cross_kv[li]);
        SC_LAUNCH_CHECK();
    }
    // key-side EnergyProjection of every layer on the sessions' pooled rows, batched over layers and sessions; the last level
    // goes to the sessions' own [layers][M] blocks
    P.energy_levels(m.mma_ke_w, m.mma_ke_b, P.pooled.get(), 0, k, P.kenergy.get(), M, (int64_t)L * M, P.b_sids);
    SC_HIP(hipStreamSynchronize(m.stream));  // d_enc may be reused by the caller
    for (int j = 0; j < k; ++j) {
        P.pos[h_sessions[j]] = 0;
        P.s_enc[h_sessions[j]] = h_s_enc[j];
    }
    P.st.begins += k;
}

void mma_pool_step(MmaPool& P, const int32_t* h_sessions, int k, const int32_t* h_tokens, int tok_stride, const int32_t* h_n_tokens,
                   const int32_t* h_blocked, int blocked_stride, const int32_t* h_n_blocked, int32_t* h_out_index, float* h_pchoose,
                   float* d_features) {
    Model& m = P.m;
    const int M = P.M, L = P.L, H = P.H, V = P.V, S = P.S;
    check_sessions("sc_mma_pool_step", P, h_sessions, k);
    int maxn = 0;
    for (int j = 0; j < k; ++j) {
        const int sid = h_sessions[j], n = h_n_tokens[j];
        SC_CHECK(P.s_enc[sid] > 0, "sc_mma_pool_step: session %d: call sc_mma_pool_begin first", sid);
        SC_CHECK(n >= 1 && n <= tok_stride, "sc_mma_pool_step: session %d: %d tokens (1..tok_stride = %d)", sid, n, tok_stride);
        SC_CHECK(P.pos[sid] + n <= P.cap, "sc_mma_pool_step: session %d: %d tokens at position %d exceed max_len %d", sid, n, P.pos[sid],
                 P.cap);
        for (int t = 0; t < n; ++t) {
            const int tok = h_tokens[(size_t)j * tok_stride + t];
            SC_CHECK(tok >= 0 && tok < V, "sc_mma_pool_step: session %d: token %d outside the vocabulary", sid, tok);
        }
        if (h_blocked)
            SC_CHECK(h_n_blocked[j] >= 0 && h_n_blocked[j] <= std::min(POOL_MAX_BLOCKED, blocked_stride),
                     "sc_mma_pool_step: session %d: %d blocked indices (0..min(%d, blocked_stride = %d))", sid, h_n_blocked[j], POOL_MAX_BLOCKED,
                     blocked_stride);
        maxn = std::max(maxn, n);
    }
    prof::set_tag("mma");
    // Right-aligned feeds: session j joins at step maxn - n_j.  Slots in joining order (call order among equals), so a
    // session keeps its slot through the call and the live slots of a step are the first n_live.
    std::vector<int> order(k), feat_off(k), n_live(maxn, 0);
    for (int j = 0; j < k; ++j) order[j] = j;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return h_n_tokens[a] > h_n_tokens[b]; });
    for (int j = 0, o = 0; j < k; ++j) feat_off[j] = o, o += h_n_tokens[j];
    int4* tab = P.h_table.p;
    for (int t = 0; t < maxn; ++t)
        for (int s = 0; s < k; ++s) {
            const int j = order[s], first = maxn - h_n_tokens[j];
            int4 rec = make_int4(0, 0, 0, 0);
            if (t >= first) {
                rec = make_int4(h_sessions[j], h_tokens[(size_t)j * tok_stride + (t - first)], feat_off[j] + (t - first), 0);
                n_live[t] = s + 1;
            }
            tab[(size_t)t * k + s] = rec;
        }
    SC_HIP(hipMemcpyAsync(P.table.get(), tab, (size_t)maxn * k * sizeof(int4), hipMemcpyHostToDevice, m.stream));
    // n_blocked | blocked, in slot order
    int* hb = P.h_ints.p;
    bool any_blocked = false;
    for (int s = 0; s < k; ++s) {
        const int j = order[s], nb = h_blocked ? h_n_blocked[j] : 0;
        hb[s] = nb;
        any_blocked = any_blocked || nb > 0;
        for (int i = 0; i < nb; ++i) hb[S + s * POOL_MAX_BLOCKED + i] = h_blocked[(size_t)j * blocked_stride + i];
    }
    if (any_blocked) {
        SC_HIP(hipMemcpyAsync(P.n_blk, hb, (size_t)k * 4, hipMemcpyHostToDevice, m.stream));
        SC_HIP(hipMemcpyAsync(P.blk.get(), hb + S, (size_t)k * POOL_MAX_BLOCKED * 4, hipMemcpyHostToDevice, m.stream));
    }
    StepCtx& c = P.c;
    P.hook.features = d_features;
    for (int t = 0; t < maxn; ++t) {
        hipLaunchKernelGGL(pool_set_slots_kernel, dim3(1), dim3(256), 0, m.stream, P.table.get() + (size_t)t * k, n_live[t], S, c.slot_rp,
                           c.slot_lane, c.d_tok, c.pos_row, P.feat_row, P.d_rows);
        SC_LAUNCH_CHECK();
        P.hook.capture = t + 1 == maxn;
        decoder_step(m, c, /*project=*/false);  // closes with launch_pool_close: positions + feature rows
        P.st.row_steps += n_live[t];
    }
    P.st.steps += maxn;
    // the last step holds all k rows.  p_choose hook: the query-side energy MLPs of every layer for the k rows, then p_choose
    // per (head, layer, row) against the row's session's key-side energies
    P.energy_levels(m.mma_qe_w, m.mma_qe_b, P.hq.get(), (int64_t)S * M, k, (P.E & 1) ? P.qe0.get() : P.qe1.get(), (int64_t)S * M, M, nullptr);
    hipLaunchKernelGGL(pchoose_rows_kernel, dim3(H, L, k), dim3(64), 0, m.stream, (P.E & 1) ? P.qe0.get() : P.qe1.get(), (int64_t)S * M,
                       P.kenergy.get(), c.slot_rp, M, M / H, m.mma_ebias, m.cfg.mma_temperature, P.pch.get());
    SC_LAUNCH_CHECK();
    // MonotonicDecoderModel.project (TiedProjection) of the k last rows on the row-independent tiled product, the blocked
    // indices per row, arg-max over the k rows (online_text_decoder.py:225-231)
    Linear proj;
    proj.w = m.mma_embed;
    proj.ldw = M;
    proj.kpad = M;
    proj.in = M;
    proj.out = V;
    linear(m, c.hN, M, proj, nullptr, 0, P.logits.get(), P.ldl, k, ACT_NONE, 1.f, /*row_independent=*/true);
    if (any_blocked) {
        hipLaunchKernelGGL(pool_fill_blocked_kernel, dim3(k), dim3(64), 0, m.stream, P.logits.get(), P.ldl, V, P.blk.get(), P.n_blk);
        SC_LAUNCH_CHECK();
    }
    launch_argmax_rows(P.logits.get(), P.ldl, k, V, nullptr, 0, -1, -1, -1, -1, 0.f, P.out_idx, nullptr, m.stream);
    int* h_idx = P.h_ints.p + (size_t)S * (POOL_MAX_BLOCKED + 1);
    SC_HIP(hipMemcpyAsync(h_idx, P.out_idx, (size_t)k * 4, hipMemcpyDeviceToHost, m.stream));
    SC_HIP(hipMemcpyAsync(P.h_pch.p, P.pch.get(), (size_t)k * L * H * 4, hipMemcpyDeviceToHost, m.stream));
    SC_HIP(hipStreamSynchronize(m.stream));
    for (int s = 0; s < k; ++s) {
        const int j = order[s];
        h_out_index[j] = h_idx[s];
        memcpy(h_pchoose + (size_t)j * L * H, P.h_pch.p + (size_t)s * L * H, (size_t)L * H * 4);
        P.pos[h_sessions[j]] += h_n_tokens[j];
    }
}

}  // namespace sc
