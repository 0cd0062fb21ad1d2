// The decoder step chain: one step of a pre-LN transformer decoder stack for all batch rows, on one of three kernel
// families (the general step: split-K skinny products / tiled GEMMs; k_dstep.hip: packed-fragment products; k_dstep3.hip:
// row-group products with fused LayerNorm / residual), the dispatch decision between them, and the scratch a step needs
// whatever loop drives it.  The loops themselves live in model_decoder.hip, model_sample.hip and engine.hip (dstep.h).
// Module order restated from ggml/examples/unity/fairseq2.cpp:979-1094.
#include "dstep.h"

namespace sc {

static std::mutex g_capture_mutex;
std::mutex& capture_mutex() { return g_capture_mutex; }

DecStack unity_stack(const Model& m) {
    DecStack w;
    w.embed = m.text_embed;
    w.embed_p = m.text_embed_p;
    w.pos = m.text_pos;
    w.layers = &m.dec;
    w.final_ln = &m.dec_final_ln;
    w.ffn_dim = m.cfg.dec_ffn_dim;
    w.ffn_act = m.ffn_act;
    w.pchoose = nullptr;
    w.vocab = m.cfg.text_vocab_size;
    w.pad_idx = m.cfg.pad_idx;
    w.unk_idx = m.cfg.unk_idx;
    w.eos_idx = m.cfg.eos_idx;
    w.max_seq_len = m.cfg.text_max_seq_len;
    return w;
}

// the v1 autoregressive T2U decoder (unit vocabulary: bos 0, pad 1, eos 2, unk 3; t2u_builder.py:143-147)
DecStack t2u_ar_stack(const Model& m) {
    DecStack w;
    w.embed = m.t2u_ar_embed;
    w.embed_p = nullptr;
    w.pos = m.t2u_ar_pos;
    w.layers = &m.t2u_ar_dec;
    w.final_ln = &m.t2u_ar_final_ln;
    w.ffn_dim = m.cfg.t2u_ffn_dim;
    w.pchoose = nullptr;
    w.vocab = m.cfg.unit_vocab_size;
    w.pad_idx = m.cfg.unit_pad_idx;
    w.unk_idx = 3;
    w.eos_idx = m.cfg.unit_eos_idx;
    w.max_seq_len = m.cfg.unit_max_seq_len;
    return w;
}

// the streaming monotonic decoder
DecStack mma_stack(const Model& m) {
    DecStack w;
    w.embed = m.mma_embed;
    w.embed_p = m.mma_embed_p;
    w.pos = m.text_pos;  // same sinusoidal table (builder.py:169-176: max_seq_len 4096, _legacy_pad_idx=1)
    w.layers = &m.mma_dec;
    w.final_ln = &m.mma_final_ln;
    w.ffn_dim = m.cfg.mma_ffn_dim;
    w.pchoose = &m.mma_pc;
    return w;
}

namespace {

// p_choose[h] = sigmoid(((q_h . k_h) / sqrt(head_dim) + energy_bias) / temperature) for one query row and one
// pooled key (PChooseLayer.forward, models/monotonic_decoder/p_choose.py:120-148, last query x last key only:
// the streaming policy reads p_choose[..., -1, -1], streaming/agents/online_text_decoder.py:236-241).
__global__ void pchoose_kernel(const float* __restrict__ q, const float* __restrict__ k, int head_dim,
                               const float* __restrict__ energy_bias, float temperature, float* __restrict__ out) {
    const int h = blockIdx.x, lane = threadIdx.x;
    float acc = 0.f;
    for (int c = lane; c < head_dim; c += 64) acc = fmaf(q[h * head_dim + c], k[h * head_dim + c], acc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) {
        float e = acc * rsqrtf((float)head_dim);
        if (energy_bias) e += energy_bias[0];
        out[h] = 1.f / (1.f + expf(-(e / temperature)));
    }
}

// One level of the query-side EnergyProjection of EVERY layer in one launch (the streaming step's p_choose hook):
//   out[l][n] = relu(b[l][n] + W[l][n][:] . in[l][:])      one row per layer, fp16 weights, fp32 arithmetic.
// grid (M / 32, layers); a wave owns 8 output features: all 16 weight loads (8 features x 2 K halves of 512) are issued
// before the first use, the row vector sits in registers (16 floats per lane), wave reduction by shuffles.
__global__ __launch_bounds__(256) void energy_level_kernel(const __half* const* __restrict__ Wt, const float* const* __restrict__ Bt,
                                                           int ldw, const float* __restrict__ in, int64_t in_ls,
                                                           float* __restrict__ out, int M) {
    typedef _Float16 h8_t __attribute__((ext_vector_type(8)));
    const int l = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = blockIdx.x * 32 + wave * 8;
    const __half* W = Wt[l];
    const float* x = in + (int64_t)l * in_ls;  // in_ls = 0: the same row for every layer
    float xv[2][8];
    h8_t w[8][2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int k = c * 512 + lane * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) xv[c][e] = k + e < M ? x[k + e] : 0.f;
#pragma unroll
        for (int f = 0; f < 8; ++f) {
            h8_t z;
#pragma unroll
            for (int e = 0; e < 8; ++e) z[e] = (_Float16)0.f;
            w[f][c] = (k < M && n0 + f < M) ? *reinterpret_cast<const h8_t*>(W + (int64_t)(n0 + f) * ldw + k) : z;
        }
    }
#pragma unroll
    for (int f = 0; f < 8; ++f) {
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc = fmaf((float)w[f][c][e], xv[c][e], acc);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane == 0 && n0 + f < M) {
            const float v = acc + (Bt[l] ? Bt[l][n0 + f] : 0.f);
            out[(int64_t)l * M + n0 + f] = !(v <= 0.f) ? v : 0.f;  // NaN stays NaN
        }
    }
}

// p_choose of every (layer, head): grid (heads, layers), see pchoose_kernel
__global__ void pchoose_all_kernel(const float* __restrict__ q, const float* __restrict__ k, int M, int head_dim,
                                   const float* const* __restrict__ energy_bias, float temperature, float* __restrict__ out) {
    const int h = blockIdx.x, l = blockIdx.y, lane = threadIdx.x, H = gridDim.x;
    const float* ql = q + (int64_t)l * M + h * head_dim;
    const float* kl = k + (int64_t)l * M + h * head_dim;
    float acc = 0.f;
    for (int c = lane; c < head_dim; c += 64) acc = fmaf(ql[c], kl[c], acc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) {
        float e = acc * rsqrtf((float)head_dim);
        if (energy_bias[l]) e += energy_bias[l][0];
        out[l * H + h] = 1.f / (1.f + expf(-(e / temperature)));
    }
}

__global__ void store_hidden_kernel(const float* __restrict__ hN, float* __restrict__ dst, int M, int hid_rows,
                                    const int* __restrict__ d_pos) {
    const int b = blockIdx.x;
    const int pos = *d_pos;
    if (pos >= hid_rows) return;
    const float4* s = reinterpret_cast<const float4*>(hN + (int64_t)b * M);
    float4* d = reinterpret_cast<float4*>(dst + ((int64_t)b * hid_rows + pos) * M);
    for (int c = threadIdx.x; c < M / 4; c += blockDim.x) d[c] = s[c];
}

// out-projection + residual + the NEXT LayerNorm:  x += in . W^T + b ;  h_out = LN_next(x).
// Up to 64 rows: split-K skinny product into K-range partials, summed in fixed order by the fused
// reduce + residual + LayerNorm kernel.  More rows: the MFMA GEMM with a residual epilogue + LayerNorm.
void out_proj_res_ln(Model& m, StepCtx& c, const float* in, int64_t ld_in, const Linear& L, const LNorm& next,
                     float* h_out) {
    const int nb = c.nb, M = m.cfg.model_dim;
    if (nb <= 64 && L.in % 64 == 0 && L.out == M && M % 4 == 0) {
        SkinnyArgs a;
        a.A = in;
        a.lda = ld_in;
        a.W = L.w;
        a.ldw = L.ldw;
        a.M = nb;
        a.N = L.out;
        a.K = L.in;
        a.splits = skinny_splits(nb, L.out, L.in, 1);
        a.partial = c.partial;
        launch_skinny(a, m.stream);
        launch_reduce_res_ln(c.partial, a.splits, L.b, c.x, next.g, next.b, h_out, nb, M, m.stream);
    } else {
        linear(m, in, ld_in, L, c.x, M, c.x, M, nb, ACT_NONE, 1.f);
        layernorm(m, c.x, next, h_out, nb);
    }
}

// in . W^T as `*splits` K-range partial sums in c.partial (no bias): the consumer adds them up.
// Returns false when the shape is outside the skinny kernel's domain (caller falls back to linear()).
bool proj_partials(Model& m, StepCtx& c, const float* in, int64_t ld_in, const Linear& L, int* splits) {
    if (c.nb > 64 || L.in % 64 != 0) return false;
    SkinnyArgs a;
    a.A = in;
    a.lda = ld_in;
    a.W = L.w;
    a.ldw = L.ldw;
    a.M = c.nb;
    a.N = L.out;
    a.K = L.in;
    a.splits = skinny_splits(c.nb, L.out, L.in, 1);
    a.partial = c.partial;
    launch_skinny(a, m.stream);
    *splits = a.splits;
    return true;
}

}  // namespace

// EnergyProjection (p_choose.py:17-45): (Linear, ReLU) x n on `rows` rows; returns the buffer holding the result.
float* energy_mlp(Model& m, const std::vector<Linear>& layers, const float* in, int64_t ld_in, float* a, float* b, int rows) {
    const int M = m.cfg.model_dim;
    const float* src = in;
    int64_t ld = ld_in;
    float* dst = a;
    for (const Linear& L : layers) {
        linear(m, src, ld, L, nullptr, 0, dst, M, rows, ACT_RELU, 1.f);
        src = dst;
        ld = M;
        dst = (dst == a) ? b : a;
    }
    return const_cast<float*>(src);
}

// ---- second-generation step (k_dstep.hip) --------------------------------------------------------------------
bool step2_eligible(const Model& m, const DecStack& W, int nb) {
    const int M = m.cfg.model_dim;
    static const bool off = knob::is_set("SC_DECODER_GEN1");  // A/B switch: the first-generation kernels
    if (off || nb < 1 || nb > 64 || M % 64 != 0 || M > 1024 || W.ffn_dim % 64 != 0 || M != m.cfg.num_heads * 64) return false;
    for (const DecoderLayer& l : *W.layers)
        if (!l.qkv.wp || !l.self_out.wp || !l.cross_q.wp || !l.cross_out.wp || !l.ffn_in.wp || !l.ffn_out.wp) return false;
    return true;
}

// the plane layout of one decoder-step context over an allocation of 4 M rb + 2 ffn rb halfs (the streaming state keeps its
// own: the planes outlive the call); rows beyond nb are never read: their lanes load out of range
void alloc_step2_views(Model& m, StepCtx& c, int ffn_dim, __half* base) {
    const int M = m.cfg.model_dim;
    c.rb = (int)align_up(c.nb, 32);  // 32 / 64 up to 64 rows; more for the wide step of the beam search
    const size_t pm = (size_t)M * c.rb, pf = (size_t)ffn_dim * c.rb;
    c.hH = base;
    c.hL = c.hH + pm;
    c.attH = c.hL + pm;
    c.attL = c.attH + pm;
    c.wideH = c.attL + pm;
    c.wideL = c.wideH + pf;
}

void alloc_step2(Model& m, StepCtx& c, int ffn_dim) {
    c.planes = Buf<__half>(m.pp(), (size_t)(4 * m.cfg.model_dim + 2 * ffn_dim) * align_up(c.nb, 32));
    alloc_step2_views(m, c, ffn_dim, c.planes.get());
}

StepTuning StepTuning::from_knobs(int rows) {
    StepTuning t;
    t.rg_small = std::min(32, std::max(1, knob::value("SC_D3_RG_SMALL", defaults(rows).rg_small)));
    t.rg_ffn = std::min(32, std::max(1, knob::value("SC_D3_RG_FFN", 32)));
    t.ffn_in_mode = std::min(2, std::max(0, knob::value("SC_D3_FFN_IN", 1)));
    t.ffn_out_mode = std::min(2, std::max(0, knob::value("SC_D3_FFN_OUT", 1)));
    return t;
}

void init_chain_scratch(Model& m, StepScratch& s, StepCtx& c, const DecStack& W, int rows, int family, const StepTuning& t) {
    const int M = m.cfg.model_dim;
    c.nb = rows;
    s.hN = Buf<float>(m.pp(), (size_t)rows * M);
    // worst case: K/256 ranges of a [rows][M] out-projection, or M/256 ranges of the [rows][3M] q/k/v projection
    s.partial = Buf<float>(m.pp(), (size_t)std::max(1, std::max(M, W.ffn_dim) / 256) * rows * 3 * M);
    c.hN = s.hN, c.partial = s.partial;
    if (family < 2) return;
    alloc_step2(m, c, W.ffn_dim);
    if (family < 3) return;
    c.gen3 = true;
    s.xg = Buf<float>(m.pp(), (size_t)M * c.rb);
    s.qkvr = Buf<float>(m.pp(), (size_t)rows * M);
    c.xg = s.xg, c.qkvr = s.qkvr;
    if (rows > 64 && !c.slot_rp) {
        s.qkv3 = Buf<float>(m.pp(), (size_t)rows * 3 * M);
        c.qkv3 = s.qkv3;
    }
    c.rg_small = t.rg_small, c.rg_ffn = t.rg_ffn, c.ffn_in_mode = t.ffn_in_mode, c.ffn_out_mode = t.ffn_out_mode;
}

void init_step_scratch(Model& m, StepScratch& s, StepCtx& c, const DecStack& W, int rows, int family, const StepTuning& t,
                       bool wide_always) {
    const int M = m.cfg.model_dim;
    s.x = Buf<float>(m.pp(), (size_t)rows * M);
    s.h = Buf<float>(m.pp(), (size_t)rows * M);
    s.wide = Buf<float>(m.pp(), family >= 2 && !wide_always ? 4 : (size_t)rows * std::max(3 * M, W.ffn_dim));
    s.att = Buf<float>(m.pp(), (size_t)rows * M);
    c.x = s.x, c.h = s.h, c.wide = s.wide, c.att = s.att;
    init_chain_scratch(m, s, c, W, rows, family, t);
}

// One level of the query- or key-side EnergyProjection of every layer (energy_level_kernel)
void launch_energy_level(Model& m, const __half* const* Wt, const float* const* Bt, int layers, const float* in, int64_t in_ls, float* out) {
    const int M = m.cfg.model_dim;
    hipLaunchKernelGGL(energy_level_kernel, dim3(cdiv(M, 32), layers), dim3(256), 0, m.stream, Wt, Bt, m.mma_qe_ldw, in, in_ls, out, M);
    SC_LAUNCH_CHECK();
}

// ---- third-generation step (k_dstep3.hip): eligibility --------------------------------------------------------------
bool step3_eligible(const Model& m, const DecStack& W, int nb) {
    static const bool off = knob::is_set("SC_DECODER_GEN2");  // A/B switch: the second-generation chain
    if (off || !step2_eligible(m, W, nb)) return false;
    const int M = m.cfg.model_dim;
    return gemv3_supported(nb, 3 * M, M, IN3_LN) && gemv3_supported(nb, M, W.ffn_dim, IN3_PLANES) && M % 8 == 0;
}

// > 64 live rows (beam search at the benchmark batch: 64 utterances x 5 beams): the same chain, every product cut into row
// groups, q | k | v on the row-group kernel too (the packed split-K product stops at 64 rows)
bool step3_wide_eligible(const Model& m, const DecStack& W, int nb) {
    static const bool off = knob::is_set("SC_DECODER_GEN2") || knob::is_set("SC_DECODER_GEN1");
    const int M = m.cfg.model_dim;
    if (off || nb <= 64 || nb > 512 || M % 64 != 0 || M > 1024 || W.ffn_dim % 64 != 0 || M != m.cfg.num_heads * 64) return false;
    for (const DecoderLayer& l : *W.layers)
        if (!l.qkv.wp || !l.self_out.wp || !l.cross_q.wp || !l.cross_out.wp || !l.ffn_in.wp || !l.ffn_out.wp) return false;
    return gemv3_supported(nb, 3 * M, M, IN3_PLANES) && gemv3_supported(nb, M, W.ffn_dim, IN3_PLANES) &&
           gemv3_supported(nb, M, M, IN3_LN) && gemv3_supported(nb, W.ffn_dim, M, IN3_LN);  // the LayerNorm-fused q / FFN-in launches
}

ArgmaxEpi step_argmax_epi(const StepCtx& c, const DecStack& W) {
    ArgmaxEpi e;
    e.part = c.am_part, e.tiles_cap = c.am_tiles, e.eos_logit = c.am_eos_logit, e.pos = c.d_pos;
    e.min_step_for_eos = c.min_seq_len, e.force_eos_step = c.force_eos_step;
    e.pad_idx = W.pad_idx, e.eos_idx = W.eos_idx, e.unk_idx = W.unk_idx, e.unk_penalty = c.unk_penalty;
    return e;
}

// THE dispatch decision (setup_session, run_generate_beam, the streaming step and decoder_step_family's report all call this
// and nothing else composes the predicates): which kernel family a step of `rows` rows over stack W runs on for caller
// 0 greedy generation, 1 / 3 beam search (text / v1 unit decoder), 2 the streaming monotonic step.
// SC_STEP_GENERAL 1, SC_STEP_PACKED 2, SC_STEP_ROWGROUP 3, SC_STEP_ROWGROUP_WIDE 4 (model.h).
int choose_family(const Model& m, const DecStack& W, int rows, int caller) {
    const int M = m.cfg.model_dim;
    if (caller == 2) return step2_eligible(m, W, 1) ? 2 : 1;
    if (caller == 0) {
        // the packed step projects through the packed embedding (a failed pack leaves it null: first-generation step then)
        const bool gen2 = step2_eligible(m, W, rows) && W.embed_p != nullptr;
        const bool fused_argmax = fused_argmax_rows(rows, M);
        const bool gen3 = gen2 && step3_eligible(m, W, rows) && fused_argmax && vocab3_supported(rows, W.vocab, M);
        if (W.ffn_act == ACT_GELU) return gen3 ? 3 : 1;  // the packed chain's FFN epilogue knows ReLU only
        return gen3 ? 3 : (gen2 ? 2 : 1);
    }
    // beam search: packed-weight step kernels up to 64 live rows, the wide row-group chain above
    const bool packed = step2_eligible(m, W, rows) || step3_wide_eligible(m, W, rows);
    if (!packed) return 1;
    if (rows > 64) return 4;
    if (W.ffn_act == ACT_GELU) return step3_eligible(m, W, rows) ? 3 : 1;
    return step3_eligible(m, W, rows) ? 3 : 2;
}

// Which kernel family a decoder step of `rows` live rows runs on, decided by the SAME predicates the callers use (the
// dispatch matrix in one place; tests/test_dispatch_gpu.py pins it).  caller: 0 greedy text generation (setup_session),
// 1 beam search over the text decoder, 2 the streaming monotonic decoder's step, 3 beam search over the v1 unit decoder.
// Returns SC_STEP_GENERAL (1: split-K skinny products up to 64 rows, tiled GEMMs above),
// SC_STEP_PACKED (2: packed-fragment products, k_dstep.hip), SC_STEP_ROWGROUP (3: row-group products with fused LayerNorm /
// residual, k_dstep3.hip) or SC_STEP_ROWGROUP_WIDE (4: the same chain cut into row groups, > 64 rows).
int decoder_step_family(const Model& m, int rows, int caller) {
    if (caller == 2) {
        if (m.mma_dec.empty()) return SC_ERR_INVALID;
        return choose_family(m, mma_stack(m), 1, 2);
    }
    if (caller == 3 && m.t2u_ar_dec.empty()) return SC_ERR_INVALID;
    return choose_family(m, caller == 3 ? t2u_ar_stack(m) : unity_stack(m), rows, caller);
}

namespace {

static void gemv2(Model& m, StepCtx& c, const __half* Ah, const __half* Al, const Linear& L, int want_splits, int* splits) {
    GemvPArgs a;
    a.Wp = L.wp;
    a.Ah = Ah;
    a.Al = Al;
    a.RB = c.rb;
    a.M = c.nb;
    a.N = L.out;
    a.K = L.in;
    a.splits = want_splits;
    a.epi = EPI_PARTIAL;
    a.partial = c.partial;
    a.d_rows = c.d_rows;
    launch_gemvp(a, m.stream);
    *splits = gemvp_splits(L.in, want_splits);
}

// Attention arguments of a packed step, everything the second- and third-generation chains share; the family adds where its
// query rows are (q / sstride / S / bias) and, third generation, the decode engine's slot tables (null otherwise).
// Self-attention of layer `li` over the K / V caches: q | k | v are columns 0 | M | 2M of a 3M-wide projection.
DAttnArgs self_attn_args(const StepCtx& c, int li, int M, int heads) {
    DAttnArgs a;
    a.ldq = 3 * M;
    a.koff = M;
    a.voff = 2 * M;
    a.kcache = c.kcache[li];
    a.vcache = c.vcache[li];
    a.cache_ld = M;
    a.cache_bs = (int64_t)c.cap * M;
    a.cap = c.cap;
    a.d_pos = c.d_pos;
    a.Oh = c.attH;
    a.Ol = c.attL;
    a.ORB = c.rb;
    a.nb = c.nb;
    a.heads = heads;
    a.anc = c.anc;
    a.d_rows = c.d_rows;
    return a;
}

// Encoder-decoder attention of layer `li` over the K | V projected once per utterance ([s_enc][2M] per cache row)
DAttnArgs cross_attn_args(const StepCtx& c, int li, int M, int heads) {
    DAttnArgs x;
    x.ldq = M;
    x.kcache = c.cross_kv[li];
    x.vcache = c.cross_kv[li] + M;
    x.cache_ld = 2 * M;
    x.cache_bs = (int64_t)c.s_enc * 2 * M;
    x.cap = c.s_enc;
    x.kv_lens = c.d_enc_lens;
    x.kv_row_div = c.cross_row_div;
    x.kv_item = c.kv_item;
    x.d_rows = c.d_rows;
    x.Oh = c.attH;
    x.Ol = c.attL;
    x.ORB = c.rb;
    x.nb = c.nb;
    x.heads = heads;
    return x;
}

// One decoder step for all batch rows on the second-generation kernels: 11 launches per layer
// (QKV | self-attention | out-proj | +res+LN | q | cross-attention | out-proj | +res+LN | FFN-in | FFN-out | +res+LN).
void decoder_step2(Model& m, StepCtx& c, bool project, const DecStack& W) {
    const sc_config& cfg = m.cfg;
    const int M = cfg.model_dim, nb = c.nb, H = cfg.num_heads;
    const std::vector<DecoderLayer>& layers = *W.layers;
    const int n_layers = (int)layers.size();
    launch_embed_ln(c.d_tok, W.embed, sqrtf((float)M), W.pos, c.d_pos, c.x, layers[0].self_ln.g, layers[0].self_ln.b, c.hH, c.hL,
                    c.rb, nb, M, m.stream);
    for (int li = 0; li < n_layers; ++li) {
        const DecoderLayer& l = layers[li];
        const bool last = li + 1 == n_layers;
        int sp = 1;
        // self attention
        gemv2(m, c, c.hH, c.hL, l.qkv, 2, &sp);
        DAttnArgs a = self_attn_args(c, li, M, H);
        a.q = c.partial;
        a.sstride = (int64_t)nb * 3 * M;
        a.S = sp;
        a.bias = l.qkv.b;
        launch_dattn(a, /*cross=*/false, m.stream);
        gemv2(m, c, c.attH, c.attL, l.self_out, 4, &sp);
        // monotonic decoder, p_choose step: the normed cross-attention input (monotonic_decoder_layer.py:170-172) of every
        // layer is kept as an fp32 row; the energy MLPs of all layers run batched after the last layer
        launch_reduce_ln(c.partial, sp, l.self_out.b, c.x, l.cross_ln.g, l.cross_ln.b, c.hH, c.hL, c.rb, nullptr, 0, 0, nullptr, nb, M,
                         m.stream, c.pchoose ? c.d_hq + (int64_t)li * M : nullptr);
        // encoder-decoder attention over the K/V projected once per utterance
        gemv2(m, c, c.hH, c.hL, l.cross_q, 4, &sp);
        DAttnArgs x = cross_attn_args(c, li, M, H);
        x.q = c.partial;
        x.sstride = (int64_t)nb * M;
        x.S = sp;
        x.bias = l.cross_q.b;
        launch_dattn(x, /*cross=*/true, m.stream);
        gemv2(m, c, c.attH, c.attL, l.cross_out, 4, &sp);
        launch_reduce_ln(c.partial, sp, l.cross_out.b, c.x, l.ffn_ln.g, l.ffn_ln.b, c.hH, c.hL, c.rb, nullptr, 0, 0, nullptr, nb, M,
                         m.stream);
        // feed-forward network: the inner activation stays in split planes
        GemvPArgs f;
        f.Wp = l.ffn_in.wp;
        f.Ah = c.hH;
        f.Al = c.hL;
        f.RB = c.rb;
        f.M = nb;
        f.N = W.ffn_dim;
        f.K = M;
        f.splits = 1;
        f.epi = EPI_PLANES;
        f.bias = l.ffn_in.b;
        f.act = ACT_RELU;
        f.Oh = c.wideH;
        f.Ol = c.wideL;
        f.ORB = c.rb;
        launch_gemvp(f, m.stream);
        gemv2(m, c, c.wideH, c.wideL, l.ffn_out, 8, &sp);
        const LNorm& next = last ? *W.final_ln : layers[li + 1].self_ln;
        // the last layer's LayerNorm is the decoder output: also kept as fp32 rows (c.hN) and, when asked for, captured
        // per position (the teacher-forced pass of the reference, generator.py:294-299)
        if (last) {
            launch_reduce_ln(c.partial, sp, l.ffn_out.b, c.x, next.g, next.b, c.hH, c.hL, c.rb, c.dec_hidden,
                             (int64_t)(c.cap - 1) * M, c.dec_hidden ? c.cap - 1 : 0, c.d_pos, nb, M, m.stream, c.hN);
        } else {
            launch_reduce_ln(c.partial, sp, l.ffn_out.b, c.x, next.g, next.b, c.hH, c.hL, c.rb, nullptr, 0, 0, nullptr, nb, M, m.stream);
        }
    }
    if (c.pchoose) {
        SC_CHECK(nb == 1 && W.pchoose && m.mma_qe_w && M <= 1024, "p_choose hook: one row on the monotonic stack only");
        const int E = cfg.mma_energy_layers;
        const float* src = c.d_hq;
        float* dst = c.qe0;
        for (int e = 0; e < E; ++e) {
            launch_energy_level(m, m.mma_qe_w + (size_t)e * n_layers, m.mma_qe_b + (size_t)e * n_layers, n_layers, src, (int64_t)M, dst);
            src = dst;
            dst = (dst == c.qe0) ? c.qe1 : c.qe0;
        }
        hipLaunchKernelGGL(pchoose_all_kernel, dim3(H, n_layers), dim3(64), 0, m.stream, src, c.d_kenergy, M, M / H, m.mma_ebias,
                           cfg.mma_temperature, c.d_pchoose);
        SC_LAUNCH_CHECK();
    }
    if (project) {
        SC_CHECK(W.embed_p, "decoder_step2: the fused vocabulary projection needs the packed embedding of this decoder stack");
        GemvPArgs v;
        v.Wp = W.embed_p;
        v.Ah = c.hH;
        v.Al = c.hL;
        v.RB = c.rb;
        v.M = nb;
        v.N = W.vocab;
        v.K = M;
        v.splits = 1;
        v.ntl = c.am_ntl;
        v.epi = EPI_ARGMAX;
        v.am = step_argmax_epi(c, W);
        launch_gemvp(v, m.stream);
        launch_argmax_finalize(v.am, gemvp_argmax_tiles(W.vocab, c.am_ntl), nb, c.d_tok, c.d_hist, c.cap, c.d_finished, c.d_out_len,
                               c.d_score, m.stream, c.d_prompt_len);
    }
    launch_add_i32(c.d_pos, 1, m.stream);
}

// ---- third-generation step (k_dstep3.hip) ---------------------------------------------------------------------
// 9 launches per layer: QKV (packed product, K-range partials) | self-attention | out-proj (+bias +residual inside) |
// q (LayerNorm inside) | cross-attention | out-proj (+bias +residual inside) | FFN-in (LayerNorm inside, ReLU, planes) |
// FFN-out (K-slice partials) | reduce + bias + residual + the NEXT LayerNorm as planes (after the last layer: the decoder output).
void decoder_step3(Model& m, StepCtx& c, bool project, const DecStack& W) {
    const sc_config& cfg = m.cfg;
    const int M = cfg.model_dim, nb = c.nb, H = cfg.num_heads;
    const std::vector<DecoderLayer>& layers = *W.layers;
    const int n_layers = (int)layers.size();
    launch_embed3(c.d_tok, W.embed, sqrtf((float)M), W.pos, c.d_pos, c.xg, c.rb, nb, M, m.stream, c.slot_rp, c.slot_rp ? c.d_rows : nullptr);
    launch_ln3(c.xg, c.rb, layers[0].self_ln.g, layers[0].self_ln.b, c.hH, c.hL, c.rb, nb, M, m.stream);
    auto out_resid = [&](const Linear& L) {  // x += att . W^T + b, finished inside the product
        Gemv3Args a;
        a.Wp = L.wp, a.M = nb, a.N = L.out, a.K = L.in;
        a.in_mode = IN3_PLANES, a.Ah = c.attH, a.Al = c.attL, a.RB = c.rb, a.rg = c.rg_small;
        a.epi = EPI3_RESID, a.bias = L.b, a.xres = c.xg, a.XRB = c.rb;
        a.d_rows = c.d_rows;
        launch_gemv3(a, m.stream);
    };
    // x += bias + partials; h = LayerNorm(x) as planes: the K-slice products' closing launch
    auto reduce_ln3 = [&](int S, const float* bias, const LNorm& ln, bool decoder_output) {
        Reduce3Args r;
        r.partial = c.partial, r.S = S, r.bias = bias, r.xg = c.xg, r.XRB = c.rb, r.rows = nb, r.C = M;
        r.gamma = ln.g, r.beta = ln.b, r.Hh = c.hH, r.Hl = c.hL, r.RB = c.rb;
        r.d_rows = c.d_rows;
        if (decoder_output) {  // also fp32 rows (c.hN) and the per-position capture (the reference's teacher-forced pass)
            r.hrow = c.dec_hidden, r.hrow_bs = (int64_t)(c.cap - 1) * M, r.hrow_rows = c.dec_hidden ? c.cap - 1 : 0, r.d_pos = c.d_pos;
            r.hfix = c.hN;
            r.slot_rp = c.slot_rp;
        }
        launch_reduce3(r, m.stream);
    };
    for (int li = 0; li < n_layers; ++li) {
        const DecoderLayer& l = layers[li];
        const bool last = li + 1 == n_layers;
        int sp = 1;
        DAttnArgs a = self_attn_args(c, li, M, H);
        if (nb <= 64 || c.slot_rp) {
            // self attention: q | k | v as K-range partials of the packed product (summed by the attention kernel); the decode
            // engine keeps this product above 64 slots too (in blocks of 64 rows): a row gets the bits it gets in a 64-slot step
            gemv2(m, c, c.hH, c.hL, l.qkv, 2, &sp);
            a.q = c.partial;
            a.sstride = (int64_t)nb * 3 * M;
            a.S = sp;
            a.bias = l.qkv.b;
        } else {  // wide step: complete rows from the row-group kernel
            Gemv3Args q;
            q.Wp = l.qkv.wp, q.M = nb, q.N = 3 * M, q.K = M;
            q.in_mode = IN3_PLANES, q.Ah = c.hH, q.Al = c.hL, q.RB = c.rb, q.rg = 32;
            q.epi = EPI3_ROWS, q.bias = l.qkv.b, q.out = c.qkv3, q.ldo = 3 * M;
            q.d_rows = c.d_rows;
            launch_gemv3(q, m.stream);
            a.q = c.qkv3;
            a.sstride = 0;
            a.S = 1;
            a.bias = nullptr;
        }
        a.slot_rp = c.slot_rp;
        a.slot_lane = c.slot_lane;
        launch_dattn(a, /*cross=*/false, m.stream);
        out_resid(l.self_out);
        // session pool, p_choose step: the query projection below normalises inside the product, so the normed
        // cross-attention input (monotonic_decoder_layer.py:170-172) of the live slots is written out by a launch of its own
        if (c.pool && c.pool->capture)
            launch_pool_capture_ln(c.xg, c.rb, l.cross_ln.g, l.cross_ln.b, c.pool->hq + (int64_t)li * nb * M, nb, M, c.d_rows, m.stream);
        // encoder-decoder attention: the query projection applies its LayerNorm itself
        {
            Gemv3Args q;
            q.Wp = l.cross_q.wp, q.M = nb, q.N = M, q.K = M;
            q.in_mode = IN3_LN, q.xg = c.xg, q.gamma = l.cross_ln.g, q.beta = l.cross_ln.b, q.RB = c.rb, q.rg = c.rg_small;
            q.epi = EPI3_ROWS, q.bias = l.cross_q.b, q.out = c.qkvr, q.ldo = M;
            q.d_rows = c.d_rows;
            launch_gemv3(q, m.stream);
        }
        DAttnArgs x = cross_attn_args(c, li, M, H);
        x.q = c.qkvr;
        x.sstride = 0;
        x.S = 1;
        x.bias = nullptr;  // added by the projection
        x.slot_rp = c.slot_rp;
        launch_dattn(x, /*cross=*/true, m.stream);
        // feed-forward network: the inner activation stays in split planes
        if (c.ffn_in_mode == 0 && nb <= 64 && W.ffn_act != ACT_GELU) {  // (the packed product knows no GELU) K-range partials + reduce / LayerNorm launch, then the packed product on planes
            gemv2(m, c, c.attH, c.attL, l.cross_out, 4, &sp);
            reduce_ln3(sp, l.cross_out.b, l.ffn_ln, false);
            GemvPArgs f;
            f.Wp = l.ffn_in.wp, f.Ah = c.hH, f.Al = c.hL, f.RB = c.rb, f.M = nb, f.N = W.ffn_dim, f.K = M;
            f.splits = 1, f.epi = EPI_PLANES, f.bias = l.ffn_in.b, f.act = ACT_RELU;
            f.Oh = c.wideH, f.Ol = c.wideL, f.ORB = c.rb;
            launch_gemvp(f, m.stream);
        } else {  // the out-projection finishes x itself, FFN-in applies the LayerNorm itself
            out_resid(l.cross_out);
            {
                Gemv3Args f;
                f.Wp = l.ffn_in.wp, f.M = nb, f.N = W.ffn_dim, f.K = M;
                f.in_mode = IN3_LN, f.xg = c.xg, f.gamma = l.ffn_ln.g, f.beta = l.ffn_ln.b, f.RB = c.rb, f.rg = c.rg_ffn;
                // (a GELU stack under SC_D3_FFN_IN=0 lands here too: it takes the default's shape, not the one-tile shape of mode 2)
                const bool gelu_mode0 = c.ffn_in_mode == 0 && nb <= 64 && W.ffn_act == ACT_GELU;
                f.shape = (c.ffn_in_mode == 1 || gelu_mode0) ? G3_T2K8 : G3_T1;
                f.epi = EPI3_PLANES, f.bias = l.ffn_in.b, f.act = W.ffn_act, f.Oh = c.wideH, f.Ol = c.wideL, f.ORB = c.rb;
                f.d_rows = c.d_rows;
                launch_gemv3(f, m.stream);
            }
        }
        if (c.ffn_out_mode == 0 && nb <= 64) {
            gemv2(m, c, c.wideH, c.wideL, l.ffn_out, 8, &sp);
        } else {
            Gemv3Args o;
            o.Wp = l.ffn_out.wp, o.M = nb, o.N = M, o.K = W.ffn_dim;
            o.in_mode = IN3_PLANES, o.Ah = c.wideH, o.Al = c.wideL, o.RB = c.rb, o.mt2 = 1;
            o.shape = c.ffn_out_mode == 1 ? G3_T2K4 : G3_T1;
            o.epi = EPI3_PARTIAL, o.out = c.partial;
            o.d_rows = c.d_rows;
            launch_gemv3(o, m.stream);
            sp = gemv3_splits(W.ffn_dim, o.shape);
        }
        reduce_ln3(sp, l.ffn_out.b, last ? *W.final_ln : layers[li + 1].self_ln, last);
    }
    if (project) {
        Vocab3Args v;
        v.Wp = W.embed_p, v.Ah = c.hH, v.Al = c.hL, v.RB = c.rb, v.M = nb, v.N = W.vocab, v.K = M;
        v.am = step_argmax_epi(c, W);
        v.d_rows = c.d_rows;
        v.slot_rp = c.slot_rp, v.limit_row = c.limit_row;
        launch_vocab3(v, m.stream);
        if (c.slot_rp) {  // decode engine: per-row rules and positions (the closing launch advances them)
            EngineFinalizeArgs f;
            f.part = c.am_part, f.tiles = vocab3_groups(nb), f.slots = nb, f.eos_logit = c.am_eos_logit;
            f.slot_rp = c.slot_rp, f.d_rows = c.d_rows, f.pad_idx = W.pad_idx, f.eos_idx = W.eos_idx;
            f.rows.tok = c.d_tok, f.rows.pos = c.pos_row, f.rows.finished = c.d_finished, f.rows.out_len = c.d_out_len;
            f.rows.limit = c.limit_row, f.rows.prefix_len = c.prefix_row, f.rows.enc_lens = c.d_enc_lens, f.rows.score = c.d_score;
            f.rows.hist = c.d_hist, f.rows.hidden = c.dec_hidden, f.rows.cap = c.cap, f.rows.M = M;
            launch_engine_finalize(f, m.stream);
            return;
        }
        launch_argmax_finalize(v.am, vocab3_groups(nb), nb, c.d_tok, c.d_hist, c.cap, c.d_finished, c.d_out_len, c.d_score, m.stream,
                               c.d_prompt_len);
    }
    if (c.pool) {  // session pool: per-slot positions, decoder outputs into the caller's packed rows; the caller projects
        SC_CHECK(c.slot_rp && c.d_rows && c.pos_row && !project, "decoder step: a pool step runs in slot mode and is not projected here");
        launch_pool_close(c.hN, c.slot_rp, c.d_rows, c.pos_row, c.pool->feat_row, c.pool->features, nb, M, m.stream);
        return;
    }
    SC_CHECK(!c.slot_rp, "decoder step: the decode engine's step always projects");
    launch_add_i32(c.d_pos, 1, m.stream);
}

}  // namespace

// One decoder step for all batch rows: feeds d_tok at position *d_pos.
void decoder_step(Model& m, StepCtx& c, bool project) {
    const sc_config& cfg = m.cfg;
    const int M = cfg.model_dim, nb = c.nb;
    const DecStack own = unity_stack(m);
    const DecStack& W = c.stack ? *c.stack : own;
    if (c.gen3) {
        decoder_step3(m, c, project, W);
        return;
    }
    if (c.rb > 0) {
        decoder_step2(m, c, project, W);
        return;
    }
    const std::vector<DecoderLayer>& layers = *W.layers;
    const int n_layers = (int)layers.size();
    launch_embed_tokens(c.d_tok, nb, W.embed, M, sqrtf((float)M), W.pos, c.d_pos, 0, c.x, M, m.stream);
    layernorm(m, c.x, layers[0].self_ln, c.h, nb);
    for (int li = 0; li < n_layers; ++li) {
        const DecoderLayer& l = layers[li];
        const bool last = li + 1 == n_layers;
        int sp = 1;
        // self attention: q/k/v partials are summed (+bias) by the attention kernel itself
        if (proj_partials(m, c, c.h, M, l.qkv, &sp)) {
            const int64_t stride = (int64_t)nb * 3 * M;
            launch_decode_attention(c.partial, 3 * M, c.partial + M, c.partial + 2 * M, 3 * M, c.kcache[li], c.vcache[li], M,
                                    (int64_t)c.cap * M, c.cap, c.att, M, nb, cfg.num_heads, c.d_pos, nullptr, 0, m.stream, sp,
                                    stride, l.qkv.b, l.qkv.b ? l.qkv.b + M : nullptr, l.qkv.b ? l.qkv.b + 2 * M : nullptr);
        } else {
            linear(m, c.h, M, l.qkv, nullptr, 0, c.wide, 3 * M, nb, ACT_NONE, 1.f);
            launch_decode_attention(c.wide, 3 * M, c.wide + M, c.wide + 2 * M, 3 * M, c.kcache[li], c.vcache[li], M,
                                    (int64_t)c.cap * M, c.cap, c.att, M, nb, cfg.num_heads, c.d_pos, nullptr, 0, m.stream);
        }
        out_proj_res_ln(m, c, c.att, M, l.self_out, l.cross_ln, c.h);
        if (c.pchoose) {  // monotonic decoder: p_choose of the normed cross-attention input (monotonic_decoder_layer.py:170-172)
            const PChooseLayer& pc = (*W.pchoose)[li];
            const float* qe = energy_mlp(m, pc.q, c.h, M, c.qe0, c.qe1, 1);
            hipLaunchKernelGGL(pchoose_kernel, dim3(cfg.num_heads), dim3(64), 0, m.stream, qe, c.d_kenergy + (int64_t)li * M,
                               M / cfg.num_heads, pc.energy_bias, cfg.mma_temperature, c.d_pchoose + (int64_t)li * cfg.num_heads);
            SC_LAUNCH_CHECK();
        }
        // encoder-decoder attention over the K/V projected once per utterance
        if (proj_partials(m, c, c.h, M, l.cross_q, &sp)) {
            launch_decode_attention(c.partial, M, nullptr, nullptr, 0, c.cross_kv[li], c.cross_kv[li] + M, 2 * M,
                                    (int64_t)c.s_enc * 2 * M, c.s_enc, c.att, M, nb, cfg.num_heads, nullptr, c.d_enc_lens, 1,
                                    m.stream, sp, (int64_t)nb * M, l.cross_q.b, nullptr, nullptr);
        } else {
            linear(m, c.h, M, l.cross_q, nullptr, 0, c.wide, M, nb, ACT_NONE, 1.f);
            launch_decode_attention(c.wide, M, nullptr, nullptr, 0, c.cross_kv[li], c.cross_kv[li] + M, 2 * M,
                                    (int64_t)c.s_enc * 2 * M, c.s_enc, c.att, M, nb, cfg.num_heads, nullptr, c.d_enc_lens, 1,
                                    m.stream);
        }
        out_proj_res_ln(m, c, c.att, M, l.cross_out, l.ffn_ln, c.h);
        linear(m, c.h, M, l.ffn_in, nullptr, 0, c.wide, W.ffn_dim, nb, W.ffn_act, 1.f);
        out_proj_res_ln(m, c, c.wide, W.ffn_dim, l.ffn_out, last ? *W.final_ln : layers[li + 1].self_ln, last ? c.hN : c.h);
    }
    if (c.dec_hidden) {
        hipLaunchKernelGGL(store_hidden_kernel, dim3(nb), dim3(256), 0, m.stream, c.hN, c.dec_hidden, M, c.cap - 1, c.d_pos);
        SC_LAUNCH_CHECK();
    }
    if (project) {
        if (fused_argmax_rows(nb, M)) {
            // vocabulary projection with the arg-max folded into its epilogue: no logits in HBM
            SkinnyArgs a;
            a.A = c.hN;
            a.lda = M;
            a.W = W.embed;
            a.ldw = M;
            a.M = nb;
            a.N = W.vocab;
            a.K = M;
            a.am = step_argmax_epi(c, W);
            launch_skinny(a, m.stream);
            launch_argmax_finalize(a.am, c.am_tiles, nb, c.d_tok, c.d_hist, c.cap, c.d_finished, c.d_out_len, c.d_score, m.stream,
                                   c.d_prompt_len);
        } else {
            Linear proj;
            proj.w = W.embed;
            proj.ldw = M;
            proj.kpad = M;
            proj.in = M;
            proj.out = W.vocab;
            linear(m, c.hN, M, proj, nullptr, 0, c.logits, W.vocab, nb, ACT_NONE, 1.f);
            launch_argmax_rows(c.logits, W.vocab, nb, W.vocab, c.d_pos, c.min_seq_len,
                               c.force_eos_step, W.pad_idx, W.eos_idx, W.unk_idx, c.unk_penalty, c.d_tok, c.d_lprob,
                               m.stream);
            launch_step_update(c.d_tok, c.d_hist, c.cap, c.d_finished, c.d_out_len, c.d_lprob, c.d_score, nb, c.d_pos,
                               W.pad_idx, W.eos_idx, nullptr, m.stream, c.d_prompt_len);
        }
    }
    launch_add_i32(c.d_pos, 1, m.stream);
}

}  // namespace sc
