// NLLB text decoder: greedy autoregressive generation with a KV cache, the
// per-step launch sequence optionally replayed from a captured hipGraph; the streaming monotonic decoder, the
// teacher-forced passes, scoring, language identification and beam search.  The step itself: model_dstep.hip.
//
// Reference call sites (src/seamless_communication/...):
//   inference/generator.py:147-156,261-263   BeamSearchSeq2SeqGenerator (beam 1 here)
//   models/unity/model.py:233-260            UnitYX2TModel.decode / project
//   inference/generator.py:281-299           teacher-forced second decoder pass
// Step rules restated from ggml/examples/unity/fairseq2.cpp:1097-1126 (max length),
// :1269-1305 (_tweak_lprobs), :1463-1594 (step loop).
#include <cstdlib>

#include "dstep.h"
#include "engine.h"

namespace sc {

int text_max_len(const Model& m, const sc_gen_opts& o, int s_enc) {
    int max_len;
    const int src = o.source_len > 0 ? o.source_len : s_enc;  // what fairseq2 calls max_source_len (see sc_gen_opts.source_len)
    if (src <= 0 || o.soft_max_seq_len_a <= 0) max_len = o.hard_max_seq_len;
    else max_len = std::min(o.hard_max_seq_len, (int)(o.soft_max_seq_len_a * (float)src) + o.soft_max_seq_len_b);
    return std::min(max_len, m.cfg.text_max_seq_len);
}

// --------------------------------------------------------------------------------------------- //
// Streaming monotonic decoder (cfg 5).  One row; the state lives in the handle between calls.
// --------------------------------------------------------------------------------------------- //
namespace {

// out[c] = (sum_t rows[t][c]) / count — the last window of AvgPool1d(kernel = stride = ratio, ceil_mode=True)
// (p_choose.py:114-118): a clipped window is divided by the number of positions it really covers.
__global__ void mean_rows_kernel(const float* __restrict__ rows, int count, int M, float* __restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= M) return;
    float acc = 0.f;
    for (int t = 0; t < count; ++t) acc += rows[(int64_t)t * M + c];
    out[c] = acc / (float)count;
}

__global__ void fill_indices_kernel(float* __restrict__ row, const int* __restrict__ idx, int n, int V, float value) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && idx[i] >= 0 && idx[i] < V) row[idx[i]] = value;
}

struct MmaWork {  // slices of MmaState::work
    float *x, *h, *att, *hN, *wide, *partial, *logits, *qe0, *qe1, *pooled, *hq;
};

MmaWork mma_work(const Model& m, float* base, size_t* total) {
    const sc_config& c = m.cfg;
    const size_t M = c.model_dim;
    const size_t wideN = std::max<size_t>(3 * M, c.mma_ffn_dim);
    const size_t part = (size_t)std::max(1, std::max(c.model_dim, c.mma_ffn_dim) / 256) * 3 * M;
    MmaWork w;
    size_t o = 0;
    auto take = [&](size_t n) {
        float* p = base ? base + o : nullptr;
        o += (n + 63) & ~(size_t)63;
        return p;
    };
    w.x = take(M);
    w.h = take(M);
    w.att = take(M);
    w.hN = take(M);
    w.wide = take(wideN);
    w.partial = take(part);
    w.logits = take(c.text_vocab_size);
    w.qe0 = take((size_t)std::max(1, c.mma_layers) * M);
    w.qe1 = take((size_t)std::max(1, c.mma_layers) * M);
    w.pooled = take(M);
    w.hq = take((size_t)std::max(1, c.mma_layers) * M);
    if (total) *total = o;
    return w;
}

}  // namespace

void run_mma_begin(Model& m, const float* d_enc, int s_enc, int max_len) {
    const sc_config& cfg = m.cfg;
    const int M = cfg.model_dim, L = cfg.mma_layers, H = cfg.num_heads;
    SC_CHECK(L > 0, "sc_mma_begin: the model was loaded without a monotonic decoder");
    SC_CHECK(s_enc > 0 && s_enc <= 4096, "sc_mma_begin: encoder length %d out of range", s_enc);
    SC_CHECK(max_len >= 2 && max_len <= cfg.text_max_seq_len && max_len <= 4096, "sc_mma_begin: max_len %d out of range", max_len);
    prof::set_tag("mma");
    size_t work_n = 0;
    mma_work(m, nullptr, &work_n);
    // The state is kept across policy rounds while it fits: a streaming session calls sc_mma_begin once per segment with a
    // growing encoder length and the same max_len.
    if (!m.mma || m.mma->cap != max_len || m.mma->cap_enc < s_enc) {
        const int grow = m.mma ? m.mma->cap_enc + m.mma->cap_enc / 2 : 0;
        const int cap_enc = std::min(4096, (int)align_up((int64_t)std::max(s_enc, grow), 64));
        m.mma.reset();  // the previous buffers go first
        std::unique_ptr<MmaState> st(new MmaState());
        st->cap = max_len;
        st->cap_enc = cap_enc;
        st->kv = Buf<float>(m.pp(), (size_t)2 * L * max_len * M);
        st->cross = Buf<float>(m.pp(), (size_t)L * cap_enc * 2 * M);
        st->kenergy = Buf<float>(m.pp(), (size_t)L * M);
        st->pchoose = Buf<float>(m.pp(), (size_t)L * H);
        st->work = Buf<float>(m.pp(), work_n);
        st->ints = Buf<int>(m.pp(), 16 + 64);
        m.mma = std::move(st);
    }
    MmaState& st = *m.mma;
    st.s_enc = s_enc;
    st.pos = 0;
    const MmaWork w = mma_work(m, st.work.get(), nullptr);
    // d_pos @0, d_tok @8, finished @9, out_len @10, enc_lens @11
    const int32_t init[16] = {0, 0, 0, 0, 0, 0, 0, 0, cfg.pad_idx, 0, max_len, s_enc, 0, 0, 0, 0};
    SC_HIP(hipMemcpyAsync(st.ints.get(), init, sizeof(init), hipMemcpyHostToDevice, m.stream));
    // last pooled source position and its key-side energies, per layer
    const int ratio = cfg.mma_pre_decision_ratio;
    const int s_p = (s_enc + ratio - 1) / ratio;
    const int start = (s_p - 1) * ratio, count = s_enc - start;
    hipLaunchKernelGGL(mean_rows_kernel, dim3((M + 255) / 256), dim3(256), 0, m.stream, d_enc + (int64_t)start * M, count, M, w.pooled);
    SC_LAUNCH_CHECK();
    for (int li = 0; li < L; ++li)
        linear(m, d_enc, M, m.mma_dec[li].cross_kv, nullptr, 0, st.cross.get() + (int64_t)li * st.cap_enc * 2 * M, 2 * M, s_enc, ACT_NONE, 1.f);
    if (m.mma_ke_w && M <= 1024) {
        // key-side EnergyProjection of every layer on the same pooled row: one batched launch per MLP level
        const int E = cfg.mma_energy_layers;
        const float* src = w.pooled;
        int64_t src_ls = 0;
        for (int e = 0; e < E; ++e) {
            float* dst = (e + 1 == E) ? st.kenergy.get() : ((e & 1) ? w.qe1 : w.qe0);
            launch_energy_level(m, m.mma_ke_w + (size_t)e * L, m.mma_ke_b + (size_t)e * L, L, src, src_ls, dst);
            src = dst;
            src_ls = M;
        }
    } else {
        for (int li = 0; li < L; ++li) {
            const float* ke = energy_mlp(m, m.mma_pc[li].k, w.pooled, M, w.qe0, w.qe1, 1);
            SC_HIP(hipMemcpyAsync(st.kenergy.get() + (int64_t)li * M, ke, (size_t)M * 4, hipMemcpyDeviceToDevice, m.stream));
        }
    }
    SC_HIP(hipStreamSynchronize(m.stream));  // `init` is a host temporary; d_enc may be reused by the caller
}

void run_mma_step(Model& m, const int32_t* h_tokens, int n_tokens, const int32_t* h_blocked, int n_blocked, int32_t* out_index,
                  float* h_pchoose, float* d_features) {
    const sc_config& cfg = m.cfg;
    const int M = cfg.model_dim, L = cfg.mma_layers, H = cfg.num_heads, V = cfg.text_vocab_size;
    SC_CHECK(m.mma != nullptr && m.mma->s_enc > 0, "sc_mma_step: call sc_mma_begin first");
    MmaState& st = *m.mma;
    SC_CHECK(n_tokens >= 1 && st.pos + n_tokens <= st.cap, "sc_mma_step: %d tokens at position %d exceed max_len %d", n_tokens,
             st.pos, st.cap);
    SC_CHECK(n_blocked >= 0 && n_blocked <= 32, "sc_mma_step: at most 32 blocked indices (got %d)", n_blocked);
    for (int t = 0; t < n_tokens; ++t)
        SC_CHECK(h_tokens[t] >= 0 && h_tokens[t] < V, "sc_mma_step: token %d outside the vocabulary", h_tokens[t]);
    prof::set_tag("mma");
    const MmaWork w = mma_work(m, st.work.get(), nullptr);
    const DecStack W = mma_stack(m);
    StepCtx c;
    c.nb = 1;
    c.cap = st.cap;
    c.s_enc = st.cap_enc;  // geometry of the cross K/V buffer; the valid length sits in device memory (d_enc_lens)
    c.d_pos = st.ints.get();
    c.d_tok = st.ints.get() + 8;
    c.d_finished = st.ints.get() + 9;
    c.d_out_len = st.ints.get() + 10;
    c.d_enc_lens = st.ints.get() + 11;
    int* d_feed = st.ints.get() + 16;     // up to 32 tokens staged per chunk
    int* d_blocked = st.ints.get() + 48;  // up to 32 blocked indices
    c.x = w.x;
    c.h = w.h;
    c.att = w.att;
    c.hN = w.hN;
    c.wide = w.wide;
    c.partial = w.partial;
    c.logits = w.logits;
    c.qe0 = w.qe0;
    c.qe1 = w.qe1;
    c.d_hq = w.hq;
    c.stack = &W;
    c.d_kenergy = st.kenergy.get();
    c.d_pchoose = st.pchoose.get();
    const bool gen2 = choose_family(m, W, 1, 2) == 2;
    if (gen2) {  // second-generation step kernels, p_choose hook batched; planes live in the state (stable addresses)
        if (!st.planes.get()) {
            alloc_step2(m, c, cfg.mma_ffn_dim);
            st.planes = std::move(c.planes);
        }
        alloc_step2_views(m, c, cfg.mma_ffn_dim, st.planes.get());
    }
    const int64_t layer_stride = (int64_t)st.cap * M;
    for (int li = 0; li < L; ++li) {
        c.kcache.push_back(st.kv.get() + (int64_t)(2 * li) * layer_stride);
        c.vcache.push_back(st.kv.get() + (int64_t)(2 * li + 1) * layer_stride);
        c.cross_kv.push_back(st.cross.get() + (int64_t)li * st.cap_enc * 2 * M);
    }
    for (int t0 = 0; t0 < n_tokens; t0 += 32) {
        const int nt = std::min(32, n_tokens - t0);
        SC_HIP(hipMemcpyAsync(d_feed, h_tokens + t0, (size_t)nt * 4, hipMemcpyHostToDevice, m.stream));
        for (int t = 0; t < nt; ++t) {
            SC_HIP(hipMemcpyAsync(c.d_tok, d_feed + t, 4, hipMemcpyDeviceToDevice, m.stream));
            // eager launches: replaying a captured step measured no gain (a one-row step is 1.3 ms of dependent GPU work
            // either way, profiles/r2_stream_latency_graph.jsonl)
            c.pchoose = t0 + t == n_tokens - 1;
            decoder_step(m, c, /*project=*/false);  // advances *d_pos
            SC_HIP(hipMemcpyAsync(d_features + (int64_t)(t0 + t) * M, c.hN, (size_t)M * 4, hipMemcpyDeviceToDevice, m.stream));
        }
        SC_HIP(hipStreamSynchronize(m.stream));  // the pageable source of d_feed may be reused
    }
    // MonotonicDecoderModel.project (TiedProjection) on the last position + arg-max (online_text_decoder.py:225-231)
    Linear proj;
    proj.w = m.mma_embed;
    proj.ldw = M;
    proj.kpad = M;
    proj.in = M;
    proj.out = V;
    linear(m, c.hN, M, proj, nullptr, 0, c.logits, V, 1, ACT_NONE, 1.f);
    if (n_blocked > 0) {
        SC_HIP(hipMemcpyAsync(d_blocked, h_blocked, (size_t)n_blocked * 4, hipMemcpyHostToDevice, m.stream));
        hipLaunchKernelGGL(fill_indices_kernel, dim3(1), dim3(64), 0, m.stream, c.logits, d_blocked, n_blocked, V, -INFINITY);
        SC_LAUNCH_CHECK();
    }
    launch_argmax_rows(c.logits, V, 1, V, nullptr, 0, -1, -1, -1, -1, 0.f, c.d_tok, nullptr, m.stream);
    SC_HIP(hipMemcpyAsync(out_index, c.d_tok, 4, hipMemcpyDeviceToHost, m.stream));
    SC_HIP(hipMemcpyAsync(h_pchoose, st.pchoose.get(), (size_t)L * H * 4, hipMemcpyDeviceToHost, m.stream));
    SC_HIP(hipStreamSynchronize(m.stream));
    st.pos += n_tokens;
}

// Buffers of one greedy generation run and the step context that points into them.  Greedy generation keeps
// one of these per handle ACROSS sc_generate_text calls (Model::dec_session): the captured hipGraph of the step bakes
// the buffer addresses and the scalar step rules in, so a call with the same key replays the cached executable graph
// instead of capturing and instantiating a new one (round 1 did that on every call).
struct DecodeSession {
    // key
    int n = 0, max_len = 0, s_enc = 0, min_seq_len = 0, has_hidden = 0, fused_argmax = 0;
    float unk_penalty = 0.f;
    StepCtx c;
    Buf<int> ints;
    StepScratch scratch;
    Buf<float> fl, logits, am_eos, hidden;
    Buf<float4> am_part;
    std::vector<Buf<float>> caches;
    // cross-attention capture (sc_generate_text_capture): its own step graph (the step + the capture launch) and the buffers
    // that graph writes, allocated by the first capture call on this session; a plain call never replays this graph
    Buf<float> xattn, xlprob;  // [n][max_len][s_enc], [n][max_len]
    Buf<int> slot_tab;         // [n] utterance held by each row slot
    StepGraph graph, cgraph;   // declared last: gone before the buffers their nodes point into
};

void delete_decode_session(DecodeSession* s) { delete s; }

namespace {

// allocates every buffer of a run and fills the step context (no device work besides the allocations)
void setup_session(Model& m, DecodeSession& S, int n, int max_len, int s_enc, bool want_hidden, const sc_gen_opts& o) {
    const sc_config& cfg = m.cfg;
    const int M = cfg.model_dim;
    StepCtx& c = S.c;
    S.n = n, S.max_len = max_len, S.s_enc = s_enc, S.min_seq_len = o.min_seq_len, S.unk_penalty = o.unk_penalty;
    S.has_hidden = want_hidden;
    c.nb = n;
    c.cap = max_len;
    c.s_enc = s_enc;
    c.min_seq_len = o.min_seq_len;
    c.force_eos_step = max_len - 2;
    c.unk_penalty = o.unk_penalty;
    S.ints = Buf<int>(m.pp(), (size_t)8 + 5 * n + (size_t)n * max_len);
    c.d_pos = S.ints;
    c.d_rows_greedy = S.ints.get() + 1;  // becomes StepCtx::d_rows of a row-group (gen-3) generation session below
    c.d_tok = S.ints.get() + 8;
    c.d_finished = c.d_tok + n;
    c.d_out_len = c.d_finished + n;
    c.d_enc_lens = c.d_out_len + n;
    c.d_prompt_len = c.d_enc_lens + n;
    c.d_hist = c.d_prompt_len + n;
    S.fl = Buf<float>(m.pp(), (size_t)2 * n);
    c.d_lprob = S.fl;
    c.d_score = S.fl.get() + n;
    const DecStack W = unity_stack(m);
    const int family = choose_family(m, W, n, 0);
    const bool fused_argmax = fused_argmax_rows(n, M);
    S.fused_argmax = fused_argmax;
    init_step_scratch(m, S.scratch, c, W, n, family, StepTuning::from_knobs(n), /*wide_always=*/false);
    S.logits = Buf<float>(m.pp(), fused_argmax ? 4 : (size_t)n * cfg.text_vocab_size);
    c.logits = S.logits;
    if (family >= 2) {
        c.am_ntl = 4;
        c.am_tiles = fused_argmax ? gemvp_argmax_tiles(cfg.text_vocab_size, c.am_ntl) : 0;
        if (family == 3) {
            // greedy generation: the row-group kernels and the attention skip the row groups / rows behind *d_rows (= n until
            // the live-row compaction of run_generate_text lowers it); the captured step reads the counter on every replay
            c.d_rows = c.d_rows_greedy;
            c.am_tiles = std::max(c.am_tiles, vocab3_groups(n));
        }
    } else {
        c.am_tiles = fused_argmax ? skinny_argmax_tiles(n, cfg.text_vocab_size) : 0;
    }
    S.am_part = Buf<float4>(m.pp(), (size_t)std::max(1, c.am_tiles) * n);
    S.am_eos = Buf<float>(m.pp(), (size_t)n);
    c.am_part = S.am_part;
    c.am_eos_logit = S.am_eos;
    if (want_hidden) {
        S.hidden = Buf<float>(m.pp(), (size_t)n * (max_len - 1) * M);
        c.dec_hidden = S.hidden;
    }
    S.caches.reserve(3 * cfg.dec_layers);
    for (int li = 0; li < cfg.dec_layers; ++li) {
        S.caches.emplace_back(m.pp(), (size_t)n * max_len * M);
        c.kcache.push_back(S.caches.back());
        S.caches.emplace_back(m.pp(), (size_t)n * max_len * M);
        c.vcache.push_back(S.caches.back());
        S.caches.emplace_back(m.pp(), (size_t)n * s_enc * 2 * M);
        c.cross_kv.push_back(S.caches.back());
    }
}

}  // namespace

// Teacher-forced decoder pass over KNOWN tokens as ONE batched forward (all positions at once, causal self-attention) - the
// way the reference runs it (generator.py:294-299: `decode(text_seqs[:, :-1], ...)`) - instead of `s_text` single-position
// steps of ~220 dependent launches each: n * s_text rows through the tiled GEMMs, the multi-query attention kernel with its
// causal mask for the self-attention, the encoder K / V projected once.  Used behind the beam search (the decoder outputs of
// the chosen hypotheses feed the T2U model) and by sc_decode_text.
// Same modules in the same order as decoder_step (fairseq2.cpp:979-1094); results agree with the decoder outputs greedy
// generation keeps step by step to fp32 re-association (tests/test_stages_gpu.py:
// test_generated_hidden_equals_teacher_forced_pass, 2e-4).
// row_independent (sc_score_text): every product is the tiled one whatever the row count, so that an item's rows carry the same
// bits alone and in any batch; otherwise up to 64 rows take the skinny products (another summation order, linear()).
// d_xattn (sc_score_text_capture; with h_seq_lens [n], whole sequence lengths): one more launch in the LAST layer, behind its
// cross_q product and project_cross_kv - the head-summed attention rows of every item (launch_xattn_rows).  Nothing else changes.
void run_decode_text_batched(Model& m, const float* d_enc, int n, int s_enc, const int32_t* h_enc_lens, const int32_t* h_tokens, int s_text,
                             float* d_hidden, bool row_independent, float* d_xattn, const int32_t* h_seq_lens) {
    const sc_config& cfg = m.cfg;
    const int M = cfg.model_dim, rows = n * s_text, erows = n * s_enc;
    SC_CHECK(s_text <= cfg.text_max_seq_len, "sc_decode_text: %d tokens exceed text_max_seq_len=%d", s_text, cfg.text_max_seq_len);
    for (int i = 0; i < rows; ++i)
        SC_CHECK(h_tokens[i] >= 0 && h_tokens[i] < cfg.text_vocab_size, "sc_decode_text: token %d outside the vocabulary", h_tokens[i]);
    for (int b = 0; b < n; ++b) SC_CHECK(h_enc_lens[b] > 0 && h_enc_lens[b] <= s_enc, "sc_decode_text: enc_lens[%d]=%d out of range", b, h_enc_lens[b]);
    prof::set_tag("dec");
    Buf<int> d_tok(m.pp(), rows), d_elens(m.pp(), n), d_slens(m.pp(), d_xattn ? n : 0);
    SC_HIP(hipMemcpyAsync(d_tok.get(), h_tokens, (size_t)rows * 4, hipMemcpyHostToDevice, m.stream));
    SC_HIP(hipMemcpyAsync(d_elens.get(), h_enc_lens, (size_t)n * 4, hipMemcpyHostToDevice, m.stream));
    if (d_xattn) SC_HIP(hipMemcpyAsync(d_slens.get(), h_seq_lens, (size_t)n * 4, hipMemcpyHostToDevice, m.stream));
    const int wideN = std::max(3 * M, cfg.dec_ffn_dim);
    Buf<float> h(m.pp(), (size_t)rows * M), wide(m.pp(), (size_t)rows * wideN), att(m.pp(), (size_t)rows * M),
        ckv(m.pp(), (size_t)erows * 2 * M);
    float* x = d_hidden;
    launch_embed_tokens(d_tok, rows, m.text_embed, M, sqrtf((float)M), m.text_pos, nullptr, s_text, x, M, m.stream);
    BatchRows br;
    br.n = n, br.S = s_text, br.rows = rows;
    SelfAttn self_at;
    self_at.heads = cfg.num_heads;
    self_at.out = att;
    self_at.causal = 1;
    for (const DecoderLayer& l : m.dec) {
        // causal self-attention
        layernorm(m, x, l.self_ln, h, rows);
        linear(m, h, M, l.qkv, nullptr, 0, wide, 3 * M, rows, ACT_NONE, 1.f, row_independent);
        self_attention(m, wide, M, br, self_at);
        linear(m, att, M, l.self_out, x, M, x, M, rows, ACT_NONE, 1.f, row_independent);
        // encoder-decoder attention
        layernorm(m, x, l.cross_ln, h, rows);
        linear(m, h, M, l.cross_q, nullptr, 0, wide, M, rows, ACT_NONE, 1.f, row_independent);
        project_cross_kv(m, d_enc, l.cross_kv, ckv, erows);
        if (d_xattn && &l == &m.dec.back()) {
            XattnRowsArgs xr;
            xr.q = wide;
            xr.k = ckv;
            xr.ldq = M;
            xr.ldk = 2 * M;
            xr.enc_lens = d_elens;
            xr.tok_lens = d_slens;
            xr.xattn = d_xattn;
            xr.n = n, xr.S1 = s_text, xr.s_enc = s_enc, xr.heads = cfg.num_heads;
            launch_xattn_rows(xr, m.stream);
        }
        AttnArgs c;
        c.q = wide;
        c.k = ckv;
        c.v = ckv.get() + M;
        c.out = att;
        c.ldq = M;
        c.ldk = c.ldv = 2 * M;
        c.ldo = M;
        c.nb = n;
        c.heads = cfg.num_heads;
        c.Sq = s_text;
        c.Skv = s_enc;
        c.kv_lens = d_elens;
        launch_attention(c, m.stream);
        linear(m, att, M, l.cross_out, x, M, x, M, rows, ACT_NONE, 1.f, row_independent);
        // feed-forward network
        layernorm(m, x, l.ffn_ln, h, rows);
        linear(m, h, M, l.ffn_in, nullptr, 0, wide, cfg.dec_ffn_dim, rows, m.ffn_act, 1.f, row_independent);
        linear(m, wide, cfg.dec_ffn_dim, l.ffn_out, x, M, x, M, rows, ACT_NONE, 1.f, row_independent);
    }
    layernorm(m, x, m.dec_final_ln, x, rows);
    SC_HIP(hipStreamSynchronize(m.stream));  // h_tokens / h_enc_lens are the caller's; outputs complete on return
}

// Teacher-forced scoring (sc_score_text): the batched causal pass over tokens[:, :-1], then final_proj (tied to the embedding,
// no bias) and log-softmax over the vocabulary for the rows that have a target - position p < tok_lens[b] - 1 scores
// tokens[b][p + 1] - packed back to back as the T2U and vocoder passes pack theirs.  The [rows][V] logits are never formed:
// launch_gemm_presplit_score keeps per-row statistics in the product's epilogue.  The reference's evaluation loss runs the same
// three steps through PyTorch (cli/m4t/finetune/trainer.py:100-125, :155-188).  Own stream, never the decode engine.
// d_xattn (sc_score_text_capture): [n][s_text - 1][s_enc], the last layer's head-summed encoder-decoder attention of the same
// pass; every other output carries the bits of the call without it.
void run_score_text(Model& m, const float* d_enc, int n, int s_enc, const int32_t* h_enc_lens, const int32_t* h_tokens,
                    const int32_t* h_tok_lens, int s_text, float* h_tok_lprob, float* h_sum_lprob, int32_t* h_top1, float* d_dec_hidden,
                    float* d_xattn) {
    const sc_config& cfg = m.cfg;
    const int M = cfg.model_dim, V = cfg.text_vocab_size, S1 = s_text - 1;
    // every argument error before any device work
    SC_CHECK(n > 0 && s_enc > 0, "sc_score_text: empty batch");
    SC_CHECK(!m.dec.empty() && m.text_embed, "sc_score_text: the handle holds no text decoder");
    SC_CHECK(s_text >= 2, "sc_score_text: s_text=%d (a sequence holds a prompt token and a target at the least)", s_text);
    SC_CHECK(s_text <= cfg.text_max_seq_len, "sc_score_text: %d tokens exceed text_max_seq_len=%d", s_text, cfg.text_max_seq_len);
    SC_CHECK(M % 32 == 0, "sc_score_text: model_dim=%d is not a multiple of 32", M);
    if (d_xattn) check_xattn_rows_geometry(cfg.num_heads, M, "sc_score_text_capture");
    int R = 0;
    for (int b = 0; b < n; ++b) {
        SC_CHECK(h_tok_lens[b] >= 2 && h_tok_lens[b] <= s_text, "sc_score_text: tok_lens[%d]=%d outside [2, %d]", b, h_tok_lens[b], s_text);
        SC_CHECK(h_enc_lens[b] > 0 && h_enc_lens[b] <= s_enc, "sc_score_text: enc_lens[%d]=%d out of range", b, h_enc_lens[b]);
        R += h_tok_lens[b] - 1;
    }
    for (int64_t i = 0; i < (int64_t)n * s_text; ++i)
        SC_CHECK(h_tokens[i] >= 0 && h_tokens[i] < V, "sc_score_text: token %d outside the vocabulary", h_tokens[i]);
    std::vector<int32_t> in_tok((size_t)n * S1), row_idx((size_t)R), tgt((size_t)R);
    for (int b = 0, r = 0; b < n; ++b) {
        for (int p = 0; p < S1; ++p) in_tok[(size_t)b * S1 + p] = h_tokens[(size_t)b * s_text + p];
        for (int p = 0; p < h_tok_lens[b] - 1; ++p, ++r) {
            row_idx[r] = b * S1 + p;
            tgt[r] = h_tokens[(size_t)b * s_text + p + 1];
        }
    }
    Buf<float> own_hidden(m.pp(), d_dec_hidden ? 0 : (size_t)n * S1 * M);
    float* hidden = d_dec_hidden ? d_dec_hidden : own_hidden.get();
    // row-independent products: a sequence's scores must not depend on what it is batched with (n-best lists are compared)
    run_decode_text_batched(m, d_enc, n, s_enc, h_enc_lens, in_tok.data(), S1, hidden, /*row_independent=*/true, d_xattn, h_tok_lens);
    prof::set_tag("score");
    const int group = std::min(gemm_score_group_rows(V), (R + 255) / 256 * 256);
    Buf<int> d_idx(m.pp(), R), d_tgt(m.pp(), R), d_top1(m.pp(), R);
    Buf<float> packed(m.pp(), (size_t)R * M), d_lp(m.pp(), R), d_sum(m.pp(), R),
        rec(m.pp(), (size_t)group * gemm_score_records(V) * SCORE_REC_FLOATS);
    Buf<__half> ph(m.pp(), (size_t)R * M), pl(m.pp(), (size_t)R * M);
    SC_HIP(hipMemcpyAsync(d_idx.get(), row_idx.data(), (size_t)R * 4, hipMemcpyHostToDevice, m.stream));
    SC_HIP(hipMemcpyAsync(d_tgt.get(), tgt.data(), (size_t)R * 4, hipMemcpyHostToDevice, m.stream));
    launch_gather_rows(hidden, M, d_idx, packed, M, R, M, m.stream);
    launch_split_f32(packed, ph, pl, (int64_t)R * M, m.stream);
    GemmPsArgs a;
    a.Ah = ph;
    a.Al = pl;
    a.lda = M;
    a.W = m.text_embed;
    a.ldw = M;
    a.M = R;
    a.N = V;
    a.K = M;
    launch_gemm_presplit_score(a, d_tgt, rec, group, d_lp, h_sum_lprob ? d_sum.get() : nullptr, nullptr, h_top1 ? d_top1.get() : nullptr,
                               m.stream);
    std::vector<float> lp((size_t)R), sl(h_sum_lprob ? (size_t)R : 0);
    std::vector<int32_t> t1(h_top1 ? (size_t)R : 0);
    SC_HIP(hipMemcpyAsync(lp.data(), d_lp.get(), (size_t)R * 4, hipMemcpyDeviceToHost, m.stream));
    if (h_sum_lprob) SC_HIP(hipMemcpyAsync(sl.data(), d_sum.get(), (size_t)R * 4, hipMemcpyDeviceToHost, m.stream));
    if (h_top1) SC_HIP(hipMemcpyAsync(t1.data(), d_top1.get(), (size_t)R * 4, hipMemcpyDeviceToHost, m.stream));
    SC_HIP(hipStreamSynchronize(m.stream));
    // positions behind an item's last target: 0, and -1 for the arg-max
    for (int b = 0, r = 0; b < n; ++b)
        for (int p = 0; p < S1; ++p) {
            const bool live = p < h_tok_lens[b] - 1;
            const size_t o = (size_t)b * S1 + p;
            h_tok_lprob[o] = live ? lp[r] : 0.f;
            if (h_sum_lprob) h_sum_lprob[o] = live ? sl[r] : 0.f;
            if (h_top1) h_top1[o] = live ? t1[r] : -1;
            r += live;
        }
}

// Spoken-language identification (sc_identify_language): the prompt (normally {</s>}) goes through run_score_text's batched
// causal pass, and the NEXT position's log-softmax over the whole vocabulary is read at the candidate tokens - raw, no step
// rules: the reference's "LID scores" (ggml/examples/unity/fairseq2.cpp:1208-1221; its `unk` target language is the arg-max of
// them, :1227-1236).  The candidate values come out of the projection's epilogue (launch_gemm_presplit_score_cand), so item b's
// lprob[j] carries the bits sc_score_text returns for the sequence prefix + {cand[j]} at its last position, and depends on
// item b alone.  Own stream, never the decode engine.
void run_identify_language(Model& m, const float* d_enc, int n, int s_enc, const int32_t* h_enc_lens, const int32_t* h_prefix,
                           int prefix_len, const int32_t* h_cand, int n_cand, float* h_lprob, int32_t* h_best) {
    const sc_config& cfg = m.cfg;
    const int M = cfg.model_dim, V = cfg.text_vocab_size;
    // every argument error before any device work
    SC_CHECK(n > 0 && s_enc > 0, "sc_identify_language: empty batch");
    SC_CHECK(!m.dec.empty() && m.text_embed, "sc_identify_language: the handle holds no text decoder");
    SC_CHECK(prefix_len >= 1 && prefix_len <= cfg.text_max_seq_len, "sc_identify_language: prefix_len=%d outside [1, %d]", prefix_len,
             cfg.text_max_seq_len);
    SC_CHECK(M % 32 == 0, "sc_identify_language: model_dim=%d is not a multiple of 32", M);
    check_score_candidates(h_cand, n_cand, V, "sc_identify_language");
    for (int b = 0; b < n; ++b)
        SC_CHECK(h_enc_lens[b] > 0 && h_enc_lens[b] <= s_enc, "sc_identify_language: enc_lens[%d]=%d out of range", b, h_enc_lens[b]);
    for (int t = 0; t < prefix_len; ++t)
        SC_CHECK(h_prefix[t] >= 0 && h_prefix[t] < V, "sc_identify_language: prompt token %d outside the vocabulary", h_prefix[t]);
    std::vector<int32_t> in_tok((size_t)n * prefix_len), row_idx((size_t)n);
    for (int b = 0; b < n; ++b) {
        std::copy(h_prefix, h_prefix + prefix_len, in_tok.begin() + (size_t)b * prefix_len);
        row_idx[b] = b * prefix_len + prefix_len - 1;  // the position that predicts the language token
    }
    Buf<float> hidden(m.pp(), (size_t)n * prefix_len * M);
    run_decode_text_batched(m, d_enc, n, s_enc, h_enc_lens, in_tok.data(), prefix_len, hidden, /*row_independent=*/true);
    prof::set_tag("lid");
    const int group = std::min(gemm_score_group_rows(V), (n + 255) / 256 * 256);
    Buf<int> d_idx(m.pp(), n), d_cand(m.pp(), n_cand), d_best(m.pp(), n);
    Buf<float> packed(m.pp(), (size_t)n * M), d_lp(m.pp(), (size_t)n * n_cand), cand_v(m.pp(), (size_t)group * n_cand),
        rec(m.pp(), (size_t)group * gemm_score_records(V) * SCORE_REC_FLOATS);
    Buf<__half> ph(m.pp(), (size_t)n * M), pl(m.pp(), (size_t)n * M);
    SC_HIP(hipMemcpyAsync(d_idx.get(), row_idx.data(), (size_t)n * 4, hipMemcpyHostToDevice, m.stream));
    SC_HIP(hipMemcpyAsync(d_cand.get(), h_cand, (size_t)n_cand * 4, hipMemcpyHostToDevice, m.stream));
    launch_gather_rows(hidden, M, d_idx, packed, M, n, M, m.stream);
    launch_split_f32(packed, ph, pl, (int64_t)n * M, m.stream);
    GemmPsArgs a;
    a.Ah = ph;
    a.Al = pl;
    a.lda = M;
    a.W = m.text_embed;
    a.ldw = M;
    a.M = n;
    a.N = V;
    a.K = M;
    launch_gemm_presplit_score_cand(a, d_cand, n_cand, rec, cand_v, group, d_lp, d_best, m.stream);
    SC_HIP(hipMemcpyAsync(h_lprob, d_lp.get(), (size_t)n * n_cand * 4, hipMemcpyDeviceToHost, m.stream));
    SC_HIP(hipMemcpyAsync(h_best, d_best.get(), (size_t)n * 4, hipMemcpyDeviceToHost, m.stream));
    SC_HIP(hipStreamSynchronize(m.stream));  // row_idx / h_cand are host memory; outputs complete on return
}

namespace {
void run_generate_text(Model& m, const GenRequest& q, int max_len);  // the greedy loop, below
}

// The checks of a generation call and its route (GenRequest, model.h): the host-driven beam loop, the decode engine, or greedy
// generation on the handle's own chain.  Rows the handle announced to its engine (Engine::expect) are released exactly once
// on every route: here where the call leaves for a loop that never uses the engine, by Engine::generate where it takes them.
void route_generate_text(Model& m, const GenRequest& q) {
    const sc_config& cfg = m.cfg;
    const sc_gen_opts& o = q.opts;
    const int n = q.n, s_enc = q.s_enc;
    SC_CHECK(n > 0 && s_enc > 0, "sc_generate_text: empty batch");
    SC_CHECK(!q.h_prefix_lens || (!q.xcap && q.prefix_stride > 0), "sc_generate_text: per-row prompt lengths need per-row prompts");
    int longest_prefix = q.prefix_len;
    if (q.h_prefix_lens)
        for (int b = 0; b < n; ++b) {
            SC_CHECK(q.h_prefix_lens[b] >= q.prefix_len && q.h_prefix_lens[b] <= q.prefix_stride, "sc_generate_text: prompt length %d of row %d",
                     q.h_prefix_lens[b], b);
            longest_prefix = std::max(longest_prefix, q.h_prefix_lens[b]);
        }
    prof::set_tag("dec");
    SC_CHECK(o.beam_size >= 1, "sc_generate_text: beam_size=%d", o.beam_size);
    SC_CHECK(o.no_repeat_ngram_size >= 0, "sc_generate_text: no_repeat_ngram_size=%d", o.no_repeat_ngram_size);
    // the capture covers the greedy step chain only: the reference sums the attention over all beams of its beam batch,
    // whose layout this library does not reproduce, and the step processors run in the host-driven loop
    SC_CHECK(!q.xcap || (o.beam_size == 1 && o.no_repeat_ngram_size == 0),
             "sc_generate_text_capture: greedy generation only (beam_size=%d, no_repeat_ngram_size=%d are not supported)", o.beam_size,
             o.no_repeat_ngram_size);
    SC_CHECK(!q.xcap || !q.banned.any(), "sc_generate_text_capture: banned sequences are not supported");
    SC_CHECK(!q.xcap || !q.boost.any(), "sc_generate_text_capture: boost phrases are not supported");
    const int max_len = text_max_len(m, o, s_enc);
    if (o.beam_size > 1 || o.no_repeat_ngram_size > 0 || q.banned.any() || q.boost.any()) {  // step processors run in the host-driven step loop
        if (m.engine) m.engine->expect(m, -n);
        run_generate_beam(m, unity_stack(m), q, max_len);
        return;
    }
    SC_CHECK(q.prefix_len >= 1, "sc_generate_text: the prompt must hold at least one token");
    SC_CHECK(o.min_seq_len <= max_len, "sc_generate_text: min_seq_len %d > effective max length %d", o.min_seq_len, max_len);
    SC_CHECK(longest_prefix < max_len, "sc_generate_text: prompt length %d >= effective max length %d", longest_prefix, max_len);
    SC_CHECK(max_len <= 4096 && max_len <= cfg.text_max_seq_len + 1, "sc_generate_text: length %d exceeds the decoder limit", max_len);
    SC_CHECK(s_enc <= 4096, "sc_generate_text: encoder length %d > 4096", s_enc);
    for (int i = 0; i < n; ++i)
        SC_CHECK(q.h_enc_lens[i] > 0 && q.h_enc_lens[i] <= s_enc, "sc_generate_text: enc_lens[%d]=%d out of range", i, q.h_enc_lens[i]);

    // ---- decode engine (sc_engine_attach): the rows join the GPU's shared step chain (engine.hip) -------------------------
    // (a capture call does not fit: it runs on the handle's own chain, whose step the capture launch follows)
    if (m.engine && q.xcap) m.engine->expect(m, -n);
    if (m.engine && !q.xcap) {
        // (per-row prompts: the longest one decides - a call with a prompt beyond the admit record's capacity runs on the
        // handle's own chain as a whole)
        if (m.engine->fits(n, s_enc, max_len, longest_prefix, o) && m.engine->has_company()) {
            m.engine->generate(m, q, max_len);
            return;
        }
        m.engine->expect(m, -n);  // announced rows that run on the handle's own chain after all
    }
    run_generate_text(m, q, max_len);
}

namespace {

// Greedy generation on the handle's own step chain (route_generate_text made the checks; max_len: the effective length limit).
// With per-row prompt lengths the prompt echo runs as far as the shortest prompt for all rows, and the rows whose prompt is
// longer are fed the rest of it by the closing launch of the step (argmax_finalize_kernel), position by position, while the
// other rows already generate.
void run_generate_text(Model& m, const GenRequest& q, int max_len) {
    const sc_config& cfg = m.cfg;
    const sc_gen_opts& o = q.opts;
    const XattnCapture* xcap = q.xcap;
    const int M = cfg.model_dim, n = q.n, s_enc = q.s_enc, prefix_len = q.prefix_len;
    float* d_dec_hidden = q.d_dec_hidden;
    // ---- the run's buffers: the handle's cached session ---------------------------------------------------------------
    const bool want_hidden = d_dec_hidden != nullptr;
    DecodeSession* cur = m.dec_session.get();
    const bool hit = cur && cur->n == n && cur->max_len == max_len && cur->s_enc == s_enc && cur->min_seq_len == o.min_seq_len &&
                     cur->unk_penalty == o.unk_penalty && cur->has_hidden == (int)want_hidden;
    if (!hit) {
        m.dec_session.reset();  // the old buffers go back to the pool first
        // built aside and installed only when complete: an allocation that throws half way must not leave a session
        // whose key matches the next call but whose buffers are missing
        std::unique_ptr<DecodeSession, void (*)(DecodeSession*)> fresh(new DecodeSession(), delete_decode_session);
        setup_session(m, *fresh, n, max_len, s_enc, want_hidden, o);
        m.dec_session = std::move(fresh);
    }
    DecodeSession* S = m.dec_session.get();
    StepCtx& c = S->c;
    if (xcap) {
        SC_CHECK(xcap->d_xattn && xcap->h_step_lprob, "sc_generate_text_capture: null capture buffer");
        SC_CHECK(c.gen3 && c.d_rows == c.d_rows_greedy && c.am_tiles > 0,
                 "sc_generate_text_capture: needs the row-group decoder step (greedy, 1..64 rows; %d rows here)", n);
        SC_CHECK(cfg.num_heads <= XCAP_MAX_HEADS && M == cfg.num_heads * 64, "sc_generate_text_capture: %d heads of width %d (<= %d heads of 64)",
                 cfg.num_heads, M / cfg.num_heads, XCAP_MAX_HEADS);
        if (!S->xattn) {
            S->xattn = Buf<float>(m.pp(), (size_t)n * max_len * s_enc);
            S->xlprob = Buf<float>(m.pp(), (size_t)n * max_len);
            S->slot_tab = Buf<int>(m.pp(), (size_t)n);
        }
    }
    // the capture launch behind a step (projected: the step chose tokens)
    auto capture_node = [&](bool projected) {
        XattnCapArgs x;
        x.q = c.qkvr, x.kv = c.cross_kv.back(), x.enc_lens = c.d_enc_lens, x.d_pos = c.d_pos, x.d_rows = c.d_rows;
        x.finished = c.d_finished, x.out_len = c.d_out_len, x.slot_utt = S->slot_tab;
        if (projected) x.am_part = c.am_part, x.am_tiles = vocab3_groups(n), x.eos_logit = c.am_eos_logit, x.force_eos_step = c.force_eos_step;
        x.xattn = S->xattn, x.lprob = S->xlprob;
        x.nb = n, x.s_enc = s_enc, x.heads = cfg.num_heads, x.cap = max_len;
        launch_xattn_capture(x, m.stream);
    };

    // encoder-decoder K/V once per utterance (fairseq2 caches them in the state bag at step 0)
    for (int li = 0; li < cfg.dec_layers; ++li) project_cross_kv(m, q.d_enc, m.dec[li].cross_kv, c.cross_kv[li], n * s_enc);

    // ---- initial state ------------------------------------------------------------
    std::vector<int32_t> hist((size_t)n * max_len, cfg.pad_idx), init(8 + 5 * n, 0);
    for (int b = 0; b < n; ++b) {
        const int own_len = q.h_prefix_lens ? q.h_prefix_lens[b] : prefix_len;
        for (int t = 0; t < own_len; ++t) hist[(size_t)b * max_len + t] = q.h_prefix[(size_t)b * q.prefix_stride + t];
        init[8 + 4 * n + b] = own_len;  // StepCtx::d_prompt_len (a uniform call writes the shared length)
    }
    init[1] = n;  // live rows (StepCtx::d_rows_greedy)
    for (int b = 0; b < n; ++b) {
        init[8 + b] = hist[(size_t)b * max_len];  // token fed at position 0
        init[8 + n + b] = 0;                      // finished
        init[8 + 2 * n + b] = max_len;            // out_len default (forced EOS at the end)
        init[8 + 3 * n + b] = q.h_enc_lens[b];
    }
    SC_HIP(hipMemcpyAsync(S->ints.get(), init.data(), init.size() * 4, hipMemcpyHostToDevice, m.stream));
    SC_HIP(hipMemcpyAsync(c.d_hist, hist.data(), hist.size() * 4, hipMemcpyHostToDevice, m.stream));
    SC_HIP(hipMemsetAsync(S->fl.get(), 0, (size_t)2 * n * 4, m.stream));
    if (c.dec_hidden) SC_HIP(hipMemsetAsync(c.dec_hidden, 0, (size_t)n * (max_len - 1) * M * 4, m.stream));
    std::vector<int> slot_utt(n);
    for (int b = 0; b < n; ++b) slot_utt[b] = b;
    if (xcap) {
        SC_HIP(hipMemsetAsync(S->xattn.get(), 0, (size_t)n * max_len * s_enc * 4, m.stream));
        SC_HIP(hipMemsetAsync(S->xlprob.get(), 0, (size_t)n * max_len * 4, m.stream));
        SC_HIP(hipMemcpyAsync(S->slot_tab.get(), slot_utt.data(), (size_t)n * 4, hipMemcpyHostToDevice, m.stream));
    }

    // ---- prompt echo: positions 0 .. prefix_len-2 are fed without projection; the next input is read from hist ----
    for (int t = 0; t + 1 < prefix_len; ++t) {
        decoder_step(m, c, /*project=*/false);
        if (xcap) capture_node(false);
        SC_HIP(hipMemcpy2DAsync(c.d_tok, 4, c.d_hist + t + 1, (size_t)max_len * 4, 4, n, hipMemcpyDeviceToDevice, m.stream));
    }

    // ---- generation loop: step_nr = prefix_len-1 .. max_len-2 -----------------------
    const int first = prefix_len - 1;
    const bool use_graph = o.use_graph != 0;
    std::vector<int32_t> fin(n);
    // ---- live-row compaction (row-group chain): a step costs the same with 5 rows alive as with 64, and on a ragged batch a
    // third of the steps run with less than half of the rows alive (bench config.decoder_rows).  Whenever the host looks at
    // the finished flags, the rows still generating are packed to the front - each one behind the new boundary moves into the
    // slot of a finished row in front of it (row_swap_kernel: K / V rows, encoder K / V, tokens, scores; the finished row's
    // results move the other way) - and *d_rows drops to their number: the attention and reduce kernels skip the rows behind
    // it, the row-group products neither read nor write them and skip whole row groups, the vocabulary projection its 32-row halves.
    // slot_utt names the utterance a slot holds; results are handed out by utterance.  SC_GREEDY_COMPACT=0 keeps the rows
    // where they are.  A row's arithmetic does not depend on its slot (tests/test_eos_gpu.py: ids, hidden states, units and
    // waveforms equal to the un-compacted run and to the oracle).
    const bool compact = c.gen3 && c.d_rows == c.d_rows_greedy && n > 16 && cfg.dec_layers <= ROWSWAP_MAX_LAYERS && n <= 255 &&
                         M % 4 == 0 && knob::live("SC_GREEDY_COMPACT", 1) != 0;
    // steps between two looks of the host at the finished flags (each is a stream synchronisation); SC_GREEDY_POLL for A/B runs
    const int poll = std::min(64, std::max(1, knob::live("SC_GREEDY_POLL", 4)));
    int live_slots = n;
    bool moved = false;
    for (int step = first; step <= max_len - 2; ++step) {
        if (xcap) {
            if (!use_graph) {
                decoder_step(m, c, true);
                capture_node(true);
            } else {
                S->cgraph.ensure(m.stream, [&] {  // as the plain step graph below, with the capture launch at its end
                    decoder_step(m, c, true);
                    capture_node(true);
                });
                S->cgraph.launch(m.stream);
            }
        } else if (use_graph) {
            S->graph.ensure(m.stream, [&] { decoder_step(m, c, true); });
            {
                // one profiler record per replayed step (launches inside the graph cannot carry events): the algorithmic
                // bytes of a step are the fp16 weights of the layers and of the tied projection, read once for all rows,
                // plus the fp32 K/V rows the attention kernels read (self: positions 0..step, cross: every encoder row)
                const double w_bytes = 2.0 * ((double)cfg.dec_layers * (4.0 * M * M + 2.0 * M * M + 2.0 * (double)M * cfg.dec_ffn_dim) +
                                              (double)cfg.text_vocab_size * M);
                const double kv_bytes = 4.0 * cfg.dec_layers * (double)n * M * (2.0 * (step + 1) + 2.0 * s_enc);
                prof::Scope scope("step_graph", (double)n * w_bytes, w_bytes + kv_bytes, m.stream);
                S->graph.launch(m.stream);
            }
        } else {
            decoder_step(m, c, true);
        }
        if ((step - first + 1) % poll == 0 && step < max_len - 2) {
            SC_HIP(hipMemcpyAsync(fin.data(), c.d_finished, (size_t)n * 4, hipMemcpyDeviceToHost, m.stream));
            SC_HIP(hipStreamSynchronize(m.stream));
            bool all = true;
            for (int b = 0; b < n; ++b) all = all && fin[b];
            if (all) break;
            if (compact) {
                int alive = 0;
                for (int b = 0; b < live_slots; ++b) alive += fin[b] ? 0 : 1;
                const int want = std::max(1, alive);  // the rows still generating, packed to the front
                if (want < live_slots) {
                    RowSwapArgs rs;
                    rs.layers = cfg.dec_layers;
                    for (int li = 0; li < cfg.dec_layers; ++li) rs.k[li] = c.kcache[li], rs.v[li] = c.vcache[li], rs.cross[li] = c.cross_kv[li];
                    rs.M = M, rs.cap = c.cap, rs.s_enc = c.s_enc, rs.filled = step + 1;
                    rs.tok = c.d_tok, rs.finished = c.d_finished, rs.out_len = c.d_out_len, rs.enc_lens = c.d_enc_lens;
                    rs.prompt_len = c.d_prompt_len;
                    rs.lprob = c.d_lprob, rs.score = c.d_score, rs.hist = c.d_hist, rs.hidden = c.dec_hidden;
                    int free_slot = 0;
                    for (int b = want; b < live_slots; ++b) {
                        if (fin[b]) continue;
                        while (!fin[free_slot]) ++free_slot;  // alive <= want: a finished slot in front exists for every such row
                        rs.src[rs.pairs] = (unsigned char)b, rs.dst[rs.pairs] = (unsigned char)free_slot;
                        ++rs.pairs;
                        std::swap(slot_utt[b], slot_utt[free_slot]);
                        fin[free_slot] = 0, fin[b] = 1;
                        if (rs.pairs == ROWSWAP_MAX_PAIRS) {
                            launch_row_swap(rs, m.stream);
                            rs.pairs = 0;
                        }
                    }
                    launch_row_swap(rs, m.stream);
                    SC_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c.d_rows_greedy), want, 1, m.stream));
                    // the capture's slot -> utterance table (slot_utt is next written after the stream synchronisation of
                    // the next look, so the copy has its source until then)
                    if (xcap) SC_HIP(hipMemcpyAsync(S->slot_tab.get(), slot_utt.data(), (size_t)n * 4, hipMemcpyHostToDevice, m.stream));
                    live_slots = want;
                    moved = true;
                }
            }
        }
    }
    std::vector<int32_t> lens(n);
    std::vector<float> scores(n);
    SC_HIP(hipMemcpyAsync(hist.data(), c.d_hist, hist.size() * 4, hipMemcpyDeviceToHost, m.stream));
    SC_HIP(hipMemcpyAsync(lens.data(), c.d_out_len, (size_t)n * 4, hipMemcpyDeviceToHost, m.stream));
    SC_HIP(hipMemcpyAsync(scores.data(), c.d_score, (size_t)n * 4, hipMemcpyDeviceToHost, m.stream));
    if (xcap) {  // indexed by utterance already
        SC_HIP(hipMemcpyAsync(xcap->d_xattn, S->xattn.get(), (size_t)n * max_len * s_enc * 4, hipMemcpyDeviceToDevice, m.stream));
        SC_HIP(hipMemcpyAsync(xcap->h_step_lprob, S->xlprob.get(), (size_t)n * max_len * 4, hipMemcpyDeviceToHost, m.stream));
    }
    if (want_hidden) {
        const size_t row = (size_t)(max_len - 1) * M;
        if (!moved) {
            SC_HIP(hipMemcpyAsync(d_dec_hidden, c.dec_hidden, (size_t)n * row * 4, hipMemcpyDeviceToDevice, m.stream));
        } else {  // slot s holds utterance slot_utt[s]
            for (int s = 0; s < n; ++s)
                SC_HIP(hipMemcpyAsync(d_dec_hidden + (size_t)slot_utt[s] * row, c.dec_hidden + (size_t)s * row, row * 4, hipMemcpyDeviceToDevice,
                                      m.stream));
        }
    }
    SC_HIP(hipStreamSynchronize(m.stream));
    for (int s = 0; s < n; ++s) {
        const int b = slot_utt[s];
        const int len = lens[s];
        for (int t = 0; t < max_len; ++t) q.h_out_ids[(size_t)b * max_len + t] = t < len ? hist[(size_t)s * max_len + t] : cfg.pad_idx;
        q.h_out_lens[b] = len;
        if (q.h_scores) q.h_scores[b] = scores[s];
    }
}

}  // namespace

// --------------------------------------------------------------------------------------------- //
// Beam search (beam_size > 1): BeamSearchSeq2SeqGenerator as the reference constructs it
// (inference/generator.py:147-156; beam_size=5 is the API default, translator.py:311-313).  Algorithm
// restated from ggml/examples/unity/fairseq2.cpp:1371-1608 (see oracle/unity.py: beam_search_generate).
// Row r = utterance * beam + b of every decoder buffer is one live beam.  Per step: decoder step for all
// rows, vocabulary projection, beam_candidates_kernel (log-softmax + step rules + cumulative score +
// best 2*beam candidates per utterance), beam_select_kernel (the candidate walk: finalise EOS hypotheses,
// refill the beams, append the tokens - sequences and finished hypotheses stay in device memory), and the
// K/V caches are re-ordered on the device (double buffered, all layers in one launch).  No host round trip
// per step: the host polls the count of unfinished utterances every fourth step.
// Step processor: NGramRepeatBlockProcessor(G) (fairseq2 0.2 generation/step_processor.py, not under
// /root/reference; call site cli/m4t/predict/predict.py:172-175) — see ngram_blocked_tokens below.
// --------------------------------------------------------------------------------------------- //
// Tokens the n-gram processor blocks for one row: seq = the row's sequence so far (prompt included, S tokens).
// G >= S: nothing.  G == 1: every token of seq.  Otherwise every window seq[j..j+G) (j = 0..S-G) whose first
// G-1 tokens equal the last G-1 tokens of seq contributes its last token.
void ngram_blocked_tokens(const int32_t* seq, int S, int G, std::vector<int32_t>& out) {
    if (G <= 0 || G >= S) return;
    if (G == 1) {
        out.insert(out.end(), seq, seq + S);
        return;
    }
    const int32_t* tail = seq + S - (G - 1);
    for (int j = 0; j + G <= S; ++j)
        if (std::equal(seq + j, seq + j + G - 1, tail)) out.push_back(seq[j + G - 1]);
}

// Tokens the banned-sequence processor blocks for one row (fairseq2 0.2 BannedSequenceProcessor, restated; the class is
// not part of the reference tree): sequence q of length L blocks its last token when its first L-1 tokens equal the last L-1 tokens of seq
// (L-1 > S: no match; L == 1: always).  In banned-list order, duplicates kept.
void banned_blocked_tokens(const int32_t* seq, int S, const BannedHost& b, std::vector<int32_t>& out) {
    for (int q = 0; q < b.n; ++q) {
        const int32_t* w = b.tokens + b.offsets[q];
        const int P = b.offsets[q + 1] - b.offsets[q] - 1;
        if (P < 0 || P > S) continue;
        if (std::equal(w, w + P, seq + S - P)) out.push_back(w[P]);
    }
}

// UnitYT2UModel generation of the v1 models (inference/generator.py:316-336): T2U encoder over the text decoder output,
// then BeamSearchSeq2SeqGenerator over the unit decoder (unit_opts: beam_size 5, soft_max_seq_len (25, 50),
// generator.py:183-191) with the prompt [eos, lang] of the unit tokenizer.  Same search as the text decoder, other stack.
void run_t2u_ar(Model& m, const float* d_dec_hidden, int n, int s_text, const int32_t* h_text_lens, const sc_gen_opts& o,
                const int32_t* h_prefix, int prefix_len, int32_t* h_out_ids, int32_t* h_out_lens, float* h_scores) {
    const sc_config& cfg = m.cfg;
    SC_CHECK(cfg.has_t2u && cfg.t2u_variant == 1 && m.t2u_ar_embed, "sc_t2u_ar: the model was loaded without an autoregressive T2U");
    SC_CHECK(n > 0 && s_text > 0, "sc_t2u_ar: empty batch");
    prof::set_tag("t2u");
    const int M = cfg.model_dim;
    Buf<int> d_tlens(m.pp(), n);
    SC_HIP(hipMemcpyAsync(d_tlens.get(), h_text_lens, (size_t)n * 4, hipMemcpyHostToDevice, m.stream));
    Buf<float> enc(m.pp(), (size_t)n * s_text * M);
    run_t2u_encoder(m, d_dec_hidden, n, s_text, d_tlens, enc, h_text_lens);
    const DecStack W = t2u_ar_stack(m);
    // length rule of the unit generator: min(hard, int(a * S_text) + b), prompt included, capped by the position table
    const int src = o.source_len > 0 ? o.source_len : s_text;
    int max_len = o.soft_max_seq_len_a > 0 ? std::min(o.hard_max_seq_len, (int)(o.soft_max_seq_len_a * (float)src) + o.soft_max_seq_len_b)
                                           : o.hard_max_seq_len;
    max_len = std::min(max_len, W.max_seq_len);
    GenRequest q;
    q.d_enc = enc, q.n = n, q.s_enc = s_text, q.h_enc_lens = h_text_lens;
    q.opts = o;
    q.h_prefix = h_prefix, q.prefix_len = prefix_len;
    q.h_out_ids = h_out_ids, q.h_out_lens = h_out_lens, q.h_scores = h_scores;
    run_generate_beam(m, W, q, max_len);
}

// ---- pieces shared with sampled generation (model_sample.hip) ------------------------------------------------------------
void check_generation_limits(const char* who, const sc_gen_opts& o, int prefix_len, int max_len, int decoder_max_seq_len, int n, int s_enc,
                             const int32_t* h_enc_lens) {
    SC_CHECK(prefix_len >= 1, "%s: the prompt must hold at least one token", who);
    SC_CHECK(o.min_seq_len <= max_len, "%s: min_seq_len %d > effective max length %d", who, o.min_seq_len, max_len);
    SC_CHECK(prefix_len < max_len, "%s: prompt length %d >= effective max length %d", who, prefix_len, max_len);
    SC_CHECK(max_len <= 4096 && max_len <= decoder_max_seq_len + 1, "%s: length %d exceeds the decoder limit", who, max_len);
    SC_CHECK(s_enc <= 4096, "%s: encoder length %d > 4096", who, s_enc);
    for (int i = 0; i < n; ++i)
        SC_CHECK(h_enc_lens[i] > 0 && h_enc_lens[i] <= s_enc, "%s: enc_lens[%d]=%d out of range", who, i, h_enc_lens[i]);
}

// BannedSequenceProcessor: the list is checked on the host (before any launch) and copied to the device once per call
BannedDevice upload_banned(Model& m, const BannedHost& banned, int V) {
    BannedDevice d;
    if (!banned.any()) return d;
    validate_banned_host(banned.tokens, banned.offsets, banned.n, V, &d.list.max_len);
    const int total = banned.offsets[banned.n];
    d.store = Buf<int>(m.pp(), (size_t)total + banned.n + 1);
    SC_HIP(hipMemcpyAsync(d.store.get(), banned.tokens, (size_t)total * 4, hipMemcpyHostToDevice, m.stream));
    SC_HIP(hipMemcpyAsync(d.store.get() + total, banned.offsets, (size_t)(banned.n + 1) * 4, hipMemcpyHostToDevice, m.stream));
    SC_HIP(hipStreamSynchronize(m.stream));  // the list is the caller's
    d.list.tokens = d.store.get();
    d.list.offsets = d.store.get() + total;
    d.list.n = banned.n;
    return d;
}

// PhraseBoostProcessor: the list is checked and sorted on the host (before any launch) and copied to the device once per call
BoostSorted check_boost_host(const BoostHost& boost, int V, int pad_idx, int eos_idx) {
    BoostSorted sorted;
    const std::string why = boost_list_build(boost.tokens, boost.offsets, boost.n, V, pad_idx, eos_idx, sorted);
    SC_CHECK(why.empty(), "%s", why.c_str());
    const std::string bad = boost_value_check(boost.boost);
    SC_CHECK(bad.empty(), "%s", bad.c_str());
    return sorted;
}

BoostDevice upload_boost(Model& m, const BoostHost& boost, int V, int pad_idx, int eos_idx) {
    BoostDevice d;
    if (!boost.any()) return d;
    const BoostSorted sorted = check_boost_host(boost, V, pad_idx, eos_idx);
    const size_t total = sorted.tokens.size();
    d.store = Buf<int>(m.pp(), total + sorted.n + 1);
    SC_HIP(hipMemcpyAsync(d.store.get(), sorted.tokens.data(), total * 4, hipMemcpyHostToDevice, m.stream));
    SC_HIP(hipMemcpyAsync(d.store.get() + total, sorted.offsets.data(), (size_t)(sorted.n + 1) * 4, hipMemcpyHostToDevice, m.stream));
    SC_HIP(hipStreamSynchronize(m.stream));  // `sorted` is a host temporary
    d.list.tokens = d.store.get();
    d.list.offsets = d.store.get() + total;
    d.list.n = sorted.n;
    d.list.max_len = sorted.max_len;
    d.list.beta = boost.boost;
    return d;
}

// fairseq2.cpp `_fan_out_encoder_output`: row r of the result is the encoder output of item r / per_item
Buf<float> fan_out_encoder(Model& m, const float* d_enc, int n, int per_item, int s_enc) {
    const int M = m.cfg.model_dim, nb = n * per_item;
    Buf<float> enc_rep(m.pp(), (size_t)nb * s_enc * M);
    std::vector<int32_t> idx((size_t)nb * s_enc);
    for (int r = 0; r < nb; ++r)
        for (int t = 0; t < s_enc; ++t) idx[(size_t)r * s_enc + t] = (r / per_item) * s_enc + t;
    Buf<int> d_idx(m.pp(), idx.size());
    SC_HIP(hipMemcpyAsync(d_idx.get(), idx.data(), idx.size() * 4, hipMemcpyHostToDevice, m.stream));
    launch_gather_rows(d_enc, M, d_idx, enc_rep, M, nb * s_enc, M, m.stream);
    SC_HIP(hipStreamSynchronize(m.stream));  // idx is a host temporary
    return enc_rep;
}

void project_logits(Model& m, StepCtx& c, const DecStack& W, bool v3, int64_t ldl) {
    const int M = m.cfg.model_dim;
    if (v3) {
        Vocab3Args v;
        v.Wp = W.embed_p, v.Ah = c.hH, v.Al = c.hL, v.RB = c.rb, v.M = c.nb, v.N = W.vocab, v.K = M;
        v.logits = c.logits, v.ldl = ldl;
        v.d_rows = c.d_rows;
        launch_vocab3(v, m.stream);
    } else {
        Linear proj;
        proj.w = W.embed, proj.ldw = M, proj.kpad = M, proj.in = M, proj.out = W.vocab;
        linear(m, c.hN, M, proj, nullptr, 0, c.logits, W.vocab, c.nb, ACT_NONE, 1.f);
    }
}

void setup_hyp_rows(Model& m, HypRows& h, const DecStack& W, const GenRequest& q, int per_item, int max_len, const StepTuning& tuning) {
    const std::vector<DecoderLayer>& dec_layers = *W.layers;
    const sc_gen_opts& o = q.opts;
    const int M = m.cfg.model_dim, V = W.vocab, n = q.n, s_enc = q.s_enc, nb = n * per_item;
    // the packed-weight step kernels read the encoder K / V of live row r from cache row r / per_item: one projection per
    // utterance instead of one per hypothesis (5 x fewer bytes to project, to keep and to stream per step at beam 5)
    const int family = choose_family(m, W, nb, 1);  // (the v1 unit decoder's search decides the same way: callers 1 and 3)
    h.packed_step = family != 1;
    if (!h.packed_step) h.enc_rep = fan_out_encoder(m, q.d_enc, n, per_item, s_enc);  // the general step: one encoder K / V per row
    StepCtx& c = h.c;
    c.stack = &W;
    c.nb = nb, c.cap = max_len, c.s_enc = s_enc;
    c.min_seq_len = o.min_seq_len, c.force_eos_step = max_len - 2, c.unk_penalty = o.unk_penalty;
    h.ints = Buf<int>(m.pp(), (size_t)8 + 5 * nb);
    c.d_pos = h.ints;
    c.d_tok = h.ints.get() + 8;
    c.d_finished = c.d_tok + nb;
    c.d_out_len = c.d_finished + nb;
    c.d_enc_lens = c.d_out_len + nb;
    h.d_spare = c.d_enc_lens + nb;
    // packed-weight step kernels up to 64 live rows, the wide third-generation chain up to 512 (the step runs without its
    // projection here)
    init_step_scratch(m, h.scratch, c, W, nb, family, tuning);
    h.logits = Buf<float>(m.pp(), (size_t)nb * (V + 3));
    c.logits = h.logits;
    // vocabulary projection of the live rows: the LDS-staged streaming kernel on the packed embedding when the step left
    // the decoder output as split planes (<= 64 rows: at 60 rows the tiled GEMM needed ~10 ms per step, this one ~0.12)
    h.proj_v3 = c.rb > 0 && W.embed_p != nullptr && vocab3_supported(nb, V, M);
    h.ldl = h.proj_v3 ? (int64_t)align_up(V, 4) : V;  // 16-byte aligned rows for the streaming kernel
    const int cross_rows = h.packed_step ? n : nb;
    c.cross_row_div = h.packed_step ? per_item : 1;
    h.cross.reserve(dec_layers.size());
    for (const DecoderLayer& l : dec_layers) {
        h.cross.emplace_back(m.pp(), (size_t)cross_rows * s_enc * 2 * M);
        c.cross_kv.push_back(h.cross.back());
        project_cross_kv(m, h.packed_step ? q.d_enc : h.enc_rep.get(), l.cross_kv, c.cross_kv.back(), cross_rows * s_enc);
    }
}

void hidden_of_best(Model& m, const float* d_enc, int n, int s_enc, const int32_t* h_enc_lens, const int32_t* h_ids,
                    const int32_t* h_lens, int ids_stride, int max_len, int pad_idx, float* d_dec_hidden) {
    const int M = m.cfg.model_dim;
    int longest = 0;
    for (int u = 0; u < n; ++u) longest = std::max(longest, h_lens[(size_t)u * ids_stride]);
    const int fl = longest - 1;  // text_seqs[:, :-1]
    std::vector<int32_t> forced((size_t)n * fl, pad_idx);
    for (int u = 0; u < n; ++u)
        for (int t = 0; t < fl && t < h_lens[(size_t)u * ids_stride]; ++t) forced[(size_t)u * fl + t] = h_ids[(size_t)u * ids_stride * max_len + t];
    Buf<float> hid(m.pp(), (size_t)n * fl * M);
    run_decode_text_batched(m, d_enc, n, s_enc, h_enc_lens, forced.data(), fl, hid);
    SC_HIP(hipMemsetAsync(d_dec_hidden, 0, (size_t)n * (max_len - 1) * M * 4, m.stream));
    SC_HIP(hipMemcpy2DAsync(d_dec_hidden, (size_t)(max_len - 1) * M * 4, hid.get(), (size_t)fl * M * 4, (size_t)fl * M * 4, n,
                            hipMemcpyDeviceToDevice, m.stream));
    SC_HIP(hipStreamSynchronize(m.stream));
}

// Beam search over one decoder stack (the UnitY text decoder or the v1 autoregressive unit decoder).
void run_generate_beam(Model& m, const DecStack& W, const GenRequest& q, int max_len) {
    // The request's fields: GenRequest (model.h).  The score history (BeamHistArgs) exists only with q.nbest.  A per-row prompt is
    // fed to each beam of its utterance.  With per-row prompt lengths the host echo below runs as far as the shortest prompt;
    // from there an utterance that is still inside its prompt is
    // handled on the device (beam_prompt_kernel): each of its beams continues itself with the known token and adds that
    // token's raw log-probability - the echo's bits, added in the echo's order - while the candidate search and the step
    // processors leave the utterance alone; its "beam 0 only" step is the one at its own prompt's end.
    const sc_gen_opts& o = q.opts;
    const int n = q.n, s_enc = q.s_enc, prefix_len = q.prefix_len, prefix_stride = q.prefix_stride;
    const int32_t *h_prefix = q.h_prefix, *h_prefix_lens = q.h_prefix_lens, *h_enc_lens = q.h_enc_lens;
    const BeamNbestOut* nbest_out = q.nbest;
    float* d_dec_hidden = q.d_dec_hidden;
    int longest_prefix = prefix_len;
    if (h_prefix_lens) {
        SC_CHECK(prefix_stride > 0, "sc_generate_text: per-row prompt lengths need per-row prompts");
        for (int u = 0; u < n; ++u) {
            SC_CHECK(h_prefix_lens[u] >= prefix_len && h_prefix_lens[u] <= prefix_stride, "sc_generate_text: prompt length %d of row %d", h_prefix_lens[u], u);
            longest_prefix = std::max(longest_prefix, h_prefix_lens[u]);
        }
        SC_CHECK(longest_prefix < max_len, "sc_generate_text: prompt length %d >= effective max length %d", longest_prefix, max_len);
    }
    const bool ragged = longest_prefix > prefix_len;
    const std::vector<DecoderLayer>& dec_layers = *W.layers;
    const int M = m.cfg.model_dim, V = W.vocab, B = o.beam_size, L = (int)dec_layers.size();
    const int nb = n * B;
    const int K = std::min(2 * B, V - 1);
    SC_CHECK(B <= 8, "sc_generate_text: beam_size %d > 8", B);
    SC_CHECK(d_dec_hidden == nullptr || W.layers == &m.dec, "beam search: decoder outputs are captured for the text decoder only");
    const bool want_hist = nbest_out != nullptr;
    SC_CHECK(!want_hist || (nbest_out->nbest >= 1 && nbest_out->nbest <= B && !d_dec_hidden), "sc_generate_text_nbest: nbest %d outside 1..%d",
             want_hist ? nbest_out->nbest : 0, B);
    check_generation_limits("sc_generate_text", o, prefix_len, max_len, W.max_seq_len, n, s_enc, h_enc_lens);
    const BannedDevice banned_dev = upload_banned(m, q.banned, V);
    const BannedList& bl = banned_dev.list;
    const BoostDevice boost_dev = upload_boost(m, q.boost, V, W.pad_idx, W.eos_idx);
    const BoostList& bo = boost_dev.list;
    const float len_penalty = o.len_penalty;
    const bool normalize = o.normalize_scores != 0;

    // the step context of the beam rows (the beams of an utterance share its encoder K / V on the packed step kernels)
    HypRows hyp;
    setup_hyp_rows(m, hyp, W, q, B, max_len, StepTuning::from_knobs(nb));
    StepCtx& c = hyp.c;
    const bool packed_step = hyp.packed_step;
    const int64_t ldl = hyp.ldl;
    int* d_src_row = hyp.d_spare;
    Buf<float> d_cum(m.pp(), (size_t)nb), d_cand_val(m.pp(), (size_t)n * K), d_pref(m.pp(), (size_t)n);
    Buf<int> d_cand_idx(m.pp(), (size_t)n * K);
    // self-attention K/V caches of all layers in one allocation, twice (re-ordered from one into the other)
    const int64_t layer_stride = (int64_t)nb * max_len * M;
    // packed step kernels: ONE allocation + an ancestor table - a beam that continues another beam reads that beam's history
    // through the table (re-ordered in place by beam_select_kernel), no cache row is ever copied; the general step keeps the
    // two allocations re-ordered into each other after every step
    const bool use_anc = packed_step && (int64_t)nb * max_len * M * 4 < (1ll << 32);  // 32-bit byte offsets in dattn_kernel<false, true>
    Buf<float> kv_a(m.pp(), (size_t)2 * L * layer_stride), kv_b(m.pp(), use_anc ? 4 : (size_t)2 * L * layer_stride);
    Buf<int> d_anc(m.pp(), use_anc ? (size_t)nb * max_len : 4);
    if (use_anc) {
        std::vector<int32_t> ident((size_t)nb * max_len);
        for (int r = 0; r < nb; ++r) std::fill(ident.begin() + (size_t)r * max_len, ident.begin() + (size_t)(r + 1) * max_len, r);
        SC_HIP(hipMemcpyAsync(d_anc.get(), ident.data(), ident.size() * 4, hipMemcpyHostToDevice, m.stream));
        SC_HIP(hipStreamSynchronize(m.stream));  // `ident` is a host temporary
        c.anc = d_anc;
    }
    float* kv_cur = kv_a;
    float* kv_alt = kv_b;
    auto bind_caches = [&](float* base) {
        c.kcache.clear();
        c.vcache.clear();
        for (int li = 0; li < L; ++li) {
            c.kcache.push_back(base + (int64_t)(2 * li) * layer_stride);
            c.vcache.push_back(base + (int64_t)(2 * li + 1) * layer_stride);
        }
    };
    bind_caches(kv_cur);

    const bool chunked = beam_chunked(V, B, K);  // large vocabulary: candidate search spread over (row, chunk) workgroups
    Buf<float> ws_f(m.pp(), chunked ? beam_ws_floats(nb, K) : 4);
    Buf<int> ws_i(m.pp(), chunked ? beam_ws_ints(nb, K) : 4);
    auto project_rows = [&]() { project_logits(m, c, W, hyp.proj_v3, ldl); };

    // ---- search state: device resident (sequences, cumulative scores, finished hypotheses, counters) ----------
    std::vector<int32_t> seqs((size_t)nb * max_len, W.pad_idx), init(8 + 5 * nb, 0), tok(nb);
    std::vector<float> cum(nb, 0.f);
    for (int r = 0; r < nb; ++r) {
        const int32_t* pre = h_prefix + (size_t)(r / B) * prefix_stride;
        const int own_len = h_prefix_lens ? h_prefix_lens[r / B] : prefix_len;
        for (int t = 0; t < own_len; ++t) {
            SC_CHECK(pre[t] >= 0 && pre[t] < V, "sc_generate_text: prompt token %d out of range", pre[t]);
            seqs[(size_t)r * max_len + t] = pre[t];
        }
        init[8 + r] = pre[0];
        init[8 + 3 * nb + r] = h_enc_lens[r / B];
    }
    SC_HIP(hipMemcpyAsync(hyp.ints.get(), init.data(), init.size() * 4, hipMemcpyHostToDevice, m.stream));
    Buf<int> d_seqs_a(m.pp(), (size_t)nb * max_len), d_seqs_b(m.pp(), (size_t)nb * max_len), d_fin_seq(m.pp(), (size_t)nb * max_len),
        d_fin_len(m.pp(), (size_t)nb), d_state(m.pp(), (size_t)2 * n + 1);
    Buf<float> d_fin_score(m.pp(), (size_t)nb);
    int* d_seqs_cur = d_seqs_a;
    int* d_seqs_new = d_seqs_b;
    int* d_fin_count = d_state;
    int* d_done = d_state.get() + n;
    int* d_remaining = d_state.get() + 2 * n;
    {
        std::vector<int32_t> st((size_t)2 * n + 1, 0);
        st[2 * n] = n;
        SC_HIP(hipMemcpyAsync(d_state.get(), st.data(), st.size() * 4, hipMemcpyHostToDevice, m.stream));
        SC_HIP(hipMemcpyAsync(d_seqs_cur, seqs.data(), seqs.size() * 4, hipMemcpyHostToDevice, m.stream));
        SC_HIP(hipMemsetAsync(d_fin_len.get(), 0, (size_t)nb * 4, m.stream));
        SC_HIP(hipStreamSynchronize(m.stream));  // `st` is a host temporary
    }
    // score history of the live rows and of the finished hypotheses (n-best only): position 0 holds 0
    // (allocated by that entry alone: the other callers of this function allocate what they always did)
    Buf<float> d_hist_a, d_hist_b, d_fin_hist;
    std::vector<float> hist_rows;
    if (want_hist) {
        d_hist_a = Buf<float>(m.pp(), (size_t)nb * max_len);
        d_hist_b = Buf<float>(m.pp(), (size_t)nb * max_len);
        d_fin_hist = Buf<float>(m.pp(), (size_t)nb * max_len);
        hist_rows.assign((size_t)nb * max_len, 0.f);
        SC_HIP(hipMemsetAsync(d_hist_b.get(), 0, (size_t)nb * max_len * 4, m.stream));
        SC_HIP(hipMemsetAsync(d_fin_hist.get(), 0, (size_t)nb * max_len * 4, m.stream));
    }
    float* d_hist_cur = d_hist_a.get();
    float* d_hist_new = d_hist_b.get();
    std::vector<float> pref(n);
    const int G = o.no_repeat_ngram_size;
    Buf<int> d_plen(m.pp(), ragged ? (size_t)n : 4);  // by UTTERANCE (read through slot_utt when the slots are packed)
    if (ragged) {
        SC_HIP(hipMemcpyAsync(d_plen.get(), h_prefix_lens, (size_t)n * 4, hipMemcpyHostToDevice, m.stream));
        SC_HIP(hipStreamSynchronize(m.stream));  // the lengths are the caller's
    }

    // ---- live-slot bookkeeping (row-group chain + ancestor table only): the slots of utterances that are still searching are
    // packed to the front every time the host looks at the counters (every 4th step); kernels skip the rows / slots behind
    // *d_rows / *d_slots.  Finished hypotheses are stored per UTTERANCE (slot_utt maps a slot to its utterance), so the
    // results below are read in utterance order whatever moved.  SC_BEAM_COMPACT=0: every slot stays where it is.
    const bool compact_env = knob::live("SC_BEAM_COMPACT", 1) != 0;  // read per call, like SC_GREEDY_COMPACT (in-process A/B)
    const bool compact = compact_env && use_anc && c.gen3 && n >= 2 && n <= 1024;
    Buf<int> d_slot(m.pp(), compact ? (size_t)n + 2 : 4);
    int* d_slot_utt = d_slot.get();
    int* d_slots = d_slot.get() + n;
    int* d_rows_live = d_slot.get() + n + 1;
    if (compact) {
        std::vector<int32_t> sl((size_t)n + 2);
        for (int u = 0; u < n; ++u) sl[u] = u;
        sl[n] = n;
        sl[n + 1] = nb;
        SC_HIP(hipMemcpyAsync(d_slot.get(), sl.data(), sl.size() * 4, hipMemcpyHostToDevice, m.stream));
        SC_HIP(hipStreamSynchronize(m.stream));  // `sl` is a host temporary
        c.d_rows = d_rows_live;
        c.kv_item = d_slot_utt;
    }

    // ---- prompt echo: feed prefix[:-1]; cum = sum_j lprob(prefix[j] | prefix[<j]) (the same for every beam row) ----
    for (int t = 0; t + 1 < prefix_len; ++t) {
        decoder_step(m, c, /*project=*/false);
        project_rows();
        // (the step has consumed d_tok: the next tokens go up first, and the per-row-token kernel reads them from there)
        for (int r = 0; r < nb; ++r) {
            tok[r] = h_prefix[(size_t)(r / B) * prefix_stride + t + 1];
            SC_CHECK(tok[r] >= 0 && tok[r] < V, "sc_generate_text: prompt token %d out of range", tok[r]);
        }
        SC_HIP(hipMemcpyAsync(c.d_tok, tok.data(), (size_t)nb * 4, hipMemcpyHostToDevice, m.stream));
        launch_row_tokens_lprob(c.logits, ldl, n, V, B, c.d_tok, d_pref, m.stream);
        SC_HIP(hipMemcpyAsync(pref.data(), d_pref.get(), (size_t)n * 4, hipMemcpyDeviceToHost, m.stream));
        SC_HIP(hipStreamSynchronize(m.stream));
        for (int r = 0; r < nb; ++r) cum[r] += pref[r / B];
        if (want_hist)  // the partial sums, as they are added
            for (int r = 0; r < nb; ++r) hist_rows[(size_t)r * max_len + t + 1] = cum[r];
    }
    SC_HIP(hipMemcpyAsync(d_cum.get(), cum.data(), (size_t)nb * 4, hipMemcpyHostToDevice, m.stream));
    if (want_hist) SC_HIP(hipMemcpyAsync(d_hist_cur, hist_rows.data(), hist_rows.size() * 4, hipMemcpyHostToDevice, m.stream));

    // ---- search: every step is device work only; the host polls the `remaining` counter every 4th step --------
    const int start = prefix_len - 1;
    int remaining = n;
    // The decoder step of the search is replayed from a captured hipGraph like the greedy one (~220 launches per step: eager
    // launching alone cost ~2.5 ms per step at 320 rows).  The K/V caches alternate between two allocations (re-ordered from
    // one into the other after every step), so there are two graphs, one per parity; everything the step reads besides its
    // baked-in buffer addresses lives in device memory (*d_pos, d_tok).
    StepGraph graphs[2];
    const bool step_graph = o.use_graph != 0 && c.rb > 0;
    for (int step = start; step <= max_len - 2 && remaining > 0; ++step) {
        if (step_graph) {
            StepGraph& g = graphs[kv_cur == kv_a.get() ? 0 : 1];
            g.ensure(m.stream, [&] { decoder_step(m, c, /*project=*/false); });
            g.launch(m.stream);
        } else {
            decoder_step(m, c, /*project=*/false);  // feeds d_tok at position `step`, advances *d_pos
        }
        project_rows();
        // step processors: not on the forced-EOS step (blocking EOS there would leave no hypothesis)
        const bool ban = (G > 0 || bl.n > 0 || bo.n > 0) && step != max_len - 2;
        BeamPrompt bp;  // empty unless an utterance may still be inside its prompt or at its end
        if (ragged && step < longest_prefix) {
            bp.len = d_plen, bp.slot_utt = compact ? d_slot_utt : nullptr, bp.step = step;
            // first in the stream: it reads the logit rows before a step processor writes into them
            launch_beam_prompt(c.logits, ldl, n, B, V, d_cum, d_seqs_cur, max_len, K, d_cand_val, d_cand_idx, bp, compact ? d_slots : nullptr,
                               m.stream);
        }
        if (chunked) {
            launch_beam_candidates_chunked(c.logits, ldl, n, B, V, d_cum, step == start, step < o.min_seq_len, step == max_len - 2,
                                           W.pad_idx, W.eos_idx, W.unk_idx, o.unk_penalty, K, d_cand_val, d_cand_idx,
                                           ban ? d_seqs_cur : nullptr, max_len, step + 1, G, ws_f, ws_i, m.stream,
                                           compact ? d_rows_live : nullptr, compact ? d_slots : nullptr, bl.n > 0 ? &bl : nullptr,
                                           bo.n > 0 ? &bo : nullptr, bp);
        } else {
            launch_beam_candidates(c.logits, ldl, n, B, V, d_cum, step == start, step < o.min_seq_len, step == max_len - 2, W.pad_idx,
                                   W.eos_idx, W.unk_idx, o.unk_penalty, K, d_cand_val, d_cand_idx, ban ? d_seqs_cur : nullptr, max_len,
                                   step + 1, G, m.stream, compact ? d_slots : nullptr, bl.n > 0 ? &bl : nullptr, bo.n > 0 ? &bo : nullptr, bp);
        }
        BeamSelectArgs a;
        a.cand_val = d_cand_val;
        a.cand_idx = d_cand_idx;
        a.seqs_cur = d_seqs_cur;
        a.seqs_new = d_seqs_new;
        a.fin_score = d_fin_score;
        a.fin_len = d_fin_len;
        a.fin_seq = d_fin_seq;
        a.fin_count = d_fin_count;
        a.done = d_done;
        a.remaining = d_remaining;
        a.tok = c.d_tok;
        a.src_row = d_src_row;
        a.cum = d_cum;
        a.beams = B;
        a.K = K;
        a.V = V;
        a.max_len = max_len;
        a.step = step;
        a.eos_idx = W.eos_idx;
        a.pad_idx = W.pad_idx;
        a.normalize = normalize ? 1 : 0;
        a.len_penalty = len_penalty;
        a.anc = use_anc ? d_anc.get() : nullptr;
        a.anc_ld = max_len;
        a.slot_utt = compact ? d_slot_utt : nullptr;
        a.d_slots = compact ? d_slots : nullptr;
        BeamHistArgs bh;
        bh.cur = d_hist_cur, bh.next = d_hist_new, bh.fin = d_fin_hist;
        launch_beam_select(a, n, m.stream, want_hist ? &bh : nullptr);
        std::swap(d_seqs_cur, d_seqs_new);
        std::swap(d_hist_cur, d_hist_new);
        if (!use_anc) {
            // K/V rows follow their beams (all layers, one launch; rows of finished utterances map onto themselves)
            launch_gather_cache(kv_cur, kv_alt, d_src_row, nb, step + 1, max_len, M, 2 * L, layer_stride, m.stream);
            std::swap(kv_cur, kv_alt);
            bind_caches(kv_cur);
        }
        if (((step - start) & 3) == 3 || step == max_len - 2) {
            if (compact && step != max_len - 2) {  // utterances that finished since the last look leave the live rows
                BeamCompactArgs k;
                k.done = d_done, k.slot_utt = d_slot_utt, k.d_slots = d_slots, k.d_rows = d_rows_live;
                k.seqs = d_seqs_cur, k.cum = d_cum, k.tok = c.d_tok, k.enc_lens = c.d_enc_lens, k.anc = d_anc;
                // (a slot that is still inside its prompt carries the rest of the prompt behind the positions written so far)
                k.n = n, k.beams = B, k.max_len = max_len, k.anc_ld = max_len, k.seq_len = std::max(step + 2, longest_prefix), k.anc_len = step + 1;
                launch_beam_compact(k, m.stream, want_hist ? d_hist_cur : nullptr);
            }
            SC_HIP(hipMemcpyAsync(&remaining, d_remaining, 4, hipMemcpyDeviceToHost, m.stream));
            SC_HIP(hipStreamSynchronize(m.stream));
        }
    }

    // ---- every finished hypothesis, ranked on the device (beam_nbest_kernel: the order of the loop below) ----
    if (want_hist) {
        const int nbest = nbest_out->nbest;
        const size_t rows = (size_t)n * nbest;
        std::vector<int32_t> fin_count(n);
        SC_HIP(hipMemcpyAsync(fin_count.data(), d_fin_count, (size_t)n * 4, hipMemcpyDeviceToHost, m.stream));
        SC_HIP(hipStreamSynchronize(m.stream));
        for (int u = 0; u < n; ++u) SC_CHECK(fin_count[u] > 0, "sc_generate_text_nbest: beam search returned no hypothesis for item %d", u);
        Buf<int> d_out_i(m.pp(), rows * max_len + rows + n);
        Buf<float> d_out_f(m.pp(), rows * max_len + rows);
        BeamNbestArgs k;
        k.fin_seq = d_fin_seq, k.fin_len = d_fin_len, k.fin_score = d_fin_score, k.fin_hist = d_fin_hist, k.fin_count = d_fin_count;
        k.out_ids = d_out_i, k.out_lens = d_out_i.get() + rows * max_len, k.out_counts = k.out_lens + rows;
        k.out_step = d_out_f, k.out_scores = d_out_f.get() + rows * max_len;
        k.n = n, k.beams = B, k.nbest = nbest, k.max_len = max_len, k.pad_idx = W.pad_idx;
        launch_beam_nbest(k, m.stream);
        SC_HIP(hipMemcpyAsync(nbest_out->h_ids, k.out_ids, rows * max_len * 4, hipMemcpyDeviceToHost, m.stream));
        SC_HIP(hipMemcpyAsync(nbest_out->h_lens, k.out_lens, rows * 4, hipMemcpyDeviceToHost, m.stream));
        SC_HIP(hipMemcpyAsync(nbest_out->h_counts, k.out_counts, (size_t)n * 4, hipMemcpyDeviceToHost, m.stream));
        SC_HIP(hipMemcpyAsync(nbest_out->h_scores, k.out_scores, rows * 4, hipMemcpyDeviceToHost, m.stream));
        if (nbest_out->h_step) SC_HIP(hipMemcpyAsync(nbest_out->h_step, k.out_step, rows * max_len * 4, hipMemcpyDeviceToHost, m.stream));
        SC_HIP(hipStreamSynchronize(m.stream));
        return;
    }

    // ---- best hypothesis per utterance (sorted by score, fairseq2.cpp:1597-1602) ----------------------
    std::vector<int32_t> fin_seq((size_t)nb * max_len), fin_len(nb), fin_count(n);
    std::vector<float> fin_score(nb);
    SC_HIP(hipMemcpyAsync(fin_seq.data(), d_fin_seq.get(), fin_seq.size() * 4, hipMemcpyDeviceToHost, m.stream));
    SC_HIP(hipMemcpyAsync(fin_len.data(), d_fin_len.get(), fin_len.size() * 4, hipMemcpyDeviceToHost, m.stream));
    SC_HIP(hipMemcpyAsync(fin_score.data(), d_fin_score.get(), fin_score.size() * 4, hipMemcpyDeviceToHost, m.stream));
    SC_HIP(hipMemcpyAsync(fin_count.data(), d_fin_count, (size_t)n * 4, hipMemcpyDeviceToHost, m.stream));
    SC_HIP(hipStreamSynchronize(m.stream));
    for (int u = 0; u < n; ++u) {
        SC_CHECK(fin_count[u] > 0, "sc_generate_text: beam search returned no hypothesis for item %d", u);
        // the order of the candidate search (k_beam.hip order_key): NaN first, then the higher score, ties to the earlier one
        int best = 0;
        for (int i = 1; i < fin_count[u]; ++i) {
            const float s = fin_score[u * B + i], t = fin_score[u * B + best];
            if (std::isnan(t) ? false : (std::isnan(s) || s > t)) best = i;
        }
        const int len = fin_len[u * B + best];
        const int32_t* hs = &fin_seq[(size_t)(u * B + best) * max_len];
        for (int t = 0; t < max_len; ++t) q.h_out_ids[(size_t)u * max_len + t] = t < len ? hs[t] : W.pad_idx;
        q.h_out_lens[u] = len;
        if (q.h_scores) q.h_scores[u] = fin_score[u * B + best];
    }
    // ---- decoder outputs of the chosen hypotheses: the reference's teacher-forced pass (generator.py:281-299)
    if (d_dec_hidden) hidden_of_best(m, q.d_enc, n, s_enc, h_enc_lens, q.h_out_ids, q.h_out_lens, 1, max_len, W.pad_idx, d_dec_hidden);
}

}  // namespace sc
