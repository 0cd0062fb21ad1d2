// Host-side runtime of libseamless_hip: weights resident in HBM, a caching
// device allocator for activations, and the per-stage launch sequences.
#pragma once
#include <algorithm>
#include <map>
#include <functional>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/seamless_hip.h"
#include "kernels.h"

namespace sc {

// Size-bucketed caching allocator.  Every launch of a handle goes to ONE
// stream, so a block can be handed out again as soon as the host released it:
// stream order already serialises the old readers and the new writer.
class DevicePool {
   public:
    ~DevicePool();
    void* get(size_t bytes);
    void put(void* p);
    void release_all();
    void trim();  // hipFree every cached (not handed out) block
    // the one stream every user of this pool's blocks launches on (the handle's): the SC_DEBUG_FILL fill is ordered on it
    void set_stream(hipStream_t s) { stream_ = s; }
    // called when hipMalloc fails after this pool's own cache was trimmed: the owner frees what its OTHER pools cache
    // (a handle's side chains each cache their own copy of the vocoder scratch) before the allocation is retried
    void set_oom_hook(std::function<void()> f) { oom_hook_ = std::move(f); }

   private:
    std::function<void()> oom_hook_;
    void* debug_filled(void* p, size_t bytes);
    hipStream_t stream_ = nullptr;
    std::multimap<size_t, void*> free_;
    std::unordered_map<void*, size_t> size_;
    size_t cached_bytes_ = 0;  // bytes sitting in free_
};

template <typename T>
class Buf {
   public:
    Buf() = default;
    Buf(DevicePool* pool, size_t n) : pool_(pool), n_(n) { p_ = n ? static_cast<T*>(pool->get(n * sizeof(T))) : nullptr; }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept : pool_(o.pool_), p_(o.p_), n_(o.n_) { o.p_ = nullptr; }
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) {
            reset();
            pool_ = o.pool_;
            p_ = o.p_;
            n_ = o.n_;
            o.p_ = nullptr;
        }
        return *this;
    }
    ~Buf() { reset(); }
    void reset() {
        if (p_) pool_->put(p_);
        p_ = nullptr;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t size() const { return n_; }

   private:
    DevicePool* pool_ = nullptr;
    T* p_ = nullptr;
    size_t n_ = 0;
};

struct Linear {
    const __half* w = nullptr;  // [out][ldw]
    const __half* wp = nullptr;  // the same values packed into MFMA fragment order (k_dstep.hip); decoder-step products only
    int64_t ldw = 0;
    const float* b = nullptr;
    int out = 0, in = 0, kpad = 0;
};
struct LNorm {
    const float* g = nullptr;
    const float* b = nullptr;
    int dim = 0;
};
struct Conv {
    const __half* w = nullptr;  // packed [cout][kpad]
    const float* b = nullptr;
    int cout = 0, cin = 0, k = 0, kpad = 0;
};
struct ConvT {
    const __half* w = nullptr;  // [stride][cout][kpad]
    const float* b = nullptr;
    int cin = 0, cout = 0, k = 0, stride = 0, pad = 0, taps = 0, kpad = 0;
};

struct ConformerLayer {
    LNorm ffn1_ln, attn_ln, conv_ln, conv_inner_ln, ffn2_ln, final_ln;
    Linear ffn1_in, ffn1_out, ffn2_in, ffn2_out, qkv, attn_out, pw1, pw2;
    Linear pw1g;  // enc_variant 0: pw1 with its value and gate rows interleaved, for the GLU epilogue (launch_gemm_presplit_glu)
    const float* rel_k = nullptr;  // [npos][64] fp32 (enc_variant 0)
    const float* dw = nullptr;     // [C][k] fp32
    // enc_variant 1 (v1 w2v-BERT): Transformer-XL relative positions + BatchNorm folded to scale / shift
    Linear r_proj;
    const float* u_bias = nullptr;    // [heads * 64]
    const float* v_bias = nullptr;    // [heads * 64]
    const float* bn_scale = nullptr;  // [C]
    const float* bn_shift = nullptr;  // [C]
};
struct AdaptorLayer {
    LNorm res_ln, attn_ln, ffn_ln;
    Conv res_conv, attn_conv;
    Linear qkv, attn_out, ffn_in, ffn_out;
};
struct DecoderLayer {
    LNorm self_ln, cross_ln, ffn_ln;
    Linear qkv, self_out, cross_q, cross_kv, cross_out, ffn_in, ffn_out;
};
struct PChooseLayer {  // monotonic decoder: EnergyProjection MLPs of the query / pooled-key sides + energy bias
    std::vector<Linear> q, k;
    const float* energy_bias = nullptr;  // [1] or null
};
// One pre-LN transformer decoder (embedding frontend, layers, final LayerNorm): the UnitY text decoder or the
// streaming monotonic decoder.  Views into ModelData.
struct DecStack {
    const __half* embed = nullptr;
    const __half* embed_p = nullptr;  // packed copy (vocabulary projection of the second-generation step)
    const float* pos = nullptr;
    const std::vector<DecoderLayer>* layers = nullptr;
    const LNorm* final_ln = nullptr;
    int ffn_dim = 0;
    int ffn_act = ACT_RELU;  // inner activation of the FFNs (ACT_GELU: the expressive model's NLLB decoder)
    const std::vector<PChooseLayer>* pchoose = nullptr;
    // vocabulary of the stack (beam search): size, special symbols, longest sequence of the position table
    int vocab = 0, pad_idx = 0, unk_idx = 1, eos_idx = 3, max_seq_len = 0;
};
struct EncoderLayer {  // standard pre-LN transformer encoder layer (T2U encoder)
    LNorm attn_ln, ffn_ln;
    Linear qkv, attn_out, ffn_in, ffn_out;
};
struct FFTLayer {  // NAR decoder layer (post-LN)
    Linear qkv, attn_out;
    LNorm attn_ln, conv_ln;
    Conv conv1, conv2;
    int film_off = 0;  // FiLM models: where the layer's gamma' | beta' sit in a row of the conditioning table
};
struct ResBlock {
    std::vector<Conv> convs1, convs2;
    std::vector<int> dil;
};

// Everything that describes the loaded model: views into the weight allocations and the host-side
// NAR tables.  Plain copyable data: a forked handle (sc_fork) copies it and shares the allocations.
struct ModelData {
    sc_config cfg{};
    int device = 0;
    // sc_load_ext: inner activation of the adaptor / NLLB FFNs and of the T2U encoder FFNs (ACT_RELU or ACT_GELU), width of the
    // FiLM conditioning vector of the NAR T2U (0: no FiLM)
    int ffn_act = ACT_RELU, t2u_ffn_act = ACT_RELU, film_cond_dim = 0;

    // raw uploaded tensors by name
    struct Raw {
        void* p;
        int dtype;
        std::vector<int64_t> shape;
        int64_t numel;
    };
    std::unordered_map<std::string, Raw> raw;

    // speech encoder
    float* fbank_consts = nullptr;
    LNorm fe_ln;
    Linear fe_proj;
    std::vector<ConformerLayer> enc;
    LNorm enc_inner_ln, enc_final_ln;
    Linear enc_proj1, enc_proj2;
    AdaptorLayer adaptor;
    // text decoder
    const __half* text_embed = nullptr;  // [V][M]
    const __half* text_embed_p = nullptr;  // packed copy for the vocabulary projection of the decoder step
    const float* text_pos = nullptr;     // [max_len][M]
    std::vector<DecoderLayer> dec;
    LNorm dec_final_ln;
    // streaming monotonic text decoder (cfg 5; models/monotonic_decoder): own embedding, layers + p_choose
    const __half* mma_embed = nullptr;
    const __half* mma_embed_p = nullptr;
    std::vector<DecoderLayer> mma_dec;
    std::vector<PChooseLayer> mma_pc;
    // query-side energy MLPs of all layers as device pointer tables [energy_layers][mma_layers] (weights fp16 [M][ldw],
    // biases fp32 [M]) + the per-layer energy bias pointers: one batched launch per MLP level (model_dstep.hip)
    const __half* const* mma_qe_w = nullptr;
    const float* const* mma_qe_b = nullptr;
    const float* const* mma_ebias = nullptr;
    const __half* const* mma_ke_w = nullptr;  // key-side energy MLPs, same table layout
    const float* const* mma_ke_b = nullptr;
    int mma_qe_ldw = 0;
    LNorm mma_final_ln;
    // text encoder (text-input tasks; shares the embedding frontend with the decoder)
    std::vector<EncoderLayer> text_enc;
    LNorm text_enc_ln;
    // t2u
    std::vector<EncoderLayer> t2u_enc;
    LNorm t2u_enc_ln;
    const __half* unit_embed = nullptr;
    const __half* char_embed = nullptr;
    const float* char_pos = nullptr;
    const float* unit_pos = nullptr;
    float pos_alpha = 1.f, pos_alpha_char = 1.f;
    Conv dp_conv1, dp_conv2;
    LNorm dp_ln1, dp_ln2;
    // v1 autoregressive T2U (UnitYT2UModel, models/unity/t2u_builder.py:140-183): unit embedding frontend + pre-LN decoder
    const __half* t2u_ar_embed = nullptr;  // [unit_vocab][M]; the tied output projection
    const float* t2u_ar_pos = nullptr;     // [unit_max_seq_len][M]
    std::vector<DecoderLayer> t2u_ar_dec;
    LNorm t2u_ar_final_ln;
    // vocoder duration predictor (codehifigan.py:46-48); vdp_proj_w == null: not loaded
    Conv vdp_conv1, vdp_conv2;
    LNorm vdp_ln1, vdp_ln2;
    const float* vdp_proj_w = nullptr;
    const float* vdp_proj_b = nullptr;
    const float* dp_proj_w = nullptr;
    const float* dp_proj_b = nullptr;
    std::vector<FFTLayer> t2u_dec;
    LNorm t2u_dec_ln;
    // FiLM-conditioned NAR T2U (film_cond_dim > 0): every projection that reads the conditioning vector stacked into one matrix
    // [t2u_film_n][film_cond_dim] - the decoder layers' FiLM (2 M rows each), the duration predictor's (2 H rows), prosody_proj
    // (M rows) - with s_gamma / s_beta and the + 1 folded into mul / add (launch_pretssel_film)
    const __half* t2u_film_w = nullptr;
    const float* t2u_film_b = nullptr;
    const float* t2u_film_mul = nullptr;
    const float* t2u_film_add = nullptr;
    int t2u_film_n = 0, t2u_film_dp_off = 0, t2u_film_pros_off = 0;
    // NAR char tables (host)
    std::vector<int32_t> tok_len;
    std::vector<uint8_t> starts_space, is_punct;
    std::vector<int64_t> char_offsets;
    std::vector<int32_t> char_ids;
    // vocoder
    const __half* voc_dict = nullptr;
    const __half* voc_lang = nullptr;
    const __half* voc_spkr = nullptr;
    Conv voc_pre, voc_post;
    std::vector<ConvT> voc_ups;
    std::vector<ResBlock> voc_res;
};

struct DecodeSession;
void delete_decode_session(DecodeSession* s);
class Engine;

// State bag of the streaming decoder between sc_mma_begin and the sc_mma_step calls of one policy round.
// Kept ACROSS policy rounds while the geometry fits (max_len unchanged, encoder length within cap_enc): the buffers then
// keep their addresses.
struct MmaState {
    int s_enc = 0, cap = 0, pos = 0;
    int cap_enc = 0;  // rows per layer of `cross` (>= s_enc; rows behind s_enc are never attended: key mask)
    Buf<float> kv, cross, kenergy, work, pchoose;
    Buf<int> ints;
    Buf<__half> planes;  // split planes of the second-generation step (alloc_step2 layout)
};

// One handle: the model description plus its own stream, scratch pool and per-call results.
struct Model : ModelData {
    hipStream_t stream = nullptr;
    hipEvent_t order_event = nullptr;  // sc_wait_stream: orders this handle's stream after a producer stream
    DevicePool pool;
    // Side chains (run_vocode: the length buckets of one call are independent and individually too small to fill the
    // chip, so they run on a few extra streams).  A side chain owns a stream AND a scratch pool - the pool's "a released
    // block may be handed out again at once" rule only holds in stream order - and `pp()` is the pool every stage helper
    // allocates from: the handle's own unless a SideScope has redirected the handle to a side chain.
    struct SideChain {
        hipStream_t stream = nullptr;
        hipEvent_t done = nullptr;
        DevicePool pool;
    };
    std::vector<std::unique_ptr<SideChain>> side;
    hipEvent_t side_fork = nullptr;
    void trim_all_pools();   // every cached block of the handle's pools (own, side chains) back to the driver
    void hook_pool(DevicePool& p) { p.set_oom_hook([this] { trim_all_pools(); }); }
    DevicePool* pool_override = nullptr;
    DevicePool* pp() { return pool_override ? pool_override : &pool; }
    SideChain& side_chain(int k);  // created on first use
    std::vector<void*> owned;  // weight allocations (empty for a forked handle: the parent owns them)

    // results of the last sc_t2u_nar call
    std::vector<int32_t> last_units, last_durations, last_char_ids, last_char_seq_lens;
    int last_n = 0, last_su = 0, last_sc = 0;
    int last_t2u_launches = 0;  // launch calls of the last sc_t2u_nar* call behind the T2U encoder (decoder front end + FFT decoder)
    int64_t last_t2u_enc_rows = 0;      // rows the last run_t2u_encoder call computed: sum of the text lengths (packed) or n * s_text
    std::vector<int32_t> t2u_enc_stage; // host side of the packed encoder's index tables, alive until the caller's synchronisation
    int64_t last_padded_unit_rows = 0;  // unit rows the NAR decoder really computed (length buckets), vs last_n * last_su
    int64_t last_vocoder_unit_rows = 0; // unit frames the vocoder really computed in the last sc_vocode* call
    int last_vocoder_packed_groups = 0; // groups of the packed pass in the last sc_vocode* call; 0: padded batch / length buckets

    std::unique_ptr<MmaState> mma;  // buffers come from `pool`: released before it (see ~Model)

    // fbank constants of sample rates other than the model's 16 kHz, built on first use (sc_fbank_rate; owned by this handle)
    struct FbankRate {
        float* consts = nullptr;
        int frame_len = 0, frame_shift = 0, nfft = 0;
    };
    std::map<int, FbankRate> fbank_rates;


    // buffers + captured step graph of the greedy text generation, kept across calls (model_decoder.hip)
    std::unique_ptr<DecodeSession, void (*)(DecodeSession*)> dec_session{nullptr, delete_decode_session};

    // decode engine attached to this handle (sc_engine_attach; not owned): greedy sc_generate_text calls that fit it hand
    // their rows to the engine's shared step chain; engine_announced = rows announced with sc_engine_expect, not yet submitted
    Engine* engine = nullptr;
    int engine_announced = 0;

    Model() = default;
    Model(const Model&) = delete;
    Model& operator=(const Model&) = delete;
    ~Model();
};

// Redirects a handle's stream and scratch pool to one of its side chains for the lifetime of the scope.
struct SideScope {
    Model& m;
    hipStream_t saved;
    SideScope(Model& mm, int k) : SideScope(mm, mm.side_chain(k)) {}
    SideScope(Model& mm, Model::SideChain& c) : m(mm), saved(mm.stream) {
        m.stream = c.stream;
        m.pool_override = &c.pool;
    }
    ~SideScope() {
        m.stream = saved;
        m.pool_override = nullptr;
    }
    SideScope(const SideScope&) = delete;
    SideScope& operator=(const SideScope&) = delete;
};

// stage implementations (model_*.hip)
struct PackedItems;
void load_model(Model& m, const sc_tensor_desc* t, size_t n);
// The HiFi-GAN stack on packed items from conv_pre's input rows [pk.rows()][in_dim] -> d_out [pk.rows() * hop], conv_post without
// the tanh.  pk.off / pk.n / pk.d_off set by the caller.  plane_split: bit 0 wide stages, bit 2 narrow stages on two fp16 planes
// (0: the unit vocoder's default, hi plane only).  Synchronises the handle's stream.
void run_hifigan_rows(Model& m, const float* d_rows_in, PackedItems& pk, float* d_out, int plane_split);
int64_t hifigan_packed_row_cap(const Model& m, int hop);  // unit rows one packed group may hold; 0: a geometry the packed kernels do not take
// sample_rate: the waveform's own rate (16000 = the model's; others get their own window / shift / FFT size / mel banks)
void run_fbank(Model& m, const float* d_wav, int n, int64_t wav_stride, const int32_t* h_ns, int standardize,
               float* d_out, int t_rows, int32_t* h_frames, int sample_rate = 16000);
// frames of a waveform of num_samples samples at a rate (snip_edges: 0 below one 25 ms window)
int fbank_num_frames(int64_t num_samples, int sample_rate);
int encoder_out_len(const Model& m, int t_frames);
void run_encode_speech(Model& m, const float* d_fbank, int n, int t_frames, const int32_t* h_lens, float* d_out,
                       int32_t* h_out_lens);
// the same on each item's own rows in one packed pass (model_encoder.hip): d_out [n][s_enc_cap][model_dim], zeros behind a length
void run_encode_speech_ragged(Model& m, const float* d_fbank, int n, int t_frames, const int32_t* h_lens, float* d_out, int s_enc_cap,
                              int32_t* h_out_lens);
void run_mma_begin(Model& m, const float* d_enc, int s_enc, int max_len);
void run_mma_step(Model& m, const int32_t* h_tokens, int n_tokens, const int32_t* h_blocked, int n_blocked, int32_t* out_index,
                  float* h_pchoose, float* d_features);
// Streaming session pool (mma_pool.hip): N sessions of the monotonic decoder on one row-group step chain in slot mode.
// The pool lives on m's stream and scratch pool and has to go before m.
struct MmaPool;
MmaPool* mma_pool_create(Model& m, const sc_mma_pool_opts& o);
void mma_pool_free(MmaPool* p);
int mma_pool_device(const MmaPool& p);
void mma_pool_begin(MmaPool& p, const int32_t* h_sessions, int k, const float* d_enc, const int32_t* h_s_enc);
void mma_pool_step(MmaPool& p, const int32_t* h_sessions, int k, const int32_t* h_tokens, int tok_stride, const int32_t* h_n_tokens,
                   const int32_t* h_blocked, int blocked_stride, const int32_t* h_n_blocked, int32_t* h_out_index, float* h_pchoose,
                   float* d_features);
void mma_pool_stats(MmaPool& p, sc_mma_pool_stats* out, bool reset);
int text_to_char_seqs_host(int vocab, const int32_t* tok_len, const uint8_t* starts_space, const uint8_t* is_punct,
                           const int64_t* offs, const int32_t* ids, int pad_idx, int unk_idx, int eos_idx, const int32_t* text_seqs,
                           int n, int s_text, int32_t* out_char_lens, int32_t* out_char_ids, int cap, int32_t* out_seq_lens);
void run_encode_text(Model& m, const int32_t* h_tokens, int n, int s_text, const int32_t* h_lens, float* d_out);
int text_max_len(const Model& m, const sc_gen_opts& o, int s_enc);
int decoder_step_family(const Model& m, int rows, int caller);
void ngram_blocked_tokens(const int32_t* seq, int S, int G, std::vector<int32_t>& out);
// sc_generate_text_capture: where the greedy step's cross-attention capture (k_xattn.hip) goes, per utterance
struct XattnCapture {
    float* d_xattn = nullptr;       // [n][max_len][s_enc] on the device
    float* h_step_lprob = nullptr;  // [n][max_len] on the host
};
// sc_generate_text_banned: the caller's banned token sequences (host CSR; BannedSequenceProcessor), copied to the device once
// per call by run_generate_beam; banned_blocked_tokens is the host restatement of the rule (sc_banned_blocked_tokens)
struct BannedHost {
    const int32_t* tokens = nullptr;
    const int32_t* offsets = nullptr;  // [n + 1]
    int n = 0;
    bool any() const { return n > 0; }  // an empty list is no list
};
void banned_blocked_tokens(const int32_t* seq, int S, const BannedHost& b, std::vector<int32_t>& out);
// sc_generate_text_boosted: the caller's boost phrases (host CSR, any order; PhraseBoostProcessor) and the boost per matched
// token; checked, sorted (boost_list.h) and copied to the device once per call by run_generate_beam
struct BoostHost {
    const int32_t* tokens = nullptr;
    const int32_t* offsets = nullptr;  // [n + 1]
    int n = 0;
    float boost = 0.f;
    bool any() const { return n > 0 && boost != 0.f; }  // no phrase or no boost is no list
};
// Teacher-forced decoder pass over known tokens [n][s_text] as one batched forward into d_hidden [n][s_text][M]
// (model_decoder.hip; sc_decode_text, and the pass behind a beam search, a sampled call, scoring and language identification)
void run_decode_text_batched(Model& m, const float* d_enc, int n, int s_enc, const int32_t* h_enc_lens, const int32_t* h_tokens, int s_text,
                             float* d_hidden, bool row_independent = false, float* d_xattn = nullptr, const int32_t* h_seq_lens = nullptr);
void run_identify_language(Model& m, const float* d_enc, int n, int s_enc, const int32_t* h_enc_lens, const int32_t* h_prefix,
                           int prefix_len, const int32_t* h_cand, int n_cand, float* h_lprob, int32_t* h_best);
void run_score_text(Model& m, const float* d_enc, int n, int s_enc, const int32_t* h_enc_lens, const int32_t* h_tokens,
                    const int32_t* h_tok_lens, int s_text, float* h_tok_lprob, float* h_sum_lprob, int32_t* h_top1, float* d_dec_hidden,
                    float* d_xattn = nullptr);
// d_cond: [n][film_cond_dim] on the device for a FiLM model, null otherwise (a mismatch is an error)
// fit: null runs launch_durations with duration_factor, as ever.  Otherwise the fit kernel (k_dub.hip) takes that one launch's
// place with one factor per item, duration_factor is unused, and everything behind it reads the per-character durations as before.
struct T2uFit {
    const int32_t* h_target;  // [n] unit budget per item, 0: none
    const float* h_lo;        // [n] bounds of the item's factor
    const float* h_hi;
    float* h_factor;          // [n] out
    int32_t* h_flags;         // [n] out, bit 0: over budget at lo
};
void run_t2u_nar(Model& m, const float* d_dec_hidden, int n, int s_text, const int32_t* h_text_lens,
                 const int32_t* h_text_seqs, float duration_factor, int32_t* h_unit_lens, int32_t* out_su,
                 int32_t* out_sc, const float* d_cond = nullptr, const T2uFit* fit = nullptr);
// h_unit_lens == null: the whole padded batch.  Otherwise only the first h_unit_lens[i] * hop samples of row i are
// guaranteed (computed exactly as in the padded batch), the rest of the row is zero.
// Conv1d (stride 1, 'same'-style padding) on pre-split planes through the DMA GEMM (k_gemm_ps.hip, implicit-conv mode):
// xh/xl [nb][t][cin] halfs; C (fp32) and/or Ch/Cl; row_valid: see GemmPsArgs
// row_pos != null: packed items (rows_total rows in all, row_pos[m] = {position, item length}); nb / t are then unused
void conv1d_presplit(Model& m, const __half* xh, const __half* xl, const Conv& c, const float* res, float* C, __half* Ch, __half* Cl,
                     int nb, int t, int pad, int dil, const unsigned char* row_valid, int act, int rows_total = 0,
                     const int2* row_pos = nullptr, float plane_neg_slope = 1.0f, int split = 1);
void run_vocoder_durations(Model& m, const int32_t* h_units, int n, int s_units, int32_t* h_durations);
void run_t2u_ar(Model& m, const float* d_dec_hidden, int n, int s_text, const int32_t* h_text_lens, const sc_gen_opts& o,
                const int32_t* h_prefix, int prefix_len, int32_t* h_out_ids, int32_t* h_out_lens, float* h_scores);
// T2U encoder (pre-LN StandardTransformerEncoder over the text decoder output; shared by the NAR and the AR T2U)
// h_text_lens (nullable): the same lengths on the host; with them the encoder computes the live rows only (model_t2u.hip)
void run_t2u_encoder(Model& m, const float* d_dec_hidden, int n, int s_text, const int* d_text_lens, float* d_out,
                     const int32_t* h_text_lens = nullptr);
// sc_generate_text_nbest: where the ranked finished hypotheses of a beam search go (host memory; h_step nullable)
struct BeamNbestOut {
    int nbest = 0;
    int32_t* h_ids = nullptr;     // [n][nbest][max_len]
    int32_t* h_lens = nullptr;    // [n][nbest]
    float* h_scores = nullptr;    // [n][nbest]
    int32_t* h_counts = nullptr;  // [n]
    float* h_step = nullptr;      // [n][nbest][max_len]
};
// One generation request, as a C entry hands it to the loops.  A plain record: a call site sets the fields it means, the
// others keep their "not given" value.  Filled once per call; the loops read it and never write it.
struct GenRequest {
    // the source: encoder output [n][s_enc][M] on the device, its lengths on the host
    const float* d_enc = nullptr;
    int n = 0, s_enc = 0;
    const int32_t* h_enc_lens = nullptr;
    sc_gen_opts opts{};
    // the prompt: prefix_len tokens are echoed for all rows.  prefix_stride 0: every row is fed h_prefix[0 .. prefix_len);
    // otherwise row b is fed h_prefix[b * prefix_stride + ...] (sc_generate_text_rows).  h_prefix_lens (nullable, with
    // prefix_stride > 0; sc_generate_text_prompts): row b's prompt is h_prefix_lens[b] tokens long and prefix_len is the
    // SHORTEST of them - the rows whose prompt is longer are fed the rest of it while the other rows already generate
    const int32_t* h_prefix = nullptr;
    int prefix_len = 0, prefix_stride = 0;
    const int32_t* h_prefix_lens = nullptr;
    // step processors of the host-driven loops (an empty list is no list: BannedHost::any, BoostHost::any)
    BannedHost banned;
    BoostHost boost;
    const XattnCapture* xcap = nullptr;  // greedy generation only (sc_generate_text_capture)
    // the outputs: ids [n][max_len], lens [n], scores [n] (nullable) on the host, decoder outputs [n][max_len - 1][M] on the
    // device (nullable).  Sampled generation writes num_gens hypotheses per utterance into the first three
    int32_t* h_out_ids = nullptr;
    int32_t* h_out_lens = nullptr;
    float* h_scores = nullptr;
    float* d_dec_hidden = nullptr;
    // beam search (nullable; sc_generate_text_nbest): every finished hypothesis leaves instead of the best one, and
    // h_out_ids / h_out_lens / h_scores are not written
    const BeamNbestOut* nbest = nullptr;
};
// The checks of a sc_generate_text* call and its route: the host-driven beam loop (beam_size > 1 or a step processor), the
// decode engine, or greedy generation on the handle's own chain (run_generate_text)
void route_generate_text(Model& m, const GenRequest& q);
// beam search over one decoder stack (the UnitY text decoder or the v1 autoregressive unit decoder)
void run_generate_beam(Model& m, const DecStack& W, const GenRequest& q, int max_len);
// sampled generation (model_sample.hip): outputs [n][num_gens][...], hypotheses of an utterance sorted by score
void run_generate_sampled(Model& m, const GenRequest& q, const sc_sample_opts& so, const uint64_t* h_streams, float* h_step_lprob);
void run_vocode(Model& m, const int32_t* h_units, int n, int s_units, const int32_t* h_lang, const int32_t* h_spkr,
                float* d_wav, const int32_t* h_unit_lens = nullptr);
std::vector<std::vector<int>> plan_length_groups(const std::vector<int>& lens, int overhead_rows, int max_groups);

// helpers shared by the stages
void linear(Model& m, const float* x, int64_t ldx, const Linear& L, const float* res, int64_t ldr, float* y,
            int64_t ldy, int rows, int act, float alpha, bool row_independent = false);
// encoder-decoder K / V of `rows` encoder rows for one decoder layer ([rows][2M]): ALWAYS the tiled product, so that an
// utterance's K / V - and with them its hypothesis - do not depend on how many utterances share the call (alone, in a batch,
// through the decode engine)
inline void project_cross_kv(Model& m, const float* d_enc, const Linear& L, float* out, int rows) {
    linear(m, d_enc, L.in, L, nullptr, 0, out, L.out, rows, ACT_NONE, 1.f, /*row_independent=*/true);
}
void layernorm(Model& m, const float* x, const LNorm& L, float* y, int rows, int act = ACT_NONE,
               const int* lens = nullptr, int t_per_batch = 1);

// ---- products, attention and whole layers shared by the stage passes (layers.hip) ----
struct Planes {  // an operand of the pre-split products: two fp16 planes [rows][dim]
    __half* hi = nullptr;
    __half* lo = nullptr;
};
// The rows of a batch, padded or packed.  Padded: item i holds rows [i * S, (i + 1) * S), rows = n * S.  Packed (d_off set):
// item i holds rows [d_off[i], d_off[i] + d_lens[i]) with nothing in between, rows = their sum, S = the longest item.
struct BatchRows {
    int n = 0, S = 0, rows = 0;
    const int* d_lens = nullptr;  // live rows (= keys) per item; nullable for a padded batch
    const int* d_off = nullptr;   // null: padded
    double pairs = 0;             // packed, profiler only: sum of len^2
};
// C (fp32) and/or out (split planes) = alpha * act(A . W^T + b) + res over `rows` rows of the planes `a`
// split 0: the hi plane only (SC_SPLIT_MODE=1, the padded speech encoder's precision study)
void linear_ps(Model& m, Planes a, const Linear& L, int rows, int act, float alpha, const float* res, float* C, Planes out = {}, int split = 1);
// Self-attention over a [rows][3M] q | k | v buffer.  The result goes to `out` (fp32 [rows][M]) or to the planes `out_p`.
struct SelfAttn {
    int heads = 0, head_dim = 64;
    float* out = nullptr;
    Planes out_p;
    int causal = 0;
    const float* rel_k = nullptr;  // Shaw relative keys, with rel_left / rel_right
    int rel_left = 0, rel_right = 0;
    const float* rp_table = nullptr;  // v1 relative positions [2S - 1][M], with the u / v query biases
    const float* q_bias_u = nullptr;
    const float* q_bias_v = nullptr;
};
void self_attention(Model& m, const float* qkv, int M, const BatchRows& b, const SelfAttn& o);

// One Conformer layer of the speech encoder on pre-split planes, x [rows][M] in place; padded and packed batches alike, which
// is why an item carries the same bits through run_encode_speech and run_encode_speech_ragged.
struct ConformerPass {
    float* x = nullptr;     // residual stream
    float* wide = nullptr;  // [rows][3M]
    float* att = nullptr;   // [rows][M]; only with fuse_conv off
    Planes hs, as, ws;      // [rows][M], [rows][M], [rows][enc_ffn_dim]
    bool fuse_conv = true;  // GLU + depthwise conv + LayerNorm + SiLU in one kernel
    bool fuse_ln = true;    // the closing LayerNorm together with the next layer's first one
    bool glu_epi = true;    // GLU in the first pointwise product's epilogue (needs fuse_conv)
    int split = 1;          // linear_ps
    const int* d_work = nullptr;  // packed: work table of the convolution module (glu_dwconv_ln_packed_work)
    int n_work = 0;
};
// next: the layer behind l (null: l is the last).  ffn1_ready: the previous layer's closing launch already wrote LN_ffn1(x) into
// p.hs; returns the same for the next layer.
bool conformer_layer(Model& m, const ConformerLayer& l, const ConformerLayer* next, const BatchRows& b, const ConformerPass& p, bool ffn1_ready);
// The adaptor layer behind its two strided convolutions (y: the attention branch, res: the residual branch, both [rows][M]):
// y = FFN(attention(y) + res) without the final LayerNorm.  aw [rows][max(3M, adaptor_ffn_dim)] and ah [rows][M] are scratch.
void adaptor_layer_tail(Model& m, const AdaptorLayer& a, const BatchRows& b, const float* res, float* y, float* aw, float* ah, bool row_independent);
// One pre-LN transformer encoder layer on the fp32-operand products, x [rows][M] in place; h, att [rows][M] and
// wide [rows][max(3M, ffn)] are scratch.
void encoder_layer(Model& m, const EncoderLayer& l, const BatchRows& b, int heads, int head_dim, int ffn_act, bool row_independent, float* x,
                   float* h, float* wide, float* att);
// One post-LN FFT layer (NAR T2U decoder, PRETSSEL) on packed rows: u (fp32) and up (planes) hold the input and receive the
// output.  film != null: FiLM behind the second LayerNorm from row film_off.. of the table, item of a row in row_item.
struct FFTPass {
    float* u = nullptr;
    float* y = nullptr;
    float* wide = nullptr;  // [rows][3M]
    Planes up, yp, ap, wp;  // [rows][M] x 3, [rows][conv inner dim]
    const int2* d_row_pos = nullptr;  // {position, item length} of every row
    int heads = 0, head_dim = 64;
    const float* film = nullptr;
    int film_ld = 0;
    const int* row_item = nullptr;
};
int fft_layer_packed(Model& m, const FFTLayer& l, int film_off, const BatchRows& b, const FFTPass& p);  // returns the launches made
// Packed items of a ragged batch (the vocoder's packed pass): item i holds the unit rows [off[i], off[i + 1]) of every
// buffer, items back to back with no rows in between; at a stage that runs `mul` rows per unit row, the rows
// [off[i] * mul, off[i + 1] * mul).  Kernels take the device copy of `off` (GemmArgs::item_off and its kin).
struct PackedItems {
    std::vector<int> off;        // [n + 1], off[0] = 0
    const int* d_off = nullptr;  // the same on the device
    int n = 0;
    // tile tables of the fused narrow-stage kernels (packed_tile_first), [n + 1] each, behind one another: table 4 * stage + j
    // for the pair kernel at ResBlock j's kernel size (j < 3), 4 * stage + 3 for the multi-receptive-field kernel
    std::vector<int> tabs;
    const int* d_tabs = nullptr;
    const int* d_tab(int idx) const { return d_tabs + (size_t)idx * (n + 1); }
    int tab_total(int idx) const { return tabs[(size_t)idx * (n + 1) + n]; }
    int rows() const { return off.empty() ? 0 : off.back(); }
    int longest() const {
        int l = 0;
        for (int i = 0; i < n; ++i) l = std::max(l, off[i + 1] - off[i]);
        return l;
    }
};
// Host-side planning of the packed vocoder pass (plain C++; sc_op_voc_pack_plan tests it without a device): items in their
// given order, cut into consecutive groups of at most `budget_rows` unit rows each (an item longer than the budget is a
// group of its own).  Returns the first item of every group, and the number of items behind them.
std::vector<int> plan_packed_groups(const std::vector<int>& need, int64_t budget_rows);
// first workgroup of every item ([n + 1]) when item i takes ceil(len_i * mul / tile_rows) tiles counted from its first row
std::vector<int> packed_tile_first(const std::vector<int>& off, int mul, int tile_rows);

// pk != null (stride 1, 'same' padding, no d_in_lens): packed items at `mul` rows per unit row; nb / t_in are unused
void conv1d(Model& m, const float* x, const Conv& c, const float* res, float* y, int nb, int t_in, int stride, int pad,
            int dil, const int* d_in_lens, int in_act, int act, const PackedItems* pk = nullptr, int mul = 1);
void conv_transpose1d(Model& m, const float* x, const ConvT& c, float* y, int nb, int t_in, int in_act, const PackedItems* pk = nullptr,
                      int mul = 1);

// 2-layer LSTM with the `y + x` skip (the waveform generator's StreamableLSTM): fp16 weights, gate order i, f, g, o
struct Lstm2 {
    const __half* wih0 = nullptr;  // [4H][H]
    const __half* whh0 = nullptr;  // [4H][H]
    const __half* w1 = nullptr;    // [4H][2H] = [W_ih1 | W_hh1]
    const float* b_ih0 = nullptr;
    const float* b_hh0 = nullptr;
    const float* b_ih1 = nullptr;
    const float* b_hh1 = nullptr;
    int H = 0;
};
// packed items (d_off [n + 1]): xproj [rows][4H], h0 / h1 [rows][H], c [2][n][H] are scratch; returns the launches made
int run_lstm2(const Lstm2& w, const float* x, const int* d_off, int n, int rows, int longest, float* xproj, float* h0, float* h1, float* c, float* y,
              float* max_pre, hipStream_t s);

}  // namespace sc
