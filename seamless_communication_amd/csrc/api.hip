// extern "C" surface of libseamless_hip.so (declared in include/seamless_hip.h).
#include <cstring>
#include <map>
#include <mutex>
#include <set>

#include "dstep.h"
#include "engine.h"
#include "handle.h"

using namespace sc;

struct sc_model {
    Model m;
    sc_config& cfg = m.cfg;  // where open_handle puts the entry's config
};

struct sc_engine {
    std::unique_ptr<Engine> e;
    int device = 0;
    const void* weights = nullptr;  // identity of the model the engine was built on (the text embedding's address)
    std::set<sc_model*> attached;   // handles routed through this engine (guarded by g_attach_mu)
};

// Engine <-> handle lifetimes are enforced HERE, not by the caller: freeing an engine detaches every handle still attached
// to it (their next greedy call runs on the handle's own chain), freeing a handle takes its announced rows back and leaves
// the engine's list.  One process-wide mutex: attach / free are rare.
static std::mutex g_attach_mu;
static std::map<Engine*, sc_engine*> g_engine_owner;

static void detach_locked(sc_model* m) {
    Engine* e = m->m.engine;
    if (!e) return;
    e->expect(m->m, -m->m.engine_announced);
    auto it = g_engine_owner.find(e);
    if (it != g_engine_owner.end()) it->second->attached.erase(m);
    m->m.engine = nullptr;
    m->m.engine_announced = 0;
}
// inside a free entry, which reports nothing: no error of the library (what SC_API_END catches) leaves it
static void detach_quietly_locked(sc_model* m) {
    try {
        detach_locked(m);
    } catch (const sc::Error&) {
    } catch (const std::exception&) {
    }
}

namespace {

// The caller's lists as the records a GenRequest holds, refused under the entry's name `who` when a count is negative or a
// pointer is missing.  An empty list is no list (BannedHost::any, BoostHost::any) - nothing else converts one.  What the lists
// hold is checked by validate_banned_host / check_boost_host, where each entry always made those checks.
BannedHost banned_arg(const char* who, const int32_t* tokens, const int32_t* offsets, int32_t n) {
    SC_CHECK(n >= 0 && (n == 0 || (tokens && offsets)), "%s: bad banned list", who);
    BannedHost b;
    b.tokens = tokens, b.offsets = offsets, b.n = n;
    return b;
}
BoostHost boost_arg(const char* who, const int32_t* tokens, const int32_t* offsets, int32_t n, float boost) {
    SC_CHECK(n >= 0 && (n == 0 || (tokens && offsets)), "%s: bad phrase list", who);
    BoostHost p;
    p.tokens = tokens, p.offsets = offsets, p.n = n, p.boost = boost;
    return p;
}

// The argument checks of sc_generate_text_prompts (shared with sc_generate_text_nbest), on the host before any device work,
// and what they found: the shortest and the longest prompt, the two lists
struct PromptsCall {
    int shortest = 0, longest = 0;
    BannedHost banned;
    BoostHost boost;
};
PromptsCall check_prompts_call(const char* who, sc_model* m, int32_t n, int32_t s_enc, const sc_gen_opts* opts, const int32_t* h_prompt_rows,
                               int32_t prompt_stride, const int32_t* h_prompt_lens, const int32_t* h_banned_tokens,
                               const int32_t* h_banned_offsets, int32_t n_banned, const int32_t* h_boost_tokens, const int32_t* h_boost_offsets,
                               int32_t n_boost, float boost) {
    SC_CHECK(n > 0 && prompt_stride >= 1, "%s: n=%d prompt_stride=%d", who, n, prompt_stride);
    PromptsCall call;
    call.banned = banned_arg(who, h_banned_tokens, h_banned_offsets, n_banned);
    call.boost = boost_arg(who, h_boost_tokens, h_boost_offsets, n_boost, boost);
    const DecStack W = unity_stack(m->m);
    const int max_len = text_max_len(m->m, *opts, s_enc);
    call.shortest = prompt_stride;
    for (int b = 0; b < n; ++b) {
        const int len = h_prompt_lens[b];
        SC_CHECK(len >= 1 && len <= prompt_stride, "%s: row %d: prompt length %d outside 1..%d", who, b, len, prompt_stride);
        SC_CHECK(len < max_len, "%s: row %d: prompt length %d >= effective max length %d", who, b, len, max_len);
        const int32_t* p = h_prompt_rows + (size_t)b * prompt_stride;
        for (int t = 0; t < len; ++t) {
            SC_CHECK(p[t] >= 0 && p[t] < W.vocab, "%s: row %d: prompt token %d outside the vocabulary", who, b, p[t]);
            SC_CHECK(t == 0 || (p[t] != W.pad_idx && p[t] != W.eos_idx), "%s: row %d: pad / EOS (%d) at prompt position %d", who, b,
                     p[t], t);
        }
        call.shortest = std::min(call.shortest, len), call.longest = std::max(call.longest, len);
    }
    validate_banned_host(call.banned.tokens, call.banned.offsets, call.banned.n, W.vocab, nullptr);
    if (n_boost > 0) check_boost_host(call.boost, W.vocab, W.pad_idx, W.eos_idx);
    return call;
}
}  // namespace

extern "C" {

const char* sc_last_error(void) { return sc::get_error(); }
int sc_abi_version(void) { return SC_ABI_VERSION; }

// sc_load / sc_load_ext; ext == null: the ReLU, unconditioned model of sc_load
static sc_model* load_handle(const sc_tensor_desc* tensors, size_t n_tensors, const sc_config* cfg, const sc_load_ext_opts* ext, int device) {
    return open_handle<sc_model>("sc_load", tensors, n_tensors, cfg, device, [ext](sc_model& h, const sc_tensor_desc* t, size_t n) {
        if (ext && (ext->abi_version != 0 || ext->ffn_activation != 0 || ext->t2u_ffn_activation != 0 || ext->film_cond_dim != 0)) {
            SC_CHECK(ext->abi_version == SC_ABI_VERSION, "sc_load_ext: extension ABI version %d != library %d", ext->abi_version, SC_ABI_VERSION);
            SC_CHECK((ext->ffn_activation == SC_FFN_RELU || ext->ffn_activation == SC_FFN_GELU) &&
                         (ext->t2u_ffn_activation == SC_FFN_RELU || ext->t2u_ffn_activation == SC_FFN_GELU),
                     "sc_load_ext: unknown FFN activation (%d, %d)", ext->ffn_activation, ext->t2u_ffn_activation);
            SC_CHECK(ext->film_cond_dim >= 0, "sc_load_ext: film_cond_dim=%d", ext->film_cond_dim);
            h.m.ffn_act = ext->ffn_activation == SC_FFN_GELU ? ACT_GELU : ACT_RELU;
            h.m.t2u_ffn_act = ext->t2u_ffn_activation == SC_FFN_GELU ? ACT_GELU : ACT_RELU;
            h.m.film_cond_dim = ext->film_cond_dim;
        }
        load_model(h.m, t, n);
    });
}

sc_model* sc_load(const sc_tensor_desc* tensors, size_t n_tensors, const sc_config* cfg, int device) {
    return load_handle(tensors, n_tensors, cfg, nullptr, device);
}

sc_model* sc_load_ext(const sc_tensor_desc* tensors, size_t n_tensors, const sc_config* cfg, const sc_load_ext_opts* ext, int device) {
    return load_handle(tensors, n_tensors, cfg, ext, device);
}

sc_model* sc_fork(sc_model* parent) {
    sc_model* h = nullptr;
    try {
        SC_CHECK(parent, "sc_fork: null handle");
        SC_HIP(hipSetDevice(parent->m.device));
        h = new sc_model();
        static_cast<ModelData&>(h->m) = static_cast<const ModelData&>(parent->m);
        open_stream(h->m);
        return h;
    } catch (const sc::Error&) {
    } catch (const std::exception& e) {
        sc::set_error("sc_fork: unexpected C++ exception: %s", e.what());
    }
    delete h;
    return nullptr;
}

void sc_free(sc_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->m.device);
    {
        std::lock_guard<std::mutex> lk(g_attach_mu);
        detach_quietly_locked(m);  // announced rows that will never come would make the engine pause below its low-water mark
    }
    delete m;
}

int sc_synchronize(sc_model* m) {
    SC_API_BEGIN
    SC_CHECK(m, "null handle");
    SC_HIP(hipSetDevice(m->m.device));
    SC_HIP(hipStreamSynchronize(m->m.stream));
    SC_API_END
}

int sc_decoder_step_family(sc_model* m, int rows, int caller) {
    if (!m || rows < 1 || caller < 0 || caller > 3) return SC_ERR_INVALID;
    try {
        return decoder_step_family(m->m, rows, caller);
    } catch (const sc::Error&) {
    } catch (const std::exception&) {
    }
    return SC_ERR_INTERNAL;
}

int sc_wait_stream(sc_model* m, void* producer_stream) {
    SC_API_BEGIN
    SC_CHECK(m, "null handle");
    SC_HIP(hipSetDevice(m->m.device));
    hipStream_t prod = static_cast<hipStream_t>(producer_stream);
    if (prod == m->m.stream) return SC_OK;
    if (!m->m.order_event) SC_HIP(hipEventCreateWithFlags(&m->m.order_event, hipEventDisableTiming));
    SC_HIP(hipEventRecord(m->m.order_event, prod));
    SC_HIP(hipStreamWaitEvent(m->m.stream, m->m.order_event, 0));
    SC_API_END
}

int sc_set_nar_tables(sc_model* m, int32_t vocab, const int32_t* tok_len, const uint8_t* starts_space,
                      const uint8_t* is_punct, const int64_t* offs, const int32_t* ids) {
    SC_API_BEGIN
    SC_CHECK(m && tok_len && starts_space && is_punct && offs && ids, "sc_set_nar_tables: null argument");
    SC_CHECK(vocab == m->m.cfg.text_vocab_size, "sc_set_nar_tables: table has %d entries, text vocabulary has %d", vocab,
             m->m.cfg.text_vocab_size);
    Model& mm = m->m;
    mm.tok_len.assign(tok_len, tok_len + vocab);
    mm.starts_space.assign(starts_space, starts_space + vocab);
    mm.is_punct.assign(is_punct, is_punct + vocab);
    mm.char_offsets.assign(offs, offs + vocab + 1);
    mm.char_ids.assign(ids, ids + offs[vocab]);
    for (int64_t i = 0; i < offs[vocab]; ++i)
        SC_CHECK(ids[i] >= 0 && ids[i] < mm.cfg.char_vocab_size, "sc_set_nar_tables: char id %d out of range", ids[i]);
    SC_API_END
}

int sc_fbank(sc_model* m, const float* d_wav, int32_t n, int64_t wav_stride, const int32_t* h_num_samples,
             int32_t standardize, float* d_out, int32_t t_rows, int32_t* h_out_frames) {
    SC_API_BEGIN
    // a batch without a single frame has a 0-row output, whose pointer may well be null: name the cause
    SC_CHECK(n > 0 && t_rows > 0, "sc_fbank: empty batch");
    SC_CHECK(m && d_wav && h_num_samples && d_out, "sc_fbank: null argument");
    SC_HIP(hipSetDevice(m->m.device));
    run_fbank(m->m, d_wav, n, wav_stride, h_num_samples, standardize, d_out, t_rows, h_out_frames);
    SC_API_END
}

int32_t sc_encoder_out_len(const sc_model* m, int32_t t_frames) { return m ? encoder_out_len(m->m, t_frames) : -1; }

int sc_fbank_rate(sc_model* m, const float* d_wav, int32_t n, int64_t wav_stride, const int32_t* h_num_samples, int32_t sample_rate,
                  int32_t standardize, float* d_out, int32_t t_rows, int32_t* h_out_frames) {
    SC_API_BEGIN
    SC_CHECK(n > 0 && t_rows > 0, "sc_fbank: empty batch");
    SC_CHECK(m && d_wav && h_num_samples && d_out, "sc_fbank_rate: null argument");
    SC_HIP(hipSetDevice(m->m.device));
    run_fbank(m->m, d_wav, n, wav_stride, h_num_samples, standardize, d_out, t_rows, h_out_frames, sample_rate);
    SC_API_END
}

int32_t sc_fbank_frames(int64_t num_samples, int32_t sample_rate) { return sample_rate > 0 ? fbank_num_frames(num_samples, sample_rate) : 0; }

int sc_encode_speech(sc_model* m, const float* d_fbank, int32_t n, int32_t t_frames, const int32_t* h_frame_lens,
                     float* d_enc_out, int32_t* h_out_lens) {
    SC_API_BEGIN
    SC_CHECK(m && d_fbank && h_frame_lens && d_enc_out, "sc_encode_speech: null argument");
    SC_HIP(hipSetDevice(m->m.device));
    run_encode_speech(m->m, d_fbank, n, t_frames, h_frame_lens, d_enc_out, h_out_lens);
    SC_API_END
}

int sc_encode_speech_ragged(sc_model* m, const float* d_fbank, int32_t n, int32_t t_frames, const int32_t* h_frame_lens, float* d_enc_out,
                            int32_t s_enc_cap, int32_t* h_out_lens) {
    SC_API_BEGIN
    SC_CHECK(m && d_fbank && h_frame_lens && d_enc_out, "sc_encode_speech_ragged: null argument");
    SC_HIP(hipSetDevice(m->m.device));
    run_encode_speech_ragged(m->m, d_fbank, n, t_frames, h_frame_lens, d_enc_out, s_enc_cap, h_out_lens);
    SC_API_END
}

int sc_encode_text(sc_model* m, const int32_t* h_tokens, int32_t n, int32_t s_text, const int32_t* h_lens, float* d_enc_out) {
    SC_API_BEGIN
    SC_CHECK(m && h_tokens && h_lens && d_enc_out, "sc_encode_text: null argument");
    SC_HIP(hipSetDevice(m->m.device));
    run_encode_text(m->m, h_tokens, n, s_text, h_lens, d_enc_out);
    SC_API_END
}

int sc_mma_begin(sc_model* m, const float* d_enc, int32_t s_enc, int32_t max_len) {
    SC_API_BEGIN
    SC_CHECK(m && d_enc, "sc_mma_begin: null argument");
    SC_HIP(hipSetDevice(m->m.device));
    run_mma_begin(m->m, d_enc, s_enc, max_len);
    SC_API_END
}

int sc_mma_step(sc_model* m, const int32_t* h_tokens, int32_t n_tokens, const int32_t* h_blocked, int32_t n_blocked,
                int32_t* out_index, float* h_pchoose, float* d_features) {
    SC_API_BEGIN
    SC_CHECK(m && h_tokens && out_index && h_pchoose && d_features && (h_blocked || n_blocked == 0), "sc_mma_step: null argument");
    SC_HIP(hipSetDevice(m->m.device));
    run_mma_step(m->m, h_tokens, n_tokens, h_blocked, n_blocked, out_index, h_pchoose, d_features);
    SC_API_END
}

sc_mma_pool* sc_mma_pool_create(sc_model* m, const sc_mma_pool_opts* opts) {
    try {
        SC_CHECK(m && opts, "sc_mma_pool_create: null argument");
        SC_CHECK(opts->abi_version == SC_ABI_VERSION, "sc_mma_pool_create: options ABI version %d != library %d", opts->abi_version,
                 SC_ABI_VERSION);
        SC_HIP(hipSetDevice(m->m.device));
        return reinterpret_cast<sc_mma_pool*>(mma_pool_create(m->m, *opts));
    } catch (const sc::Error&) {
    } catch (const std::exception& e) {
        sc::set_error("sc_mma_pool_create: unexpected C++ exception: %s", e.what());
    }
    return nullptr;
}

void sc_mma_pool_free(sc_mma_pool* p) {
    if (!p) return;
    MmaPool* q = reinterpret_cast<MmaPool*>(p);
    (void)hipSetDevice(mma_pool_device(*q));
    mma_pool_free(q);
}

int sc_mma_pool_begin(sc_mma_pool* p, const int32_t* h_sessions, int32_t k, const float* d_enc, const int32_t* h_s_enc) {
    SC_API_BEGIN
    SC_CHECK(p && h_sessions && d_enc && h_s_enc, "sc_mma_pool_begin: null argument");
    MmaPool& q = *reinterpret_cast<MmaPool*>(p);
    SC_HIP(hipSetDevice(mma_pool_device(q)));
    mma_pool_begin(q, h_sessions, k, d_enc, h_s_enc);
    SC_API_END
}

int sc_mma_pool_step(sc_mma_pool* p, const int32_t* h_sessions, int32_t k, const int32_t* h_tokens, int32_t tok_stride,
                     const int32_t* h_n_tokens, const int32_t* h_blocked, int32_t blocked_stride, const int32_t* h_n_blocked,
                     int32_t* h_out_index, float* h_pchoose, float* d_features) {
    SC_API_BEGIN
    SC_CHECK(p && h_sessions && h_tokens && h_n_tokens && h_out_index && h_pchoose && d_features && (!h_blocked || h_n_blocked),
             "sc_mma_pool_step: null argument");
    MmaPool& q = *reinterpret_cast<MmaPool*>(p);
    SC_HIP(hipSetDevice(mma_pool_device(q)));
    mma_pool_step(q, h_sessions, k, h_tokens, tok_stride, h_n_tokens, h_blocked, blocked_stride, h_n_blocked, h_out_index, h_pchoose,
                  d_features);
    SC_API_END
}

int sc_mma_pool_get_stats(sc_mma_pool* p, sc_mma_pool_stats* out, int32_t reset) {
    SC_API_BEGIN
    SC_CHECK(p && out, "sc_mma_pool_get_stats: null argument");
    mma_pool_stats(*reinterpret_cast<MmaPool*>(p), out, reset != 0);
    SC_API_END
}

int32_t sc_text_max_len(const sc_model* m, const sc_gen_opts* opts, int32_t s_enc) {
    return (m && opts) ? text_max_len(m->m, *opts, s_enc) : -1;
}

int sc_generate_text(sc_model* m, const float* d_enc, int32_t n, int32_t s_enc, const int32_t* h_enc_lens,
                     const sc_gen_opts* opts, const int32_t* h_prefix, int32_t prefix_len, int32_t* h_out_ids,
                     int32_t* h_out_lens, float* h_out_scores, float* d_dec_hidden) {
    SC_API_BEGIN
    SC_CHECK(m && d_enc && h_enc_lens && opts && h_prefix && h_out_ids && h_out_lens, "sc_generate_text: null argument");
    SC_HIP(hipSetDevice(m->m.device));
    GenRequest q;
    q.d_enc = d_enc, q.n = n, q.s_enc = s_enc, q.h_enc_lens = h_enc_lens, q.opts = *opts;
    q.h_prefix = h_prefix, q.prefix_len = prefix_len;
    q.h_out_ids = h_out_ids, q.h_out_lens = h_out_lens, q.h_scores = h_out_scores, q.d_dec_hidden = d_dec_hidden;
    route_generate_text(m->m, q);
    SC_API_END
}

int sc_generate_text_banned(sc_model* m, const float* d_enc, int32_t n, int32_t s_enc, const int32_t* h_enc_lens,
                            const sc_gen_opts* opts, const int32_t* h_prefix, int32_t prefix_len, int32_t* h_out_ids,
                            int32_t* h_out_lens, float* h_out_scores, float* d_dec_hidden, const int32_t* h_banned_tokens,
                            const int32_t* h_banned_offsets, int32_t n_banned) {
    SC_API_BEGIN
    SC_CHECK(m && d_enc && h_enc_lens && opts && h_prefix && h_out_ids && h_out_lens, "sc_generate_text_banned: null argument");
    GenRequest q;
    q.banned = banned_arg("sc_generate_text_banned", h_banned_tokens, h_banned_offsets, n_banned);
    validate_banned_host(q.banned.tokens, q.banned.offsets, q.banned.n, m->m.cfg.text_vocab_size, nullptr);  // refused before any device work
    SC_HIP(hipSetDevice(m->m.device));
    q.d_enc = d_enc, q.n = n, q.s_enc = s_enc, q.h_enc_lens = h_enc_lens, q.opts = *opts;
    q.h_prefix = h_prefix, q.prefix_len = prefix_len;
    q.h_out_ids = h_out_ids, q.h_out_lens = h_out_lens, q.h_scores = h_out_scores, q.d_dec_hidden = d_dec_hidden;
    route_generate_text(m->m, q);
    SC_API_END
}

int sc_generate_text_boosted(sc_model* m, const float* d_enc, int32_t n, int32_t s_enc, const int32_t* h_enc_lens,
                             const sc_gen_opts* opts, const int32_t* h_prefix, int32_t prefix_len, int32_t* h_out_ids,
                             int32_t* h_out_lens, float* h_out_scores, float* d_dec_hidden, const int32_t* h_banned_tokens,
                             const int32_t* h_banned_offsets, int32_t n_banned, const int32_t* h_boost_tokens,
                             const int32_t* h_boost_offsets, int32_t n_boost, float boost) {
    SC_API_BEGIN
    SC_CHECK(m && d_enc && h_enc_lens && opts && h_prefix && h_out_ids && h_out_lens, "sc_generate_text_boosted: null argument");
    GenRequest q;
    q.banned = banned_arg("sc_generate_text_boosted", h_banned_tokens, h_banned_offsets, n_banned);
    q.boost = boost_arg("sc_generate_text_boosted", h_boost_tokens, h_boost_offsets, n_boost, boost);
    // refused before any device work (the call itself checks and sorts the list again where it copies it)
    const DecStack W = unity_stack(m->m);
    validate_banned_host(q.banned.tokens, q.banned.offsets, q.banned.n, W.vocab, nullptr);
    check_boost_host(q.boost, W.vocab, W.pad_idx, W.eos_idx);
    SC_HIP(hipSetDevice(m->m.device));
    q.d_enc = d_enc, q.n = n, q.s_enc = s_enc, q.h_enc_lens = h_enc_lens, q.opts = *opts;
    q.h_prefix = h_prefix, q.prefix_len = prefix_len;
    q.h_out_ids = h_out_ids, q.h_out_lens = h_out_lens, q.h_scores = h_out_scores, q.d_dec_hidden = d_dec_hidden;
    route_generate_text(m->m, q);
    SC_API_END
}

int sc_generate_text_sampled(sc_model* m, const float* d_enc, int32_t n, int32_t s_enc, const int32_t* h_enc_lens,
                             const sc_gen_opts* opts, const sc_sample_opts* sample_opts, const uint64_t* h_streams, const int32_t* h_prefix,
                             int32_t prefix_len, int32_t* h_out_ids, int32_t* h_out_lens, float* h_out_scores, float* h_step_lprob,
                             float* d_dec_hidden, const int32_t* h_banned_tokens, const int32_t* h_banned_offsets, int32_t n_banned) {
    SC_API_BEGIN
    SC_CHECK(m && d_enc && h_enc_lens && opts && sample_opts && h_prefix && h_out_ids && h_out_lens, "sc_generate_text_sampled: null argument");
    SC_CHECK(sample_opts->abi_version == SC_ABI_VERSION, "sc_generate_text_sampled: options ABI version %d != library %d",
             sample_opts->abi_version, SC_ABI_VERSION);
    GenRequest q;
    q.banned = banned_arg("sc_generate_text_sampled", h_banned_tokens, h_banned_offsets, n_banned);  // (its content: upload_banned)
    SC_HIP(hipSetDevice(m->m.device));
    q.d_enc = d_enc, q.n = n, q.s_enc = s_enc, q.h_enc_lens = h_enc_lens, q.opts = *opts;
    q.h_prefix = h_prefix, q.prefix_len = prefix_len;
    q.h_out_ids = h_out_ids, q.h_out_lens = h_out_lens, q.h_scores = h_out_scores, q.d_dec_hidden = d_dec_hidden;
    run_generate_sampled(m->m, q, *sample_opts, h_streams, h_step_lprob);
    SC_API_END
}

int sc_generate_text_capture(sc_model* m, const float* d_enc, int32_t n, int32_t s_enc, const int32_t* h_enc_lens,
                             const sc_gen_opts* opts, const int32_t* h_prefix, int32_t prefix_len, int32_t* h_out_ids,
                             int32_t* h_out_lens, float* h_out_scores, float* d_dec_hidden, float* d_xattn, float* h_step_lprob) {
    SC_API_BEGIN
    SC_CHECK(m && d_enc && h_enc_lens && opts && h_prefix && h_out_ids && h_out_lens && d_xattn && h_step_lprob,
             "sc_generate_text_capture: null argument");
    SC_HIP(hipSetDevice(m->m.device));
    XattnCapture xc;
    xc.d_xattn = d_xattn;
    xc.h_step_lprob = h_step_lprob;
    GenRequest q;
    q.d_enc = d_enc, q.n = n, q.s_enc = s_enc, q.h_enc_lens = h_enc_lens, q.opts = *opts;
    q.h_prefix = h_prefix, q.prefix_len = prefix_len;
    q.xcap = &xc;
    q.h_out_ids = h_out_ids, q.h_out_lens = h_out_lens, q.h_scores = h_out_scores, q.d_dec_hidden = d_dec_hidden;
    route_generate_text(m->m, q);
    SC_API_END
}

sc_engine* sc_engine_create(sc_model* m, const sc_engine_opts* opts) {
    sc_engine* h = nullptr;
    try {
        SC_CHECK(m && opts, "sc_engine_create: null argument");
        SC_HIP(hipSetDevice(m->m.device));
        h = new sc_engine();
        h->device = m->m.device;
        h->weights = m->m.text_embed;
        h->e.reset(new Engine(m->m, *opts));
        {
            std::lock_guard<std::mutex> lk(g_attach_mu);
            g_engine_owner[h->e.get()] = h;
        }
        return h;
    } catch (const sc::Error&) {
    } catch (const std::exception& e) {
        sc::set_error("sc_engine_create: unexpected C++ exception: %s", e.what());
    }
    delete h;
    return nullptr;
}

void sc_engine_free(sc_engine* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    {
        std::lock_guard<std::mutex> lk(g_attach_mu);
        for (sc_model* m : std::set<sc_model*>(e->attached)) {  // no handle keeps a pointer to the engine about to go
            detach_quietly_locked(m);
        }
        g_engine_owner.erase(e->e.get());
    }
    delete e;
}

int sc_engine_attach(sc_model* m, sc_engine* e) {
    SC_API_BEGIN
    SC_CHECK(m, "sc_engine_attach: null handle");
    if (e) SC_CHECK(e->e && e->device == m->m.device && e->weights == m->m.text_embed,
                    "sc_engine_attach: the engine was built on another model or device");
    std::lock_guard<std::mutex> lk(g_attach_mu);
    detach_locked(m);
    if (e) {
        m->m.engine = e->e.get();
        e->attached.insert(m);
    }
    SC_API_END
}

int sc_engine_expect(sc_model* m, int32_t n_rows) {
    SC_API_BEGIN
    SC_CHECK(m, "sc_engine_expect: null handle");
    if (m->m.engine && n_rows != 0) m->m.engine->expect(m->m, n_rows);
    SC_API_END
}

int sc_engine_get_stats(sc_engine* e, sc_engine_stats* out, int32_t reset) {
    SC_API_BEGIN
    SC_CHECK(e && e->e && out, "sc_engine_get_stats: null argument");
    e->e->stats(out, reset != 0);
    SC_API_END
}

int sc_decode_text(sc_model* m, const float* d_enc, int32_t n, int32_t s_enc, const int32_t* h_enc_lens,
                   const int32_t* h_tokens, int32_t s_text, float* d_dec_hidden) {
    SC_API_BEGIN
    SC_CHECK(m && d_enc && h_enc_lens && h_tokens && d_dec_hidden && s_text > 0, "sc_decode_text: bad argument");
    SC_HIP(hipSetDevice(m->m.device));
    SC_CHECK(n > 0 && s_enc > 0, "sc_generate_text: empty batch");  // (the text callers have always read for this refusal)
    run_decode_text_batched(m->m, d_enc, n, s_enc, h_enc_lens, h_tokens, s_text, d_dec_hidden);
    SC_API_END
}

int sc_score_text(sc_model* m, const float* d_enc, int32_t n, int32_t s_enc, const int32_t* h_enc_lens, const int32_t* h_tokens,
                  const int32_t* h_tok_lens, int32_t s_text, float* h_tok_lprob, float* h_sum_lprob, int32_t* h_top1,
                  float* d_dec_hidden) {
    SC_API_BEGIN
    SC_CHECK(m && d_enc && h_enc_lens && h_tokens && h_tok_lens && h_tok_lprob, "sc_score_text: null argument");
    SC_HIP(hipSetDevice(m->m.device));
    run_score_text(m->m, d_enc, n, s_enc, h_enc_lens, h_tokens, h_tok_lens, s_text, h_tok_lprob, h_sum_lprob, h_top1, d_dec_hidden);
    SC_API_END
}

int sc_score_text_capture(sc_model* m, const float* d_enc, int32_t n, int32_t s_enc, const int32_t* h_enc_lens, const int32_t* h_tokens,
                          const int32_t* h_tok_lens, int32_t s_text, float* h_tok_lprob, float* h_sum_lprob, int32_t* h_top1,
                          float* d_dec_hidden, float* d_xattn) {
    SC_API_BEGIN
    SC_CHECK(m && d_enc && h_enc_lens && h_tokens && h_tok_lens && h_tok_lprob, "sc_score_text_capture: null argument");
    SC_CHECK(d_xattn, "sc_score_text_capture: null d_xattn (sc_score_text is the call without the attention rows)");
    SC_HIP(hipSetDevice(m->m.device));
    run_score_text(m->m, d_enc, n, s_enc, h_enc_lens, h_tokens, h_tok_lens, s_text, h_tok_lprob, h_sum_lprob, h_top1, d_dec_hidden, d_xattn);
    SC_API_END
}


int sc_identify_language(sc_model* m, const float* d_enc, int32_t n, int32_t s_enc, const int32_t* h_enc_lens, const int32_t* h_prefix,
                         int32_t prefix_len, const int32_t* h_cand, int32_t n_cand, float* h_lprob, int32_t* h_best) {
    SC_API_BEGIN
    // (the count first: an empty list may well come with a null pointer, and the caller should read which of the two it was)
    SC_CHECK(n_cand >= 1 && n_cand <= SCORE_MAX_CAND, "sc_identify_language: n_cand=%d outside 1..%d", n_cand, SCORE_MAX_CAND);
    SC_CHECK(m && d_enc && h_enc_lens && h_prefix && h_cand && h_lprob && h_best, "sc_identify_language: null argument");
    SC_HIP(hipSetDevice(m->m.device));
    run_identify_language(m->m, d_enc, n, s_enc, h_enc_lens, h_prefix, prefix_len, h_cand, n_cand, h_lprob, h_best);
    SC_API_END
}

int sc_generate_text_rows(sc_model* m, const float* d_enc, int32_t n, int32_t s_enc, const int32_t* h_enc_lens,
                          const sc_gen_opts* opts, const int32_t* h_prefix_rows, int32_t prefix_len, int32_t* h_out_ids,
                          int32_t* h_out_lens, float* h_out_scores, float* d_dec_hidden) {
    SC_API_BEGIN
    SC_CHECK(m && d_enc && h_enc_lens && opts && h_prefix_rows && h_out_ids && h_out_lens, "sc_generate_text_rows: null argument");
    SC_CHECK(n > 0 && prefix_len >= 1, "sc_generate_text_rows: n=%d prefix_len=%d", n, prefix_len);
    for (int64_t i = 0; i < (int64_t)n * prefix_len; ++i)
        SC_CHECK(h_prefix_rows[i] >= 0 && h_prefix_rows[i] < m->m.cfg.text_vocab_size,
                 "sc_generate_text_rows: prompt token %d (row %d) outside the vocabulary", h_prefix_rows[i], (int)(i / prefix_len));
    SC_HIP(hipSetDevice(m->m.device));
    GenRequest q;
    q.d_enc = d_enc, q.n = n, q.s_enc = s_enc, q.h_enc_lens = h_enc_lens, q.opts = *opts;
    q.h_prefix = h_prefix_rows, q.prefix_len = prefix_len, q.prefix_stride = prefix_len;
    q.h_out_ids = h_out_ids, q.h_out_lens = h_out_lens, q.h_scores = h_out_scores, q.d_dec_hidden = d_dec_hidden;
    route_generate_text(m->m, q);
    SC_API_END
}

int sc_generate_text_prompts(sc_model* m, const float* d_enc, int32_t n, int32_t s_enc, const int32_t* h_enc_lens,
                             const sc_gen_opts* opts, const int32_t* h_prompt_rows, int32_t prompt_stride, const int32_t* h_prompt_lens,
                             int32_t* h_out_ids, int32_t* h_out_lens, float* h_out_scores, float* d_dec_hidden,
                             const int32_t* h_banned_tokens, const int32_t* h_banned_offsets, int32_t n_banned,
                             const int32_t* h_boost_tokens, const int32_t* h_boost_offsets, int32_t n_boost, float boost) {
    SC_API_BEGIN
    SC_CHECK(m && d_enc && h_enc_lens && opts && h_prompt_rows && h_prompt_lens && h_out_ids && h_out_lens,
             "sc_generate_text_prompts: null argument");
    const PromptsCall call = check_prompts_call("sc_generate_text_prompts", m, n, s_enc, opts, h_prompt_rows, prompt_stride, h_prompt_lens,
                                                h_banned_tokens, h_banned_offsets, n_banned, h_boost_tokens, h_boost_offsets, n_boost, boost);
    SC_HIP(hipSetDevice(m->m.device));
    GenRequest q;
    q.d_enc = d_enc, q.n = n, q.s_enc = s_enc, q.h_enc_lens = h_enc_lens, q.opts = *opts;
    // equal lengths: sc_generate_text_rows with the lists; otherwise the shortest prompt is echoed for all rows and the per-row
    // lengths go down with the call
    q.h_prefix = h_prompt_rows, q.prefix_len = call.shortest, q.prefix_stride = prompt_stride;
    q.h_prefix_lens = call.shortest == call.longest ? nullptr : h_prompt_lens;
    q.banned = call.banned, q.boost = call.boost;
    q.h_out_ids = h_out_ids, q.h_out_lens = h_out_lens, q.h_scores = h_out_scores, q.d_dec_hidden = d_dec_hidden;
    route_generate_text(m->m, q);
    SC_API_END
}

int sc_generate_text_nbest(sc_model* m, const float* d_enc, int32_t n, int32_t s_enc, const int32_t* h_enc_lens, const sc_gen_opts* opts,
                           const int32_t* h_prompt_rows, int32_t prompt_stride, const int32_t* h_prompt_lens, int32_t nbest,
                           int32_t* h_out_ids, int32_t* h_out_lens, float* h_out_scores, int32_t* h_out_counts, float* h_step_scores,
                           const int32_t* h_banned_tokens, const int32_t* h_banned_offsets, int32_t n_banned,
                           const int32_t* h_boost_tokens, const int32_t* h_boost_offsets, int32_t n_boost, float boost) {
    SC_API_BEGIN
    SC_CHECK(m && d_enc && h_enc_lens && opts && h_prompt_rows && h_prompt_lens && h_out_ids && h_out_lens && h_out_scores && h_out_counts,
             "sc_generate_text_nbest: null argument");
    SC_CHECK(opts->beam_size >= 1 && opts->beam_size <= 8, "sc_generate_text_nbest: beam_size %d outside 1..8", opts->beam_size);
    SC_CHECK(nbest >= 1 && nbest <= opts->beam_size, "sc_generate_text_nbest: nbest %d outside 1..beam_size (%d)", nbest, opts->beam_size);
    SC_CHECK(opts->no_repeat_ngram_size >= 0, "sc_generate_text_nbest: no_repeat_ngram_size=%d", opts->no_repeat_ngram_size);
    const PromptsCall call = check_prompts_call("sc_generate_text_nbest", m, n, s_enc, opts, h_prompt_rows, prompt_stride, h_prompt_lens,
                                                h_banned_tokens, h_banned_offsets, n_banned, h_boost_tokens, h_boost_offsets, n_boost, boost);
    SC_CHECK(s_enc > 0, "sc_generate_text_nbest: empty batch");
    const DecStack W = unity_stack(m->m);
    const int max_len = text_max_len(m->m, *opts, s_enc);
    check_generation_limits("sc_generate_text_nbest", *opts, call.shortest, max_len, W.max_seq_len, n, s_enc, h_enc_lens);
    BeamNbestOut out;
    out.nbest = nbest, out.h_ids = h_out_ids, out.h_lens = h_out_lens, out.h_scores = h_out_scores, out.h_counts = h_out_counts;
    out.h_step = h_step_scores;
    SC_HIP(hipSetDevice(m->m.device));
    GenRequest q;
    q.d_enc = d_enc, q.n = n, q.s_enc = s_enc, q.h_enc_lens = h_enc_lens, q.opts = *opts;
    q.h_prefix = h_prompt_rows, q.prefix_len = call.shortest, q.prefix_stride = prompt_stride;  // prompts as sc_generate_text_prompts
    q.h_prefix_lens = call.shortest == call.longest ? nullptr : h_prompt_lens;
    q.banned = call.banned, q.boost = call.boost;
    q.nbest = &out;
    // always the host-driven beam loop (route_generate_text's beam route, whatever the beam size)
    prof::set_tag("dec");
    if (m->m.engine) m->m.engine->expect(m->m, -n);
    run_generate_beam(m->m, W, q, max_len);
    SC_API_END
}

int sc_t2u_nar(sc_model* m, const float* d_dec_hidden, int32_t n, int32_t s_text, const int32_t* h_text_lens,
               const int32_t* h_text_seqs, float duration_factor, int32_t* h_unit_lens, int32_t* out_s_unit_max,
               int32_t* out_s_char_max) {
    SC_API_BEGIN
    SC_CHECK(m && d_dec_hidden && h_text_lens && h_text_seqs, "sc_t2u_nar: null argument");
    SC_HIP(hipSetDevice(m->m.device));
    run_t2u_nar(m->m, d_dec_hidden, n, s_text, h_text_lens, h_text_seqs, duration_factor, h_unit_lens, out_s_unit_max,
                out_s_char_max);
    SC_API_END
}

int sc_t2u_nar_cond(sc_model* m, const float* d_dec_hidden, int32_t n, int32_t s_text, const int32_t* h_text_lens,
                    const int32_t* h_text_seqs, float duration_factor, const float* d_cond, int32_t* h_unit_lens, int32_t* out_s_unit_max,
                    int32_t* out_s_char_max) {
    SC_API_BEGIN
    SC_CHECK(m && d_dec_hidden && h_text_lens && h_text_seqs && d_cond, "sc_t2u_nar_cond: null argument");
    SC_HIP(hipSetDevice(m->m.device));
    run_t2u_nar(m->m, d_dec_hidden, n, s_text, h_text_lens, h_text_seqs, duration_factor, h_unit_lens, out_s_unit_max, out_s_char_max,
                d_cond);
    SC_API_END
}

int sc_t2u_nar_fit(sc_model* m, const float* d_dec_hidden, int32_t n, int32_t s_text, const int32_t* h_text_lens, const int32_t* h_text_seqs,
                   const int32_t* h_target_units, const float* h_lo, const float* h_hi, const float* d_cond, int32_t* h_unit_lens,
                   int32_t* out_s_unit_max, int32_t* out_s_char_max, float* h_factor, int32_t* h_flags) {
    SC_API_BEGIN
    // every argument check comes before the first device call
    SC_CHECK(m && d_dec_hidden && h_text_lens && h_text_seqs && h_target_units && h_lo && h_hi && h_factor && h_flags,
             "sc_t2u_nar_fit: null argument");
    SC_CHECK(n > 0, "sc_t2u_nar_fit: empty batch");
    check_fit_items("sc_t2u_nar_fit", n, h_target_units, h_lo, h_hi);
    SC_CHECK(m->m.film_cond_dim <= 0 || d_cond, "sc_t2u_nar_fit: this T2U is FiLM-conditioned (film_cond_dim=%d): d_cond is required",
             m->m.film_cond_dim);
    SC_CHECK(m->m.film_cond_dim > 0 || !d_cond, "sc_t2u_nar_fit: the model was loaded without FiLM conditioning, d_cond must be null");
    SC_HIP(hipSetDevice(m->m.device));
    const T2uFit fit{h_target_units, h_lo, h_hi, h_factor, h_flags};
    run_t2u_nar(m->m, d_dec_hidden, n, s_text, h_text_lens, h_text_seqs, 1.0f, h_unit_lens, out_s_unit_max, out_s_char_max, d_cond, &fit);
    SC_API_END
}

int32_t sc_op_t2u_last_launches(sc_model* m) { return m ? m->m.last_t2u_launches : -1; }

int sc_op_t2u_encoder(sc_model* m, const float* d_dec_hidden, int32_t n, int32_t s_text, const int32_t* h_text_lens, float* d_out,
                      int64_t* out_rows) {
    SC_API_BEGIN
    SC_CHECK(m && d_dec_hidden && h_text_lens && d_out, "sc_op_t2u_encoder: null argument");
    SC_CHECK(m->m.cfg.has_t2u, "sc_op_t2u_encoder: the model was loaded without a T2U sub-model");
    SC_CHECK(n > 0 && s_text > 0, "sc_op_t2u_encoder: empty batch");
    SC_HIP(hipSetDevice(m->m.device));
    prof::set_tag("t2u");
    Buf<int> d_tlens(m->m.pp(), n);
    SC_HIP(hipMemcpyAsync(d_tlens.get(), h_text_lens, (size_t)n * 4, hipMemcpyHostToDevice, m->m.stream));
    run_t2u_encoder(m->m, d_dec_hidden, n, s_text, d_tlens, d_out, h_text_lens);
    SC_HIP(hipStreamSynchronize(m->m.stream));
    if (out_rows) *out_rows = m->m.last_t2u_enc_rows;
    SC_API_END
}

int sc_get_units(sc_model* m, int32_t* h_units) {
    SC_API_BEGIN
    SC_CHECK(m && h_units, "sc_get_units: null argument");
    SC_CHECK(!m->m.last_units.empty(), "sc_get_units: no sc_t2u_nar result is available");
    std::memcpy(h_units, m->m.last_units.data(), m->m.last_units.size() * 4);
    SC_API_END
}

int sc_get_durations(sc_model* m, int32_t* h_durations, int32_t* h_char_ids, int32_t* h_char_seq_lens) {
    SC_API_BEGIN
    SC_CHECK(m, "sc_get_durations: null handle");
    SC_CHECK(!m->m.last_durations.empty(), "sc_get_durations: no sc_t2u_nar result is available");
    if (h_durations) std::memcpy(h_durations, m->m.last_durations.data(), m->m.last_durations.size() * 4);
    if (h_char_ids) std::memcpy(h_char_ids, m->m.last_char_ids.data(), m->m.last_char_ids.size() * 4);
    if (h_char_seq_lens) std::memcpy(h_char_seq_lens, m->m.last_char_seq_lens.data(), m->m.last_char_seq_lens.size() * 4);
    SC_API_END
}

int32_t sc_vocoder_hop(const sc_model* m) {
    if (!m) return -1;
    int hop = 1;
    for (int i = 0; i < m->m.cfg.voc_num_upsamples; ++i) hop *= m->m.cfg.voc_upsample_rates[i];
    return hop;
}

int sc_vocode(sc_model* m, const int32_t* h_units, int32_t n, int32_t s_units, const int32_t* h_lang_idx,
              const int32_t* h_spkr_idx, float* d_wav) {
    SC_API_BEGIN
    SC_CHECK(m && h_units && h_lang_idx && h_spkr_idx && d_wav, "sc_vocode: null argument");
    SC_HIP(hipSetDevice(m->m.device));
    run_vocode(m->m, h_units, n, s_units, h_lang_idx, h_spkr_idx, d_wav);
    SC_API_END
}

static int t2u_ar_len(const sc::Model& M, const sc_gen_opts& o, int s_text) {
    const int src = o.source_len > 0 ? o.source_len : s_text;
    int max_len = o.soft_max_seq_len_a > 0 ? std::min(o.hard_max_seq_len, (int)(o.soft_max_seq_len_a * (float)src) + o.soft_max_seq_len_b)
                                           : o.hard_max_seq_len;
    return std::min(max_len, M.cfg.unit_max_seq_len);
}

int32_t sc_t2u_ar_max_len(sc_model* m, const sc_gen_opts* opts, int32_t s_text) {
    if (!m || !opts) return -1;
    return t2u_ar_len(m->m, *opts, s_text);
}

int sc_t2u_ar(sc_model* m, const float* d_dec_hidden, int32_t n, int32_t s_text, const int32_t* h_text_lens, const sc_gen_opts* opts,
              const int32_t* h_prefix, int32_t prefix_len, int32_t* h_out_ids, int32_t unit_cap, int32_t* h_out_lens, float* h_scores) {
    SC_API_BEGIN
    SC_CHECK(m && d_dec_hidden && h_text_lens && opts && h_prefix && h_out_ids && h_out_lens, "sc_t2u_ar: null argument");
    SC_HIP(hipSetDevice(m->m.device));
    SC_CHECK(opts->beam_size >= 1 && opts->beam_size <= 8, "sc_t2u_ar: beam_size %d out of range (1..8)", opts->beam_size);
    const int max_len = t2u_ar_len(m->m, *opts, s_text);
    SC_CHECK(unit_cap >= max_len, "sc_t2u_ar: unit_cap %d < effective maximum length %d (sc_t2u_ar_max_len)", unit_cap, max_len);
    std::vector<int32_t> ids((size_t)n * max_len);
    run_t2u_ar(m->m, d_dec_hidden, n, s_text, h_text_lens, *opts, h_prefix, prefix_len, ids.data(), h_out_lens, h_scores);
    for (int b = 0; b < n; ++b)
        for (int t = 0; t < unit_cap; ++t) h_out_ids[(size_t)b * unit_cap + t] = t < max_len ? ids[(size_t)b * max_len + t] : m->m.cfg.unit_pad_idx;
    SC_API_END
}

int sc_vocoder_durations(sc_model* m, const int32_t* h_units, int32_t n, int32_t s_units, int32_t* h_durations) {
    SC_API_BEGIN
    SC_CHECK(m && h_units && h_durations, "sc_vocoder_durations: null argument");
    SC_HIP(hipSetDevice(m->m.device));
    run_vocoder_durations(m->m, h_units, n, s_units, h_durations);
    SC_API_END
}

int sc_vocode_ragged(sc_model* m, const int32_t* h_units, int32_t n, int32_t s_units, const int32_t* h_unit_lens,
                     const int32_t* h_lang_idx, const int32_t* h_spkr_idx, float* d_wav) {
    SC_API_BEGIN
    SC_CHECK(m && h_units && h_unit_lens && h_lang_idx && h_spkr_idx && d_wav, "sc_vocode_ragged: null argument");
    SC_HIP(hipSetDevice(m->m.device));
    run_vocode(m->m, h_units, n, s_units, h_lang_idx, h_spkr_idx, d_wav, h_unit_lens);
    SC_API_END
}

int sc_s2st(sc_model* m, const float* d_fbank, int32_t n, int32_t t_frames, const int32_t* h_frame_lens, const sc_gen_opts* opts,
            const int32_t* h_prefix, int32_t prefix_len, float duration_factor, const int32_t* h_lang_idx, const int32_t* h_spkr_idx,
            int32_t* h_text_ids, int32_t text_cap, int32_t* h_text_lens, int32_t* h_units, int32_t unit_cap, int32_t* h_unit_lens,
            float* d_wav, int32_t* out_s_unit_max) {
    SC_API_BEGIN
    SC_CHECK(m && d_fbank && h_frame_lens && opts && h_prefix && h_lang_idx && h_spkr_idx && h_text_ids && h_text_lens && h_units &&
                 h_unit_lens && d_wav,
             "sc_s2st: null argument");
    Model& M = m->m;
    SC_CHECK(M.film_cond_dim == 0, "sc_s2st: this T2U is FiLM-conditioned and the fused chain takes no conditioning vectors; run the stages "
             "(sc_encode_speech, sc_generate_text, sc_t2u_nar_cond)");
    SC_HIP(hipSetDevice(M.device));
    const int D = M.cfg.model_dim;
    // speech encoder
    const int s_enc = encoder_out_len(M, t_frames);
    Buf<float> enc(&M.pool, (size_t)n * s_enc * D);
    std::vector<int32_t> enc_lens(n);
    run_encode_speech(M, d_fbank, n, t_frames, h_frame_lens, enc, enc_lens.data());
    // text generation (the soft length rule refers to the fbank frames unless the caller says otherwise)
    sc_gen_opts o = *opts;
    if (o.source_len <= 0) o.source_len = t_frames;
    const int max_len = text_max_len(M, o, s_enc);
    SC_CHECK(text_cap >= max_len, "sc_s2st: text_cap %d < effective maximum text length %d (sc_text_max_len)", text_cap, max_len);
    std::vector<int32_t> ids((size_t)n * max_len), lens(n);
    Buf<float> hidden(&M.pool, (size_t)n * (max_len - 1) * D);
    GenRequest q;
    q.d_enc = enc, q.n = n, q.s_enc = s_enc, q.h_enc_lens = enc_lens.data(), q.opts = o;
    q.h_prefix = h_prefix, q.prefix_len = prefix_len;
    q.h_out_ids = ids.data(), q.h_out_lens = lens.data(), q.d_dec_hidden = hidden;
    route_generate_text(M, q);
    // generator.py:281-291: the last column is trimmed, every length shrinks by one
    std::vector<int32_t> text_seqs((size_t)n * (max_len - 1)), text_lens(n);
    for (int b = 0; b < n; ++b) {
        std::copy(ids.begin() + (size_t)b * max_len, ids.begin() + (size_t)b * max_len + max_len - 1, text_seqs.begin() + (size_t)b * (max_len - 1));
        text_lens[b] = lens[b] - 1;
        for (int t = 0; t < text_cap; ++t) h_text_ids[(size_t)b * text_cap + t] = t < max_len ? ids[(size_t)b * max_len + t] : M.cfg.pad_idx;
        h_text_lens[b] = lens[b];
    }
    // NAR text-to-unit
    int32_t su = 0, sc_ = 0;
    run_t2u_nar(M, hidden, n, max_len - 1, text_lens.data(), text_seqs.data(), duration_factor, h_unit_lens, &su, &sc_);
    SC_CHECK(su <= unit_cap, "sc_s2st: %d units exceed unit_cap %d", su, unit_cap);
    for (int b = 0; b < n; ++b)
        for (int t = 0; t < unit_cap; ++t) h_units[(size_t)b * unit_cap + t] = t < su ? M.last_units[(size_t)b * su + t] : M.cfg.unit_pad_idx;
    // vocoder on the padded unit matrix, only what the proportional trim keeps is synthesised; rows land at the caller's stride
    int hop = 1;
    for (int i = 0; i < M.cfg.voc_num_upsamples; ++i) hop *= M.cfg.voc_upsample_rates[i];
    Buf<float> wav(&M.pool, (size_t)n * su * hop);
    run_vocode(M, M.last_units.data(), n, su, h_lang_idx, h_spkr_idx, wav, h_unit_lens);
    SC_HIP(hipMemsetAsync(d_wav, 0, (size_t)n * unit_cap * hop * sizeof(float), M.stream));
    SC_HIP(hipMemcpy2DAsync(d_wav, (size_t)unit_cap * hop * sizeof(float), wav.get(), (size_t)su * hop * sizeof(float),
                            (size_t)su * hop * sizeof(float), n, hipMemcpyDeviceToDevice, M.stream));
    SC_HIP(hipStreamSynchronize(M.stream));
    if (out_s_unit_max) *out_s_unit_max = su;
    SC_API_END
}

int sc_last_padding(sc_model* m, int64_t* t2u_rows_computed, int64_t* t2u_rows_padded, int64_t* vocoder_rows_computed) {
    SC_API_BEGIN
    SC_CHECK(m, "sc_last_padding: null handle");
    if (t2u_rows_computed) *t2u_rows_computed = m->m.last_padded_unit_rows;
    if (t2u_rows_padded) *t2u_rows_padded = (int64_t)m->m.last_n * m->m.last_su;
    if (vocoder_rows_computed) *vocoder_rows_computed = m->m.last_vocoder_unit_rows;
    SC_API_END
}

int sc_prof_enable(int on) {
    sc::prof::enable(on != 0);
    return SC_OK;
}
int sc_prof_reset(void) {
    sc::prof::reset();
    return SC_OK;
}
int64_t sc_prof_report(char* buf, int64_t cap) { return (int64_t)sc::prof::report(buf, (size_t)(cap > 0 ? cap : 0)); }

int32_t sc_text_to_char_seqs(int32_t vocab, const int32_t* h_tok_len, const uint8_t* h_starts_space, const uint8_t* h_is_punct,
                             const int64_t* h_char_offsets, const int32_t* h_char_ids, int32_t pad_idx, int32_t unk_idx,
                             int32_t eos_idx, const int32_t* h_text_seqs, int32_t n, int32_t s_text, int32_t* h_char_lens,
                             int32_t* h_out_char_ids, int32_t cap, int32_t* h_char_seq_lens) {
    try {
        SC_CHECK(h_tok_len && h_starts_space && h_is_punct && h_char_offsets && h_char_ids && h_text_seqs && h_char_lens &&
                     h_out_char_ids && h_char_seq_lens && cap >= 0,
                 "sc_text_to_char_seqs: null argument");
        return text_to_char_seqs_host(vocab, h_tok_len, h_starts_space, h_is_punct, h_char_offsets, h_char_ids, pad_idx, unk_idx,
                                      eos_idx, h_text_seqs, n, s_text, h_char_lens, h_out_char_ids, cap, h_char_seq_lens);
    } catch (const sc::Error& e) {
        return e.code;
    } catch (const std::exception& e) {
        sc::set_error("unexpected C++ exception: %s", e.what());
        return SC_ERR_INTERNAL;
    }
}

int32_t sc_ngram_blocked_tokens(const int32_t* h_seq, int32_t len, int32_t ngram_size, int32_t* h_out, int32_t cap) {
    try {
        SC_CHECK(len >= 0 && ngram_size >= 1 && cap >= 0 && (h_seq || len == 0) && (h_out || cap == 0),
                 "sc_ngram_blocked_tokens: bad argument");
        std::vector<int32_t> out;
        sc::ngram_blocked_tokens(h_seq, len, ngram_size, out);
        for (size_t i = 0; i < out.size() && i < (size_t)cap; ++i) h_out[i] = out[i];
        return (int32_t)out.size();
    } catch (const sc::Error& e) {
        return e.code;
    } catch (const std::exception& e) {
        sc::set_error("unexpected C++ exception: %s", e.what());
        return SC_ERR_INTERNAL;
    }
}

int32_t sc_banned_blocked_tokens(const int32_t* h_seq, int32_t len, const int32_t* h_banned_tokens, const int32_t* h_banned_offsets,
                                 int32_t n_banned, int32_t* h_out, int32_t cap) {
    try {
        SC_CHECK(len >= 0 && cap >= 0 && (h_seq || len == 0) && (h_out || cap == 0), "sc_banned_blocked_tokens: bad argument");
        sc::validate_banned_host(h_banned_tokens, h_banned_offsets, n_banned, -1, nullptr);
        sc::BannedHost b;
        b.tokens = h_banned_tokens, b.offsets = h_banned_offsets, b.n = n_banned;
        std::vector<int32_t> out;
        sc::banned_blocked_tokens(h_seq, len, b, out);
        for (size_t i = 0; i < out.size() && i < (size_t)cap; ++i) h_out[i] = out[i];
        return (int32_t)out.size();
    } catch (const sc::Error& e) {
        return e.code;
    } catch (const std::exception& e) {
        sc::set_error("unexpected C++ exception: %s", e.what());
        return SC_ERR_INTERNAL;
    }
}

int32_t sc_boost_deltas(const int32_t* h_seq, int32_t len, const int32_t* h_boost_tokens, const int32_t* h_boost_offsets, int32_t n_boost,
                        int32_t* h_out_tokens, int32_t* h_out_k, int32_t cap, int32_t* out_dp) {
    try {
        SC_CHECK(len >= 0 && cap >= 0 && (h_seq || len == 0) && ((h_out_tokens && h_out_k) || cap == 0), "sc_boost_deltas: bad argument");
        sc::BoostSorted sorted;
        const std::string why = sc::boost_list_build(h_boost_tokens, h_boost_offsets, n_boost, -1, -1, -1, sorted);
        SC_CHECK(why.empty(), "%s", why.c_str());
        std::vector<int32_t> toks, depth;
        int dp = 0;
        sc::boost_deltas(h_seq, len, sorted, toks, depth, &dp);
        for (size_t i = 0; i < toks.size() && i < (size_t)cap; ++i) h_out_tokens[i] = toks[i], h_out_k[i] = depth[i];
        if (out_dp) *out_dp = dp;
        return (int32_t)toks.size();
    } catch (const sc::Error& e) {
        return e.code;
    } catch (const std::exception& e) {
        sc::set_error("unexpected C++ exception: %s", e.what());
        return SC_ERR_INTERNAL;
    }
}

int32_t sc_op_last_vocoder_packed_groups(sc_model* m) { return m ? m->m.last_vocoder_packed_groups : -1; }

}  // extern "C"
