/*
 * seamless_hip.h — C ABI of libseamless_hip.so, the MI355X (gfx950) native
 * implementation of the SeamlessM4T-v2 speech-to-speech hot path.
 *
 * This is the drop-in boundary for the arithmetic that the reference reaches
 * through fairseq2/PyTorch operators from
 *   src/seamless_communication/inference/translator.py:216-428 (Translator.predict)
 *   src/seamless_communication/inference/generator.py:228-364  (UnitYGenerator.__call__)
 * and is shaped after the reference's own native boundary
 *   ggml/examples/unity/lib/unity_lib.h:45-61, ggml/examples/unity/fairseq2.h:86-334
 * but C-clean: plain pointers and sizes, no C++ types, no exceptions across the
 * boundary.  Every function returns 0 on success or a negative sc_status; the
 * message of the last failure on the calling thread is sc_last_error().
 *
 * Pointer conventions
 *   d_*   device pointers (HBM of the model's GPU), fp32 unless stated
 *   h_*   host pointers (small integer arrays: lengths, token ids)
 * A handle owns one HIP stream; it is not thread-safe; handles on different
 * GPUs are independent (one process per GPU in the data-parallel driver).
 */
#ifndef SEAMLESS_HIP_H_
#define SEAMLESS_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SC_ABI_VERSION 10
#define SC_MAX_UPSAMPLES 8
#define SC_MAX_RESBLOCK_KERNELS 4
#define SC_MAX_RESBLOCK_DILATIONS 4

typedef enum sc_status {
    SC_OK = 0,
    SC_ERR_INVALID = -1,  /* bad argument / missing tensor / shape mismatch */
    SC_ERR_HIP = -2,      /* a HIP runtime call failed                      */
    SC_ERR_CAPACITY = -3, /* caller buffer too small                        */
    SC_ERR_INTERNAL = -4
} sc_status;

typedef enum sc_dtype { SC_F16 = 0, SC_F32 = 1, SC_I32 = 2 } sc_dtype;

/* One entry of the weight table handed to sc_load(): tensors carry the
 * fairseq2 state-dict key names produced by the reference's
 * convert_unity_checkpoint / convert_vocoder_checkpoint
 * (models/unity/loader.py:27-155, models/vocoder/loader.py:20-36). */
typedef struct sc_tensor_desc {
    const char* name;
    int32_t dtype; /* sc_dtype */
    int32_t ndim;
    int64_t shape[4];
    const void* data; /* host pointer, or device pointer when on_device != 0 */
    int32_t on_device;
} sc_tensor_desc;

/* Architecture description (reference: unity `base_v2` builder.py:165-192,
 * conformer_shaw 600m builder.py:54-68, t2u `base_nar` t2u_builder.py:186-232,
 * vocoder `base` vocoder/builder.py:42-64). */
typedef struct sc_config {
    int32_t abi_version;
    int32_t model_dim, num_heads;
    int32_t num_fbank_channels, fbank_stride;
    int32_t enc_layers, enc_ffn_dim, depthwise_conv_kernel_size, shaw_max_left, shaw_max_right;
    int32_t adaptor_kernel_size, adaptor_stride, adaptor_ffn_dim, adaptor_proj_dim;
    int32_t dec_layers, dec_ffn_dim, text_vocab_size, text_max_seq_len;
    int32_t pad_idx, unk_idx, bos_idx, eos_idx;
    int32_t t2u_enc_layers, t2u_dec_layers, t2u_ffn_dim, t2u_conv_kernel, t2u_conv_inner_dim;
    int32_t unit_vocab_size, unit_pad_idx, unit_eos_idx, unit_max_seq_len;
    int32_t char_vocab_size, char_max_seq_len, var_pred_hidden_dim, var_pred_kernel_size;
    /* vocoder */
    int32_t voc_num_upsamples;
    int32_t voc_upsample_rates[SC_MAX_UPSAMPLES];
    int32_t voc_upsample_kernel_sizes[SC_MAX_UPSAMPLES];
    int32_t voc_upsample_initial_channel;
    int32_t voc_num_resblock_kernels;
    int32_t voc_resblock_kernel_sizes[SC_MAX_RESBLOCK_KERNELS];
    int32_t voc_num_resblock_dilations;
    int32_t voc_resblock_dilation_sizes[SC_MAX_RESBLOCK_KERNELS][SC_MAX_RESBLOCK_DILATIONS];
    int32_t voc_num_embeddings, voc_embedding_dim, voc_lang_embedding_dim, voc_num_langs;
    int32_t voc_spkr_embedding_dim, voc_num_spkrs;
    int32_t has_t2u, has_vocoder;
    /* NLLB text encoder of the text-input tasks (T2TT / T2ST; builder.py:169-173, :430-434): 0 layers = not loaded */
    int32_t text_enc_layers, text_enc_ffn_dim;
    /* streaming monotonic text decoder (models/monotonic_decoder/builder.py:81-99 `dense_1b`): 0 layers = not loaded.
     * Its tensors carry the fairseq2 names of convert_monotonic_checkpoint under the prefix "monotonic_decoder.". */
    int32_t mma_layers, mma_ffn_dim, mma_energy_layers, mma_pre_decision_ratio;
    float mma_temperature;
    /* speech encoder family (ABI v5).  0: Conformer-Shaw of seamlessM4T_v2_large (Shaw relative keys, causal depthwise
     * convolution + LayerNorm; models/conformer_shaw/builder.py:127-156).  1: w2v-BERT of the v1 models seamlessM4T_medium /
     * seamlessM4T_large (models/unity/builder.py:109-162): Transformer-XL relative positions (tensors
     * `...self_attn.sdpa.{r_proj.weight,u_bias,v_bias}`) and a centred depthwise convolution + BatchNorm1d
     * (`...conv.batch_norm.{weight,bias,running_mean,running_var}`); restated in ggml/examples/unity/fairseq2.cpp:605-756. */
    int32_t enc_variant;
    /* Code-HiFi-GAN duration predictor (models/vocoder/codehifigan.py:46-48, builder.py:53-58: VariancePredictor on the unit
     * embeddings, hidden dim / kernel size); 0 = not loaded.  Used by sc_vocoder_durations (v1 models: the autoregressive T2U
     * emits de-duplicated units and Translator.predict calls the vocoder with dur_prediction=True, translator.py:385-389). */
    int32_t voc_dur_pred_hidden_dim, voc_dur_pred_kernel_size;
    /* T2U family.  0: UnitY2 non-autoregressive T2U (sc_t2u_nar).  1: the v1 autoregressive UnitYT2UModel
     * (models/unity/t2u_builder.py:140-183: encoder + unit embedding frontend + pre-LN decoder, beam search over units;
     * inference/generator.py:316-336): sc_t2u_ar. */
    int32_t t2u_variant;
} sc_config;

/* Text generation options: the fields of SequenceGeneratorOptions
 * (inference/generator.py:59-84) that the HIP path honours. */
typedef struct sc_gen_opts {
    int32_t beam_size;        /* 1: greedy arg-max with a graph-captured step; 2..8: beam search (host-driven steps) */
    float soft_max_seq_len_a; /* max_len = min(hard, int(a*source_len) + b), prefix included */
    int32_t soft_max_seq_len_b;
    int32_t hard_max_seq_len;
    int32_t min_seq_len;
    float unk_penalty;
    int32_t use_graph; /* replay the decoder step from a captured hipGraph (greedy only) */
    float len_penalty;        /* beam search: hypothesis score / (len)^len_penalty (generator.py:81-84) */
    int32_t normalize_scores; /* beam search: apply the length normalisation (fairseq2 default: true) */
    /* SequenceGeneratorOptions.step_processor = NGramRepeatBlockProcessor(ngram_size) (generator.py:75,
     * cli/m4t/predict/predict.py:172-175): 0 = none; G > 0: a token that would complete a G-gram already
     * present in the row's sequence (prompt included) gets log-probability -inf.  Runs the host-driven
     * step loop for every beam_size (1 included). */
    int32_t no_repeat_ngram_size;
    /* Length of the SOURCE sequence the soft length rule is applied to.  fairseq2's generator is handed the source
     * sequences themselves (fbank frames for speech input, tokens for text input: inference/generator.py:261-263) and
     * computes int(a * source_len + b) from their padded length; 0 = use the encoder output length (the rule of the
     * ggml port, fairseq2.cpp:1097-1105, which is 8 x shorter for speech). */
    int32_t source_len;
} sc_gen_opts;

typedef struct sc_model sc_model;

const char* sc_last_error(void);
int sc_abi_version(void);

/* Copies the weights into HBM (the library owns them), repacks conv weights,
 * folds weight-norm, fuses QKV.  Replaces load_unity_model/load_vocoder_model +
 * model.to(device) (inference/translator.py:113-154). */
sc_model* sc_load(const sc_tensor_desc* tensors, size_t n_tensors, const sc_config* cfg, int device);
/* sc_load for the models sc_config cannot describe (added within ABI v10, purely additive; sc_config keeps its layout): the
 * SeamlessExpressive model `seamless_expressivity` (unity arch `expressivity_v2`, T2U arch `expressivity_nar`;
 * models/unity/builder.py:195-224, t2u_builder.py:235-281).
 *   ffn_activation      inner activation of the adaptor layer's FFN and of every NLLB FFN (use_gelu: builder.py:509-513, :581-590)
 *   t2u_ffn_activation  inner activation of the T2U encoder's FFNs (t2u_builder.py:697)
 *   film_cond_dim       > 0: the NAR T2U is FiLM-conditioned (models/unity/film.py) on a vector of this width.  Loads
 *                       t2u_model.decoder.layers.N.film.{proj.weight,proj.bias,s_gamma,s_beta}, t2u_model.decoder_frontend.
 *                       variance_adaptor.duration_predictor.film.* and t2u_model.prosody_proj.{weight,bias}.  Such a model runs
 *                       the packed T2U pass only (SC_T2U_PACKED=0 is ignored, with a message): model_dim and
 *                       var_pred_hidden_dim must be multiples of 64 up to 1024, t2u_conv_inner_dim a multiple of 32, the kernel
 *                       sizes odd - anything else fails here.  Needs the non-autoregressive T2U.
 * ext == NULL or an all-zero struct: sc_load.  Otherwise ext->abi_version must be SC_ABI_VERSION.  A GELU model is refused under
 * the SC_DECODER_GEN1 / SC_DECODER_GEN2 debug switches.  sc_fork carries all of it. */
typedef enum sc_ffn_activation { SC_FFN_RELU = 0, SC_FFN_GELU = 1 } sc_ffn_activation;
typedef struct sc_load_ext_opts {
    int32_t abi_version;
    int32_t ffn_activation;     /* sc_ffn_activation */
    int32_t t2u_ffn_activation; /* sc_ffn_activation */
    int32_t film_cond_dim;      /* 0 = no FiLM */
} sc_load_ext_opts;
sc_model* sc_load_ext(const sc_tensor_desc* tensors, size_t n_tensors, const sc_config* cfg, const sc_load_ext_opts* ext, int device);
/* A second handle on the SAME weights with its own HIP stream, scratch pool and result slots, so that
 * several micro-batches can be in flight on one GPU (one host thread per handle).  The parent must
 * outlive its forks; freeing a fork releases only its own scratch.  NAR tables set on the parent
 * before the fork are inherited. */
sc_model* sc_fork(sc_model* parent);
void sc_free(sc_model* m);
int sc_synchronize(sc_model* m);
/* Orders the handle's stream after everything enqueued so far on `producer_stream` (a hipStream_t; NULL = the
 * legacy default stream) without blocking the host: event record + hipStreamWaitEvent.  The handle's stream is
 * non-blocking, so a caller that fills device inputs on another stream (PyTorch's current stream in the Python
 * host) calls this before the stage that reads them.  Every stage returns only after its outputs are complete. */
int sc_wait_stream(sc_model* m, void* producer_stream);
/* Per-vocabulary tables for NARDecoderFrontend's string rules
 * (models/unity/nar_decoder_frontend.py:158-259), built once by the host from
 * the text / char tokenizers: token length, "starts with SPACE and len>1",
 * "is punctuation", CSR char ids. */
int sc_set_nar_tables(sc_model* m, int32_t vocab, const int32_t* h_tok_len, const uint8_t* h_starts_space,
                      const uint8_t* h_is_punct, const int64_t* h_char_offsets, const int32_t* h_char_ids);

/* a1: WaveformToFbankConverter(num_mel_bins=80, waveform_scale=2**15, standardize)
 * (translator.py:136-143) + Collater zero padding.  d_wav: [n][wav_stride] fp32
 * in [-1,1).  d_out: [n][t_rows][80]; rows >= frames are zero. */
int sc_fbank(sc_model* m, const float* d_wav, int32_t n, int64_t wav_stride, const int32_t* h_num_samples,
             int32_t standardize, float* d_out, int32_t t_rows, int32_t* h_out_frames);

/* The same at the waveform's OWN sample rate: fairseq2's converter takes {"waveform", "sample_rate"} and hands the rate to
 * kaldi without resampling (translator.py:270-292: `sample_rate` of predict(), or the decoded file's) - window int(rate * 25 ms),
 * shift int(rate * 10 ms), FFT size the next power of two, mel banks up to the rate's Nyquist.  16000 = sc_fbank.
 * sc_fbank_frames: frames of num_samples samples at that rate (0 below one window). */
int sc_fbank_rate(sc_model* m, const float* d_wav, int32_t n, int64_t wav_stride, const int32_t* h_num_samples, int32_t sample_rate,
                  int32_t standardize, float* d_out, int32_t t_rows, int32_t* h_out_frames);
int32_t sc_fbank_frames(int64_t num_samples, int32_t sample_rate);

/* a3-a7: UnitYModel.encode_speech (models/unity/model.py:132-139).
 * d_fbank [n][t_frames][80] (t_frames even), d_enc_out [n][sc_encoder_out_len(t_frames)][model_dim]. */
int32_t sc_encoder_out_len(const sc_model* m, int32_t t_frames);
int sc_encode_speech(sc_model* m, const float* d_fbank, int32_t n, int32_t t_frames, const int32_t* h_frame_lens,
                     float* d_enc_out, int32_t* h_out_lens);

/* The same on a RAGGED batch in one packed pass: item i is encoded from its own h_frame_lens[i] / fbank_stride stacked rows (a
 * trailing frame that does not fill a stride is dropped) and nothing else, so the batch costs the rows it has and an item's output
 * has the same bits in any batch, in any order and alone.  Above 64 stacked and 64 output rows they are the bits of
 * sc_encode_speech on the item alone; below, sc_encode_speech takes split-K products and the two agree to the encoder tolerance.
 * d_fbank [n][t_frames][80]: t_frames is the buffer's row stride only (any value >= the longest item).  d_enc_out
 * [n][s_enc_cap][model_dim] receives item i's h_out_lens[i] rows followed by zeros.  Runs on the handle's stream (forked handles
 * too) and returns with the stream drained.
 * SC_ERR_INVALID, sc_last_error naming the reason: a v1 model (enc_variant 1), dimensions the packed kernels do not take
 * (model_dim a multiple of 64 up to 1024, enc_ffn_dim a multiple of 32, 31 depthwise taps), an item with fewer than fbank_stride
 * frames, a frame length outside [0, t_frames].  SC_ERR_CAPACITY: s_enc_cap below the longest output length, or more packed rows
 * than a product operand of 2^31 elements holds (encode the batch in groups).  Nothing is written in either case. */
int sc_encode_speech_ragged(sc_model* m, const float* d_fbank, int32_t n, int32_t t_frames, const int32_t* h_frame_lens,
                            float* d_enc_out /* [n][s_enc_cap][model_dim] */, int32_t s_enc_cap, int32_t* h_out_lens);

/* a8-a11: greedy text generation with KV cache (BeamSearchSeq2SeqGenerator with
 * beam_size=1, echo_prompt=True; generator.py:147-156, :261-263).  h_out_ids
 * [n][max_len] (pad filled), h_out_lens[n] include prompt and EOS.  If
 * d_dec_hidden != NULL it receives the decoder output (after the final
 * LayerNorm) of every fed position: [n][max_len-1][model_dim] — the tensor the
 * reference recomputes with a second teacher-forced pass (generator.py:294-299). */
/* Text input (T2TT / T2ST): UnitYModel.encode_text (models/unity/model.py:138-151) = the shared embedding
 * frontend (embed * sqrt(model_dim) + sinusoidal positions from 0) and the pre-LN NLLB encoder stack + final
 * LayerNorm.  h_tokens [n][s_text] (pad filled), h_lens the PaddingMask; d_enc_out [n][s_text][model_dim]
 * feeds sc_generate_text with s_enc = s_text and h_enc_lens = h_lens. */
int sc_encode_text(sc_model* m, const int32_t* h_tokens, int32_t n, int32_t s_text, const int32_t* h_lens, float* d_enc_out);

/* Streaming (cfg 5): the monotonic multihead attention decoder the simultaneous policy drives
 * (MonotonicDecoderModel.decode / project, models/monotonic_decoder/model.py:41-66; caller
 * streaming/agents/online_text_decoder.py:205-243, :303-387).
 * sc_mma_begin = a fresh IncrementalStateBag over a (re-)encoded source (online_text_decoder.py:317): projects the
 * encoder-decoder K/V of every layer and the key-side energies of the LAST average-pooled source position.
 * d_enc [s_enc][model_dim] (one stream per handle); max_len = tokens that may be fed before the next begin.
 * sc_mma_step feeds h_tokens[0..n_tokens) at the next positions (the first call of a round feeds prefix + all
 * tokens written so far, later calls one token), and returns for the LAST fed token: *out_index = arg-max of the
 * projected logits with the h_blocked entries (may be NULL) set to -inf (online_text_decoder.py:226-231),
 * h_pchoose [mma_layers][num_heads] = p_choose[layer, head, -1, -1] (the policy reduces them: min / mean / median),
 * and d_features [n_tokens][model_dim] = the decoder outputs of the fed tokens. */
int sc_mma_begin(sc_model* m, const float* d_enc, int32_t s_enc, int32_t max_len);
int sc_mma_step(sc_model* m, const int32_t* h_tokens, int32_t n_tokens, const int32_t* h_blocked, int32_t n_blocked,
                int32_t* out_index, float* h_pchoose, float* d_features);

/* Streaming session pool (additive, ABI 10; no reference counterpart - SimulEval drives one stream): `sessions` concurrent
 * streams of the monotonic decoder share every decoder step.  Each session owns a self-attention K / V lane of max_len
 * positions, an encoder-decoder K / V lane of s_enc_cap rows per layer, its key-side energies, its position and its encoder
 * length; all memory is fixed at creation (sc_mma_pool_get_stats).  The pool runs on m's stream (forked handles work) and must
 * be freed before m; one host thread calls at a time.  A session's results do not depend on which other sessions exist, are
 * named in the same call, feed how many tokens or sit in which lanes: they are those of the same calls on a pool of one session,
 * bit for bit (they agree with sc_mma_step to fp32 re-association, not to the bit: other products, other summation order).
 * sc_mma_pool_begin = sc_mma_begin for the k sessions h_sessions[0..k) at once: d_enc holds their encoder outputs packed
 * [sum h_s_enc][model_dim] in call order; their positions return to 0.
 * sc_mma_pool_step = sc_mma_step for the k named sessions: session j feeds h_tokens[j * tok_stride .. + h_n_tokens[j]).  The call
 * runs max(h_n_tokens) decoder steps with the feeds right-aligned (session j joins at step max - h_n_tokens[j]), so that every
 * session's last token falls into the last step; for that token it returns h_out_index[j] (arg-max of the logits with the
 * session's h_blocked[j * blocked_stride .. + h_n_blocked[j]) entries at -inf; h_blocked may be NULL) and h_pchoose
 * [k][mma_layers][num_heads]; d_features receives the decoder outputs of all fed tokens, packed [sum h_n_tokens][model_dim] in
 * call order.  Sessions a call does not name are not touched.
 * SC_ERR_INVALID before any device work, no state changed: a NULL pointer, k outside 1..sessions, a session id out of range or
 * named twice, s_enc outside 1..s_enc_cap, a token outside the vocabulary, n_tokens < 1 or > tok_stride, position + n_tokens >
 * max_len (sc_last_error names the session), n_blocked outside 0..min(32, blocked_stride), a step on a session that never began.
 * sc_mma_pool_create returns NULL (sc_last_error) for a model without a monotonic decoder, sessions outside 1..512, or a model the
 * row-group step chain does not take.
 * Stats: the three byte counts are fixed at creation; begins = sessions begun, steps = decoder steps run, row_steps = rows those
 * steps carried (row_steps / steps = mean rows per step). */
typedef struct sc_mma_pool sc_mma_pool;
typedef struct sc_mma_pool_opts {
    int32_t abi_version, sessions /* 1..512 */, max_len, s_enc_cap;
} sc_mma_pool_opts;
typedef struct sc_mma_pool_stats {
    int64_t self_kv_bytes, cross_kv_bytes, work_bytes, begins, steps, row_steps;
} sc_mma_pool_stats;
sc_mma_pool* sc_mma_pool_create(sc_model* m, const sc_mma_pool_opts* opts);
void sc_mma_pool_free(sc_mma_pool* p);
int sc_mma_pool_begin(sc_mma_pool* p, const int32_t* h_sessions, int32_t k, const float* d_enc, const int32_t* h_s_enc);
int sc_mma_pool_step(sc_mma_pool* p, const int32_t* h_sessions, int32_t k, const int32_t* h_tokens, int32_t tok_stride,
                     const int32_t* h_n_tokens, const int32_t* h_blocked, int32_t blocked_stride, const int32_t* h_n_blocked,
                     int32_t* h_out_index, float* h_pchoose, float* d_features);
int sc_mma_pool_get_stats(sc_mma_pool* p, sc_mma_pool_stats* out, int32_t reset);

int32_t sc_text_max_len(const sc_model* m, const sc_gen_opts* opts, int32_t s_enc);
int sc_generate_text(sc_model* m, const float* d_enc, int32_t n, int32_t s_enc, const int32_t* h_enc_lens,
                     const sc_gen_opts* opts, const int32_t* h_prefix, int32_t prefix_len, int32_t* h_out_ids,
                     int32_t* h_out_lens, float* h_out_scores, float* d_dec_hidden);

/* sc_generate_text with a banned-sequence step processor (additive, ABI 10; fairseq2 0.2 BannedSequenceProcessor, the step
 * processor of the reference's MinTox re-decode, toxicity/mintox.py): h_banned_tokens / h_banned_offsets [n_banned + 1] are the
 * banned token sequences in CSR form (sequence q = tokens[offsets[q] .. offsets[q+1])).  At every step but the forced-EOS
 * one, for a row whose sequence so far (prompt included) has S tokens and every banned sequence b of length L: if L - 1 <= S
 * and the row's last L - 1 tokens equal b[0 .. L-1), the log-probability of b[L-1] becomes -inf (blocked after the row's
 * log-sum-exp, not renormalised; L == 1 bans its token always).  May be combined with opts->no_repeat_ngram_size.
 * n_banned == 0 is sc_generate_text.  With n_banned > 0 the call runs the host-driven step loop for every beam_size (1
 * included), never the decode engine; ids, lengths, scores and decoder outputs are otherwise what sc_generate_text documents.
 * The list is copied to the device once per call.  Limits (SC_ERR_INVALID before any device work): n_banned <= 4096, 1..64
 * tokens per sequence, 65536 tokens in all, every token inside the text vocabulary.  sc_generate_text_capture and sc_s2st
 * take no banned sequences. */
int sc_generate_text_banned(sc_model* m, const float* d_enc, int32_t n, int32_t s_enc, const int32_t* h_enc_lens,
                            const sc_gen_opts* opts, const int32_t* h_prefix, int32_t prefix_len, int32_t* h_out_ids,
                            int32_t* h_out_lens, float* h_out_scores, float* d_dec_hidden, const int32_t* h_banned_tokens,
                            const int32_t* h_banned_offsets /* [n_banned + 1] */, int32_t n_banned);

/* sc_generate_text_banned with phrase boosting (additive, ABI 10; "hot words" / contextual biasing.  An extension of this
 * library: the rule is in neither the reference nor fairseq2 0.2, and its effect on real speech has not been evaluated).
 * h_boost_tokens / h_boost_offsets [n_boost + 1]: the phrases as token sequences in CSR form, in any order; boost: the bonus in
 * log-probability units per matched token.  For a row whose sequence so far is y (prompt included): d(y) = the length of the
 * longest suffix of y that is a prefix of some phrase (a whole phrase counts; 0 if none); dp(y) = d(y) if that suffix is a
 * proper prefix of a phrase, 0 if it is a whole phrase; for every token t, k(y, t) = d(y + t) - dp(y) (-63 .. 64) and the row's
 * logit becomes fmaf(boost, (float)k, x[t]) - one fp32 operation on the unmodified logit, k == 0 keeps the bits.  Applied after
 * the row's log-sum-exp (not renormalised), after the n-gram and banned processors (-inf stays -inf), at every step but the
 * forced-EOS one, on the first step for beam 0 only.  So extending a match earns +boost, completing a phrase keeps what was
 * earned, and leaving a match of depth d unfinished costs every non-continuing token (EOS included) -boost * d: over a
 * hypothesis the sum is boost * (the summed lengths of the completed phrase occurrences) + boost * dp(final), the last term
 * non-zero only for a hypothesis cut at the length limit.  The returned scores INCLUDE the bonus.  boost < 0 is a soft ban.
 * n_boost == 0 or boost == 0 is sc_generate_text_banned.  Otherwise the call runs the host-driven step loop for every beam_size
 * (1 included), never the decode engine.  The list is sorted and copied to the device once per call.  Limits (SC_ERR_INVALID
 * before any device work, sc_last_error names the reason): n_boost <= 4096, 1..64 tokens per phrase, 65536 tokens in all, every
 * token inside the text vocabulary and neither pad nor EOS, no phrase a prefix of another (duplicates included), boost finite
 * with |boost| <= 100.  sc_generate_text_sampled, sc_generate_text_capture and sc_s2st take no phrase list. */
int sc_generate_text_boosted(sc_model* m, const float* d_enc, int32_t n, int32_t s_enc, const int32_t* h_enc_lens,
                             const sc_gen_opts* opts, const int32_t* h_prefix, int32_t prefix_len, int32_t* h_out_ids,
                             int32_t* h_out_lens, float* h_out_scores, float* d_dec_hidden, const int32_t* h_banned_tokens,
                             const int32_t* h_banned_offsets /* [n_banned + 1] */, int32_t n_banned, const int32_t* h_boost_tokens,
                             const int32_t* h_boost_offsets /* [n_boost + 1] */, int32_t n_boost, float boost);

/* Sampled text generation (additive, ABI 10; fairseq2 0.2 SamplingSeq2SeqGenerator with TopKSampler / TopPSampler - not part
 * of the reference tree, restated from memory: UNVERIFIED): num_gens stochastic hypotheses per utterance, drawn inside the step
 * loop.  At every step the logits are divided by `temperature`, the step processors (opts->no_repeat_ngram_size, the banned
 * list) and the step rules of sc_generate_text apply, top_k (0 = off) keeps the k most probable tokens, top_p then keeps a token
 * iff the probability mass strictly before it (descending order) is <= top_p, and one token is drawn from the kept set.  The
 * draw is a pure function of (row of logits, options, seed, stream id of the utterance, hypothesis number, position): integer
 * masses floor(p * 2^36) and Philox4x32-10, neither torch's generator nor the batch composition enters it (a token of
 * probability below 2^-36 is never drawn).  top_k == 1 is the arg-max with ties to the lowest index.
 * h_streams [n] (NULL: 0 .. n-1): the caller's 64-bit id of each utterance.  Outputs, per utterance sorted by score (NaN first,
 * then descending, ties in hypothesis order): h_out_ids [n][num_gens][max_len] (max_len = sc_text_max_len), h_out_lens and
 * h_out_scores [n][num_gens] (the score of sc_generate_text: the sum of the log-probabilities under the temperature and the
 * rules, prompt echo included, normalised as opts says), h_step_lprob [n][num_gens][max_len] (nullable; the log-probability of
 * every drawn token at its position, 0 elsewhere), d_dec_hidden [n][max_len - 1][M] (nullable; the teacher-forced decoder
 * outputs of hypothesis 0 after sorting).  opts->beam_size is ignored.  Runs the host-driven step loop, never the decode
 * engine.  SC_ERR_INVALID before any device work: num_gens outside 1..64, n * num_gens above 512, temperature not positive and
 * finite, top_k < 0, top_p outside (0, 1], a bad banned list (limits of sc_generate_text_banned). */
typedef struct sc_sample_opts {
    int32_t abi_version; /* SC_ABI_VERSION */
    int32_t num_gens;
    int32_t top_k;
    float top_p;
    float temperature;
    uint64_t seed;
} sc_sample_opts;
int sc_generate_text_sampled(sc_model* m, const float* d_enc, int32_t n, int32_t s_enc, const int32_t* h_enc_lens,
                             const sc_gen_opts* opts, const sc_sample_opts* sample_opts, const uint64_t* h_streams /* [n] or NULL */,
                             const int32_t* h_prefix, int32_t prefix_len, int32_t* h_out_ids, int32_t* h_out_lens, float* h_out_scores,
                             float* h_step_lprob, float* d_dec_hidden, const int32_t* h_banned_tokens,
                             const int32_t* h_banned_offsets /* [n_banned + 1] */, int32_t n_banned);

/* Greedy generation that also returns what the reference's Transcriber hooks into the model (ABI 10;
 * inference/transcriber.py:39-57, 124-127): per utterance and per FED position p (prompt positions included) the
 * probabilities of the last decoder layer's encoder-decoder attention of the query fed at p, summed over the heads,
 * d_xattn [n][max_len][s_enc] on the device (0 behind the utterance's encoder length), and h_step_lprob [n][max_len] on the
 * host: the log-probability (after the step rules) of the token chosen at p, 0 at prompt positions.  Positions at which an
 * utterance was not fed (after its EOS) are 0 in both.  max_len = sc_text_max_len(opts, s_enc).  Ids, lengths, scores and
 * decoder outputs equal sc_generate_text's bit for bit.  Greedy only (beam_size 1, no_repeat_ngram_size 0) on the row-group
 * decoder step (1..64 rows, heads of width 64, at most 16); other cases fail.  Runs on the handle's own step chain even
 * with a decode engine attached. */
int sc_generate_text_capture(sc_model* m, const float* d_enc, int32_t n, int32_t s_enc, const int32_t* h_enc_lens,
                             const sc_gen_opts* opts, const int32_t* h_prefix, int32_t prefix_len, int32_t* h_out_ids,
                             int32_t* h_out_lens, float* h_out_scores, float* d_dec_hidden, float* d_xattn, float* h_step_lprob);

/* Decode engine (ABI 8; no reference counterpart - the reference generates one batch at a time, inference/generator.py:
 * 227-299, and has no serving layer).  ONE greedy decoder-step chain per GPU, shared by every handle it is attached to: a
 * greedy sc_generate_text call on such a handle hands its rows to the engine after projecting their encoder K / V, the engine
 * puts them into free slots of its captured step, advances every slot at its row's own position, drops a row when it has
 * emitted EOS (or reached its own length limit) and refills the slot with a waiting row of any request - the decoder's
 * weights are streamed once per step for the rows of all passes in flight, a hypothesis costs as many steps as it has tokens,
 * and no pass carries its finished rows.  Per row the results (ids, lengths, scores, captured decoder outputs) are those of
 * the call without an engine, bit for bit: a row's arithmetic depends neither on its slot nor on its neighbours nor on the
 * step at which it entered.  Calls that do not fit (beam search, step processors, longer limits than the engine was built
 * for, other min_seq_len / unk_penalty) run on the handle's own chain as before, and so does a LONE call: when no other
 * request is inside the engine and no rows are announced (sc_engine_expect), there is nothing to share the chain with, and
 * the handle's own chain - whose kernels are sized for the call's rows, not for the engine's slots - is faster (batch-1
 * latency 95 instead of 121 ms).
 *   slots        rows per step (1..512; 0 = 64)                 rows   row states kept: rows in slots + rows that wait (0 = 4 x slots)
 *   max_len      longest hypothesis (prompt + tokens + EOS) a request may ask for (the K / V positions kept per row)
 *   s_enc        longest encoder output a request may bring
 *   poll         steps between two looks of the engine at the finished flags (0 = 4)
 *   low_water    with fewer rows than this the engine pauses WHILE announced rows (sc_engine_expect) are still on their way,
 *                at most max_wait_ms (0 = 100) - a step costs the same for 5 rows as for 64; 0 = never pause
 *   use_graph    replay the step from a captured hipGraph
 * The engine runs its own host thread and HIP stream; sc_engine_free stops it (requests still inside fail).  The model handle
 * given to sc_engine_create (and its weights) must outlive the engine, the engine the handles it is attached to. */
typedef struct sc_engine sc_engine;
typedef struct sc_engine_opts {
    int32_t slots, rows, max_len, s_enc;
    int32_t min_seq_len;
    float unk_penalty;
    int32_t poll, low_water, max_wait_ms, use_graph;
} sc_engine_opts;
typedef struct sc_engine_stats {
    int64_t steps;            /* step replays */
    int64_t row_steps;        /* sum over the steps of the rows in slots */
    int64_t useful_row_steps; /* sum over retired rows of the positions they needed (length - 1) */
    int64_t rows_admitted, rows_retired, requests, max_live;
    double busy_us;           /* wall time of the engine thread between starting an admit/step/look round and its end */
    double wait_us;           /* wall time paused below low_water */
    /* device memory the engine holds (fixed at creation): self-attention K / V = 2 * layers * slots * max_len * model_dim * 4
     * (one lane per SLOT), encoder K / V and captured decoder outputs per ROW STATE */
    int64_t self_kv_bytes, cross_kv_bytes, hidden_bytes;
} sc_engine_stats;
sc_engine* sc_engine_create(sc_model* m, const sc_engine_opts* opts);
void sc_engine_free(sc_engine* e);
/* e != NULL: greedy sc_generate_text calls of handle m that fit go through the engine (same device, same weights); NULL detaches */
int sc_engine_attach(sc_model* m, sc_engine* e);
/* handle m will submit n_rows rows soon (called when a pass starts, before its encoder stage): lets the engine wait for them
 * instead of stepping a nearly empty chain; the announcement ends with the handle's next sc_generate_text call, whatever
 * path that takes, or with n_rows < 0 (takes back up to -n_rows rows) */
int sc_engine_expect(sc_model* m, int32_t n_rows);
int sc_engine_get_stats(sc_engine* e, sc_engine_stats* out, int32_t reset);

/* Teacher-forced decoder pass over given tokens (UnitYModel.decode without
 * state bag, models/unity/model.py:154-180).  h_tokens [n][s_text];
 * d_dec_hidden [n][s_text][model_dim]. */
int sc_decode_text(sc_model* m, const float* d_enc, int32_t n, int32_t s_enc, const int32_t* h_enc_lens,
                   const int32_t* h_tokens, int32_t s_text, float* d_dec_hidden);

/* Teacher-forced scoring: how probable the model finds GIVEN target sequences (forced-decoding scores, n-best re-ranking,
 * perplexity / held-out loss, token accuracy) - the forward half of the reference's evaluation loss
 * (cli/m4t/finetune/trainer.py:100-125 UnitYFinetuneWrapper.forward, S2T half: encode, teacher-forced decode, final_proj;
 * :155-188 CalcLoss).  d_enc / h_enc_lens: sc_encode_speech or sc_encode_text output, as for sc_generate_text.
 *   h_tokens   [n][s_text]  whole sequences, prompt ... EOS (</s> __lang__ w1 ... </s>), pad-filled behind tok_lens[b]
 *   h_tok_lens [n]          2 .. s_text;  s_text <= text_max_seq_len
 * Position p < tok_lens[b] - 1 feeds tokens[b][p] (with everything in front of it) and scores tokens[b][p + 1]:
 *   h_tok_lprob [n][s_text-1]            log p(tokens[b][p+1] | tokens[b][..p]), always <= 0
 *   h_sum_lprob [n][s_text-1] (nullable) sum over the vocabulary of the log-probabilities at p (label smoothing's term)
 *   h_top1      [n][s_text-1] (nullable) the arg-max token at p (lowest id among equal values)
 * Positions behind tok_lens[b] - 1 hold 0 (h_top1: -1).  d_dec_hidden (nullable) [n][s_text-1][model_dim] receives the decoder
 * output of tokens[:, :-1].  An item's results do not depend, to the bit, on what else is in the batch or on the padded
 * widths: the decoder pass runs its tiled products whatever the row count, and the vocabulary projection keeps per-row
 * log-softmax statistics in the product's epilogue (no [rows][vocab] buffer exists).  d_dec_hidden therefore equals
 * sc_decode_text's output to the bit wherever that runs the tiled products too (more than 64 rows, n * (s_text - 1));
 * below, sc_decode_text takes skinny products with another summation order and the two agree to fp32 re-association.
 * Runs on the handle's own stream (never the decode engine); works on forked handles and for every text decoder the
 * handle can hold.  SC_ERR_INVALID before any device work for a NULL pointer, a
 * tok_lens / enc_lens entry out of range, a token outside the vocabulary or s_text > text_max_seq_len. */
int sc_score_text(sc_model* m, const float* d_enc, int32_t n, int32_t s_enc, const int32_t* h_enc_lens, const int32_t* h_tokens,
                  const int32_t* h_tok_lens, int32_t s_text, float* h_tok_lprob, float* h_sum_lprob, int32_t* h_top1,
                  float* d_dec_hidden);

/* sc_score_text with the decoder's cross-attention rows (additive, ABI 10): forced alignment - WHEN the words of a given text
 * were spoken.  The reference's Transcriber hooks the last decoder layer's encoder-decoder attention while it generates
 * (inference/transcriber.py:39-57); here the same quantity comes out of the one batched teacher-forced pass, for known tokens:
 *   d_xattn [n][s_text-1][s_enc] (device)  d_xattn[b][p][j] = sum over the heads, in head order, of
 *                                          softmax_j(q_h(b, p) . k_h(b, j) / 8) of the LAST decoder layer, for
 *                                          p < tok_lens[b] - 1 and j < enc_lens[b]; 0 everywhere else (the call writes
 *                                          those zeros: the buffer need not be cleared).  A live row sums to the head count.
 * Everything sc_score_text documents holds unchanged, and h_tok_lprob / h_sum_lprob / h_top1 / d_dec_hidden carry the bits
 * sc_score_text returns on the same arguments: the call adds ONE launch behind the last layer's query and key products
 * (fp32 scores, soft-max and head sum; k_xattn.hip states the arithmetic order) and changes nothing else.  An item's rows do
 * not depend, to the bit, on what else is in the batch or on the padded widths.  They agree with sc_generate_text_capture's
 * rows for the same tokens to fp32 re-association, not to the bit (other products form the queries).  Runs on the handle's
 * own stream (never the decode engine); works on forked handles.  SC_ERR_INVALID before any device work for a NULL d_xattn,
 * for everything sc_score_text rejects, and for a decoder whose heads are not 64 wide or number more than 16. */
int sc_score_text_capture(sc_model* m, const float* d_enc, int32_t n, int32_t s_enc, const int32_t* h_enc_lens, const int32_t* h_tokens,
                          const int32_t* h_tok_lens, int32_t s_text, float* h_tok_lprob, float* h_sum_lprob, int32_t* h_top1,
                          float* d_dec_hidden, float* d_xattn);

/* Spoken-language identification (additive, ABI 10): which __lang__ token the text decoder expects after the prompt - the
 * reference's "LID scores" (ggml/examples/unity/fairseq2.cpp:1208-1221: the decoder is fed the prompt's </s>, the log-softmax of
 * the next position is read at every language token; its target language `unk` takes their arg-max, :1227-1236).
 *   h_prefix [prefix_len]   the tokens fed, normally {</s>}; 1 <= prefix_len <= text_max_seq_len; one prompt for all items
 *   h_cand   [n_cand]       candidate token ids, strictly ascending, inside the vocabulary; 1 <= n_cand <= 512
 *   h_lprob  [n][n_cand]    log-softmax over the WHOLE vocabulary at the position behind the prompt, read at the candidates:
 *                           raw (no step rules, not renormalised over the candidates), always <= 0
 *   h_best   [n]            index into h_cand of the largest value (the lowest index among equal values)
 * The prompt goes through sc_score_text's batched causal pass and the vocabulary projection reads the candidate columns in its
 * epilogue: h_lprob[b][j] carries the bits of sc_score_text's h_tok_lprob at the last position of the sequence
 * prefix + {h_cand[j]}, at the cost of ONE pass over the projection weight, and an item's results do not depend on what else is
 * in the batch.  Runs on the handle's own stream (never the decode engine); works on forked handles and for every text decoder
 * the handle can hold.  SC_ERR_INVALID before any device work for a NULL pointer, n_cand outside 1..512, a list that is not
 * strictly ascending, an id outside the vocabulary, an enc_lens entry out of range or prefix_len outside 1..text_max_seq_len. */
int sc_identify_language(sc_model* m, const float* d_enc, int32_t n, int32_t s_enc, const int32_t* h_enc_lens, const int32_t* h_prefix,
                         int32_t prefix_len, const int32_t* h_cand, int32_t n_cand, float* h_lprob, int32_t* h_best);

/* sc_generate_text with ONE PROMPT PER ROW (additive, ABI 10): h_prefix_rows [n][prefix_len], row b is fed its own prompt - a
 * batch in mixed target languages, e.g. the languages sc_identify_language chose.  All prompts of a call have the same length.
 * Everything else is sc_generate_text's, on every path it takes: the handle's greedy chain, the decode engine (per-row tokens
 * in the admit record) and the host-driven beam / n-gram loop (every beam of an utterance gets its utterance's prompt).  A row's
 * results carry the bits of the sc_generate_text call whose shared prompt is that row's.  SC_ERR_INVALID for a prompt token
 * outside the vocabulary.  sc_generate_text_banned, sc_generate_text_sampled and sc_generate_text_capture keep the shared
 * prompt. */
int sc_generate_text_rows(sc_model* m, const float* d_enc, int32_t n, int32_t s_enc, const int32_t* h_enc_lens,
                          const sc_gen_opts* opts, const int32_t* h_prefix_rows /* [n][prefix_len] */, int32_t prefix_len,
                          int32_t* h_out_ids, int32_t* h_out_lens, float* h_out_scores, float* d_dec_hidden);

/* FORCED TARGET PREFIXES: sc_generate_text with one prompt per row, of ANY length per row (additive, ABI 10).  Row b is fed
 * h_prompt_rows[b][0 .. h_prompt_lens[b]) - normally `</s> __lang__ p1 .. pk`, k = 0 allowed - and generates from there; what
 * lies behind a row's length is ignored.  max_len = sc_text_max_len(opts, s_enc), shared by the call.
 * The contract: for every row b the ids, the length, the score and the decoder-output rows are, bit for bit, those of row b of
 * the uniform call (sc_generate_text / _banned / _boosted) on the same batch whose shared prompt is row b's prompt.  Hence: a
 * greedy score leaves the prompt out, a beam score includes the echoed prompt's raw log-probabilities; the step processors
 * (n-gram, banned sequences, boost phrases) see the prompt as part of the row's sequence, but nothing is chosen, blocked or
 * boosted at a forced position; min_seq_len, unk_penalty and the forced EOS at max_len - 2 act on free positions only.
 * One qualification, for d_dec_hidden in a beam search (beam_size > 1 or any step processor): there the decoder outputs do not
 * come from the step but from one teacher-forced pass over the chosen hypotheses of the whole batch, whose products are chosen
 * by its row count n * (longest hypothesis - 1), at most 64 rows or more.  They carry the uniform call's bits when both calls'
 * passes fall on the same side of that threshold and agree to fp32 re-association otherwise - as with sc_generate_text_rows;
 * ids, lengths and scores are not affected.
 * With all lengths equal the call IS sc_generate_text_rows (with the banned / boost lists of sc_generate_text_boosted).  Mixed
 * lengths stay ONE batch on every path: the greedy chain and the beam loop echo the prompts up to the shortest one on the host
 * and handle the longer ones inside the step, per row; the decode engine takes the per-row lengths in its admit record, which
 * holds at most 12 prompt tokens - a call with a longer prompt runs on the handle's own chain as a whole.
 * Lists as sc_generate_text_boosted's (n_banned == 0 / n_boost == 0: none).
 * SC_ERR_INVALID before any device work, sc_last_error naming the row: a NULL pointer, a length outside 1 .. prompt_stride or
 * >= max_len, a token outside the vocabulary, pad or EOS at any prompt position but 0, and whatever the banned / boosted
 * entries reject.  Not evaluated on real speech.  sc_generate_text_sampled and sc_generate_text_capture keep the shared prompt. */
int sc_generate_text_prompts(sc_model* m, const float* d_enc, int32_t n, int32_t s_enc, const int32_t* h_enc_lens,
                             const sc_gen_opts* opts, const int32_t* h_prompt_rows /* [n][prompt_stride] */, int32_t prompt_stride,
                             const int32_t* h_prompt_lens /* [n], 1 .. prompt_stride */, int32_t* h_out_ids, int32_t* h_out_lens,
                             float* h_out_scores, float* d_dec_hidden, const int32_t* h_banned_tokens,
                             const int32_t* h_banned_offsets, int32_t n_banned, const int32_t* h_boost_tokens,
                             const int32_t* h_boost_offsets, int32_t n_boost, float boost);

/* Beam n-best lists with per-token scores: sc_generate_text_prompts' arguments (one prompt per row, of any length; lists as
 * sc_generate_text_boosted's), but EVERY finished hypothesis of the search leaves, best first - the reference generator's list of
 * hypotheses with seq, score and step_scores (ggml/examples/unity/fairseq2.cpp:1310-1348, :1597-1602).  beam_size is 1..8 and the
 * call always runs the host-driven beam loop (never the decode engine or the greedy chain); nbest is 1..beam_size.
 * Outputs (host): h_out_ids [n][nbest][max_len] (max_len = sc_text_max_len(opts, s_enc); pad behind a hypothesis' length),
 * h_out_lens / h_out_scores [n][nbest], h_out_counts [n] = min(finished hypotheses, nbest) >= 1, and h_step_scores (nullable)
 * [n][nbest][max_len]: step[0] = 0, step[t] = c[t] - c[t-1] for 1 <= t < len, one fp32 subtraction of the search's cumulative
 * scores c (prompt positions: the echoed prompt's raw log-probabilities; the last one: the EOS candidate's un-normalised score),
 * 0 behind the length.  So sum(step) is the hypothesis' un-normalised score and score = sum / (len - 1)^len_penalty when
 * normalize_scores is set.  Hypothesis rows behind h_out_counts[u] are pad / length 0 / score 0 / step 0.  The order is the one
 * the other entries pick their winner in: NaN first, then the higher score, ties to the hypothesis that finished earlier.
 * The contract: hypothesis 0 of every utterance equals sc_generate_text_prompts on the same arguments bit for bit - ids, length
 * and score.  With a boost list the scores and the step scores include the bonus, as sc_generate_text_boosted documents.
 * The score history lives in device memory beside the beams' sequences and is allocated by this entry alone.
 * SC_ERR_INVALID before any device work, sc_last_error naming the reason: a NULL pointer (h_step_scores may be NULL), beam_size
 * outside 1..8, nbest outside 1..beam_size, and everything sc_generate_text_prompts refuses.  An utterance without a finished
 * hypothesis is an error, as it is there.  Decoder outputs are not captured (the n-best of sc_t2u_ar / sc_s2st: not built). */
int sc_generate_text_nbest(sc_model* m, const float* d_enc, int32_t n, int32_t s_enc, const int32_t* h_enc_lens, const sc_gen_opts* opts,
                           const int32_t* h_prompt_rows /* [n][prompt_stride] */, int32_t prompt_stride,
                           const int32_t* h_prompt_lens /* [n], 1 .. prompt_stride */, int32_t nbest,
                           int32_t* h_out_ids /* [n][nbest][max_len] */, int32_t* h_out_lens /* [n][nbest] */,
                           float* h_out_scores /* [n][nbest] */, int32_t* h_out_counts /* [n] */,
                           float* h_step_scores /* [n][nbest][max_len], nullable */, const int32_t* h_banned_tokens,
                           const int32_t* h_banned_offsets, int32_t n_banned, const int32_t* h_boost_tokens,
                           const int32_t* h_boost_offsets, int32_t n_boost, float boost);

/* a12-a17: UnitYNART2UModel.forward + argmax + unit decoding
 * (models/unity/model.py:379-441, generator.py:338-353).  h_text_seqs
 * [n][s_text] is text_seqs[:, :-1] (pad filled), h_text_lens its PaddingMask.
 * Results are kept in the handle: sizes via the out params, ids via
 * sc_get_units / sc_get_durations. */
int sc_t2u_nar(sc_model* m, const float* d_dec_hidden, int32_t n, int32_t s_text, const int32_t* h_text_lens,
               const int32_t* h_text_seqs, float duration_factor, int32_t* h_unit_lens, int32_t* out_s_unit_max,
               int32_t* out_s_char_max);
/* sc_t2u_nar of a FiLM-conditioned model (sc_load_ext with film_cond_dim > 0; UnitYNART2UModel.forward with film_cond_emb,
 * models/unity/model.py:379-403): d_cond [n][film_cond_dim] fp32 on the device, one conditioning vector per item (the prosody
 * encoder's output, inference/generator.py:305-314).  prosody_proj(cond) is added to the T2U encoder output of every position;
 * the duration predictor and every FFT decoder layer apply FiLM behind their last LayerNorm.  An item's result does not depend on
 * its companions.  SC_ERR_INVALID: a model without FiLM here, a FiLM model in sc_t2u_nar or sc_s2st - no entry produces
 * unconditioned units from a conditioned model. */
int sc_t2u_nar_cond(sc_model* m, const float* d_dec_hidden, int32_t n, int32_t s_text, const int32_t* h_text_lens,
                    const int32_t* h_text_seqs, float duration_factor, const float* d_cond, int32_t* h_unit_lens,
                    int32_t* out_s_unit_max, int32_t* out_s_char_max);
/* sc_t2u_nar with one duration factor PER ITEM, fitted on the device to a unit budget (added within ABI v10, purely additive;
 * an extension of this project for long-form speech translation, no reference counterpart).  With
 * e_k = exp(x_k) - 1 of item b's characters (x_k: the duration predictor's output, as in sc_t2u_nar),
 * dur_k(f) = clamp(round_half_even(e_k * f), 1, 1000000) and U_b(f) = sum_k dur_k(f), the item's factor is the largest point of
 * the grid f_j = min(hi, lo + (hi - lo) * j / 65536), j = 0..65536 (f_65536 = hi exactly; fp32, each operation rounded), with
 * U_b(f_j) <= h_target_units[b].  A target of 0 is no budget: the factor is h_hi[b].  If even h_lo[b] does not fit, the factor
 * is h_lo[b] and bit 0 of h_flags[b] is set.  h_factor [n] and h_flags [n] are written; units, lengths and durations stay in
 * the handle as for sc_t2u_nar.  Row b equals row b of sc_t2u_nar / sc_t2u_nar_cond on the same batch with duration_factor =
 * h_factor[b].  d_cond: NULL, or [n][film_cond_dim] for a FiLM-conditioned model (required there, refused elsewhere).
 * SC_ERR_INVALID before any device work, sc_last_error naming the item: a null pointer, a negative target, a bound that is not
 * finite, lo <= 0, lo > hi. */
int sc_t2u_nar_fit(sc_model* m, const float* d_dec_hidden, int32_t n, int32_t s_text, const int32_t* h_text_lens,
                   const int32_t* h_text_seqs, const int32_t* h_target_units, const float* h_lo, const float* h_hi,
                   const float* d_cond, int32_t* h_unit_lens, int32_t* out_s_unit_max, int32_t* out_s_char_max, float* h_factor,
                   int32_t* h_flags);
int sc_get_units(sc_model* m, int32_t* h_units /* [n][s_unit_max], pad = unit_pad_idx */);
int sc_get_durations(sc_model* m, int32_t* h_durations /* [n][s_char_max] */, int32_t* h_char_ids,
                     int32_t* h_char_seq_lens);

/* a19-a20: Vocoder.forward with dur_prediction=False (models/vocoder/vocoder.py:25-49,
 * codehifigan.py:75-101, hifigan.py:180-196).  d_wav [n][s_units*hop]. */
int32_t sc_vocoder_hop(const sc_model* m);
int sc_vocode(sc_model* m, const int32_t* h_units, int32_t n, int32_t s_units, const int32_t* h_lang_idx,
              const int32_t* h_spkr_idx, float* d_wav);
/* v1 models: UnitYT2UModel generation (inference/generator.py:316-336).  d_dec_hidden [n][s_text][model_dim]: decoder
 * outputs of the text sequences without their final EOS (as for sc_t2u_nar), h_text_lens their lengths.  Beam search over
 * the unit decoder with `opts` (the reference's unit_opts: beam_size 5, soft_max_seq_len (25, 50)) from the prompt
 * `h_prefix` (UnitTokenizer encoder prefix: [eos, lang]).  h_out_ids [n][unit_cap] (prompt echoed, EOS included, padded
 * with the unit pad index), unit_cap >= sc_t2u_ar_max_len(...). */
int sc_t2u_ar(sc_model* m, const float* d_dec_hidden, int32_t n, int32_t s_text, const int32_t* h_text_lens, const sc_gen_opts* opts,
              const int32_t* h_prefix, int32_t prefix_len, int32_t* h_out_ids, int32_t unit_cap, int32_t* h_out_lens, float* h_scores);
int32_t sc_t2u_ar_max_len(sc_model* m, const sc_gen_opts* opts, int32_t s_text);

/* CodeGenerator.forward with dur_prediction=True, first half (models/vocoder/codehifigan.py:79-88): durations
 * clamp(round(exp(dur_predictor(dict(units))) - 1), min=1) of every unit position, h_durations [n][s_units].  The caller
 * repeats each unit by its duration (embedding lookup and repeat_interleave commute) and passes the expanded sequence to
 * sc_vocode.  Like the reference there is no padding mask: every position of the [n][s_units] matrix gets a duration. */
int sc_vocoder_durations(sc_model* m, const int32_t* h_units, int32_t n, int32_t s_units, int32_t* h_durations);

/* The same for a padded batch of which only the first h_unit_lens[i] * hop samples of row i will be kept (the
 * proportional trim of Translator.predict, inference/translator.py:411-419, never keeps more): rows are vocoded in length
 * buckets, each on min(s_units, unit_lens[i] + receptive field) frames of the padded row, so the kept samples are those of
 * the padded batch while the padding itself is not synthesised.  Samples behind that window read as zero. */
int sc_vocode_ragged(sc_model* m, const int32_t* h_units, int32_t n, int32_t s_units, const int32_t* h_unit_lens,
                     const int32_t* h_lang_idx, const int32_t* h_spkr_idx, float* d_wav);
/* The whole speech-to-speech chain of Translator.predict(fbank SequenceData, "S2ST") in one call (inference/translator.py:
 * 304-428 without the string conversions): sc_encode_speech -> sc_generate_text -> sc_t2u_nar -> sc_vocode_ragged on
 * buffers the library owns.  d_fbank [n][t_frames][80] on the device; h_text_ids [n][text_cap] (pad filled, text_cap >=
 * sc_text_max_len(opts with source_len = t_frames)), h_text_lens [n]; h_units [n][unit_cap] (pad = unit_pad_idx) and
 * h_unit_lens [n]; d_wav [n][unit_cap * hop] on the device, row i valid up to h_unit_lens[i] * hop samples (what the
 * proportional trim of translator.py:411-419 keeps at most), zero behind.  *out_s_unit_max = the batch's longest unit
 * sequence (the reference's padded width, needed for that trim).  SC_ERR_* when a capacity is too small. */
int sc_s2st(sc_model* m, const float* d_fbank, int32_t n, int32_t t_frames, const int32_t* h_frame_lens, const sc_gen_opts* opts,
            const int32_t* h_prefix, int32_t prefix_len, float duration_factor, const int32_t* h_lang_idx, const int32_t* h_spkr_idx,
            int32_t* h_text_ids, int32_t text_cap, int32_t* h_text_lens, int32_t* h_units, int32_t unit_cap, int32_t* h_unit_lens,
            float* d_wav, int32_t* out_s_unit_max);
/* Unit rows the last sc_t2u_nar call computed in its length buckets / would have computed padded to the batch maximum,
 * and the unit frames the last sc_vocode* call computed (measurement: padding is not useful work). */
int sc_last_padding(sc_model* m, int64_t* t2u_rows_computed, int64_t* t2u_rows_padded, int64_t* vocoder_rows_computed);

/* Per-kernel HIP-event timing on the handle's stream (bench.py roofline).  The report is text:
 * one "name launches total_ms algorithmic_flops algorithmic_bytes" line per kernel family. */
int sc_prof_enable(int on);
int sc_prof_reset(void);
int64_t sc_prof_report(char* buf, int64_t cap);

/* Host logic of NARDecoderFrontend's string rules (models/unity/nar_decoder_frontend.py:31-49, :158-259) exactly as
 * sc_t2u_nar runs it, on caller-supplied tables (the arguments of sc_set_nar_tables) — no device work, callable without a
 * GPU.  h_text_seqs [n][s_text] is text_seqs[:, :-1]; writes the per-subword character counts [n][s_text] (zero at the
 * language slot and on padding), the character ids [n][cap] and their number per item; returns the longest sequence or a
 * negative status. */
int32_t sc_text_to_char_seqs(int32_t vocab, const int32_t* h_tok_len, const uint8_t* h_starts_space, const uint8_t* h_is_punct,
                             const int64_t* h_char_offsets, const int32_t* h_char_ids, int32_t pad_idx, int32_t unk_idx,
                             int32_t eos_idx, const int32_t* h_text_seqs, int32_t n, int32_t s_text, int32_t* h_char_lens,
                             int32_t* h_out_char_ids, int32_t cap, int32_t* h_char_seq_lens);

/* Host logic of the n-gram step processor (no device work; callable without a GPU): the tokens
 * NGramRepeatBlockProcessor(ngram_size) blocks after the `len` tokens of `h_seq`.  Writes at most `cap`
 * of them to h_out (in window order, duplicates kept) and returns how many there are, or a negative status. */
int32_t sc_ngram_blocked_tokens(const int32_t* h_seq, int32_t len, int32_t ngram_size, int32_t* h_out, int32_t cap);

/* Host logic of the banned-sequence step processor (no device work; callable without a GPU): the tokens that the list of
 * sc_generate_text_banned (same limits, except that there is no vocabulary to check tokens against) blocks after the `len`
 * tokens of `h_seq`.  Writes at most `cap` of them to h_out (in banned-list order, duplicates kept) and returns how many
 * there are, or a negative status. */
int32_t sc_banned_blocked_tokens(const int32_t* h_seq, int32_t len, const int32_t* h_banned_tokens, const int32_t* h_banned_offsets,
                                 int32_t n_banned, int32_t* h_out, int32_t cap);

/* Host logic of the phrase-boost step processor (no device work; callable without a GPU): for the `len` tokens y of `h_seq`
 * and the list of sc_generate_text_boosted (same limits, except that there is no vocabulary, pad or EOS to check tokens
 * against), the tokens t with d(y + t) > 0 in ascending order to h_out_tokens and d(y + t) to h_out_k (at most `cap` each),
 * dp(y) to *out_dp (nullable).  k(y, t) = d(y + t) - dp(y); every token not listed has d(y + t) = 0.  Returns how many tokens
 * there are, or a negative status. */
int32_t sc_boost_deltas(const int32_t* h_seq, int32_t len, const int32_t* h_boost_tokens, const int32_t* h_boost_offsets, int32_t n_boost,
                        int32_t* h_out_tokens, int32_t* h_out_k, int32_t cap, int32_t* out_dp);

/* UnitY2 forced aligner (the `nar_t2u_aligner` card; added within ABI v10, purely additive).  A handle of its own: the aligner
 * is a separate checkpoint with its own vocabularies, stream and scratch pool.  Configuration as
 * models/aligner/builder.py:64-87 (`nar_t2u_aligner_base`: model_dim = feat_dim = 1024, 2 text layers, 3 feature layers,
 * temperature 1.0, reduction_factor 1, 10943 characters, 10082 units).  Tensor names are those of the converted checkpoint
 * (models/aligner/loader.py:22-57): alignment_frontend.embed_text.weight, alignment_frontend.embed_unit.weight,
 * alignment_encoder.t_conv.{1 + 3 i}.{weight,bias}, alignment_encoder.f_conv.{1 + 3 i}.{weight,bias} (the positions of the
 * Conv1d modules inside the nn.Sequential of models/aligner/model.py:99-144); weights are held as fp16, biases as fp32. */
typedef struct sc_aligner_config {
    int32_t abi_version; /* must be SC_ABI_VERSION */
    int32_t model_dim, feat_dim; /* multiples of 32 */
    int32_t text_layers, feat_layers; /* Conv1d(k=3, pad=1) + ReLU each, the last one Conv1d(k=1) (stride reduction_factor on the feature side) */
    float temperature;
    int32_t reduction_factor;
    int32_t char_vocab_size, unit_vocab_size;
} sc_aligner_config;
typedef struct sc_aligner sc_aligner;
sc_aligner* sc_aligner_load(const sc_tensor_desc* tensors, size_t n_tensors, const sc_aligner_config* cfg, int device);
void sc_aligner_free(sc_aligner* a);
/* UnitY2AlignmentModel.forward (models/aligner/model.py:293-304: frontend :68-71, encoder :146-190, viterbi_decode :246-277)
 * on a ragged batch: h_text_ids [n][s_text] char ids (alignment_frontend.tokenize_text), h_unit_ids [n][s_unit] unit ids of
 * the NAR unit encoder (tokenize_unit), positions behind an item's length hold any id of the vocabulary.  h_durations
 * [n][s_text]: frames of every character, zeros behind the text length; with reduction_factor > 1 they count REDUCED frames
 * (ceil(unit_len / reduction_factor) in all) and the caller applies postprocess_alignment (model.py:192-209).
 * d_lprob_or_null: device buffer [n][ceil(s_unit / reduction_factor)][s_text] that receives attn_lprob (-inf behind the text
 * length, zeros behind the feature length).  The search (model.py:212-243) runs on the device with a double-precision Q and
 * the reference's tie rule; limits: 2048 characters and 8192 (reduced) frames per item, SC_ERR_INVALID above. */
int sc_align(sc_aligner* a, const int32_t* h_text_ids, int32_t n, int32_t s_text, const int32_t* h_text_lens,
             const int32_t* h_unit_ids, int32_t s_unit, const int32_t* h_unit_lens, int32_t* h_durations,
             float* d_lprob_or_null);

/* UnitExtractor (the `xlsr2_1b_v2` card + a k-means table; added within ABI v10, purely additive).  A handle of its own.
 * Configuration as models/unit_extractor/wav2vec2_layer_output.py:23-53 (model_dim 1280, 16 heads, FFN 5120, 48 layers,
 * extractor (512,10,5) + 4 x (512,3,2) + 2 x (512,2,2) with bias and per-layer LayerNorm, position conv k = 128 in 16 groups).
 * The head dimension model_dim / heads must be 64 or 80.  Tensor names are fairseq2's:
 *   encoder_frontend.feature_extractor.layers.{i}.conv.{weight,bias}, ...layers.{i}.layer_norm.{weight,bias},
 *   encoder_frontend.post_extract_layer_norm.*, encoder_frontend.model_dim_proj.*,
 *   encoder_frontend.pos_encoder.conv.{weight,bias} - `weight` [model_dim][model_dim / groups][k] with the weight-norm
 *   (weight_g, weight_v, dim = 2) already folded, kept as fp32,
 *   encoder.layers.{i}.{self_attn_layer_norm,ffn_layer_norm}.*, encoder.layers.{i}.self_attn.{q,k,v,output}_proj.*,
 *   encoder.layers.{i}.ffn.{inner,output}_proj.*, and kmeans.centroids [model_dim][num_centroids] (kmeans.py:19-21).
 * Linear / Conv1d weights are held as fp16, everything else as fp32. */
#define SC_UE_MAX_FE_LAYERS 8
typedef struct sc_unit_extractor_config {
    int32_t abi_version; /* must be SC_ABI_VERSION */
    int32_t model_dim, heads, ffn_dim, layers;
    int32_t feature_dim; /* width of the convolutional feature extractor */
    int32_t fe_layers;   /* <= SC_UE_MAX_FE_LAYERS; layer 0 has one input channel */
    int32_t fe_kernel[SC_UE_MAX_FE_LAYERS], fe_stride[SC_UE_MAX_FE_LAYERS];
    int32_t pos_conv_kernel, pos_conv_groups;
    int32_t num_centroids;
} sc_unit_extractor_config;
typedef struct sc_unit_extractor sc_unit_extractor;
sc_unit_extractor* sc_unit_extractor_load(const sc_tensor_desc* tensors, size_t n_tensors, const sc_unit_extractor_config* cfg, int device);
void sc_unit_extractor_free(sc_unit_extractor* u);
/* frames the extractor table yields for num_samples samples: floor((L - k) / s) + 1 per layer, 0 when the input is too short */
int32_t sc_unit_extractor_num_frames(const sc_unit_extractor_config* cfg, int64_t num_samples);
/* UnitExtractor.predict (unit_extractor.py:62-98) on a ragged batch of mono 16 kHz waveforms: h_wav [n][wav_stride] on the
 * host, h_num_samples [n].  Every item is normalised over its own samples (an odd length counts one more sample of value 1.0,
 * the reference's Collater(pad_value=1, pad_to_multiple=2); the frame count comes from the unpadded length), runs the feature
 * extractor, the projection, the position encoder and Transformer layers 0 .. out_layer_idx - later layers are not run, the
 * final encoder LayerNorm is not applied - and the k-means arg-min (lowest index among equal distances).
 * h_units [n][max_frames] int32 (zeros behind an item's frames), h_frames [n]; d_features_or_null: device buffer
 * [n][longest item's frames][model_dim] that receives the layer output (rows behind an item's frames are undefined).
 * SC_ERR_INVALID, with nothing launched: out_layer_idx outside 0 .. layers-1, an item with fewer samples than one frame needs
 * or with more than 4096 frames (1 310 800 samples at the xlsr2_1b_v2 table), max_frames below the longest item. */
int sc_extract_units(sc_unit_extractor* u, const float* h_wav, int32_t n, int64_t wav_stride, const int32_t* h_num_samples,
                     int32_t out_layer_idx, int32_t* h_units, int32_t max_frames, int32_t* h_frames, float* d_features_or_null);

/* ProsodyEncoder: the ECAPA-TDNN of SeamlessExpressive (models/pretssel/ecapa_tdnn.py, arch `base` of ecapa_tdnn_builder.py;
 * added within ABI v10, purely additive).  A handle of its own.  n_blocks = entries of channels / kernel_sizes / dilations in
 * use (5 at `base`: one TDNN block, three SE-Res2Net blocks, the aggregation).  Tensor names are the module's own:
 *   blocks.0.{conv,norm}.*, blocks.{i}.tdnn1.{conv,norm}.*, blocks.{i}.res2net_block.blocks.{j}.{conv,norm}.*,
 *   blocks.{i}.tdnn2.{conv,norm}.*, blocks.{i}.se_block.conv{1,2}.*, mfa.{conv,norm}.*, asp.tdnn.{conv,norm}.*, asp.conv.*,
 *   asp_norm.*, fc.*; Conv1d weights [out][in][k].  Conv1d weights are held as fp16, everything else as fp32.
 * Limits (SC_ERR_INVALID from sc_prosody_encoder_load): channels[0 .. n_blocks-2] equal (no shortcut convolution) and a
 * multiple of 32, channels[n_blocks-1] = (n_blocks - 2) * channels[0], kernel 3 in the SE-Res2Net blocks and 1 in the
 * aggregation, a Res2Net chunk channels / res2net_scale of 32 or 64, res2net_scale 2..8, dilations 1..8, global_context = 1. */
#define SC_PE_MAX_BLOCKS 8
typedef struct sc_prosody_encoder_config {
    int32_t abi_version; /* must be SC_ABI_VERSION */
    int32_t input_dim, embed_dim, res2net_scale, se_channels, attention_channels, global_context, n_blocks;
    int32_t channels[SC_PE_MAX_BLOCKS], kernel_sizes[SC_PE_MAX_BLOCKS], dilations[SC_PE_MAX_BLOCKS];
} sc_prosody_encoder_config;
typedef struct sc_prosody_encoder sc_prosody_encoder;
sc_prosody_encoder* sc_prosody_encoder_load(const sc_tensor_desc* tensors, size_t n_tensors, const sc_prosody_encoder_config* cfg, int device);
void sc_prosody_encoder_free(sc_prosody_encoder* p);
/* ECAPA_TDNN.forward (ecapa_tdnn.py:111-143) on a padded batch: d_fbank [n][t_rows][input_dim] fp32 on the device,
 * h_lens_or_null [n] valid frames per item (NULL: every item has t_rows frames and no mask is applied, the reference's
 * padding_mask=None), d_out [n][embed_dim]: L2-normalised rows.  Rows of d_fbank behind an item's length are read as zeros; the
 * TDNN blocks then compute those frames like real ones, as the reference does on a zero-padded batch, so an item's result in a
 * ragged batch is the reference's padded-batch result, not the item's result alone.  d_gcmvn_mean_or_null / d_gcmvn_std_or_null
 * [input_dim] (both or neither): (x - mean) / std is applied to the frames in front of each length on the way in.
 * SC_ERR_INVALID, with nothing launched: a length outside 1..t_rows, t_rows above 4096, n outside 1..4096. */
int sc_prosody_encode(sc_prosody_encoder* p, const float* d_fbank, int32_t n, int32_t t_rows, const int32_t* h_lens_or_null,
                      const float* d_gcmvn_mean_or_null, const float* d_gcmvn_std_or_null, float* d_out);

/* ---- PRETSSEL acoustic model: units + prosody vector -> mel spectrogram (reference models/generator/vocoder.py:488-513, the first
 * half of PretsselVocoder.forward; the waveform generator behind it is sc_pretssel_wave below) ------------------------------
 * A handle of its own.  sc_pretssel_load takes the module's own state-dict names (the reference loader converts nothing):
 *   encoder_frontend.{embed_tokens.weight, pos_emb_alpha, embed_lang.weight}, {encoder,decoder}.layers.N.{self_attn.{q,k,v,output}_proj,
 *   self_attn_layer_norm, conv1d.conv{1,2}, conv1d_layer_norm, film.proj}.*, .film.{s_gamma,s_beta},
 *   decoder_frontend.variance_adaptor.{pitch,vuv,energy}_predictor.{conv{1,2}.0, ln{1,2}, proj, film.proj}.*, .film.{s_gamma,s_beta},
 *   decoder_frontend.variance_adaptor.embed_{pitch,energy}.*, decoder_frontend.pos_emb_alpha, final_proj.*,
 *   layers.{i}.0.{weight,bias}, layers.{i}.1.{weight,bias,running_mean,running_var} for the post_layers post-net blocks, and three
 *   tables the caller builds: pos_encoder.freqs [max_seq_len][model_dim] (sinusoidal, fairseq layout, first row = position
 *   pad_idx + 1), gcmvn_mean / gcmvn_std [mel_dim].  Other tensors (the prosody encoder, the waveform half) are ignored.
 * Limits (SC_ERR_INVALID from sc_pretssel_load): model_dim = heads * 128, at most 512; pred_hidden_dim a multiple of 64 up to 1024;
 * conv_inner_dim a multiple of 32 up to 8192; post_dim a multiple of 32 up to 4096; odd kernel sizes up to 31; 1..32 layers per
 * stack; post_layers 2..8; mel_dim a multiple of 4 up to 96. */
typedef struct sc_pretssel_config {
    int32_t abi_version; /* must be SC_ABI_VERSION */
    int32_t model_dim, num_heads, enc_layers, dec_layers, conv_inner_dim, conv_kernel;
    int32_t film_cond_dim, lang_embed_dim, num_langs; /* film_cond_dim = prosody vector + lang_embed_dim */
    int32_t pred_hidden_dim, pred_kernel;
    int32_t vocab_size, pad_idx, max_seq_len, mel_dim;
    int32_t post_layers, post_dim, post_kernel;
    float upsample_delta;
} sc_pretssel_config;
typedef struct sc_pretssel sc_pretssel;
sc_pretssel* sc_pretssel_load(const sc_tensor_desc* tensors, size_t n_tensors, const sc_pretssel_config* cfg, int device);
void sc_pretssel_free(sc_pretssel* p);
/* One packed pass over all items.  h_tokens / h_durations [n][s_tok] (host; tokens already offset and EOS-terminated, rows
 * padded behind h_tok_lens[i]), lang_index the row of embed_lang, d_prosody [n][film_cond_dim - lang_embed_dim] fp32 on the
 * device, d_mel [n][t_cap][mel_dim] fp32 on the device, h_frame_lens [n] (nullable) receives the frames of every item (the sum of
 * its durations).  Item i's frames are the reference's PADDED-BATCH result (the post-net sees final_proj's bias on the rows
 * between an item's end and the batch maximum); rows of d_mel behind an item's frames are zeros.
 * SC_ERR_INVALID, with nothing launched: an item without tokens or without frames, a negative duration, a token outside the
 * vocabulary, a token count or frame count + pad_idx + 1 above max_seq_len, frames above t_cap, lang_index outside the table. */
int sc_pretssel_mel(sc_pretssel* p, const int32_t* h_tokens, int32_t n, int32_t s_tok, const int32_t* h_tok_lens, const int32_t* h_durations,
                    int32_t lang_index, const float* d_prosody, float* d_mel, int32_t t_cap, int32_t* h_frame_lens_or_null);

/* ---- PRETSSEL waveform generator: mel spectrogram -> waveform (reference models/generator/vocoder.py:515-573, the second half of
 * PretsselVocoder.forward; added within ABI v10, purely additive) ----------------------------------------------------------
 * A handle of its own (sc_pretssel ignores these tensors).  sc_pretssel_wave_load takes the module's own names.  With P =
 * post_layers, U = num_upsamples and the 32 stream layers in four chunks of 8 at layers.{P, P+9, P+17+U, P+25+4U}:
 *   SConv: layers.N.conv.conv.{bias,weight_g,weight_v}; residual block: layers.N.block.{1,3}.conv.conv.*; transposed:
 *   layers.N.convtr.convtr.*; LSTM: layers.N.lstm.{weight,bias}_{ih,hh}_l{0,1}; conv_pre layers.{P+8}, ups layers.{P+17+i},
 *   conv_post layers.{P+33+4U}: .{bias,weight_g,weight_v}; HiFi-GAN ResBlocks layers.{P+25+U+j}.convs{1,2}.D.*; mean, scale.
 * Weight norm is folded at load.  Matrices and convolution weights are held as fp16, everything else as fp32.
 * Limits (SC_ERR_INVALID from sc_pretssel_wave_load, as are a missing tensor and a zero in `scale`): mel_dim a multiple of 4
 * up to 128; 1..8 upsamples with kernel = 2 * rate, upsample_initial_channel divisible by 2^U with at least 4 channels left;
 * 3 ResBlock kernels (odd) x 3 dilations, every stage on a kernel that takes packed items (C >= 128 a multiple of 32, or the
 * fused narrow-stage kernels); 4 ratios of 1..16; 16 * n_filters (the LSTM width) a multiple of 32 up to 2048; dimension 1..1024;
 * post_layers 0..64. */
typedef struct sc_pretssel_wave_config {
    int32_t abi_version; /* must be SC_ABI_VERSION */
    int32_t mel_dim, post_layers;
    int32_t upsample_initial_channel, num_upsamples;
    int32_t upsample_rates[SC_MAX_UPSAMPLES], upsample_kernel_sizes[SC_MAX_UPSAMPLES];
    int32_t resblock_kernel_sizes[3], resblock_dilation_sizes[3][3];
    int32_t n_filters, ratios[4], dimension; /* ratios in the decoder's order (the reference's [8, 5, 4, 2]) */
} sc_pretssel_wave_config;
typedef struct sc_pretssel_wave_model sc_pretssel_wave_model;
sc_pretssel_wave_model* sc_pretssel_wave_load(const sc_tensor_desc* tensors, size_t n_tensors, const sc_pretssel_wave_config* cfg, int device);
void sc_pretssel_wave_free(sc_pretssel_wave_model* p);
/* Every item by itself, as the reference loops: d_mel [n][t_cap][mel_dim] fp32 on the device (sc_pretssel_mel's output), of which
 * item i's first h_frame_lens[i] rows are used; d_wav [n][wav_cap] fp32 on the device receives frames * hop samples per item
 * (hop = the product of the upsample rates) and zeros behind them; h_wav_lens_or_null [n] the sample counts.  An item's samples do
 * not depend on its companions, to the bit.  The items are packed and go in groups of at most 2^22 samples (32 channels x 4 B per
 * sample and tensor at sample rate: 512 MB).  flags bit 0: the HiFi-GAN ResBlock products on two fp16 planes instead of the unit
 * vocoder's default (hi plane only).
 * SC_ERR_INVALID, with nothing launched: n outside 1..1024, an item without frames, frames above t_cap, frames * hop above
 * wav_cap or above 2^22. */
int sc_pretssel_wave(sc_pretssel_wave_model* p, const float* d_mel, int32_t n, int32_t t_cap, const int32_t* h_frame_lens, float* d_wav, int32_t wav_cap,
                     int32_t* h_wav_lens_or_null, int32_t flags);

/* ---- Audio resampling (added within ABI v10, purely additive): the windowed-sinc polyphase resampler the reference calls as
 * torchaudio.functional.resample in front of every model that opens a file (cli/m4t/predict/predict.py:226-231,
 * cli/expressivity/predict/predict.py:115, models/aligner/alignment_extractor.py:63-71).  A restatement of that algorithm, not
 * torchaudio itself (DESIGN.md section 7h has the definition).  With g = gcd(orig_freq, new_freq), orig = orig_freq / g,
 * new = new_freq / g: out_len = ceil(new * L / orig), y[f * new + p] = sum_k h[p][k] * x[f * orig + k - width] with x = 0 outside
 * [0, L); the bank h is built on the host in double, rounded to fp32 and cached per (orig, new, options); sums are fp32 in
 * ascending tap order, one output per thread, so a row's result does not depend on its companions, to the bit.
 * No handle: the resampler has no weights.  It runs on the CURRENT device, on the default stream (ordered behind the caller's
 * work there), and returns when the output is complete.
 *   d_in  [n][in_stride] fp32, row i valid up to h_in_len[i] (what lies behind is never read into a result)
 *   d_out [n][out_stride] fp32, row i holds h_out_len[i] samples and zeros up to out_stride; must not overlap d_in
 *   opts  NULL or all-zero: lowpass_filter_width 6, rolloff 0.99, hann.  Otherwise abi_version must be SC_ABI_VERSION and every
 *         field is taken as given, except that beta == 0 is the default 14.769656459379492 and that rolloff / beta equal to
 *         their default rounded to fp32 stand for the default in double (the bank is built in double).
 * orig == new is a row copy.  SC_ERR_INVALID, before any device work: a null pointer, rates <= 0, orig or new above 1024 after
 * reduction, a bank (new x taps per phase x 4 bytes) above 64 KB, lowpass_filter_width < 1, rolloff outside (0, 1], an unknown
 * method, n outside 1..65535, a length above in_stride, out_stride below the longest out_len, overlapping buffers.
 * sc_resample_len: out_len of num_samples samples (host only; negative on rates <= 0 or a negative length). */
typedef struct sc_resample_opts {
    int32_t abi_version;
    int32_t lowpass_filter_width;
    float rolloff;
    int32_t method; /* 0 hann (sinc_interp_hann), 1 kaiser (sinc_interp_kaiser) */
    float beta;     /* kaiser only */
} sc_resample_opts;
int64_t sc_resample_len(int64_t num_samples, int32_t orig_freq, int32_t new_freq);
int sc_resample(const float* d_in, int32_t n, int64_t in_stride, const int64_t* h_in_len, int32_t orig_freq, int32_t new_freq,
                const sc_resample_opts* opts, float* d_out, int64_t out_stride, int64_t* h_out_len);

/* ---- Timeline mix (added within ABI v10, purely additive; an extension for long-form speech translation, no reference
 * counterpart): n waveforms placed at absolute sample offsets in one track of T samples, with linear fades
 * at their edges, over an optional bed that is attenuated where a segment sounds.  No handle, current device, default stream,
 * returns when d_out is complete (the conventions of sc_resample).
 *   d_seg [n][seg_stride] fp32, row i valid up to h_len[i];  h_start [n] ascending, segment i covers [h_start[i], h_start[i] + h_len[i])
 *   w_i(k) = min(1, min(k + 1, L_i - k) / (fade + 1));  c(t) = max_i clamp(1 - dist_i(t) / (ramp + 1), 0, 1), dist_i(t) the
 *   distance in samples from t to segment i (0 inside; an empty segment covers nothing)
 *   d_out[t] = sum over the segments covering t, ascending i, of h_gain[i] * w_i(t - p_i) * seg_i[t - p_i]
 *              + d_bed[t] * (1 - (1 - duck) * c(t))            (the bed term last; absent when d_bed is NULL)
 * in fp32, the exact operation order in k_dub.hip's header.  Overlaps of any depth are legal; every sample of d_out[0, T) is
 * written (+0.0 where nothing sounds and there is no bed).  SC_ERR_INVALID before any device work: a null pointer, starts not
 * ascending or negative, a segment past T or longer than seg_stride, duck outside [0, 1], fade or ramp outside 0..2^20, a gain
 * that is not finite. */
int sc_mix_timeline(const float* d_seg, int32_t n, int64_t seg_stride, const int32_t* h_len, const int64_t* h_start,
                    const float* h_gain, int32_t fade, const float* d_bed /* nullable [T] */, float duck, int32_t ramp, float* d_out,
                    int64_t T);

/* ---- Time-scale modification (added within ABI v10, purely additive; an extension of this project, no reference counterpart;
 * DESIGN.md section 7w): row i of L = h_in_len[i] samples becomes Lo = h_out_len[i] samples at the same pitch, by a
 * waveform-similarity overlap-add (WSOLA).  No handle, current device, default stream, returns when d_out is complete (the
 * conventions of sc_resample).  With N = frame (even, 64..2048), Hs = N / 2, D = radius (0..Hs), x = +0 outside [0, L):
 *   q[i]   = clamp(rint(x[i] * 2^(14 - e)), -32767, 32767), e = floor(log2(max |x| over the finite samples)); 0 for a sample that is
 *            not finite, and everywhere when no sample is finite or the maximum lies below 2^-100      (for the search only)
 *   M      = ceil(Lo / Hs) + 1 frames; a_m = floor(m * Hs * L / Lo); c_0 = 0; c_m = a_m + d_m, where d_m in [-D, D] minimises
 *            SAD(d) = sum_{k < N} |q[c_{m-1} + k] - q[a_m + d - Hs + k]| in integers; ties: the smallest |d|, then the negative one
 *   y[t]   = w[k + Hs] * x[c_m + k] + w[k] * x[c_{m+1} - Hs + k], m = t / Hs, k = t - m * Hs, w[k] = 0.5 - 0.5 cos(2 pi k / N) built
 *            in double on the host and rounded to fp32; two fp32 products and one fp32 sum, the order in k_tsm.hip's header
 * Lo == L is a copy of the row's bits.  Only d_out[i][0, Lo) is written.  An item's result does not depend on its companions, to
 * the bit.
 *   opts  NULL or all-zero: frame 512, radius 160.  Otherwise abi_version must be SC_ABI_VERSION; a zero field stands for its
 *         default, radius -1 for D = 0 (no search: plain overlap-add).
 * SC_ERR_INVALID, before any device work: a null pointer, n outside 1..65535, a length that is negative or above its stride, L above
 * 2^30, L == 0 with Lo != 0, L > 0 with Lo < 1, Lo > 4 L or L > 4 Lo, a frame that is odd or outside 64..2048, a radius above
 * frame / 2, overlapping buffers. */
typedef struct sc_tsm_opts {
    int32_t abi_version;
    int32_t frame;  /* N, samples; 0: 512 */
    int32_t radius; /* D, samples; 0: 160, -1: none */
} sc_tsm_opts;
int sc_time_stretch(const float* d_in, int32_t n, int64_t in_stride, const int64_t* h_in_len, const sc_tsm_opts* opts /* nullable */,
                    float* d_out, int64_t out_stride, const int64_t* h_out_len);

/* ---- Speech detection (added within ABI v10, purely additive): a speech probability per window of `window` samples, the track
 * the reference takes from Silero VAD (segment/silero_vad.py get_speech_probs) in front of its segmentation of long input.  NOT a
 * learned model: an energy detector whose threshold adapts to the row (DESIGN.md section 7m has the definition; its constants are
 * this project's choice and their quality on real speech has not been measured).  For a row x[0..L), n_w = ceil(L / window):
 *   db_w = 10 log10(max(e_w, 1e-10)), e_w the variance of window w zero-padded to `window` (two passes in fp32, fixed order);
 *          NaN for a window that holds a non-finite sample (or whose fp32 energy is not finite)
 *   F_q, P = the order statistics floor(floor_quantile (k-1)) and floor(peak_quantile (k-1)) of the k finite db_w (exact, no
 *          interpolation), F = min(F_q, noise_ceiling_db), c = F + max(min_margin_db, range_fraction (P - F))
 *   s_w  = the largest finite db within `hangover` windows of w;  p_w = 1 / (1 + exp(-(s_w - c) / slope_db)), NaN where db_w is
 * No handle: it runs on the CURRENT device, on the default stream, and returns when the output is complete.  A row's bits do not
 * depend on its companions or on the strides.
 *   d_wav   [n][wav_stride] fp32, row i valid up to h_num_samples[i]
 *   d_probs [n][probs_stride] fp32: n_w probabilities, zeros behind them
 *   d_db    NULL, or [n][probs_stride] fp32: db_w, zeros behind them
 *   h_stats NULL, or [n][4] fp32 on the host: F, P, c, k (all NaN but k = 0 for a row without a finite window)
 *   opts    NULL or all-zero: the defaults below.  Otherwise abi_version must be SC_ABI_VERSION and a zero field stands for its
 *           default; hangover -1 is no hangover.  The quantiles equal to their default rounded to fp32 stand for it in double.
 * SC_ERR_INVALID, before any device work: a null pointer, window outside 32..8192, n outside 1..65535, a negative length, a length
 * above wav_stride, more than 2^20 windows in a row, probs_stride below the most windows of a row, a quantile outside [0, 1],
 * slope_db <= 0, min_margin_db < 0, range_fraction < 0, hangover outside -1..8, a field that is not a number.
 * sc_vad_windows: ceil(num_samples / window) (host only; negative on a negative length or window <= 0). */
typedef struct sc_vad_opts {
    int32_t abi_version;
    int32_t hangover;       /* windows each side, 0..8, default 1; -1: none */
    float floor_quantile;   /* 0.10 */
    float peak_quantile;    /* 0.95 */
    float noise_ceiling_db; /* -45 */
    float min_margin_db;    /* 6 */
    float range_fraction;   /* 0.35 */
    float slope_db;         /* 1.5 */
} sc_vad_opts;
int64_t sc_vad_windows(int64_t num_samples, int32_t window);
int sc_vad_probs(const float* d_wav, int32_t n, int64_t wav_stride, const int64_t* h_num_samples, int32_t window, const sc_vad_opts* opts,
                 float* d_probs, int64_t probs_stride, float* d_db, float* h_stats);

/* ---- Streaming speech detection (added within ABI v10, purely additive): the detector above made CAUSAL, for endless streams.
 * sc_vad_probs takes its threshold from the whole recording; here a lane (one per session) keeps the levels of its last
 * H = history_windows windows on the device and a window's probability depends on the lane's windows up to it only.  NOT a learned
 * model, and NOT the reference's Silero VAD: an energy detector whose constants are this project's choice and whose quality on real
 * speech has not been measured.  For window t (0-based since the lane's reset) of `window` samples:
 *   db_t as db_w above (whole windows only: nothing is zero-padded)
 *   S_t  = the finite db_u for max(0, t-H+1) <= u <= t, k = |S_t|, d(0) <= ... <= d(k-1) its sorted values
 *   F_q = d(floor(floor_quantile (k-1))), P = d(floor(peak_quantile (k-1))) (ranks in double, exact order statistics),
 *   F = min(F_q, noise_ceiling_db) (no warm-up: a stream that opens with speech has F = noise_ceiling_db and is speech),
 *   c = F + max(min_margin_db, range_fraction (P - F))
 *   s_t = the largest finite db of windows t-hangover .. t (BACKWARDS only, clipped at the reset)
 *   p_t = 1 / (1 + exp(-(s_t - c) / slope_db)); NaN where db_t is NaN (such a window enters neither S nor a later s) or k = 0
 * How a stream is cut into pushes, who else is in a push and the strides change no bit.
 * sc_vad_stream_create: host only - device memory is taken on the CURRENT device by the first reset or push, and every later call
 *   must run on that device.  Work runs on the default stream; reset and push return when their results are complete.
 *   opts NULL or all-zero: the defaults; otherwise abi_version must be SC_ABI_VERSION, the detector fields follow sc_vad_opts' rules
 *   and history_windows is 1..1024 (0: 312, 10 s of 512-sample windows at 16 kHz).
 * sc_vad_stream_reset: the n named lanes start over (t = 0, empty history).  A new handle's lanes are fresh.
 * sc_vad_stream_push: n >= 0 distinct lanes in one call (two kernel launches whatever n is); named lane i reads
 *   d_wav[i * wav_stride .. + h_num_samples[i]) and handles floor(h_num_samples[i] / window) whole windows; the samples behind
 *   them are ignored (not kept for the next push).
 *   d_probs [n][probs_stride] fp32: the windows' probabilities; nothing is written behind them
 *   d_db    NULL, or [n][probs_stride] fp32: db_t of the windows handled
 *   h_stats NULL, or [n][5] fp32 on the host: F, P, c, k of the lane's last window (of an earlier push if this one held none; NaN,
 *           NaN, NaN, 0 before the first) and the number of windows handled
 * SC_ERR_INVALID, before any device work: sessions outside 1..65535, window outside 1..8192, a null pointer, more lanes than
 * sessions, a lane outside 0..sessions-1 or named twice, a negative length, a length above wav_stride, more than 2^20 windows of a
 * lane in one push, probs_stride below the most windows of a lane, and the option errors of sc_vad_probs. */
typedef struct sc_vad_stream sc_vad_stream;
typedef struct sc_vad_stream_opts {
    int32_t abi_version;
    int32_t hangover;       /* windows BACK, 0..8, default 1; -1: none */
    float floor_quantile;   /* 0.10 */
    float peak_quantile;    /* 0.95 */
    float noise_ceiling_db; /* -45 */
    float min_margin_db;    /* 6 */
    float range_fraction;   /* 0.35 */
    float slope_db;         /* 1.5 */
    int32_t history_windows; /* H, 1..1024, default 312 */
} sc_vad_stream_opts;
int sc_vad_stream_create(int32_t sessions, int32_t window, const sc_vad_stream_opts* opts, sc_vad_stream** out);
void sc_vad_stream_destroy(sc_vad_stream* h);
int sc_vad_stream_reset(sc_vad_stream* h, const int32_t* h_lanes, int32_t n);
int sc_vad_stream_push(sc_vad_stream* h, const int32_t* h_lanes, int32_t n, const float* d_wav, int64_t wav_stride, const int64_t* h_num_samples,
                       float* d_probs, int64_t probs_stride, float* d_db, float* h_stats);

/* ---- Minimum-Bayes-risk selection (added within ABI v10, purely additive): of the hypotheses sampled for an utterance
 * (sc_generate_text_sampled), the one with the highest expected utility against all of them.  An extension without a counterpart
 * in the reference; the utility is this project's "token n-gram F-score" (DESIGN.md section 7o has the definition; it has not
 * been evaluated on real translations).  For a hypothesis h and a pseudo-reference r (int32 token ids) and n = 1..max_order:
 *   m_n = sum over n-grams g of min(count of g in h, count of g in r), H_n = max(|h| - n + 1, 0), R_n = max(|r| - n + 1, 0);
 *   over the E orders with H_n > 0 and R_n > 0 (ascending n): P = (sum m_n / H_n) / E, R = (sum m_n / R_n) / E;
 *   U(h, r) = (1 + beta^2) P R / (beta^2 P + R), 0 where E = 0 or the denominator is 0; all of it in double.
 *   expected_i = (sum_j w_j U(h_i, h_j)) / (sum_j w_j) over ascending j, j = i included; best = the lowest i with the largest
 *   expected_i.  n-grams are compared as token tuples (exact for every non-negative int32 id); every sum has a fixed order, so
 *   an utterance's bits do not depend on its companions and equal hypotheses get equal values.
 * No handle: it runs on the CURRENT device, on the default stream, and returns when the outputs are complete.  All pointers are
 * HOST memory (the ids are on the host for detokenisation anyway).
 *   typedef struct sc_mbr_opts { int32_t abi_version; int32_t max_order; float beta; int32_t reserved; } sc_mbr_opts;
 *   int sc_mbr_select(const int32_t* h_ids,           [n][hyp_stride][len_stride]
 *                     int32_t n, int32_t hyp_stride, int32_t len_stride,
 *                     const int32_t* h_num_hyps,      [n], 1..hyp_stride
 *                     const int32_t* h_lens,          [n][hyp_stride], 0..len_stride
 *                     const float* h_weights_or_null, [n][hyp_stride]; NULL: every weight 1
 *                     const sc_mbr_opts* opts,        NULL or all-zero = defaults (max_order 4, beta 1)
 *                     double* h_expected,             [n][hyp_stride], 0 behind num_hyps
 *                     int32_t* h_best,                [n]
 *                     double* h_utility_or_null,      [n][hyp_stride][hyp_stride]: U(h_i, h_j), 0 behind num_hyps
 *                     int32_t* h_match_or_null);      [n][hyp_stride][hyp_stride][4]: m_1..m_4, 0 for orders above max_order
 *   opts: otherwise abi_version must be SC_ABI_VERSION; max_order 0 and beta 0 stand for their defaults; beta is used as
 *         (double)beta.
 * SC_ERR_INVALID, before any device work: a null required pointer, n outside 1..4096, hyp_stride outside 1..128, len_stride
 * outside 1..1024, a count outside 1..hyp_stride, a length outside 0..len_stride, a negative token, max_order outside 0..4, a
 * beta that is negative or not finite, a weight that is negative or not finite, an utterance whose weights sum to 0. */
typedef struct sc_mbr_opts {
    int32_t abi_version;
    int32_t max_order; /* 1..4, default 4 */
    float beta;        /* recall counts beta times as much as precision; default 1 */
    int32_t reserved;
} sc_mbr_opts;
int sc_mbr_select(const int32_t* h_ids, int32_t n, int32_t hyp_stride, int32_t len_stride, const int32_t* h_num_hyps, const int32_t* h_lens,
                  const float* h_weights_or_null, const sc_mbr_opts* opts, double* h_expected, int32_t* h_best, double* h_utility_or_null,
                  int32_t* h_match_or_null);

/* ---- Quality metrics: the two device primitives (added within ABI v10, purely additive).  BLEU, chrF / chrF++
 * and chrF as an MBR utility are sums of clipped n-gram matches, WER / CER are sums of edit distances; the strings, the tokenizers and
 * the score formulas are host work (seamless_communication_amd/metrics.py).  Both entries work on a POOL of int32 symbol sequences
 * (character code points, interned word ids) and a PAIR LIST into it:
 *   h_symbols  the sequences one behind the other; every symbol >= 0.  May be NULL when the pool holds no symbol.
 *   h_offsets  [n_seq + 1] int64: sequence s is h_symbols[h_offsets[s] .. h_offsets[s + 1]); h_offsets[0] = 0, never decreasing
 *   h_pairs    [n_pairs][2] int32: (a, b), both in 0..n_seq-1; a = b is allowed, and any number of pairs may name a sequence
 * No handle: they run on the CURRENT device, on the default stream, and return when the output is complete.  All pointers are HOST
 * memory.  n_pairs = 0 is allowed and does nothing.  A pair's result depends on its two sequences only.
 *
 * sc_ngram_match: h_match [n_pairs][6] int32.  For the pair (a, b) and n = 1..max_order,
 *   h_match[p][n - 1] = sum over the distinct n-grams g of a of min(count of g in a, count of g in b);
 *   the columns of the orders above max_order are 0.  Every column of every pair is written.
 *   n-grams are compared as symbol tuples (exact for every non-negative int32 symbol).  A sequence holds 0..4096 symbols; each
 *   sequence that a pair names is sorted once per launch set (a call is one launch set up to 2^21 symbols of named sequences and
 *   2^20 pairs), and pairs that follow each other's first sequence share its staged row.
 * SC_ERR_INVALID, before any device work: a null required pointer, n_seq < 1, n_pairs outside 0..2^31-1, offsets that do not
 * start at 0 or decrease, a negative symbol, a pair index outside 0..n_seq-1, max_order outside 1..6, a sequence of more than 4096
 * symbols (whether a pair names it or not).
 *
 * sc_edit_distance: h_dist [n_pairs] int32: the Levenshtein distance of a and b with unit costs (substitution, insertion and
 *   deletion 1 each); an empty side gives the other side's length.  The SHORTER sequence of a pair holds at most 8192 symbols, the
 *   longer one at most 2^20 = 1048576.
 * SC_ERR_INVALID, before any device work: as above, and a pair whose shorter side exceeds 8192 or whose longer side exceeds 2^20
 * (the message names the limit). */
int sc_ngram_match(const int32_t* h_symbols, const int64_t* h_offsets, int32_t n_seq, const int32_t* h_pairs, int64_t n_pairs, int32_t max_order,
                   int32_t* h_match);
int sc_edit_distance(const int32_t* h_symbols, const int64_t* h_offsets, int32_t n_seq, const int32_t* h_pairs, int64_t n_pairs, int32_t* h_dist);

/* The kernel-level test hooks (sc_op_*) and the dispatch introspection the parity tests drive are exported too but are NOT part
 * of the drop-in boundary: include/seamless_hip_internal.h. */

#ifdef __cplusplus
}
#endif
#endif /* SEAMLESS_HIP_H_ */
