// PRETSSEL acoustic model: units + prosody vector -> mel spectrogram, the first half of PretsselVocoder.forward.  A handle of
// its own (separate checkpoint, stream and scratch pool) and its C entries, after the pattern of model_ecapa.hip.
//
// Reference call sites (src/seamless_communication/models/...):
//   generator/vocoder.py:96-121    PretsselEncoderFrontend.forward;  :147-162 PretsselDecoderFrontend.forward
//   generator/vocoder.py:488-513   PretsselVocoder.forward up to gcmvn_denormalize
//   unity/fft_decoder_layer.py     FeedForwardTransformerLayer (POST norm, FiLM behind the second LayerNorm);  unity/film.py
//   unity/length_regulator.py      VariancePredictor :172-218, VarianceAdaptor :275-321, GaussianUpsampling :42-96
//
// One packed pass over all items, as the NAR T2U decoder of model_t2u.hip: the tokens of all items back to back for the
// encoder and the variance adaptor, the frames back to back for the decoder.  No padded row exists, so every "mask" of the
// reference is the packed geometry itself: the attention takes the items' row offsets, the convolutions the {position, length}
// of every row.  The post-net is the one stage that is NOT independent of the batch: the reference runs it on the padded batch
// without a mask, where the rows between an item's end and the batch maximum hold final_proj's bias.  It therefore runs on
// EXTENDED rows: every item's frames followed by min(post-net reach, T_max - len) halo rows that hold the bias.
#include <algorithm>
#include <cmath>
#include <string>

#include "handle.h"
#include "loader.h"

using namespace sc;

namespace {
struct Film {
    int off = 0;  // column of gamma' in the per-item FiLM table
};
struct PretsselLayer {
    FFTLayer fft;
    Film film;
};
struct BnFold {
    const float* scale = nullptr;
    const float* shift = nullptr;
};
}  // namespace

struct sc_pretssel {
    Model m;
    sc_pretssel_config cfg{};
    const __half* embed = nullptr;  // [vocab][M]
    const float* lang = nullptr;    // [langs][Lg]
    const float* pos = nullptr;     // [max_seq_len][M], row t = position t + pad_idx + 1
    float alpha_enc = 1.f, alpha_dec = 1.f;
    std::vector<PretsselLayer> enc, dec;
    // every FiLM projection stacked: encoder layers, decoder layers, then the pitch / voiced / energy predictors
    const __half* film_w = nullptr;  // [film_n][cond]
    const float* film_b = nullptr;
    const float* film_mul = nullptr;
    const float* film_add = nullptr;
    int film_n = 0, film_pred_off = 0;
    // variance adaptor: predictors in the order pitch, voiced / unvoiced, energy
    Conv pred_c1;     // the three first convolutions stacked: [3H][k * M]
    Conv pred_c2[3];  // [H][k * H]
    const float* pred_ln1_g = nullptr;  // [3][H]
    const float* pred_ln1_b = nullptr;
    const float* pred_ln2_g = nullptr;
    const float* pred_ln2_b = nullptr;
    const float* pred_pw = nullptr;  // [3][H]
    const float* pred_pb = nullptr;  // [3]
    const float* emb_pitch_w = nullptr;
    const float* emb_pitch_b = nullptr;
    const float* emb_energy_w = nullptr;
    const float* emb_energy_b = nullptr;
    Linear proj;  // final_proj [mel][M]
    std::vector<Conv> post;  // post[0].cin is mel_dim padded to a multiple of 32
    std::vector<BnFold> post_bn;
    const float* gmean = nullptr;
    const float* gstd = nullptr;
    int mel_pad = 0;
    int last_launches = 0;
};

namespace {

constexpr int PRETSSEL_MAX_ITEMS = 1024;

void check_config(const sc_pretssel_config& c) {
    SC_CHECK(c.num_heads >= 1 && c.model_dim == c.num_heads * 128, "sc_pretssel_load: model_dim=%d with %d heads: only head dimension 128 is built", c.model_dim,
             c.num_heads);
    SC_CHECK(pretssel_ln_supported(c.model_dim) && c.model_dim <= 64 * PRETSSEL_UPS_VPL, "sc_pretssel_load: model_dim=%d must be a multiple of 64 up to %d",
             c.model_dim, 64 * PRETSSEL_UPS_VPL);
    SC_CHECK(c.conv_inner_dim >= 32 && c.conv_inner_dim % 32 == 0 && c.conv_inner_dim <= 8192, "sc_pretssel_load: conv_inner_dim=%d must be a multiple of 32",
             c.conv_inner_dim);
    SC_CHECK(pretssel_ln_supported(c.pred_hidden_dim), "sc_pretssel_load: pred_hidden_dim=%d must be a multiple of 64 up to 1024", c.pred_hidden_dim);
    SC_CHECK(c.conv_kernel >= 1 && c.conv_kernel % 2 == 1 && c.conv_kernel <= 31 && c.pred_kernel >= 1 && c.pred_kernel % 2 == 1 && c.pred_kernel <= 31 &&
                 c.post_kernel >= 1 && c.post_kernel % 2 == 1 && c.post_kernel <= 31,
             "sc_pretssel_load: kernel sizes %d / %d / %d must be odd ('same' padding) and at most 31", c.conv_kernel, c.pred_kernel, c.post_kernel);
    SC_CHECK(c.enc_layers >= 1 && c.enc_layers <= 32 && c.dec_layers >= 1 && c.dec_layers <= 32, "sc_pretssel_load: %d + %d layers outside 1..32", c.enc_layers,
             c.dec_layers);
    SC_CHECK(c.lang_embed_dim >= 1 && c.film_cond_dim > c.lang_embed_dim && c.film_cond_dim <= 8192 && c.num_langs >= 1,
             "sc_pretssel_load: film_cond_dim=%d lang_embed_dim=%d num_langs=%d", c.film_cond_dim, c.lang_embed_dim, c.num_langs);
    SC_CHECK(c.vocab_size >= 2 && c.pad_idx >= 0 && c.pad_idx < c.vocab_size && c.max_seq_len > c.pad_idx + 1 && c.max_seq_len <= (1 << 20),
             "sc_pretssel_load: vocab_size=%d pad_idx=%d max_seq_len=%d", c.vocab_size, c.pad_idx, c.max_seq_len);
    SC_CHECK(c.mel_dim >= 4 && c.mel_dim % 4 == 0 && c.mel_dim <= 96, "sc_pretssel_load: mel_dim=%d must be a multiple of 4 up to 96", c.mel_dim);
    SC_CHECK(c.post_layers >= 2 && c.post_layers <= 8 && c.post_dim >= 32 && c.post_dim % 32 == 0 && c.post_dim <= 4096,
             "sc_pretssel_load: post-net of %d layers (2..8) at %d channels (a multiple of 32)", c.post_layers, c.post_dim);
    SC_CHECK(c.upsample_delta > 0.f && c.upsample_delta <= 10.f, "sc_pretssel_load: upsample_delta=%g outside (0, 10]", (double)c.upsample_delta);
}

void load_pretssel(sc_pretssel& a, const sc_tensor_desc* t, size_t n) {
    const sc_pretssel_config& c = a.cfg;
    check_config(c);
    const int M = c.model_dim, Ci = c.conv_inner_dim, H = c.pred_hidden_dim, D = c.film_cond_dim, K = c.conv_kernel, PK = c.pred_kernel;
    Loader L(a.m, "sc_pretssel_load", t, n);
    a.embed = L.f16("encoder_frontend.embed_tokens.weight", {c.vocab_size, M});
    a.lang = L.f32("encoder_frontend.embed_lang.weight", {c.num_langs, c.lang_embed_dim});
    a.pos = L.f32("pos_encoder.freqs", {c.max_seq_len, M});
    a.alpha_enc = L.scalar("encoder_frontend.pos_emb_alpha");
    a.alpha_dec = L.scalar("decoder_frontend.pos_emb_alpha");
    // ---- FiLM table ----
    a.film_pred_off = (c.enc_layers + c.dec_layers) * 2 * M;
    a.film_n = a.film_pred_off + 3 * 2 * H;
    __half* fw = static_cast<__half*>(L.dalloc((size_t)a.film_n * D * 2));
    float* fb = static_cast<float*>(L.dalloc((size_t)a.film_n * 4));
    std::vector<float> mul((size_t)a.film_n), add((size_t)a.film_n);
    auto film = [&](const std::string& p, int off, int C) {
        L.f16_into(p + ".proj.weight", {2 * C, D}, fw + (size_t)off * D);
        L.f32_into(p + ".proj.bias", {2 * C}, fb + off);
        const float sg = L.scalar(p + ".s_gamma"), sb = L.scalar(p + ".s_beta");
        for (int j = 0; j < C; ++j) {
            mul[(size_t)off + j] = sg;
            add[(size_t)off + j] = 1.f;
            mul[(size_t)off + C + j] = sb;
            add[(size_t)off + C + j] = 0.f;
        }
    };
    // ---- FFT layers ----
    auto layer = [&](const std::string& p, int off) {
        PretsselLayer l;
        l.fft.qkv = L.fuse({p + ".self_attn.q_proj", p + ".self_attn.k_proj", p + ".self_attn.v_proj"}, M, M);
        l.fft.attn_out = L.lin(p + ".self_attn.output_proj", M, M);
        l.fft.attn_ln = L.ln(p + ".self_attn_layer_norm", M);
        l.fft.conv1 = L.conv(p + ".conv1d.conv1", Ci, M, K);
        l.fft.conv2 = L.conv(p + ".conv1d.conv2", M, Ci, K);
        l.fft.conv_ln = L.ln(p + ".conv1d_layer_norm", M);
        l.film.off = off;
        film(p + ".film", off, M);
        return l;
    };
    for (int i = 0; i < c.enc_layers; ++i) a.enc.push_back(layer("encoder.layers." + std::to_string(i), i * 2 * M));
    for (int i = 0; i < c.dec_layers; ++i) a.dec.push_back(layer("decoder.layers." + std::to_string(i), (c.enc_layers + i) * 2 * M));
    // ---- variance adaptor ----
    const std::string va = "decoder_frontend.variance_adaptor.";
    const char* preds[3] = {"pitch_predictor", "vuv_predictor", "energy_predictor"};
    {
        Conv& s = a.pred_c1;
        s.cout = 3 * H;
        s.cin = M;
        s.k = PK;
        s.kpad = M * PK;
        __half* w = static_cast<__half*>(L.dalloc((size_t)3 * H * s.kpad * 2));
        float* b = static_cast<float*>(L.dalloc((size_t)3 * H * 4));
        float* g1 = static_cast<float*>(L.dalloc((size_t)3 * H * 4));
        float* b1 = static_cast<float*>(L.dalloc((size_t)3 * H * 4));
        float* g2 = static_cast<float*>(L.dalloc((size_t)3 * H * 4));
        float* b2 = static_cast<float*>(L.dalloc((size_t)3 * H * 4));
        float* pw = static_cast<float*>(L.dalloc((size_t)3 * H * 4));
        float* pb = static_cast<float*>(L.dalloc(3 * 4));
        for (int j = 0; j < 3; ++j) {
            const std::string p = va + preds[j];
            L.pack_conv(p + ".conv1.0.weight", H, M, PK, M, s.kpad, w + (size_t)j * H * s.kpad);
            L.f32_into(p + ".conv1.0.bias", {H}, b + (size_t)j * H);
            a.pred_c2[j] = L.conv(p + ".conv2.0", H, H, PK);
            L.f32_into(p + ".ln1.weight", {H}, g1 + (size_t)j * H);
            L.f32_into(p + ".ln1.bias", {H}, b1 + (size_t)j * H);
            L.f32_into(p + ".ln2.weight", {H}, g2 + (size_t)j * H);
            L.f32_into(p + ".ln2.bias", {H}, b2 + (size_t)j * H);
            L.f32_into(p + ".proj.weight", {1, H}, pw + (size_t)j * H);
            L.f32_into(p + ".proj.bias", {1}, pb + j);
            film(p + ".film", a.film_pred_off + j * 2 * H, H);
        }
        s.w = w;
        s.b = b;
        a.pred_ln1_g = g1;
        a.pred_ln1_b = b1;
        a.pred_ln2_g = g2;
        a.pred_ln2_b = b2;
        a.pred_pw = pw;
        a.pred_pb = pb;
    }
    a.emb_pitch_w = L.f32(va + "embed_pitch.weight", {M, 1, 1});
    a.emb_pitch_b = L.f32(va + "embed_pitch.bias", {M});
    a.emb_energy_w = L.f32(va + "embed_energy.weight", {M, 1, 1});
    a.emb_energy_b = L.f32(va + "embed_energy.bias", {M});
    float* fm = static_cast<float*>(L.dalloc((size_t)a.film_n * 4));
    float* fa = static_cast<float*>(L.dalloc((size_t)a.film_n * 4));
    SC_HIP(hipMemcpy(fm, mul.data(), (size_t)a.film_n * 4, hipMemcpyHostToDevice));
    SC_HIP(hipMemcpy(fa, add.data(), (size_t)a.film_n * 4, hipMemcpyHostToDevice));
    a.film_w = fw;
    a.film_b = fb;
    a.film_mul = fm;
    a.film_add = fa;
    // ---- projection, post-net, gcmvn ----
    a.proj = L.lin("final_proj", c.mel_dim, M);
    a.mel_pad = (int)align_up(c.mel_dim, 32);
    for (int i = 0; i < c.post_layers; ++i) {
        const std::string p = "layers." + std::to_string(i);
        const int cin = i == 0 ? c.mel_dim : c.post_dim, cout = i == c.post_layers - 1 ? c.mel_dim : c.post_dim;
        a.post.push_back(L.conv(p + ".0", cout, cin, c.post_kernel, /*bias=*/true, i == 0 ? a.mel_pad : cin));
        const float* g = L.f32(p + ".1.weight", {cout}, /*keep=*/false);
        const float* b = L.f32(p + ".1.bias", {cout}, /*keep=*/false);
        const float* mu = L.f32(p + ".1.running_mean", {cout}, /*keep=*/false);
        const float* var = L.f32(p + ".1.running_var", {cout}, /*keep=*/false);
        float* scale = static_cast<float*>(L.dalloc((size_t)cout * 4));
        float* shift = static_cast<float*>(L.dalloc((size_t)cout * 4));
        launch_bn_fold(g, b, mu, var, 1e-5f, cout, scale, shift, a.m.stream);
        a.post_bn.push_back(BnFold{scale, shift});
    }
    a.gmean = L.f32("gcmvn_mean", {c.mel_dim});
    a.gstd = L.f32("gcmvn_std", {c.mel_dim});
    L.release_unused();
}

template <typename T>
Buf<T> to_device(Model& m, const std::vector<T>& h) {
    Buf<T> d(m.pp(), std::max<size_t>(h.size(), 1));
    if (!h.empty()) SC_HIP(hipMemcpyAsync(d.get(), h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, m.stream));
    return d;
}

// Post-net + de-normalisation on the packed projection rows d_proj [sum lens][mel]; lens: frames of every item (host)
void run_postnet(sc_pretssel& a, const float* d_proj, int n, const int32_t* lens, float* d_mel, int t_cap) {
    Model& m = a.m;
    const sc_pretssel_config& c = a.cfg;
    const int mel = c.mel_dim, reach = c.post_layers * (c.post_kernel / 2);
    int tmax = 0;
    for (int i = 0; i < n; ++i) tmax = std::max(tmax, lens[i]);
    std::vector<int> frame_off((size_t)n + 1, 0), ext_item, ext_pos;
    for (int i = 0; i < n; ++i) {
        frame_off[(size_t)i + 1] = frame_off[i] + lens[i];
        const int ext = lens[i] + std::min(reach, tmax - lens[i]);
        for (int t = 0; t < ext; ++t) {
            ext_item.push_back(i);
            ext_pos.push_back(t);
            ext_pos.push_back(ext);
        }
    }
    const int Re = (int)ext_item.size();
    Buf<int> d_frame_off = to_device(m, frame_off), d_ext_item = to_device(m, ext_item), d_ext_pos = to_device(m, ext_pos);
    const int2* d_pos2 = reinterpret_cast<const int2*>(d_ext_pos.get());
    const int P = std::max(c.post_dim, a.mel_pad);
    Buf<__half> planes(m.pp(), (size_t)4 * Re * P);
    __half* ah = planes.get();
    __half* al = ah + (size_t)Re * P;
    __half* bh = al + (size_t)Re * P;
    __half* bl = bh + (size_t)Re * P;
    Buf<float> cb(m.pp(), (size_t)Re * P);
    SC_HIP(hipMemsetAsync(d_mel, 0, (size_t)n * t_cap * mel * 4, m.stream));
    launch_pretssel_postnet_in(d_proj, a.proj.b, d_ext_item, d_pos2, d_frame_off, Re, mel, a.mel_pad, ah, al, m.stream);
    ++a.last_launches;
    for (int l = 0; l < c.post_layers; ++l) {
        const Conv& cv = a.post[l];
        conv1d_presplit(m, ah, al, cv, nullptr, cb, nullptr, nullptr, 0, 0, c.post_kernel / 2, 1, nullptr, ACT_NONE, Re, d_pos2);
        if (l + 1 < c.post_layers) {
            launch_pretssel_postnet_bn_tanh(cb, a.post_bn[l].scale, a.post_bn[l].shift, Re, cv.cout, bh, bl, m.stream);
            std::swap(ah, bh);
            std::swap(al, bl);
        } else {
            launch_pretssel_postnet_out(cb, a.post_bn[l].scale, a.post_bn[l].shift, d_proj, a.gstd, a.gmean, d_ext_item, d_pos2, d_frame_off, Re, mel, t_cap,
                                        d_mel, m.stream);
        }
        a.last_launches += 2;
    }
}

void run_pretssel_mel(sc_pretssel& a, const int32_t* h_tokens, int n, int s_tok, const int32_t* h_tok_lens, const int32_t* h_dur, int lang_index,
                      const float* d_pros, float* d_mel, int t_cap, int32_t* h_frame_lens) {
    Model& m = a.m;
    const sc_pretssel_config& c = a.cfg;
    const int M = c.model_dim, Ci = c.conv_inner_dim, H = c.pred_hidden_dim, PK = c.pred_kernel;
    // ---- every refusal before the first launch ----
    SC_CHECK(n >= 1 && n <= PRETSSEL_MAX_ITEMS, "sc_pretssel_mel: n=%d outside 1..%d", n, PRETSSEL_MAX_ITEMS);
    SC_CHECK(s_tok >= 1 && t_cap >= 1, "sc_pretssel_mel: s_tok=%d t_cap=%d", s_tok, t_cap);
    SC_CHECK(lang_index >= 0 && lang_index < c.num_langs, "sc_pretssel_mel: lang_index=%d outside the %d languages", lang_index, c.num_langs);
    const int pos0 = c.pad_idx + 1;
    std::vector<int> tok_off((size_t)n + 1, 0), frame_off((size_t)n + 1, 0), tok_lens(n), frame_lens(n);
    int smax = 0, tmax = 0;
    for (int i = 0; i < n; ++i) {
        const int L = h_tok_lens[i];
        SC_CHECK(L >= 1 && L <= s_tok, "sc_pretssel_mel: item %d has %d tokens (1..%d)", i, L, s_tok);
        SC_CHECK(L + pos0 <= c.max_seq_len, "sc_pretssel_mel: item %d: %d tokens run past max_seq_len=%d", i, L, c.max_seq_len);
        int64_t frames = 0;
        for (int k = 0; k < L; ++k) {
            const int tk = h_tokens[(size_t)i * s_tok + k], d = h_dur[(size_t)i * s_tok + k];
            SC_CHECK(tk >= 0 && tk < c.vocab_size, "sc_pretssel_mel: item %d token %d = %d outside the vocabulary of %d", i, k, tk, c.vocab_size);
            SC_CHECK(d >= 0 && d <= c.max_seq_len, "sc_pretssel_mel: item %d duration %d = %d", i, k, d);
            frames += d;
        }
        SC_CHECK(frames >= 1, "sc_pretssel_mel: item %d has no frames (all durations are zero)", i);
        SC_CHECK(frames + pos0 <= c.max_seq_len, "sc_pretssel_mel: item %d: %lld frames run past max_seq_len=%d", i, (long long)frames, c.max_seq_len);
        SC_CHECK(frames <= t_cap, "sc_pretssel_mel: item %d has %lld frames, t_cap=%d", i, (long long)frames, t_cap);
        tok_lens[i] = L;
        frame_lens[i] = (int)frames;
        tok_off[(size_t)i + 1] = tok_off[i] + L;
        frame_off[(size_t)i + 1] = frame_off[i] + (int)frames;
        smax = std::max(smax, L);
        tmax = std::max(tmax, (int)frames);
    }
    const int Rt = tok_off[n], Rf = frame_off[n];
    const int wide = std::max(std::max(3 * M, Ci), 3 * H);
    SC_CHECK(((int64_t)Rf + (int64_t)n * 64) * std::max(wide, std::max(c.post_dim, a.mel_pad)) * 4 < (1ll << 31) && (int64_t)Rt * wide * 4 < (1ll << 31) &&
                 (int64_t)n * t_cap * c.mel_dim < (1ll << 40),
             "sc_pretssel_mel: batch too large (%d tokens, %d frames)", Rt, Rf);
    if (h_frame_lens)
        for (int i = 0; i < n; ++i) h_frame_lens[i] = frame_lens[i];
    prof::set_tag("pretssel");
    a.last_launches = 0;

    // ---- host tables of the packed geometry ----
    std::vector<int> tok((size_t)Rt), dur((size_t)Rt), tok_t((size_t)Rt), tok_item((size_t)Rt), tok_pos((size_t)2 * Rt);
    std::vector<int> frm_item((size_t)Rf), frm_pos((size_t)2 * Rf);
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < tok_lens[i]; ++k) {
            const size_t r = (size_t)tok_off[i] + k;
            tok[r] = h_tokens[(size_t)i * s_tok + k];
            dur[r] = h_dur[(size_t)i * s_tok + k];
            tok_t[r] = k;
            tok_item[r] = i;
            tok_pos[2 * r] = k;
            tok_pos[2 * r + 1] = tok_lens[i];
        }
        for (int t = 0; t < frame_lens[i]; ++t) {
            const size_t r = (size_t)frame_off[i] + t;
            frm_item[r] = i;
            frm_pos[2 * r] = t;
            frm_pos[2 * r + 1] = frame_lens[i];
        }
    }
    Buf<int> d_tok = to_device(m, tok), d_dur = to_device(m, dur), d_tok_t = to_device(m, tok_t), d_tok_item = to_device(m, tok_item),
             d_tok_pos = to_device(m, tok_pos), d_frm_item = to_device(m, frm_item), d_frm_pos = to_device(m, frm_pos), d_tok_off = to_device(m, tok_off),
             d_frame_off = to_device(m, frame_off), d_tok_lens = to_device(m, tok_lens), d_frame_lens = to_device(m, frame_lens);

    // ---- every FiLM projection of the call ----
    Buf<float> film(m.pp(), (size_t)n * a.film_n);
    launch_pretssel_film(d_pros, c.film_cond_dim - c.lang_embed_dim, a.lang + (size_t)lang_index * c.lang_embed_dim, c.lang_embed_dim, a.film_w, a.film_b,
                         a.film_mul, a.film_add, n, a.film_n, film, m.stream);
    ++a.last_launches;

    const int Rmax = std::max(Rt, Rf);
    Buf<float> ubuf(m.pp(), (size_t)Rmax * M), ybuf(m.pp(), (size_t)Rmax * M), wbuf(m.pp(), (size_t)Rmax * wide);
    float* u = ubuf;  // the residual stream; u and y trade places behind the upsampling
    float* y = ybuf;
    Buf<__half> planes(m.pp(), (size_t)Rmax * (6 * M + 2 * wide));
    __half* up_h = planes.get();
    __half* up_l = up_h + (size_t)Rmax * M;
    const size_t RM = (size_t)Rmax * M;
    __half* wp_h = up_h + 6 * RM;
    __half* wp_l = wp_h + (size_t)Rmax * wide;
    // the FFT layers on R packed rows: u (fp32) and up_h / up_l (planes) hold the input and receive the output
    auto fft_layers = [&](const std::vector<PretsselLayer>& layers, int R, const int* d_row_off, const int* d_lens, int S, double pairs,
                          const int2* d_row_pos, const int* d_row_item) {
        FFTPass fp;
        fp.u = u, fp.y = y, fp.wide = wbuf;
        fp.up = {up_h, up_l}, fp.yp = {up_h + 2 * RM, up_h + 3 * RM}, fp.ap = {up_h + 4 * RM, up_h + 5 * RM}, fp.wp = {wp_h, wp_l};
        fp.d_row_pos = d_row_pos, fp.heads = c.num_heads, fp.head_dim = 128;
        fp.film = film, fp.film_ld = a.film_n, fp.row_item = d_row_item;
        BatchRows br;
        br.n = n, br.S = S, br.rows = R, br.d_lens = d_lens, br.d_off = d_row_off, br.pairs = pairs;
        for (const PretsselLayer& l : layers) a.last_launches += fft_layer_packed(m, l.fft, l.film.off, br, fp);
    };

    // ---- encoder front end + encoder over the packed tokens ----
    const int2* d_tok_pos2 = reinterpret_cast<const int2*>(d_tok_pos.get());
    launch_pretssel_embed_pos(d_tok, d_tok_t, a.embed, a.pos, a.alpha_enc, Rt, M, u, up_h, up_l, m.stream);
    ++a.last_launches;
    double pairs = 0;
    for (int i = 0; i < n; ++i) pairs += (double)tok_lens[i] * tok_lens[i];
    fft_layers(a.enc, Rt, d_tok_off, d_tok_lens, smax, pairs, d_tok_pos2, d_tok_item);

    // ---- variance adaptor: the three predictors side by side ----
    {
        float* h1 = wbuf;  // [Rt][3H]
        conv1d_presplit(m, up_h, up_l, a.pred_c1, nullptr, h1, nullptr, nullptr, 0, 0, PK / 2, 1, nullptr, ACT_RELU, Rt, d_tok_pos2);
        PretsselLnArgs f;
        f.x = h1;
        f.ldx = 3 * H;
        f.g = a.pred_ln1_g;
        f.b = a.pred_ln1_b;
        f.yh = wp_h;
        f.yl = wp_l;
        f.ldh = 3 * H;
        f.rows = Rt;
        f.C = H;
        f.groups = 3;
        launch_pretssel_film_ln(f, m.stream);
        for (int j = 0; j < 3; ++j) {
            const Conv& cv = a.pred_c2[j];
            GemmPsArgs g;
            g.Ah = wp_h + (size_t)j * H;
            g.Al = wp_l + (size_t)j * H;
            g.lda = 3 * H;
            g.W = cv.w;
            g.ldw = cv.kpad;
            g.bias = cv.b;
            g.C = h1 + (size_t)j * H;
            g.ldc = 3 * H;
            g.M = Rt;
            g.N = H;
            g.K = cv.kpad;
            g.act = ACT_RELU;
            g.conv_taps = PK;
            g.conv_cin = H;
            g.conv_dil = 1;
            g.conv_pad = PK / 2;
            g.row_pos = d_tok_pos2;
            launch_gemm_presplit(g, m.stream);
        }
        PretsselLnArgs f2;
        f2.x = h1;
        f2.ldx = 3 * H;
        f2.g = a.pred_ln2_g;
        f2.b = a.pred_ln2_b;
        f2.film = film;
        f2.film_ld = a.film_n;
        f2.film_off = a.film_pred_off;
        f2.row_item = d_tok_item;
        f2.y = h1;
        f2.ldy = 3 * H;
        f2.rows = Rt;
        f2.C = H;
        f2.groups = 3;
        launch_pretssel_film_ln(f2, m.stream);
        PretsselTailArgs tl;
        tl.f = h1;
        tl.pw = a.pred_pw;
        tl.pb = a.pred_pb;
        tl.wp = a.emb_pitch_w;
        tl.bp = a.emb_pitch_b;
        tl.we = a.emb_energy_w;
        tl.be = a.emb_energy_b;
        tl.x = u;
        tl.rows = Rt;
        tl.H = H;
        tl.C = M;
        launch_pretssel_var_tail(tl, m.stream);
        a.last_launches += 7;
    }

    // ---- Gaussian upsampling with the decoder's position term: tokens (u) -> frames (y and the planes), then y becomes u ----
    {
        Buf<float> centre(m.pp(), (size_t)Rt);
        PretsselUpsArgs g;
        g.x = u;
        g.dur = d_dur;
        g.tok_off = d_tok_off;
        g.frame_off = d_frame_off;
        g.centre = centre;
        g.pos_table = a.pos;
        g.pos_alpha = a.alpha_dec;
        g.delta = c.upsample_delta;
        g.y = y;
        g.yh = up_h;
        g.yl = up_l;
        g.n = n;
        g.frames = Rf;
        g.C = M;
        launch_pretssel_upsample(g, m.stream);
        std::swap(u, y);
        a.last_launches += 2;
    }

    // ---- decoder over the packed frames, projection ----
    const int2* d_frm_pos2 = reinterpret_cast<const int2*>(d_frm_pos.get());
    pairs = 0;
    for (int i = 0; i < n; ++i) pairs += (double)frame_lens[i] * frame_lens[i];
    fft_layers(a.dec, Rf, d_frame_off, d_frame_lens, tmax, pairs, d_frm_pos2, d_frm_item);
    Buf<float> proj(m.pp(), (size_t)Rf * c.mel_dim);
    linear_ps(m, {up_h, up_l}, a.proj, Rf, ACT_NONE, 1.f, nullptr, proj);
    ++a.last_launches;

    // ---- post-net on the extended rows, de-normalisation ----
    run_postnet(a, proj, n, frame_lens.data(), d_mel, t_cap);
    SC_HIP(hipStreamSynchronize(m.stream));  // the caller's stream is not ours: the output is complete on return
}

}  // namespace

extern "C" {

sc_pretssel* sc_pretssel_load(const sc_tensor_desc* tensors, size_t n_tensors, const sc_pretssel_config* cfg, int device) {
    return open_handle<sc_pretssel>("sc_pretssel_load", tensors, n_tensors, cfg, device, load_pretssel);
}

void sc_pretssel_free(sc_pretssel* p) { free_handle(p); }

int sc_pretssel_mel(sc_pretssel* p, const int32_t* h_tokens, int32_t n, int32_t s_tok, const int32_t* h_tok_lens, const int32_t* h_durations,
                    int32_t lang_index, const float* d_prosody, float* d_mel, int32_t t_cap, int32_t* h_frame_lens_or_null) {
    SC_API_BEGIN
    SC_CHECK(p && h_tokens && h_tok_lens && h_durations && d_prosody && d_mel, "sc_pretssel_mel: null argument");
    SC_HIP(hipSetDevice(p->m.device));
    run_pretssel_mel(*p, h_tokens, n, s_tok, h_tok_lens, h_durations, lang_index, d_prosody, d_mel, t_cap, h_frame_lens_or_null);
    SC_API_END
}

int32_t sc_op_pretssel_last_launches(sc_pretssel* p) { return p ? p->last_launches : -1; }

int32_t sc_op_pretssel_postnet_tile(int32_t rows, int32_t dim) { return rows > 0 && dim > 0 ? gemm_presplit_tile(rows, dim) : 0; }

float sc_op_pretssel_ups_cutoff(void) { return pretssel_ups_cutoff(); }

int sc_op_pretssel_postnet(sc_pretssel* p, const float* d_proj, int32_t n, const int32_t* h_frame_lens, float* d_mel, int32_t t_cap) {
    SC_API_BEGIN
    SC_CHECK(p && d_proj && h_frame_lens && d_mel && n >= 1 && n <= PRETSSEL_MAX_ITEMS && t_cap >= 1, "sc_op_pretssel_postnet: bad argument");
    int64_t rows = 0;
    for (int i = 0; i < n; ++i) {
        SC_CHECK(h_frame_lens[i] >= 1 && h_frame_lens[i] <= t_cap, "sc_op_pretssel_postnet: lens[%d]=%d outside 1..%d", i, h_frame_lens[i], t_cap);
        rows += h_frame_lens[i];
    }
    SC_CHECK((rows + (int64_t)n * 64) * std::max(p->cfg.post_dim, p->mel_pad) * 4 < (1ll << 31), "sc_op_pretssel_postnet: batch too large");
    SC_HIP(hipSetDevice(p->m.device));
    p->last_launches = 0;
    run_postnet(*p, d_proj, n, h_frame_lens, d_mel, t_cap);
    SC_HIP(hipStreamSynchronize(p->m.stream));
    SC_API_END
}

int sc_op_attention128(const float* d_q, const float* d_k, const float* d_v, float* d_out, int32_t nb, int32_t heads, int32_t sq, int32_t skv,
                       int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, const int32_t* d_kv_lens, const int32_t* d_row_off, void* d_out_hi,
                       void* d_out_lo, int64_t ldoh) {
    SC_API_BEGIN
    AttnArgs a;
    a.q = d_q;
    a.k = d_k;
    a.v = d_v;
    a.out = d_out;
    a.ldq = ldq;
    a.ldk = ldk;
    a.ldv = ldv;
    a.ldo = ldo;
    a.nb = nb;
    a.heads = heads;
    a.Sq = sq;
    a.Skv = skv;
    a.kv_lens = d_kv_lens;
    a.row_off = d_row_off;
    a.out_hi = static_cast<__half*>(d_out_hi);
    a.out_lo = static_cast<__half*>(d_out_lo);
    a.ldoh = ldoh;
    a.head_dim = 128;
    launch_attention(a, nullptr);
    SC_HIP(hipStreamSynchronize(nullptr));
    SC_API_END
}

int sc_op_pretssel_film(const float* d_pros, int32_t P, const float* d_lang, int32_t Lg, const void* d_w_f16, const float* d_bias, const float* d_mul,
                        const float* d_add, int32_t n, int32_t N, float* d_out) {
    SC_API_BEGIN
    launch_pretssel_film(d_pros, P, d_lang, Lg, static_cast<const __half*>(d_w_f16), d_bias, d_mul, d_add, n, N, d_out, nullptr);
    SC_HIP(hipStreamSynchronize(nullptr));
    SC_API_END
}

int sc_op_pretssel_film_ln(const float* d_x, const float* d_gamma, const float* d_beta, const float* d_film, int32_t film_ld, int32_t film_off,
                           const int32_t* d_row_item, float* d_y, void* d_yh_f16, void* d_yl_f16, int32_t rows, int32_t C, int32_t groups) {
    SC_API_BEGIN
    PretsselLnArgs a;
    a.x = d_x;
    a.ldx = (int64_t)C * groups;
    a.g = d_gamma;
    a.b = d_beta;
    a.film = d_film;
    a.film_ld = film_ld;
    a.film_off = film_off;
    a.row_item = d_row_item;
    a.y = d_y;
    a.ldy = (int64_t)C * groups;
    a.yh = static_cast<__half*>(d_yh_f16);
    a.yl = static_cast<__half*>(d_yl_f16);
    a.ldh = (int64_t)C * groups;
    a.rows = rows;
    a.C = C;
    a.groups = groups;
    launch_pretssel_film_ln(a, nullptr);
    SC_HIP(hipStreamSynchronize(nullptr));
    SC_API_END
}

int sc_op_pretssel_var_tail(const float* d_f, const float* d_pw, const float* d_pb, const float* d_wp, const float* d_bp, const float* d_we,
                            const float* d_be, float* d_x, float* d_vals, int32_t rows, int32_t H, int32_t C) {
    SC_API_BEGIN
    PretsselTailArgs a;
    a.f = d_f;
    a.pw = d_pw;
    a.pb = d_pb;
    a.wp = d_wp;
    a.bp = d_bp;
    a.we = d_we;
    a.be = d_be;
    a.x = d_x;
    a.vals = d_vals;
    a.rows = rows;
    a.H = H;
    a.C = C;
    launch_pretssel_var_tail(a, nullptr);
    SC_HIP(hipStreamSynchronize(nullptr));
    SC_API_END
}

int sc_op_pretssel_upsample(const float* d_x, const int32_t* h_tok_lens, const int32_t* h_dur, int32_t n, int32_t C, float delta,
                            const float* d_pos_table, float pos_alpha, float* d_y, void* d_yh_f16, void* d_yl_f16, float* d_wsum) {
    SC_API_BEGIN
    SC_CHECK(d_x && h_tok_lens && h_dur && n >= 1 && n <= PRETSSEL_MAX_ITEMS, "sc_op_pretssel_upsample: bad argument");
    std::vector<int> tok_off((size_t)n + 1, 0), frame_off((size_t)n + 1, 0), dur;
    for (int i = 0; i < n; ++i) {
        SC_CHECK(h_tok_lens[i] >= 1, "sc_op_pretssel_upsample: item %d has no tokens", i);
        int64_t frames = 0;
        for (int k = 0; k < h_tok_lens[i]; ++k) {
            const int d = h_dur[(size_t)tok_off[i] + k];
            SC_CHECK(d >= 0 && d < (1 << 20), "sc_op_pretssel_upsample: duration %d", d);
            dur.push_back(d);
            frames += d;
        }
        SC_CHECK(frames >= 1 && frames < (1 << 22), "sc_op_pretssel_upsample: item %d has %lld frames", i, (long long)frames);
        tok_off[(size_t)i + 1] = tok_off[i] + h_tok_lens[i];
        frame_off[(size_t)i + 1] = frame_off[i] + (int)frames;
    }
    OpScratch sc_;
    PretsselUpsArgs a;
    a.x = d_x;
    a.dur = sc_.put(dur);
    a.tok_off = sc_.put(tok_off);
    a.frame_off = sc_.put(frame_off);
    a.centre = sc_.get<float>(dur.size());
    a.pos_table = d_pos_table;
    a.pos_alpha = pos_alpha;
    a.delta = delta;
    a.y = d_y;
    a.yh = static_cast<__half*>(d_yh_f16);
    a.yl = static_cast<__half*>(d_yl_f16);
    a.wsum = d_wsum;
    a.n = n;
    a.frames = frame_off[n];
    a.C = C;
    launch_pretssel_upsample(a, nullptr);
    SC_HIP(hipStreamSynchronize(nullptr));
    SC_API_END
}

}  // extern "C"
