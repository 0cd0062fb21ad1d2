// Speech side of the hot path: fbank front-end and the W2v-BERT 2.0
// Conformer-Shaw encoder with the UnitY length adaptor.
//
// Reference call sites (src/seamless_communication/...):
//   inference/translator.py:136-143,293  WaveformToFbankConverter + Collater
//   models/unity/model.py:132-139        UnitYModel.encode_speech
//   models/unity/adaptor_block.py:98-125 UnitYEncoderAdaptor.forward
//   models/unity/adaptor_block.py:237-314 UnitYTransformerAdaptorLayer
//   models/conformer_shaw/builder.py:127-156 Shaw SDPA + causal depthwise conv
#include <cstdlib>

#include <cmath>
#include "model.h"

namespace sc {

static void upload_i32(Model& m, int* d, const int32_t* h, int n) {
    SC_HIP(hipMemcpyAsync(d, h, (size_t)n * 4, hipMemcpyHostToDevice, m.stream));
}

// kaldi's FrameExtractionOptions at a sample rate (feature-window.h): float arithmetic, truncated
static void fbank_geometry(int sample_rate, int& frame_len, int& frame_shift, int& nfft) {
    frame_len = (int)((float)sample_rate * 0.001f * 25.0f);
    frame_shift = (int)((float)sample_rate * 0.001f * 10.0f);
    nfft = 1;
    while (nfft < frame_len) nfft *= 2;
}

int fbank_num_frames(int64_t num_samples, int sample_rate) {
    int fl, fs, nf;
    fbank_geometry(sample_rate, fl, fs, nf);
    return num_samples < fl ? 0 : (int)(1 + (num_samples - fl) / fs);
}

// window | melT[nfft/2][80] | cos | sin of a rate, built once per handle (the expressions of build_fbank_consts, model_load.hip:
// feature-window.cc:30-55 povey window; mel-computations.cc:107-210 mel banks, high_freq 0 = the rate's Nyquist)
static const Model::FbankRate& fbank_rate_consts(Model& m, int sample_rate) {
    auto it = m.fbank_rates.find(sample_rate);
    if (it != m.fbank_rates.end()) return it->second;
    Model::FbankRate r;
    fbank_geometry(sample_rate, r.frame_len, r.frame_shift, r.nfft);
    SC_CHECK(r.frame_shift >= 1 && r.nfft >= 256 && r.nfft <= 2048,
             "sc_fbank_rate: sample rate %d Hz gives a %d-sample window (supported: 129 .. 2048 samples, 5.2 - 81.9 kHz)", sample_rate, r.frame_len);
    const int half = r.nfft / 2, nb = m.cfg.num_fbank_channels;
    SC_CHECK(nb == 80, "sc_fbank_rate: %d mel bins (the kernel is built for 80)", nb);
    std::vector<float> c((size_t)r.frame_len + (size_t)half * nb + 2 * (size_t)half, 0.f);
    const double a = 2.0 * M_PI / (r.frame_len - 1);
    for (int i = 0; i < r.frame_len; ++i) c[i] = (float)std::pow(0.5 - 0.5 * std::cos(a * (double)i), 0.85);
    auto mel_scale = [](float f) { return 1127.0f * logf(1.0f + f / 700.0f); };
    const float nyquist = 0.5f * (float)sample_rate, fft_bin_width = (float)sample_rate / (float)r.nfft;
    const float mel_low = mel_scale(20.0f), mel_high = mel_scale(nyquist);
    const float delta = (mel_high - mel_low) / (float)(nb + 1);
    float* melT = c.data() + r.frame_len;
    for (int b = 0; b < nb; ++b) {
        const float left = mel_low + b * delta, center = mel_low + (b + 1) * delta, right = mel_low + (b + 2) * delta;
        for (int i = 0; i < half; ++i) {
            const float mel = mel_scale(fft_bin_width * i);
            if (mel > left && mel < right) melT[i * nb + b] = mel <= center ? (mel - left) / (center - left) : (right - mel) / (right - center);
        }
    }
    float* tw = melT + (size_t)half * nb;
    for (int k = 0; k < half; ++k) {
        tw[k] = (float)std::cos(-2.0 * M_PI * k / (double)r.nfft);
        tw[half + k] = (float)std::sin(-2.0 * M_PI * k / (double)r.nfft);
    }
    void* d = nullptr;
    SC_HIP(hipMalloc(&d, c.size() * 4));
    SC_HIP(hipMemcpy(d, c.data(), c.size() * 4, hipMemcpyHostToDevice));
    r.consts = static_cast<float*>(d);
    return m.fbank_rates.emplace(sample_rate, r).first->second;
}

void run_fbank(Model& m, const float* d_wav, int n, int64_t wav_stride, const int32_t* h_ns, int standardize,
               float* d_out, int t_rows, int32_t* h_frames, int sample_rate) {
    SC_CHECK(n > 0 && t_rows > 0, "sc_fbank: empty batch");
    SC_CHECK(sample_rate > 0, "sc_fbank: sample rate %d", sample_rate);
    std::vector<int32_t> frames(n);
    for (int i = 0; i < n; ++i) {
        SC_CHECK(h_ns[i] >= 0 && h_ns[i] <= wav_stride, "sc_fbank: num_samples[%d]=%d exceeds the row stride", i, h_ns[i]);
        frames[i] = fbank_num_frames(h_ns[i], sample_rate);
        SC_CHECK(frames[i] <= t_rows, "sc_fbank: item %d has %d frames but the output has only %d rows", i, frames[i],
                 t_rows);
        if (h_frames) h_frames[i] = frames[i];
    }
    Buf<int> d_ns(m.pp(), n), d_fr(m.pp(), n);
    upload_i32(m, d_ns, h_ns, n);
    upload_i32(m, d_fr, frames.data(), n);
    if (sample_rate == 16000) {
        launch_fbank(d_wav, wav_stride, d_ns, n, d_out, t_rows, m.fbank_consts, 32768.0f, m.stream);
    } else {
        const Model::FbankRate& r = fbank_rate_consts(m, sample_rate);
        launch_fbank_any(d_wav, wav_stride, d_ns, n, d_out, t_rows, r.consts, 32768.0f, r.frame_len, r.frame_shift, r.nfft, m.stream);
    }
    if (standardize) launch_standardize(d_out, n, t_rows, d_fr, m.cfg.num_fbank_channels, m.stream);
    SC_HIP(hipStreamSynchronize(m.stream));  // host-side length vectors must outlive the copies
}

static int adaptor_len(const sc_config& c, int len) {
    // _compute_new_padding_mask (adaptor_block.py:426-438): floor((len + 2*pad - k)/stride + 1)
    const int pad = c.adaptor_kernel_size / 2;
    const double v = (double)(len + 2 * pad - c.adaptor_kernel_size) / (double)c.adaptor_stride + 1.0;
    return (int)std::floor(v);
}

int encoder_out_len(const Model& m, int t_frames) {
    const sc_config& c = m.cfg;
    const int S = t_frames / c.fbank_stride;
    const int pad = c.adaptor_kernel_size / 2;
    return (S + 2 * pad - c.adaptor_kernel_size) / c.adaptor_stride + 1;  // Conv1d output length
}

void run_encode_speech(Model& m, const float* d_fbank, int n, int t_frames, const int32_t* h_lens, float* d_out,
                       int32_t* h_out_lens) {
    const sc_config& c = m.cfg;
    const int M = c.model_dim;
    SC_CHECK(n > 0 && t_frames > 0, "sc_encode_speech: empty batch");
    prof::set_tag("enc");
    SC_CHECK(t_frames % c.fbank_stride == 0, "sc_encode_speech: t_frames=%d must be a multiple of fbank_stride=%d (Collater pad_to_multiple)",
             t_frames, c.fbank_stride);
    const int S = t_frames / c.fbank_stride;
    const int rows = n * S;
    const int feat = c.num_fbank_channels * c.fbank_stride;
    std::vector<int32_t> lens(n), alens(n);
    for (int i = 0; i < n; ++i) {
        SC_CHECK(h_lens[i] >= 0 && h_lens[i] <= t_frames, "sc_encode_speech: frame_lens[%d]=%d out of range", i, h_lens[i]);
        lens[i] = h_lens[i] / c.fbank_stride;
        alens[i] = adaptor_len(c, lens[i]);
        if (h_out_lens) h_out_lens[i] = alens[i];
    }
    Buf<int> d_lens(m.pp(), n), d_alens(m.pp(), n);
    upload_i32(m, d_lens, lens.data(), n);
    upload_i32(m, d_alens, alens.data(), n);

    const int F = std::max(std::max(c.enc_ffn_dim, c.adaptor_proj_dim), std::max(3 * M, c.adaptor_ffn_dim));
    Buf<float> x(m.pp(), (size_t)rows * M), h(m.pp(), (size_t)rows * std::max(M, feat)), wide(m.pp(), (size_t)rows * F),
        att(m.pp(), (size_t)rows * M);

    // frontend: stack fbank_stride frames (a pure reinterpretation of the
    // contiguous [n][t_frames][80] buffer), LayerNorm, Linear
    launch_layernorm(d_fbank, feat, m.fe_ln.g, m.fe_ln.b, h, feat, rows, feat, ACT_NONE, nullptr, 1, m.stream);
    linear(m, h, feat, m.fe_proj, nullptr, 0, x, M, rows, ACT_NONE, 1.f);

    // Operands of the products are kept as two fp16 planes (hi, lo) written by their producers - LayerNorm, the FFN
    // inner product's epilogue, the attention kernel - and consumed by the DMA-fed product kernel (k_gemm_ps.hip);
    // the residual stream x and the tensors read by element-wise kernels stay fp32.  SC_PRESPLIT=0 selects the
    // on-the-fly split path (same bits).
    static const bool presplit = knob::value("SC_PRESPLIT", 1) != 0;
    const bool v1 = c.enc_variant == 1;  // w2v-BERT of the v1 models: fp32-operand path below (not the throughput path)
    const bool ps_ok = !v1 && presplit && M % 32 == 0 && c.enc_ffn_dim % 32 == 0 && (int64_t)rows * std::max(M, c.enc_ffn_dim) * 2 < (1ll << 31);
    // v1: position table [2S-1][M] once per call, its projection r_proj(table) per layer
    Buf<float> rp_tab(m.pp(), v1 ? (size_t)(2 * S - 1) * M : 0), rp_proj(m.pp(), v1 ? (size_t)(2 * S - 1) * M : 0);
    if (v1) launch_relpos_table(S, M, rp_tab, m.stream);
    Buf<__half> hs(m.pp(), ps_ok ? (size_t)2 * rows * M : 0), ws(m.pp(), ps_ok ? (size_t)2 * rows * c.enc_ffn_dim : 0),
        as(m.pp(), ps_ok ? (size_t)2 * rows * M : 0);
    BatchRows br;
    br.n = n, br.S = S, br.rows = rows, br.d_lens = d_lens;
    // fused element-wise passes (SC_ENC_FUSE=0: the separate launches, same bits): GLU + depthwise conv + LayerNorm + SiLU
    // in one kernel; a layer's closing LayerNorm together with the next layer's first one
    static const bool fuse = knob::value("SC_ENC_FUSE", 1) != 0;
    // SC_SPLIT_MODE=1 (precision study, scripts/split_study.py; never the default): the Conformer products use the
    // hi plane only, i.e. the activation operand is rounded to fp16 once instead of being carried to ~2^-22
    static const bool single = knob::value("SC_SPLIT_MODE", 0) == 1;
    ConformerPass cp;
    cp.x = x, cp.wide = wide, cp.att = att;
    cp.hs = {hs.get(), ps_ok ? hs.get() + (size_t)rows * M : nullptr};
    cp.as = {as.get(), ps_ok ? as.get() + (size_t)rows * M : nullptr};
    cp.ws = {ws.get(), ps_ok ? ws.get() + (size_t)rows * c.enc_ffn_dim : nullptr};
    cp.fuse_conv = fuse && glu_dwconv_ln_supported(M, c.depthwise_conv_kernel_size);
    cp.fuse_ln = fuse && M <= 1024;
    // GLU of the convolution module inside the first pointwise product (SC_ENC_GLU_EPI=0, read per call: pw1 writes both halves
    // and the depthwise kernel gates them; same bits)
    cp.glu_epi = ps_ok && cp.fuse_conv && !single && knob::live("SC_ENC_GLU_EPI", 1) != 0;
    cp.split = single ? 0 : 1;
    bool ffn1_planes_ready = false;  // the previous layer's closing launch already wrote LN_ffn1(x) as planes
    for (int li = 0; li < c.enc_layers; ++li) {
        const ConformerLayer& l = m.enc[li];
        if (ps_ok) {
            ffn1_planes_ready = conformer_layer(m, l, li + 1 < c.enc_layers ? &m.enc[li + 1] : nullptr, br, cp, ffn1_planes_ready);
            continue;
        }
        // x += 0.5 * FFN1(LN(x))
        layernorm(m, x, l.ffn1_ln, h, rows);
        linear(m, h, M, l.ffn1_in, nullptr, 0, wide, c.enc_ffn_dim, rows, ACT_SILU, 1.f);
        linear(m, wide, c.enc_ffn_dim, l.ffn1_out, x, M, x, M, rows, ACT_NONE, 0.5f);
        // x += MHA_shaw(LN(x))   (v1: Transformer-XL relative positions, fairseq2.cpp:605-696)
        layernorm(m, x, l.attn_ln, h, rows);
        linear(m, h, M, l.qkv, nullptr, 0, wide, 3 * M, rows, ACT_NONE, 1.f);
        SelfAttn at;
        at.heads = c.num_heads;
        at.out = att;
        if (v1) {
            linear(m, rp_tab, M, l.r_proj, nullptr, 0, rp_proj, M, 2 * S - 1, ACT_NONE, 1.f);
            at.rp_table = rp_proj;
            at.q_bias_u = l.u_bias;
            at.q_bias_v = l.v_bias;
        } else if (l.rel_k) {
            at.rel_k = l.rel_k;
            at.rel_left = c.shaw_max_left;
            at.rel_right = c.shaw_max_right;
        }
        self_attention(m, wide, M, br, at);
        linear(m, att, M, l.attn_out, x, M, x, M, rows, ACT_NONE, 1.f);
        // x += Conv(LN(x))
        layernorm(m, x, l.conv_ln, h, rows);
        linear(m, h, M, l.pw1, nullptr, 0, wide, 2 * M, rows, ACT_NONE, 1.f);
        if (v1) {  // centred depthwise conv + BatchNorm (folded) + SiLU in one pass (fairseq2.cpp:698-731)
            launch_glu_dwconv(wide, 2 * M, l.dw, h, M, n, S, M, c.depthwise_conv_kernel_size, d_lens, m.stream,
                              c.depthwise_conv_kernel_size / 2, l.bn_scale, l.bn_shift);
        } else {
            launch_glu_dwconv(wide, 2 * M, l.dw, att, M, n, S, M, c.depthwise_conv_kernel_size, d_lens, m.stream);
            layernorm(m, att, l.conv_inner_ln, h, rows, ACT_SILU);
        }
        linear(m, h, M, l.pw2, x, M, x, M, rows, ACT_NONE, 1.f);
        // x += 0.5 * FFN2(LN(x)); x = LN(x)
        layernorm(m, x, l.ffn2_ln, h, rows);
        linear(m, h, M, l.ffn2_in, nullptr, 0, wide, c.enc_ffn_dim, rows, ACT_SILU, 1.f);
        linear(m, wide, c.enc_ffn_dim, l.ffn2_out, x, M, x, M, rows, ACT_NONE, 0.5f);
        layernorm(m, x, l.final_ln, x, rows);
    }
    // adaptor head (adaptor_block.py:105-109)
    layernorm(m, x, m.enc_inner_ln, x, rows);
    linear(m, x, M, m.enc_proj1, nullptr, 0, wide, c.adaptor_proj_dim, rows, ACT_RELU, 1.f);
    linear(m, wide, c.adaptor_proj_dim, m.enc_proj2, x, M, x, M, rows, ACT_NONE, 0.5f);

    // adaptor layer (adaptor_block.py:249-314)
    const AdaptorLayer& a = m.adaptor;
    const int Sa = encoder_out_len(m, t_frames);
    const int arows = n * Sa;
    const int k = c.adaptor_kernel_size, st = c.adaptor_stride, pad = k / 2;
    Buf<float> res(m.pp(), (size_t)arows * M), y(m.pp(), (size_t)arows * M), conv(m.pp(), (size_t)arows * 2 * M),
        aw(m.pp(), (size_t)arows * std::max(3 * M, c.adaptor_ffn_dim)), ah(m.pp(), (size_t)arows * M);
    layernorm(m, x, a.res_ln, h, rows);
    conv1d(m, h, a.res_conv, nullptr, conv, n, S, st, pad, 1, nullptr, IN_NONE, ACT_NONE);
    launch_glu(conv, 2 * M, res, M, arows, M, m.stream);
    layernorm(m, x, a.attn_ln, h, rows);
    conv1d(m, h, a.attn_conv, nullptr, conv, n, S, st, pad, 1, nullptr, IN_NONE, ACT_NONE);
    launch_glu(conv, 2 * M, y, M, arows, M, m.stream);
    BatchRows ab;
    ab.n = n, ab.S = Sa, ab.rows = arows, ab.d_lens = d_alens;
    adaptor_layer_tail(m, a, ab, res, y, aw, ah, /*row_independent=*/false);
    launch_layernorm(y, M, m.enc_final_ln.g, m.enc_final_ln.b, d_out, M, arows, M, ACT_NONE, nullptr, 1, m.stream);
    SC_HIP(hipStreamSynchronize(m.stream));
}

// The speech encoder on a ragged batch in ONE packed pass (sc_encode_speech_ragged).  Item i contributes its own
// S_i = frame_lens[i] / fbank_stride stacked rows and nothing else: the Conformer stack runs on R = sum S_i rows, the adaptor
// layer on Ra = sum adaptor_len(S_i) rows, items back to back.  The layers are run_encode_speech's own (conformer_layer,
// adaptor_layer_tail: layers.hip) on packed rows, every product the tiled one (row_independent), so an item carries the same bits
// in any batch and - above 64 rows, where run_encode_speech takes the tiled products too - the bits of run_encode_speech on the
// item alone.  One form only: planes with the fused passes (SC_PRESPLIT / SC_ENC_FUSE do not apply).
// The adaptor's two strided convolutions are plain products over gathered windows: row j of item i holds the
// adaptor_kernel_size packed rows j * stride - pad .. tap-major, the order of the packed Conv1d weight [C_out][tap * C_in + c].
void run_encode_speech_ragged(Model& m, const float* d_fbank, int n, int t_frames, const int32_t* h_lens, float* d_out, int s_enc_cap,
                              int32_t* h_out_lens) {
    const sc_config& c = m.cfg;
    const int M = c.model_dim, Fd = c.enc_ffn_dim;
    const int stride = c.fbank_stride, feat = c.num_fbank_channels * c.fbank_stride;
    const int k = c.adaptor_kernel_size, st = c.adaptor_stride, pad = k / 2;
    const AdaptorLayer& ad = m.adaptor;
    SC_CHECK(n > 0 && t_frames > 0 && s_enc_cap > 0, "sc_encode_speech_ragged: empty batch");
    SC_CHECK(c.enc_variant != 1, "sc_encode_speech_ragged: the v1 speech encoder (enc_variant 1) has no packed pass; use sc_encode_speech");
    SC_CHECK(M % 32 == 0 && Fd % 32 == 0 && glu_dwconv_ln_supported(M, c.depthwise_conv_kernel_size) && feat % 4 == 0 &&
                 ad.res_conv.kpad == k * M && ad.attn_conv.kpad == k * M,
             "sc_encode_speech_ragged: model_dim=%d, enc_ffn_dim=%d, %d depthwise taps: the packed pass needs dimensions that are multiples "
             "of 32, model_dim a multiple of 64 up to 1024 and 31 taps",
             M, Fd, c.depthwise_conv_kernel_size);
    SC_CHECK((int64_t)n * t_frames < (1ll << 31) && (int64_t)n * s_enc_cap < (1ll << 31), "sc_encode_speech_ragged: n=%d x t_frames=%d rows", n, t_frames);
    std::vector<int32_t> lens(n), alens(n), off(n), aoff(n);
    int64_t R64 = 0, Ra64 = 0;
    int S = 0, Sa = 0;
    double pairs = 0, apairs = 0;
    for (int i = 0; i < n; ++i) {
        SC_CHECK(h_lens[i] >= 0 && h_lens[i] <= t_frames, "sc_encode_speech_ragged: frame_lens[%d]=%d outside [0, t_frames=%d]", i, h_lens[i], t_frames);
        SC_CHECK(h_lens[i] >= stride, "sc_encode_speech_ragged: item %d has %d frames, fewer than one stride of %d", i, h_lens[i], stride);
        lens[i] = h_lens[i] / stride;
        alens[i] = adaptor_len(c, lens[i]);
        SC_CHECK(alens[i] >= 1, "sc_encode_speech_ragged: item %d has no output row", i);
        R64 += lens[i];
        Ra64 += alens[i];
        S = std::max(S, lens[i]);
        Sa = std::max(Sa, alens[i]);
        pairs += (double)lens[i] * lens[i];
        apairs += (double)alens[i] * alens[i];
    }
    auto capacity = [](bool ok, const char* fmt, auto... args) {
        if (ok) return;
        set_error(fmt, args...);
        throw Error{SC_ERR_CAPACITY};
    };
    capacity(s_enc_cap >= Sa, "sc_encode_speech_ragged: the longest item has %d output rows, s_enc_cap is %d", Sa, s_enc_cap);
    capacity(R64 * std::max(std::max(M, Fd), feat) * 2 < (1ll << 31) && Ra64 * k * M < (1ll << 31),
             "sc_encode_speech_ragged: %lld packed rows exceed the 2^31-element bound of a product operand; encode the batch in groups",
             (long long)R64);
    const int R = (int)R64, Ra = (int)Ra64;
    prof::set_tag("enc");
    for (int i = 0, r = 0, ra = 0; i < n; r += lens[i], ra += alens[i], ++i) {
        off[i] = r;
        aoff[i] = ra;
        if (h_out_lens) h_out_lens[i] = alens[i];
    }

    // host tables, one upload: the convolution module's work table first (16-byte records), then offsets and lengths, then the
    // three row-index lists of the gathers (-1: a row of zeros)
    std::vector<int32_t> tab;
    glu_dwconv_ln_packed_work(off.data(), lens.data(), n, tab);
    const int n_work = (int)(tab.size() / 4);
    const size_t o_off = tab.size(), o_lens = o_off + n, o_aoff = o_lens + n, o_alens = o_aoff + n, o_fidx = o_alens + n,
                 o_widx = o_fidx + R, o_sidx = o_widx + (size_t)Ra * k;
    tab.resize(o_sidx + (size_t)n * s_enc_cap, -1);
    for (int i = 0; i < n; ++i) {
        tab[o_off + i] = off[i];
        tab[o_lens + i] = lens[i];
        tab[o_aoff + i] = aoff[i];
        tab[o_alens + i] = alens[i];
        for (int t = 0; t < lens[i]; ++t) tab[o_fidx + off[i] + t] = i * t_frames + t * stride;  // fbank row of the stacked row's first frame
        for (int j = 0; j < alens[i]; ++j) {
            tab[o_sidx + (size_t)i * s_enc_cap + j] = aoff[i] + j;
            for (int tap = 0; tap < k; ++tap) {
                const int t = j * st - pad + tap;
                if (t >= 0 && t < lens[i]) tab[o_widx + (size_t)(aoff[i] + j) * k + tap] = off[i] + t;
            }
        }
    }
    Buf<int> d_tab(m.pp(), tab.size());
    SC_HIP(hipMemcpyAsync(d_tab.get(), tab.data(), tab.size() * 4, hipMemcpyHostToDevice, m.stream));
    const int* d_work = d_tab.get();
    const int *d_off = d_work + o_off, *d_lens = d_work + o_lens, *d_aoff = d_work + o_aoff, *d_alens = d_work + o_alens,
              *d_fidx = d_work + o_fidx, *d_widx = d_work + o_widx, *d_sidx = d_work + o_sidx;

    const int F = std::max(c.adaptor_proj_dim, 3 * M);
    Buf<float> x(m.pp(), (size_t)R * M), h(m.pp(), (size_t)R * std::max(M, feat)), wide(m.pp(), (size_t)R * F);
    Buf<__half> planes(m.pp(), (size_t)R * (4 * M + 2 * Fd));
    // the padded entry's layer with this entry's fixed choices: fused passes, both planes, SC_ENC_GLU_EPI read per call
    ConformerPass cp;
    cp.x = x, cp.wide = wide;
    cp.hs = {planes.get(), planes.get() + (size_t)R * M};
    cp.as = {cp.hs.lo + (size_t)R * M, cp.hs.lo + (size_t)2 * R * M};
    cp.ws = {cp.as.lo + (size_t)R * M, cp.as.lo + (size_t)R * M + (size_t)R * Fd};
    cp.glu_epi = knob::live("SC_ENC_GLU_EPI", 1) != 0;
    cp.d_work = d_work, cp.n_work = n_work;
    BatchRows br, ab;
    br.n = ab.n = n;
    br.S = S, br.rows = R, br.d_lens = d_lens, br.d_off = d_off, br.pairs = pairs;
    ab.S = Sa, ab.rows = Ra, ab.d_lens = d_alens, ab.d_off = d_aoff, ab.pairs = apairs;

    // frontend: stack fbank_stride frames of the item's own rows into packed order, LayerNorm, Linear
    launch_gather_rows(d_fbank, c.num_fbank_channels, d_fidx, h, feat, R, feat, m.stream);
    launch_layernorm(h, feat, m.fe_ln.g, m.fe_ln.b, h, feat, R, feat, ACT_NONE, nullptr, 1, m.stream);
    linear(m, h, feat, m.fe_proj, nullptr, 0, x, M, R, ACT_NONE, 1.f, /*row_independent=*/true);

    bool ffn1_planes_ready = false;
    for (int li = 0; li < c.enc_layers; ++li)
        ffn1_planes_ready = conformer_layer(m, m.enc[li], li + 1 < c.enc_layers ? &m.enc[li + 1] : nullptr, br, cp, ffn1_planes_ready);
    // adaptor head (adaptor_block.py:105-109)
    layernorm(m, x, m.enc_inner_ln, x, R);
    linear(m, x, M, m.enc_proj1, nullptr, 0, wide, c.adaptor_proj_dim, R, ACT_RELU, 1.f, true);
    linear(m, wide, c.adaptor_proj_dim, m.enc_proj2, x, M, x, M, R, ACT_NONE, 0.5f, true);

    // adaptor layer (adaptor_block.py:249-314) on Ra packed rows
    Buf<float> win(m.pp(), (size_t)Ra * k * M), res(m.pp(), (size_t)Ra * M), y(m.pp(), (size_t)Ra * M), conv(m.pp(), (size_t)Ra * 2 * M),
        aw(m.pp(), (size_t)Ra * std::max(3 * M, c.adaptor_ffn_dim)), ah(m.pp(), (size_t)Ra * M);
    auto strided_conv_glu = [&](const LNorm& L, const Conv& cv, float* out) {
        layernorm(m, x, L, h, R);
        launch_gather_rows(h, M, d_widx, win, M, Ra * k, M, m.stream);  // win [Ra][k * M]: tap-major windows
        Linear w;
        w.w = cv.w;
        w.ldw = cv.kpad;
        w.b = cv.b;
        w.out = cv.cout;
        w.in = w.kpad = cv.kpad;
        linear(m, win, (int64_t)k * M, w, nullptr, 0, conv, 2 * M, Ra, ACT_NONE, 1.f, true);
        launch_glu(conv, 2 * M, out, M, Ra, M, m.stream);
    };
    strided_conv_glu(ad.res_ln, ad.res_conv, res);
    strided_conv_glu(ad.attn_ln, ad.attn_conv, y);
    adaptor_layer_tail(m, ad, ab, res, y, aw, ah, /*row_independent=*/true);
    layernorm(m, y, m.enc_final_ln, y, Ra);
    // packed rows into the padded [n][s_enc_cap][M] output, zeros behind each item's length
    launch_gather_rows(y, M, d_sidx, d_out, M, n * s_enc_cap, M, m.stream);
    SC_HIP(hipStreamSynchronize(m.stream));
}

}  // namespace sc
