// PRETSSEL waveform generator (sc_pretssel_wave_*): mel rows -> normalise -> the mel HiFi-GAN (the unit vocoder's stage loop,
// model_t2u.hip) -> SEANet encoder, two 2-layer LSTMs, decoder (k_seanet.hip) -> 0.8 * h[:L] + tanh(skip); and the kernel-level
// entries the tests drive (include/seamless_hip_internal.h).  Reference: models/generator/vocoder.py:515-573, streamable.py.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "handle.h"
#include "loader.h"

using namespace sc;

namespace {

constexpr int WAVE_MAX_ITEMS = 1024;

// lens [n] -> offsets [n + 1]; returns the longest item
int offsets_of(const char* what, const int32_t* lens, int n, std::vector<int>& off) {
    SC_CHECK(lens && n >= 1 && n <= WAVE_MAX_ITEMS, "%s: n=%d outside 1..%d", what, n, WAVE_MAX_ITEMS);
    off.assign((size_t)n + 1, 0);
    int longest = 0;
    for (int i = 0; i < n; ++i) {
        SC_CHECK(lens[i] >= 1 && (int64_t)off[i] + lens[i] < (1 << 24), "%s: lens[%d]=%d (at least 1, 2^24 rows in all)", what, i, lens[i]);
        off[(size_t)i + 1] = off[i] + lens[i];
        longest = std::max(longest, lens[i]);
    }
    return longest;
}

}  // namespace

namespace sc {

// y = LSTM(x) + x over packed items: x / y [rows][H], d_off [n + 1]; longest + 1 step launches behind one input product.
// The product is launch_gemm's tiled kernel.  Which tile shape it picks depends on the row count, but every tile shape walks K
// in the same order (the row_independent contract of linear(), model_load.hip), so a row's bits do not depend on the rows
// around it; tests/test_pretssel_wave_gpu.py checks it at row counts on both sides of the tile switches.
int run_lstm2(const Lstm2& w, const float* x, const int* d_off, int n, int rows, int longest, float* xproj, float* h0, float* h1, float* c, float* y,
              float* max_pre, hipStream_t s) {
    const int H = w.H;
    GemmArgs g;
    g.A = x;
    g.lda = H;
    g.W = w.wih0;
    g.ldw = H;
    g.C = xproj;
    g.ldc = 4 * H;
    g.M = rows;
    g.N = 4 * H;
    g.K = H;
    g.rows_per_batch = rows;
    g.t_in = rows;
    g.t_out = rows;
    g.taps = 1;
    g.cin = H;
    launch_gemm(g, s);
    SC_HIP(hipMemsetAsync(c, 0, (size_t)2 * n * H * sizeof(float), s));
    LstmStepArgs a;
    a.xproj = xproj;
    a.x = x;
    a.whh0 = w.whh0;
    a.w1 = w.w1;
    a.b_ih0 = w.b_ih0;
    a.b_hh0 = w.b_hh0;
    a.b_ih1 = w.b_ih1;
    a.b_hh1 = w.b_hh1;
    a.h0 = h0;
    a.h1 = h1;
    a.c0 = c;
    a.c1 = c + (size_t)n * H;
    a.y = y;
    a.max_pre = max_pre;
    a.row_off = d_off;
    a.H = H;
    for (int t = 0; t <= longest; ++t) launch_lstm2_step(a, n, t, s);
    return longest + 2;  // launches: the product and the steps
}

}  // namespace sc

// ---- the handle ------------------------------------------------------------------------------------------------------------
namespace {
struct SConv {  // a streamable convolution, weight norm folded: wt [k * cin][cout]
    const __half* wt = nullptr;
    const float* b = nullptr;
    int cin = 0, cout = 0, k = 0, stride = 1;
};
struct SRes {  // the residual block: fused at C = 32 / 64 (w1, w2), else two convolution launches (c1, c2)
    int C = 0;
    const __half* w1 = nullptr;
    const __half* w2 = nullptr;
    SConv c1, c2;
};
}  // namespace

struct sc_pretssel_wave_model {
    Model m;
    sc_pretssel_wave_config cfg{};
    int hop = 1;
    const float* mean = nullptr;
    const float* scale = nullptr;
    SConv first, enc_down[4], enc_out, dec_in, dec_up[4];
    SRes enc_res[4], dec_res[4];
    Lstm2 lstm_enc, lstm_dec;
    const __half* tail_w = nullptr;
    const float* tail_b = nullptr;
    int tail_k = 7;
    float* probe[4] = {nullptr, nullptr, nullptr, nullptr};
    int last_launches = 0;
    // stage boundaries of a group on the handle's stream, and the last call's time per stage (WAVE_STAGES: normalisation +
    // HiFi-GAN, encoder, encoder LSTM, the two convolutions around the bottleneck, decoder LSTM, decoder + tail)
    hipEvent_t stage_ev[7] = {};
    float stage_ms[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    ~sc_pretssel_wave_model() {
        for (hipEvent_t e : stage_ev)
            if (e) (void)hipEventDestroy(e);
    }
};

namespace {

constexpr int WAVE_STREAM_K = 7, WAVE_RES_K = 3;
constexpr int64_t WAVE_GROUP_SAMPLES = 1ll << 22;

struct WaveLoader : Loader {  // what is the waveform generator's own
    using Loader::Loader;
    // weight-normed weight [d0][d1][k] with g [d0][1][1] -> folded fp32 (scratch of the pool)
    Buf<float> folded(const std::string& p, int d0, int d1, int k) {
        const __half* v = f16(p + ".weight_v", {d0, d1, k}, /*keep=*/false);
        const __half* g = f16(p + ".weight_g", {d0, 1, 1}, /*keep=*/false);
        Buf<float> f(m.pp(), (size_t)d0 * d1 * k);
        launch_weight_norm_fold(v, g, f, d0, d1 * k, m.stream);
        return f;
    }
    SConv sconv(const std::string& p, int cin, int cout, int k, int stride, bool transposed) {
        SC_CHECK(transposed ? (k == 2 * stride && (size_t)cin * 5 * 4 <= 48 * 1024) : sconv_supported(cin, cout, k, stride),
                 "%s: '%s' %d -> %d k=%d stride=%d is outside the convolution kernels' limits", who, p.c_str(), cin, cout, k, stride);
        SConv c;
        c.cin = cin, c.cout = cout, c.k = k, c.stride = stride;
        Buf<float> f = transposed ? folded(p, cin, cout, k) : folded(p, cout, cin, k);
        __half* wt = static_cast<__half*>(dalloc((size_t)k * cin * cout * 2));
        launch_pack_sconv_weight(f, wt, cin, cout, k, transposed, m.stream);
        c.wt = wt;
        c.b = f32(p + ".bias", {cout});
        return c;
    }
    // [cout][cin][k] folded -> fp16 rows [cout][k * cin] (tap-major)
    const __half* packed_rows(const std::string& p, int cout, int cin, int k) {
        Buf<float> f = folded(p, cout, cin, k);
        Buf<__half> h(m.pp(), (size_t)cout * cin * k);
        launch_cvt_f32_f16(f, h, (int64_t)cout * cin * k, m.stream);
        __half* d = static_cast<__half*>(dalloc((size_t)cout * cin * k * 2));
        launch_pack_conv_weight(h, d, cout, cin, k, cin * k, m.stream);
        return d;
    }
    SRes res(const std::string& p, int C) {
        SC_CHECK(C >= 2 && C % 2 == 0, "%s: residual block at %d channels", who, C);
        SRes r;
        r.C = C;
        const std::string p1 = p + ".block.1.conv.conv", p2 = p + ".block.3.conv.conv";
        if (seanet_resblock_supported(C)) {
            r.w1 = packed_rows(p1, C / 2, C, WAVE_RES_K);
            r.w2 = packed_rows(p2, C, C / 2, 1);
            r.c1.b = f32(p1 + ".bias", {C / 2});
            r.c2.b = f32(p2 + ".bias", {C});
        } else {
            r.c1 = sconv(p1, C, C / 2, WAVE_RES_K, 1, false);
            r.c2 = sconv(p2, C / 2, C, 1, 1, false);
        }
        return r;
    }
    Lstm2 lstm(const std::string& p, int H) {
        Lstm2 w;
        w.H = H;
        w.wih0 = f16(p + ".weight_ih_l0", {4 * H, H});
        w.whh0 = f16(p + ".weight_hh_l0", {4 * H, H});
        const __half* wih1 = f16(p + ".weight_ih_l1", {4 * H, H}, /*keep=*/false);
        const __half* whh1 = f16(p + ".weight_hh_l1", {4 * H, H}, /*keep=*/false);
        __half* w1 = static_cast<__half*>(dalloc((size_t)4 * H * 2 * H * 2));  // [W_ih1 | W_hh1]
        SC_HIP(hipMemcpy2DAsync(w1, (size_t)2 * H * 2, wih1, (size_t)H * 2, (size_t)H * 2, (size_t)4 * H, hipMemcpyDeviceToDevice, m.stream));
        SC_HIP(hipMemcpy2DAsync(w1 + H, (size_t)2 * H * 2, whh1, (size_t)H * 2, (size_t)H * 2, (size_t)4 * H, hipMemcpyDeviceToDevice, m.stream));
        w.w1 = w1;
        w.b_ih0 = f32(p + ".bias_ih_l0", {4 * H});
        w.b_hh0 = f32(p + ".bias_hh_l0", {4 * H});
        w.b_ih1 = f32(p + ".bias_ih_l1", {4 * H});
        w.b_hh1 = f32(p + ".bias_hh_l1", {4 * H});
        return w;
    }
};

void check_wave_config(const sc_pretssel_wave_config& c) {
    SC_CHECK(c.mel_dim >= 4 && c.mel_dim % 4 == 0 && c.mel_dim <= 128, "sc_pretssel_wave_load: mel_dim=%d must be a multiple of 4 up to 128", c.mel_dim);
    SC_CHECK(c.post_layers >= 0 && c.post_layers <= 64, "sc_pretssel_wave_load: post_layers=%d outside 0..64", c.post_layers);
    SC_CHECK(c.num_upsamples >= 1 && c.num_upsamples <= SC_MAX_UPSAMPLES, "sc_pretssel_wave_load: %d upsamples outside 1..%d", c.num_upsamples, SC_MAX_UPSAMPLES);
    SC_CHECK(c.upsample_initial_channel >= (4 << c.num_upsamples) && c.upsample_initial_channel % (1 << c.num_upsamples) == 0 && c.upsample_initial_channel <= 4096,
             "sc_pretssel_wave_load: upsample_initial_channel=%d with %d upsamples", c.upsample_initial_channel, c.num_upsamples);
    int64_t hop = 1;
    for (int i = 0; i < c.num_upsamples; ++i) {
        SC_CHECK(c.upsample_rates[i] >= 1 && c.upsample_rates[i] <= 16 && c.upsample_kernel_sizes[i] == 2 * c.upsample_rates[i],
                 "sc_pretssel_wave_load: upsample %d: rate %d, kernel %d (kernel = 2 * rate, rate 1..16)", i, c.upsample_rates[i], c.upsample_kernel_sizes[i]);
        hop *= c.upsample_rates[i];
    }
    SC_CHECK(hop <= 4096, "sc_pretssel_wave_load: hop %lld above 4096", (long long)hop);
    for (int j = 0; j < 3; ++j) {
        SC_CHECK(c.resblock_kernel_sizes[j] >= 1 && c.resblock_kernel_sizes[j] % 2 == 1 && c.resblock_kernel_sizes[j] <= 31,
                 "sc_pretssel_wave_load: ResBlock kernel %d must be odd and at most 31", c.resblock_kernel_sizes[j]);
        for (int d = 0; d < 3; ++d)
            SC_CHECK(c.resblock_dilation_sizes[j][d] >= 1 && c.resblock_dilation_sizes[j][d] <= 16, "sc_pretssel_wave_load: dilation %d outside 1..16",
                     c.resblock_dilation_sizes[j][d]);
    }
    SC_CHECK(c.n_filters >= 2 && lstm2_supported(16 * c.n_filters), "sc_pretssel_wave_load: n_filters=%d: 16 * n_filters must be a multiple of 32 up to 2048",
             c.n_filters);
    for (int i = 0; i < 4; ++i) SC_CHECK(c.ratios[i] >= 1 && c.ratios[i] <= 16, "sc_pretssel_wave_load: ratio %d outside 1..16", c.ratios[i]);
    SC_CHECK(c.dimension >= 1 && c.dimension <= 1024, "sc_pretssel_wave_load: dimension=%d outside 1..1024", c.dimension);
}

void load_wave(sc_pretssel_wave_model& a, const sc_tensor_desc* t, size_t n) {
    const sc_pretssel_wave_config& c = a.cfg;
    check_wave_config(c);
    Model& m = a.m;
    const int P = c.post_layers, U = c.num_upsamples, F = c.n_filters;
    const auto layer = [](int i) { return "layers." + std::to_string(i); };
    const int chunk[4] = {P, P + 9, P + 17 + U, P + 25 + 4 * U};
    const auto stream = [&](int i) { return layer(chunk[i / 8] + i % 8); };
    WaveLoader L(m, "sc_pretssel_wave_load", t, n);
    // ---- the HiFi-GAN: the unit vocoder's Model fields and loaders ----
    sc_config& v = m.cfg;
    v.voc_num_upsamples = U;
    v.voc_upsample_initial_channel = c.upsample_initial_channel;
    v.voc_num_resblock_kernels = 3;
    v.voc_num_resblock_dilations = 3;
    v.voc_embedding_dim = c.mel_dim;  // conv_pre's input width (the row cap's widest-row term)
    a.hop = 1;
    for (int i = 0; i < U; ++i) {
        v.voc_upsample_rates[i] = c.upsample_rates[i];
        v.voc_upsample_kernel_sizes[i] = c.upsample_kernel_sizes[i];
        a.hop *= c.upsample_rates[i];
    }
    HifiganNames nm;
    nm.pre = layer(P + 8);
    nm.post = layer(P + 33 + 4 * U);
    for (int i = 0; i < U; ++i) nm.ups.push_back(layer(P + 17 + i));
    for (int j = 0; j < 3; ++j) {
        v.voc_resblock_kernel_sizes[j] = c.resblock_kernel_sizes[j];
        for (int d = 0; d < 3; ++d) v.voc_resblock_dilation_sizes[j][d] = c.resblock_dilation_sizes[j][d];
    }
    for (int i = 0; i < 3 * U; ++i) nm.res.push_back(layer(P + 25 + U + i));
    load_hifigan_stack(L, nm, c.mel_dim);
    SC_CHECK(hifigan_packed_row_cap(m, a.hop) > 0, "sc_pretssel_wave_load: a HiFi-GAN stage has a shape no packed-item kernel takes");
    // ---- normalisation ----
    a.mean = L.f32("mean", {c.mel_dim});
    a.scale = L.f32("scale", {c.mel_dim});
    {
        std::vector<float> sc_h((size_t)c.mel_dim);
        SC_HIP(hipStreamSynchronize(m.stream));
        SC_HIP(hipMemcpy(sc_h.data(), a.scale, sc_h.size() * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < c.mel_dim; ++i) SC_CHECK(sc_h[i] != 0.f && std::isfinite(sc_h[i]), "sc_pretssel_wave_load: scale[%d] = %g", i, (double)sc_h[i]);
    }
    // ---- SEANet: stream layer 0 the first convolution; 1 + 3j / 3 + 3j the encoder's blocks; 13 / 17 the LSTMs; 15 / 16 the
    // convolutions around the bottleneck; 19 + 3j / 20 + 3j the decoder's blocks; 31 the last convolution ----
    a.first = L.sconv(stream(0) + ".conv.conv", 1, F, WAVE_STREAM_K, 1, false);
    int C = F;
    for (int j = 0; j < 4; ++j) {
        const int r = c.ratios[3 - j];
        a.enc_res[j] = L.res(stream(1 + 3 * j), C);
        a.enc_down[j] = L.sconv(stream(3 + 3 * j) + ".conv.conv", C, 2 * C, 2 * r, r, false);
        C *= 2;
    }
    a.lstm_enc = L.lstm(stream(13) + ".lstm", C);
    a.enc_out = L.sconv(stream(15) + ".conv.conv", C, c.dimension, WAVE_STREAM_K, 1, false);
    a.dec_in = L.sconv(stream(16) + ".conv.conv", c.dimension, C, WAVE_STREAM_K, 1, false);
    a.lstm_dec = L.lstm(stream(17) + ".lstm", C);
    for (int j = 0; j < 4; ++j) {
        const int r = c.ratios[j];
        a.dec_up[j] = L.sconv(stream(19 + 3 * j) + ".convtr.convtr", C, C / 2, 2 * r, r, true);
        C /= 2;
        a.dec_res[j] = L.res(stream(20 + 3 * j), C);
    }
    SC_CHECK(seanet_tail_supported(F, WAVE_STREAM_K), "sc_pretssel_wave_load: n_filters=%d is above the tail kernel's limit", F);
    a.tail_w = L.packed_rows(stream(31) + ".conv.conv", 1, F, WAVE_STREAM_K);
    a.tail_b = L.f32(stream(31) + ".conv.conv.bias", {1});
    a.tail_k = WAVE_STREAM_K;
    L.release_unused();
}

// lengths of one item of `samples` samples: the encoder's four levels down (ceil), the decoder's four levels up
void wave_lens(const sc_pretssel_wave_config& c, int64_t samples, int64_t enc[5], int64_t dec[5]) {
    enc[0] = samples;
    for (int j = 0; j < 4; ++j) enc[j + 1] = (enc[j] + c.ratios[3 - j] - 1) / c.ratios[3 - j];
    dec[0] = enc[4];
    for (int j = 0; j < 4; ++j) dec[j + 1] = dec[j] * c.ratios[j];
}

struct WaveRun {
    sc_pretssel_wave_model& a;
    Model& m;
    int n = 0;
    const int* d_tab = nullptr;  // level tables [n + 1] each: 0 frames, 1..5 encoder levels, 6..9 decoder levels 1..4
    std::vector<int> tab;
    int launches = 0;
    const int* off(int level) const { return d_tab + (size_t)level * (n + 1); }
    int total(int level) const { return tab[(size_t)level * (n + 1) + n]; }
    int longest(int level) const {
        int l = 0;
        for (int i = 0; i < n; ++i) l = std::max(l, tab[(size_t)level * (n + 1) + i + 1] - tab[(size_t)level * (n + 1) + i]);
        return l;
    }
    Buf<float> conv(const float* x, const SConv& c, int in_level, int out_level, int in_act, bool transposed, const float* res = nullptr) {
        Buf<float> y(m.pp(), (size_t)total(out_level) * c.cout);
        SconvArgs s;
        s.x = x, s.wt = c.wt, s.bias = c.b, s.res = res, s.y = y;
        s.in_off = off(in_level), s.out_off = off(out_level);
        s.n = n, s.longest_out = longest(out_level);
        s.cin = c.cin, s.cout = c.cout, s.k = c.k, s.stride = c.stride;
        s.left = (c.k - c.stride) - (c.k - c.stride) / 2;
        s.in_act = in_act;
        if (transposed) launch_sconvtr(s, m.stream);
        else launch_sconv(s, m.stream);
        ++launches;
        return y;
    }
    Buf<float> res(const float* x, const SRes& r, int level) {
        if (r.w1) {
            Buf<float> y(m.pp(), (size_t)total(level) * r.C);
            SeanetResArgs s;
            s.x = x, s.w1 = r.w1, s.b1 = r.c1.b, s.w2 = r.w2, s.b2 = r.c2.b, s.y = y;
            s.row_off = off(level), s.n = n, s.longest = longest(level), s.C = r.C;
            launch_seanet_resblock(s, m.stream);
            ++launches;
            return y;
        }
        Buf<float> t = conv(x, r.c1, level, level, SEANET_IN_ELU, false);
        return conv(t, r.c2, level, level, SEANET_IN_ELU, false, x);
    }
    Buf<float> lstm(const float* x, const Lstm2& w, int level) {
        const size_t rows = (size_t)total(level), H = (size_t)w.H;
        Buf<float> y(m.pp(), rows * H), xproj(m.pp(), rows * 4 * H), h0(m.pp(), rows * H), h1(m.pp(), rows * H), c(m.pp(), (size_t)2 * n * H);
        launches += run_lstm2(w, x, off(level), n, (int)rows, longest(level), xproj, h0, h1, c, y, nullptr, m.stream);
        return y;
    }
};

void run_wave_group(sc_pretssel_wave_model& a, const float* d_mel, int t_cap, const int32_t* frames, int n, float* d_wav, int wav_cap, int flags, bool probes) {
    Model& m = a.m;
    const sc_pretssel_wave_config& c = a.cfg;
    WaveRun R{a, m};
    R.n = n;
    R.tab.assign((size_t)10 * (n + 1), 0);
    for (int i = 0; i < n; ++i) {
        int64_t enc[5], dec[5];
        wave_lens(c, (int64_t)frames[i] * a.hop, enc, dec);
        const int64_t lens[10] = {frames[i], enc[0], enc[1], enc[2], enc[3], enc[4], dec[1], dec[2], dec[3], dec[4]};
        for (int l = 0; l < 10; ++l) R.tab[(size_t)l * (n + 1) + i + 1] = R.tab[(size_t)l * (n + 1) + i] + (int)lens[l];
    }
    // run_wave's checks bound every table below 2^31: a group holds at most WAVE_GROUP_SAMPLES = 2^22 samples, and a level adds at
    // most the product of the ratios (16^4) per item of rounding, 2^26 at 1024 items.  The kernels index elements with 64 bits.
    Buf<int> d_tab(m.pp(), R.tab.size());
    const auto mark = [&](int i) {
        if (!a.stage_ev[i]) SC_HIP(hipEventCreate(&a.stage_ev[i]));
        SC_HIP(hipEventRecord(a.stage_ev[i], m.stream));
    };
    mark(0);
    SC_HIP(hipMemcpyAsync(d_tab.get(), R.tab.data(), R.tab.size() * sizeof(int), hipMemcpyHostToDevice, m.stream));
    R.d_tab = d_tab.get();
    // ---- mel rows -> normalise -> HiFi-GAN (conv_post without the tanh): skip [samples] ----
    PackedItems pk;
    pk.n = n;
    pk.off.assign(R.tab.begin(), R.tab.begin() + n + 1);
    pk.d_off = R.off(0);
    Buf<float> skip(m.pp(), (size_t)R.total(1));
    {
        Buf<float> rows(m.pp(), (size_t)pk.rows() * c.mel_dim);
        launch_mel_norm_pack(d_mel, a.mean, a.scale, pk.d_off, n, pk.longest(), t_cap, c.mel_dim, rows, m.stream);
        run_hifigan_rows(m, rows, pk, skip, (flags & 1) ? 5 : 0);
    }
    const auto probe = [&](int which, const float* src, size_t count) {
        if (probes && a.probe[which]) SC_HIP(hipMemcpyAsync(a.probe[which], src, count * sizeof(float), hipMemcpyDeviceToDevice, m.stream));
    };
    probe(0, skip, (size_t)R.total(1));
    mark(1);
    // ---- SEANet encoder ----
    Buf<float> x = R.conv(skip, a.first, 1, 1, SEANET_IN_TANH, false);
    for (int j = 0; j < 4; ++j) {
        x = R.res(x, a.enc_res[j], 1 + j);
        x = R.conv(x, a.enc_down[j], 1 + j, 2 + j, SEANET_IN_ELU, false);
    }
    mark(2);
    x = R.lstm(x, a.lstm_enc, 5);
    mark(3);
    probe(1, x, (size_t)R.total(5) * a.lstm_enc.H);
    x = R.conv(x, a.enc_out, 5, 5, SEANET_IN_ELU, false);
    // ---- decoder: on the rounded-up lengths, nothing trimmed until the tail ----
    x = R.conv(x, a.dec_in, 5, 5, SEANET_IN_NONE, false);
    mark(4);
    x = R.lstm(x, a.lstm_dec, 5);
    mark(5);
    probe(2, x, (size_t)R.total(5) * a.lstm_dec.H);
    for (int j = 0; j < 4; ++j) {
        x = R.conv(x, a.dec_up[j], 5 + j, 6 + j, SEANET_IN_ELU, true);
        x = R.res(x, a.dec_res[j], 6 + j);
    }
    probe(3, x, (size_t)R.total(9) * c.n_filters);
    SeanetTailArgs t;
    t.h = x, t.w = a.tail_w, t.bias = a.tail_b, t.skip = skip, t.wav = d_wav;
    t.in_off = R.off(9), t.out_off = R.off(1);
    t.wav_stride = wav_cap, t.n = n, t.longest_out = R.longest(1), t.cin = c.n_filters, t.k = a.tail_k;
    launch_seanet_tail(t, m.stream);
    a.last_launches += R.launches + 2;  // + the normalisation and the tail
    mark(6);
    SC_HIP(hipStreamSynchronize(m.stream));  // R.tab is the source of an asynchronous copy
    for (int i = 0; i < 6; ++i) {
        float ms = 0.f;
        SC_HIP(hipEventElapsedTime(&ms, a.stage_ev[i], a.stage_ev[i + 1]));
        a.stage_ms[i] += ms;
    }
}

void run_wave(sc_pretssel_wave_model& a, const float* d_mel, int n, int t_cap, const int32_t* frames, float* d_wav, int wav_cap, int32_t* h_wav_lens, int flags) {
    SC_CHECK(n >= 1 && n <= WAVE_MAX_ITEMS && t_cap >= 1 && wav_cap >= 1, "sc_pretssel_wave: n=%d (1..%d) t_cap=%d wav_cap=%d", n, WAVE_MAX_ITEMS, t_cap, wav_cap);
    SC_CHECK((flags & ~1) == 0, "sc_pretssel_wave: flags=%d", flags);
    for (int i = 0; i < n; ++i) {
        SC_CHECK(frames[i] >= 1 && frames[i] <= t_cap, "sc_pretssel_wave: item %d has %d frames (1..t_cap=%d)", i, frames[i], t_cap);
        SC_CHECK((int64_t)frames[i] * a.hop <= wav_cap && (int64_t)frames[i] * a.hop <= WAVE_GROUP_SAMPLES,
                 "sc_pretssel_wave: item %d: %d frames * hop %d is above wav_cap=%d or %lld", i, frames[i], a.hop, wav_cap, (long long)WAVE_GROUP_SAMPLES);
    }
    Model& m = a.m;
    a.last_launches = 0;
    for (float& v : a.stage_ms) v = 0.f;
    SC_HIP(hipMemsetAsync(d_wav, 0, (size_t)n * wav_cap * sizeof(float), m.stream));
    // groups of consecutive items of at most WAVE_GROUP_SAMPLES samples (and the HiFi-GAN's own row cap); an item's bits do not
    // depend on the grouping: every kernel works from the item's own rows
    const int64_t budget = std::min<int64_t>(WAVE_GROUP_SAMPLES / a.hop, hifigan_packed_row_cap(m, a.hop));
    std::vector<int> need(frames, frames + n);
    const std::vector<int> first = plan_packed_groups(need, std::max<int64_t>(budget, 1));
    const bool one_group = first.size() == 2;
    for (size_t g = 0; g + 1 < first.size(); ++g)
        run_wave_group(a, d_mel + (size_t)first[g] * t_cap * a.cfg.mel_dim, t_cap, frames + first[g], first[g + 1] - first[g], d_wav + (size_t)first[g] * wav_cap, wav_cap,
                       flags, one_group);
    for (float*& p : a.probe) p = nullptr;
    if (h_wav_lens)
        for (int i = 0; i < n; ++i) h_wav_lens[i] = frames[i] * a.hop;
}

}  // namespace

extern "C" {

sc_pretssel_wave_model* sc_pretssel_wave_load(const sc_tensor_desc* tensors, size_t n_tensors, const sc_pretssel_wave_config* cfg, int device) {
    return open_handle<sc_pretssel_wave_model>("sc_pretssel_wave_load", tensors, n_tensors, cfg, device, load_wave);
}

void sc_pretssel_wave_free(sc_pretssel_wave_model* p) { free_handle(p); }

int sc_pretssel_wave(sc_pretssel_wave_model* p, const float* d_mel, int32_t n, int32_t t_cap, const int32_t* h_frame_lens, float* d_wav, int32_t wav_cap,
                     int32_t* h_wav_lens_or_null, int32_t flags) {
    SC_API_BEGIN
    SC_CHECK(p && d_mel && h_frame_lens && d_wav, "sc_pretssel_wave: null argument");
    SC_HIP(hipSetDevice(p->m.device));
    run_wave(*p, d_mel, n, t_cap, h_frame_lens, d_wav, wav_cap, h_wav_lens_or_null, flags);
    SC_API_END
}

int sc_op_pretssel_wave_probe(sc_pretssel_wave_model* p, float* d_hifi, float* d_lstm_enc, float* d_lstm_dec, float* d_dec) {
    SC_API_BEGIN
    SC_CHECK(p, "sc_op_pretssel_wave_probe: null handle");
    p->probe[0] = d_hifi, p->probe[1] = d_lstm_enc, p->probe[2] = d_lstm_dec, p->probe[3] = d_dec;
    SC_API_END
}

int sc_op_pretssel_wave_lens(sc_pretssel_wave_model* p, int32_t frames, int32_t* h_steps, int32_t* h_dec_len) {
    SC_API_BEGIN
    SC_CHECK(p && h_steps && h_dec_len && frames >= 1 && (int64_t)frames * p->hop <= WAVE_GROUP_SAMPLES, "sc_op_pretssel_wave_lens: bad argument");
    int64_t enc[5], dec[5];
    wave_lens(p->cfg, (int64_t)frames * p->hop, enc, dec);
    *h_steps = (int32_t)enc[4];
    *h_dec_len = (int32_t)dec[4];
    SC_API_END
}

int32_t sc_op_pretssel_wave_last_launches(sc_pretssel_wave_model* p) { return p ? p->last_launches : -1; }

int sc_op_pretssel_wave_stage_ms(sc_pretssel_wave_model* p, float* h_ms6) {
    SC_API_BEGIN
    SC_CHECK(p && h_ms6, "sc_op_pretssel_wave_stage_ms: null argument");
    std::copy(p->stage_ms, p->stage_ms + 6, h_ms6);
    SC_API_END
}

int sc_op_lstm2(const float* d_x, const int32_t* h_lens, int32_t n, int32_t H, const void* d_wih0_f16, const void* d_whh0_f16, const float* d_b_ih0,
                const float* d_b_hh0, const void* d_wih1_f16, const void* d_whh1_f16, const float* d_b_ih1, const float* d_b_hh1, float* d_y,
                float* d_max_pre_or_null, int32_t* h_launches_or_null) {
    SC_API_BEGIN
    SC_CHECK(d_x && d_wih0_f16 && d_whh0_f16 && d_b_ih0 && d_b_hh0 && d_wih1_f16 && d_whh1_f16 && d_b_ih1 && d_b_hh1 && d_y, "sc_op_lstm2: null argument");
    SC_CHECK(lstm2_supported(H), "sc_op_lstm2: H=%d must be a multiple of 32 up to 2048", H);
    std::vector<int> off;
    const int longest = offsets_of("sc_op_lstm2", h_lens, n, off);
    const int rows = off[n];
    SC_CHECK((int64_t)rows * 4 * H < (1ll << 31), "sc_op_lstm2: %d rows at H=%d", rows, H);
    OpScratch sc_;
    Lstm2 w;
    w.H = H;
    w.wih0 = static_cast<const __half*>(d_wih0_f16);
    w.whh0 = static_cast<const __half*>(d_whh0_f16);
    // layer 1's two matrices side by side: [4H][2H]
    __half* w1 = sc_.get<__half>((size_t)4 * H * 2 * H);
    SC_HIP(hipMemcpy2D(w1, (size_t)2 * H * 2, d_wih1_f16, (size_t)H * 2, (size_t)H * 2, (size_t)4 * H, hipMemcpyDeviceToDevice));
    SC_HIP(hipMemcpy2D(w1 + H, (size_t)2 * H * 2, d_whh1_f16, (size_t)H * 2, (size_t)H * 2, (size_t)4 * H, hipMemcpyDeviceToDevice));
    w.w1 = w1;
    w.b_ih0 = d_b_ih0;
    w.b_hh0 = d_b_hh0;
    w.b_ih1 = d_b_ih1;
    w.b_hh1 = d_b_hh1;
    if (d_max_pre_or_null) SC_HIP(hipMemset(d_max_pre_or_null, 0, sizeof(float)));
    const int launches = run_lstm2(w, d_x, sc_.put(off), n, rows, longest, sc_.get<float>((size_t)rows * 4 * H), sc_.get<float>((size_t)rows * H),
                                   sc_.get<float>((size_t)rows * H), sc_.get<float>((size_t)2 * n * H), d_y, d_max_pre_or_null, nullptr);
    if (h_launches_or_null) *h_launches_or_null = launches;
    SC_HIP(hipStreamSynchronize(nullptr));
    SC_API_END
}

int32_t sc_op_seanet_resblock_tile(void) { return SEANET_RES_TILE; }

int sc_op_seanet_resblock(const float* d_x, const int32_t* h_lens, int32_t n, int32_t C, const void* d_w1_f16, const float* d_b1, const void* d_w2_f16,
                          const float* d_b2, float* d_y) {
    SC_API_BEGIN
    SC_CHECK(d_x && d_w1_f16 && d_b1 && d_w2_f16 && d_b2 && d_y, "sc_op_seanet_resblock: null argument");
    SC_CHECK(seanet_resblock_supported(C), "sc_op_seanet_resblock: C=%d (32 or 64)", C);
    std::vector<int> off;
    const int longest = offsets_of("sc_op_seanet_resblock", h_lens, n, off);
    OpScratch sc_;
    __half* w1 = sc_.get<__half>((size_t)(C / 2) * 3 * C);
    launch_pack_conv_weight(static_cast<const __half*>(d_w1_f16), w1, C / 2, C, 3, 3 * C, nullptr);
    SeanetResArgs a;
    a.x = d_x;
    a.w1 = w1;
    a.b1 = d_b1;
    a.w2 = static_cast<const __half*>(d_w2_f16);  // [C][C/2][1] is [C][C/2]
    a.b2 = d_b2;
    a.y = d_y;
    a.row_off = sc_.put(off);
    a.n = n;
    a.longest = longest;
    a.C = C;
    launch_seanet_resblock(a, nullptr);
    SC_HIP(hipStreamSynchronize(nullptr));
    SC_API_END
}

int sc_op_sconv(const float* d_x, const int32_t* h_lens, int32_t n, int32_t cin, int32_t cout, int32_t k, int32_t stride, int32_t transposed,
                int32_t in_act, const float* d_w, const float* d_bias, const float* d_res_or_null, float* d_y, int32_t* h_out_lens) {
    SC_API_BEGIN
    SC_CHECK(d_x && d_w && d_bias && d_y && h_out_lens, "sc_op_sconv: null argument");
    SC_CHECK(in_act >= SEANET_IN_NONE && in_act <= SEANET_IN_TANH, "sc_op_sconv: in_act=%d", in_act);
    SC_CHECK(transposed ? (cin >= 1 && cout >= 1 && stride >= 1 && k == 2 * stride && !d_res_or_null) : sconv_supported(cin, cout, k, stride),
             "sc_op_sconv: cin=%d cout=%d k=%d stride=%d is not supported%s", cin, cout, k, stride, transposed ? " (transposed: k = 2 * stride, no residual)" : "");
    std::vector<int> in_off, out_lens(n > 0 ? (size_t)n : 0), out_off;
    offsets_of("sc_op_sconv", h_lens, n, in_off);
    for (int i = 0; i < n; ++i) {
        SC_CHECK((int64_t)h_lens[i] * stride < (1 << 24), "sc_op_sconv: lens[%d]=%d", i, h_lens[i]);
        out_lens[i] = transposed ? h_lens[i] * stride : cdiv(h_lens[i], stride);
    }
    const int longest_out = offsets_of("sc_op_sconv", out_lens.data(), n, out_off);
    std::copy(out_lens.begin(), out_lens.end(), h_out_lens);
    OpScratch sc_;
    __half* wt = sc_.get<__half>((size_t)k * cin * cout);
    launch_pack_sconv_weight(d_w, wt, cin, cout, k, transposed != 0, nullptr);
    SconvArgs a;
    a.x = d_x;
    a.wt = wt;
    a.bias = d_bias;
    a.res = d_res_or_null;
    a.y = d_y;
    a.in_off = sc_.put(in_off);
    a.out_off = sc_.put(out_off);
    a.n = n;
    a.longest_out = longest_out;
    a.cin = cin;
    a.cout = cout;
    a.k = k;
    a.stride = stride;
    a.left = (k - stride) - (k - stride) / 2;  // padding_total = k - stride, the smaller half on the right
    a.in_act = in_act;
    if (transposed) launch_sconvtr(a, nullptr);
    else launch_sconv(a, nullptr);
    SC_HIP(hipStreamSynchronize(nullptr));
    SC_API_END
}

int sc_op_seanet_tail(const float* d_h, const int32_t* h_dec_lens, const int32_t* h_out_lens, int32_t n, int32_t cin, int32_t k, const void* d_w_f16,
                      const float* d_bias, const float* d_skip, float* d_wav, int64_t wav_stride) {
    SC_API_BEGIN
    SC_CHECK(d_h && d_w_f16 && d_bias && d_skip && d_wav && wav_stride >= 0, "sc_op_seanet_tail: bad argument");
    SC_CHECK(seanet_tail_supported(cin, k), "sc_op_seanet_tail: cin=%d k=%d", cin, k);
    std::vector<int> in_off, out_off;
    offsets_of("sc_op_seanet_tail", h_dec_lens, n, in_off);
    const int longest_out = offsets_of("sc_op_seanet_tail", h_out_lens, n, out_off);
    for (int i = 0; i < n; ++i)
        SC_CHECK(h_out_lens[i] <= h_dec_lens[i] && (!wav_stride || h_out_lens[i] <= wav_stride), "sc_op_seanet_tail: item %d keeps %d of %d samples (row of %lld)", i,
                 h_out_lens[i], h_dec_lens[i], (long long)wav_stride);
    OpScratch sc_;
    __half* w = sc_.get<__half>((size_t)k * cin);
    launch_pack_conv_weight(static_cast<const __half*>(d_w_f16), w, 1, cin, k, k * cin, nullptr);
    SeanetTailArgs a;
    a.h = d_h;
    a.w = w;
    a.bias = d_bias;
    a.skip = d_skip;
    a.wav = d_wav;
    a.in_off = sc_.put(in_off);
    a.out_off = sc_.put(out_off);
    a.wav_stride = wav_stride;
    a.n = n;
    a.longest_out = longest_out;
    a.cin = cin;
    a.k = k;
    launch_seanet_tail(a, nullptr);
    SC_HIP(hipStreamSynchronize(nullptr));
    SC_API_END
}

}  // extern "C"
