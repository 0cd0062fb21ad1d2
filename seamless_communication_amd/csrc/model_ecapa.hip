// ProsodyEncoder: the ECAPA-TDNN of SeamlessExpressive.  A handle of its own (separate checkpoint, stream and scratch pool)
// and its C entries, after the pattern of model_align.hip / model_w2v2.hip.
//
// Reference call sites (src/seamless_communication/models/pretssel/...):
//   ecapa_tdnn_builder.py      arch `base`
//   ecapa_tdnn.py:111-143      ECAPA_TDNN.forward;  :191-195 TDNNBlock (Conv1d, ReLU, LayerNorm over the channels, no mask)
//   ecapa_tdnn.py:250-263      Res2NetBlock;  :296-309 SEBlock;  :466-477 SERes2NetBlock;  :341-394 AttentiveStatisticsPooling
//
// A call is 32 launches at `base` (33 with gcmvn): per TDNN block a product and the ReLU + LayerNorm pass (2), per SE-Res2Net
// block tdnn1 (2), the fused chain (1), tdnn2 (2), the gate (1), gate * y + residual into the concat slice (1); the aggregation
// (2); pooling: statistics, per-item bias, product, ReLU + LayerNorm + tanh, product, soft-max statistics (6); the tail (1).
#include <algorithm>
#include <cmath>
#include <string>

#include "handle.h"
#include "loader.h"

using namespace sc;

namespace {
struct Tdnn {
    Conv conv;
    LNorm norm;
};
struct SeRes2Net {
    Tdnn tdnn1, tdnn2;
    std::vector<Tdnn> chain;
    const __half* se_w1 = nullptr;  // [se][C]
    const float* se_b1 = nullptr;
    const __half* se_w2 = nullptr;  // [C][se]
    const float* se_b2 = nullptr;
    int dil = 1;
};
}  // namespace

struct sc_prosody_encoder {
    Model m;
    sc_prosody_encoder_config cfg{};
    Tdnn first, mfa, asp_tdnn;
    std::vector<SeRes2Net> blocks;
    Conv asp_conv;
    LNorm asp_norm;
    const __half* fc_w = nullptr;  // [embed][2 C]
    const float* fc_b = nullptr;
    int last_launches = 0;
};

namespace {

constexpr int PE_MAX_FRAMES = 4096;

Tdnn load_tdnn(Loader& L, const std::string& p, int cout, int cin, int k) {
    Tdnn t;
    t.conv = L.conv(p + ".conv", cout, cin, k);
    t.norm = L.ln(p + ".norm", cout);
    return t;
}

void check_config(const sc_prosody_encoder_config& c) {
    SC_CHECK(c.n_blocks >= 3 && c.n_blocks <= SC_PE_MAX_BLOCKS, "sc_prosody_encoder_load: n_blocks=%d outside 3..%d", c.n_blocks, SC_PE_MAX_BLOCKS);
    SC_CHECK(c.input_dim >= 1 && c.input_dim <= 4096 && c.embed_dim >= 1 && c.embed_dim <= 4096 && c.se_channels >= 1 && c.se_channels <= 1024 &&
                 c.attention_channels >= 1 && c.attention_channels <= 4096,
             "sc_prosody_encoder_load: input_dim=%d embed_dim=%d se_channels=%d attention_channels=%d out of range", c.input_dim, c.embed_dim,
             c.se_channels, c.attention_channels);
    SC_CHECK(c.global_context == 1, "sc_prosody_encoder_load: global_context=%d: only the global-context pooling (1) is built", c.global_context);
    const int C = c.channels[0], nb = c.n_blocks;
    SC_CHECK(C >= 32 && C % 32 == 0 && C <= 4096, "sc_prosody_encoder_load: channels[0]=%d must be a multiple of 32 up to 4096", C);
    SC_CHECK(c.kernel_sizes[0] >= 1 && c.kernel_sizes[0] % 2 == 1 && c.kernel_sizes[0] <= 15 && c.dilations[0] >= 1 && c.dilations[0] <= 8,
             "sc_prosody_encoder_load: first block kernel=%d (odd, <= 15) dilation=%d (1..8)", c.kernel_sizes[0], c.dilations[0]);
    SC_CHECK(c.res2net_scale >= 2 && c.res2net_scale <= ECAPA_MAX_SCALE && C % c.res2net_scale == 0, "sc_prosody_encoder_load: res2net_scale=%d outside 2..%d or not a divisor of %d",
             c.res2net_scale, ECAPA_MAX_SCALE, C);
    for (int i = 1; i < nb - 1; ++i) {
        SC_CHECK(c.channels[i] == C, "sc_prosody_encoder_load: channels[%d]=%d != channels[0]=%d (the shortcut convolution is not built)", i, c.channels[i], C);
        SC_CHECK(ecapa_chain_supported(C / c.res2net_scale, c.res2net_scale, c.kernel_sizes[i], c.dilations[i]),
                 "sc_prosody_encoder_load: block %d: the Res2Net chain kernel has chunk widths 32 and 64 (got %d), kernel 3 (got %d), dilations 1..8 (got %d)", i,
                 C / c.res2net_scale, c.kernel_sizes[i], c.dilations[i]);
    }
    SC_CHECK(c.channels[nb - 1] == (nb - 2) * C && c.kernel_sizes[nb - 1] == 1 && c.dilations[nb - 1] == 1,
             "sc_prosody_encoder_load: the aggregation must have %d channels (got %d), kernel 1 and dilation 1", (nb - 2) * C, c.channels[nb - 1]);
    SC_CHECK((size_t)(2 * c.channels[nb - 1] + c.embed_dim) * 4 <= 60 * 1024, "sc_prosody_encoder_load: %d pooled values + %d outputs exceed the tail kernel's 60 KiB of LDS",
             2 * c.channels[nb - 1], c.embed_dim);
}

void load_prosody_encoder(sc_prosody_encoder& a, const sc_tensor_desc* t, size_t n) {
    const sc_prosody_encoder_config& c = a.cfg;
    check_config(c);
    const int C = c.channels[0], nb = c.n_blocks, CM = c.channels[nb - 1], w = C / c.res2net_scale;
    Loader L(a.m, "sc_prosody_encoder_load", t, n);
    a.first = load_tdnn(L, "blocks.0", C, c.input_dim, c.kernel_sizes[0]);
    for (int i = 1; i < nb - 1; ++i) {
        const std::string p = "blocks." + std::to_string(i);
        SeRes2Net b;
        b.dil = c.dilations[i];
        b.tdnn1 = load_tdnn(L, p + ".tdnn1", C, C, 1);
        for (int j = 0; j + 1 < c.res2net_scale; ++j) b.chain.push_back(load_tdnn(L, p + ".res2net_block.blocks." + std::to_string(j), w, w, c.kernel_sizes[i]));
        b.tdnn2 = load_tdnn(L, p + ".tdnn2", C, C, 1);
        b.se_w1 = L.f16(p + ".se_block.conv1.weight", {c.se_channels, C, 1});
        b.se_b1 = L.f32(p + ".se_block.conv1.bias", {c.se_channels});
        b.se_w2 = L.f16(p + ".se_block.conv2.weight", {C, c.se_channels, 1});
        b.se_b2 = L.f32(p + ".se_block.conv2.bias", {C});
        a.blocks.push_back(std::move(b));
    }
    a.mfa = load_tdnn(L, "mfa", CM, CM, 1);
    a.asp_tdnn = load_tdnn(L, "asp.tdnn", c.attention_channels, 3 * CM, 1);
    a.asp_conv = L.conv("asp.conv", CM, c.attention_channels, 1);
    a.asp_norm = L.ln("asp_norm", 2 * CM);
    a.fc_w = L.f16("fc.weight", {c.embed_dim, 2 * CM, 1});
    a.fc_b = L.f32("fc.bias", {c.embed_dim});
    L.release_unused();
}

// y[rows][ldc] = x[rows][lda] (*) conv (implicit convolution, 'same' padding) + bias (nullable); K = the first `cin_used` input
// channels of a k = 1 weight row when cin_used > 0
void product(sc_prosody_encoder& a, const float* x, int64_t lda, const Conv& c, bool bias, float* y, int64_t ldc, int nb, int T, int dil,
             const int* d_in_lens, int cin_used = 0) {
    GemmArgs g;
    g.A = x;
    g.lda = lda;
    g.W = c.w;
    g.ldw = c.kpad;
    g.bias = bias ? c.b : nullptr;
    g.C = y;
    g.ldc = ldc;
    g.M = nb * T;
    g.N = c.cout;
    g.K = cin_used ? cin_used : c.kpad;
    g.rows_per_batch = T;
    g.t_in = T;
    g.t_out = T;
    g.taps = c.k;
    g.cin = cin_used ? cin_used : c.cin;
    g.dil = dil;
    g.stride = 1;
    g.pad = dil * (c.k - 1) / 2;
    g.in_lens = d_in_lens;
    launch_gemm(g, a.m.stream);
    ++a.last_launches;
}

void tdnn(sc_prosody_encoder& a, const float* x, int64_t lda, const Tdnn& t, float* y, int64_t ldc, int nb, int T, int dil, const int* d_in_lens = nullptr) {
    product(a, x, lda, t.conv, true, y, ldc, nb, T, dil, d_in_lens);
    launch_ecapa_relu_ln(y, ldc, nullptr, 0, t.norm.g, t.norm.b, y, ldc, nb * T, t.conv.cout, ACT_NONE, a.m.stream);
    ++a.last_launches;
}

void check_lens(const char* who, const int32_t* lens, int n, int T) {
    if (!lens) return;
    for (int b = 0; b < n; ++b) SC_CHECK(lens[b] >= 1 && lens[b] <= T, "%s: lens[%d]=%d outside 1..%d", who, b, lens[b], T);
}

void run_prosody_encode(sc_prosody_encoder& a, const float* d_fbank, int n, int T, const int32_t* h_lens, const float* d_mean, const float* d_std,
                        float* d_out) {
    Model& m = a.m;
    const sc_prosody_encoder_config& c = a.cfg;
    // ---- every refusal before the first launch ----
    SC_CHECK(n >= 1 && n <= 4096, "sc_prosody_encode: n=%d outside 1..4096", n);
    SC_CHECK(T >= 1 && T <= PE_MAX_FRAMES, "sc_prosody_encode: t_rows=%d outside 1..%d frames", T, PE_MAX_FRAMES);
    SC_CHECK((d_mean == nullptr) == (d_std == nullptr), "sc_prosody_encode: gcmvn mean and std must be given together");
    check_lens("sc_prosody_encode", h_lens, n, T);
    const int C = c.channels[0], nbk = c.n_blocks, CM = c.channels[nbk - 1], A = c.attention_channels, D = c.input_dim;
    SC_CHECK((int64_t)n * T * CM < (1ll << 31), "sc_prosody_encode: batch too large (n=%d t_rows=%d)", n, T);
    prof::set_tag("ecapa");
    a.last_launches = 0;
    const int rows = n * T;
    Buf<int> d_lens;
    if (h_lens) {
        d_lens = Buf<int>(m.pp(), n);
        SC_HIP(hipMemcpyAsync(d_lens.get(), h_lens, (size_t)n * 4, hipMemcpyHostToDevice, m.stream));
    }
    const int* lens = h_lens ? d_lens.get() : nullptr;
    // ---- first TDNN block; rows behind an item's length are read as zeros (after gcmvn, when given) ----
    Buf<float> xn;
    const float* in = d_fbank;
    const int* in_lens = lens;
    if (d_mean) {
        xn = Buf<float>(m.pp(), (size_t)rows * D);
        launch_ecapa_gcmvn(d_fbank, d_mean, d_std, lens, n, T, D, xn, m.stream);
        ++a.last_launches;
        in = xn;
        in_lens = nullptr;
    }
    Buf<float> x0(m.pp(), (size_t)rows * C), cat(m.pp(), (size_t)rows * CM), u(m.pp(), (size_t)rows * C), v(m.pp(), (size_t)rows * C);
    Buf<float> gate(m.pp(), (size_t)n * C);
    tdnn(a, in, D, a.first, x0, C, n, T, c.dilations[0], in_lens);
    // ---- SE-Res2Net blocks, each into its slice of the concat buffer ----
    const float* xin = x0;
    int64_t ldin = C;
    for (size_t i = 0; i < a.blocks.size(); ++i) {
        const SeRes2Net& b = a.blocks[i];
        tdnn(a, xin, ldin, b.tdnn1, u, C, n, T, 1);
        EcapaChainArgs ch;
        ch.x = u;
        ch.ldx = C;
        ch.out = v;
        ch.ldo = C;
        ch.ldw = b.chain[0].conv.kpad;
        for (size_t j = 0; j < b.chain.size(); ++j) {
            ch.w[j] = b.chain[j].conv.w;
            ch.bias[j] = b.chain[j].conv.b;
            ch.gamma[j] = b.chain[j].norm.g;
            ch.beta[j] = b.chain[j].norm.b;
        }
        ch.nb = n;
        ch.T = T;
        ch.CW = C / c.res2net_scale;
        ch.scale = c.res2net_scale;
        ch.dil = b.dil;
        launch_ecapa_chain(ch, m.stream);
        ++a.last_launches;
        tdnn(a, v, C, b.tdnn2, u, C, n, T, 1);
        launch_ecapa_se_gate(u, C, n, T, lens, C, c.se_channels, b.se_w1, b.se_b1, b.se_w2, b.se_b2, gate, m.stream);
        float* slice = cat.get() + i * C;
        launch_ecapa_se_apply(u, C, gate, xin, ldin, slice, CM, n, T, C, m.stream);
        a.last_launches += 2;
        xin = slice;
        ldin = CM;
    }
    // ---- aggregation ----
    Buf<float> f(m.pp(), (size_t)rows * CM);
    tdnn(a, cat, CM, a.mfa, f, CM, n, T, 1);
    // ---- attentive statistics pooling; the time-constant two thirds of the 3 CM wide product become a per-item bias ----
    Buf<float> gst(m.pp(), (size_t)n * 2 * CM), ib(m.pp(), (size_t)n * A), h(m.pp(), (size_t)rows * A), pooled(m.pp(), (size_t)n * 2 * CM);
    launch_ecapa_gstats(f, n, T, CM, lens, gst, m.stream);
    launch_ecapa_item_bias(a.asp_tdnn.conv.w, a.asp_tdnn.conv.kpad, CM, a.asp_tdnn.conv.b, gst, n, 2 * CM, A, ib, m.stream);
    a.last_launches += 2;
    product(a, f, CM, a.asp_tdnn.conv, false, h, A, n, T, 1, nullptr, CM);
    launch_ecapa_relu_ln(h, A, ib, T, a.asp_tdnn.norm.g, a.asp_tdnn.norm.b, h, A, rows, A, ACT_TANH, m.stream);
    ++a.last_launches;
    float* logits = cat;  // the concat buffer is dead
    product(a, h, A, a.asp_conv, true, logits, CM, n, T, 1, nullptr);
    launch_ecapa_pool(f, logits, n, T, CM, lens, pooled, m.stream);
    launch_ecapa_tail(pooled, n, 2 * CM, a.asp_norm.g, a.asp_norm.b, a.fc_w, 2 * CM, a.fc_b, c.embed_dim, d_out, m.stream);
    a.last_launches += 2;
    SC_HIP(hipStreamSynchronize(m.stream));  // the caller's stream is not ours: the output is complete on return
}

int* op_lens(OpScratch& sc_, const int32_t* h, int n) { return h ? sc_.put(std::vector<int>(h, h + n)) : nullptr; }

}  // namespace

extern "C" {

sc_prosody_encoder* sc_prosody_encoder_load(const sc_tensor_desc* tensors, size_t n_tensors, const sc_prosody_encoder_config* cfg, int device) {
    return open_handle<sc_prosody_encoder>("sc_prosody_encoder_load", tensors, n_tensors, cfg, device, load_prosody_encoder);
}

void sc_prosody_encoder_free(sc_prosody_encoder* p) { free_handle(p); }

int sc_prosody_encode(sc_prosody_encoder* p, const float* d_fbank, int32_t n, int32_t t_rows, const int32_t* h_lens_or_null,
                      const float* d_gcmvn_mean_or_null, const float* d_gcmvn_std_or_null, float* d_out) {
    SC_API_BEGIN
    SC_CHECK(p && d_fbank && d_out, "sc_prosody_encode: null argument");
    SC_HIP(hipSetDevice(p->m.device));
    run_prosody_encode(*p, d_fbank, n, t_rows, h_lens_or_null, d_gcmvn_mean_or_null, d_gcmvn_std_or_null, d_out);
    SC_API_END
}

int32_t sc_op_prosody_last_launches(sc_prosody_encoder* p) { return p ? p->last_launches : -1; }

int32_t sc_op_ecapa_chain_tile(int32_t chunk, int32_t scale, int32_t dil) {
    return ecapa_chain_supported(chunk, scale, 3, dil) ? ecapa_chain_tile_rows(scale, dil) : 0;
}

int sc_op_ecapa_chain(const float* d_x, const void* d_w_f16, const float* d_bias, const float* d_gamma, const float* d_beta, float* d_out, int32_t nb,
                      int32_t T, int32_t chunk, int32_t scale, int32_t dil) {
    SC_API_BEGIN
    SC_CHECK(d_x && d_w_f16 && d_bias && d_gamma && d_beta && d_out, "sc_op_ecapa_chain: null argument");
    SC_CHECK(ecapa_chain_supported(chunk, scale, 3, dil), "sc_op_ecapa_chain: unsupported chunk width %d (32 or 64), scale %d (2..8) or dilation %d (1..8)",
             chunk, scale, dil);
    SC_CHECK(nb > 0 && T > 0 && T <= PE_MAX_FRAMES && (int64_t)nb * T * scale * chunk < (1ll << 31), "sc_op_ecapa_chain: bad geometry");
    OpScratch sc_;
    const int kpad = (int)align_up(3 * chunk, 32);
    __half* packed = sc_.get<__half>((size_t)(scale - 1) * chunk * kpad);
    EcapaChainArgs a;
    for (int j = 0; j + 1 < scale; ++j) {
        launch_pack_conv_weight(static_cast<const __half*>(d_w_f16) + (size_t)j * chunk * chunk * 3, packed + (size_t)j * chunk * kpad, chunk, chunk, 3, kpad,
                                nullptr);
        a.w[j] = packed + (size_t)j * chunk * kpad;
        a.bias[j] = d_bias + j * chunk;
        a.gamma[j] = d_gamma + j * chunk;
        a.beta[j] = d_beta + j * chunk;
    }
    a.x = d_x;
    a.out = d_out;
    a.ldx = a.ldo = (int64_t)scale * chunk;
    a.ldw = kpad;
    a.nb = nb;
    a.T = T;
    a.CW = chunk;
    a.scale = scale;
    a.dil = dil;
    launch_ecapa_chain(a, nullptr);
    SC_HIP(hipStreamSynchronize(nullptr));
    SC_API_END
}

int sc_op_ecapa_relu_ln(const float* d_x, const float* d_item_bias, int32_t t_per_item, const float* d_gamma, const float* d_beta, float* d_y,
                        int32_t rows, int32_t C, int32_t act) {
    SC_API_BEGIN
    SC_CHECK(d_x && d_gamma && d_beta && d_y, "sc_op_ecapa_relu_ln: null argument");
    launch_ecapa_relu_ln(d_x, C, d_item_bias, t_per_item, d_gamma, d_beta, d_y, C, rows, C, act, nullptr);
    SC_HIP(hipStreamSynchronize(nullptr));
    SC_API_END
}

int sc_op_ecapa_se_gate(const float* d_x, int32_t nb, int32_t T, const int32_t* h_lens, int32_t C, int32_t S, const void* d_w1_f16, const float* d_b1,
                        const void* d_w2_f16, const float* d_b2, float* d_gate) {
    SC_API_BEGIN
    SC_CHECK(d_x && d_w1_f16 && d_b1 && d_w2_f16 && d_b2 && d_gate && nb > 0 && T > 0, "sc_op_ecapa_se_gate: null argument");
    check_lens("sc_op_ecapa_se_gate", h_lens, nb, T);
    OpScratch sc_;
    launch_ecapa_se_gate(d_x, C, nb, T, op_lens(sc_, h_lens, nb), C, S, static_cast<const __half*>(d_w1_f16), d_b1, static_cast<const __half*>(d_w2_f16), d_b2,
                         d_gate, nullptr);
    SC_HIP(hipStreamSynchronize(nullptr));
    SC_API_END
}

int sc_op_ecapa_pool(const float* d_x, const float* d_logits, int32_t nb, int32_t T, int32_t C, const int32_t* h_lens, float* d_pooled, float* d_gstats) {
    SC_API_BEGIN
    SC_CHECK(d_x && nb > 0 && T > 0 && C > 0 && (!d_pooled || d_logits), "sc_op_ecapa_pool: null argument");
    check_lens("sc_op_ecapa_pool", h_lens, nb, T);
    OpScratch sc_;
    const int* lens = op_lens(sc_, h_lens, nb);
    if (d_gstats) launch_ecapa_gstats(d_x, nb, T, C, lens, d_gstats, nullptr);
    if (d_pooled) launch_ecapa_pool(d_x, d_logits, nb, T, C, lens, d_pooled, nullptr);
    SC_HIP(hipStreamSynchronize(nullptr));
    SC_API_END
}

int sc_op_ecapa_tail(const float* d_pooled, int32_t nb, int32_t C2, const float* d_gamma, const float* d_beta, const void* d_w_f16, const float* d_bias,
                     int32_t E, float* d_out) {
    SC_API_BEGIN
    SC_CHECK(d_pooled && d_gamma && d_beta && d_w_f16 && d_bias && d_out, "sc_op_ecapa_tail: null argument");
    launch_ecapa_tail(d_pooled, nb, C2, d_gamma, d_beta, static_cast<const __half*>(d_w_f16), C2, d_bias, E, d_out, nullptr);
    SC_HIP(hipStreamSynchronize(nullptr));
    SC_API_END
}

}  // extern "C"
