// UnitExtractor: wav2vec 2.0 (XLS-R) layer output + k-means units.  A handle of its own (separate checkpoint, stream and
// scratch pool) and its C entries, after the pattern of model_align.hip.
//
// Reference call sites (src/seamless_communication/models/unit_extractor/...):
//   unit_extractor.py:91-98         collate (pad to even with 1.0), F.layer_norm over the utterance, model, k-means
//   wav2vec2_layer_output.py:23-53  the xlsr2_1b_v2 architecture;  :89-119 the output of layer out_layer_idx, later layers not run
//   kmeans.py:24-30                 argmin_j |x|^2 - 2 x.c_j + |c_j|^2
// Tensor names are fairseq2's (models/conformer_shaw/loader.py:44-71 gives the fairseq -> fairseq2 map of the shared parts).
#include <algorithm>
#include <cmath>
#include <string>

#include "handle.h"
#include "loader.h"

using namespace sc;

struct sc_unit_extractor {
    Model m;
    sc_unit_extractor_config cfg{};
    const float* c0_w = nullptr;  // first extractor layer [C][k] fp32
    const float* c0_b = nullptr;
    std::vector<LNorm> fe_ln;     // one per extractor layer
    std::vector<Conv> fe_conv;    // layers 1 .. (index 0 unused)
    LNorm post_ln;
    Linear proj;
    const float* pos_w = nullptr;  // packed [group][tap][c_in][c_out] fp32
    const float* pos_b = nullptr;
    std::vector<EncoderLayer> layers;
    const __half* km_w = nullptr;  // [K][2 model_dim] = [c_hi | c_lo]
    const float* km_bias = nullptr;  // -|c|^2 / 2
};

namespace {

constexpr int UE_MAX_FRAMES = 4096;

void check_config(const sc_unit_extractor_config& c) {
    SC_CHECK(c.model_dim > 0 && c.heads > 0 && c.model_dim % c.heads == 0 && (c.model_dim / c.heads == 64 || c.model_dim / c.heads == 80),
             "sc_unit_extractor_load: model_dim=%d heads=%d (the head dimension must be 64 or 80)", c.model_dim, c.heads);
    SC_CHECK(c.model_dim % 32 == 0 && c.ffn_dim > 0 && c.ffn_dim % 32 == 0 && c.layers >= 1 && c.layers <= 256,
             "sc_unit_extractor_load: model_dim=%d ffn_dim=%d (multiples of 32) layers=%d", c.model_dim, c.ffn_dim, c.layers);
    SC_CHECK(c.feature_dim > 0 && c.feature_dim % 32 == 0 && c.feature_dim <= 1024, "sc_unit_extractor_load: feature_dim=%d (multiple of 32, <= 1024)",
             c.feature_dim);
    SC_CHECK(c.fe_layers >= 1 && c.fe_layers <= SC_UE_MAX_FE_LAYERS, "sc_unit_extractor_load: %d extractor layers outside 1..%d", c.fe_layers,
             SC_UE_MAX_FE_LAYERS);
    for (int i = 0; i < c.fe_layers; ++i)
        SC_CHECK(c.fe_kernel[i] >= 1 && c.fe_kernel[i] <= 16 && c.fe_stride[i] >= 1 && c.fe_stride[i] <= 64,
                 "sc_unit_extractor_load: extractor layer %d has kernel %d / stride %d", i, c.fe_kernel[i], c.fe_stride[i]);
    SC_CHECK(c.pos_conv_groups > 0 && c.model_dim % c.pos_conv_groups == 0 && c.model_dim / c.pos_conv_groups <= 128 && c.pos_conv_kernel >= 2 &&
                 c.pos_conv_kernel % 2 == 0 && c.pos_conv_kernel <= 256,
             "sc_unit_extractor_load: position conv kernel=%d (even, <= 256) groups=%d (<= 128 channels each)", c.pos_conv_kernel, c.pos_conv_groups);
    SC_CHECK(c.num_centroids >= 1, "sc_unit_extractor_load: num_centroids=%d", c.num_centroids);
}

void load_unit_extractor(sc_unit_extractor& a, const sc_tensor_desc* t, size_t n) {
    const sc_unit_extractor_config& c = a.cfg;
    check_config(c);
    const int M = c.model_dim, F = c.feature_dim;
    Loader L(a.m, "sc_unit_extractor_load", t, n);
    const std::string fe = "encoder_frontend.feature_extractor.layers.";
    a.c0_w = L.f32(fe + "0.conv.weight", {F, 1, c.fe_kernel[0]});
    a.c0_b = L.f32(fe + "0.conv.bias", {F});
    a.fe_conv.resize(c.fe_layers);
    for (int i = 0; i < c.fe_layers; ++i) {
        a.fe_ln.push_back(L.ln(fe + std::to_string(i) + ".layer_norm", F));
        if (i > 0) a.fe_conv[i] = L.conv(fe + std::to_string(i) + ".conv", F, F, c.fe_kernel[i]);
    }
    a.post_ln = L.ln("encoder_frontend.post_extract_layer_norm", F);
    a.proj = L.lin("encoder_frontend.model_dim_proj", M, F);
    {
        // the weight-norm (dim = 2) is folded by the caller: "weight" is g * v / |v| in fp32
        const int cg = M / c.pos_conv_groups, K = c.pos_conv_kernel;
        const float* w = L.f32("encoder_frontend.pos_encoder.conv.weight", {M, cg, K}, /*keep=*/false);
        float* packed = static_cast<float*>(L.dalloc((size_t)M * cg * K * 4));
        launch_w2v2_pack_pos_weight(w, packed, M, c.pos_conv_groups, K, a.m.stream);
        a.pos_w = packed;
        a.pos_b = L.f32("encoder_frontend.pos_encoder.conv.bias", {M});
    }
    for (int i = 0; i < c.layers; ++i) {
        const std::string p = "encoder.layers." + std::to_string(i);
        EncoderLayer l;
        l.attn_ln = L.ln(p + ".self_attn_layer_norm", M);
        l.qkv = L.fuse({p + ".self_attn.q_proj", p + ".self_attn.k_proj", p + ".self_attn.v_proj"}, M, M);
        l.attn_out = L.lin(p + ".self_attn.output_proj", M, M);
        l.ffn_ln = L.ln(p + ".ffn_layer_norm", M);
        l.ffn_in = L.lin(p + ".ffn.inner_proj", c.ffn_dim, M);
        l.ffn_out = L.lin(p + ".ffn.output_proj", M, c.ffn_dim);
        a.layers.push_back(l);
    }
    {
        const int K = c.num_centroids;
        const float* cent = L.f32("kmeans.centroids", {M, K}, /*keep=*/false);  // the reference's transposed layout (kmeans.py:19)
        __half* w = static_cast<__half*>(L.dalloc((size_t)K * 2 * M * 2));
        float* b = static_cast<float*>(L.dalloc((size_t)K * 4));
        launch_w2v2_pack_centroids(cent, M, K, w, b, a.m.stream);
        a.km_w = w;
        a.km_bias = b;
    }
    L.release_unused();
}

// frames of `num_samples` samples behind the first `upto` extractor layers: floor((L - k) / s) + 1 each, 0 once a layer's
// input is shorter than its kernel
int ue_frames(const sc_unit_extractor_config& c, int64_t num_samples, int upto) {
    int64_t L = num_samples;
    for (int i = 0; i < upto; ++i) {
        if (L < c.fe_kernel[i]) return 0;
        L = (L - c.fe_kernel[i]) / c.fe_stride[i] + 1;
    }
    return (int)std::min<int64_t>(L, 1 << 30);
}

// arg-min of the k-means distance of `rows` feature rows [rows][C] as the fused arg-max of x.c - |c|^2 / 2
void kmeans_units(DevicePool* pool, const float* x, int rows, int C, const __half* km_w, const float* km_bias, int K, int* d_idx, hipStream_t s) {
    Buf<__half> hi(pool, (size_t)rows * 2 * C), lo(pool, (size_t)rows * 2 * C);
    launch_w2v2_dup_split(x, C, rows, C, hi, lo, s);
    const int nch = gemm_presplit_amax_chunks(rows, K);
    Buf<float2> part(pool, (size_t)rows * nch);
    GemmPsArgs g;
    g.Ah = hi;
    g.Al = lo;
    g.lda = 2 * C;
    g.W = km_w;
    g.ldw = 2 * C;
    g.bias = km_bias;
    g.M = rows;
    g.N = K;
    g.K = 2 * C;
    g.amax = part;
    g.amax_ld = nch;
    launch_gemm_presplit(g, s);
    launch_amax_finish(part, nch, rows, d_idx, s);
}

void run_extract_units(sc_unit_extractor& a, const float* h_wav, int n, int64_t wav_stride, const int32_t* h_ns, int out_layer_idx, int32_t* h_units,
                       int max_frames, int32_t* h_frames, float* d_features) {
    Model& m = a.m;
    const sc_unit_extractor_config& c = a.cfg;
    const int M = c.model_dim, F = c.feature_dim;
    // ---- every refusal before the first launch ----
    SC_CHECK(n > 0 && n <= 4096, "sc_extract_units: n=%d outside 1..4096", n);
    SC_CHECK(out_layer_idx >= 0 && out_layer_idx < c.layers, "sc_extract_units: out_layer_idx=%d outside 0..%d", out_layer_idx, c.layers - 1);
    std::vector<int32_t> frames(n);
    int TF = 0;
    int64_t max_ns = 0;
    for (int b = 0; b < n; ++b) {
        SC_CHECK(h_ns[b] >= 1 && (int64_t)h_ns[b] <= wav_stride, "sc_extract_units: num_samples[%d]=%d outside 1..stride=%lld", b, h_ns[b],
                 (long long)wav_stride);
        frames[b] = ue_frames(c, h_ns[b], c.fe_layers);
        SC_CHECK(frames[b] >= 1, "sc_extract_units: item %d has %d samples, too few for one frame", b, h_ns[b]);
        SC_CHECK(frames[b] <= UE_MAX_FRAMES, "sc_extract_units: item %d has %d frames, the limit is %d per item", b, frames[b], UE_MAX_FRAMES);
        TF = std::max(TF, frames[b]);
        max_ns = std::max<int64_t>(max_ns, h_ns[b]);
    }
    SC_CHECK(max_frames >= TF, "sc_extract_units: max_frames=%d < %d frames of the longest item", max_frames, TF);
    std::vector<int> T(c.fe_layers);
    for (int i = 0; i < c.fe_layers; ++i) T[i] = ue_frames(c, max_ns, i + 1);
    SC_CHECK((int64_t)n * T[0] * F < (1ll << 31) && (int64_t)n * TF * std::max(3 * M, c.ffn_dim) < (1ll << 31),
             "sc_extract_units: batch too large (n=%d, %lld samples)", n, (long long)max_ns);
    prof::set_tag("w2v2");

    // ---- waveform, statistics, first layer ----
    const int64_t dstride = align_up(max_ns, 4);
    Buf<float> d_wav(m.pp(), (size_t)n * dstride), d_stats(m.pp(), 2 * (size_t)n);
    Buf<int> d_ns(m.pp(), n), d_frames(m.pp(), n);
    SC_HIP(hipMemcpy2DAsync(d_wav.get(), (size_t)dstride * 4, h_wav, (size_t)wav_stride * 4, (size_t)max_ns * 4, n, hipMemcpyHostToDevice, m.stream));
    SC_HIP(hipMemcpyAsync(d_ns.get(), h_ns, (size_t)n * 4, hipMemcpyHostToDevice, m.stream));
    SC_HIP(hipMemcpyAsync(d_frames.get(), frames.data(), (size_t)n * 4, hipMemcpyHostToDevice, m.stream));
    launch_w2v2_wave_stats(d_wav, dstride, d_ns, n, d_stats, m.stream);
    Buf<float> x(m.pp(), (size_t)n * T[0] * F);
    launch_w2v2_conv0(d_wav, dstride, d_ns, d_stats, n, a.c0_w, a.c0_b, a.fe_ln[0].g, a.fe_ln[0].b, F, c.fe_kernel[0], c.fe_stride[0], x, T[0],
                      m.stream);
    // ---- extractor layers 1 ..: implicit-convolution product, then LayerNorm + GELU.  Rows behind an item's own frame count
    // are computed from whatever lies there (finite) and masked below ----
    for (int i = 1; i < c.fe_layers; ++i) {
        Buf<float> y(m.pp(), (size_t)n * T[i] * F);
        conv1d(m, x, a.fe_conv[i], nullptr, y, n, T[i - 1], c.fe_stride[i], 0, 1, nullptr, IN_NONE, ACT_NONE);
        layernorm(m, y, a.fe_ln[i], y, n * T[i], ACT_GELU);
        x = std::move(y);
    }
    // ---- projection; padded rows zero in front of it and again (on read) in front of the position convolution ----
    const int rows = n * TF;
    Buf<float> h(m.pp(), (size_t)rows * std::max(M, F)), xp(m.pp(), (size_t)rows * M), xs(m.pp(), (size_t)rows * M);
    launch_layernorm(x, F, a.post_ln.g, a.post_ln.b, h, F, rows, F, ACT_NONE, d_frames, TF, m.stream);
    linear(m, h, F, a.proj, nullptr, 0, xp, M, rows, ACT_NONE, 1.f, /*row_independent=*/true);
    launch_w2v2_pos_conv(xp, a.pos_w, a.pos_b, xs, n, TF, M, c.pos_conv_groups, c.pos_conv_kernel, d_frames, m.stream);
    // ---- pre-norm Transformer layers 0 .. out_layer_idx; the chosen layer's raw output is the result ----
    const int wideN = std::max(3 * M, c.ffn_dim);
    Buf<float> wide(m.pp(), (size_t)rows * wideN), att(m.pp(), (size_t)rows * M);
    float* xr = xs;
    BatchRows br;
    br.n = n, br.S = TF, br.rows = rows, br.d_lens = d_frames;
    for (int i = 0; i <= out_layer_idx; ++i) encoder_layer(m, a.layers[i], br, c.heads, M / c.heads, ACT_GELU, true, xr, h, wide, att);
    if (d_features) SC_HIP(hipMemcpyAsync(d_features, xr, (size_t)rows * M * 4, hipMemcpyDeviceToDevice, m.stream));
    // ---- k-means ----
    Buf<int> d_idx(m.pp(), rows);
    kmeans_units(m.pp(), xr, rows, M, a.km_w, a.km_bias, c.num_centroids, d_idx, m.stream);
    std::vector<int32_t> idx(rows);
    SC_HIP(hipMemcpyAsync(idx.data(), d_idx.get(), (size_t)rows * 4, hipMemcpyDeviceToHost, m.stream));
    SC_HIP(hipStreamSynchronize(m.stream));
    for (int b = 0; b < n; ++b) {
        h_frames[b] = frames[b];
        for (int t = 0; t < max_frames; ++t) h_units[(size_t)b * max_frames + t] = t < frames[b] ? idx[(size_t)b * TF + t] : 0;
    }
}

}  // namespace

extern "C" {

sc_unit_extractor* sc_unit_extractor_load(const sc_tensor_desc* tensors, size_t n_tensors, const sc_unit_extractor_config* cfg, int device) {
    return open_handle<sc_unit_extractor>("sc_unit_extractor_load", tensors, n_tensors, cfg, device, load_unit_extractor);
}

void sc_unit_extractor_free(sc_unit_extractor* u) { free_handle(u); }

int32_t sc_unit_extractor_num_frames(const sc_unit_extractor_config* cfg, int64_t num_samples) {
    if (!cfg || num_samples < 0 || cfg->fe_layers < 1 || cfg->fe_layers > SC_UE_MAX_FE_LAYERS) return -1;
    return ue_frames(*cfg, num_samples, cfg->fe_layers);
}

int sc_extract_units(sc_unit_extractor* u, const float* h_wav, int32_t n, int64_t wav_stride, const int32_t* h_num_samples, int32_t out_layer_idx,
                     int32_t* h_units, int32_t max_frames, int32_t* h_frames, float* d_features_or_null) {
    SC_API_BEGIN
    SC_CHECK(u && h_wav && h_num_samples && h_units && h_frames, "sc_extract_units: null argument");
    SC_HIP(hipSetDevice(u->m.device));
    run_extract_units(*u, h_wav, n, wav_stride, h_num_samples, out_layer_idx, h_units, max_frames, h_frames, d_features_or_null);
    SC_API_END
}

int sc_op_attention_hd(const float* d_q, const float* d_k, const float* d_v, float* d_out, int32_t nb, int32_t heads, int32_t sq, int32_t skv,
                       int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, const int32_t* d_kv_lens, int32_t head_dim) {
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
    a.head_dim = head_dim;
    launch_attention(a, nullptr);
    SC_HIP(hipStreamSynchronize(nullptr));
    SC_API_END
}

int sc_op_w2v2_frontend(const float* d_wav, int64_t wav_stride, const int32_t* h_num_samples, int32_t nb, const float* d_w, const float* d_bias,
                        const float* d_gamma, const float* d_beta, int32_t C, int32_t k, int32_t stride, float* d_out, int32_t t_rows,
                        float* d_stats) {
    SC_API_BEGIN
    SC_CHECK(d_wav && h_num_samples && d_out && d_stats && nb > 0, "sc_op_w2v2_frontend: null argument");
    SC_CHECK(t_rows >= 1, "sc_op_w2v2_frontend: t_rows=%d", t_rows);
    for (int b = 0; b < nb; ++b)
        SC_CHECK(h_num_samples[b] >= 1 && h_num_samples[b] <= wav_stride, "sc_op_w2v2_frontend: num_samples[%d]=%d outside 1..stride", b,
                 h_num_samples[b]);
    OpScratch sc_;
    const int* d_ns = sc_.put(std::vector<int>(h_num_samples, h_num_samples + nb));
    launch_w2v2_wave_stats(d_wav, wav_stride, d_ns, nb, d_stats, nullptr);
    launch_w2v2_conv0(d_wav, wav_stride, d_ns, d_stats, nb, d_w, d_bias, d_gamma, d_beta, C, k, stride, d_out, t_rows, nullptr);
    SC_HIP(hipStreamSynchronize(nullptr));
    SC_API_END
}

int sc_op_w2v2_pos_conv(const float* d_x, const float* d_w, const float* d_bias, float* d_y, int32_t nb, int32_t T, int32_t C, int32_t groups,
                        int32_t k, const int32_t* d_lens) {
    SC_API_BEGIN
    SC_CHECK(d_x && d_w && d_bias && d_y && groups > 0 && C > 0 && C % groups == 0 && k > 0, "sc_op_w2v2_pos_conv: bad argument");
    OpScratch sc_;
    float* packed = sc_.get<float>((size_t)C * (C / groups) * k);
    launch_w2v2_pack_pos_weight(d_w, packed, C, groups, k, nullptr);
    launch_w2v2_pos_conv(d_x, packed, d_bias, d_y, nb, T, C, groups, k, d_lens, nullptr);
    SC_HIP(hipStreamSynchronize(nullptr));
    SC_API_END
}

int sc_op_kmeans(const float* d_x, const float* d_centroids, int32_t rows, int32_t C, int32_t K, int32_t* d_idx) {
    SC_API_BEGIN
    SC_CHECK(d_x && d_centroids && d_idx && rows > 0 && C > 0 && C % 16 == 0 && K > 0, "sc_op_kmeans: bad argument (C must be a multiple of 16)");
    OpScratch sc_;
    __half* w = sc_.get<__half>((size_t)K * 2 * C);
    float* b = sc_.get<float>(K);
    launch_w2v2_pack_centroids(d_centroids, C, K, w, b, nullptr);
    DevicePool pool;
    kmeans_units(&pool, d_x, rows, C, w, b, K, d_idx, nullptr);
    SC_HIP(hipStreamSynchronize(nullptr));
    SC_API_END
}

}  // extern "C"
