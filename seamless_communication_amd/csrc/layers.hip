// Host-side composition shared by the stage passes (model_*.hip): the pre-split product of a Linear, self-attention over a
// q | k | v buffer, and the transformer layers that more than one pass runs.  Launch sequences only; the kernels are in k_*.hip.
#include "model.h"

namespace sc {

void linear_ps(Model& m, Planes a, const Linear& L, int rows, int act, float alpha, const float* res, float* C, Planes out, int split) {
    GemmPsArgs g;
    g.Ah = a.hi;
    g.Al = a.lo;
    g.lda = L.in;
    g.W = L.w;
    g.ldw = L.ldw;
    g.bias = L.b;
    g.res = res;
    g.ldr = L.out;
    g.C = C;
    g.ldc = L.out;
    g.Ch = out.hi;
    g.Cl = out.lo;
    g.ldcs = L.out;
    g.M = rows;
    g.N = L.out;
    g.K = L.in;
    g.act = act;
    g.alpha = alpha;
    g.split = split;
    launch_gemm_presplit(g, m.stream);
}

void self_attention(Model& m, const float* qkv, int M, const BatchRows& b, const SelfAttn& o) {
    AttnArgs a;
    a.q = qkv;
    a.k = qkv + M;
    a.v = qkv + 2 * M;
    a.ldq = a.ldk = a.ldv = 3 * M;
    a.out = o.out;
    a.ldo = M;
    a.out_hi = o.out_p.hi;
    a.out_lo = o.out_p.lo;
    a.ldoh = o.out_p.hi ? M : 0;
    a.nb = b.n;
    a.heads = o.heads;
    a.head_dim = o.head_dim;
    a.Sq = a.Skv = b.S;
    a.kv_lens = b.d_lens;
    a.row_off = b.d_off;
    a.pairs = b.pairs;
    a.causal = o.causal;
    a.rel_k = o.rel_k;
    a.rel_left = o.rel_left;
    a.rel_right = o.rel_right;
    a.rp_table = o.rp_table;
    a.rp_ld = o.rp_table ? M : 0;
    a.q_bias_u = o.q_bias_u;
    a.q_bias_v = o.q_bias_v;
    launch_attention(a, m.stream);
}

bool conformer_layer(Model& m, const ConformerLayer& l, const ConformerLayer* next, const BatchRows& b, const ConformerPass& p, bool ffn1_ready) {
    const sc_config& c = m.cfg;
    const int M = c.model_dim, rows = b.rows, taps = c.depthwise_conv_kernel_size;
    float* x = p.x;
    auto ln_split = [&](const float* src, const LNorm& L, int act) {
        launch_layernorm_split(src, L.dim, L.g, L.b, p.hs.hi, p.hs.lo, L.dim, rows, L.dim, act, nullptr, 1, m.stream);
    };
    auto ps = [&](Planes a, const Linear& L, int act, float alpha, const float* res, float* C, Planes out = {}) {
        linear_ps(m, a, L, rows, act, alpha, res, C, out, p.split);
    };
    // x += 0.5 * FFN1(LN(x))
    if (!ffn1_ready) ln_split(x, l.ffn1_ln, ACT_NONE);
    ps(p.hs, l.ffn1_in, ACT_SILU, 1.f, nullptr, nullptr, p.ws);
    ps(p.ws, l.ffn1_out, ACT_NONE, 0.5f, x, x);
    // x += MHA_shaw(LN(x)) over each item's own rows
    ln_split(x, l.attn_ln, ACT_NONE);
    ps(p.hs, l.qkv, ACT_NONE, 1.f, nullptr, p.wide);
    SelfAttn at;
    at.heads = c.num_heads;
    at.out_p = p.as;
    at.rel_k = l.rel_k;
    at.rel_left = c.shaw_max_left;
    at.rel_right = c.shaw_max_right;
    self_attention(m, p.wide, M, b, at);
    ps(p.as, l.attn_out, ACT_NONE, 1.f, x, x);
    // x += Conv(LN(x))
    ln_split(x, l.conv_ln, ACT_NONE);
    if (p.glu_epi) {
        // the product's epilogue gates: `wide` is [rows][M], the gate half never reaches HBM (131 MB written and read back per
        // layer at 64 x 10 s), and the depthwise kernel loads one value per element instead of two
        GemmPsArgs a;
        a.Ah = p.hs.hi;
        a.Al = p.hs.lo;
        a.lda = M;
        a.W = l.pw1g.w;
        a.ldw = l.pw1g.ldw;
        a.bias = l.pw1g.b;
        a.C = p.wide;
        a.ldc = M;
        a.M = rows;
        a.N = 2 * M;
        a.K = M;
        launch_gemm_presplit_glu(a, m.stream);
    } else {
        ps(p.hs, l.pw1, ACT_NONE, 1.f, nullptr, p.wide);
    }
    const int ldw = p.glu_epi ? M : 2 * M;
    if (b.d_off) {  // packed rows: the fused kernel only
        launch_glu_dwconv_ln_packed(p.wide, ldw, l.dw, l.conv_inner_ln.g, l.conv_inner_ln.b, ACT_SILU, p.hs.hi, p.hs.lo, M, p.d_work, p.n_work,
                                    (double)rows, M, taps, m.stream, /*gated=*/p.glu_epi);
    } else if (p.fuse_conv) {
        launch_glu_dwconv_ln(p.wide, ldw, l.dw, l.conv_inner_ln.g, l.conv_inner_ln.b, ACT_SILU, p.hs.hi, p.hs.lo, M, b.n, b.S, M, taps, b.d_lens,
                             m.stream, /*gated=*/p.glu_epi);
    } else {
        launch_glu_dwconv(p.wide, 2 * M, l.dw, p.att, M, b.n, b.S, M, taps, b.d_lens, m.stream);
        ln_split(p.att, l.conv_inner_ln, ACT_SILU);
    }
    ps(p.hs, l.pw2, ACT_NONE, 1.f, x, x);
    // x += 0.5 * FFN2(LN(x)); x = LN(x)
    ln_split(x, l.ffn2_ln, ACT_NONE);
    ps(p.hs, l.ffn2_in, ACT_SILU, 1.f, nullptr, nullptr, p.ws);
    ps(p.ws, l.ffn2_out, ACT_NONE, 0.5f, x, x);
    if (p.fuse_ln && next) {  // x = LN_final(x) and the next layer's LN_ffn1(x) planes from one read of x
        const LNorm& nx = next->ffn1_ln;
        launch_layernorm2_split(x, M, l.final_ln.g, l.final_ln.b, x, M, nx.g, nx.b, p.hs.hi, p.hs.lo, M, rows, M, m.stream);
        return true;
    }
    layernorm(m, x, l.final_ln, x, rows);
    return false;
}

void adaptor_layer_tail(Model& m, const AdaptorLayer& a, const BatchRows& b, const float* res, float* y, float* aw, float* ah, bool row_independent) {
    const int M = m.cfg.model_dim, Fd = m.cfg.adaptor_ffn_dim, rows = b.rows;
    linear(m, y, M, a.qkv, nullptr, 0, aw, 3 * M, rows, ACT_NONE, 1.f, row_independent);
    SelfAttn at;
    at.heads = m.cfg.num_heads;
    at.out = ah;
    self_attention(m, aw, M, b, at);
    linear(m, ah, M, a.attn_out, res, M, y, M, rows, ACT_NONE, 1.f, row_independent);
    layernorm(m, y, a.ffn_ln, ah, rows);
    linear(m, ah, M, a.ffn_in, nullptr, 0, aw, Fd, rows, m.ffn_act, 1.f, row_independent);
    linear(m, aw, Fd, a.ffn_out, y, M, y, M, rows, ACT_NONE, 1.f, row_independent);
}

void encoder_layer(Model& m, const EncoderLayer& l, const BatchRows& b, int heads, int head_dim, int ffn_act, bool row_independent, float* x,
                   float* h, float* wide, float* att) {
    const int M = l.attn_ln.dim, Fd = l.ffn_in.out, rows = b.rows;
    layernorm(m, x, l.attn_ln, h, rows);
    linear(m, h, M, l.qkv, nullptr, 0, wide, 3 * M, rows, ACT_NONE, 1.f, row_independent);
    SelfAttn at;
    at.heads = heads;
    at.head_dim = head_dim;
    at.out = att;
    self_attention(m, wide, M, b, at);
    linear(m, att, M, l.attn_out, x, M, x, M, rows, ACT_NONE, 1.f, row_independent);
    layernorm(m, x, l.ffn_ln, h, rows);
    linear(m, h, M, l.ffn_in, nullptr, 0, wide, Fd, rows, ffn_act, 1.f, row_independent);
    linear(m, wide, Fd, l.ffn_out, x, M, x, M, rows, ACT_NONE, 1.f, row_independent);
}

int fft_layer_packed(Model& m, const FFTLayer& l, int film_off, const BatchRows& b, const FFTPass& p) {
    const int M = l.attn_ln.dim, R = b.rows;
    linear_ps(m, p.up, l.qkv, R, ACT_NONE, 1.f, nullptr, p.wide);
    SelfAttn at;
    at.heads = p.heads;
    at.head_dim = p.head_dim;
    at.out_p = p.ap;
    self_attention(m, p.wide, M, b, at);
    linear_ps(m, p.ap, l.attn_out, R, ACT_NONE, 1.f, p.u, p.y);
    launch_layernorm_both(p.y, M, l.attn_ln.g, l.attn_ln.b, p.y, M, p.yp.hi, p.yp.lo, M, R, M, ACT_NONE, nullptr, 1, m.stream);
    conv1d_presplit(m, p.yp.hi, p.yp.lo, l.conv1, nullptr, nullptr, p.wp.hi, p.wp.lo, 0, 0, l.conv1.k / 2, 1, nullptr, ACT_RELU, R, p.d_row_pos);
    conv1d_presplit(m, p.wp.hi, p.wp.lo, l.conv2, p.y, p.u, nullptr, nullptr, 0, 0, l.conv2.k / 2, 1, nullptr, ACT_NONE, R, p.d_row_pos);
    if (p.film) {  // conv1d_layer_norm -> FiLM (-> mask: packed rows are all live) in one pass (fft_decoder_layer.py:185-191)
        PretsselLnArgs f;
        f.x = p.u, f.ldx = M, f.g = l.conv_ln.g, f.b = l.conv_ln.b;
        f.film = p.film, f.film_ld = p.film_ld, f.film_off = film_off, f.row_item = p.row_item;
        f.y = p.u, f.ldy = M, f.yh = p.up.hi, f.yl = p.up.lo, f.ldh = M, f.rows = R, f.C = M;
        launch_pretssel_film_ln(f, m.stream);
    } else {
        launch_layernorm_both(p.u, M, l.conv_ln.g, l.conv_ln.b, p.u, M, p.up.hi, p.up.lo, M, R, M, ACT_NONE, nullptr, 1, m.stream);
    }
    return 7;  // QKV, attention, out-projection, LayerNorm, conv, conv, LayerNorm (+ FiLM)
}

}  // namespace sc
