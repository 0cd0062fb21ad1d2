// The sc_op_* test hooks of libseamless_hip.so (declared in include/seamless_hip_internal.h): kernel-level entry points for
// the parity tests, on the default stream, synchronous.  Hooks that read a model handle stay in api.hip; hooks of a model
// with its own entry file live beside it.
#include <atomic>

#include "dstep.h"
#include "handle.h"

using namespace sc;

namespace {
hipStream_t g_op_stream = nullptr;  // ops use the default stream

std::vector<int32_t> op_read_ints(const int32_t* d, size_t n) {  // n ints of device memory, synchronously
    std::vector<int32_t> h(n);
    if (n) SC_HIP(hipMemcpy(h.data(), d, n * 4, hipMemcpyDeviceToHost));
    return h;
}

int op_row_slots(int rows) { return rows <= 32 ? 32 : (rows <= 64 ? 64 : (int)align_up(rows, 32)); }  // StepCtx::rb

// n elements with every byte `byte`: 0 or 0xff (NaN / -1: what a kernel must write, or must not let leak, shows)
template <typename T>
T* op_filled(OpScratch& s, size_t n, int byte) {
    T* p = s.get<T>(n);
    SC_HIP(hipMemsetAsync(p, byte, n * sizeof(T), g_op_stream));
    return p;
}

int* op_device_int(OpScratch& s, int v) {  // the step kernels read their scalar position from the device
    int* d = s.get<int>(4);
    SC_HIP(hipMemcpyAsync(d, &v, 4, hipMemcpyHostToDevice, g_op_stream));
    return d;
}

__half* op_packed_weight(OpScratch& s, const void* d_w_f16, int N, int K) {  // [N][K] fp16 in MFMA fragment order
    __half* wp = s.get<__half>((size_t)packed_weight_halfs(N, K));
    launch_pack_weight(static_cast<const __half*>(d_w_f16), K, N, K, wp, g_op_stream);
    return wp;
}

// fp32 rows [M][K] as the step's split planes / its k-group-major fp32 stream of RB row slots; NaN in the unused slots
struct OpPlanes {
    __half *hi, *lo;
};
OpPlanes op_nan_planes(OpScratch& s, size_t C, int RB) {
    return {op_filled<__half>(s, C * RB, 0xff), op_filled<__half>(s, C * RB, 0xff)};
}
OpPlanes op_planes(OpScratch& s, const float* d_x, int M, int K, int RB) {
    const OpPlanes p = op_nan_planes(s, K, RB);
    launch_rows_to_planes(d_x, K, M, K, RB, p.hi, p.lo, g_op_stream);
    return p;
}
float* op_kgm(OpScratch& s, const float* d_x, int M, int K, int RB) {
    float* xg = op_filled<float>(s, (size_t)K * RB, 0xff);
    launch_rows_to_kgm(d_x, K, M, K, RB, xg, g_op_stream);
    return xg;
}

// n fp32 values split into hi / lo fp16, and the pre-split product of x [M][K] with W [N][K] on them
OpPlanes op_split(OpScratch& s, const float* d_x, size_t n) {
    const OpPlanes p = {s.get<__half>(n), s.get<__half>(n)};
    launch_split_f32(d_x, p.hi, p.lo, (int64_t)n, g_op_stream);
    return p;
}
GemmPsArgs op_presplit_args(OpScratch& s, const float* d_x, const void* d_w_f16, const float* d_bias, int M, int N, int K) {
    const OpPlanes x = op_split(s, d_x, (size_t)M * K);
    GemmPsArgs a;
    a.Ah = x.hi, a.Al = x.lo, a.lda = K;
    a.W = static_cast<const __half*>(d_w_f16), a.ldw = K;
    a.bias = d_bias;
    a.M = M, a.N = N, a.K = K;
    return a;
}

template <typename Args>  // GemmArgs / SkinnyArgs: y [M][N] = alpha * act(x [M][K] . W [N][K]^T + bias) + res
Args op_linear_args(const float* d_x, const void* d_w_f16, const float* d_bias, const float* d_res, float* d_y, int M, int N, int K,
                    int act = ACT_NONE, float alpha = 1.f) {
    Args a;
    a.A = d_x, a.lda = K;
    a.W = static_cast<const __half*>(d_w_f16), a.ldw = K;
    a.bias = d_bias;
    a.res = d_res, a.ldr = N;
    a.C = d_y, a.ldc = N;
    a.M = M, a.N = N, a.K = K;
    a.act = act, a.alpha = alpha;
    return a;
}

ArgmaxEpi op_argmax_epi(float4* part, int tiles, float* eos_logit, const int* d_pos, int min_step_for_eos, int force_eos_step, int pad_idx,
                        int eos_idx, int unk_idx, float unk_penalty) {
    ArgmaxEpi e;
    e.part = part, e.tiles_cap = tiles, e.eos_logit = eos_logit, e.pos = d_pos;
    e.min_step_for_eos = min_step_for_eos, e.force_eos_step = force_eos_step;
    e.pad_idx = pad_idx, e.eos_idx = eos_idx, e.unk_idx = unk_idx, e.unk_penalty = unk_penalty;
    return e;
}

// The greedy state of the three fused arg-max hooks at step `step`: records | eos logit | pos | hist[M][step + 2] | finished |
// out_len, all zero but the position (the records only when zero_part); close() runs the finalize launch into d_idx and
// d_lprob, which starts at zero: the score accumulates the winner's log-probability.
struct OpGreedy {
    ArgmaxEpi am;
    int tiles, M, hist_ld;
    int *hist, *finished, *out_len;
    float* d_lprob;
    void close(int32_t* d_idx) {
        launch_argmax_finalize(am, tiles, M, d_idx, hist, hist_ld, finished, out_len, d_lprob, g_op_stream);
        SC_HIP(hipStreamSynchronize(g_op_stream));
    }
};
OpGreedy op_greedy(OpScratch& s, int tiles, int M, int step, int min_step_for_eos, int force_eos_step, int pad_idx, int eos_idx, int unk_idx,
                   float unk_penalty, float* d_lprob, bool zero_part = false) {
    OpGreedy g;
    g.tiles = tiles, g.M = M, g.hist_ld = step + 2, g.d_lprob = d_lprob;
    float4* part = zero_part ? op_filled<float4>(s, (size_t)tiles * M, 0) : s.get<float4>((size_t)tiles * M);
    float* eos_logit = op_filled<float>(s, M, 0);
    int* ints = op_filled<int>(s, (size_t)4 + (size_t)M * g.hist_ld + 2 * M, 0);
    g.hist = ints + 4, g.finished = g.hist + (size_t)M * g.hist_ld, g.out_len = g.finished + M;
    SC_HIP(hipMemcpyAsync(ints, &step, 4, hipMemcpyHostToDevice, g_op_stream));
    SC_HIP(hipMemsetAsync(d_lprob, 0, (size_t)M * 4, g_op_stream));
    g.am = op_argmax_epi(part, tiles, eos_logit, ints, min_step_for_eos, force_eos_step, pad_idx, eos_idx, unk_idx, unk_penalty);
    return g;
}
}  // namespace

extern "C" {

int32_t sc_op_xattn_rows_tile(int32_t which) { return which == 0 ? XROWS_QT : which == 1 ? XROWS_KC : 0; }

int sc_op_xattn_rows(const float* d_q, int64_t ldq, const float* d_k, int64_t ldk, int32_t n, int32_t s1, int32_t s_enc, int32_t heads,
                     const int32_t* h_enc_lens, const int32_t* h_tok_lens, float* d_xattn) {
    SC_API_BEGIN
    SC_CHECK(d_q && d_k && h_enc_lens && h_tok_lens && d_xattn, "sc_op_xattn_rows: null argument");
    SC_CHECK(n > 0 && s1 > 0 && s_enc > 0, "sc_op_xattn_rows: n=%d s1=%d s_enc=%d", n, s1, s_enc);
    check_xattn_rows_geometry(heads, heads * 64, "sc_op_xattn_rows");
    for (int b = 0; b < n; ++b) {
        SC_CHECK(h_tok_lens[b] >= 2 && h_tok_lens[b] <= s1 + 1, "sc_op_xattn_rows: tok_lens[%d]=%d outside [2, %d]", b, h_tok_lens[b], s1 + 1);
        SC_CHECK(h_enc_lens[b] > 0 && h_enc_lens[b] <= s_enc, "sc_op_xattn_rows: enc_lens[%d]=%d out of range", b, h_enc_lens[b]);
    }
    OpScratch scratch;
    int* d_lens = scratch.get<int>((size_t)2 * n);
    SC_HIP(hipMemcpy(d_lens, h_enc_lens, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    SC_HIP(hipMemcpy(d_lens + n, h_tok_lens, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    XattnRowsArgs a;
    a.q = d_q, a.k = d_k, a.ldq = ldq, a.ldk = ldk;
    a.enc_lens = d_lens, a.tok_lens = d_lens + n;
    a.xattn = d_xattn;
    a.n = n, a.S1 = s1, a.s_enc = s_enc, a.heads = heads;
    launch_xattn_rows(a, nullptr);
    SC_HIP(hipStreamSynchronize(nullptr));
    SC_API_END
}

// --------------------------------------------------------------------------- //
// kernel-level entry points for the parity tests (default stream, synchronous)
// --------------------------------------------------------------------------- //
// test hook: an unknown name (a typo in a script) answers with the default instead of taking the process down
int sc_op_knob(const char* name, int dflt) { return sc::knob::known(name) ? sc::knob::value(name, dflt) : dflt; }

static std::atomic<int> g_op_single{0};
int sc_op_single_plane(int on) {
    g_op_single.store(on ? 1 : 0);
    return SC_OK;
}

// host planning of the packed vocoder pass (no device work)
int32_t sc_op_voc_pack_plan(const int32_t* h_need, int32_t n, int64_t budget_rows, int32_t* h_group_first, int32_t cap) {
    try {
        SC_CHECK(h_need && n > 0 && budget_rows > 0 && (h_group_first || cap == 0) && cap >= 0, "sc_op_voc_pack_plan: bad argument");
        const std::vector<int> first = sc::plan_packed_groups(std::vector<int>(h_need, h_need + n), budget_rows);
        for (size_t i = 0; i < first.size() && i < (size_t)cap; ++i) h_group_first[i] = first[i];
        return (int32_t)first.size() - 1;
    } catch (const sc::Error& e) {
        return e.code;
    }
}
int32_t sc_op_voc_tile_first(const int32_t* h_off, int32_t n, int32_t mul, int32_t tile_rows, int32_t* h_first) {
    try {
        SC_CHECK(h_off && h_first && n > 0 && mul > 0 && tile_rows > 0, "sc_op_voc_tile_first: bad argument");
        const std::vector<int> first = sc::packed_tile_first(std::vector<int>(h_off, h_off + n + 1), mul, tile_rows);
        for (int i = 0; i <= n; ++i) h_first[i] = first[i];
        return SC_OK;
    } catch (const sc::Error& e) {
        return e.code;
    }
}

int sc_op_force_general_gemm(int on) {
    sc::g_force_general_gemm.store(on ? 1 : 0);
    return SC_OK;
}

int sc_op_layernorm(const float* d_x, const float* d_gamma, const float* d_beta, float* d_y, int32_t rows, int32_t C,
                    int32_t act) {
    SC_API_BEGIN
    launch_layernorm(d_x, C, d_gamma, d_beta, d_y, C, rows, C, act, nullptr, 1, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_linear(const float* d_x, const void* d_w_f16, const float* d_bias, const float* d_res, float* d_y, int32_t M,
                 int32_t N, int32_t K, int32_t act, float alpha, int32_t split, int32_t force_gemv) {
    SC_API_BEGIN
    if (force_gemv) {
        launch_gemv(d_x, K, static_cast<const __half*>(d_w_f16), K, d_bias, d_res, N, d_y, N, M, N, K, act, alpha, g_op_stream);
    } else {
        GemmArgs a = op_linear_args<GemmArgs>(d_x, d_w_f16, d_bias, d_res, d_y, M, N, K, act, alpha);
        a.rows_per_batch = M, a.t_in = M, a.t_out = M;
        a.taps = 1, a.cin = K;
        a.split = split;
        launch_gemm(a, g_op_stream);
    }
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_skinny_linear(const float* d_x, const void* d_w_f16, const float* d_bias, const float* d_res, float* d_y,
                        int32_t M, int32_t N, int32_t K, int32_t act, float alpha) {
    SC_API_BEGIN
    launch_skinny(op_linear_args<SkinnyArgs>(d_x, d_w_f16, d_bias, d_res, d_y, M, N, K, act, alpha), g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_skinny_res_ln(const float* d_in, const void* d_w_f16, const float* d_bias, float* d_x_inout,
                        const float* d_gamma, const float* d_beta, float* d_h, int32_t M, int32_t N, int32_t K,
                        int32_t splits) {
    SC_API_BEGIN
    OpScratch scratch;
    SkinnyArgs a = op_linear_args<SkinnyArgs>(d_in, d_w_f16, nullptr, nullptr, nullptr, M, N, K);
    a.splits = splits > 0 ? splits : skinny_splits(M, N, K, 1);
    a.partial = scratch.get<float>((size_t)a.splits * M * N);
    launch_skinny(a, g_op_stream);
    launch_reduce_res_ln(a.partial, a.splits, d_bias, d_x_inout, d_gamma, d_beta, d_h, M, N, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_skinny_argmax(const float* d_x, const void* d_w_f16, int32_t M, int32_t N, int32_t K, int32_t step,
                        int32_t min_step_for_eos, int32_t force_eos_step, int32_t pad_idx, int32_t eos_idx,
                        int32_t unk_idx, float unk_penalty, int32_t* d_idx, float* d_lprob) {
    SC_API_BEGIN
    SC_CHECK(M >= 1 && M <= 64, "sc_op_skinny_argmax: M=%d out of range", M);
    OpScratch scratch;
    const int tiles = skinny_argmax_tiles(M, N);
    OpGreedy g = op_greedy(scratch, tiles, M, step, min_step_for_eos, force_eos_step, pad_idx, eos_idx, unk_idx, unk_penalty, d_lprob,
                           /*zero_part=*/true);
    SkinnyArgs a = op_linear_args<SkinnyArgs>(d_x, d_w_f16, nullptr, nullptr, nullptr, M, N, K);
    a.am = g.am;
    launch_skinny(a, g_op_stream);
    g.close(d_idx);
    SC_API_END
}

// ---- second-generation decoder-step kernels (k_dstep.hip), op level ------------------------------------------------

int sc_op_dstep_res_ln(const float* d_in, const void* d_w_f16, const float* d_bias, float* d_x_inout, const float* d_gamma,
                       const float* d_beta, float* d_h, int32_t M, int32_t N, int32_t K, int32_t splits) {
    SC_API_BEGIN
    SC_CHECK(gemvp_supported(M, N, K), "sc_op_dstep_res_ln: M=%d N=%d K=%d unsupported", M, N, K);
    OpScratch scratch;
    const int RB = op_row_slots(M);
    const int S = gemvp_splits(K, splits > 0 ? splits : 4);
    float* partial = scratch.get<float>((size_t)S * M * N);
    const OpPlanes x = op_planes(scratch, d_in, M, K, RB);
    GemvPArgs a;
    a.Wp = op_packed_weight(scratch, d_w_f16, N, K), a.Ah = x.hi, a.Al = x.lo, a.RB = RB, a.M = M, a.N = N, a.K = K;
    a.splits = splits > 0 ? splits : 4;
    a.epi = EPI_PARTIAL;
    a.partial = partial;
    launch_gemvp(a, g_op_stream);
    launch_reduce_ln(partial, S, d_bias, d_x_inout, d_gamma, d_beta, nullptr, nullptr, RB, nullptr, 0, 0, nullptr, M, N, g_op_stream, d_h);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_dstep_linear_planes(const float* d_x, const void* d_w_f16, const float* d_bias, float* d_y, int32_t M, int32_t N, int32_t K,
                              int32_t act) {
    SC_API_BEGIN
    SC_CHECK(gemvp_supported(M, N, K) && N % 8 == 0, "sc_op_dstep_linear_planes: M=%d N=%d K=%d unsupported", M, N, K);
    OpScratch scratch;
    const int RB = op_row_slots(M);
    __half* oh = scratch.get<__half>((size_t)N * RB);
    __half* ol = scratch.get<__half>((size_t)N * RB);
    const OpPlanes x = op_planes(scratch, d_x, M, K, RB);
    GemvPArgs a;
    a.Wp = op_packed_weight(scratch, d_w_f16, N, K), a.Ah = x.hi, a.Al = x.lo, a.RB = RB, a.M = M, a.N = N, a.K = K;
    a.splits = 1;
    a.epi = EPI_PLANES;
    a.bias = d_bias;
    a.act = act;
    a.Oh = oh, a.Ol = ol, a.ORB = RB;
    launch_gemvp(a, g_op_stream);
    launch_planes_to_rows(oh, ol, RB, d_y, N, M, N, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_dstep_argmax(const float* d_x, const void* d_w_f16, int32_t M, int32_t N, int32_t K, int32_t step,
                       int32_t min_step_for_eos, int32_t force_eos_step, int32_t pad_idx, int32_t eos_idx, int32_t unk_idx,
                       float unk_penalty, int32_t ntl, int32_t* d_idx, float* d_lprob) {
    SC_API_BEGIN
    SC_CHECK(gemvp_supported(M, N, K), "sc_op_dstep_argmax: M=%d N=%d K=%d unsupported", M, N, K);
    OpScratch scratch;
    const int RB = op_row_slots(M);
    if (ntl < 1) ntl = 4;
    const int tiles = gemvp_argmax_tiles(N, ntl);
    OpGreedy g = op_greedy(scratch, tiles, M, step, min_step_for_eos, force_eos_step, pad_idx, eos_idx, unk_idx, unk_penalty, d_lprob);
    const OpPlanes x = op_planes(scratch, d_x, M, K, RB);
    GemvPArgs a;
    a.Wp = op_packed_weight(scratch, d_w_f16, N, K), a.Ah = x.hi, a.Al = x.lo, a.RB = RB, a.M = M, a.N = N, a.K = K;
    a.splits = 1;
    a.ntl = ntl;
    a.epi = EPI_ARGMAX;
    a.am = g.am;
    launch_gemvp(a, g_op_stream);
    g.close(d_idx);
    SC_API_END
}

int sc_op_dstep3_gemv(int32_t mode, const float* d_x, const void* d_w_f16, const float* d_bias, const float* d_gamma,
                      const float* d_beta, const float* d_res, float* d_y, float* d_h, int32_t M, int32_t N, int32_t K, int32_t act,
                      int32_t rg, int32_t shape) {
    SC_API_BEGIN
    SC_CHECK(mode >= 0 && mode <= 3 && d_x && d_w_f16 && d_y, "sc_op_dstep3_gemv: bad argument");
    const int in_mode = (mode == 0 || mode == 2) ? IN3_LN : IN3_PLANES;
    SC_CHECK(gemv3_supported(M, N, K, in_mode), "sc_op_dstep3_gemv: M=%d N=%d K=%d mode=%d unsupported", M, N, K, mode);
    OpScratch scratch;
    const int RB = op_row_slots(M);
    Gemv3Args a;
    a.Wp = op_packed_weight(scratch, d_w_f16, N, K), a.M = M, a.N = N, a.K = K, a.in_mode = in_mode, a.RB = RB, a.rg = rg, a.bias = d_bias, a.shape = shape & 15;
    // bits 4..7 of `shape`: 0 the launcher decides, 15 one workgroup per row group, k weights stationary with k workgroups per tile
    a.stationary = ((shape >> 4) & 15) == 0 ? -1 : (((shape >> 4) & 15) == 15 ? 0 : ((shape >> 4) & 15));
    shape &= 15;
    // bits 8.. of `rg`: live rows (the device-side row count of the beam search / the decode engine; rows behind it are
    // neither read nor written); 0 = all M rows
    const int live = rg >> 8;
    rg &= 255;
    a.rg = rg;
    int* d_live = nullptr;
    if (live > 0) {
        SC_CHECK(live <= M, "sc_op_dstep3_gemv: %d live rows of %d", live, M);
        d_live = op_device_int(scratch, live);
        a.d_rows = d_live;
    }
    if (in_mode == IN3_LN) {
        a.xg = op_kgm(scratch, d_x, M, K, RB), a.gamma = d_gamma, a.beta = d_beta;
    } else {
        const OpPlanes x = op_planes(scratch, d_x, M, K, RB);
        a.Ah = x.hi, a.Al = x.lo;
    }
    if (mode == 0) {
        a.epi = EPI3_ROWS, a.out = d_y, a.ldo = N;
        launch_gemv3(a, g_op_stream);
    } else if (mode == 2) {
        // NaN in every slot of the output planes: a row the kernel leaves alone (behind the live rows) comes back as NaN
        const OpPlanes o = op_nan_planes(scratch, N, RB);
        a.epi = EPI3_PLANES, a.act = act, a.Oh = o.hi, a.Ol = o.lo, a.ORB = RB;
        launch_gemv3(a, g_op_stream);
        launch_planes_to_rows(o.hi, o.lo, RB, d_y, N, M, N, g_op_stream);
    } else {
        SC_CHECK(d_res, "sc_op_dstep3_gemv: modes 1 and 3 need the residual");
        float* xres = op_kgm(scratch, d_res, M, N, RB);
        if (mode == 1) {
            a.epi = EPI3_RESID, a.xres = xres, a.XRB = RB;
            launch_gemv3(a, g_op_stream);
        } else {
            const int S = gemv3_splits(K, shape);
            float* partial = scratch.get<float>((size_t)S * M * N);
            a.epi = EPI3_PARTIAL, a.out = partial, a.mt2 = 1, a.bias = nullptr;
            launch_gemv3(a, g_op_stream);
            Reduce3Args r;
            r.partial = partial, r.S = S, r.bias = d_bias, r.xg = xres, r.XRB = RB, r.rows = M, r.C = N, r.d_rows = d_live;
            if (d_gamma) r.gamma = d_gamma, r.beta = d_beta, r.hfix = d_h, r.RB = RB;
            launch_reduce3(r, g_op_stream);
        }
        launch_kgm_to_rows(xres, RB, d_y, N, M, N, g_op_stream);
    }
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_dstep3_argmax(const float* d_x, const void* d_w_f16, int32_t M, int32_t N, int32_t K, int32_t step,
                        int32_t min_step_for_eos, int32_t force_eos_step, int32_t pad_idx, int32_t eos_idx, int32_t unk_idx,
                        float unk_penalty, int32_t* d_idx, float* d_lprob) {
    SC_API_BEGIN
    SC_CHECK(vocab3_supported(M, N, K), "sc_op_dstep3_argmax: M=%d N=%d K=%d unsupported", M, N, K);
    OpScratch scratch;
    const int RB = op_row_slots(M);
    const int groups = vocab3_groups(M);
    OpGreedy g = op_greedy(scratch, groups, M, step, min_step_for_eos, force_eos_step, pad_idx, eos_idx, unk_idx, unk_penalty, d_lprob);
    const OpPlanes x = op_planes(scratch, d_x, M, K, RB);
    Vocab3Args v;
    v.Wp = op_packed_weight(scratch, d_w_f16, N, K), v.Ah = x.hi, v.Al = x.lo, v.RB = RB, v.M = M, v.N = N, v.K = K;
    v.am = g.am;
    launch_vocab3(v, g_op_stream);
    g.close(d_idx);
    SC_API_END
}

/* Single-query attention of the decoder step.  d_proj: [S][nb][ld] partial sums of the fused projection (self: q | k | v at
 * columns 0 / M / 2M, M = heads * 64; cross: q only, ld = M).  self (cross == 0): the new key / value row is appended to the
 * caches [nb][cap][M] at position `pos`, keys 0..pos take part.  cross: d_kcache = [nb][cap][2M] with keys at column 0 and
 * values at column M, d_vcache ignored, d_lens [nb] valid keys.  d_out [nb][M]. */
int sc_op_dstep_attention(const float* d_proj, int32_t S, const float* d_bias, float* d_kcache, float* d_vcache, int32_t cap,
                          int32_t pos, const int32_t* d_lens, int32_t cross, int32_t nb, int32_t heads, float* d_out) {
    SC_API_BEGIN
    SC_CHECK(nb >= 1 && nb <= 64 && heads >= 1 && S >= 1, "sc_op_dstep_attention: bad shape");
    OpScratch scratch;
    const int M = heads * 64, RB = op_row_slots(nb);
    __half* oh = scratch.get<__half>((size_t)M * RB);
    __half* ol = scratch.get<__half>((size_t)M * RB);
    int* d_pos = op_device_int(scratch, pos);
    DAttnArgs a;
    a.q = d_proj;
    a.S = S;
    a.bias = d_bias;
    a.cap = cap;
    a.Oh = oh, a.Ol = ol, a.ORB = RB;
    a.nb = nb, a.heads = heads;
    if (cross) {
        a.ldq = M, a.sstride = (int64_t)nb * M;
        a.kcache = d_kcache, a.vcache = d_kcache + M;
        a.cache_ld = 2 * M, a.cache_bs = (int64_t)cap * 2 * M;
        a.kv_lens = d_lens;
    } else {
        a.ldq = 3 * M, a.sstride = (int64_t)nb * 3 * M;
        a.koff = M, a.voff = 2 * M;
        a.kcache = d_kcache, a.vcache = d_vcache;
        a.cache_ld = M, a.cache_bs = (int64_t)cap * M;
        a.d_pos = d_pos;
    }
    launch_dattn(a, cross != 0, g_op_stream);
    launch_planes_to_rows(oh, ol, RB, d_out, M, nb, M, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

/* Diagnostic: `n` launches of ONE decoder-step kernel (kind) as a dependent chain in a captured hipGraph, replayed
 * `reps` times; *us_per_kernel = wall time per launch.  Shapes are those of the full-size model with `rows` batch rows.
 * kind 0 add_i32 | 1 reduce_ln (4 partials) | 2 gemvp 1024x1024 (4 K ranges) | 3 gemvp 1024x8192 (8 ranges) |
 * 4 gemvp 8192x1024 planes epilogue | 5 self-attention (position 20) | 6 cross-attention (63 keys) | 7 = 2 + 1 alternating */
int sc_op_chain_bench(int32_t kind, int32_t rows, int32_t n, int32_t reps, float* us_per_kernel) {
    SC_API_BEGIN
    SC_CHECK(kind >= 0 && kind <= 7 && rows >= 1 && rows <= 64 && n >= 1 && reps >= 1 && us_per_kernel, "sc_op_chain_bench: bad argument");
    OpScratch scratch;
    const int M = 1024, F = 8192, H = 16, RB = rows <= 32 ? 32 : 64, cap = 42, s_enc = 63;
    __half* wp = scratch.get<__half>((size_t)packed_weight_halfs(F, M));
    __half* planes = scratch.get<__half>((size_t)4 * F * RB);
    float* partial = scratch.get<float>((size_t)8 * rows * 3 * M);
    float* x = scratch.get<float>((size_t)rows * M);
    float* gb = scratch.get<float>((size_t)3 * M);
    float* kv = scratch.get<float>((size_t)rows * s_enc * 2 * M);
    int* ints = scratch.get<int>(64 + rows);
    SC_HIP(hipMemset(wp, 0, (size_t)packed_weight_halfs(F, M) * 2));
    SC_HIP(hipMemset(planes, 0, (size_t)4 * F * RB * 2));
    SC_HIP(hipMemset(partial, 0, (size_t)8 * rows * 3 * M * 4));
    SC_HIP(hipMemset(x, 0, (size_t)rows * M * 4));
    SC_HIP(hipMemset(gb, 0, (size_t)3 * M * 4));
    SC_HIP(hipMemset(kv, 0, (size_t)rows * s_enc * 2 * M * 4));
    std::vector<int> hi(64 + rows, s_enc);
    hi[0] = 20;
    SC_HIP(hipMemcpy(ints, hi.data(), hi.size() * 4, hipMemcpyHostToDevice));
    __half *ah = planes, *al = planes + (size_t)F * RB, *oh = al + (size_t)F * RB, *ol = oh + (size_t)F * RB;
    hipStream_t st = nullptr;
    SC_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    auto one = [&](int k) {
        if (k == 0) {
            launch_add_i32(ints + 1, 1, st);
        } else if (k == 1) {
            launch_reduce_ln(partial, 4, gb, x, gb + M, gb + 2 * M, ah, al, RB, nullptr, 0, 0, nullptr, rows, M, st);
        } else if (k == 2 || k == 3 || k == 4) {
            GemvPArgs a;
            a.Wp = wp, a.Ah = ah, a.Al = al, a.RB = RB, a.M = rows;
            a.N = k == 4 ? F : M;
            a.K = k == 3 ? F : M;
            a.splits = k == 2 ? 4 : (k == 3 ? 8 : 1);
            a.epi = k == 4 ? EPI_PLANES : EPI_PARTIAL;
            a.partial = partial;
            a.bias = k == 4 ? gb : nullptr;
            a.act = ACT_RELU;
            a.Oh = oh, a.Ol = ol, a.ORB = RB;
            launch_gemvp(a, st);
        } else {
            DAttnArgs a;
            a.q = partial;
            a.bias = gb;
            a.Oh = oh, a.Ol = ol, a.ORB = RB;
            a.nb = rows, a.heads = H;
            if (k == 5) {
                a.S = 2, a.ldq = 3 * M, a.sstride = (int64_t)rows * 3 * M, a.koff = M, a.voff = 2 * M;
                a.kcache = kv, a.vcache = kv + (size_t)rows * cap * M, a.cache_ld = M, a.cache_bs = (int64_t)cap * M, a.cap = cap;
                a.d_pos = ints;
            } else {
                a.S = 4, a.ldq = M, a.sstride = (int64_t)rows * M;
                a.kcache = kv, a.vcache = kv + M, a.cache_ld = 2 * M, a.cache_bs = (int64_t)s_enc * 2 * M, a.cap = s_enc;
                a.kv_lens = ints + 64;
            }
            launch_dattn(a, k == 6, st);
        }
    };
    StepGraph g;
    g.ensure(st, [&] {
        for (int i = 0; i < n; ++i) {
            if (kind == 7) one(i & 1 ? 1 : 2);
            else one(kind);
        }
    });
    for (int r = 0; r < 2; ++r) g.launch(st);
    SC_HIP(hipStreamSynchronize(st));
    hipEvent_t e0, e1;
    SC_HIP(hipEventCreate(&e0));
    SC_HIP(hipEventCreate(&e1));
    SC_HIP(hipEventRecord(e0, st));
    for (int r = 0; r < reps; ++r) g.launch(st);
    SC_HIP(hipEventRecord(e1, st));
    SC_HIP(hipStreamSynchronize(st));
    float ms = 0.f;
    SC_HIP(hipEventElapsedTime(&ms, e0, e1));
    *us_per_kernel = 1e3f * ms / (float)(reps * n);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    g = StepGraph();  // before its stream goes
    (void)hipStreamDestroy(st);
    SC_API_END
}

int sc_op_pack_conv_weight(const void* d_w_f16, void* d_dst_f16, int32_t cout, int32_t cin, int32_t k) {
    SC_API_BEGIN
    const int kpad = (int)align_up((int64_t)cin * k, 32);
    launch_pack_conv_weight(static_cast<const __half*>(d_w_f16), static_cast<__half*>(d_dst_f16), cout, cin, k, kpad,
                            g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_conv1d(const float* d_x, const void* d_w_f16_packed, const float* d_bias, const float* d_res, float* d_y,
                 int32_t nb, int32_t t_in, int32_t cin, int32_t cout, int32_t k, int32_t stride, int32_t pad, int32_t dil,
                 const int32_t* d_in_lens, int32_t in_act, int32_t act) {
    SC_API_BEGIN
    Model tmp;  // only the stream (null = default) is used by conv1d()
    Conv c;
    c.w = static_cast<const __half*>(d_w_f16_packed);
    c.b = d_bias;
    c.cout = cout;
    c.cin = cin;
    c.k = k;
    c.kpad = (int)align_up((int64_t)cin * k, 32);
    conv1d(tmp, d_x, c, d_res, d_y, nb, t_in, stride, pad, dil, d_in_lens, in_act, act);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_conv_transpose1d(const float* d_x, const void* d_v_f16, const void* d_g_f16, const float* d_bias, float* d_y,
                           int32_t nb, int32_t t_in, int32_t cin, int32_t cout, int32_t k, int32_t stride, int32_t pad,
                           int32_t in_act) {
    SC_API_BEGIN
    // k - stride odd: padding rounded up with output_padding 1 (the PRETSSEL generator's upsampling convolutions at odd rates)
    SC_CHECK(k >= stride && pad == (k - stride + 1) / 2 && k - 2 * pad + (k - stride) % 2 == stride, "sc_op_conv_transpose1d: unsupported geometry");
    Model tmp;
    ConvT c;
    c.cin = cin;
    c.cout = cout;
    c.k = k;
    c.stride = stride;
    c.pad = pad;
    c.taps = cdiv(k, stride);
    c.kpad = (int)align_up((int64_t)cin * c.taps, 32);
    OpScratch scratch;
    float* folded = scratch.get<float>((size_t)cin * cout * k);
    __half* packed = scratch.get<__half>((size_t)stride * cout * c.kpad);
    launch_weight_norm_fold(static_cast<const __half*>(d_v_f16), static_cast<const __half*>(d_g_f16), folded, cin, cout * k,
                            g_op_stream);
    launch_pack_convT_weight(folded, packed, cin, cout, k, stride, c.kpad, g_op_stream);
    c.w = packed;
    c.b = d_bias;
    conv_transpose1d(tmp, d_x, c, d_y, nb, t_in, in_act);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_linear_presplit(const float* d_x, const void* d_w_f16, const float* d_bias, const float* d_res, float* d_y,
                          void* d_yh_f16, void* d_yl_f16, int32_t M, int32_t N, int32_t K, int32_t act, float alpha) {
    SC_API_BEGIN
    SC_CHECK(d_x && d_w_f16 && (d_y || d_yh_f16), "sc_op_linear_presplit: null argument");
    OpScratch scratch;
    GemmPsArgs a = op_presplit_args(scratch, d_x, d_w_f16, d_bias, M, N, K);
    a.res = d_res, a.ldr = N;
    a.C = d_y, a.ldc = N;
    a.Ch = static_cast<__half*>(d_yh_f16), a.Cl = static_cast<__half*>(d_yl_f16), a.ldcs = N;
    a.act = act, a.alpha = alpha;
    launch_gemm_presplit(a, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_linear_presplit_glu(const float* d_x, const void* d_w_f16, const float* d_bias, float* d_y, int32_t M, int32_t N, int32_t K,
                              int32_t fused) {
    SC_API_BEGIN
    SC_CHECK(d_x && d_w_f16 && d_y && M > 0 && N > 0 && N % 2 == 0 && K > 0, "sc_op_linear_presplit_glu: bad argument");
    OpScratch scratch;
    GemmPsArgs a = op_presplit_args(scratch, d_x, d_w_f16, d_bias, M, N, K);
    if (fused) {
        __half* wg = scratch.get<__half>((size_t)N * K);
        float* bg = d_bias ? scratch.get<float>((size_t)N) : nullptr;
        launch_glu_interleave_rows(static_cast<const __half*>(d_w_f16), K, d_bias, N / 2, K, wg, K, bg, g_op_stream);
        a.W = wg;
        a.bias = bg;
        a.C = d_y;
        a.ldc = N / 2;
        launch_gemm_presplit_glu(a, g_op_stream);
    } else {
        float* wide = scratch.get<float>((size_t)M * N);
        a.C = wide;
        a.ldc = N;
        launch_gemm_presplit(a, g_op_stream);
        launch_glu(wide, N, d_y, N / 2, M, N / 2, g_op_stream);
    }
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_linear_presplit_argmax(const float* d_x, const void* d_w_f16, const float* d_bias, int32_t* d_idx, int32_t M, int32_t N,
                                 int32_t K) {
    SC_API_BEGIN
    SC_CHECK(d_x && d_w_f16 && d_idx, "sc_op_linear_presplit_argmax: null argument");
    OpScratch scratch;
    const int nch = gemm_presplit_amax_chunks(M, N);
    float2* part = op_filled<float2>(scratch, (size_t)M * nch, 0xff);  // NaN / -1: every entry must be written
    GemmPsArgs a = op_presplit_args(scratch, d_x, d_w_f16, d_bias, M, N, K);
    a.amax = part;
    a.amax_ld = nch;
    launch_gemm_presplit(a, g_op_stream);
    launch_amax_finish(part, nch, M, d_idx, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_linear_presplit_score_grouped(const float* d_x, const void* d_w_f16, const float* d_bias, const int32_t* d_target,
                                        float* d_lprob, float* d_sum_lprob, float* d_lse, int32_t* d_top1, int32_t M, int32_t N,
                                        int32_t K, int32_t group_rows) {
    SC_API_BEGIN
    SC_CHECK(d_x && d_w_f16 && d_target && (d_lprob || d_sum_lprob || d_lse || d_top1), "sc_op_linear_presplit_score: null argument");
    SC_CHECK(M > 0 && N > 0 && K > 0 && group_rows >= 0, "sc_op_linear_presplit_score: M=%d N=%d K=%d group_rows=%d", M, N, K, group_rows);
    const int group = std::min(group_rows > 0 ? group_rows : gemm_score_group_rows(N), M);
    OpScratch scratch;
    // NaN / -1: every record must be written
    float* rec = op_filled<float>(scratch, (size_t)group * gemm_score_records(N) * SCORE_REC_FLOATS, 0xff);
    const GemmPsArgs a = op_presplit_args(scratch, d_x, d_w_f16, d_bias, M, N, K);
    launch_gemm_presplit_score(a, d_target, rec, group, d_lprob, d_sum_lprob, d_lse, d_top1, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_linear_presplit_score(const float* d_x, const void* d_w_f16, const float* d_bias, const int32_t* d_target, float* d_lprob,
                                float* d_sum_lprob, float* d_lse, int32_t* d_top1, int32_t M, int32_t N, int32_t K) {
    return sc_op_linear_presplit_score_grouped(d_x, d_w_f16, d_bias, d_target, d_lprob, d_sum_lprob, d_lse, d_top1, M, N, K, 0);
}

int sc_op_score_candidates(const float* d_x, const void* d_w_f16, const float* d_bias, const int32_t* h_cand, int32_t n_cand, float* d_lprob,
                           int32_t* d_best, int32_t M, int32_t N, int32_t K) {
    SC_API_BEGIN
    SC_CHECK(d_x && d_w_f16 && h_cand && d_lprob && d_best, "sc_op_score_candidates: null argument");
    SC_CHECK(M > 0 && N > 0 && K > 0, "sc_op_score_candidates: M=%d N=%d K=%d", M, N, K);
    check_score_candidates(h_cand, n_cand, N, "sc_op_score_candidates");
    const int group = std::min(gemm_score_group_rows(N), M);
    OpScratch scratch;
    // NaN / -1: every record and every value must be written
    float* rec = op_filled<float>(scratch, (size_t)group * gemm_score_records(N) * SCORE_REC_FLOATS, 0xff);
    float* cv = op_filled<float>(scratch, (size_t)group * n_cand, 0xff);
    int* cand = scratch.get<int>((size_t)n_cand);
    SC_HIP(hipMemcpyAsync(cand, h_cand, (size_t)n_cand * 4, hipMemcpyHostToDevice, g_op_stream));
    const GemmPsArgs a = op_presplit_args(scratch, d_x, d_w_f16, d_bias, M, N, K);
    launch_gemm_presplit_score_cand(a, cand, n_cand, rec, cv, group, d_lprob, d_best, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int32_t sc_op_score_record_cols(int32_t N) { return N > 0 ? gemm_score_record_cols(N) : -1; }
int32_t sc_op_score_group_rows(int32_t N) { return N > 0 ? gemm_score_group_rows(N) : -1; }

int sc_op_conv1d_presplit(const float* d_x, const void* d_w_f16_packed, const float* d_bias, const float* d_res, float* d_y,
                          void* d_yh_f16, void* d_yl_f16, int32_t nb, int32_t t, int32_t cin, int32_t cout, int32_t k, int32_t pad,
                          int32_t dil, const unsigned char* d_row_valid, int32_t act) {
    SC_API_BEGIN
    SC_CHECK(d_x && d_w_f16_packed && (d_y || d_yh_f16), "sc_op_conv1d_presplit: null argument");
    OpScratch scratch;
    const OpPlanes x = op_split(scratch, d_x, (size_t)nb * t * cin);
    Model tmp;
    Conv c;
    c.w = static_cast<const __half*>(d_w_f16_packed);
    c.b = d_bias;
    c.cout = cout;
    c.cin = cin;
    c.k = k;
    c.kpad = (int)align_up((int64_t)cin * k, 32);
    conv1d_presplit(tmp, x.hi, x.lo, c, d_res, d_y, static_cast<__half*>(d_yh_f16), static_cast<__half*>(d_yl_f16), nb, t, pad, dil, d_row_valid,
                    act);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

/* One HiFi-GAN dilation pair  out = x + conv2_{k,1}(lrelu(conv1_{k,dil}(lrelu(x)) + b1)) + b2  the way the wide vocoder
 * stages (C >= 128) run it: LeakyReLU(x) split into fp16 planes, both convolutions on the DMA-fed GEMM in implicit-convolution
 * mode, the first one's epilogue writing the LeakyReLU'd planes the second one reads (model_t2u.hip: vocode_batch). */
int sc_op_resblock_pair_ps(const float* d_x, const void* d_w1_packed, const float* d_b1, const void* d_w2_packed, const float* d_b2,
                           float* d_out, int32_t nb, int32_t T, int32_t C, int32_t k, int32_t dil) {
    SC_API_BEGIN
    SC_CHECK(d_x && d_w1_packed && d_w2_packed && d_out && C % 32 == 0 && (k & 1), "sc_op_resblock_pair_ps: bad argument");
    OpScratch scratch;
    const size_t n = (size_t)nb * T * C;
    const bool one = g_op_single.load() != 0;  // hi planes only: no lo plane is produced or read
    __half* xh = scratch.get<__half>(n);
    __half* xl = one ? nullptr : scratch.get<__half>(n);
    __half* th = scratch.get<__half>(n);
    __half* tl = one ? nullptr : scratch.get<__half>(n);
    launch_lrelu_split_f32(d_x, 0.1f, xh, xl, (int64_t)n, g_op_stream);
    Model tmp;
    Conv c1, c2;
    c1.w = static_cast<const __half*>(d_w1_packed), c1.b = d_b1, c1.cin = c1.cout = C, c1.k = k, c1.kpad = C * k;
    c2.w = static_cast<const __half*>(d_w2_packed), c2.b = d_b2, c2.cin = c2.cout = C, c2.k = k, c2.kpad = C * k;
    conv1d_presplit(tmp, xh, xl, c1, nullptr, nullptr, th, tl, nb, T, (k * dil - dil) / 2, dil, nullptr, ACT_NONE, 0, nullptr, 0.1f, one ? 0 : 1);
    conv1d_presplit(tmp, th, tl, c2, d_x, d_out, nullptr, nullptr, nb, T, (k - 1) / 2, 1, nullptr, ACT_NONE, 0, nullptr, 0.1f, one ? 0 : 1);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_resblock_pair(const float* d_x, const void* d_w1_packed, const float* d_b1, const void* d_w2_packed,
                        const float* d_b2, float* d_out, int32_t nb, int32_t T, int32_t C, int32_t k, int32_t dil,
                        float slope, const float* d_avg_a, const float* d_avg_b) {
    SC_API_BEGIN
    SC_CHECK(d_x && d_w1_packed && d_w2_packed && d_out, "sc_op_resblock_pair: null argument");
    ResPairArgs a;
    a.x = d_x;
    a.out = d_out;
    a.w1 = static_cast<const __half*>(d_w1_packed);
    a.w2 = static_cast<const __half*>(d_w2_packed);
    a.ldw1 = a.ldw2 = align_up((int64_t)C * k, 32);
    a.b1 = d_b1;
    a.b2 = d_b2;
    a.nb = nb;
    a.T = T;
    a.C = C;
    a.k = k;
    a.dil = dil;
    a.slope = slope;
    a.avg_a = d_avg_a;
    a.avg_b = d_avg_b;
    a.single = g_op_single.load();
    launch_resblock_pair(a, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_mrf_fused(const float* d_x, const void* const* d_w1_packed, const float* const* d_b1, const void* const* d_w2_packed,
                    const float* const* d_b2, float* d_out, int32_t nb, int32_t T, int32_t C, const int32_t* k, const int32_t* dil,
                    float slope) {
    SC_API_BEGIN
    SC_CHECK(d_x && d_w1_packed && d_b1 && d_w2_packed && d_b2 && d_out && k && dil, "sc_op_mrf_fused: null argument");
    MrfArgs a;
    a.x = d_x;
    a.out = d_out;
    a.nb = nb;
    a.T = T;
    a.C = C;
    a.slope = slope;
    for (int j = 0; j < 3; ++j) a.k[j] = k[j];
    for (int q = 0; q < 9; ++q) {
        a.dil[q] = dil[q];
        a.w1[q] = static_cast<const __half*>(d_w1_packed[q]);
        a.w2[q] = static_cast<const __half*>(d_w2_packed[q]);
        a.ldw1[q] = a.ldw2[q] = align_up((int64_t)C * k[q / 3], 32);
        a.b1[q] = d_b1[q];
        a.b2[q] = d_b2[q];
    }
    a.single = g_op_single.load();
    launch_mrf_fused(a, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_attention(const float* d_q, const float* d_k, const float* d_v, float* d_out, int32_t nb, int32_t heads,
                    int32_t sq, int32_t skv, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, const int32_t* d_kv_lens,
                    int32_t causal, const float* d_rel_k, int32_t rel_left, int32_t rel_right) {
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
    a.causal = causal;
    a.rel_k = d_rel_k;
    a.rel_left = rel_left;
    a.rel_right = rel_right;
    launch_attention(a, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_attention_ex(const float* d_q, const float* d_k, const float* d_v, float* d_out, int32_t nb, int32_t heads,
                       int32_t sq, int32_t skv, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, const int32_t* d_kv_lens,
                       int32_t causal, const float* d_rel_k, int32_t rel_left, int32_t rel_right, const int32_t* d_row_off,
                       const float* d_rp_table, int64_t rp_ld, const float* d_q_bias_u, const float* d_q_bias_v, void* d_out_hi,
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
    a.causal = causal;
    a.rel_k = d_rel_k;
    a.rel_left = rel_left;
    a.rel_right = rel_right;
    a.row_off = d_row_off;
    a.rp_table = d_rp_table;
    a.rp_ld = rp_ld;
    a.q_bias_u = d_q_bias_u;
    a.q_bias_v = d_q_bias_v;
    a.out_hi = static_cast<__half*>(d_out_hi);
    a.out_lo = static_cast<__half*>(d_out_lo);
    a.ldoh = ldoh;
    launch_attention(a, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_glu_dwconv(const float* d_x, const float* d_w, float* d_y, int32_t nb, int32_t T, int32_t C, int32_t k,
                     const int32_t* d_lens) {
    SC_API_BEGIN
    launch_glu_dwconv(d_x, 2 * C, d_w, d_y, C, nb, T, C, k, d_lens, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_glu_dwconv_ln(const float* d_x, const float* d_w, const float* d_gamma, const float* d_beta, int32_t act, void* d_yh_f16,
                        void* d_yl_f16, int32_t nb, int32_t T, int32_t C, int32_t k, const int32_t* d_lens, int32_t fused) {
    SC_API_BEGIN
    SC_CHECK(d_x && d_w && d_gamma && d_beta && d_yh_f16 && d_yl_f16, "sc_op_glu_dwconv_ln: null argument");
    __half* yh = static_cast<__half*>(d_yh_f16);
    __half* yl = static_cast<__half*>(d_yl_f16);
    if (fused == 2) {  // the gated form: x [nb*T][C] already holds GLU(.)
        launch_glu_dwconv_ln(d_x, C, d_w, d_gamma, d_beta, act, yh, yl, C, nb, T, C, k, d_lens, g_op_stream, /*gated=*/true);
    } else if (fused) {
        launch_glu_dwconv_ln(d_x, 2 * C, d_w, d_gamma, d_beta, act, yh, yl, C, nb, T, C, k, d_lens, g_op_stream);
    } else {
        OpScratch scratch;
        float* mid = scratch.get<float>((size_t)nb * T * C);
        launch_glu_dwconv(d_x, 2 * C, d_w, mid, C, nb, T, C, k, d_lens, g_op_stream);
        launch_layernorm_split(mid, C, d_gamma, d_beta, yh, yl, C, nb * T, C, act, nullptr, 1, g_op_stream);
        SC_HIP(hipStreamSynchronize(g_op_stream));
    }
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_glu_dwconv_ln_packed(const float* d_x, const float* d_w, const float* d_gamma, const float* d_beta, int32_t act, void* d_yh_f16,
                               void* d_yl_f16, int32_t n, const int32_t* h_row_off, const int32_t* h_lens, int32_t C, int32_t k, int32_t gated) {
    SC_API_BEGIN
    SC_CHECK(d_x && d_w && d_gamma && d_beta && d_yh_f16 && d_yl_f16 && h_row_off && h_lens && n > 0, "sc_op_glu_dwconv_ln_packed: null argument");
    std::vector<int32_t> work;
    glu_dwconv_ln_packed_work(h_row_off, h_lens, n, work);
    double rows = 0;
    for (int i = 0; i < n; ++i) rows += h_lens[i];
    OpScratch scratch;
    int* d_work = scratch.get<int>(work.size());
    SC_HIP(hipMemcpyAsync(d_work, work.data(), work.size() * 4, hipMemcpyHostToDevice, g_op_stream));
    launch_glu_dwconv_ln_packed(d_x, gated ? C : 2 * C, d_w, d_gamma, d_beta, act, static_cast<__half*>(d_yh_f16), static_cast<__half*>(d_yl_f16),
                                C, d_work, (int)(work.size() / 4), rows, C, k, g_op_stream, gated != 0);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_layernorm2(const float* d_x, const float* d_ga, const float* d_ba, const float* d_gb, const float* d_bb, float* d_y,
                     void* d_yh_f16, void* d_yl_f16, int32_t rows, int32_t C, int32_t fused) {
    SC_API_BEGIN
    SC_CHECK(d_x && d_ga && d_ba && d_gb && d_bb && d_y && d_yh_f16 && d_yl_f16, "sc_op_layernorm2: null argument");
    __half* yh = static_cast<__half*>(d_yh_f16);
    __half* yl = static_cast<__half*>(d_yl_f16);
    if (fused) {
        launch_layernorm2_split(d_x, C, d_ga, d_ba, d_y, C, d_gb, d_bb, yh, yl, C, rows, C, g_op_stream);
    } else {
        launch_layernorm(d_x, C, d_ga, d_ba, d_y, C, rows, C, ACT_NONE, nullptr, 1, g_op_stream);
        launch_layernorm_split(d_y, C, d_gb, d_bb, yh, yl, C, rows, C, ACT_NONE, nullptr, 1, g_op_stream);
    }
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_argmax(const float* d_logits, int32_t rows, int32_t V, int32_t* d_idx, float* d_lprob) {
    SC_API_BEGIN
    launch_argmax_rows(d_logits, V, rows, V, nullptr, -1, -1, -1, -1, -1, 0.f, d_idx, d_lprob, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

// beam-search step kernels (k_beam.hip) through the launchers run_generate_beam calls.  Index arrays that the kernels follow
// into other buffers (slot -> utterance, candidate -> beam, source rows) are checked on the host first (op_read_ints): a test
// that hands in a bad one gets an error, not an out-of-bounds access.

static int op_beam_candidates(float* d_logits, int64_t ld, int32_t n_utt, int32_t beams, int32_t V, const float* d_cum, int32_t first_step,
                              int32_t no_eos, int32_t force_eos, int32_t pad_idx, int32_t eos_idx, int32_t unk_idx, float unk_penalty, int32_t K,
                              float* d_cand_val, int32_t* d_cand_idx, const int32_t* d_seqs, int32_t seq_ld, int32_t S, int32_t G,
                              const int32_t* d_rows, const int32_t* d_slots, int32_t chunked, const int32_t* d_banned_tokens,
                              const int32_t* d_banned_offsets, int32_t n_banned, const int32_t* d_boost_tokens = nullptr,
                              const int32_t* d_boost_offsets = nullptr, int32_t n_boost = 0, float boost_value = 0.f) {
    SC_API_BEGIN
    // the phrase list is read back, checked and sorted on the host, and the sorted list goes up again
    BoostList bo;
    OpScratch boost_scratch;
    if (n_boost != 0 && boost_value != 0.f) {
        SC_CHECK(n_boost > 0 && n_boost <= BOOST_MAX_PHRASES && d_boost_tokens && d_boost_offsets && d_seqs,
                 "boost phrases: bad list (%d phrases, at most %d; needs d_seqs)", n_boost, BOOST_MAX_PHRASES);
        const std::vector<int32_t> off = op_read_ints(d_boost_offsets, (size_t)n_boost + 1);
        SC_CHECK(off[0] == 0 && off[n_boost] >= 0, "boost phrases: bad offsets");
        for (int q = 0; q < n_boost; ++q) SC_CHECK(off[q + 1] >= off[q], "boost phrases: offsets decrease at %d", q);
        SC_CHECK(off[n_boost] <= BOOST_MAX_TOKENS, "boost phrases: %d tokens in all (at most %d)", off[n_boost], BOOST_MAX_TOKENS);
        const std::vector<int32_t> tok = op_read_ints(d_boost_tokens, (size_t)off[n_boost]);
        BoostSorted sorted;
        const std::string why = boost_list_build(tok.data(), off.data(), n_boost, V, pad_idx, eos_idx, sorted);
        SC_CHECK(why.empty(), "%s", why.c_str());
        const std::string bad = boost_value_check(boost_value);
        SC_CHECK(bad.empty(), "%s", bad.c_str());
        int* store = boost_scratch.get<int>(sorted.tokens.size() + sorted.n + 1);
        SC_HIP(hipMemcpy(store, sorted.tokens.data(), sorted.tokens.size() * 4, hipMemcpyHostToDevice));
        SC_HIP(hipMemcpy(store + sorted.tokens.size(), sorted.offsets.data(), (size_t)(sorted.n + 1) * 4, hipMemcpyHostToDevice));
        bo.tokens = store, bo.offsets = store + sorted.tokens.size(), bo.n = sorted.n, bo.max_len = sorted.max_len, bo.beta = boost_value;
    }
    const BoostList* boost = bo.n > 0 ? &bo : nullptr;
    // the device list is read back and checked on the host first: a bad one is an error, not an out-of-bounds access
    BannedList bl;
    if (n_banned != 0) {
        SC_CHECK(n_banned > 0 && n_banned <= BANNED_MAX_SEQS && d_banned_tokens && d_banned_offsets && d_seqs,
                 "sc_op_beam_candidates_banned: bad banned list (n_banned=%d; needs d_seqs)", n_banned);
        const std::vector<int32_t> off = op_read_ints(d_banned_offsets, (size_t)n_banned + 1);
        SC_CHECK(off[0] == 0 && off[n_banned] >= 0 && off[n_banned] <= BANNED_MAX_TOKENS, "sc_op_beam_candidates_banned: bad offsets");
        for (int q = 0; q < n_banned; ++q) SC_CHECK(off[q + 1] >= off[q], "sc_op_beam_candidates_banned: offsets decrease at %d", q);
        const std::vector<int32_t> tok = op_read_ints(d_banned_tokens, (size_t)off[n_banned]);
        validate_banned_host(tok.data(), off.data(), n_banned, V, &bl.max_len);
        bl.tokens = d_banned_tokens, bl.offsets = d_banned_offsets, bl.n = n_banned;
    }
    const BannedList* banned = bl.n > 0 ? &bl : nullptr;
    SC_CHECK(d_logits && d_cum && d_cand_val && d_cand_idx && n_utt >= 1 && V >= 1 && ld >= V, "sc_op_beam_candidates: bad arguments");
    SC_CHECK(!d_seqs || (G >= 0 && S >= 0 && seq_ld >= S), "sc_op_beam_candidates: bad n-gram arguments (S=%d G=%d seq_ld=%d)", S, G, seq_ld);
    if (d_slots) SC_CHECK(op_read_ints(d_slots, 1)[0] <= n_utt, "sc_op_beam_candidates: *d_slots > n_utt");
    if (chunked) {
        SC_CHECK(beam_chunked(V, beams, K), "sc_op_beam_candidates: the chunked search does not take V=%d beams=%d K=%d", V, beams, K);
        if (d_rows) SC_CHECK(op_read_ints(d_rows, 1)[0] <= n_utt * beams, "sc_op_beam_candidates: *d_rows > n_utt * beams");
        OpScratch scratch;
        const int rows = n_utt * beams;
        float* ws_f = scratch.get<float>(beam_ws_floats(rows, K));
        int* ws_i = scratch.get<int>(beam_ws_ints(rows, K));
        SC_HIP(hipMemsetAsync(ws_f, 0xff, beam_ws_floats(rows, K) * 4, g_op_stream));  // NaN / -1: unwritten entries show
        SC_HIP(hipMemsetAsync(ws_i, 0xff, beam_ws_ints(rows, K) * 4, g_op_stream));
        launch_beam_candidates_chunked(d_logits, ld, n_utt, beams, V, d_cum, first_step, no_eos, force_eos, pad_idx, eos_idx, unk_idx,
                                       unk_penalty, K, d_cand_val, d_cand_idx, d_seqs, seq_ld, S, G, ws_f, ws_i, g_op_stream, d_rows, d_slots, banned,
                                       boost);
        SC_HIP(hipStreamSynchronize(g_op_stream));
    } else {
        SC_CHECK(!d_rows, "sc_op_beam_candidates: d_rows is an argument of the chunked search only (the single-workgroup one takes d_slots)");
        launch_beam_candidates(d_logits, ld, n_utt, beams, V, d_cum, first_step, no_eos, force_eos, pad_idx, eos_idx, unk_idx, unk_penalty, K,
                               d_cand_val, d_cand_idx, d_seqs, seq_ld, S, G, g_op_stream, d_slots, banned, boost);
        SC_HIP(hipStreamSynchronize(g_op_stream));
    }
    SC_API_END
}

int sc_op_beam_candidates(float* d_logits, int64_t ld, int32_t n_utt, int32_t beams, int32_t V, const float* d_cum, int32_t first_step,
                          int32_t no_eos, int32_t force_eos, int32_t pad_idx, int32_t eos_idx, int32_t unk_idx, float unk_penalty, int32_t K,
                          float* d_cand_val, int32_t* d_cand_idx, const int32_t* d_seqs, int32_t seq_ld, int32_t S, int32_t G,
                          const int32_t* d_rows, const int32_t* d_slots, int32_t chunked) {
    return op_beam_candidates(d_logits, ld, n_utt, beams, V, d_cum, first_step, no_eos, force_eos, pad_idx, eos_idx, unk_idx, unk_penalty, K,
                              d_cand_val, d_cand_idx, d_seqs, seq_ld, S, G, d_rows, d_slots, chunked, nullptr, nullptr, 0);
}

int sc_op_beam_candidates_banned(float* d_logits, int64_t ld, int32_t n_utt, int32_t beams, int32_t V, const float* d_cum,
                                 int32_t first_step, int32_t no_eos, int32_t force_eos, int32_t pad_idx, int32_t eos_idx, int32_t unk_idx,
                                 float unk_penalty, int32_t K, float* d_cand_val, int32_t* d_cand_idx, const int32_t* d_seqs,
                                 int32_t seq_ld, int32_t S, int32_t G, const int32_t* d_rows, const int32_t* d_slots, int32_t chunked,
                                 const int32_t* d_banned_tokens, const int32_t* d_banned_offsets, int32_t n_banned) {
    return op_beam_candidates(d_logits, ld, n_utt, beams, V, d_cum, first_step, no_eos, force_eos, pad_idx, eos_idx, unk_idx, unk_penalty, K,
                              d_cand_val, d_cand_idx, d_seqs, seq_ld, S, G, d_rows, d_slots, chunked, d_banned_tokens, d_banned_offsets,
                              n_banned);
}

int sc_op_beam_candidates_boost(float* d_logits, int64_t ld, int32_t n_utt, int32_t beams, int32_t V, const float* d_cum,
                                int32_t first_step, int32_t no_eos, int32_t force_eos, int32_t pad_idx, int32_t eos_idx, int32_t unk_idx,
                                float unk_penalty, int32_t K, float* d_cand_val, int32_t* d_cand_idx, const int32_t* d_seqs,
                                int32_t seq_ld, int32_t S, int32_t G, const int32_t* d_rows, const int32_t* d_slots, int32_t chunked,
                                const int32_t* d_banned_tokens, const int32_t* d_banned_offsets, int32_t n_banned,
                                const int32_t* d_boost_tokens, const int32_t* d_boost_offsets, int32_t n_boost, float boost) {
    return op_beam_candidates(d_logits, ld, n_utt, beams, V, d_cum, first_step, no_eos, force_eos, pad_idx, eos_idx, unk_idx, unk_penalty, K,
                              d_cand_val, d_cand_idx, d_seqs, seq_ld, S, G, d_rows, d_slots, chunked, d_banned_tokens, d_banned_offsets,
                              n_banned, d_boost_tokens, d_boost_offsets, n_boost, boost);
}

// the sampling step (k_sample.hip) through the launcher run_generate_sampled calls
int sc_op_sample_rows(float* d_logits, int64_t ld, int32_t rows, int32_t V, const uint64_t* d_stream, const int32_t* d_gen,
                      const int32_t* d_position, float temperature, int32_t top_k, float top_p, uint64_t seed, int32_t no_eos, int32_t force_eos,
                      int32_t pad_idx, int32_t eos_idx, int32_t unk_idx, float unk_penalty, const int32_t* d_seqs, int32_t seq_ld, int32_t S,
                      int32_t G, const int32_t* d_banned_tokens, const int32_t* d_banned_offsets, int32_t n_banned, int32_t* d_tok,
                      float* d_lprob, int32_t* d_kept, uint64_t* d_z_kept) {
    SC_API_BEGIN
    SC_CHECK(d_logits && d_stream && d_gen && d_position && d_tok && d_lprob && d_kept && d_z_kept, "sc_op_sample_rows: null argument");
    SampleArgs a;
    if (n_banned != 0) {  // read back and checked on the host first, as sc_op_beam_candidates_banned does
        SC_CHECK(n_banned > 0 && n_banned <= BANNED_MAX_SEQS && d_banned_tokens && d_banned_offsets && d_seqs,
                 "sc_op_sample_rows: bad banned list (n_banned=%d; needs d_seqs)", n_banned);
        const std::vector<int32_t> off = op_read_ints(d_banned_offsets, (size_t)n_banned + 1);
        SC_CHECK(off[0] == 0 && off[n_banned] >= 0 && off[n_banned] <= BANNED_MAX_TOKENS, "sc_op_sample_rows: bad offsets");
        for (int q = 0; q < n_banned; ++q) SC_CHECK(off[q + 1] >= off[q], "sc_op_sample_rows: offsets decrease at %d", q);
        const std::vector<int32_t> tok = op_read_ints(d_banned_tokens, (size_t)off[n_banned]);
        validate_banned_host(tok.data(), off.data(), n_banned, V, &a.banned.max_len);
        a.banned.tokens = d_banned_tokens, a.banned.offsets = d_banned_offsets, a.banned.n = n_banned;
    }
    a.logits = d_logits, a.ld = ld, a.rows = rows, a.V = V;
    a.stream = reinterpret_cast<const unsigned long long*>(d_stream), a.gen = d_gen, a.position = d_position;
    a.temperature = temperature, a.top_k = top_k, a.top_p = top_p, a.seed = seed;
    a.no_eos = no_eos, a.force_eos = force_eos, a.pad_idx = pad_idx, a.eos_idx = eos_idx, a.unk_idx = unk_idx, a.unk_penalty = unk_penalty;
    a.seqs_in = d_seqs, a.seq_ld = seq_ld, a.S = S, a.G = G;
    a.tok = d_tok, a.lprob = d_lprob, a.kept = d_kept, a.z_kept = reinterpret_cast<unsigned long long*>(d_z_kept);
    launch_sample_rows(a, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_beam_select(const float* d_cand_val, const int32_t* d_cand_idx, const int32_t* d_seqs_cur, int32_t* d_seqs_new, float* d_fin_score,
                      int32_t* d_fin_len, int32_t* d_fin_seq, int32_t* d_fin_count, int32_t* d_done, int32_t* d_remaining, int32_t* d_tok,
                      int32_t* d_src_row, float* d_cum, int32_t* d_anc, int32_t anc_ld, const int32_t* d_slot_utt, const int32_t* d_slots,
                      int32_t n, int32_t beams, int32_t K, int32_t V, int32_t max_len, int32_t step, int32_t eos_idx, int32_t pad_idx,
                      int32_t normalize, float len_penalty) {
    SC_API_BEGIN
    SC_CHECK(d_cand_val && d_cand_idx && d_seqs_cur && d_seqs_new && d_fin_score && d_fin_len && d_fin_seq && d_fin_count && d_done &&
                 d_remaining && d_tok && d_src_row && d_cum && (!d_anc || anc_ld >= 1),
             "sc_op_beam_select: null argument");
    SC_CHECK(n >= 1 && beams >= 1 && K >= 1 && V >= 1 && step >= 0 && step + 1 < max_len, "sc_op_beam_select: bad shape (n=%d beams=%d K=%d "
             "V=%d step=%d max_len=%d)", n, beams, K, V, step, max_len);
    for (int32_t c : op_read_ints(d_cand_idx, (size_t)n * K))
        SC_CHECK(c >= 0 && (int64_t)c < (int64_t)beams * V, "sc_op_beam_select: candidate index %d outside beams * V", c);
    if (d_slot_utt)
        for (int32_t u : op_read_ints(d_slot_utt, n)) SC_CHECK(u >= 0 && u < n, "sc_op_beam_select: slot_utt entry %d outside 0..%d", u, n - 1);
    const std::vector<int32_t> done = op_read_ints(d_done, n), count = op_read_ints(d_fin_count, n);
    for (int u = 0; u < n; ++u)  // a searching utterance has a free hypothesis slot
        SC_CHECK(done[u] || (count[u] >= 0 && count[u] < beams), "sc_op_beam_select: fin_count[%d] = %d with done = 0", u, count[u]);
    BeamSelectArgs a;
    a.cand_val = d_cand_val, a.cand_idx = d_cand_idx, a.seqs_cur = d_seqs_cur, a.seqs_new = d_seqs_new;
    a.fin_score = d_fin_score, a.fin_len = d_fin_len, a.fin_seq = d_fin_seq, a.fin_count = d_fin_count, a.done = d_done;
    a.remaining = d_remaining, a.tok = d_tok, a.src_row = d_src_row, a.cum = d_cum, a.anc = d_anc, a.anc_ld = anc_ld;
    a.slot_utt = d_slot_utt, a.d_slots = d_slots;
    a.beams = beams, a.K = K, a.V = V, a.max_len = max_len, a.step = step;
    a.eos_idx = eos_idx, a.pad_idx = pad_idx, a.normalize = normalize, a.len_penalty = len_penalty;
    launch_beam_select(a, n, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_beam_compact(const int32_t* d_done, int32_t* d_slot_utt, int32_t* d_slots, int32_t* d_rows, int32_t* d_seqs, float* d_cum,
                       int32_t* d_tok, int32_t* d_enc_lens, int32_t* d_anc, int32_t n, int32_t beams, int32_t max_len, int32_t anc_ld,
                       int32_t seq_len, int32_t anc_len) {
    SC_API_BEGIN
    SC_CHECK(d_slot_utt && d_slots && n >= 1 && n <= 1024, "sc_op_beam_compact: bad arguments (n=%d)", n);
    SC_CHECK(seq_len >= 0 && seq_len <= max_len && anc_len >= 0 && (!d_anc || anc_len <= anc_ld), "sc_op_beam_compact: bad lengths");
    const int32_t slots = op_read_ints(d_slots, 1)[0];
    SC_CHECK(slots >= 0 && slots <= n, "sc_op_beam_compact: *d_slots = %d outside 0..%d", slots, n);
    for (int32_t u : op_read_ints(d_slot_utt, slots)) SC_CHECK(u >= 0 && u < n, "sc_op_beam_compact: slot_utt entry %d outside 0..%d", u, n - 1);
    BeamCompactArgs a;
    a.done = d_done, a.slot_utt = d_slot_utt, a.d_slots = d_slots, a.d_rows = d_rows;
    a.seqs = d_seqs, a.cum = d_cum, a.tok = d_tok, a.enc_lens = d_enc_lens, a.anc = d_anc;
    a.n = n, a.beams = beams, a.max_len = max_len, a.anc_ld = anc_ld, a.seq_len = seq_len, a.anc_len = anc_len;
    launch_beam_compact(a, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

// the same walk with the score history (BeamHistArgs): beam_select_kernel<true>
int sc_op_beam_select_hist(const float* d_cand_val, const int32_t* d_cand_idx, const int32_t* d_seqs_cur, int32_t* d_seqs_new,
                           float* d_fin_score, int32_t* d_fin_len, int32_t* d_fin_seq, int32_t* d_fin_count, int32_t* d_done,
                           int32_t* d_remaining, int32_t* d_tok, int32_t* d_src_row, float* d_cum, int32_t* d_anc, int32_t anc_ld,
                           const int32_t* d_slot_utt, const int32_t* d_slots, int32_t n, int32_t beams, int32_t K, int32_t V, int32_t max_len,
                           int32_t step, int32_t eos_idx, int32_t pad_idx, int32_t normalize, float len_penalty, const float* d_hist_cur,
                           float* d_hist_new, float* d_fin_hist) {
    SC_API_BEGIN
    SC_CHECK(d_cand_val && d_cand_idx && d_seqs_cur && d_seqs_new && d_fin_score && d_fin_len && d_fin_seq && d_fin_count && d_done &&
                 d_remaining && d_tok && d_src_row && d_cum && (!d_anc || anc_ld >= 1) && d_hist_cur && d_hist_new && d_fin_hist,
             "sc_op_beam_select_hist: null argument");
    SC_CHECK(n >= 1 && beams >= 1 && K >= 1 && V >= 1 && step >= 0 && step + 1 < max_len, "sc_op_beam_select_hist: bad shape (n=%d beams=%d K=%d "
             "V=%d step=%d max_len=%d)", n, beams, K, V, step, max_len);
    for (int32_t c : op_read_ints(d_cand_idx, (size_t)n * K))
        SC_CHECK(c >= 0 && (int64_t)c < (int64_t)beams * V, "sc_op_beam_select_hist: candidate index %d outside beams * V", c);
    if (d_slot_utt)
        for (int32_t u : op_read_ints(d_slot_utt, n)) SC_CHECK(u >= 0 && u < n, "sc_op_beam_select_hist: slot_utt entry %d outside 0..%d", u, n - 1);
    if (d_slots) {
        const int32_t slots = op_read_ints(d_slots, 1)[0];
        SC_CHECK(slots >= 0 && slots <= n, "sc_op_beam_select_hist: *d_slots = %d outside 0..%d", slots, n);
    }
    const std::vector<int32_t> done = op_read_ints(d_done, n), count = op_read_ints(d_fin_count, n);
    for (int u = 0; u < n; ++u)  // a searching utterance has a free hypothesis slot
        SC_CHECK(done[u] || (count[u] >= 0 && count[u] < beams), "sc_op_beam_select_hist: fin_count[%d] = %d with done = 0", u, count[u]);
    BeamSelectArgs a;
    a.cand_val = d_cand_val, a.cand_idx = d_cand_idx, a.seqs_cur = d_seqs_cur, a.seqs_new = d_seqs_new;
    a.fin_score = d_fin_score, a.fin_len = d_fin_len, a.fin_seq = d_fin_seq, a.fin_count = d_fin_count, a.done = d_done;
    a.remaining = d_remaining, a.tok = d_tok, a.src_row = d_src_row, a.cum = d_cum, a.anc = d_anc, a.anc_ld = anc_ld;
    a.slot_utt = d_slot_utt, a.d_slots = d_slots;
    BeamHistArgs h;
    h.cur = d_hist_cur, h.next = d_hist_new, h.fin = d_fin_hist;
    a.beams = beams, a.K = K, a.V = V, a.max_len = max_len, a.step = step;
    a.eos_idx = eos_idx, a.pad_idx = pad_idx, a.normalize = normalize, a.len_penalty = len_penalty;
    launch_beam_select(a, n, g_op_stream, &h);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_beam_compact_hist(const int32_t* d_done, int32_t* d_slot_utt, int32_t* d_slots, int32_t* d_rows, int32_t* d_seqs, float* d_cum,
                            int32_t* d_tok, int32_t* d_enc_lens, int32_t* d_anc, int32_t n, int32_t beams, int32_t max_len, int32_t anc_ld,
                            int32_t seq_len, int32_t anc_len, float* d_hist) {
    SC_API_BEGIN
    SC_CHECK(d_slot_utt && d_slots && d_hist && n >= 1 && n <= 1024, "sc_op_beam_compact_hist: bad arguments (n=%d)", n);
    SC_CHECK(seq_len >= 0 && seq_len <= max_len && anc_len >= 0 && (!d_anc || anc_len <= anc_ld), "sc_op_beam_compact_hist: bad lengths");
    const int32_t slots = op_read_ints(d_slots, 1)[0];
    SC_CHECK(slots >= 0 && slots <= n, "sc_op_beam_compact_hist: *d_slots = %d outside 0..%d", slots, n);
    for (int32_t u : op_read_ints(d_slot_utt, slots)) SC_CHECK(u >= 0 && u < n, "sc_op_beam_compact_hist: slot_utt entry %d outside 0..%d", u, n - 1);
    BeamCompactArgs a;
    a.done = d_done, a.slot_utt = d_slot_utt, a.d_slots = d_slots, a.d_rows = d_rows;
    a.seqs = d_seqs, a.cum = d_cum, a.tok = d_tok, a.enc_lens = d_enc_lens, a.anc = d_anc;
    a.n = n, a.beams = beams, a.max_len = max_len, a.anc_ld = anc_ld, a.seq_len = seq_len, a.anc_len = anc_len;
    launch_beam_compact(a, g_op_stream, d_hist);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_beam_nbest(const int32_t* d_fin_seq, const int32_t* d_fin_len, const float* d_fin_score, const float* d_fin_hist,
                     const int32_t* d_fin_count, int32_t n, int32_t beams, int32_t nbest, int32_t max_len, int32_t pad_idx, int32_t* d_out_ids,
                     int32_t* d_out_lens, float* d_out_scores, int32_t* d_out_counts, float* d_out_step) {
    SC_API_BEGIN
    SC_CHECK(d_fin_seq && d_fin_len && d_fin_score && d_fin_hist && d_fin_count && d_out_ids && d_out_lens && d_out_scores && d_out_counts &&
                 d_out_step,
             "sc_op_beam_nbest: null argument");
    SC_CHECK(n >= 1 && beams >= 1 && beams <= 8 && nbest >= 1 && nbest <= beams && max_len >= 1,
             "sc_op_beam_nbest: bad shape (n=%d beams=%d nbest=%d max_len=%d)", n, beams, nbest, max_len);
    const std::vector<int32_t> count = op_read_ints(d_fin_count, n), lens = op_read_ints(d_fin_len, (size_t)n * beams);
    for (int u = 0; u < n; ++u) {
        SC_CHECK(count[u] >= 0 && count[u] <= beams, "sc_op_beam_nbest: fin_count[%d] = %d outside 0..%d", u, count[u], beams);
        for (int i = 0; i < count[u]; ++i)
            SC_CHECK(lens[(size_t)u * beams + i] >= 0 && lens[(size_t)u * beams + i] <= max_len, "sc_op_beam_nbest: fin_len[%d][%d] = %d", u, i,
                     lens[(size_t)u * beams + i]);
    }
    BeamNbestArgs a;
    a.fin_seq = d_fin_seq, a.fin_len = d_fin_len, a.fin_score = d_fin_score, a.fin_hist = d_fin_hist, a.fin_count = d_fin_count;
    a.out_ids = d_out_ids, a.out_lens = d_out_lens, a.out_scores = d_out_scores, a.out_counts = d_out_counts, a.out_step = d_out_step;
    a.n = n, a.beams = beams, a.nbest = nbest, a.max_len = max_len, a.pad_idx = pad_idx;
    launch_beam_nbest(a, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_gather_cache(const float* d_src, float* d_dst, const int32_t* d_src_row, int32_t rows, int32_t len, int32_t cap, int32_t M,
                       int32_t layers, int64_t layer_stride) {
    SC_API_BEGIN
    SC_CHECK(d_src && d_dst && d_src_row && rows >= 1 && layers >= 1 && len <= cap && layer_stride >= (int64_t)rows * cap * M,
             "sc_op_gather_cache: bad arguments");
    for (int32_t r : op_read_ints(d_src_row, rows)) SC_CHECK(r >= 0 && r < rows, "sc_op_gather_cache: source row %d outside 0..%d", r, rows - 1);
    launch_gather_cache(d_src, d_dst, d_src_row, rows, len, cap, M, layers, layer_stride, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_row_token_lprob(const float* d_logits, int64_t ld, int32_t rows, int32_t V, int32_t row_stride, int32_t token, float* d_out) {
    SC_API_BEGIN
    SC_CHECK(d_logits && d_out && rows >= 1 && V >= 1 && ld >= V && row_stride >= 1, "sc_op_row_token_lprob: bad arguments");
    launch_row_token_lprob(d_logits, ld, rows, V, row_stride, token, d_out, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

/* ---- decode-engine / beam modes of the step kernels and the engine / greedy bookkeeping (tests/test_engine_kernels_gpu.py) ----
 * Every hook reads the index tables it is handed back to the host and refuses entries that would take a kernel outside the
 * buffers the caller described: the kernels themselves trust their tables. */

static void op_check_slot_table(const char* who, const int32_t* d_slot_rp, int32_t slots, int32_t n_states, int32_t pos_end) {
    const std::vector<int32_t> rp = op_read_ints(d_slot_rp, (size_t)2 * slots);
    for (int s = 0; s < slots; ++s)
        SC_CHECK(rp[2 * s] >= 0 && rp[2 * s] < n_states && rp[2 * s + 1] >= 0 && rp[2 * s + 1] < pos_end,
                 "%s: slot %d = {row state %d, position %d} outside %d row states / %d positions", who, s, rp[2 * s], rp[2 * s + 1], n_states, pos_end);
}

/* sc_op_dstep_attention with the remaining fields of DAttnArgs (nullable device pointers) and up to 512 rows.  The caches hold
 * `cache_rows` rows ([cache_rows][cap][M], cross: [cache_rows][cap][2M]); d_lens is indexed like the caches' owner (row state
 * in engine mode, live row otherwise).  The output planes are NaN before the launch: a row the kernel skips reads back as NaN. */
int sc_op_dstep_attention_ex(const float* d_proj, int32_t S, const float* d_bias, float* d_kcache, float* d_vcache, int32_t cap,
                             int32_t cache_rows, int32_t pos, const int32_t* d_lens, int32_t cross, int32_t nb, int32_t heads,
                             const int32_t* d_slot_rp, const int32_t* d_slot_lane, const int32_t* d_anc, const int32_t* d_kv_item,
                             int32_t kv_row_div, const int32_t* d_rows, float* d_out) {
    SC_API_BEGIN
    SC_CHECK(nb >= 1 && nb <= 512 && heads >= 1 && S >= 1 && cap >= 1 && cache_rows >= 1 && kv_row_div >= 1 && d_proj && d_kcache && d_out,
             "sc_op_dstep_attention_ex: bad shape");
    SC_CHECK(cross ? d_lens != nullptr : (d_vcache != nullptr && pos >= 0 && pos < cap), "sc_op_dstep_attention_ex: bad cache arguments");
    int live = nb;
    if (d_rows) {
        live = op_read_ints(d_rows, 1)[0];
        SC_CHECK(live >= 0 && live <= nb, "sc_op_dstep_attention_ex: *d_rows = %d outside 0..%d", live, nb);
    }
    if (d_slot_rp) {
        // self-attention indexes nothing by the row state: its cache row is the slot's lane
        op_check_slot_table("sc_op_dstep_attention_ex", d_slot_rp, nb, cross ? cache_rows : 0x7fffffff, cap);
        if (!cross) {
            SC_CHECK(d_slot_lane, "sc_op_dstep_attention_ex: the engine's self-attention needs d_slot_lane");
            for (int32_t l : op_read_ints(d_slot_lane, nb)) SC_CHECK(l >= 0 && l < cache_rows, "sc_op_dstep_attention_ex: lane %d outside 0..%d", l, cache_rows - 1);
        }
    } else if (cross) {
        if (d_kv_item) {
            for (int32_t u : op_read_ints(d_kv_item, (size_t)(nb - 1) / kv_row_div + 1))
                SC_CHECK(u >= 0 && u < cache_rows, "sc_op_dstep_attention_ex: kv_item entry %d outside 0..%d", u, cache_rows - 1);
        } else {
            SC_CHECK((nb - 1) / kv_row_div < cache_rows, "sc_op_dstep_attention_ex: %d rows / %d need more than %d cache rows", nb, kv_row_div, cache_rows);
        }
    } else {
        SC_CHECK(nb <= cache_rows, "sc_op_dstep_attention_ex: %d rows append to %d cache rows", nb, cache_rows);
        if (d_anc) {
            SC_CHECK((int64_t)cache_rows * cap * heads * 64 * 4 < (1ll << 32), "sc_op_dstep_attention_ex: cache too large for the ancestor-table addressing");
            const std::vector<int32_t> anc = op_read_ints(d_anc, (size_t)nb * cap);
            for (int b = 0; b < nb; ++b)
                for (int j = 0; j <= pos; ++j)
                    SC_CHECK(anc[(size_t)b * cap + j] >= 0 && anc[(size_t)b * cap + j] < cache_rows, "sc_op_dstep_attention_ex: anc[%d][%d] = %d outside 0..%d",
                             b, j, anc[(size_t)b * cap + j], cache_rows - 1);
        }
    }
    OpScratch scratch;
    const int M = heads * 64, RB = op_row_slots(nb);
    __half* oh = scratch.get<__half>((size_t)M * RB);
    __half* ol = scratch.get<__half>((size_t)M * RB);
    SC_HIP(hipMemsetAsync(oh, 0xff, (size_t)M * RB * 2, g_op_stream));
    SC_HIP(hipMemsetAsync(ol, 0xff, (size_t)M * RB * 2, g_op_stream));
    int* d_pos = op_device_int(scratch, pos);
    DAttnArgs a;
    a.q = d_proj;
    a.S = S;
    a.bias = d_bias;
    a.cap = cap;
    a.Oh = oh, a.Ol = ol, a.ORB = RB;
    a.nb = nb, a.heads = heads;
    a.d_rows = d_rows;
    a.slot_rp = reinterpret_cast<const int2*>(d_slot_rp);
    if (cross) {
        a.ldq = M, a.sstride = (int64_t)nb * M;
        a.kcache = d_kcache, a.vcache = d_kcache + M;
        a.cache_ld = 2 * M, a.cache_bs = (int64_t)cap * 2 * M;
        a.kv_lens = d_lens;
        a.kv_row_div = kv_row_div, a.kv_item = d_kv_item;
    } else {
        a.ldq = 3 * M, a.sstride = (int64_t)nb * 3 * M;
        a.koff = M, a.voff = 2 * M;
        a.kcache = d_kcache, a.vcache = d_vcache;
        a.cache_ld = M, a.cache_bs = (int64_t)cap * M;
        a.d_pos = d_pos;
        a.anc = d_anc;
        a.slot_lane = d_slot_lane;
    }
    launch_dattn(a, cross != 0, g_op_stream);
    launch_planes_to_rows(oh, ol, RB, d_out, M, nb, M, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

/* The closing pair of an engine step: launch_vocab3 in slot mode (x [M][K] fp32 -> planes, W [N][K] fp16 packed here) and
 * launch_engine_finalize on the caller's EngineRows arrays (n_states row states, hist [n_states][cap]).  Slot m of the first
 * *d_rows works on row state d_slot_rp[m].x at position d_slot_rp[m].y. */
int sc_op_engine_step_close(const float* d_x, const void* d_w_f16, int32_t M, int32_t N, int32_t K, int32_t min_step_for_eos, int32_t pad_idx,
                            int32_t eos_idx, int32_t unk_idx, float unk_penalty, int32_t* d_slot_rp, const int32_t* d_rows, int32_t n_states,
                            int32_t cap, int32_t* d_tok, int32_t* d_pos, int32_t* d_finished, int32_t* d_out_len, const int32_t* d_limit,
                            const int32_t* d_prefix_len, float* d_score, int32_t* d_hist) {
    SC_API_BEGIN
    SC_CHECK(vocab3_supported(M, N, K), "sc_op_engine_step_close: M=%d N=%d K=%d unsupported", M, N, K);
    SC_CHECK(d_x && d_w_f16 && d_slot_rp && d_rows && n_states >= 1 && cap >= 2 && d_tok && d_pos && d_finished && d_out_len && d_limit &&
                 d_prefix_len && d_score && d_hist,
             "sc_op_engine_step_close: null argument");
    const int32_t live = op_read_ints(d_rows, 1)[0];
    SC_CHECK(live >= 0 && live <= M, "sc_op_engine_step_close: *d_rows = %d outside 0..%d", live, M);
    op_check_slot_table("sc_op_engine_step_close", d_slot_rp, M, n_states, cap - 1);  // hist[r][pos + 1] is written
    OpScratch scratch;
    const int RB = op_row_slots(M);
    const int groups = vocab3_groups(M);
    float4* part = op_filled<float4>(scratch, (size_t)groups * M, 0xff);
    float* eos_logit = op_filled<float>(scratch, M, 0xff);
    const OpPlanes x = op_planes(scratch, d_x, M, K, RB);
    Vocab3Args v;
    v.Wp = op_packed_weight(scratch, d_w_f16, N, K), v.Ah = x.hi, v.Al = x.lo, v.RB = RB, v.M = M, v.N = N, v.K = K;
    v.am = op_argmax_epi(part, groups, eos_logit, nullptr, min_step_for_eos, -1, pad_idx, eos_idx, unk_idx, unk_penalty);
    v.d_rows = d_rows;
    v.slot_rp = reinterpret_cast<const int2*>(d_slot_rp), v.limit_row = d_limit;
    launch_vocab3(v, g_op_stream);
    EngineFinalizeArgs f;
    f.part = part, f.tiles = groups, f.slots = M, f.eos_logit = eos_logit;
    f.slot_rp = reinterpret_cast<int2*>(d_slot_rp), f.d_rows = d_rows, f.pad_idx = pad_idx, f.eos_idx = eos_idx;
    f.rows.tok = d_tok, f.rows.pos = d_pos, f.rows.finished = d_finished, f.rows.out_len = d_out_len;
    f.rows.limit = const_cast<int32_t*>(d_limit), f.rows.prefix_len = const_cast<int32_t*>(d_prefix_len), f.rows.score = d_score;
    f.rows.hist = d_hist, f.rows.cap = cap, f.rows.M = K;
    launch_engine_finalize(f, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

/* launch_engine_admit: d_recs [n][4 + ENGINE_MAX_PREFIX] ints = {row state, limit, prefix_len, enc_len, prefix tokens} */
int sc_op_engine_admit(const int32_t* d_recs, int32_t n, int32_t n_states, int32_t cap, int32_t pad_idx, int32_t* d_tok, int32_t* d_pos,
                       int32_t* d_finished, int32_t* d_out_len, int32_t* d_limit, int32_t* d_prefix_len, int32_t* d_enc_lens, float* d_score,
                       int32_t* d_hist) {
    SC_API_BEGIN
    static_assert(sizeof(EngineAdmitRec) == (4 + ENGINE_MAX_PREFIX) * 4, "EngineAdmitRec is a row of ints");
    SC_CHECK(d_recs && n >= 0 && n_states >= 1 && cap >= 1 && d_tok && d_pos && d_finished && d_out_len && d_limit && d_prefix_len && d_enc_lens &&
                 d_score && d_hist,
             "sc_op_engine_admit: null argument");
    const std::vector<int32_t> recs = op_read_ints(d_recs, (size_t)n * (4 + ENGINE_MAX_PREFIX));
    for (int i = 0; i < n; ++i) {
        const int32_t* r = recs.data() + (size_t)i * (4 + ENGINE_MAX_PREFIX);
        SC_CHECK(r[0] >= 0 && r[0] < n_states && r[2] >= 1 && r[2] <= ENGINE_MAX_PREFIX, "sc_op_engine_admit: record %d: row state %d, prefix of %d", i, r[0], r[2]);
    }
    EngineRows R;
    R.tok = d_tok, R.pos = d_pos, R.finished = d_finished, R.out_len = d_out_len, R.limit = d_limit, R.prefix_len = d_prefix_len;
    R.enc_lens = d_enc_lens, R.score = d_score, R.hist = d_hist, R.cap = cap;
    launch_engine_admit(reinterpret_cast<const EngineAdmitRec*>(d_recs), n, R, pad_idx, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

/* launch_engine_set_slots: d_rids [2][slots] = row states, then K / V lanes; d_pos [n_states] */
int sc_op_engine_set_slots(const int32_t* d_rids, int32_t n_live, int32_t slots, int32_t n_states, int32_t* d_slot_rp, int32_t* d_slot_lane,
                           const int32_t* d_pos, int32_t* d_rows) {
    SC_API_BEGIN
    SC_CHECK(d_rids && slots >= 1 && n_live >= 0 && n_live <= slots && n_states >= 1 && d_slot_rp && d_slot_lane && d_pos && d_rows,
             "sc_op_engine_set_slots: bad argument");
    for (int32_t r : op_read_ints(d_rids, n_live)) SC_CHECK(r >= 0 && r < n_states, "sc_op_engine_set_slots: row state %d outside 0..%d", r, n_states - 1);
    launch_engine_set_slots(d_rids, n_live, slots, reinterpret_cast<int2*>(d_slot_rp), d_slot_lane, d_pos, d_rows, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

/* launch_engine_retire: record i = {h_rid[i], h_dst_rows[i], h_dst[i]} (host arrays; h_dst holds device pointers, entries may
 * be NULL); d_hidden [n_states][cap - 1][M]; d_stage [n][2 + cap] */
int sc_op_engine_retire(const int32_t* h_rid, const int32_t* h_dst_rows, float* const* h_dst, int32_t n, int32_t n_states, int32_t cap, int32_t M,
                        const int32_t* d_out_len, const float* d_score, const int32_t* d_hist, const float* d_hidden, int32_t* d_stage) {
    SC_API_BEGIN
    SC_CHECK(h_rid && h_dst_rows && h_dst && n >= 0 && n_states >= 1 && cap >= 2 && d_out_len && d_score && d_hist && d_hidden && d_stage,
             "sc_op_engine_retire: null argument");
    std::vector<EngineRetireRec> recs(n);
    for (int i = 0; i < n; ++i) {
        SC_CHECK(h_rid[i] >= 0 && h_rid[i] < n_states && h_dst_rows[i] >= 0, "sc_op_engine_retire: record %d: row state %d, %d rows", i, h_rid[i], h_dst_rows[i]);
        recs[i].rid = h_rid[i], recs[i].dst_rows = h_dst_rows[i], recs[i].dst = h_dst[i];
    }
    OpScratch scratch;
    EngineRetireRec* d_recs = scratch.get<EngineRetireRec>((size_t)std::max(n, 1));
    if (n) SC_HIP(hipMemcpyAsync(d_recs, recs.data(), (size_t)n * sizeof(EngineRetireRec), hipMemcpyHostToDevice, g_op_stream));
    EngineRows R;
    R.out_len = const_cast<int32_t*>(d_out_len), R.score = const_cast<float*>(d_score), R.hist = const_cast<int32_t*>(d_hist);
    R.hidden = const_cast<float*>(d_hidden), R.cap = cap, R.M = M;
    launch_engine_retire(d_recs, n, R, d_stage, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

/* launch_embed3 with the engine's slot table (nullable, like d_rows): x [rows][C] = embed[tok[..]] * scale + pos_table[..] read
 * back from the k-group-major stream, which is NaN before the launch.  d_tok holds n_states tokens (rows without the table),
 * the embedding `vocab` rows, the position table n_pos rows; pos: the scalar position without the table. */
int sc_op_dstep3_embed_ex(const int32_t* d_tok, const void* d_embed_f16, float scale, const float* d_pos_table, int32_t pos,
                          const int32_t* d_slot_rp, const int32_t* d_rows, int32_t rows, int32_t C, int32_t n_states, int32_t n_pos, int32_t vocab,
                          float* d_x) {
    SC_API_BEGIN
    SC_CHECK(d_tok && d_embed_f16 && d_pos_table && d_x && rows >= 1 && rows <= 512 && n_states >= 1 && pos >= 0 && pos < n_pos && vocab >= 1,
             "sc_op_dstep3_embed_ex: bad argument");
    SC_CHECK(d_slot_rp || n_states >= rows, "sc_op_dstep3_embed_ex: %d rows read %d tokens", rows, n_states);
    if (d_slot_rp) op_check_slot_table("sc_op_dstep3_embed_ex", d_slot_rp, rows, n_states, n_pos);
    for (int32_t t : op_read_ints(d_tok, n_states)) SC_CHECK(t >= 0 && t < vocab, "sc_op_dstep3_embed_ex: token %d outside 0..%d", t, vocab - 1);
    if (d_rows) {
        const int32_t live = op_read_ints(d_rows, 1)[0];
        SC_CHECK(live >= 0 && live <= rows, "sc_op_dstep3_embed_ex: *d_rows = %d outside 0..%d", live, rows);
    }
    OpScratch scratch;
    const int RB = op_row_slots(rows);
    float* xg = scratch.get<float>((size_t)C * RB);
    SC_HIP(hipMemsetAsync(xg, 0xff, (size_t)C * RB * 4, g_op_stream));
    int* d_pos = op_device_int(scratch, pos);
    launch_embed3(d_tok, static_cast<const __half*>(d_embed_f16), scale, d_pos_table, d_pos, xg, RB, rows, C, g_op_stream,
                  reinterpret_cast<const int2*>(d_slot_rp), d_rows);
    launch_kgm_to_rows(xg, RB, d_x, C, rows, C, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

/* launch_reduce3 as the step's last launch runs it: x [rows][C] += bias + sum of the S partials [S][rows][C], h =
 * LayerNorm(x) -> d_h [rows][C] and the captured row d_hrow[owner][pos][C] (owner stride hrow_bs floats, positions
 * 0 .. hrow_rows-1; owner / position = the slot table's, without it the row itself at `pos`).  d_hrow holds n_states owners. */
int sc_op_dstep3_reduce_capture_ex(const float* d_partial, int32_t S, const float* d_bias, float* d_x_inout, const float* d_gamma, const float* d_beta,
                                   float* d_h, float* d_hrow, int64_t hrow_bs, int32_t hrow_rows, int32_t pos, const int32_t* d_slot_rp,
                                   const int32_t* d_rows, int32_t rows, int32_t C, int32_t n_states) {
    SC_API_BEGIN
    SC_CHECK(d_partial && d_x_inout && d_gamma && d_beta && d_h && d_hrow && S >= 1 && rows >= 1 && rows <= 512 && n_states >= 1 && pos >= 0 &&
                 hrow_rows >= 0 && hrow_bs >= (int64_t)hrow_rows * C,
             "sc_op_dstep3_reduce_capture_ex: bad argument");
    SC_CHECK(d_slot_rp || n_states >= rows, "sc_op_dstep3_reduce_capture_ex: %d rows capture into %d owners", rows, n_states);
    if (d_slot_rp) op_check_slot_table("sc_op_dstep3_reduce_capture_ex", d_slot_rp, rows, n_states, 0x7fffffff);
    if (d_rows) {
        const int32_t live = op_read_ints(d_rows, 1)[0];
        SC_CHECK(live >= 0 && live <= rows, "sc_op_dstep3_reduce_capture_ex: *d_rows = %d outside 0..%d", live, rows);
    }
    OpScratch scratch;
    const int RB = op_row_slots(rows);
    float* xg = scratch.get<float>((size_t)C * RB);
    SC_HIP(hipMemsetAsync(xg, 0xff, (size_t)C * RB * 4, g_op_stream));
    int* d_pos = op_device_int(scratch, pos);
    launch_rows_to_kgm(d_x_inout, C, rows, C, RB, xg, g_op_stream);
    Reduce3Args r;
    r.partial = d_partial, r.S = S, r.bias = d_bias, r.xg = xg, r.XRB = RB, r.rows = rows, r.C = C;
    r.gamma = d_gamma, r.beta = d_beta, r.hfix = d_h;
    r.hrow = d_hrow, r.hrow_bs = hrow_bs, r.hrow_rows = hrow_rows, r.d_pos = d_pos;
    r.d_rows = d_rows, r.slot_rp = reinterpret_cast<const int2*>(d_slot_rp);
    launch_reduce3(r, g_op_stream);
    launch_kgm_to_rows(xg, RB, d_x_inout, C, rows, C, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

/* launch_step_update at host position `pos` (hist [nb][hist_ld]; d_score / d_n_unfinished nullable) */
int sc_op_step_update(int32_t* d_next_tok, int32_t* d_hist, int32_t hist_ld, int32_t* d_finished, int32_t* d_out_len, const float* d_lprob,
                      float* d_score, int32_t nb, int32_t pos, int32_t pad_idx, int32_t eos_idx, int32_t* d_n_unfinished) {
    SC_API_BEGIN
    SC_CHECK(d_next_tok && d_hist && d_finished && d_out_len && (d_lprob || !d_score) && nb >= 1 && pos >= 0 && pos + 1 < hist_ld,
             "sc_op_step_update: bad argument");
    OpScratch scratch;
    int* d_pos = op_device_int(scratch, pos);
    launch_step_update(d_next_tok, d_hist, hist_ld, d_finished, d_out_len, d_lprob, d_score, nb, d_pos, pad_idx, eos_idx, d_n_unfinished, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

/* launch_row_swap: d_k / d_v [layers][n_rows][cap][M], d_cross [layers][n_rows][s_enc][2M], h_src / h_dst [pairs] host arrays,
 * per-row state of n_rows rows, d_hidden [n_rows][cap - 1][M] or NULL */
int sc_op_row_swap(float* d_k, float* d_v, float* d_cross, int32_t layers, int32_t pairs, const int32_t* h_src, const int32_t* h_dst, int32_t n_rows,
                   int32_t M, int32_t cap, int32_t s_enc, int32_t filled, int32_t* d_tok, int32_t* d_finished, int32_t* d_out_len,
                   int32_t* d_enc_lens, float* d_lprob, float* d_score, int32_t* d_hist, float* d_hidden) {
    SC_API_BEGIN
    SC_CHECK(d_k && d_v && d_cross && h_src && h_dst && layers >= 1 && layers <= ROWSWAP_MAX_LAYERS && pairs >= 0 && pairs <= ROWSWAP_MAX_PAIRS &&
                 n_rows >= 1 && n_rows <= 256 && cap >= 2 && s_enc >= 1,
             "sc_op_row_swap: bad argument");
    RowSwapArgs a;
    for (int li = 0; li < layers; ++li) {
        a.k[li] = d_k + (int64_t)li * n_rows * cap * M;
        a.v[li] = d_v + (int64_t)li * n_rows * cap * M;
        a.cross[li] = d_cross + (int64_t)li * n_rows * s_enc * 2 * M;
    }
    a.layers = layers, a.pairs = pairs;
    for (int i = 0; i < pairs; ++i) {
        SC_CHECK(h_src[i] >= 0 && h_src[i] < n_rows && h_dst[i] >= 0 && h_dst[i] < n_rows, "sc_op_row_swap: pair %d = (%d, %d) outside 0..%d", i, h_src[i],
                 h_dst[i], n_rows - 1);
        a.src[i] = (unsigned char)h_src[i], a.dst[i] = (unsigned char)h_dst[i];
    }
    a.M = M, a.cap = cap, a.s_enc = s_enc, a.filled = filled;
    a.tok = d_tok, a.finished = d_finished, a.out_len = d_out_len, a.enc_lens = d_enc_lens, a.lprob = d_lprob, a.score = d_score;
    a.hist = d_hist, a.hidden = d_hidden;
    launch_row_swap(a, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

// ---- the row kernels between the products (k_norm.hip, k_misc.hip), op level ----------------------------------------

int sc_op_layernorm_ex(const float* d_x, int64_t ldx, const float* d_gamma, const float* d_beta, float* d_y, int64_t ldy, void* d_yh_f16,
                       void* d_yl_f16, int64_t ldh, int32_t rows, int32_t C, int32_t act, const int32_t* d_lens, int32_t t_per_batch) {
    SC_API_BEGIN
    SC_CHECK(d_x && d_gamma && d_beta && (d_y || d_yh_f16) && !d_yh_f16 == !d_yl_f16 && (!d_lens || t_per_batch > 0),
             "sc_op_layernorm_ex: bad argument");
    __half* yh = static_cast<__half*>(d_yh_f16);
    __half* yl = static_cast<__half*>(d_yl_f16);
    if (!yh) launch_layernorm(d_x, ldx, d_gamma, d_beta, d_y, ldy, rows, C, act, d_lens, t_per_batch, g_op_stream);
    else if (!d_y) launch_layernorm_split(d_x, ldx, d_gamma, d_beta, yh, yl, ldh, rows, C, act, d_lens, t_per_batch, g_op_stream);
    else launch_layernorm_both(d_x, ldx, d_gamma, d_beta, d_y, ldy, yh, yl, ldh, rows, C, act, d_lens, t_per_batch, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_embed_tokens(const int32_t* d_tok, int32_t rows, const void* d_emb_f16, int32_t M, float scale, const float* d_pos_table,
                       const int32_t* d_pos, int32_t t_per_batch, float* d_out, int64_t ldo) {
    SC_API_BEGIN
    SC_CHECK(d_tok && d_emb_f16 && d_pos_table && d_out && M > 0 && ldo >= M && t_per_batch >= 0, "sc_op_embed_tokens: bad argument");
    launch_embed_tokens(d_tok, rows, static_cast<const __half*>(d_emb_f16), M, scale, d_pos_table, d_pos, t_per_batch, d_out, ldo, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_gather_rows(const float* d_src, int64_t lds, const int32_t* d_idx, const float* d_add, int64_t ld_add, int32_t rows_per_item,
                      float* d_dst, int64_t ldd, int32_t rows, int32_t C) {
    SC_API_BEGIN
    SC_CHECK(d_src && d_idx && d_dst && C > 0 && lds >= C && ldd >= C, "sc_op_gather_rows: bad argument");
    if (d_add) launch_gather_rows_add(d_src, lds, d_idx, d_add, ld_add, rows_per_item, d_dst, ldd, rows, C, g_op_stream);
    else launch_gather_rows(d_src, lds, d_idx, d_dst, ldd, rows, C, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_char_embed_add(float* d_seqs, int64_t ld, const int32_t* d_char_ids, const void* d_embed_f16, const float* d_pos_table,
                         int32_t t_per_batch, float alpha, float scale, int32_t rows, int32_t M) {
    SC_API_BEGIN
    SC_CHECK(d_seqs && d_char_ids && d_embed_f16 && d_pos_table && t_per_batch > 0 && M > 0 && ld >= M, "sc_op_char_embed_add: bad argument");
    launch_char_embed_add(d_seqs, ld, d_char_ids, static_cast<const __half*>(d_embed_f16), d_pos_table, t_per_batch, alpha, scale, rows, M,
                          g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_pos_add(float* d_seqs, int64_t ld, const float* d_pos_table, int32_t t_per_batch, const int32_t* d_row_t, float alpha, int32_t rows,
                  int32_t M) {
    SC_API_BEGIN
    SC_CHECK(d_seqs && d_pos_table && (d_row_t || t_per_batch > 0) && M > 0 && ld >= M, "sc_op_pos_add: bad argument");
    if (d_row_t) launch_pos_add_rows(d_seqs, ld, d_pos_table, d_row_t, alpha, rows, M, g_op_stream);
    else launch_pos_add(d_seqs, ld, d_pos_table, t_per_batch, alpha, rows, M, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_durations(const float* d_h, int64_t ld, const float* d_w, const float* d_b, int32_t rows, int32_t H, int32_t t_per_batch,
                    const int32_t* d_lens, float duration_factor, int32_t min_dur, int32_t* d_durations) {
    SC_API_BEGIN
    SC_CHECK(d_h && d_w && d_b && d_durations && H > 0 && ld >= H && t_per_batch > 0, "sc_op_durations: bad argument");
    launch_durations(d_h, ld, d_w, d_b, rows, H, t_per_batch, d_lens, duration_factor, min_dur, d_durations, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_vocoder_embed(const int32_t* d_units, int32_t nb, int32_t T, const void* d_dict_f16, int32_t E, const void* d_lang_f16, int32_t Lg,
                        const int32_t* d_lang_idx, const void* d_spkr_f16, int32_t Sp, const int32_t* d_spkr_idx, float* d_out,
                        const int32_t* d_item_off, int32_t rows_total) {
    SC_API_BEGIN
    SC_CHECK(d_units && d_dict_f16 && d_lang_idx && d_spkr_idx && d_out && nb > 0 && E > 0 && Lg >= 0 && Sp >= 0 && (d_item_off || T > 0),
             "sc_op_vocoder_embed: bad argument");
    launch_vocoder_embed(d_units, nb, T, static_cast<const __half*>(d_dict_f16), E, static_cast<const __half*>(d_lang_f16), Lg, d_lang_idx,
                         static_cast<const __half*>(d_spkr_f16), Sp, d_spkr_idx, d_out, g_op_stream, d_item_off, rows_total);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_item_row_pos(const int32_t* d_item_off, int32_t n_items, int32_t mul, int32_t rows, int32_t* d_row_pos) {
    SC_API_BEGIN
    SC_CHECK(d_item_off && d_row_pos && n_items > 0 && mul > 0 && (reinterpret_cast<uintptr_t>(d_row_pos) & 7) == 0,
             "sc_op_item_row_pos: bad argument");
    launch_item_row_pos(d_item_off, n_items, mul, rows, reinterpret_cast<int2*>(d_row_pos), g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_scatter_items(const float* d_src, const int32_t* d_item_off, const int32_t* d_item_of, int32_t n_items, int32_t mul, int32_t longest,
                        int64_t dst_stride, float* d_dst) {
    SC_API_BEGIN
    SC_CHECK(d_src && d_item_off && d_item_of && d_dst && mul > 0 && dst_stride >= longest, "sc_op_scatter_items: bad argument");
    launch_scatter_items(d_src, d_item_off, d_item_of, n_items, mul, longest, dst_stride, d_dst, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_glu_dwconv_ex(const float* d_x, const float* d_w, float* d_y, int32_t nb, int32_t T, int32_t C, int32_t k, const int32_t* d_lens,
                        int32_t left, const float* d_bn_g, const float* d_bn_b, const float* d_bn_mean, const float* d_bn_var) {
    SC_API_BEGIN
    SC_CHECK(d_x && d_w && d_y && C > 0 && k > 0 && left < k, "sc_op_glu_dwconv_ex: bad argument");
    SC_CHECK(!d_bn_g == !d_bn_b && !d_bn_g == !d_bn_mean && !d_bn_g == !d_bn_var, "sc_op_glu_dwconv_ex: BatchNorm needs g, b, mean and var");
    OpScratch scratch;
    float* fold = nullptr;
    if (d_bn_g) {  // the load-time fold of the v1 encoder layer (model_load.hip)
        fold = scratch.get<float>((size_t)2 * C);
        launch_bn_fold(d_bn_g, d_bn_b, d_bn_mean, d_bn_var, 1e-5f, C, fold, fold + C, g_op_stream);
    }
    launch_glu_dwconv(d_x, 2 * C, d_w, d_y, C, nb, T, C, k, d_lens, g_op_stream, left, fold, fold ? fold + C : nullptr);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_relpos_table(int32_t S, int32_t M, float* d_out) {
    SC_API_BEGIN
    SC_CHECK(d_out && S > 0 && M > 0 && M % 2 == 0, "sc_op_relpos_table: S=%d M=%d", S, M);
    launch_relpos_table(S, M, d_out, g_op_stream);
    SC_HIP(hipStreamSynchronize(g_op_stream));
    SC_API_END
}

int sc_op_tsm_centres(const float* d_in, int32_t n, int64_t in_stride, const int64_t* h_in_len, const int64_t* h_out_len,
                      const sc_tsm_opts* opts, int32_t* h_centres, int64_t m_stride) {
    SC_API_BEGIN
    run_time_stretch("sc_op_tsm_centres", d_in, n, in_stride, h_in_len, h_out_len, opts, false, nullptr, 0, h_centres, m_stride);
    SC_API_END
}

}  // extern "C"
