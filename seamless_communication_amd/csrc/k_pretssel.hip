// Kernels of the PRETSSEL acoustic model (model_pretssel.hip; reference models/generator/vocoder.py:488-513,
// models/unity/film.py, models/unity/length_regulator.py): every FiLM projection of a call in one launch, LayerNorm -> FiLM ->
// mask in one pass, the variance adaptor's tail, the fused Gaussian upsampling, and the post-net's row passes.
// All of them are row kernels: one wave per row (or per output value), lanes over the channels, fp32 arithmetic.
#include "device_util.h"

namespace sc {

namespace {


__device__ __forceinline__ void store_planes(__half* yh, __half* yl, int64_t off, float v) {
    const _Float16 h = (_Float16)v;  // the split, inline: split1 binds both planes first, which moves a store in film_ln_kernel
    reinterpret_cast<_Float16*>(yh)[off] = h;
    reinterpret_cast<_Float16*>(yl)[off] = (_Float16)(v - (float)h);
}

// ---- FiLM projections: out[i][j] = mul[j] * (W[j] . cond_i + bias[j]) + add[j], cond_i = [prosody_i | lang] ----
__global__ __launch_bounds__(256) void film_proj_kernel(const float* __restrict__ pros, int P, const float* __restrict__ lang, int Lg,
                                                        const __half* __restrict__ W, const float* __restrict__ bias, const float* __restrict__ mul,
                                                        const float* __restrict__ add, int N, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int i = blockIdx.y;
    if (j >= N) return;
    const int D = P + Lg;
    const _Float16* w = reinterpret_cast<const _Float16*>(W) + (int64_t)j * D;
    float acc = 0.f;
    for (int k = lane; k < D; k += 64) {
        const float c = k < P ? pros[(int64_t)i * P + k] : lang[k - P];
        acc = fmaf((float)w[k], c, acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) out[(int64_t)i * N + j] = mul[j] * (acc + bias[j]) + add[j];
}

// ---- LayerNorm -> FiLM -> mask -> fp32 rows and / or planes; one wave per (row, group) ----
template <int VPL>  // values per lane: C = 64 * VPL
__global__ __launch_bounds__(256) void film_ln_kernel(PretsselLnArgs p) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= (int64_t)p.rows * p.groups) return;
    const int row = (int)(wid / p.groups), grp = (int)(wid - (int64_t)row * p.groups);
    const int C = 64 * VPL;
    const int item = p.row_item ? p.row_item[row] : 0;
    const int64_t col0 = (int64_t)grp * C;
    float v[VPL];
    if (item < 0) {  // a row behind its item's length: exact zeros
#pragma unroll
        for (int e = 0; e < VPL; ++e) v[e] = 0.f;
    } else {
        const float* x = p.x + (int64_t)row * p.ldx + col0;
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < VPL; ++e) {
            v[e] = x[lane + 64 * e];
            s += v[e];
        }
        const float mean = wave_sum(s) / (float)C;
        float q = 0.f;
#pragma unroll
        for (int e = 0; e < VPL; ++e) {
            v[e] -= mean;
            q += v[e] * v[e];
        }
        const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + 1e-5f);
        const float* fg = p.film ? p.film + (int64_t)item * p.film_ld + p.film_off + (int64_t)grp * 2 * C : nullptr;
#pragma unroll
        for (int e = 0; e < VPL; ++e) {
            const int c = lane + 64 * e;
            float y = v[e] * rstd * p.g[col0 + c] + p.b[col0 + c];
            if (fg) y = fg[c] * y + fg[C + c];
            v[e] = y;
        }
    }
#pragma unroll
    for (int e = 0; e < VPL; ++e) {
        const int c = lane + 64 * e;
        if (p.y) p.y[(int64_t)row * p.ldy + col0 + c] = v[e];
        if (p.yh) store_planes(p.yh, p.yl, (int64_t)row * p.ldh + col0 + c, v[e]);
    }
}

// ---- variance tail: three dot products, the voiced gate, x += embed_pitch(pitch) + embed_energy(energy) ----
__global__ __launch_bounds__(256) void var_tail_kernel(PretsselTailArgs p) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.rows) return;
    const float* f = p.f + (int64_t)row * 3 * p.H;
    float d[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        float acc = 0.f;
        for (int c = lane; c < p.H; c += 64) acc = fmaf(f[j * p.H + c], p.pw[j * p.H + c], acc);
        d[j] = wave_sum(acc) + p.pb[j];
    }
    // order of the predictors: pitch, voiced / unvoiced, energy.  sigmoid(v) >= 0.5 <=> v >= 0
    const float pitch = d[1] >= 0.f ? d[0] : 0.f;
    const float energy = d[2];
    if (p.vals && lane == 0) {
        p.vals[(int64_t)row * 3] = d[0];
        p.vals[(int64_t)row * 3 + 1] = d[1];
        p.vals[(int64_t)row * 3 + 2] = d[2];
    }
    float* x = p.x + (int64_t)row * p.C;
    for (int c = lane; c < p.C; c += 64) x[c] = (x[c] + (pitch * p.wp[c] + p.bp[c])) + (energy * p.we[c] + p.be[c]);
}

// ---- Gaussian upsampling ----
// centres c_k = cumsum(d)_k - d_k / 2 of every item's tokens; one wave per item, 64 tokens per step with a carried total.
// Durations are small integers: the sums are exact in fp32 below 2^23.
__global__ __launch_bounds__(64) void ups_centres_kernel(const int* __restrict__ dur, const int* __restrict__ tok_off, float* __restrict__ centre) {
    const int lane = threadIdx.x, i = blockIdx.x;
    const int t0 = tok_off[i], L = tok_off[i + 1] - t0;
    int carry = 0;
    for (int k0 = 0; k0 < L; k0 += 64) {
        const int k = k0 + lane;
        const int d = k < L ? dur[t0 + k] : 0;
        int s = d;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(s, o);
            if (lane >= o) s += u;
        }
        if (k < L) centre[t0 + k] = (float)(carry + s) - 0.5f * (float)d;
        carry += __shfl(s, 63);
    }
}

// One wave per frame.  energy_k = -delta (t - c_k)^2; the centres are non-decreasing, so the energies rise up to the centre
// nearest to t and fall behind it: the row maximum is the nearest centre's energy (binary search), and the tokens within
// UPS_CUT of the maximum are one contiguous run around it.  Tokens below the cut-off are dropped: each has a weight under
// exp(-UPS_CUT) = 8.8e-27 of the largest, so with at most 2^24 tokens the dropped share of a row's soft-max mass is below
// 2^24 * 8.8e-27 < 1.5e-19 - twelve orders under fp32 resolution.  Frames far from every centre (inside a long token) are
// normalised like any other: the window is relative to the row maximum, not to the position.
constexpr float UPS_CUT = 60.0f;

__global__ __launch_bounds__(256) void ups_frames_kernel(PretsselUpsArgs p) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= p.frames) return;
    const int i = item_search(p.n, m, [&](int j) { return p.frame_off[j]; });
    const int t = m - p.frame_off[i];
    const int t0 = p.tok_off[i], L = p.tok_off[i + 1] - t0;
    const float* c = p.centre + t0;
    const float tf = (float)t;
    // nearest centre: first centre >= t, or its left neighbour
    int lo = 0, hi = L;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (c[mid] < tf) lo = mid + 1;
        else hi = mid;
    }
    int kb = lo < L ? lo : L - 1;
    if (lo > 0 && lo < L && tf - c[lo - 1] < c[lo] - tf) kb = lo - 1;
    const float db = tf - c[kb];
    const float emax = -p.delta * (db * db);
    float acc[PRETSSEL_UPS_VPL];
#pragma unroll
    for (int e = 0; e < PRETSSEL_UPS_VPL; ++e) acc[e] = 0.f;
    float wsum = 0.f;
    auto take = [&](int k) -> bool {
        const float dd = tf - c[k];
        const float rel = -p.delta * (dd * dd) - emax;
        if (rel < -UPS_CUT) return false;
        const float w = expf(rel);
        wsum += w;
        const float* x = p.x + (int64_t)(t0 + k) * p.C;
#pragma unroll
        for (int e = 0; e < PRETSSEL_UPS_VPL; ++e) {
            const int ch = lane + 64 * e;
            if (ch < p.C) acc[e] = fmaf(w, x[ch], acc[e]);
        }
        return true;
    };
    for (int k = kb; k >= 0 && take(k); --k) {
    }
    for (int k = kb + 1; k < L && take(k); ++k) {
    }
    const float inv = 1.0f / wsum;
    const float* pos = p.pos_table ? p.pos_table + (int64_t)t * p.C : nullptr;
#pragma unroll
    for (int e = 0; e < PRETSSEL_UPS_VPL; ++e) {
        const int ch = lane + 64 * e;
        if (ch >= p.C) continue;
        const float y = acc[e] * inv + (pos ? p.pos_alpha * pos[ch] : 0.f);
        if (p.y) p.y[(int64_t)m * p.C + ch] = y;
        if (p.yh) store_planes(p.yh, p.yl, (int64_t)m * p.C + ch, y);
    }
    if (p.wsum && lane == 0) p.wsum[m] = wsum;
}

// ---- front end: x[m] = embed[tok[m]] + alpha * pos[row_t[m]] -> fp32 rows and planes ----
__global__ __launch_bounds__(256) void embed_pos_kernel(const int* __restrict__ tok, const int* __restrict__ row_t, const __half* __restrict__ embed,
                                                        const float* __restrict__ pos_table, float alpha, int rows, int C, float* __restrict__ y,
                                                        __half* __restrict__ yh, __half* __restrict__ yl) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)rows * C) return;
    const int m = (int)(idx / C), c = (int)(idx - (int64_t)m * C);
    const float v = (float)reinterpret_cast<const _Float16*>(embed)[(int64_t)tok[m] * C + c] + alpha * pos_table[(int64_t)row_t[m] * C + c];
    y[idx] = v;
    store_planes(yh, yl, idx, v);
}

// ---- post-net row passes over the extended rows (every item's frames followed by its halo rows) ----
// input planes [ext_rows][CP]: frame rows hold the projection, halo rows the projection's bias, columns C .. CP-1 zeros
__global__ __launch_bounds__(256) void postnet_in_kernel(const float* __restrict__ proj, const float* __restrict__ bias, const int* __restrict__ ext_item,
                                                         const int2* __restrict__ ext_pos, const int* __restrict__ frame_off, int ext_rows, int C, int CP,
                                                         __half* __restrict__ yh, __half* __restrict__ yl) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)ext_rows * CP) return;
    const int m = (int)(idx / CP), c = (int)(idx - (int64_t)m * CP);
    const int i = ext_item[m], t = ext_pos[m].x;
    const int len = frame_off[i + 1] - frame_off[i];
    float v = 0.f;
    if (c < C) v = t < len ? proj[(int64_t)(frame_off[i] + t) * C + c] : bias[c];
    store_planes(yh, yl, idx, v);
}

// BatchNorm (folded) + Tanh on the convolution's rows -> planes of the next convolution
__global__ __launch_bounds__(256) void postnet_bn_tanh_kernel(const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
                                                              int64_t n, int C, __half* __restrict__ yh, __half* __restrict__ yl) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int c = (int)(idx % C);
    store_planes(yh, yl, idx, tanhf(x[idx] * scale[c] + shift[c]));
}

// last layer: mel[i][t] = (proj + BatchNorm(conv)) * std + mean on the frame rows; halo rows are dropped
__global__ __launch_bounds__(256) void postnet_out_kernel(const float* __restrict__ x, const float* __restrict__ scale, const float* __restrict__ shift,
                                                          const float* __restrict__ proj, const float* __restrict__ gstd, const float* __restrict__ gmean,
                                                          const int* __restrict__ ext_item, const int2* __restrict__ ext_pos,
                                                          const int* __restrict__ frame_off, int ext_rows, int C, int t_cap, float* __restrict__ mel) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)ext_rows * C) return;
    const int m = (int)(idx / C), c = (int)(idx - (int64_t)m * C);
    const int i = ext_item[m], t = ext_pos[m].x;
    if (t >= frame_off[i + 1] - frame_off[i]) return;
    const float pn = x[idx] * scale[c] + shift[c];
    const float v = proj[(int64_t)(frame_off[i] + t) * C + c] + pn;
    mel[((int64_t)i * t_cap + t) * C + c] = v * gstd[c] + gmean[c];
}

}  // namespace

void launch_pretssel_film(const float* pros, int P, const float* lang, int Lg, const __half* W, const float* bias, const float* mul, const float* add,
                          int n, int N, float* out, hipStream_t s) {
    SC_CHECK(pros && (lang || Lg == 0) && W && bias && mul && add && out && n > 0 && N > 0 && P >= 0 && Lg >= 0 && P + Lg > 0, "pretssel film: bad argument");
    SC_CHECK(n <= 65535, "pretssel film: %d items exceed the grid", n);
    hipLaunchKernelGGL(film_proj_kernel, dim3(cdiv(N, 4), n), dim3(256), 0, s, pros, P, lang, Lg, W, bias, mul, add, N, out);
    SC_LAUNCH_CHECK();
}

bool pretssel_ln_supported(int C) { return C >= 64 && C % 64 == 0 && C <= 1024; }

void launch_pretssel_film_ln(const PretsselLnArgs& a, hipStream_t s) {
    SC_CHECK(a.x && a.g && a.b && (a.y || (a.yh && a.yl)) && a.rows > 0 && a.groups >= 1, "pretssel film_ln: bad argument");
    SC_CHECK(pretssel_ln_supported(a.C), "pretssel film_ln: C=%d must be a multiple of 64 up to 1024", a.C);
    SC_CHECK(!a.yh || a.yl, "pretssel film_ln: a hi plane needs its lo plane");
    const int64_t waves = (int64_t)a.rows * a.groups;
    SC_CHECK(waves < (1ll << 31), "pretssel film_ln: too many rows");
    const dim3 grid((unsigned)cdiv64(waves, 4));
#define SC_FILM_LN(V)                                                              \
    case V:                                                                        \
        hipLaunchKernelGGL((film_ln_kernel<V>), grid, dim3(256), 0, s, a);         \
        break;
    switch (a.C / 64) {
        SC_FILM_LN(1) SC_FILM_LN(2) SC_FILM_LN(3) SC_FILM_LN(4) SC_FILM_LN(5) SC_FILM_LN(6) SC_FILM_LN(7) SC_FILM_LN(8)
        SC_FILM_LN(9) SC_FILM_LN(10) SC_FILM_LN(11) SC_FILM_LN(12) SC_FILM_LN(13) SC_FILM_LN(14) SC_FILM_LN(15) SC_FILM_LN(16)
    }
#undef SC_FILM_LN
    SC_LAUNCH_CHECK();
}

void launch_pretssel_var_tail(const PretsselTailArgs& a, hipStream_t s) {
    SC_CHECK(a.f && a.pw && a.pb && a.wp && a.bp && a.we && a.be && a.x && a.rows > 0 && a.H > 0 && a.C > 0, "pretssel var_tail: bad argument");
    hipLaunchKernelGGL(var_tail_kernel, dim3(cdiv(a.rows, 4)), dim3(256), 0, s, a);
    SC_LAUNCH_CHECK();
}

float pretssel_ups_cutoff() { return UPS_CUT; }

void launch_pretssel_upsample(const PretsselUpsArgs& a, hipStream_t s) {
    SC_CHECK(a.x && a.dur && a.tok_off && a.frame_off && a.centre && (a.y || (a.yh && a.yl)) && a.n > 0 && a.frames > 0,
             "pretssel upsample: bad argument");
    SC_CHECK(a.C > 0 && a.C <= 64 * PRETSSEL_UPS_VPL, "pretssel upsample: C=%d above %d", a.C, 64 * PRETSSEL_UPS_VPL);
    SC_CHECK(a.n <= 65535, "pretssel upsample: %d items exceed the grid", a.n);
    hipLaunchKernelGGL(ups_centres_kernel, dim3(a.n), dim3(64), 0, s, a.dur, a.tok_off, a.centre);
    hipLaunchKernelGGL(ups_frames_kernel, dim3(cdiv(a.frames, 4)), dim3(256), 0, s, a);
    SC_LAUNCH_CHECK();
}

void launch_pretssel_embed_pos(const int* tok, const int* row_t, const __half* embed, const float* pos_table, float alpha, int rows, int C, float* y,
                               __half* yh, __half* yl, hipStream_t s) {
    SC_CHECK(tok && row_t && embed && pos_table && y && yh && yl && rows > 0 && C > 0, "pretssel embed: bad argument");
    hipLaunchKernelGGL(embed_pos_kernel, dim3((unsigned)cdiv64((int64_t)rows * C, 256)), dim3(256), 0, s, tok, row_t, embed, pos_table, alpha, rows, C,
                       y, yh, yl);
    SC_LAUNCH_CHECK();
}

void launch_pretssel_postnet_in(const float* proj, const float* bias, const int* ext_item, const int2* ext_pos, const int* frame_off, int ext_rows, int C,
                                int CP, __half* yh, __half* yl, hipStream_t s) {
    SC_CHECK(proj && bias && ext_item && ext_pos && frame_off && yh && yl && ext_rows > 0 && C > 0 && CP >= C, "pretssel postnet_in: bad argument");
    hipLaunchKernelGGL(postnet_in_kernel, dim3((unsigned)cdiv64((int64_t)ext_rows * CP, 256)), dim3(256), 0, s, proj, bias, ext_item, ext_pos, frame_off,
                       ext_rows, C, CP, yh, yl);
    SC_LAUNCH_CHECK();
}

void launch_pretssel_postnet_bn_tanh(const float* x, const float* scale, const float* shift, int rows, int C, __half* yh, __half* yl, hipStream_t s) {
    SC_CHECK(x && scale && shift && yh && yl && rows > 0 && C > 0, "pretssel postnet_bn_tanh: bad argument");
    const int64_t n = (int64_t)rows * C;
    hipLaunchKernelGGL(postnet_bn_tanh_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, s, x, scale, shift, n, C, yh, yl);
    SC_LAUNCH_CHECK();
}

void launch_pretssel_postnet_out(const float* x, const float* scale, const float* shift, const float* proj, const float* gstd, const float* gmean,
                                 const int* ext_item, const int2* ext_pos, const int* frame_off, int ext_rows, int C, int t_cap, float* mel, hipStream_t s) {
    SC_CHECK(x && scale && shift && proj && gstd && gmean && ext_item && ext_pos && frame_off && mel && ext_rows > 0 && C > 0 && t_cap > 0,
             "pretssel postnet_out: bad argument");
    hipLaunchKernelGGL(postnet_out_kernel, dim3((unsigned)cdiv64((int64_t)ext_rows * C, 256)), dim3(256), 0, s, x, scale, shift, proj, gstd, gmean,
                       ext_item, ext_pos, frame_off, ext_rows, C, t_cap, mel);
    SC_LAUNCH_CHECK();
}

}  // namespace sc
