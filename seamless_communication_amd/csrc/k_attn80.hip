// Attention at head_dim = 80 (the wav2vec 2.0 / XLS-R encoder: 1280 wide, 16 heads), plain mode with an optional key-length
// mask.  The scheme is attn_mfma16_kernel's (k_attn.hip), restated for the other head size:
//   S^T[key][query] = K . Q^T      A = K tile from LDS (two fp16 planes), B = Q^T held in registers: 80 dims are FIVE 16-wide
//                                  reduction chunks of v_mfma_f32_32x32x16_f16, three terms each (hi.hi + hi.lo + lo.hi);
//   O^T[dim][query] += V^T . P^T   A = V^T from LDS, B = P^T = the S^T accumulator registers.  80 output dims do not fill
//                                  32-row tiles: V^T is held as 96 rows in LDS, rows 80 .. 95 written as zeros ONCE before the
//                                  loop (the staging never touches them), and the third accumulator's upper half is not stored.
// The 16x16x32 form would avoid the 16 idle rows (5 tiles of 16 dims) but needs P^T in another register layout than the one
// the 32x32 S^T accumulator leaves it in, i.e. a trip through LDS per tile; the padded form wastes 1/6 of the second
// product's matrix cycles (18 instead of 15 instructions' worth per 32 keys) and moves nothing.
// Soft-max in the base-2 domain, scale 80^-0.5 applied to the fp32 logits.
#include "kernels.h"

namespace sc {

namespace {

constexpr int HD = 80;
constexpr int HDP = 96;   // V^T rows in LDS (three 32-row tiles)
constexpr int MQ = 128;   // queries per workgroup
constexpr int MKV = 32;   // keys per iteration
constexpr int KH_LD = 88;  // halfs per K-plane row (80 dims + 8 pad; 176 B: 11 sixteen-byte slots, odd)
constexpr int VT_LD = 40;  // halfs per V^T-plane row (32 keys + 8 pad)
constexpr int OS = 84;     // floats per row of the output tile
constexpr int PIECES = HD / 4;  // float4 pieces per key row
typedef _Float16 h8_t __attribute__((ext_vector_type(8)));
typedef _Float16 h4_t __attribute__((ext_vector_type(4)));
typedef float f16v __attribute__((ext_vector_type(16)));
typedef float f4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void split8(const float* x, h8_t& hi, h8_t& lo) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const _Float16 h = (_Float16)x[e];
        hi[e] = h;
        lo[e] = (_Float16)(x[e] - (float)h);
    }
}

constexpr size_t LDS_LOOP = (size_t)(2 * MKV * KH_LD + 2 * HDP * VT_LD) * 2;  // 26 624 B
constexpr size_t LDS_OUT = (size_t)(4 * 32 * OS) * 4;                        // 43 008 B
constexpr size_t LDS_BYTES = LDS_OUT > LDS_LOOP ? LDS_OUT : LDS_LOOP;

__global__ __launch_bounds__(256) void attn80_kernel(AttnArgs p, float scale) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    _Float16* sKh = reinterpret_cast<_Float16*>(smem);  // [32][KH_LD]
    _Float16* sKl = sKh + MKV * KH_LD;
    _Float16* sVh = sKl + MKV * KH_LD;  // [96][VT_LD]
    _Float16* sVl = sVh + HDP * VT_LD;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ql = lane & 31, hh = lane >> 5;
    const int qb = blockIdx.x, h = blockIdx.y, n = blockIdx.z;
    const int q0 = qb * MQ + wave * 32;
    const int qi = q0 + ql;
    const int kv_len = p.kv_lens ? min(p.kv_lens[n], p.Skv) : p.Skv;
    const int64_t qbase = (int64_t)n * p.Sq, kvbase = (int64_t)n * p.Skv;
    const bool qok = qi < p.Sq;
    const float* qrow = p.q + (qbase + (qok ? qi : 0)) * p.ldq + h * HD;

    // Q^T operand: chunk c (dims 16c .. 16c+15), this lane's half holds dims 16c + 8 hh .. + 7
    h8_t qh[5], qlo[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = 0.f;
        if (qok) {
            const f4v v0 = *reinterpret_cast<const f4v*>(qrow + 16 * c + 8 * hh);
            const f4v v1 = *reinterpret_cast<const f4v*>(qrow + 16 * c + 8 * hh + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                x[e] = v0[e];
                x[4 + e] = v1[e];
            }
        }
        split8(x, qh[c], qlo[c]);
    }

    f16v o0, o1, o2;  // O^T: dims 0..31 / 32..63 / 64..95 (rows) x queries (lanes)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        o0[r] = 0.f;
        o1[r] = 0.f;
        o2[r] = 0.f;
    }
    float m_i = -1e30f, l_i = 0.f;

    // the zero rows 80 .. 95 of both V^T planes (16 rows x VT_LD halfs each), never written again
    for (int idx = tid; idx < (HDP - HD) * VT_LD; idx += 256) {
        sVh[HD * VT_LD + idx] = (_Float16)0.f;
        sVl[HD * VT_LD + idx] = (_Float16)0.f;
    }

    // staging role of this thread: float4 pieces idx = tid + 256 u (u < 3) of the [32 keys][20 pieces] tile
    f4v kf[3], vf[3];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int idx = tid + 256 * u;
            const int r = idx / PIECES, c4 = idx - r * PIECES;
            kf[u] = f4v{0.f, 0.f, 0.f, 0.f};
            vf[u] = kf[u];
            if (idx < MKV * PIECES && k0 + r < kv_len) {
                const int64_t row = kvbase + k0 + r;
                kf[u] = *reinterpret_cast<const f4v*>(p.k + row * p.ldk + h * HD + c4 * 4);
                vf[u] = *reinterpret_cast<const f4v*>(p.v + row * p.ldv + h * HD + c4 * 4);
            }
        }
    };
    const int k_end = kv_len;
    if (k_end > 0) fetch(0);

    for (int k0 = 0; k0 < k_end; k0 += MKV) {
        __syncthreads();  // previous tile fully consumed (and, the first time, the zero rows written)
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int idx = tid + 256 * u;
            if (idx < MKV * PIECES) {
                const int r = idx / PIECES, c4 = idx - r * PIECES;
                h4_t khi, klo, vhi, vlo;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const _Float16 a = (_Float16)kf[u][e];
                    khi[e] = a;
                    klo[e] = (_Float16)(kf[u][e] - (float)a);
                    const _Float16 b = (_Float16)vf[u][e];
                    vhi[e] = b;
                    vlo[e] = (_Float16)(vf[u][e] - (float)b);
                }
                *reinterpret_cast<h4_t*>(&sKh[r * KH_LD + 4 * c4]) = khi;
                *reinterpret_cast<h4_t*>(&sKl[r * KH_LD + 4 * c4]) = klo;
                // V^T: position of key r inside its 16-chunk = 8 * half + e with key = (e & 3) + 8 (e >> 2) + 4 half
                const int w = r & 15;
                const int pos = (r & 16) + 8 * ((w >> 2) & 1) + (w & 3) + 4 * (w >> 3);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    sVh[(4 * c4 + e) * VT_LD + pos] = vhi[e];
                    sVl[(4 * c4 + e) * VT_LD + pos] = vlo[e];
                }
            }
        }
        if (k0 + MKV < k_end) fetch(k0 + MKV);  // in flight during this tile's arithmetic
        __syncthreads();

        // ---- S^T = K . Q^T (rows = keys, lanes = queries): three terms per 16-wide chunk, five chunks ----
        f16v st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            const h8_t kh = *reinterpret_cast<const h8_t*>(&sKh[ql * KH_LD + 16 * c + 8 * hh]);
            const h8_t kl = *reinterpret_cast<const h8_t*>(&sKl[ql * KH_LD + 16 * c + 8 * hh]);
            st = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, qh[c], st, 0, 0, 0);
            st = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, qlo[c], st, 0, 0, 0);
            st = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl, qh[c], st, 0, 0, 0);
        }
        // ---- scale, key mask, online soft-max: register r of half hh is key (r&3) + 8*(r>>2) + 4*hh ----
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kj = k0 + (r & 3) + 8 * (r >> 2) + 4 * hh;
            const float sc = st[r] * scale + (kj < kv_len ? 0.f : -INFINITY);
            st[r] = sc;
            mx = fmaxf(mx, sc);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m_i, mx);
        constexpr float LOG2E = 1.44269504088896340736f;
        const float alpha = __builtin_amdgcn_exp2f((m_i - m_new) * LOG2E);
        float rs = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float pv = __builtin_amdgcn_exp2f((st[r] - m_new) * LOG2E);
            st[r] = pv;
            rs += pv;
        }
        rs += __shfl_xor(rs, 32);
        l_i = l_i * alpha + rs;
        m_i = m_new;
        if (__builtin_amdgcn_ballot_w64(alpha != 1.f) != 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                o0[r] *= alpha;
                o1[r] *= alpha;
                o2[r] *= alpha;
            }
        }
        // ---- O^T += V^T . P^T: chunk c contracts the 16 keys that registers 8c .. 8c+7 of the two halves hold ----
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float x[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = st[8 * c + e];
            h8_t ph, pl;
            split8(x, ph, pl);
            const h8_t v0h = *reinterpret_cast<const h8_t*>(&sVh[ql * VT_LD + 16 * c + 8 * hh]);
            const h8_t v0l = *reinterpret_cast<const h8_t*>(&sVl[ql * VT_LD + 16 * c + 8 * hh]);
            const h8_t v1h = *reinterpret_cast<const h8_t*>(&sVh[(32 + ql) * VT_LD + 16 * c + 8 * hh]);
            const h8_t v1l = *reinterpret_cast<const h8_t*>(&sVl[(32 + ql) * VT_LD + 16 * c + 8 * hh]);
            const h8_t v2h = *reinterpret_cast<const h8_t*>(&sVh[(64 + ql) * VT_LD + 16 * c + 8 * hh]);
            const h8_t v2l = *reinterpret_cast<const h8_t*>(&sVl[(64 + ql) * VT_LD + 16 * c + 8 * hh]);
            o0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(v0h, ph, o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(v1h, ph, o1, 0, 0, 0);
            o2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(v2h, ph, o2, 0, 0, 0);
            o0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(v0h, pl, o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(v1h, pl, o1, 0, 0, 0);
            o2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(v2h, pl, o2, 0, 0, 0);
            o0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(v0l, ph, o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(v1l, ph, o1, 0, 0, 0);
            o2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(v2l, ph, o2, 0, 0, 0);
        }
    }

    // ---- O^T (dims x queries) -> this wave's [32 queries][80 dims] tile in LDS -> 16-byte row stores ----
    __syncthreads();  // every wave is done with the K/V tiles
    float* ot = smem + wave * (32 * OS);
    const float inv = l_i > 0.f ? 1.0f / l_i : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int d = (r & 3) + 8 * (r >> 2) + 4 * hh;
        ot[ql * OS + d] = o0[r] * inv;
        ot[ql * OS + 32 + d] = o1[r] * inv;
        if (d < HD - 64) ot[ql * OS + 64 + d] = o2[r] * inv;
    }
    // the wave reads back only what it wrote itself: 32 rows x 20 float4 = 640 pieces, 10 per lane
#pragma unroll
    for (int it = 0; it < 10; ++it) {
        const int idx = it * 64 + lane;
        const int row = idx / PIECES, c0 = (idx - row * PIECES) * 4;
        const int qq = q0 + row;
        if (qq >= p.Sq) continue;
        *reinterpret_cast<f4v*>(p.out + (qbase + qq) * p.ldo + h * HD + c0) = *reinterpret_cast<const f4v*>(&ot[row * OS + c0]);
    }
}

}  // namespace

void launch_attention80(const AttnArgs& a, hipStream_t s) {
    SC_CHECK(a.head_dim == HD, "attention80: head_dim=%d", a.head_dim);
    SC_CHECK(a.nb > 0 && a.heads > 0 && a.Sq > 0 && a.Skv > 0, "attention80: empty problem");
    SC_CHECK(!a.causal && !a.rel_k && !a.rp_table && !a.row_off && !a.out_hi && !a.out_lo,
             "attention80: head_dim 80 takes the plain mode only (no causal mask, relative positions, packed rows or plane output)");
    SC_CHECK(a.q && a.k && a.v && a.out, "attention80: null operand");
    SC_CHECK(a.ldq % 4 == 0 && a.ldk % 4 == 0 && a.ldv % 4 == 0 && a.ldo % 4 == 0 &&
                 ((reinterpret_cast<uintptr_t>(a.q) | reinterpret_cast<uintptr_t>(a.k) | reinterpret_cast<uintptr_t>(a.v) |
                   reinterpret_cast<uintptr_t>(a.out)) & 15) == 0,
             "attention80: row strides must be multiples of 4 and the operands 16-byte aligned");
    SC_CHECK(a.heads <= 65535 && a.nb <= 65535, "attention80: heads=%d nb=%d exceed the grid", a.heads, a.nb);
    const double pairs = a.pairs > 0 ? a.pairs : (double)a.nb * a.Sq * a.Skv;
    prof::Scope scope("attention80", 4.0 * a.heads * pairs * HD, 4.0 * a.nb * a.heads * HD * (2.0 * a.Sq + 2.0 * a.Skv), s);
    dim3 grid(cdiv(a.Sq, MQ), a.heads, a.nb);
    hipLaunchKernelGGL(attn80_kernel, grid, dim3(256), LDS_BYTES, s, a, 1.0f / sqrtf((float)HD));
    SC_LAUNCH_CHECK();
}

}  // namespace sc
