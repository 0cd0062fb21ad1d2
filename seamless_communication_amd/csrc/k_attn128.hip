// Attention at head_dim = 128 (the PRETSSEL acoustic model: 256 wide, 2 heads), key-length mask, padded or packed rows,
// fp32 rows or split fp16 planes out.  The scheme is attn80_kernel's (k_attn80.hip) at the other head size:
//   S^T[key][query] = K . Q^T      A = K tile from LDS (two fp16 planes), B = Q^T held in registers: 128 dims are EIGHT 16-wide
//                                  reduction chunks of v_mfma_f32_32x32x16_f16, three terms each (hi.hi + hi.lo + lo.hi);
//   O^T[dim][query] += V^T . P^T   A = V^T from LDS, B = P^T = the S^T accumulator registers.  128 output dims are FOUR 32-row
//                                  tiles: no padded rows, every matrix cycle is useful.
// Soft-max in the base-2 domain, scale 128^-0.5 applied to the fp32 logits.  Per wave: 64 accumulator registers for O^T, 64
// for the two Q^T planes, 16 for S^T - one workgroup of four waves per SIMD set has room for them.
#include "kernels.h"

namespace sc {

namespace {

constexpr int HD = 128;
constexpr int MQ = 128;    // queries per workgroup
constexpr int MKV = 32;    // keys per iteration
constexpr int KH_LD = 136;  // halfs per K-plane row (128 dims + 8 pad; 272 B: 17 sixteen-byte slots, odd)
constexpr int VT_LD = 40;   // halfs per V^T-plane row (32 keys + 8 pad)
constexpr int OS = 132;     // floats per row of the output tile
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

constexpr size_t LDS_LOOP = (size_t)(2 * MKV * KH_LD + 2 * HD * VT_LD) * 2;  // 37 888 B
constexpr size_t LDS_OUT = (size_t)(4 * 32 * OS) * 4;                       // 67 584 B
constexpr size_t LDS_BYTES = LDS_OUT > LDS_LOOP ? LDS_OUT : LDS_LOOP;

__global__ __launch_bounds__(256) void attn128_kernel(AttnArgs p, float scale) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    _Float16* sKh = reinterpret_cast<_Float16*>(smem);  // [32][KH_LD]
    _Float16* sKl = sKh + MKV * KH_LD;
    _Float16* sVh = sKl + MKV * KH_LD;  // [128][VT_LD]
    _Float16* sVl = sVh + HD * VT_LD;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ql = lane & 31, hh = lane >> 5;
    const int qb = blockIdx.x, h = blockIdx.y, n = blockIdx.z;
    const int q0 = qb * MQ + wave * 32;
    const int qi = q0 + ql;
    const int kv_len = p.kv_lens ? min(p.kv_lens[n], p.Skv) : p.Skv;
    // packed items: rows row_off[n] .. + kv_len, queries beyond the item's own length do not exist
    const int sq_n = p.row_off ? kv_len : p.Sq;
    const int64_t qbase = p.row_off ? (int64_t)p.row_off[n] : (int64_t)n * p.Sq;
    const int64_t kvbase = p.row_off ? (int64_t)p.row_off[n] : (int64_t)n * p.Skv;
    if (qb * MQ >= sq_n) return;  // the whole workgroup lies behind the item's end
    const bool qok = qi < sq_n;
    const float* qrow = p.q + (qbase + (qok ? qi : 0)) * p.ldq + h * HD;

    // Q^T operand: chunk c (dims 16c .. 16c+15), this lane's half holds dims 16c + 8 hh .. + 7
    h8_t qh[8], qlo[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
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

    f16v o[4];  // O^T: dims 32 j .. 32 j + 31 (rows) x queries (lanes)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[j][r] = 0.f;
    float m_i = -1e30f, l_i = 0.f;

    // staging role of this thread: float4 pieces idx = tid + 256 u (u < 4) of the [32 keys][32 pieces] tile
    f4v kf[4], vf[4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = tid + 256 * u;
            const int r = idx / PIECES, c4 = idx - r * PIECES;
            kf[u] = f4v{0.f, 0.f, 0.f, 0.f};
            vf[u] = kf[u];
            if (k0 + r < kv_len) {
                const int64_t row = kvbase + k0 + r;
                kf[u] = *reinterpret_cast<const f4v*>(p.k + row * p.ldk + h * HD + c4 * 4);
                vf[u] = *reinterpret_cast<const f4v*>(p.v + row * p.ldv + h * HD + c4 * 4);
            }
        }
    };
    const int k_end = kv_len;
    if (k_end > 0) fetch(0);

    for (int k0 = 0; k0 < k_end; k0 += MKV) {
        __syncthreads();  // previous tile fully consumed
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = tid + 256 * u;
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
        if (k0 + MKV < k_end) fetch(k0 + MKV);  // in flight during this tile's arithmetic
        __syncthreads();

        // ---- S^T = K . Q^T (rows = keys, lanes = queries): three terms per 16-wide chunk, eight chunks ----
        f16v st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
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
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[j][r] *= alpha;
        }
        // ---- O^T += V^T . P^T: chunk c contracts the 16 keys that registers 8c .. 8c+7 of the two halves hold ----
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float x[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = st[8 * c + e];
            h8_t ph, pl;
            split8(x, ph, pl);
            h8_t vh[4], vl[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                vh[j] = *reinterpret_cast<const h8_t*>(&sVh[(32 * j + ql) * VT_LD + 16 * c + 8 * hh]);
                vl[j] = *reinterpret_cast<const h8_t*>(&sVl[(32 * j + ql) * VT_LD + 16 * c + 8 * hh]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh[j], ph, o[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh[j], pl, o[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl[j], ph, o[j], 0, 0, 0);
        }
    }

    // ---- O^T (dims x queries) -> this wave's [32 queries][128 dims] tile in LDS -> 16-byte row stores ----
    __syncthreads();  // every wave is done with the K/V tiles
    float* ot = smem + wave * (32 * OS);
    const float inv = l_i > 0.f ? 1.0f / l_i : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int d = (r & 3) + 8 * (r >> 2) + 4 * hh;
            ot[ql * OS + 32 * j + d] = o[j][r] * inv;
        }
    // the wave reads back only what it wrote itself: 32 rows x 32 float4 = 1024 pieces, 16 per lane
#pragma unroll
    for (int it = 0; it < 16; ++it) {
        const int idx = it * 64 + lane;
        const int row = idx / PIECES, c0 = (idx - row * PIECES) * 4;
        const int qq = q0 + row;
        if (qq >= sq_n) continue;
        const f4v of = *reinterpret_cast<const f4v*>(&ot[row * OS + c0]);
        if (p.out_hi) {
            const h4_t hi = __builtin_convertvector(of, h4_t);
            const f4v back = __builtin_convertvector(hi, f4v);
            const int64_t off = (qbase + qq) * p.ldoh + h * HD + c0;
            *reinterpret_cast<h4_t*>(reinterpret_cast<_Float16*>(p.out_hi) + off) = hi;
            *reinterpret_cast<h4_t*>(reinterpret_cast<_Float16*>(p.out_lo) + off) = __builtin_convertvector(of - back, h4_t);
        } else {
            *reinterpret_cast<f4v*>(p.out + (qbase + qq) * p.ldo + h * HD + c0) = of;
        }
    }
}

bool g_attn128_attr_set = false;

}  // namespace

void launch_attention128(const AttnArgs& a, hipStream_t s) {
    SC_CHECK(a.head_dim == HD, "attention128: head_dim=%d", a.head_dim);
    SC_CHECK(a.nb > 0 && a.heads > 0 && a.Sq > 0 && a.Skv > 0, "attention128: empty problem");
    SC_CHECK(!a.causal && !a.rel_k && !a.rp_table,
             "attention128: head_dim 128 takes the key-length mask only (no causal mask, no Shaw or Transformer-XL relative positions)");
    SC_CHECK(a.q && a.k && a.v && (a.out || (a.out_hi && a.out_lo)), "attention128: null operand");
    SC_CHECK(!a.row_off || (a.kv_lens && a.Sq == a.Skv), "attention128: packed rows need kv_lens and Sq == Skv");
    SC_CHECK(a.ldq % 4 == 0 && a.ldk % 4 == 0 && a.ldv % 4 == 0 &&
                 ((reinterpret_cast<uintptr_t>(a.q) | reinterpret_cast<uintptr_t>(a.k) | reinterpret_cast<uintptr_t>(a.v)) & 15) == 0,
             "attention128: row strides must be multiples of 4 and the operands 16-byte aligned");
    if (a.out_hi)
        SC_CHECK(a.ldoh % 4 == 0 && ((reinterpret_cast<uintptr_t>(a.out_hi) | reinterpret_cast<uintptr_t>(a.out_lo)) & 7) == 0,
                 "attention128: the output planes need a row stride that is a multiple of 4 and 8-byte alignment");
    else
        SC_CHECK(a.ldo % 4 == 0 && (reinterpret_cast<uintptr_t>(a.out) & 15) == 0, "attention128: the output needs a row stride that is a multiple of 4 and 16-byte alignment");
    SC_CHECK(a.heads <= 65535 && a.nb <= 65535, "attention128: heads=%d nb=%d exceed the grid", a.heads, a.nb);
    if (!g_attn128_attr_set) {
        SC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&attn128_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES));
        g_attn128_attr_set = true;
    }
    const double pairs = a.pairs > 0 ? a.pairs : (double)a.nb * a.Sq * a.Skv;
    prof::Scope scope("attention128", 4.0 * a.heads * pairs * HD, 4.0 * a.nb * a.heads * HD * (2.0 * a.Sq + 2.0 * a.Skv), s);
    dim3 grid(cdiv(a.Sq, MQ), a.heads, a.nb);
    hipLaunchKernelGGL(attn128_kernel, grid, dim3(256), LDS_BYTES, s, a, 1.0f / sqrtf((float)HD));
    SC_LAUNCH_CHECK();
}

}  // namespace sc
