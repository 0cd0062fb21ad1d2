// Attention at head_dim HD = 80 (the wav2vec 2.0 / XLS-R encoder: 1280 wide, 16 heads; plain mode with an optional key-length
// mask) and HD = 128 (the PRETSSEL acoustic model: 256 wide, 2 heads; key-length mask, padded or packed rows, fp32 rows or split
// fp16 planes out): one kernel template, two instantiations.  Head dim 64 (k_attn.hip) is not folded in: it has the
// relative-position modes, the XCD remapping of workgroup ids and a different staging map.  The scheme is its kernel's:
//   S^T[key][query] = K . Q^T      A = K tile from LDS (two fp16 planes), B = Q^T held in registers: HD dims are NC = HD / 16
//                                  16-wide reduction chunks of v_mfma_f32_32x32x16_f16, three terms each (hi.hi + hi.lo + lo.hi);
//   O^T[dim][query] += V^T . P^T   A = V^T from LDS, B = P^T = the S^T accumulator registers, NJ = HDP / 32 output tiles of 32
//                                  rows with HDP = HD rounded up to 32.  128 dims are four full tiles: every matrix cycle is
//                                  useful.  80 dims do not fill three: V^T is held as 96 rows in LDS, rows 80 .. 95 written as
//                                  zeros ONCE before the loop (the staging never touches them), and the last accumulator's
//                                  upper half is not stored.
// The 16x16x32 form would avoid the 16 idle rows at HD = 80 (5 tiles of 16 dims) but needs P^T in another register layout than
// the one the 32x32 S^T accumulator leaves it in, i.e. a trip through LDS per tile; the padded form wastes 1/6 of the second
// product's matrix cycles (18 instead of 15 instructions' worth per 32 keys) and moves nothing.
// LDS rows: a K-plane row is HD + 8 halfs (176 B / 272 B: 11 / 17 sixteen-byte slots, odd, so the 16 lanes of a ds_read_b128
// group hit 16 distinct slots), a V^T-plane row 32 keys + 8 halfs (80 B: 5 slots).
// Registers per wave: 16 NJ accumulators for O^T, 8 NC for the two Q^T planes, 16 for S^T.  At HD = 80 (48 + 40 + 16) two
// workgroups of four waves share a SIMD set, at HD = 128 (64 + 64 + 16) one has room.
// Soft-max in the base-2 domain, scale HD^-0.5 applied to the fp32 logits.
#include "device_util.h"

namespace sc {

namespace {

constexpr int MQ = 128;   // queries per workgroup
constexpr int MKV = 32;   // keys per iteration
constexpr int VT_LD = 40;  // halfs per V^T-plane row (32 keys + 8 pad)

template <int HD>
struct AttnHd {
    static constexpr int HDP = (HD + 31) / 32 * 32;  // V^T rows in LDS
    static constexpr int NJ = HDP / 32;              // 32-row output tiles
    static constexpr int NC = HD / 16;               // 16-wide reduction chunks of S^T
    static constexpr int KH_LD = HD + 8;             // halfs per K-plane row
    static constexpr int OS = HD + 4;                // floats per row of the output tile
    static constexpr int PIECES = HD / 4;            // float4 pieces per key row
    static constexpr int NU = (MKV * PIECES + 255) / 256;  // staging pieces per thread
    static constexpr size_t LDS_LOOP = (size_t)(2 * MKV * KH_LD + 2 * HDP * VT_LD) * 2;  // 26 624 B / 37 888 B
    static constexpr size_t LDS_OUT = (size_t)(4 * 32 * OS) * 4;                         // 43 008 B / 67 584 B
    static constexpr size_t LDS_BYTES = LDS_OUT > LDS_LOOP ? LDS_OUT : LDS_LOOP;
    static_assert(HD % 16 == 0 && (32 * PIECES) % 64 == 0, "attn_hd_kernel: whole chunks, whole read-back rounds");
};

template <int HD>
__global__ __launch_bounds__(256) void attn_hd_kernel(AttnArgs p, float scale) {
    using C = AttnHd<HD>;
    constexpr int HDP = C::HDP, NJ = C::NJ, NC = C::NC, KH_LD = C::KH_LD, OS = C::OS, PIECES = C::PIECES, NU = C::NU;
    constexpr bool PAD = HDP > HD;                    // zero rows HD .. HDP-1 of V^T
    constexpr bool RAGGED = MKV * PIECES < 256 * NU;  // the last staging piece of some threads lies behind the tile
    extern __shared__ __attribute__((aligned(16))) float smem[];
    _Float16* sKh = reinterpret_cast<_Float16*>(smem);  // [32][KH_LD]
    _Float16* sKl = sKh + MKV * KH_LD;
    _Float16* sVh = sKl + MKV * KH_LD;  // [HDP][VT_LD]
    _Float16* sVl = sVh + HDP * VT_LD;

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
    half8_t qh[NC], qlo[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = 0.f;
        if (qok) {
            const f32x4_t v0 = *reinterpret_cast<const f32x4_t*>(qrow + 16 * c + 8 * hh);
            const f32x4_t v1 = *reinterpret_cast<const f32x4_t*>(qrow + 16 * c + 8 * hh + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                x[e] = v0[e];
                x[4 + e] = v1[e];
            }
        }
        split8(x, qh[c], qlo[c]);
    }

    float16_t o[NJ];  // O^T: dims 32 j .. 32 j + 31 (rows) x queries (lanes)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[j][r] = 0.f;
    float m_i = -1e30f, l_i = 0.f;

    if (PAD) {  // the zero rows HD .. HDP-1 of both V^T planes, never written again
        for (int idx = tid; idx < (HDP - HD) * VT_LD; idx += 256) {
            sVh[HD * VT_LD + idx] = (_Float16)0.f;
            sVl[HD * VT_LD + idx] = (_Float16)0.f;
        }
    }

    // staging role of this thread: float4 pieces idx = tid + 256 u (u < NU) of the [32 keys][PIECES] tile
    f32x4_t kf[NU], vf[NU];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int idx = tid + 256 * u;
            const int r = idx / PIECES, c4 = idx - r * PIECES;
            kf[u] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            vf[u] = kf[u];
            if ((!RAGGED || idx < MKV * PIECES) && k0 + r < kv_len) {
                const int64_t row = kvbase + k0 + r;
                kf[u] = *reinterpret_cast<const f32x4_t*>(p.k + row * p.ldk + h * HD + c4 * 4);
                vf[u] = *reinterpret_cast<const f32x4_t*>(p.v + row * p.ldv + h * HD + c4 * 4);
            }
        }
    };
    const int k_end = kv_len;
    if (k_end > 0) fetch(0);

    for (int k0 = 0; k0 < k_end; k0 += MKV) {
        __syncthreads();  // previous tile fully consumed (and, the first time, the zero rows written)
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int idx = tid + 256 * u;
            if (!RAGGED || idx < MKV * PIECES) {
                const int r = idx / PIECES, c4 = idx - r * PIECES;
                half4_t khi, klo, vhi, vlo;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    // the split, inline: split1 through temporaries changes the HD = 128 instruction stream (measured 0.5 % slower)
                    const _Float16 a = (_Float16)kf[u][e];
                    khi[e] = a;
                    klo[e] = (_Float16)(kf[u][e] - (float)a);
                    const _Float16 b = (_Float16)vf[u][e];
                    vhi[e] = b;
                    vlo[e] = (_Float16)(vf[u][e] - (float)b);
                }
                *reinterpret_cast<half4_t*>(&sKh[r * KH_LD + 4 * c4]) = khi;
                *reinterpret_cast<half4_t*>(&sKl[r * KH_LD + 4 * c4]) = klo;
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

        // ---- S^T = K . Q^T (rows = keys, lanes = queries): three terms per 16-wide chunk, chunks ascending ----
        float16_t st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const half8_t kh = *reinterpret_cast<const half8_t*>(&sKh[ql * KH_LD + 16 * c + 8 * hh]);
            const half8_t kl = *reinterpret_cast<const half8_t*>(&sKl[ql * KH_LD + 16 * c + 8 * hh]);
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
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[j][r] *= alpha;
        }
        // ---- O^T += V^T . P^T: chunk c contracts the 16 keys that registers 8c .. 8c+7 of the two halves hold; per chunk
        //      every tile's V_hi . P_hi, then every tile's V_hi . P_lo, then every tile's V_lo . P_hi ----
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            float x[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = st[8 * c + e];
            half8_t ph, pl;
            split8(x, ph, pl);
            half8_t vh[NJ], vl[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                vh[j] = *reinterpret_cast<const half8_t*>(&sVh[(32 * j + ql) * VT_LD + 16 * c + 8 * hh]);
                vl[j] = *reinterpret_cast<const half8_t*>(&sVl[(32 * j + ql) * VT_LD + 16 * c + 8 * hh]);
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) o[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh[j], ph, o[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NJ; ++j) o[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh[j], pl, o[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NJ; ++j) o[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl[j], ph, o[j], 0, 0, 0);
        }
    }

    // ---- O^T (dims x queries) -> this wave's [32 queries][HD dims] tile in LDS -> 16-byte row stores ----
    __syncthreads();  // every wave is done with the K/V tiles
    float* ot = smem + wave * (32 * OS);
    const float inv = l_i > 0.f ? 1.0f / l_i : 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int d = (r & 3) + 8 * (r >> 2) + 4 * hh;
            if (!PAD || 32 * j + d < HD) ot[ql * OS + 32 * j + d] = o[j][r] * inv;
        }
    // the wave reads back only what it wrote itself: 32 rows x PIECES float4, PIECES / 2 per lane
#pragma unroll
    for (int it = 0; it < 32 * PIECES / 64; ++it) {
        const int idx = it * 64 + lane;
        const int row = idx / PIECES, c0 = (idx - row * PIECES) * 4;
        const int qq = q0 + row;
        if (qq >= sq_n) continue;
        const f32x4_t of = *reinterpret_cast<const f32x4_t*>(&ot[row * OS + c0]);
        if (p.out_hi) {
            const half4_t hi = __builtin_convertvector(of, half4_t);
            const f32x4_t back = __builtin_convertvector(hi, f32x4_t);
            const int64_t off = (qbase + qq) * p.ldoh + h * HD + c0;
            *reinterpret_cast<half4_t*>(reinterpret_cast<_Float16*>(p.out_hi) + off) = hi;
            *reinterpret_cast<half4_t*>(reinterpret_cast<_Float16*>(p.out_lo) + off) = __builtin_convertvector(of - back, half4_t);
        } else {
            *reinterpret_cast<f32x4_t*>(p.out + (qbase + qq) * p.ldo + h * HD + c0) = of;
        }
    }
}

template <int HD>
void launch_hd(const AttnArgs& a, const char* name, hipStream_t s) {
    constexpr size_t LDS_BYTES = AttnHd<HD>::LDS_BYTES;
    if (LDS_BYTES > 64 * 1024) {  // beyond what a launch may ask for without the attribute
        static bool attr_set = false;
        if (!attr_set) {
            SC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_hd_kernel<HD>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES));
            attr_set = true;
        }
    }
    const double pairs = a.pairs > 0 ? a.pairs : (double)a.nb * a.Sq * a.Skv;
    prof::Scope scope(name, 4.0 * a.heads * pairs * HD, 4.0 * a.nb * a.heads * HD * (2.0 * a.Sq + 2.0 * a.Skv), s);
    dim3 grid(cdiv(a.Sq, MQ), a.heads, a.nb);
    hipLaunchKernelGGL(attn_hd_kernel<HD>, grid, dim3(256), LDS_BYTES, s, a, 1.0f / sqrtf((float)HD));
    SC_LAUNCH_CHECK();
}

}  // namespace

void launch_attention_hd(const AttnArgs& a, hipStream_t s) {
    SC_CHECK(a.head_dim == 80 || a.head_dim == 128, "attention_hd: head_dim=%d", a.head_dim);
    const bool hd80 = a.head_dim == 80;
    SC_CHECK(a.nb > 0 && a.heads > 0 && a.Sq > 0 && a.Skv > 0, "attention%d: empty problem", a.head_dim);
    if (hd80)
        SC_CHECK(!a.causal && !a.rel_k && !a.rp_table && !a.row_off && !a.out_hi && !a.out_lo,
                 "attention80: head_dim 80 takes the plain mode only (no causal mask, relative positions, packed rows or plane output)");
    else
        SC_CHECK(!a.causal && !a.rel_k && !a.rp_table,
                 "attention128: head_dim 128 takes the key-length mask only (no causal mask, no Shaw or Transformer-XL relative positions)");
    SC_CHECK(a.q && a.k && a.v && (a.out || (a.out_hi && a.out_lo)), "attention%d: null operand", a.head_dim);
    SC_CHECK(!a.row_off || (a.kv_lens && a.Sq == a.Skv), "attention%d: packed rows need kv_lens and Sq == Skv", a.head_dim);
    SC_CHECK(a.ldq % 4 == 0 && a.ldk % 4 == 0 && a.ldv % 4 == 0 &&
                 ((reinterpret_cast<uintptr_t>(a.q) | reinterpret_cast<uintptr_t>(a.k) | reinterpret_cast<uintptr_t>(a.v)) & 15) == 0,
             "attention%d: row strides must be multiples of 4 and the operands 16-byte aligned", a.head_dim);
    if (a.out_hi)
        SC_CHECK(a.ldoh % 4 == 0 && ((reinterpret_cast<uintptr_t>(a.out_hi) | reinterpret_cast<uintptr_t>(a.out_lo)) & 7) == 0,
                 "attention%d: the output planes need a row stride that is a multiple of 4 and 8-byte alignment", a.head_dim);
    else
        SC_CHECK(a.ldo % 4 == 0 && (reinterpret_cast<uintptr_t>(a.out) & 15) == 0,
                 "attention%d: the output needs a row stride that is a multiple of 4 and 16-byte alignment", a.head_dim);
    SC_CHECK(a.heads <= 65535 && a.nb <= 65535, "attention%d: heads=%d nb=%d exceed the grid", a.head_dim, a.heads, a.nb);
    if (hd80)
        launch_hd<80>(a, "attention80", s);
    else
        launch_hd<128>(a, "attention128", s);
}

}  // namespace sc
