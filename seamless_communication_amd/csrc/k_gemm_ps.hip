// Dense product with a PRE-SPLIT activation operand:  C = alpha * act(A x W^T + bias) + res, where the
// fp32 activation matrix A is stored by its producer (LayerNorm, a previous product's epilogue, attention)
// as two fp16 planes  A_hi = fp16(A),  A_lo = fp16(A - A_hi)  -- the same split the other product
// kernels (k_gemm.hip, k_gemm2.hip) compute on the fly, so the results are bit-identical to theirs.
//
// With fp16 operands on both sides nothing has to pass through registers on the way in: all three
// operand tiles (A_hi, A_lo, W; 128 x 32 halfs = 8 KB each) are moved global -> LDS by the buffer
// unit itself (`buffer_load_dwordx4 ... lds`, 1 KB per wave instruction).  The slab loop then holds only
// ds_read_b128 + MFMA + 6 DMA issues per wave: no conversion VALU, no ds_write, no staging VGPRs.
//
//   * LDS layout of a tile: [rows][32 halfs] unpadded (the DMA writes lane order: lane p of a 1 KB
//     chunk lands at byte 16 p), with the four 16-byte segments of a row XOR-swizzled by (row>>2)&3 -
//     each lane fetches the global segment that belongs at its fixed LDS position - so that the
//     ds_read_b128 fragment reads of a 16-lane group hit 16 distinct 16-byte slots;
//   * three LDS stages (72 KB, two workgroups per CU), prefetch distance 2, ONE s_barrier per K slab;
//     DMA completion is awaited with explicit s_waitcnt vmcnt(6) (the six DMAs of the next slab may
//     stay in flight) - __syncthreads() would drain them all;
//   * rows beyond M / N get an out-of-range buffer offset and arrive as zeros;
//   * same MFMA order as the other kernels: per 16-wide K chunk and fragment pair, hi then lo.
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "device_util.h"

namespace sc {


namespace {

constexpr int PBK = 32;
#define SC_LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))


// raw buffer resource: base (48 bit), stride 0, num_records = bytes, dword 3 as for every gfx9 raw buffer
__device__ __forceinline__ i32x4_t make_rsrc_words(const void* base, uint32_t bytes) {
    const uint64_t b = reinterpret_cast<uint64_t>(base);
    i32x4_t r;
    r[0] = __builtin_amdgcn_readfirstlane((int)(uint32_t)b);
    r[1] = __builtin_amdgcn_readfirstlane((int)(uint32_t)((b >> 32) & 0xffff));
    r[2] = __builtin_amdgcn_readfirstlane((int)bytes);
    r[3] = 0x00020000;
    return r;
}

// byte offset of (row, 16-byte segment s) inside an unpadded [rows][64 B] tile
__device__ __forceinline__ int swz(int row, int s) { return row * 64 + ((s ^ ((row >> 2) & 3)) << 4); }

// Reads the wave's fp32 tile back row-major: the four 16-lane groups of a ds_read_b128 ({0-3,12-15,20-27},
// {4-11,16-19,28-31} and the same +32) each take whole rows, 16 bytes per lane, so that the LDS reads are
// conflict free and every global access is a run of 16-byte pieces of one output row.
template <int WM, int WN, int EP_LD, int ACT>
__device__ __forceinline__ void ps_epilogue(const GemmPsArgs& p, const float* ep, int m0w, int n0w, int lane) {
    constexpr int LPR = WN / 4;        // lanes per row
    constexpr int RPG = 16 / LPR;      // rows per 16-lane group
    constexpr int RPI = 4 * RPG;       // rows per wave instruction
    const int l5 = lane & 31;
    const bool g1 = (l5 >= 4 && l5 < 12) || (l5 >= 16 && l5 < 20) || l5 >= 28;
    const int rank = g1 ? (l5 < 12 ? l5 - 4 : l5 < 20 ? l5 - 8 : l5 - 16) : (l5 < 4 ? l5 : l5 < 16 ? l5 - 8 : l5 - 12);
    const int grp = (lane >> 5) * 2 + (g1 ? 1 : 0);
    const int row_in = grp * RPG + rank / LPR;
    const int c0 = (rank % LPR) * 4;
    const int col = n0w + c0;
    const bool vec_ok = (col + 3 < p.N) && ((p.ldc | p.ldr | p.ldcs) % 4 == 0) && (n0w % 4 == 0);
    f32x4_t b4 = {0.f, 0.f, 0.f, 0.f};
    if (p.bias) {
#pragma unroll
        for (int e = 0; e < 4; ++e) b4[e] = (col + e < p.N) ? p.bias[col + e] : 0.f;
    }
#pragma unroll
    for (int it = 0; it < WM / RPI; ++it) {
        const int row = it * RPI + row_in;
        const int64_t m = m0w + row;
        const f32x4_t a = *reinterpret_cast<const f32x4_t*>(ep + row * EP_LD + c0);
        if (m >= p.M || col >= p.N) continue;
        const bool dead = p.row_valid && p.row_valid[m] == 0;  // padded row of a length bucket: exact zeros
        f32x4_t v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = dead ? 0.f : act<ACT>(a[e] + b4[e]) * p.alpha;
        if (vec_ok) {
            if (p.res && !dead) v += *reinterpret_cast<const f32x4_t*>(p.res + m * p.ldr + col);
            if (p.C) *reinterpret_cast<f32x4_t*>(p.C + m * p.ldc + col) = v;
            if (p.Ch) {
                if (p.plane_neg_slope != 1.0f) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = lrelu_in(v[e], p.plane_neg_slope);
                }
                const half4_t hi = __builtin_convertvector(v, half4_t);
                *reinterpret_cast<half4_t*>(reinterpret_cast<_Float16*>(p.Ch) + m * p.ldcs + col) = hi;
                if (p.Cl)  // null: the consumer multiplies the hi plane only (GemmPsArgs::split == 0), no lo plane is produced
                    *reinterpret_cast<half4_t*>(reinterpret_cast<_Float16*>(p.Cl) + m * p.ldcs + col) =
                        __builtin_convertvector(v - __builtin_convertvector(hi, f32x4_t), half4_t);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (col + e >= p.N) continue;
                float x = v[e];
                if (p.res && !dead) x += p.res[m * p.ldr + col + e];
                if (p.C) p.C[m * p.ldc + col + e] = x;
                if (p.Ch) {
                    if (p.plane_neg_slope != 1.0f) x = lrelu_in(x, p.plane_neg_slope);
                    const _Float16 h = (_Float16)x;  // not split1: the lo half is formed only where p.Cl takes it
                    reinterpret_cast<_Float16*>(p.Ch)[m * p.ldcs + col + e] = h;
                    if (p.Cl) reinterpret_cast<_Float16*>(p.Cl)[m * p.ldcs + col + e] = (_Float16)(x - (float)h);
                }
            }
        }
    }
}

// GLU epilogue (launch_gemm_presplit_glu): the weight's rows were interleaved at load (column 2j = value j, column 2j + 1 =
// gate j), so a lane's 16-byte piece holds (a_j, g_j, a_j+1, g_j+1) after the bias; it stores a * sigmoid(g) of both pairs -
// glu_kernel's expression - to an fp32 C of N / 2 columns.  Same lane -> (row, column) walk as ps_epilogue; N % 4 == 0.
template <int WM, int WN, int EP_LD>
__device__ __forceinline__ void ps_epilogue_glu(const GemmPsArgs& p, const float* ep, int m0w, int n0w, int lane) {
    constexpr int LPR = WN / 4;
    constexpr int RPG = 16 / LPR;
    constexpr int RPI = 4 * RPG;
    const int l5 = lane & 31;
    const bool g1 = (l5 >= 4 && l5 < 12) || (l5 >= 16 && l5 < 20) || l5 >= 28;
    const int rank = g1 ? (l5 < 12 ? l5 - 4 : l5 < 20 ? l5 - 8 : l5 - 16) : (l5 < 4 ? l5 : l5 < 16 ? l5 - 8 : l5 - 12);
    const int grp = (lane >> 5) * 2 + (g1 ? 1 : 0);
    const int row_in = grp * RPG + rank / LPR;
    const int c0 = (rank % LPR) * 4;
    const int col = n0w + c0;
    f32x4_t b4 = {0.f, 0.f, 0.f, 0.f};
    if (p.bias && col < p.N) b4 = *reinterpret_cast<const f32x4_t*>(p.bias + col);
#pragma unroll
    for (int it = 0; it < WM / RPI; ++it) {
        const int row = it * RPI + row_in;
        const int64_t m = m0w + row;
        const f32x4_t acc = *reinterpret_cast<const f32x4_t*>(ep + row * EP_LD + c0);
        if (m >= p.M || col >= p.N) continue;
        f32x4_t v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = act<ACT_NONE>(acc[e] + b4[e]) * p.alpha;  // = what ps_epilogue stores to C
        float2 o;
        o.x = v[0] / (1.f + expf(-v[1]));
        o.y = v[2] / (1.f + expf(-v[3]));
        *reinterpret_cast<float2*>(p.C + m * p.ldc + (col >> 1)) = o;
    }
}

// WGM x WGN waves per workgroup.  2 x 2 waves on a 128 x 128 (64 x 64) tile is the round-1 shape; 4 x 2 waves on a
// 256 x 256 tile (wave tile 64 x 128) halves the barriers per MFMA (32 matrix instructions per slab and wave instead of
// 16) and takes the fragment reads from 0.75 to 0.5 ds_read_b128 per MFMA at the same 6 DMAs per wave and slab; its
// three stages fill 144 KB of the 160 KB LDS (one workgroup of 8 waves per CU = the same 2 waves per SIMD).
// SPLIT = false (GemmPsArgs::split == 0): the lo plane is neither fetched nor multiplied - A rounded to fp16 once.
// AMAX: the epilogue keeps, per row, the largest value of the wave's columns and its (lowest) column instead of writing the
// tile (GemmPsArgs::amax); a separate instantiation, so that the other kernels' code does not change by a single instruction.
// SCORE: the epilogue keeps, per row, one log-softmax record of the wave's columns (GemmScoreArgs, kernels.h) instead of
// writing the tile - the vocabulary projection of teacher-forced scoring; a kernel of its own (gemm_score_kernel) around the
// same body, so that gemm_ps_kernel keeps its instantiations, their names and their code.
//
// The K loop's schedule follows from SPLIT and the wave count; every schedule issues the same instructions per accumulator
// in the same order (slab, 16-wide K chunk, hi then lo): bit-identical results.
// In all of them the DMA instructions that refill the free stage are issued BETWEEN the matrix instructions of a slab
// instead of as a block in front of them: an LDS-DMA issue costs the wave 60-180 cycles (MI355X_MICROARCH.md,
// per-instruction constants), six of them in a row are as long as the slab's 16 MFMAs, and with the block form the matrix
// pipe of the SIMD idles through them unless the other resident workgroup happens to be in its compute phase.
//   * hi plane only (PS_STEP): one barrier in front of each slab, DMA q of the refill after the q-th MFMA.
//   * split, 4 waves (mid-slab barrier): the slab's barrier sits in the MIDDLE of its matrix instructions instead of in
//     front of them.  With the barrier in front, all the waves leave it together, request their 16 fragments together
//     (128 KB of LDS reads per 8-wave workgroup) and nobody has a matrix instruction to issue until the first ones are
//     back; the hi/lo pairs of the slab's second 16-wide K chunk and the next slab's first-chunk fragments are then
//     fetched under running MFMAs:
//       step s:  read chunk-1 fragments of slab s | MFMA chunk 0 (fragments carried in registers) + DMAs 3..5 of slab s+2
//                wait for slab s+1's DMAs, BARRIER | read chunk-0 fragments of slab s+1 | MFMA chunk 1 + DMAs 0..2 of slab s+3
//     After the barrier every wave has matrix work in registers at once.  The barrier of step s also says that every wave
//     is done reading slab s (both chunks: lgkmcnt(0) in front of it), so slab s+3 may land in the same stage from there on.
//   * split, 8 waves (alternating segments): the two waves of a SIMD take TURNS.  With the mid-slab barrier both run the
//     same program in lock step - both ask LDS for fragments at the same time, both issue their DMAs at the same time, both
//     want the matrix pipe at the same time - and the pipe measured 47 - 53 % busy (profiles/r3_gemm_ps256_pmc_sq.txt).
//     Here every 16-wide K chunk of a slab is a LOAD segment (the chunk's 8 fragment reads into registers + 3 of the
//     wave's 6 DMAs of the slab two ahead) and a COMPUTE segment (the chunk's 16 matrix instructions out of registers,
//     nothing else, s_setprio 1), one s_barrier after each; waves 0-3 (one per SIMD) load while waves 4-7 compute and the
//     other way round:
//       segment 4s   : waves 0-3  LOAD (s, 0)      waves 4-7  COMPUTE (s-1, 1)
//       segment 4s+1 : waves 0-3  COMPUTE (s, 0)   waves 4-7  LOAD (s, 0)
//       segment 4s+2 : waves 0-3  LOAD (s, 1)      waves 4-7  COMPUTE (s, 0)
//       segment 4s+3 : waves 0-3  COMPUTE (s, 1)   waves 4-7  LOAD (s, 1);  all: wait for slab s+1
//     A wave's matrix instructions find the pipe free (its partner is in its load segment), and its loads cost no matrix
//     time.  Moving some of a chunk's DMAs from the load segment in between the compute segment's matrix instructions
//     measured slower, and neither dropping the priorities, nor raising the load segment's, nor whole-slab segments (two
//     barriers per slab) moved the time (profiles/r5_gemm_alternating_schedule.txt).
//     Ordering: the DMAs of slab s+1 are awaited (counted vmcnt, the 6 of slab s+2 stay in flight) in front of the barrier
//     that ends segment 4s+3 and read from segment 4s+4 on; a stage is refilled (slab s+2 -> stage of slab s-1) from
//     segment 4s on, its last reads were issued in segment 4s-1 and retired (lgkmcnt(0)) in front of that segment's barrier.
// The kernel body lives in k_gemm_ps_body.h and is included by two kernels: gemm_ps_kernel (store and arg-max epilogues, the
// kernel arguments, instantiations and names it always had) and gemm_score_kernel (the SCORE epilogue, GemmScoreArgs behind the
// same arguments).  The body reads the template parameters BM, BN, WGM, WGN, SPLIT, CONV, AMAX, SCORE and the arguments by name.
template <int BM, int BN, int WGM, int WGN, bool SPLIT, bool CONV, bool AMAX>
__global__ __launch_bounds__(WGM* WGN * 64) void gemm_ps_kernel(GemmPsArgs p, int tiles_n, int tiles_total, int tiles_per_xcd,
                                                                 uint32_t a_bytes, uint32_t w_bytes) {
    constexpr bool SCORE = false, CAND = false, GLU = false;
    const GemmScoreArgs sc{};  // never read: every use sits behind `if constexpr (SCORE)`
    const GemmCandArgs cd{};   // nor this one (`if constexpr (CAND)`)
#include "k_gemm_ps_body.h"
}

// the split plain product with the SCORE epilogue (launch_gemm_presplit_score)
template <int BM, int BN, int WGM, int WGN>
__global__ __launch_bounds__(WGM* WGN * 64) void gemm_score_kernel(GemmPsArgs p, int tiles_n, int tiles_total, int tiles_per_xcd,
                                                                    uint32_t a_bytes, uint32_t w_bytes, GemmScoreArgs sc) {
    constexpr bool SPLIT = true, CONV = false, AMAX = false, SCORE = true, CAND = false, GLU = false;
    const GemmCandArgs cd{};  // never read: every use sits behind `if constexpr (CAND)`
#include "k_gemm_ps_body.h"
}

// the SCORE epilogue with a candidate list instead of a target per row (launch_gemm_presplit_score_cand); a kernel of its own
// for the same reason: the two above keep their code
template <int BM, int BN, int WGM, int WGN>
__global__ __launch_bounds__(WGM* WGN * 64) void gemm_cand_kernel(GemmPsArgs p, int tiles_n, int tiles_total, int tiles_per_xcd,
                                                                   uint32_t a_bytes, uint32_t w_bytes, GemmScoreArgs sc, GemmCandArgs cd) {
    constexpr bool SPLIT = true, CONV = false, AMAX = false, SCORE = true, CAND = true, GLU = false;
#include "k_gemm_ps_body.h"
}

// the split plain product with the GLU epilogue (launch_gemm_presplit_glu: the first pointwise convolution of the Conformer
// convolution module); a kernel of its own like the two above: the K loop is the shared body, the others keep their code
template <int BM, int BN, int WGM, int WGN>
__global__ __launch_bounds__(WGM* WGN * 64) void gemm_glu_kernel(GemmPsArgs p, int tiles_n, int tiles_total, int tiles_per_xcd,
                                                                  uint32_t a_bytes, uint32_t w_bytes) {
    constexpr bool SPLIT = true, CONV = false, AMAX = false, SCORE = false, CAND = false, GLU = true;
    const GemmScoreArgs sc{};  // never read: every use sits behind `if constexpr (SCORE)`
    const GemmCandArgs cd{};   // nor this one (`if constexpr (CAND)`)
#include "k_gemm_ps_body.h"
}

template <int BM, int BN, int WGM, int WGN>
void launch_ps_cfg(const GemmPsArgs& a, hipStream_t s, const GemmScoreArgs* score = nullptr, const GemmCandArgs* cand = nullptr,
                   bool glu = false) {
    const int tiles_m = cdiv(a.M, BM), tiles_n = cdiv(a.N, BN);
    const int tiles_total = tiles_m * tiles_n;
    const int tiles_per_xcd = cdiv(tiles_total, 8);
    char name[64];
    snprintf(name, sizeof(name), "gemm_%dx%d_presplit", BM, BN);
    prof::Scope scope(name, 2.0 * a.M * (double)a.N * a.K,
                      4.0 * a.M * (double)a.K + 2.0 * a.N * (double)a.K + (score ? 4.0 * a.M * (SCORE_REC_FLOATS * (double)score->ld + (cand ? cand->n_cand : 0)) : a.amax ? 8.0 * a.M * (double)a.amax_ld : glu ? 2.0 * a.M * (double)a.N : 4.0 * a.M * (double)a.N * (a.res ? 2.0 : 1.0)), s);
    const dim3 grid(tiles_per_xcd * 8), block(WGM * WGN * 64);
    const uint32_t ab = (uint32_t)((int64_t)a.M * a.lda * 2), wb = (uint32_t)((int64_t)a.N * a.ldw * 2);
    const auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, 0, s, a, tiles_n, tiles_total, tiles_per_xcd, ab, wb); };
    const bool conv = a.conv_taps > 0;
    if (score && cand) hipLaunchKernelGGL((gemm_cand_kernel<BM, BN, WGM, WGN>), grid, block, 0, s, a, tiles_n, tiles_total, tiles_per_xcd, ab, wb, *score, *cand);
    else if (score) hipLaunchKernelGGL((gemm_score_kernel<BM, BN, WGM, WGN>), grid, block, 0, s, a, tiles_n, tiles_total, tiles_per_xcd, ab, wb, *score);
    else if (glu) launch(gemm_glu_kernel<BM, BN, WGM, WGN>);
    else if (a.amax) launch(gemm_ps_kernel<BM, BN, WGM, WGN, true, false, true>);  // split, plain product (launch_gemm_presplit)
    else if (a.split && conv) launch(gemm_ps_kernel<BM, BN, WGM, WGN, true, true, false>);
    else if (a.split) launch(gemm_ps_kernel<BM, BN, WGM, WGN, true, false, false>);
    else if (conv) launch(gemm_ps_kernel<BM, BN, WGM, WGN, false, true, false>);
    else launch(gemm_ps_kernel<BM, BN, WGM, WGN, false, false, false>);
}

// The scoring product's tile, from N alone: a row's record boundaries - and with them the order in which its exponentials
// are summed - must not move with the number of rows in the launch, nor with a tile-choice switch (SC_PS_TILE and its kin
// change no result, and here the tile decides the summation order).  The widest tile from 1024 columns on (128-column
// records: the fewest records, and the product streams W once per 256 rows), 128 x 128 from 256, 64 x 64 below.
int score_tile(int N) { return N >= 1024 ? 256 : N >= 256 ? 128 : 64; }

// tile choice: 256 x 256 (8 waves) once it fills the chip about once, 128 x 128 down to one round of 256 tiles,
// 64 x 64 below.  SC_PS_TILE=128 (development A/B) keeps the round-1 choice.  All three accumulate every output
// element in the same order (16-wide K chunks, hi then lo): identical bits.
int ps_tile(int M, int N) {
    static const int max_tile = knob::value("SC_PS_TILE", 256);
    const int64_t tiles128 = (int64_t)cdiv(M, 128) * cdiv(N, 128);
    const int64_t tiles256 = (int64_t)cdiv(M, 256) * cdiv(N, 256);
    // (N <= 128: a 256-wide tile would idle half its columns - the 128-channel vocoder stage)
    static const int min256 = knob::value("SC_PS_MIN256", 224);
    static const int min128 = knob::value("SC_PS_MIN128", 256);
    if (max_tile >= 256 && tiles256 >= min256 && N > 128) return 256;
    return tiles128 >= min128 ? 128 : 64;
}

}  // namespace

void launch_gemm_presplit(const GemmPsArgs& a, hipStream_t s) {
    SC_CHECK(a.Ah && (a.Al || !a.split) && a.W && (a.C || a.Ch || a.amax), "presplit gemm: null operand");
    SC_CHECK(a.Ch || !a.Cl, "presplit gemm: a lo output plane needs its hi plane");
    SC_CHECK(a.act >= ACT_NONE && a.act <= ACT_TANH, "presplit gemm: activation %d has no epilogue here", a.act);
    SC_CHECK(a.M > 0 && a.N > 0 && a.K > 0 && a.K % PBK == 0, "presplit gemm: M=%d N=%d K=%d (K must be a multiple of 32)", a.M, a.N, a.K);
    SC_CHECK(a.lda % 8 == 0 && a.ldw % 8 == 0 && a.ldw >= a.K, "presplit gemm: lda=%lld ldw=%lld", (long long)a.lda,
             (long long)a.ldw);
    SC_CHECK(((reinterpret_cast<uintptr_t>(a.Ah) | reinterpret_cast<uintptr_t>(a.Al) | reinterpret_cast<uintptr_t>(a.W) |
               reinterpret_cast<uintptr_t>(a.C) | reinterpret_cast<uintptr_t>(a.res)) & 15) == 0 &&
                 ((reinterpret_cast<uintptr_t>(a.Ch) | reinterpret_cast<uintptr_t>(a.Cl)) & 7) == 0,
             "presplit gemm: operands must be 16-byte aligned");
    SC_CHECK((int64_t)a.M * a.lda * 2 < (1ll << 31) && (int64_t)a.N * a.ldw * 2 < (1ll << 31), "presplit gemm: operand larger than 2 GB");
    if (a.conv_taps > 0) {
        SC_CHECK(a.conv_cin % PBK == 0 && a.K == a.conv_taps * a.conv_cin && a.lda >= a.conv_cin &&
                     (a.row_pos || (a.rows_per_item > 0 && a.M % a.rows_per_item == 0)) && a.conv_dil >= 1 && a.conv_pad >= 0,
                 "presplit conv: taps=%d cin=%d K=%d rows_per_item=%d M=%d", a.conv_taps, a.conv_cin, a.K, a.rows_per_item, a.M);
    } else {
        SC_CHECK(a.lda >= a.K, "presplit gemm: lda=%lld < K=%d", (long long)a.lda, a.K);
    }
    if (a.amax) {
        SC_CHECK(a.split && a.conv_taps == 0 && !a.C && !a.Ch && !a.res && !a.row_valid && a.act == ACT_NONE,
                 "presplit gemm: the fused arg-max takes a plain product (no C / planes / residual / activation)");
        SC_CHECK(a.amax_ld == gemm_presplit_amax_chunks(a.M, a.N), "presplit gemm: amax_ld=%d, this shape produces %d partial results per row",
                 a.amax_ld, gemm_presplit_amax_chunks(a.M, a.N));
    }
    const int tile = ps_tile(a.M, a.N);
    if (tile == 256) launch_ps_cfg<256, 256, 4, 2>(a, s);
    else if (tile == 128) launch_ps_cfg<128, 128, 2, 2>(a, s);
    else launch_ps_cfg<64, 64, 2, 2>(a, s);
    SC_LAUNCH_CHECK();
}

// C [M][N / 2] = GLU over the column pairs (2j, 2j + 1) of A.W^T + bias: W (and bias) with the value and the gate rows
// interleaved (launch_glu_interleave_rows).  Tile choice and K loop are launch_gemm_presplit's for (M, N): every value and
// every gate is accumulated exactly as that call would, and gated with launch_glu's expression.
void launch_gemm_presplit_glu(const GemmPsArgs& a, hipStream_t s) {
    SC_CHECK(a.Ah && a.Al && a.W && a.C && a.split, "presplit glu gemm: null operand");
    SC_CHECK(!a.Ch && !a.Cl && !a.res && !a.row_valid && !a.amax && a.conv_taps == 0 && a.act == ACT_NONE && a.alpha == 1.0f,
             "presplit glu gemm: a plain product (no planes / residual / activation / scale)");
    SC_CHECK(a.M > 0 && a.N > 0 && a.N % 4 == 0 && a.K > 0 && a.K % PBK == 0, "presplit glu gemm: M=%d N=%d K=%d (N %% 4, K %% 32)", a.M, a.N, a.K);
    SC_CHECK(a.lda % 8 == 0 && a.ldw % 8 == 0 && a.ldw >= a.K && a.lda >= a.K && a.ldc % 2 == 0 && a.ldc >= a.N / 2,
             "presplit glu gemm: lda=%lld ldw=%lld ldc=%lld", (long long)a.lda, (long long)a.ldw, (long long)a.ldc);
    SC_CHECK(((reinterpret_cast<uintptr_t>(a.Ah) | reinterpret_cast<uintptr_t>(a.Al) | reinterpret_cast<uintptr_t>(a.W) |
               reinterpret_cast<uintptr_t>(a.C) | reinterpret_cast<uintptr_t>(a.bias)) & 15) == 0,
             "presplit glu gemm: operands must be 16-byte aligned");
    SC_CHECK((int64_t)a.M * a.lda * 2 < (1ll << 31) && (int64_t)a.N * a.ldw * 2 < (1ll << 31), "presplit glu gemm: operand larger than 2 GB");
    const int tile = ps_tile(a.M, a.N);
    if (tile == 256) launch_ps_cfg<256, 256, 4, 2>(a, s, nullptr, nullptr, true);
    else if (tile == 128) launch_ps_cfg<128, 128, 2, 2>(a, s, nullptr, nullptr, true);
    else launch_ps_cfg<64, 64, 2, 2>(a, s, nullptr, nullptr, true);
    SC_LAUNCH_CHECK();
}

int gemm_presplit_tile(int M, int N) { return ps_tile(M, N); }

// every tile shape has two waves side by side (WGN = 2): two partial results per tile column
int gemm_presplit_amax_chunks(int M, int N) { return 2 * cdiv(N, ps_tile(M, N)); }

namespace {
// one wave per row: the partial results in column order, the largest value wins, the lowest column among equal values
__global__ __launch_bounds__(256) void amax_finish_kernel(const float2* __restrict__ part, int ld, int rows, int* __restrict__ out_idx) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float2* pr = part + (int64_t)row * ld;
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    for (int i = lane; i < ld; i += 64) {
        const float2 v = pr[i];
        const int vi = __float_as_int(v.y);
        if (v.x > best || (v.x == best && vi < bidx)) {
            best = v.x;
            bidx = vi;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(bidx, o);
        if (ob > best || (ob == best && oi < bidx)) {
            best = ob;
            bidx = oi;
        }
    }
    if (lane == 0) out_idx[row] = argmax_stored_index(bidx);
}
}  // namespace

void launch_amax_finish(const float2* part, int ld, int rows, int* out_idx, hipStream_t s) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(amax_finish_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, s, part, ld, rows, out_idx);
    SC_LAUNCH_CHECK();
}

// ---- teacher-forced scoring: log-softmax statistics of A x W^T without the logits ----
int gemm_score_record_cols(int N) { return score_tile(N) / 2; }  // two waves side by side in every tile shape
int gemm_score_records(int N) { return cdiv(N, gemm_score_record_cols(N)); }
int gemm_score_group_rows(int N) {
    const int64_t per_row = (int64_t)gemm_score_records(N) * SCORE_REC_FLOATS * 4;
    const int64_t rows = SCORE_SCRATCH_BYTES / per_row;
    return (int)std::min<int64_t>(std::max<int64_t>(rows / 256 * 256, 256), 1 << 20);  // whole 256-row tiles; one tile row at the least
}

namespace {
// One wave per row.  Lane l takes records l, l + 64, ... in ascending order, the 64 partial results meet in a butterfly
// (xor 32 ... 1): the order depends on the number of records only.  First the row's maximum and its lowest column, then the
// records' sums rescaled to that maximum.
// (every lane of the wave ends up with the row's four values)
__device__ __forceinline__ void score_fold(const float* __restrict__ pr, int ld, int lane, float& best, int& bidx, float& tot, float& sv) {
    best = -INFINITY;
    bidx = 0x7fffffff;
    for (int i = lane; i < ld; i += 64) {
        const float v = pr[i * SCORE_REC_FLOATS];
        const int vi = __float_as_int(pr[i * SCORE_REC_FLOATS + 4]);
        if (v > best || (v == best && vi < bidx)) {
            best = v;
            bidx = vi;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(bidx, o);
        if (ob > best || (ob == best && oi < bidx)) {
            best = ob;
            bidx = oi;
        }
    }
    tot = 0.f, sv = 0.f;
    for (int i = lane; i < ld; i += 64) {
        // product and sum rounded separately, by pragma: left to the compiler, score_finish_kernel rounds twice (it adds tot
        // and sv as a pair) while a kernel that drops sv fuses the two into one fma - and a lane with more than one record
        // (ld > 64: the full-size vocabulary) then sums to other bits
        const float ex = expf(pr[i * SCORE_REC_FLOATS] - best);
        {
#pragma clang fp contract(off)
            const float term = pr[i * SCORE_REC_FLOATS + 1] * ex;
            tot = tot + term;
        }
        sv += pr[i * SCORE_REC_FLOATS + 2];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        tot += __shfl_xor(tot, o);
        sv += __shfl_xor(sv, o);
    }
}

__global__ __launch_bounds__(256) void score_finish_kernel(const float* __restrict__ rec, int ld, int rows, int N, int cols,
                                                            const int* __restrict__ target, float* __restrict__ lprob,
                                                            float* __restrict__ sum_lprob, float* __restrict__ lse_out,
                                                            int* __restrict__ top1) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* pr = rec + (int64_t)row * ld * SCORE_REC_FLOATS;
    float best, tot, sv;
    int bidx;
    score_fold(pr, ld, lane, best, bidx, tot, sv);
    if (lane != 0) return;
    // the record that holds the maximum contributes its own sum unscaled, and that sum holds exp(0) = 1: tot >= 1, log >= 0
    const float lt = logf(tot);
    const float lse = best + lt;
    const int tgt = target[row];
    if (lprob) {
        float lp = 0.f;  // no target (< 0 or outside the row): 0
        if (tgt >= 0 && tgt < N) lp = (pr[(tgt / cols) * SCORE_REC_FLOATS + 3] - best) - lt;  // <= 0; exactly -log(tot) at the maximum
        lprob[row] = lp;
    }
    if (sum_lprob) sum_lprob[row] = sv - (float)N * lse;
    if (lse_out) lse_out[row] = lse;
    if (top1) top1[row] = argmax_stored_index(bidx);
}

// The candidate form's finish: the same fold, then lane l takes candidates l, l + 64, ...: the log-probability by the target
// form's expression, and the arg-max over the candidates' values (the lowest j among equal values; NaN never wins, a row of
// NaN keeps the sentinel = stored as 0).
__global__ __launch_bounds__(256) void cand_finish_kernel(const float* __restrict__ rec, int ld, int rows, const float* __restrict__ cand_v,
                                                           int n_cand, float* __restrict__ lprob, int* __restrict__ best_j) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float best, tot, sv;
    int bidx;
    score_fold(rec + (int64_t)row * ld * SCORE_REC_FLOATS, ld, lane, best, bidx, tot, sv);
    const float lt = logf(tot);
    float cb = -INFINITY;
    int cj = 0x7fffffff;
    for (int j = lane; j < n_cand; j += 64) {
        const float v = cand_v[(int64_t)row * n_cand + j];
        lprob[(int64_t)row * n_cand + j] = (v - best) - lt;
        if (v > cb || (v == cb && j < cj)) {
            cb = v;
            cj = j;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(cb, o);
        const int oj = __shfl_xor(cj, o);
        if (ob > cb || (ob == cb && oj < cj)) {
            cb = ob;
            cj = oj;
        }
    }
    if (lane == 0) best_j[row] = argmax_stored_index(cj);
}
}  // namespace

void launch_gemm_presplit_score(const GemmPsArgs& a, const int* target, float* rec, int rec_rows, float* lprob, float* sum_lprob,
                                float* lse, int* top1, hipStream_t s) {
    SC_CHECK(a.Ah && a.Al && a.W && target && rec && rec_rows > 0, "presplit score: null operand");
    SC_CHECK(a.split && a.conv_taps == 0 && !a.C && !a.Ch && !a.Cl && !a.res && !a.row_valid && !a.amax && a.act == ACT_NONE,
             "presplit score: takes a plain product (no C / planes / residual / activation)");
    SC_CHECK(a.M > 0 && a.N > 0 && a.K > 0 && a.K % PBK == 0, "presplit score: M=%d N=%d K=%d (K must be a multiple of 32)", a.M, a.N, a.K);
    SC_CHECK(a.lda % 8 == 0 && a.ldw % 8 == 0 && a.ldw >= a.K && a.lda >= a.K, "presplit score: lda=%lld ldw=%lld", (long long)a.lda,
             (long long)a.ldw);
    SC_CHECK(((reinterpret_cast<uintptr_t>(a.Ah) | reinterpret_cast<uintptr_t>(a.Al) | reinterpret_cast<uintptr_t>(a.W)) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(rec) & 7) == 0,
             "presplit score: operands must be 16-byte aligned");
    SC_CHECK((int64_t)a.N * a.ldw * 2 < (1ll << 31), "presplit score: weight larger than 2 GB");
    const int tile = score_tile(a.N), cols = tile / 2, ld = cdiv(a.N, cols);
    // rows in groups of rec_rows: the records of one group at a time (a row's results do not depend on its group)
    for (int r0 = 0; r0 < a.M; r0 += rec_rows) {
        GemmPsArgs g = a;
        g.M = std::min(rec_rows, a.M - r0);
        g.Ah = a.Ah + (int64_t)r0 * a.lda;
        g.Al = a.Al + (int64_t)r0 * a.lda;
        SC_CHECK((int64_t)g.M * a.lda * 2 < (1ll << 31), "presplit score: row group larger than 2 GB");
        GemmScoreArgs sa;
        sa.rec = rec;
        sa.target = target + r0;
        sa.ld = ld;
        if (tile == 256) launch_ps_cfg<256, 256, 4, 2>(g, s, &sa);
        else if (tile == 128) launch_ps_cfg<128, 128, 2, 2>(g, s, &sa);
        else launch_ps_cfg<64, 64, 2, 2>(g, s, &sa);
        SC_LAUNCH_CHECK();
        hipLaunchKernelGGL(score_finish_kernel, dim3(cdiv(g.M, 4)), dim3(256), 0, s, rec, ld, g.M, a.N, cols, target + r0,
                           lprob ? lprob + r0 : nullptr, sum_lprob ? sum_lprob + r0 : nullptr, lse ? lse + r0 : nullptr,
                           top1 ? top1 + r0 : nullptr);
        SC_LAUNCH_CHECK();
    }
}

void check_score_candidates(const int32_t* h_cand, int n_cand, int N, const char* who) {
    SC_CHECK(h_cand, "%s: null candidate list", who);
    SC_CHECK(n_cand >= 1 && n_cand <= SCORE_MAX_CAND, "%s: n_cand=%d outside 1..%d", who, n_cand, SCORE_MAX_CAND);
    for (int j = 0; j < n_cand; ++j) {
        SC_CHECK(h_cand[j] >= 0 && h_cand[j] < N, "%s: candidate %d (entry %d) outside the vocabulary [0, %d)", who, h_cand[j], j, N);
        SC_CHECK(j == 0 || h_cand[j] > h_cand[j - 1], "%s: the candidate list is not strictly ascending at entry %d (%d after %d)", who, j,
                 h_cand[j], h_cand[j - 1]);
    }
}

void launch_gemm_presplit_score_cand(const GemmPsArgs& a, const int* cand, int n_cand, float* rec, float* cand_v, int rec_rows,
                                     float* lprob, int* best_j, hipStream_t s) {
    SC_CHECK(a.Ah && a.Al && a.W && cand && rec && cand_v && lprob && best_j && rec_rows > 0, "presplit candidates: null operand");
    SC_CHECK(n_cand >= 1 && n_cand <= SCORE_MAX_CAND, "presplit candidates: %d candidates outside 1..%d", n_cand, SCORE_MAX_CAND);
    SC_CHECK(a.split && a.conv_taps == 0 && !a.C && !a.Ch && !a.Cl && !a.res && !a.row_valid && !a.amax && a.act == ACT_NONE,
             "presplit candidates: takes a plain product (no C / planes / residual / activation)");
    SC_CHECK(a.M > 0 && a.N > 0 && a.K > 0 && a.K % PBK == 0, "presplit candidates: M=%d N=%d K=%d (K must be a multiple of 32)", a.M, a.N, a.K);
    SC_CHECK(a.lda % 8 == 0 && a.ldw % 8 == 0 && a.ldw >= a.K && a.lda >= a.K, "presplit candidates: lda=%lld ldw=%lld", (long long)a.lda,
             (long long)a.ldw);
    SC_CHECK(((reinterpret_cast<uintptr_t>(a.Ah) | reinterpret_cast<uintptr_t>(a.Al) | reinterpret_cast<uintptr_t>(a.W)) & 15) == 0 &&
                 (reinterpret_cast<uintptr_t>(rec) & 7) == 0,
             "presplit candidates: operands must be 16-byte aligned");
    SC_CHECK((int64_t)a.N * a.ldw * 2 < (1ll << 31), "presplit candidates: weight larger than 2 GB");
    const int tile = score_tile(a.N), cols = tile / 2, ld = cdiv(a.N, cols);
    for (int r0 = 0; r0 < a.M; r0 += rec_rows) {  // row groups as in launch_gemm_presplit_score
        GemmPsArgs g = a;
        g.M = std::min(rec_rows, a.M - r0);
        g.Ah = a.Ah + (int64_t)r0 * a.lda;
        g.Al = a.Al + (int64_t)r0 * a.lda;
        SC_CHECK((int64_t)g.M * a.lda * 2 < (1ll << 31), "presplit candidates: row group larger than 2 GB");
        GemmScoreArgs sa;
        sa.rec = rec;
        sa.ld = ld;
        GemmCandArgs ca;
        ca.cand = cand;
        ca.v = cand_v;
        ca.n_cand = n_cand;
        if (tile == 256) launch_ps_cfg<256, 256, 4, 2>(g, s, &sa, &ca);
        else if (tile == 128) launch_ps_cfg<128, 128, 2, 2>(g, s, &sa, &ca);
        else launch_ps_cfg<64, 64, 2, 2>(g, s, &sa, &ca);
        SC_LAUNCH_CHECK();
        hipLaunchKernelGGL(cand_finish_kernel, dim3(cdiv(g.M, 4)), dim3(256), 0, s, rec, ld, g.M, cand_v, n_cand,
                           lprob + (int64_t)r0 * n_cand, best_j + r0);
        SC_LAUNCH_CHECK();
    }
}

}  // namespace sc
