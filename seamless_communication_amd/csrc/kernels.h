// Kernel launchers of libseamless_hip (gfx950 / CDNA4 only, wave64).
//
// Conventions
//   * activations: fp32, row-major [rows, channels], rows = batch-major time
//     (row = n * T + t), zero-padded to the batch maximum T;
//   * GEMM weights: fp16 [N_out, K] with K contiguous (nn.Linear layout); Conv1d
//     weights are repacked at load to [C_out, tap * C_in + c];
//   * every dense product is "A(fp32) x W(fp16)": A is split on the fly into
//     hi = fp16(x), lo = fp16(x - hi) (round to nearest even, fp16 subnormals
//     kept) and both halves go through v_mfma_f32_32x32x16_f16 with fp32
//     accumulation, at 2x the fp16 MFMA cost.  Numeric range (DESIGN.md 4b,
//     tests/split_model.py is the same statement as code):
//       - rows of about unit scale and larger: an fp32 x fp16 product to
//         ~2^-22 relative (needed for bit-exact greedy ids against the fp32
//         CPU reference).  Below |x| ~ 2^-3 the lo half is an fp16 subnormal
//         and a row that is small as a whole loses bits: ~6e-7 of the row's
//         maximum at 2^-4, 1e-5 at 2^-8, 2e-4 at 2^-12, 3e-3 at 2^-16;
//       - finite for |x| < 65520.  An element beyond it splits into inf and
//         -inf and its row of the product is NaN in every column;
//       - NaN stays NaN through every activation (ReLU is !(v <= 0) ? v : 0,
//         LeakyReLU in front of a split is lrelu_in below) and stays in its
//         row: the other rows of the launch keep their bits;
//       - the row arg-max kernels store an index inside the row whatever the
//         row holds (argmax_stored_index below); a NaN row's log-probability
//         is NaN.  The beam-search candidate kernels (plain, banned, chunked)
//         store only indices of real (beam, token) pairs and order them as
//         torch.topk does: NaN of any sign above +inf, then descending value,
//         ties (among NaNs too) to the lower flattened index; a token that a
//         step rule excludes is -inf even in a NaN row; the host picks the
//         best finished hypothesis in the same order (k_beam.hip order_key);
//       - the fp32 FMA GEMV (launch_gemv) does not split: exact fp32 x fp16
//         at every scale, no overflow at 65520.
#pragma once
#include <atomic>
#include <vector>

#include "common.h"
#include "boost_list.h"
#include "prof.h"

struct sc_tsm_opts;  // include/seamless_hip.h

namespace sc {

// ACT_GELU: exact (erf) GELU, 0.5 v (1 + erf(v / sqrt 2)); implemented by launch_gemm (both the fast and the general kernel),
// the LayerNorm launchers and the plane epilogue of launch_gemv3 behind its fused LayerNorm (the FFN-in of the row-group
// decoder step) - launch_gemm_presplit, launch_skinny and launch_gemvp refuse or ignore it
enum Act { ACT_NONE = 0, ACT_RELU = 1, ACT_SILU = 2, ACT_TANH = 3, ACT_GELU = 4 };
enum InAct { IN_NONE = 0, IN_LRELU_01 = 1, IN_LRELU_001 = 2 };

// What a row arg-max stores: its running index starts at 0x7fffffff and no comparison with NaN is true, so a row that is all
// NaN would hand that value on as a token id (the next step's embedding reads emb + tok * M).  Such a row gets index 0; its
// log-probability is NaN, which is how the caller sees it.  Every other row, all -inf included, has its index in range already.
__device__ __forceinline__ int argmax_stored_index(int idx) { return idx == 0x7fffffff ? 0 : idx; }

// LeakyReLU in front of a split (conv input activation, activated output planes).  One expression for every kernel that
// claims the bits of another; fmaxf / fminf drop a NaN operand, so NaN is handed through by hand - an input that is not a
// number must not turn into a finite product.  Finite and infinite x keep the bits the bare expression gives.
__device__ __forceinline__ float lrelu_in(float x, float slope) {
    const float r = fmaxf(x, 0.f) + slope * fminf(x, 0.f);
    return x != x ? x : r;
}

struct GemmArgs {
    const float* A = nullptr;
    int64_t lda = 0;  // floats between consecutive input rows
    const __half* W = nullptr;
    int64_t ldw = 0;             // halfs between weight rows (= padded K)
    int64_t w_phase_stride = 0;  // halfs between per-phase weight blocks
    const float* bias = nullptr;
    const float* res = nullptr;  // residual, indexed like C
    int64_t ldr = 0;
    float* C = nullptr;
    int64_t ldc = 0;
    int M = 0;  // GEMM rows = batch * rows_per_batch
    int N = 0;
    int K = 0;  // padded to a multiple of 32; k >= taps*cin reads as zero
    // implicit 1-D convolution addressing (plain GEMM: taps=1, cin=K, rows_per_batch=M)
    int rows_per_batch = 0;
    int t_in = 0;   // input rows per batch item
    int t_out = 0;  // output rows per batch item
    int taps = 1, cin = 0, dil = 0, stride = 1, pad = 0;  // src_t = q*stride + tap*dil - pad
    int out_mul = 1, out_off = 0, out_off_phase_step = 0;  // dst_t = q*out_mul + out_off + phase*step
    const int* in_lens = nullptr;  // per batch item: input rows >= len read as zero
    int in_act = IN_NONE;
    int act = ACT_NONE;
    float alpha = 1.0f;  // C = alpha * act(acc + bias) + res
    int phases = 1;
    int split = 1;  // 1: hi+lo split (near-fp32), 0: single fp16 rounding of A
    double algo_flops = 0;  // algorithmic FLOPs of this launch for the profiler (0: 2*M*N*taps*cin*phases)
    // packed items (the ragged vocoder pass): item i holds unit rows [item_off[i], item_off[i + 1]) and, at this product's
    // input rate, the input rows [item_off[i] * item_mul, item_off[i + 1] * item_mul) - items back to back, no rows in
    // between.  Its GEMM rows start at item_off[i] * item_mul + i * item_extra (item_extra = rows_per_batch - t_in of the
    // uniform form: 1 for the polyphase transposed convolution), its output rows at item_off[i] * item_mul * item_out_mul
    // (item_out_mul = t_out / t_in of the uniform form).  Replaces rows_per_batch / t_in / t_out, which are unused then;
    // M = item_off[n_items] * item_mul + n_items * item_extra.  in_lens must be null.
    const int* item_off = nullptr;  // [n_items + 1] on the device, null: uniform batch
    int n_items = 0, item_mul = 1, item_extra = 0, item_out_mul = 1;
};

#if defined(__HIPCC__)
// largest i in [0, n) with first(i) <= key, for a non-decreasing first() with first(0) <= key
template <typename F>
__device__ __forceinline__ int item_search(int n, int key, F first) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first(mid) <= key) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Walks the GEMM rows of a packed product in ascending order: seek(m) moves to the item that holds row m (m < M, not
// below the previous row), one comparison per row and one table read per item boundary.
struct GemmItemCursor {
    int n = 0, start = 0, next = 0x7fffffff;  // item, its first GEMM row, the next item's first GEMM row
    __device__ __forceinline__ static int first(const GemmArgs& p, int i) { return p.item_off[i] * p.item_mul + i * p.item_extra; }
    __device__ __forceinline__ void init(const GemmArgs& p, int m) {
        n = item_search(p.n_items, m, [&](int i) { return first(p, i); });
        start = first(p, n);
        next = first(p, n + 1);
    }
    __device__ __forceinline__ void seek(const GemmArgs& p, int m) {
        while (m >= next) {
            ++n;
            start = next;
            next = first(p, n + 1);
        }
    }
    __device__ __forceinline__ int q(int m) const { return m - start; }                        // row inside the item
    __device__ __forceinline__ int in_row0(const GemmArgs& p) const { return start - n * p.item_extra; }
    __device__ __forceinline__ int t_in(const GemmArgs& p) const { return next - start - p.item_extra; }
    __device__ __forceinline__ int t_out(const GemmArgs& p) const { return t_in(p) * p.item_out_mul; }
    __device__ __forceinline__ int64_t out_row0(const GemmArgs& p) const { return (int64_t)in_row0(p) * p.item_out_mul; }
};
#endif

void launch_gemm(const GemmArgs& a, hipStream_t s);
// k_gemm2.hip: double-buffered, XCD-aware fast path for split products with cin % 32 == 0 (same bits)
extern std::atomic<int> g_force_general_gemm;  // tests / A-B timing: 1 routes every product to the general kernel
bool gemm_fast_eligible(const GemmArgs& a);
void launch_gemm_fast(const GemmArgs& a, hipStream_t s);

// k_gemm_ps.hip: product with a PRE-SPLIT activation operand (two fp16 planes hi = fp16(a), lo = fp16(a - hi),
// written by the producer kernel); operands go global -> LDS by DMA.  C (fp32) and/or Ch/Cl (split planes for the
// next product) receive alpha * act(A.W^T + bias) + res.  Bit-identical to launch_gemm on the same values.
struct GemmPsArgs {
    const __half* Ah = nullptr;
    const __half* Al = nullptr;
    int64_t lda = 0;  // halfs between rows of Ah / Al
    const __half* W = nullptr;
    int64_t ldw = 0;
    const float* bias = nullptr;
    const float* res = nullptr;
    int64_t ldr = 0;
    float* C = nullptr;
    int64_t ldc = 0;
    __half* Ch = nullptr;
    __half* Cl = nullptr;
    int64_t ldcs = 0;
    int M = 0, N = 0, K = 0;
    int act = ACT_NONE;
    float alpha = 1.0f;
    int split = 1;  // 0: only the hi plane is multiplied (A rounded to fp16 once) - precision study, never the default
    // the planes Ch / Cl hold max(v, 0) + plane_neg_slope * min(v, 0) of the value v that goes to C (1: v itself): the next
    // convolution's LeakyReLU input of the HiFi-GAN ResBlocks, while C keeps the un-activated residual stream
    float plane_neg_slope = 1.0f;
    // implicit 1-D convolution over the rows of the planes (stride 1): the planes hold [items][rows_per_item][conv_cin]
    // (lda = row stride), K = conv_taps * conv_cin in tap-major order (the packed Conv1d weight layout), output row (i, t)
    // reads input rows t + tap * conv_dil - conv_pad of item i, rows outside [0, rows_per_item) as zeros.  conv_taps = 0:
    // plain product.  conv_cin % 32 == 0 (a 32-wide K slab stays inside one tap).
    int conv_taps = 0, conv_cin = 0, conv_dil = 1, conv_pad = 0, rows_per_item = 0;
    // rows with row_valid[m] == 0 (nullable) are written as exact zeros in every output (padded rows of a length
    // bucket: the next convolution's zero padding behind an item's end)
    const unsigned char* row_valid = nullptr;
    // packed (varlen) convolution: row_pos[m] = {position of row m inside its item, length of that item} (nullable);
    // replaces the uniform rows_per_item geometry: items of different lengths lie back to back, no padding rows
    const int2* row_pos = nullptr;
    // fused arg-max over the columns (the unit projection + arg-max of the NAR T2U, models/unity/model.py:438-441 +
    // inference/generator.py:346): nothing is written to C / Ch; every wave writes {largest value, its lowest column} of its
    // columns of row m to amax[m * amax_ld + chunk] (amax_ld = gemm_presplit_amax_chunks(M, N)); launch_amax_finish picks the
    // row's arg-max (lowest column among equal values, as launch_argmax_rows does on the stored logits).  act / res unused.
    float2* amax = nullptr;
    int amax_ld = 0;
};
void launch_gemm_presplit(const GemmPsArgs& a, hipStream_t s);
// The split plain product with GLU in its epilogue: W [N][K] (and bias [N]) hold the value and the gate rows of a [2C][K]
// weight INTERLEAVED (row 2j = value j, row 2j + 1 = gate j: launch_glu_interleave_rows), C [M][N / 2] fp32 receives
// value * sigmoid(gate).  Bit-identical to launch_gemm_presplit on the original weight followed by launch_glu: every element is
// accumulated in the same order (a column's place in the tile does not enter its arithmetic) and gated by the same expression.
// No planes / residual / activation / alpha; N % 4 == 0.
void launch_gemm_presplit_glu(const GemmPsArgs& a, hipStream_t s);
// dst row 2j = src row j, dst row 2j + 1 = src row C + j for j < C; rows of K halfs (ld_src / ld_dst apart); the bias
// (nullable, with its destination) likewise.  Done once per weight at load.
void launch_glu_interleave_rows(const __half* src, int64_t ld_src, const float* bias, int C, int K, __half* dst, int64_t ld_dst,
                                float* bias_dst, hipStream_t s);
int gemm_presplit_tile(int M, int N);         // rows (= columns) of the tile launch_gemm_presplit chooses for this shape
int gemm_presplit_amax_chunks(int M, int N);  // partial results per row the tile choice for this shape produces
void launch_amax_finish(const float2* part, int ld, int rows, int* out_idx, hipStream_t s);

// Teacher-forced scoring: per row m of the split plain product v = alpha * (A.W^T + bias), the log-softmax statistics
//   lse[m] = log sum_j exp(v[m][j]),  lprob[m] = v[m][target[m]] - lse[m]  (0 where target[m] < 0),
//   sum_lprob[m] = sum_j v[m][j] - N * lse[m],  top1[m] = arg-max (lowest column among equal values, launch_argmax_rows' rule)
// without the [M][N] logits: the product's epilogue writes, per row and per wave's column range (gemm_score_record_cols(N)
// columns, chosen from N alone), one record
//   {max, sum of exp(v - max), sum of v, v at the target column if it lies in the range, lowest column of max, -}
// (columns ascending inside a record), and a finish kernel folds a row's records in a fixed order.  A row's four results
// depend on that row of A, W, bias and its target only - not on M, not on the other rows, not on the row group.
// Rows go through in groups of rec_rows (the capacity of `rec`: rec_rows * gemm_score_records(N) * SCORE_REC_FLOATS floats);
// gemm_score_group_rows(N) keeps `rec` within SCORE_SCRATCH_BYTES.  A NaN in a row of A gives NaN lse / lprob / sum_lprob for
// that row only, top1 inside [0, N); a logit of +-inf makes its row NaN as well.  Any of the four outputs may be null.
constexpr int SCORE_REC_FLOATS = 6;
constexpr int64_t SCORE_SCRATCH_BYTES = 32ll << 20;
struct GemmScoreArgs {
    float* rec = nullptr;         // [rows of the launch][ld][SCORE_REC_FLOATS]
    const int* target = nullptr;  // [rows of the launch]
    int ld = 0;                   // records per row
};
int gemm_score_record_cols(int N);
int gemm_score_records(int N);
int gemm_score_group_rows(int N);
void launch_gemm_presplit_score(const GemmPsArgs& a, const int* target, float* rec, int rec_rows, float* lprob, float* sum_lprob,
                                float* lse, int* top1, hipStream_t s);

// Candidate-set form of the same product (language identification): instead of one target per row, a strictly ascending
// device list cand[0 .. n_cand) of columns shared by all rows, 1 <= n_cand <= SCORE_MAX_CAND, every entry inside [0, N) (the
// caller checks the list: the kernel trusts it).  Each wave writes, besides its record, v at every candidate column inside
// its column range - the record's own expression, read from the same LDS pass - to cand_v[m][j]; the finish kernel folds the
// records in launch_gemm_presplit_score's order and writes
//   lprob[m][j] = (cand_v[m][j] - max) - log(sum)   = bit for bit what the target form returns for target cand[j],
//   best_j[m]   = arg-max_j cand_v[m][j], the lowest j among equal values; 0 for a row whose values are all NaN.
// cand_v holds rec_rows * n_cand floats.  A row's results depend on that row only, as above.
constexpr int SCORE_MAX_CAND = 512;
struct GemmCandArgs {
    const int* cand = nullptr;  // [n_cand], strictly ascending
    float* v = nullptr;         // [rows of the launch][n_cand]
    int n_cand = 0;
};
// the host's check of a candidate list (1 .. SCORE_MAX_CAND entries, strictly ascending, inside [0, N)); throws, naming `who`
void check_score_candidates(const int32_t* h_cand, int n_cand, int N, const char* who);
void launch_gemm_presplit_score_cand(const GemmPsArgs& a, const int* cand, int n_cand, float* rec, float* cand_v, int rec_rows,
                                     float* lprob, int* best_j, hipStream_t s);

// k_resblock.hip: out = x + conv2_{k,1}(lrelu(conv1_{k,dil}(lrelu(x)) + b1)) + b2 for C in {16, 32, 64}, the
// intermediate kept in LDS; optionally out = ((avg_a + avg_b) + that) / 3.  Weights packed [C][ldw], tap-major.
struct ResPairArgs {
    const float* x = nullptr;  // [nb][T][C]
    float* out = nullptr;      // [nb][T][C]
    const __half* w1 = nullptr;
    int64_t ldw1 = 0;
    const float* b1 = nullptr;
    const __half* w2 = nullptr;
    int64_t ldw2 = 0;
    const float* b2 = nullptr;
    int nb = 0, T = 0, C = 0, k = 0, dil = 1;
    float slope = 0.1f;
    const float* avg_a = nullptr;
    const float* avg_b = nullptr;
    int single = 0;  // the hi fp16 plane of the activations only: one matrix instruction per fragment, no lo plane in LDS (the vocoder's default)
    // packed items (see GemmArgs::item_off): nb items, item i holds the rows [item_off[i] * item_mul, item_off[i + 1] * item_mul)
    // of x / out (T: the mean item length, for the profiler's figures only); a workgroup owns a tile of ONE item, tiles counted from the item's first row, and
    // tile_first[i] (nb + 1 entries, resblock_tile_first / mrf_tile_first) is the first workgroup of item i
    const int* item_off = nullptr;
    const int* tile_first = nullptr;
    int item_mul = 1, total_tiles = 0;
};
bool resblock_pair_supported(int C, int k, int dil);
int resblock_pair_tile_rows(int k);  // output rows a workgroup owns
void launch_resblock_pair(const ResPairArgs& a, hipStream_t s);

// k_resblock.hip: the three ResBlocks (kernel sizes k[0..2], three dilation pairs each) of a narrow stage and their
// average, out = (RB_0(x) + RB_1(x) + RB_2(x)) / 3, in one kernel for C in {16, 32}: bit-identical to nine
// launch_resblock_pair calls (the last one averaging).  Pair q = 3 * block + pair-in-block.
struct MrfArgs {
    const float* x = nullptr;  // [nb][T][C]
    float* out = nullptr;      // [nb][T][C], not x
    int nb = 0, T = 0, C = 0;
    float slope = 0.1f;
    int halo = 0;              // filled by the launcher: rows of context per side
    int k[3] = {0, 0, 0};
    int dil[9] = {1, 1, 1, 1, 1, 1, 1, 1, 1};
    const __half* w1[9] = {};
    const __half* w2[9] = {};
    int64_t ldw1[9] = {};
    int64_t ldw2[9] = {};
    const float* b1[9] = {};
    const float* b2[9] = {};
    int single = 0;  // the hi fp16 plane of the activations only: one matrix instruction per fragment, no lo plane in LDS (the vocoder's default)
    // packed items (see GemmArgs::item_off): nb items, item i holds the rows [item_off[i] * item_mul, item_off[i + 1] * item_mul)
    // of x / out (T: the mean item length, for the profiler's figures only); a workgroup owns a tile of ONE item, tiles counted from the item's first row, and
    // tile_first[i] (nb + 1 entries, resblock_tile_first / mrf_tile_first) is the first workgroup of item i
    const int* item_off = nullptr;
    const int* tile_first = nullptr;
    int item_mul = 1, total_tiles = 0;
};
bool mrf_fused_supported(int C, const int* k, const int* dil);
int mrf_tile_rows(const int* k, const int* dil);  // output rows a workgroup owns
void launch_mrf_fused(const MrfArgs& a, hipStream_t s);

// out[m][n] = alpha*act(sum_k x[m][k]*W[n][k] + bias[n]) + res[m][n], exact fp32 FMA, M <= 8.
void launch_gemv(const float* x, int64_t ldx, const __half* W, int64_t ldw, const float* bias,
                 const float* res, int64_t ldr, float* out, int64_t ldo, int M, int N, int K,
                 int act, float alpha, hipStream_t s);

// The greedy step rules of a fused vocabulary projection (k_skinny.hip, k_dstep.hip EPI_ARGMAX, k_dstep3.hip vocab3), one
// record for the three kernel families: no logits go to HBM; per (workgroup, row) one record {best tweaked logit, its index,
// max, sumexp} goes to part[tile][M] and the raw EOS logit to eos_logit[M]; launch_argmax_finalize combines them.  The
// device side of the rules is argmax_push / argmax_merge (device_util.h).
struct ArgmaxEpi {
    float4* part = nullptr;
    int tiles_cap = 0;  // capacity of part in tiles
    float* eos_logit = nullptr;
    const int* pos = nullptr;
    int min_step_for_eos = 0, force_eos_step = -1;
    int pad_idx = -1, eos_idx = -1, unk_idx = -1;
    float unk_penalty = 0.f;
};

// Skinny product for 1..64 rows (decoder step), see k_skinny.hip.  With partial != nullptr the
// kernel writes raw K-range partial sums to partial[split][M][N] (no epilogue); otherwise
// C = alpha*act(A.W^T + bias) + res.
struct SkinnyArgs {
    const float* A = nullptr;
    int64_t lda = 0;
    const __half* W = nullptr;
    int64_t ldw = 0;
    const float* bias = nullptr;
    const float* res = nullptr;
    int64_t ldr = 0;
    float* C = nullptr;
    int64_t ldc = 0;
    float* partial = nullptr;
    int M = 0, N = 0, K = 0;
    int act = ACT_NONE;
    float alpha = 1.0f;
    int splits = 1;
    int kc = 0;  // filled by the launcher
    ArgmaxEpi am;      // fused arg-max epilogue: with am.part != nullptr no logits are written
    int am_tiles = 0;  // filled by the launcher: tiles written
};
// number of am.part tiles launch_skinny will write for N output features and M rows
int skinny_argmax_tiles(int M, int N);
// combines the `tiles` records per row that a projection wrote under `am` and does the step's bookkeeping for the nb rows
void launch_argmax_finalize(const ArgmaxEpi& am, int tiles, int nb, int* next_tok, int* hist, int hist_ld, int* finished,
                            int* out_len, float* score, hipStream_t s, const int* prompt_len = nullptr);
void launch_skinny(const SkinnyArgs& a, hipStream_t s);
// number of K ranges that brings the grid to >= 256 workgroups (1 when want_split == 0)
int skinny_splits(int M, int N, int K, int want_split);
// x[row] += bias + sum_s partial[s][row]; h[row] = LayerNorm(x[row]) (h may be null)
void launch_reduce_res_ln(const float* partial, int splits, const float* bias, float* x, const float* gamma,
                          const float* beta, float* h, int rows, int C, hipStream_t s);

// ---- decoder step, second generation (k_dstep.hip) ---------------------------------------------------------------
// Weights packed at load into MFMA fragment order Wp[ceil(N/32)][K/16][64 lanes][8] (rows >= N zero); activations as
// two fp16 planes (hi, lo) in k-group-major order P[K/8][RB][8], RB = 32 or 64 row slots.
int64_t packed_weight_halfs(int N, int K);
void launch_pack_weight(const __half* w, int64_t ldw, int N, int K, __half* dst, hipStream_t s);
enum GemvEpilogue {
    EPI_PARTIAL = 0,  // raw K-range partial sums -> partial[split][M][N] (no bias)
    EPI_PLANES = 1,   // act(sum + bias) as split planes Oh / Ol [N/8][ORB][8] (whole K in one workgroup)
    EPI_ARGMAX = 2,   // vocabulary projection: per (workgroup, row) arg-max / log-sum-exp record, no logits in HBM
};
struct GemvPArgs {
    const __half* Wp = nullptr;
    const __half* Ah = nullptr;  // activation planes [K/8][RB][8]
    const __half* Al = nullptr;
    int RB = 32;
    int M = 0, N = 0, K = 0;
    int splits = 1;  // in: wanted K ranges; the launcher rounds it to what the tiling allows (gemvp_splits)
    int ntl = 1;     // consecutive 32-feature tiles per workgroup (EPI_ARGMAX: records per row = ceil(N/32/ntl))
    int epi = EPI_PARTIAL;
    float* partial = nullptr;
    const float* bias = nullptr;
    int act = ACT_NONE;
    __half* Oh = nullptr;
    __half* Ol = nullptr;
    int ORB = 32;
    ArgmaxEpi am;  // EPI_ARGMAX
    // filled by the launcher
    int KS = 0, NT = 0, ks_per_wg = 0;
    uint32_t w_bytes = 0, a_bytes = 0;
    const int* d_rows = nullptr;  // rows behind *d_rows are neither read nor written (see Gemv3Args::d_rows)
};
bool gemvp_supported(int M, int N, int K);
int gemvp_splits(int K, int want_splits);  // K ranges launch_gemvp will really use
int gemvp_argmax_tiles(int N, int ntl);
void launch_gemvp(const GemvPArgs& a, hipStream_t s);
// x[row] += bias + sum_s partial[s][row]; h = LayerNorm(x[row]) -> planes Hh / Hl (nullable) and / or the fp32 row
// hrow + row * hrow_bs + *d_pos * C when *d_pos < hrow_rows (nullable): the captured decoder output; hfix (nullable):
// h as plain fp32 rows [rows][C]
void launch_reduce_ln(const float* partial, int S, const float* bias, float* x, const float* gamma, const float* beta, __half* Hh,
                      __half* Hl, int RB, float* hrow, int64_t hrow_bs, int hrow_rows, const int* d_pos, int rows, int C,
                      hipStream_t s, float* hfix = nullptr);
// x[row] = embed[tok[row]] * scale + pos_table[*d_pos]; h = LayerNorm(x[row]) -> planes
void launch_embed_ln(const int* tok, const __half* embed, float scale, const float* pos_table, const int* d_pos, float* x,
                     const float* gamma, const float* beta, __half* Hh, __half* Hl, int RB, int rows, int C, hipStream_t s);
struct DAttnArgs {
    const float* q = nullptr;  // projection partials: element (s, b, col) at q[s * sstride + b * ldq + col]
    int64_t ldq = 0, sstride = 0;
    int S = 1;
    int koff = 0, voff = 0;      // self-attention: columns of the new key / value row inside the fused projection
    const float* bias = nullptr; // bias of the fused projection (same column layout), nullable
    float* kcache = nullptr;     // key row j of (b, head) at kcache + b * cache_bs + j * cache_ld + head * 64
    float* vcache = nullptr;
    int64_t cache_ld = 0, cache_bs = 0;
    int cap = 0;
    const int* d_pos = nullptr;    // self: position of the new row, kv_len = *d_pos + 1
    const int* kv_lens = nullptr;  // cross: valid keys per batch row
    int kv_row_div = 1;            // cross: batch row b reads cache row b / kv_row_div (the beams of an utterance share its K / V)
    // self (beam search): anc[b * cap + j] = cache row that holds key / value j of batch row b.  Beams that continue another
    // beam inherit its history through this table instead of having their cache rows copied (k_beam.hip: beam_select_kernel
    // re-orders the table); a row always appends at its own cache row.  null: row b reads its own cache row.
    const int* anc = nullptr;
    const int* kv_item = nullptr;  // cross (beam search): row b reads the encoder K / V of item kv_item[b / kv_row_div] (null: b / kv_row_div)
    const int* d_rows = nullptr;   // see Gemv3Args::d_rows: (row, head) pairs of rows behind *d_rows return at once
    // decode engine (engine.hip): slot b works on row state slot_rp[b].x at position slot_rp[b].y (d_pos unused): the K / V
    // cache rows, the encoder K / V rows and kv_lens are indexed by the row state, q and the output planes by the slot
    const int2* slot_rp = nullptr;
    // decode engine, self-attention: the K / V cache rows belong to the LANE slot b's row holds while it is in the chain
    // (slot_lane[b]; handed out on admission, returned at retirement), not to the row state: the caches are [slots][cap][M]
    // whatever the number of row states.  null: the cache row is the row state.
    const int* slot_lane = nullptr;
    __half* Oh = nullptr;          // output planes [heads*8][ORB][8]
    __half* Ol = nullptr;
    int ORB = 32;
    int nb = 0, heads = 0;
};
void launch_dattn(const DAttnArgs& a, bool cross, hipStream_t s);
void launch_planes_to_rows(const __half* Hh, const __half* Hl, int RB, float* out, int64_t ldo, int rows, int C, hipStream_t s);
void launch_rows_to_planes(const float* x, int64_t ldx, int rows, int C, int RB, __half* Hh, __half* Hl, hipStream_t s);

// ---- decoder step, third generation (k_dstep3.hip) ----------------------------------------------------------------
// Row-group GEMV: a workgroup owns 32 output features x a group of <= 32 (64) batch rows x the whole K range (or a
// 1024-wide K slice), applies the LayerNorm in front of the product itself (IN3_LN: input = the fp32 residual stream in
// k-group-major order X[K/8][RB][8]) and finishes the output itself (bias, residual, ReLU + split planes).
enum In3 { IN3_PLANES = 0, IN3_LN = 1 };
enum Epi3 {
    EPI3_ROWS = 0,     // out[row * ldo + feature] = product + bias                    (q / k / v rows)
    EPI3_RESID = 1,    // xres (k-group-major fp32 [N/8][XRB][8]) += product + bias    (out-projections)
    EPI3_PLANES = 2,   // act(product + bias) as split fp16 planes [N/8][ORB][8]       (FFN inner activation)
    EPI3_PARTIAL = 3,  // out[(split * M + row) * N + feature] = partial product       (K > 1024: FFN-out)
};
struct Gemv3Args {
    const __half* Wp = nullptr;  // packed fragments (launch_pack_weight)
    int M = 0, N = 0, K = 0;
    int in_mode = IN3_PLANES;
    const float* xg = nullptr;  // IN3_LN: residual stream, k-group-major fp32 [K/8][RB][8]
    const float* gamma = nullptr;
    const float* beta = nullptr;
    const __half* Ah = nullptr;  // IN3_PLANES: activation planes [K/8][RB][8]
    const __half* Al = nullptr;
    int RB = 32;   // row slots of the input buffers
    int rg = 0;    // rows per row group (<= 32; <= 64 with mt2); 0 = as many as the shape allows
    int mt2 = 0;   // 33..64 rows as ONE row group (two MFMA row tiles per workgroup)
    int stationary = -1;  // FFN-in / FFN-out shapes over several row groups: -1 the launcher decides, 0 one workgroup per row group,
                          // k >= 1 weights stationary with k workgroups per tile walking the row groups (same bits; tests)
    int shape = 0; // G3_T1 / G3_T2K8 / G3_T2K4: tiles per workgroup x waves x k-steps per wave (k_dstep3.hip)
    int epi = EPI3_ROWS;
    const float* bias = nullptr;
    float* out = nullptr;
    int64_t ldo = 0;
    float* xres = nullptr;
    int XRB = 32;
    __half* Oh = nullptr;
    __half* Ol = nullptr;
    int ORB = 32;
    int act = ACT_NONE;  // EPI3_PLANES: ACT_NONE, ACT_RELU, or ACT_GELU (IN3_LN only: a kernel variant of its own)
    // beam search: *d_rows = live rows (the rows of utterances still searching, packed to the front); row groups that start
    // behind it return at once.  null: all M rows.
    const int* d_rows = nullptr;
    // filled by the launcher
    int KS = 0, NT_total = 0;
    uint32_t w_bytes = 0, a_bytes = 0;
    int xcd_swizzle = 0, touch = 0;  // gemv3s_kernel: K slices dealt out per XCD; cooperative L2 touch of the activations
};
enum Gemv3Shape { G3_T1 = 0, G3_T2K8 = 1, G3_T2K4 = 2 };
bool gemv3_supported(int M, int N, int K, int in_mode);
int gemv3_splits(int K, int shape);  // K ranges (EPI3_PARTIAL slabs) launch_gemv3 uses for this K and workgroup shape
void launch_gemv3(const Gemv3Args& a, hipStream_t s);
// x[row] += bias + sum_s partial[s][row] on the k-group-major residual stream; gamma != null: h = LayerNorm(x[row]) ->
// planes Hh / Hl, fp32 rows hfix [rows][C], captured rows hrow (see launch_reduce_ln)
struct Reduce3Args {
    const float* partial = nullptr;  // [S][rows][C]
    int S = 0;
    const float* bias = nullptr;
    float* xg = nullptr;
    int XRB = 32;
    const float* gamma = nullptr;
    const float* beta = nullptr;
    __half* Hh = nullptr;
    __half* Hl = nullptr;
    int RB = 32;
    float* hrow = nullptr;
    int64_t hrow_bs = 0;
    int hrow_rows = 0;
    const int* d_pos = nullptr;
    float* hfix = nullptr;
    int rows = 0, C = 0;
    const int* d_rows = nullptr;  // see Gemv3Args::d_rows
    const int2* slot_rp = nullptr;  // decode engine: the captured row of slot s goes to hrow[slot_rp[s].x] at position slot_rp[s].y
};
void launch_reduce3(const Reduce3Args& a, hipStream_t s);
// slot_rp != null (decode engine): slot s embeds tok[slot_rp[s].x] at position slot_rp[s].y; slots behind *d_rows are skipped
void launch_embed3(const int* tok, const __half* embed, float scale, const float* pos_table, const int* d_pos, float* xg, int XRB,
                   int rows, int C, hipStream_t s, const int2* slot_rp = nullptr, const int* d_rows = nullptr);
void launch_ln3(const float* xg, int XRB, const float* gamma, const float* beta, __half* Hh, __half* Hl, int RB, int rows, int C,
                hipStream_t s);
void launch_rows_to_kgm(const float* x, int64_t ldx, int rows, int C, int XRB, float* xg, hipStream_t s);
void launch_kgm_to_rows(const float* xg, int XRB, float* out, int64_t ldo, int rows, int C, hipStream_t s);
// vocabulary projection with the generation rules fused (record format of GemvPArgs' EPI_ARGMAX)
struct Vocab3Args {
    const __half* Wp = nullptr;
    const __half* Ah = nullptr;
    const __half* Al = nullptr;
    int RB = 32;
    int M = 0, N = 0, K = 0;
    const float* bias = nullptr;
    float* logits = nullptr;    // != null: raw logits [M][ldl] fp32 go to HBM and the fused rules are skipped (beam search)
    int64_t ldl = 0;
    ArgmaxEpi am;  // part is [vocab3_groups(M)][M]
    const int* d_rows = nullptr;  // see Gemv3Args::d_rows
    // decode engine: the step rules of slot m are those of row state slot_rp[m].x at position slot_rp[m].y (am.pos unused),
    // forced EOS at position limit_row[row state] - 2 (am.force_eos_step unused)
    const int2* slot_rp = nullptr;
    const int* limit_row = nullptr;
    // filled by the launcher
    int KS = 0, NT_total = 0, tpg = 0, halves = 1;
    uint32_t w_bytes = 0;
};
bool vocab3_supported(int M, int N, int K);
int vocab3_groups(int M);
void launch_vocab3(const Vocab3Args& a, hipStream_t s);

// y = act(LayerNorm(x) * gamma + beta); rows masked to zero when t >= lens[n] (optional).
void launch_layernorm(const float* x, int64_t ldx, const float* gamma, const float* beta, float* y,
                      int64_t ldy, int rows, int C, int act, const int* lens, int t_per_batch,
                      hipStream_t s);

// same, result written as two fp16 planes hi = fp16(y), lo = fp16(y - hi) (the A operand of launch_gemm_presplit)
void launch_layernorm_split(const float* x, int64_t ldx, const float* gamma, const float* beta, __half* yh, __half* yl,
                            int64_t ldh, int rows, int C, int act, const int* lens, int t_per_batch, hipStream_t s);
// y = LN_a(x) as fp32 rows (may alias x) and the split planes of LN_b(y) in one pass (C <= 1024): bit-identical to
// launch_layernorm followed by launch_layernorm_split
void launch_layernorm2_split(const float* x, int64_t ldx, const float* ga, const float* ba, float* y, int64_t ldy, const float* gb2,
                             const float* bb2, __half* yh, __half* yl, int64_t ldh, int rows, int C, hipStream_t s);
// fp32 rows AND planes in one pass; the length mask zeroes the planes only
void launch_layernorm_both(const float* x, int64_t ldx, const float* gamma, const float* beta, float* y, int64_t ldy, __half* yh,
                           __half* yl, int64_t ldh, int rows, int C, int act, const int* lens, int t_per_batch, hipStream_t s);
// the same of max(x, 0) + neg_slope * min(x, 0) (LeakyReLU): the first convolution of a HiFi-GAN ResBlock on the DMA GEMM
void launch_lrelu_split_f32(const float* x, float neg_slope, __half* hi, __half* lo, int64_t n, hipStream_t s);
// hi = fp16(x), lo = fp16(x - hi), elementwise over n values (n % 4 == 0)
void launch_split_f32(const float* x, __half* hi, __half* lo, int64_t n, hipStream_t s);

// y[r][c] = x[r][c] * sigmoid(x[r][C + c])
void launch_glu(const float* x, int64_t ldx, float* y, int64_t ldy, int rows, int C, hipStream_t s);

// The same followed by LayerNorm over the channels + activation, written as split planes, in one pass (k = 31, C % 64 == 0,
// C <= 1024): bit-identical to launch_glu_dwconv + launch_layernorm_split
// gated: x is [rows][C] and already holds GLU(.) (launch_gemm_presplit_glu wrote it); the same bits from half the input bytes
bool glu_dwconv_ln_supported(int C, int ksize);
void launch_glu_dwconv_ln(const float* x, int64_t ldx, const float* w, const float* gamma, const float* beta, int act, __half* yh,
                          __half* yl, int64_t ldh, int nb, int T, int C, int ksize, const int* lens, hipStream_t s, bool gated = false);
// The same on PACKED rows (the ragged speech encoder): item i owns rows row_off[i] .. row_off[i] + lens[i] of x / yh / yl, nothing
// in between; an item's rows carry the bits launch_glu_dwconv_ln gives them when the item runs alone (T = its length), whatever
// its neighbours hold.  glu_dwconv_ln_packed_work builds the launch's work table on the host - int4 records {row_off, len,
// t_begin, t_end}, ranges of at least 32 rows in multiples of 8, about 256 workgroups over the whole batch - and d_work is its
// copy on the device (16-byte aligned, n_work = work.size() / 4 records); rows = sum of the lengths (profiler only).
void glu_dwconv_ln_packed_work(const int32_t* row_off, const int32_t* lens, int n, std::vector<int32_t>& work);
void launch_glu_dwconv_ln_packed(const float* x, int64_t ldx, const float* w, const float* gamma, const float* beta, int act, __half* yh,
                                 __half* yl, int64_t ldh, const int* d_work, int n_work, double rows, int C, int ksize, hipStream_t s,
                                 bool gated = false);
// Conformer conv middle: g = GLU(x) (masked by lens), y = causal depthwise conv_k(g)
void launch_glu_dwconv(const float* x, int64_t ldx, const float* w, float* y, int64_t ldy, int nb, int T,
                       int C, int ksize, const int* lens, hipStream_t s, int left = -1, const float* bn_scale = nullptr,
                       const float* bn_shift = nullptr);
// v1 speech encoder helpers (k_norm.hip): BatchNorm1d (inference) folded to scale / shift; relative position table
void launch_bn_fold(const float* g, const float* b, const float* mean, const float* var, float eps, int C, float* scale, float* shift,
                    hipStream_t s);
void launch_relpos_table(int S, int M, float* out, hipStream_t s);

struct AttnArgs {
    const float* q = nullptr;  // [nb*Sq rows][ldq], head h at column h*64
    const float* k = nullptr;
    const float* v = nullptr;
    float* out = nullptr;
    int64_t ldq = 0, ldk = 0, ldv = 0, ldo = 0;
    int nb = 0, heads = 0, Sq = 0, Skv = 0;
    const int* kv_lens = nullptr;  // per batch item valid keys (nullable)
    int causal = 0;                // key j visible iff j <= i + (Skv - Sq)
    const float* rel_k = nullptr;  // Shaw relative keys [left+1+right][64] (nullable)
    int rel_left = 0, rel_right = 0;
    // Transformer-XL relative positions of the v1 speech encoder (fairseq2 RelativePositionSDPA, fairseq2.cpp:605-696; self-
    // attention only): logits[i][j] = ((q_i + u).k_j + (q_i + v).r_{i-j}) / 8.  rp_table = r_proj(position table), fp32
    // [2*Skv-1][rp_ld], row t = relative position (Skv-1) - t, head h at column h*64; q_bias_u / q_bias_v fp32 [heads*64]
    const float* rp_table = nullptr;
    int64_t rp_ld = 0;
    const float* q_bias_u = nullptr;
    const float* q_bias_v = nullptr;
    // packed (varlen) self-attention: item n owns rows row_off[n] .. row_off[n] + kv_lens[n] of q / k / v / out (no padding
    // rows between items); Sq = Skv = the longest item (grid size only).  Needs kv_lens.
    const int* row_off = nullptr;
    double pairs = 0;  // profiler only: sum over items of (queries x keys) really computed (0: nb * Sq * Skv)
    // optional: write the result as two fp16 planes (hi, lo) for launch_gemm_presplit instead of `out`
    __half* out_hi = nullptr;
    __half* out_lo = nullptr;
    int64_t ldoh = 0;
    // 64: the kernel of k_attn.hip (every mode above).  80 and 128: the kernel template of k_attn_hd.hip.  80 (wav2vec 2.0 /
    // XLS-R): plain mode with kv_lens only, head h at column h*80, logits scaled by 80^-0.5.  128 (PRETSSEL): kv_lens, packed
    // rows and plane output, head h at column h*128, logits scaled by 128^-0.5
    int head_dim = 64;
};
void launch_attention(const AttnArgs& a, hipStream_t s);
void launch_attention_hd(const AttnArgs& a, hipStream_t s);  // k_attn_hd.hip (head_dim 80 and 128); reached through launch_attention

// Single-query attention over a KV cache (decoder step).  q: [nb][heads*64];
// key/value row j of (b, h) lives at base + b*cache_bs + j*cache_ld + h*64.  If k_new != null the
// new key/value rows are appended at position *d_pos first.  kv_len = use_lens ? lens[b] : *d_pos + 1.
void launch_decode_attention(const float* q, int64_t ldq, const float* k_new, const float* v_new,
                             int64_t ldkv, float* kcache, float* vcache, int64_t cache_ld, int64_t cache_bs,
                             int cap, float* out, int64_t ldo, int nb, int heads, const int* d_pos,
                             const int* kv_lens, int use_lens, hipStream_t s, int in_splits = 1,
                             int64_t in_split_stride = 0, const float* bias_q = nullptr,
                             const float* bias_k = nullptr, const float* bias_v = nullptr);

// beam search (k_beam.hip)
// Banned token sequences of a call (BannedSequenceProcessor), CSR in device memory: sequence q = tokens[offsets[q] ..
// offsets[q+1]).  Limits (validate_banned_host; SC_ERR_INVALID): at most BANNED_MAX_SEQS sequences of 1..BANNED_MAX_LEN tokens,
// BANNED_MAX_TOKENS in all, every token inside the vocabulary.
constexpr int BANNED_MAX_SEQS = 4096, BANNED_MAX_LEN = 64, BANNED_MAX_TOKENS = 65536;
struct BannedList {
    const int* tokens = nullptr;
    const int* offsets = nullptr;  // [n + 1]
    int n = 0;
    int max_len = 0;  // longest sequence
};
void validate_banned_host(const int32_t* tokens, const int32_t* offsets, int n_banned, int V, int* out_max_len);
// Boost phrases of a call (PhraseBoostProcessor; the rule and the limits: boost_list.h), CSR in device memory, the phrases in
// lexicographic order and prefix-free (boost_list_build made the list).  The row's logit of token t moves by beta * k(y, t).
struct BoostList {
    const int* tokens = nullptr;
    const int* offsets = nullptr;  // [n + 1]
    int n = 0;
    int max_len = 0;  // longest phrase
    float beta = 0.f;
};
// Per-utterance prompts of a beam search (sc_generate_text_prompts).  len == null: every utterance's prompt ended before the
// search's first step (the launch's first_step flag says whether this is that step).  Otherwise len[utterance] is its prompt
// length (the utterance of slot u is slot_utt[u], or u), `step` the search step, and at a step with
//   step + 1 <  len: the utterance is still inside its prompt - the candidate search and the step processors leave its rows
//                    and its candidate list alone (launch_beam_prompt wrote the list);
//   step + 1 == len: this is the utterance's first free step: beam 0 only (its beams are copies of each other).
struct BeamPrompt {
    const int* len = nullptr;
    const int* slot_utt = nullptr;
    int step = 0;
};
// The forced step of the utterances still inside their prompt: candidate i < beams of such an utterance is (beam i, the token
// seqs already holds at position step + 1), valued cum[beam i] + that token's raw log-probability in beam 0's logit row - the
// value launch_row_tokens_lprob gives (same reductions), so the cumulative score gets the bits of the host's prompt echo;
// beam_select_kernel then continues every beam with itself.  Launched BEFORE the candidate search of the step (the step
// processors write into the logit rows).  One workgroup per slot; other utterances' lists are not touched.
void launch_beam_prompt(const float* logits, int64_t ld, int n_utt, int beams, int V, const float* cum, const int* seqs, int seq_ld, int K,
                        float* cand_val, int* cand_idx, const BeamPrompt& bp, const int* d_slots, hipStream_t s);
// seqs [n_utt*beams][seq_ld] (nullable): the rows' sequences so far (S tokens) for the n-gram step processor (G = n-gram
// size, 0 = off); logits is modified (blocked tokens).  banned (nullable): the call's banned-sequence list, applied to the same
// rows when seqs is given (another kernel then: beam_candidates_banned_kernel / one step_processors_kernel launch for both rules).
// boost (nullable): the call's phrase list, applied after the other two (beam_candidates_boost_kernel / step_processors_boost_kernel)
void launch_beam_candidates(float* logits, int64_t ld, int n_utt, int beams, int V, const float* cum, int first_step,
                            int no_eos, int force_eos, int pad_idx, int eos_idx, int unk_idx, float unk_penalty, int K,
                            float* cand_val, int* cand_idx, const int* seqs, int seq_ld, int S, int G, hipStream_t s,
                            const int* d_slots = nullptr, const BannedList* banned = nullptr, const BoostList* boost = nullptr,
                            const BeamPrompt& bp = BeamPrompt{});
// the same search for large vocabularies: every (row, 1/32 of V) on its own workgroup, then a merge per utterance;
// ws_f / ws_i: workspaces of beam_ws_floats / beam_ws_ints elements
bool beam_chunked(int V, int beams, int K);
size_t beam_ws_floats(int rows, int K);
size_t beam_ws_ints(int rows, int K);
void launch_beam_candidates_chunked(float* logits, int64_t ld, int n_utt, int beams, int V, const float* cum, int first_step, int no_eos,
                                    int force_eos, int pad_idx, int eos_idx, int unk_idx, float unk_penalty, int K, float* cand_val,
                                    int* cand_idx, const int* seqs, int seq_ld, int S, int G, float* ws_f, int* ws_i, hipStream_t s,
                                    const int* d_rows = nullptr, const int* d_slots = nullptr, const BannedList* banned = nullptr,
                                    const BoostList* boost = nullptr, const BeamPrompt& bp = BeamPrompt{});
// device-resident beam-search state of one sc_generate_text call (k_beam.hip: beam_select_kernel)
struct BeamSelectArgs {
    const float* cand_val = nullptr;  // [n][K] best first
    const int* cand_idx = nullptr;    // [n][K] flattened beam * V + token
    const int* seqs_cur = nullptr;    // [n*beams][max_len]
    int* seqs_new = nullptr;
    float* fin_score = nullptr;  // [n][beams]
    int* fin_len = nullptr;      // [n][beams]
    int* fin_seq = nullptr;      // [n][beams][max_len]
    int* fin_count = nullptr;    // [n]
    int* done = nullptr;         // [n]
    int* remaining = nullptr;    // [1] utterances still searching
    int* tok = nullptr;          // [n*beams] token fed at the next step
    int* src_row = nullptr;      // [n*beams] row whose K/V cache the beam continues
    float* cum = nullptr;        // [n*beams] cumulative scores
    int* anc = nullptr;          // [n*beams][anc_ld] ancestor table of the K/V caches (DAttnArgs::anc), re-ordered in place; nullable
    int anc_ld = 0;
    // live-slot bookkeeping (nullable): slot u of the candidate / sequence arrays holds utterance slot_utt[u]; fin_* / done /
    // fin_count are indexed by UTTERANCE; slots behind *d_slots are idle (their utterances finished) and are skipped
    const int* slot_utt = nullptr;
    const int* d_slots = nullptr;
    int beams = 0, K = 0, V = 0, max_len = 0, step = 0;
    int eos_idx = 0, pad_idx = 0, normalize = 1;
    float len_penalty = 1.f;
};
// Score history of a beam search (sc_generate_text_nbest only; its own argument block, so that the kernel of every other call
// keeps its arguments and its code): hist[r][t] = cumulative score of row r's hypothesis after position t, moved exactly as the
// sequence rows are - the parent's row, then the candidate's score at step + 1; a finished hypothesis keeps its parent's
// history and the RAW (un-normalised) score of its EOS candidate at step + 1, 0 behind it.
struct BeamHistArgs {
    const float* cur = nullptr;  // [n*beams][max_len]
    float* next = nullptr;       // [n*beams][max_len]
    float* fin = nullptr;        // [n][beams][max_len]
};
// hist == null: beam_select_kernel<false>, the kernel without it; otherwise beam_select_kernel<true> (the same walk, the history moved with the sequences)
void launch_beam_select(const BeamSelectArgs& a, int n_utt, hipStream_t s, const BeamHistArgs* hist = nullptr);
// Packs the slots of utterances that are still searching to the front (stable), in place: per-row sequences, cumulative
// scores, next tokens, encoder lengths and K/V ancestor rows move with their slot; slot_utt follows; *d_slots / *d_rows = the
// new counts.  One workgroup (the arrays are a few hundred KB).  K/V cache rows do not move: the ancestor table names them.
struct BeamCompactArgs {
    const int* done = nullptr;  // [n] by utterance
    int* slot_utt = nullptr;    // [n]
    int* d_slots = nullptr;
    int* d_rows = nullptr;
    int* seqs = nullptr;        // [n*beams][max_len]
    float* cum = nullptr;       // [n*beams]
    int* tok = nullptr;         // [n*beams]
    int* enc_lens = nullptr;    // [n*beams]
    int* anc = nullptr;         // [n*beams][anc_ld]
    int n = 0, beams = 0, max_len = 0, anc_ld = 0;
    int seq_len = 0, anc_len = 0;  // sequence positions / table positions in use
};
// hist (nullable): the live rows' score history [n*beams][max_len] (BeamHistArgs), moved like seqs (beam_compact_kernel<true>)
void launch_beam_compact(const BeamCompactArgs& a, hipStream_t s, float* hist = nullptr);
// The n-best list of a finished beam search (sc_generate_text_nbest), one workgroup per utterance: the utterance's fin_count
// finished hypotheses ranked in the order the host picks the winner in (order_key: NaN first, then the higher score, ties to the
// earlier finish slot), the first `nbest` packed into the outputs.  out_step[t] = hist[t] - hist[t-1] (one fp32 subtraction,
// fairseq2.cpp:1333-1341), out_step[0] = 0.  Behind a hypothesis' length: pad / 0; rows behind out_counts[u]: pad, length 0, score 0.
struct BeamNbestArgs {
    const int* fin_seq = nullptr;      // [n][beams][max_len]
    const int* fin_len = nullptr;      // [n][beams]
    const float* fin_score = nullptr;  // [n][beams]
    const float* fin_hist = nullptr;   // [n][beams][max_len]
    const int* fin_count = nullptr;    // [n]
    int* out_ids = nullptr;            // [n][nbest][max_len]
    int* out_lens = nullptr;           // [n][nbest]
    float* out_scores = nullptr;       // [n][nbest]
    int* out_counts = nullptr;         // [n] = min(fin_count, nbest)
    float* out_step = nullptr;         // [n][nbest][max_len]
    int n = 0, beams = 0, nbest = 0, max_len = 0, pad_idx = 0;
};
void launch_beam_nbest(const BeamNbestArgs& a, hipStream_t s);
void launch_row_token_lprob(const float* logits, int64_t ld, int rows, int V, int row_stride, int token, float* out, hipStream_t s);
// the per-row-token form: output i is the log-softmax value of row_tokens[i * row_stride] (a device array with one token per
// logit row, e.g. StepCtx::d_tok; the caller has checked the tokens against V) in logit row i * row_stride
void launch_row_tokens_lprob(const float* logits, int64_t ld, int rows, int V, int row_stride, const int* row_tokens, float* out, hipStream_t s);
void launch_gather_cache(const float* src, float* dst, const int* src_row, int rows, int len, int cap, int M, int layers,
                         int64_t layer_stride, hipStream_t s);

// sampled generation (k_sample.hip): one top-k / top-p draw per live logit row, one workgroup per row.  The draw
// is a pure function of (row, options, seed, stream, gen, position): integer masses floor(exp(v) * 2^36), Philox4x32-10.
struct SampleArgs {
    float* logits = nullptr;  // [rows][ld]; the step processors write -inf into it
    int64_t ld = 0;
    int rows = 0, V = 0;
    const unsigned long long* stream = nullptr;  // [rows] the utterance's 64-bit id
    const int* gen = nullptr;                    // [rows] hypothesis number
    const int* position = nullptr;               // [rows] index the drawn token will occupy; null: `pos` for every row
    int pos = 0;
    float temperature = 1.f, top_p = 1.f;
    int top_k = 0;
    unsigned long long seed = 0;
    int no_eos = 0, force_eos = 0, pad_idx = 0, eos_idx = 0, unk_idx = 0;
    float unk_penalty = 0.f;
    // step processors (seqs nullable = none): S tokens so far per row, n-gram size G (0 = off), banned list (n == 0: none)
    const int* seqs_in = nullptr;
    int seq_ld = 0, S = 0, G = 0;
    BannedList banned;
    // results per row (each nullable)
    int* tok = nullptr;
    float* lprob = nullptr;
    int* kept = nullptr;
    unsigned long long* z_kept = nullptr;
    // loop state (run_generate_sampled; all nullable together): a finished row is skipped; otherwise the token is appended to
    // seqs[r][pos], fed next (next_tok), cum += lprob, step_lprob[r][pos] = lprob, and EOS finishes the row (out_len = pos + 1,
    // *remaining -= 1)
    int* seqs = nullptr;        // [rows][seq_ld]
    int* next_tok = nullptr;    // [rows]
    float* cum = nullptr;       // [rows]
    float* step_lprob = nullptr;  // [rows][seq_ld]
    int* finished = nullptr;    // [rows]
    int* out_len = nullptr;     // [rows]
    int* remaining = nullptr;   // [1]
};
void launch_sample_rows(const SampleArgs& a, hipStream_t s);
// out[i] += y[token] - lse(y) with y = logits[i * row_stride] / temperature (the echoed prompt's score under the sampler's temperature)
void launch_sample_prompt_lprob(const float* logits, int64_t ld, int rows, int V, int row_stride, int token, float temperature, float* out,
                                hipStream_t s);

// fbank front-end
// consts = window[400] | melT[256][80] | twiddle cos[256] | twiddle sin[256]
void launch_fbank(const float* wav, int64_t wav_stride, const int* num_samples, int nb, float* out,
                  int t_rows /*rows per item in out*/, const float* consts, float scale, hipStream_t s);
// any sample rate (k_fbank.hip: fbank_any_kernel): consts = window[frame_len] | melT[nfft/2][80] | cos[nfft/2] | sin[nfft/2]
void launch_fbank_any(const float* wav, int64_t wav_stride, const int* num_samples, int nb, float* out, int t_rows, const float* consts,
                      float scale, int frame_len, int frame_shift, int nfft, hipStream_t s);
void launch_standardize(float* feat, int nb, int t_rows, const int* num_frames, int C, hipStream_t s);

// misc elementwise / gather kernels (k_misc.hip)
// out[row] = emb[tok[row]]*scale + pos_table[(d_pos ? *d_pos : 0) + (t_per_batch>0 ? row%t_per_batch : 0)]
void launch_embed_tokens(const int* tokens, int rows, const __half* emb, int M, float scale,
                         const float* pos_table, const int* d_pos, int t_per_batch, float* out,
                         int64_t ldo, hipStream_t s);
void launch_step_update(int* next_tok, int* hist, int hist_ld, int* finished, int* out_len,
                        const float* lprob, float* score, int nb, const int* d_pos, int pad_idx,
                        int eos_idx, int* n_unfinished, hipStream_t s, const int* prompt_len = nullptr);
void launch_argmax_rows(const float* logits, int64_t ld, int rows, int V, const int* d_pos,
                        int min_pos_for_eos, int force_eos_pos, int pad_idx, int eos_idx, int unk_idx,
                        float unk_penalty, int* out_idx, float* out_lprob, hipStream_t s);
void launch_cvt_f16_f32(const __half* src, float* dst, int64_t n, hipStream_t s);
void launch_cvt_f32_f16(const float* src, __half* dst, int64_t n, hipStream_t s);
void launch_pack_conv_weight(const __half* w /*[Co][Ci][k]*/, __half* dst /*[Co][Kpad]*/, int Co,
                             int Ci, int k, int Kpad, hipStream_t s);
void launch_pack_convT_weight(const float* w /*[Ci][Co][k] folded*/, __half* dst /*[s][Co][Kpad]*/,
                              int Ci, int Co, int k, int stride, int Kpad, hipStream_t s);
void launch_weight_norm_fold(const __half* v, const __half* g, float* out, int d0, int inner,
                             hipStream_t s);
void launch_gather_rows(const float* src, int64_t lds, const int* row_idx /*-1 => zero*/, float* dst,
                        int64_t ldd, int rows, int C, hipStream_t s);
// dst[r] = src[row_idx[r]] + add[r / rows_per_item] (add rows ld_add apart, 16-byte aligned); row_idx < 0: zeros
void launch_gather_rows_add(const float* src, int64_t lds, const int* row_idx, const float* add, int64_t ld_add, int rows_per_item, float* dst,
                            int64_t ldd, int rows, int C, hipStream_t s);
void launch_char_embed_add(float* seqs /*in-place [rows][M]*/, int64_t ld, const int* char_ids,
                           const __half* embed_char, const float* pos_table, int t_per_batch,
                           float alpha, float scale, int rows, int M, hipStream_t s);
// same with the position of every row given (packed rows of items of different lengths)
void launch_pos_add_rows(float* seqs, int64_t ld, const float* pos_table, const int* row_t, float alpha, int rows, int M, hipStream_t s);
void launch_pos_add(float* seqs, int64_t ld, const float* pos_table, int t_per_batch, float alpha,
                    int rows, int M, hipStream_t s);
void launch_durations(const float* h /*[rows][H]*/, int64_t ld, const float* w, const float* b,
                      int rows, int H, int t_per_batch, const int* lens, float duration_factor,
                      int min_dur, int* durations, hipStream_t s);
// The duration rule with one factor per item, fitted on the device to a unit budget (k_dub.hip).  One
// workgroup per item b of n; rows are [n][s_char].
struct FitArgs {
    const float* h = nullptr;  // [n * s_char][ld] duration predictor features; null: e holds the values expf(x) - 1 already
    int64_t ld = 0;
    const float* w = nullptr;  // [H], b [1]: VariancePredictor.proj
    const float* b = nullptr;
    int H = 0;
    float* e = nullptr;           // [n][s_char] scratch row per item (written by stage 1, read by the search)
    int s_char = 0;
    const int* lens = nullptr;    // [n] characters per item
    const int* target = nullptr;  // [n] unit budget, 0: none
    const float* lo = nullptr;    // [n] 0 < lo <= hi
    const float* hi = nullptr;
    int min_dur = 1;
    int* durations = nullptr;     // [n][s_char], 0 behind an item's characters
    float* factor = nullptr;      // [n]
    long long* total = nullptr;   // [n] sum of the item's durations
    int* flags = nullptr;         // [n] bit 0: even lo does not fit the budget
};
void launch_fit_durations(const FitArgs& a, int n, hipStream_t s);
// SC_ERR_INVALID naming the item: a negative target, a bound that is not finite, lo <= 0, lo > hi (host only)
void check_fit_items(const char* who, int n, const int32_t* h_target, const float* h_lo, const float* h_hi);
// Time-scale modification (k_tsm.hip): the body of sc_time_stretch and of sc_op_tsm_centres.  Every
// argument check (SC_ERR_INVALID naming `who`) comes before the first device call; then the peak, the frame walk (one workgroup
// per item) and - with d_out - the overlap-add, on the default stream; returns when the results are complete.  with_out: d_out / out_stride
// are checked and written (sc_time_stretch); otherwise the search alone, and h_centres [n][m_stride] takes the centres.
void run_time_stretch(const char* who, const float* d_in, int n, int64_t in_stride, const int64_t* h_in_len, const int64_t* h_out_len,
                      const ::sc_tsm_opts* opts, bool with_out, float* d_out, int64_t out_stride, int32_t* h_centres, int64_t m_stride);
void launch_vocoder_embed(const int* units, int nb, int T, const __half* dict, int E,
                          const __half* lang, int Lg, const int* lang_idx, const __half* spkr, int Sp,
                          const int* spkr_idx, float* out /*[nb*T][Lg+E+Sp]*/, hipStream_t s,
                          const int* item_off = nullptr /*packed items: [nb + 1] unit-row offsets, T unused*/, int rows_total = 0);
void launch_avg3(const float* a, const float* b, const float* c, float* out, int64_t n, hipStream_t s);
// Conv1d(cin -> 1, k taps, 'same') with LeakyReLU(in_slope) on the input and `act` on the output (k_misc.hip: the vocoder's conv_post)
bool conv_to_mono_supported(int cin, int cout, int k, int stride, int pad, int dil, int act);
void launch_conv_to_mono(const float* x, const __half* w_packed, const float* bias, int nb, int T, int cin, int k, float in_slope, int act,
                         float* y, hipStream_t s, const int* item_off = nullptr /*packed items: T = the longest item's rows*/,
                         int item_mul = 1, int64_t rows_total = 0);
// packed items (GemmArgs::item_off) at `mul` rows per unit row: the {position, item length} table of GemmPsArgs::row_pos
void launch_item_row_pos(const int* item_off, int n_items, int mul, int rows, int2* row_pos, hipStream_t s);
// dst[item_of[i] * dst_stride + t] = src[item_off[i] * mul + t] for t < (item_off[i + 1] - item_off[i]) * mul
void launch_scatter_items(const float* src, const int* item_off, const int* item_of, int n_items, int mul, int longest, int64_t dst_stride,
                          float* dst, hipStream_t s);
void launch_fill_i32(int* p, int v, int n, hipStream_t s);
void launch_add_i32(int* p, int v, hipStream_t s);

// Greedy generation, live-row compaction (model_decoder.hip: run_generate_text): pair i moves the state of the still
// generating row src[i] into slot dst[i], whose own hypothesis has finished, and keeps that hypothesis' results in slot
// src[i]: K / V rows 0 .. filled-1 of every layer and the encoder K / V go src -> dst (the finished row's are dead),
// tokens, flags, lengths, scores, the sequence and the captured decoder outputs are exchanged.
constexpr int ROWSWAP_MAX_LAYERS = 32;
constexpr int ROWSWAP_MAX_PAIRS = 64;
struct RowSwapArgs {
    float* k[ROWSWAP_MAX_LAYERS];
    float* v[ROWSWAP_MAX_LAYERS];
    float* cross[ROWSWAP_MAX_LAYERS];
    int layers = 0, pairs = 0;
    unsigned char src[ROWSWAP_MAX_PAIRS], dst[ROWSWAP_MAX_PAIRS];
    int M = 0, cap = 0, s_enc = 0, filled = 0;  // K / V row length, rows per cache slot, encoder rows, positions written so far
    int* tok = nullptr;
    int* finished = nullptr;
    int* out_len = nullptr;
    int* enc_lens = nullptr;
    int* prompt_len = nullptr;  // per-row prompt lengths (nullable): a row may move while it is still inside its prompt
    float* lprob = nullptr;
    float* score = nullptr;
    int* hist = nullptr;      // [rows][cap]
    float* hidden = nullptr;  // [rows][cap - 1][M] or null
};
void launch_row_swap(const RowSwapArgs& a, hipStream_t s);

// Greedy generation with cross-attention capture (k_xattn.hip; sc_generate_text_capture): one launch after a step of the
// row-group chain.  Row slot b that was fed at this step (position *d_pos - 1) gets the soft-max of the LAST decoder layer's
// encoder-decoder attention summed over the heads in head order, xattn[slot_utt[b]][pos][0 .. s_enc) (0 behind the row's
// encoder length), and the log-probability of the token the step chose, lprob[slot_utt[b]][pos] (0 without am_part: a
// prompt position fed without vocabulary projection).  Rows behind *d_rows and rows finished at an earlier step are skipped.
constexpr int XCAP_MAX_HEADS = 16;
struct XattnCapArgs {
    const float* q = nullptr;       // [nb][M] complete query rows of the last layer's cross attention (StepCtx::qkvr)
    const float* kv = nullptr;      // the last layer's encoder K / V [nb][s_enc][2M], keys at column 0, head h at h * 64
    const int* enc_lens = nullptr;  // [nb]
    const int* d_pos = nullptr;     // position counter, already advanced by the step
    const int* d_rows = nullptr;    // live rows (null: all)
    const int* finished = nullptr;
    const int* out_len = nullptr;
    const int* slot_utt = nullptr;  // [nb]: utterance held by slot b (the live-row compaction moves rows)
    const float4* am_part = nullptr;  // the step's arg-max records [am_tiles][nb] (null: the step did not project)
    int am_tiles = 0;
    const float* eos_logit = nullptr;
    int force_eos_step = -1;
    float* xattn = nullptr;  // [utterances][cap][s_enc]
    float* lprob = nullptr;  // [utterances][cap]
    int nb = 0, s_enc = 0, heads = 0, cap = 0;
};
void launch_xattn_capture(const XattnCapArgs& a, hipStream_t s);

// The same rows for a whole teacher-forced pass (k_xattn.hip; sc_score_text_capture): xattn[b][p][j] = sum over the heads, in
// head order, of softmax_j(q_h(b, p) . k_h(b, j) / 8) for p < tok_lens[b] - 1 and j < enc_lens[b], 0 everywhere else (the
// kernel writes the zeros: the output needs no memset).  One workgroup per XROWS_QT query rows of one item, keys staged
// XROWS_KC rows at a time.  A row's bits depend on its own item only.  Head width 64, at most XCAP_MAX_HEADS heads.
constexpr int XROWS_QT = 16, XROWS_KC = 64;
struct XattnRowsArgs {
    const float* q = nullptr;  // [n * S1] query rows, stride ldq, head h at column h * 64
    const float* k = nullptr;  // [n * s_enc] key rows, stride ldk, head h at column h * 64
    int64_t ldq = 0, ldk = 0;
    const int* enc_lens = nullptr;  // [n] on the device
    const int* tok_lens = nullptr;  // [n] on the device: whole sequence lengths, tok_lens[b] - 1 live rows
    float* xattn = nullptr;         // [n][S1][s_enc]
    int n = 0, S1 = 0, s_enc = 0, heads = 0;
};
void launch_xattn_rows(const XattnRowsArgs& a, hipStream_t s);
// SC_CHECK that `heads` heads of width 64 make up model_dim and fit XCAP_MAX_HEADS; `who` opens the message
void check_xattn_rows_geometry(int heads, int model_dim, const char* who);

// ---- UnitY2 forced aligner (k_align.hip; reference models/aligner/model.py) --------------------------------------
// out[row] = table[ids[row]] (fp16 table, no scale, no positions)
void launch_align_embed(const int* ids, int rows, const __half* table, int C, float* out, hipStream_t s);
// lprob[b][f][t] = log_softmax_t(-temperature * ||feat[b][f] - text[b][t]||_2): text [n][St][C], feat [n][Sf][C] fp32
// (C % 32 == 0), ragged by the device length tables; text positions behind an item's length are -inf, feature rows behind
// its length zeros
void launch_align_lprob(const float* text, const float* feat, int n, int St, int Sf, int C, const int* d_text_lens, const int* d_feat_lens,
                        float temperature, float* lprob, hipStream_t s);
// Monotonic alignment search + back-track of every item of lprob [n][Sf][St]: dur [n][St] int32 (zeros behind the text
// length).  bits: scratch of n * mas_bits_words(max_text_len, Sf) 64-bit words (one decision bit per cell).  Limits:
// max_text_len <= mas_max_text() (2048), max_feat_len <= mas_max_feat() (8192); above, an error and no launch.
int mas_max_text();
int mas_max_feat();
size_t mas_bits_words(int max_text_len, int Sf);
void launch_mas(const float* lprob, int n, int St, int Sf, const int* d_text_lens, const int* d_feat_lens, int max_text_len,
                int max_feat_len, unsigned long long* bits, int* dur, hipStream_t s);

// ---- wav2vec 2.0 front end of the UnitExtractor (k_w2v2.hip; reference models/unit_extractor) ---------------------
// stats[2 i] = mean, stats[2 i + 1] = 1 / sqrt(biased variance + 1e-5) of item i's samples (F.layer_norm over the utterance).
// An odd num_samples[i] counts one more sample of value 1.0 (the reference's Collater(pad_value=1, pad_to_multiple=2)).
void launch_w2v2_wave_stats(const float* wav, int64_t wav_stride, const int* num_samples, int nb, float* stats, hipStream_t s);
// First extractor layer on the normalised waveform: Conv1d(1 -> C, k taps, stride, bias, no padding), LayerNorm over the C
// channels (eps 1e-5) and exact GELU in one pass; out [nb][t_rows][C], row t of item i from samples t*stride .. + k - 1
// (samples behind the item's - padded - length read as zeros).  w fp32 [C][k].  C % 4 == 0, C <= 1024, k <= 16.
void launch_w2v2_conv0(const float* wav, int64_t wav_stride, const int* num_samples, const float* stats, int nb, const float* w,
                       const float* bias, const float* gamma, const float* beta, int C, int k, int stride, float* out, int t_rows,
                       hipStream_t s);
// Position encoder: y = x + GELU(conv(x) + bias), conv = grouped Conv1d(C -> C, k taps, padding k/2, `groups` groups) with its
// last output step dropped (k even); x / y [nb][T][C] fp32 (y != x), rows t >= lens[i] of x read as zeros (lens nullable).
// w fp32 packed [group][tap][c_in][c_out] (launch_w2v2_pack_pos_weight from the checkpoint's [C][C/groups][k]).
// C / groups <= 128.
void launch_w2v2_pack_pos_weight(const float* w, float* dst, int C, int groups, int k, hipStream_t s);
void launch_w2v2_pos_conv(const float* x, const float* w_packed, const float* bias, float* y, int nb, int T, int C, int groups, int k,
                          const int* lens, hipStream_t s);
// k-means operands (kmeans.py:24-30 as an arg-max, see model_w2v2.hip): rows of x [rows][C] as planes [rows][2C] = [x | x]
void launch_w2v2_dup_split(const float* x, int64_t ldx, int rows, int C, __half* hi, __half* lo, hipStream_t s);
// centroids cent [C][K] fp32 (the reference's transposed layout) -> W [K][2C] = [fp16(c) | fp16(c - fp16(c))] and
// bias[j] = -||c_hi + c_lo||^2 / 2 (fp32 sum in ascending channel order)
void launch_w2v2_pack_centroids(const float* cent, int C, int K, __half* W, float* bias, hipStream_t s);

// ---- ECAPA-TDNN prosody encoder (k_ecapa.hip; reference models/pretssel/ecapa_tdnn.py) ------------------------------
// The Res2Net chain of one SE-Res2Net block in one launch: out[:, 0:CW] = x[:, 0:CW]; y_1 = B_0(x_1), y_i = B_{i-1}(x_i + y_{i-1}),
// B = Conv1d(CW -> CW, k = 3, dilation dil, 'same') + ReLU + LayerNorm(CW, eps 1e-12); out[:, i CW : (i + 1) CW] = y_i.  x / out
// [nb][T][ldx / ldo] fp32 (out != x), frames outside [0, T) zeros at the input of every stage.  w[i]: packed tap-major
// [CW][ldw] fp16 (launch_pack_conv_weight), bias / gamma / beta [CW] fp32.  CW in {32, 64}, dil <= 8.
constexpr int ECAPA_MAX_SCALE = 8;
struct EcapaChainArgs {
    const float* x = nullptr;
    int64_t ldx = 0;
    float* out = nullptr;
    int64_t ldo = 0;
    const __half* w[ECAPA_MAX_SCALE - 1] = {};
    int64_t ldw = 0;
    const float* bias[ECAPA_MAX_SCALE - 1] = {};
    const float* gamma[ECAPA_MAX_SCALE - 1] = {};
    const float* beta[ECAPA_MAX_SCALE - 1] = {};
    int nb = 0, T = 0, CW = 0, scale = 0, dil = 1;
};
bool ecapa_chain_supported(int chunk, int scale, int k, int dil);
int ecapa_chain_tile_rows(int scale, int dil);  // frames a workgroup stores
void launch_ecapa_chain(const EcapaChainArgs& a, hipStream_t s);
// y[row] = act(LayerNorm(relu(x[row] + item_bias[row / t_per_item]))) over C channels, eps 1e-12; act ACT_NONE / ACT_TANH; y may be x
void launch_ecapa_relu_ln(const float* x, int64_t ldx, const float* item_bias, int t_per_item, const float* g, const float* b, float* y, int64_t ldy,
                          int rows, int C, int act, hipStream_t s);
// gate[n][C] = sigmoid(W2 relu(W1 s + b1) + b2), s = sum over t < lens[n] of x[n][t] / lens[n] (lens null: T); w1 [S][C], w2 [C][S] fp16
void launch_ecapa_se_gate(const float* x, int64_t ldx, int nb, int T, const int* d_lens, int C, int S, const __half* w1, const float* b1,
                          const __half* w2, const float* b2, float* gate, hipStream_t s);
// out = y * gate[item] + res on every frame
void launch_ecapa_se_apply(const float* y, int64_t ldy, const float* gate, const float* res, int64_t ldr, float* out, int64_t ldo, int nb, int T, int C,
                           hipStream_t s);
// gstats[n] = [mean | sqrt(max(variance around the mean, 1e-12))] of x [nb][T][C] over the frames t < lens[n]
void launch_ecapa_gstats(const float* x, int nb, int T, int C, const int* d_lens, float* gstats, hipStream_t s);
// out[n][j] = W[j][k0 .. k0 + K) . v[n] + bias[j]
void launch_ecapa_item_bias(const __half* W, int64_t ldw, int k0, const float* bias, const float* v, int nb, int K, int N, float* out, hipStream_t s);
// pooled[n] = [sum_t a_t x_t | sqrt(max(sum_t a_t (x_t - mean)^2, 1e-12))], a = softmax over t < lens[n] of logits [nb][T][C] per channel
void launch_ecapa_pool(const float* x, const float* logits, int nb, int T, int C, const int* d_lens, float* pooled, hipStream_t s);
// out[n] = normalize(W LayerNorm(pooled[n]) + bias): LayerNorm(C2, eps 1e-12), W [E][ldw] fp16, L2 norm clamped at 1e-12
void launch_ecapa_tail(const float* pooled, int nb, int C2, const float* g, const float* b, const __half* W, int64_t ldw, const float* bias, int E,
                       float* out, hipStream_t s);
// y = (x - mean) / std on the frames t < lens[n] of x [nb][T][D], zeros behind
void launch_ecapa_gcmvn(const float* x, const float* mean, const float* stdv, const int* d_lens, int nb, int T, int D, float* y, hipStream_t s);

// ---- PRETSSEL acoustic model (k_pretssel.hip; reference models/generator/vocoder.py:488-513) --------------------------
// Every FiLM projection of a call: out[i][j] = mul[j] * (W[j] . [pros_i | lang] + bias[j]) + add[j] for the N stacked output rows
// of all FiLM layers (W [N][P + Lg] fp16; mul = s_gamma / s_beta, add = 1 / 0 of the gamma / beta halves), fp32 FMA.  Lg == 0
// (lang may be null): the conditioning vector alone; rows with mul = 1, add = 0 are plain linear slices (the expressive T2U's
// prosody_proj rides in the same launch)
void launch_pretssel_film(const float* pros, int P, const float* lang, int Lg, const __half* W, const float* bias, const float* mul, const float* add,
                          int n, int N, float* out, hipStream_t s);
// y = mask(FiLM(LayerNorm(x))) per row and group: x [rows][ldx] holds `groups` slices of C channels, g / b [groups][C] (eps 1e-5);
// film (nullable) [items][film_ld]: group grp of item i reads gamma' at film_off + grp * 2C, beta' behind it, y = gamma' * ln + beta';
// row_item[row] (nullable: item 0) names the row's item, < 0 marks a row behind its item's length: exact zeros.
// y (fp32) and / or the planes yh / yl.  C a multiple of 64 up to 1024.
struct PretsselLnArgs {
    const float* x = nullptr;
    int64_t ldx = 0;
    const float* g = nullptr;
    const float* b = nullptr;
    const float* film = nullptr;
    int64_t film_ld = 0;
    int film_off = 0;
    const int* row_item = nullptr;
    float* y = nullptr;
    int64_t ldy = 0;
    __half* yh = nullptr;
    __half* yl = nullptr;
    int64_t ldh = 0;
    int rows = 0, C = 0, groups = 1;
};
bool pretssel_ln_supported(int C);
void launch_pretssel_film_ln(const PretsselLnArgs& a, hipStream_t s);
// variance adaptor tail (length_regulator.py:295-312): f [rows][3][H] = the pitch / voiced / energy predictors' rows behind their
// FiLM, pw [3][H] / pb [3] their projections; pitch = vuv >= 0 ? pitch : 0; x [rows][C] += (pitch wp + bp) + (energy we + be).
// vals (nullable) [rows][3]: the three projections.
struct PretsselTailArgs {
    const float* f = nullptr;
    const float* pw = nullptr;
    const float* pb = nullptr;
    const float* wp = nullptr;
    const float* bp = nullptr;
    const float* we = nullptr;
    const float* be = nullptr;
    float* x = nullptr;
    float* vals = nullptr;
    int rows = 0, H = 0, C = 0;
};
void launch_pretssel_var_tail(const PretsselTailArgs& a, hipStream_t s);
// Gaussian upsampling (length_regulator.py:42-96) of packed items: tokens [tok_off[i], tok_off[i + 1]) of x [tokens][C] with
// durations dur become the frames [frame_off[i], frame_off[i + 1]); y[m] = softmax_k(-delta (t - c_k)^2) . x + pos_alpha *
// pos_table[t] (pos_table nullable).  centre: scratch [tokens].  wsum (nullable) [frames]: the kept soft-max mass relative to the
// row maximum.  Tokens whose energy lies more than pretssel_ups_cutoff() under the row maximum are dropped (k_pretssel.hip).
constexpr int PRETSSEL_UPS_VPL = 8;  // C <= 512
struct PretsselUpsArgs {
    const float* x = nullptr;
    const int* dur = nullptr;
    const int* tok_off = nullptr;
    const int* frame_off = nullptr;
    float* centre = nullptr;
    const float* pos_table = nullptr;
    float pos_alpha = 0.f, delta = 0.1f;
    float* y = nullptr;
    __half* yh = nullptr;
    __half* yl = nullptr;
    float* wsum = nullptr;
    int n = 0, frames = 0, C = 0;
};
float pretssel_ups_cutoff();
void launch_pretssel_upsample(const PretsselUpsArgs& a, hipStream_t s);
// y[m] = embed[tok[m]] + alpha * pos_table[row_t[m]] as fp32 rows and planes
void launch_pretssel_embed_pos(const int* tok, const int* row_t, const __half* embed, const float* pos_table, float alpha, int rows, int C, float* y,
                               __half* yh, __half* yl, hipStream_t s);
// post-net over the EXTENDED rows: item i's frames followed by its halo rows (ext_item[m], ext_pos[m] = {position, frames + halo})
//   _in:      planes [ext_rows][CP] of the projection rows (halo rows: the projection's bias; columns C .. CP-1 zeros)
//   _bn_tanh: planes of tanh(x * scale + shift)
//   _out:     mel[i][t][C] (row stride t_cap) = (proj + x * scale + shift) * gstd + gmean on the frame rows
void launch_pretssel_postnet_in(const float* proj, const float* bias, const int* ext_item, const int2* ext_pos, const int* frame_off, int ext_rows, int C,
                                int CP, __half* yh, __half* yl, hipStream_t s);
void launch_pretssel_postnet_bn_tanh(const float* x, const float* scale, const float* shift, int rows, int C, __half* yh, __half* yl, hipStream_t s);
void launch_pretssel_postnet_out(const float* x, const float* scale, const float* shift, const float* proj, const float* gstd, const float* gmean,
                                 const int* ext_item, const int2* ext_pos, const int* frame_off, int ext_rows, int C, int t_cap, float* mel, hipStream_t s);

// ---- PRETSSEL waveform generator, SEANet half (k_seanet.hip; reference models/generator/streamable.py, vocoder.py:556-572) ---
// Packed items: rows [time][C] of every item back to back, row_off / in_off / out_off [n + 1] on the device.
// 2-layer LSTM (gate order i, f, g, o), one launch per step: the launch at t computes layer 0 at step t (xproj = x . W_ih0^T
// for all rows comes from one product up front) and layer 1 at step t - 1 from [h0 ; h1] against w1 = [W_ih1 | W_hh1], and
// writes y = h1 + x.  Steps 0 .. longest item inclusive: T + 1 launches.  c0 / c1 [n][H] start as zeros.
struct LstmStepArgs {
    const float* xproj = nullptr;  // [rows][4H]
    const float* x = nullptr;      // [rows][H]
    const __half* whh0 = nullptr;  // [4H][H]
    const __half* w1 = nullptr;    // [4H][2H]
    const float* b_ih0 = nullptr;
    const float* b_hh0 = nullptr;
    const float* b_ih1 = nullptr;
    const float* b_hh1 = nullptr;
    float* h0 = nullptr;  // [rows][H]
    float* h1 = nullptr;  // [rows][H]
    float* c0 = nullptr;  // [n][H]
    float* c1 = nullptr;
    float* y = nullptr;   // [rows][H]
    float* max_pre = nullptr;  // nullable: largest |gate pre-activation|
    const int* row_off = nullptr;
    int H = 0;
};
bool lstm2_supported(int H);  // a multiple of 32 up to 2048
void launch_lstm2_step(const LstmStepArgs& a, int n, int t, hipStream_t s);
// y = x + conv_k1(ELU(conv_k3(ELU(x)))), C -> C / 2 -> C, at C = 32 / 64; w1 [C/2][3 * C] tap-major, w2 [C][C/2] fp16
constexpr int SEANET_RES_TILE = 64;
struct SeanetResArgs {
    const float* x = nullptr;
    const __half* w1 = nullptr;
    const float* b1 = nullptr;
    const __half* w2 = nullptr;
    const float* b2 = nullptr;
    float* y = nullptr;  // must not alias x
    const int* row_off = nullptr;
    int n = 0, longest = 0, C = 0;
};
bool seanet_resblock_supported(int C);
void launch_seanet_resblock(const SeanetResArgs& a, hipStream_t s);
// streamable convolutions: y[q] = bias + sum_tap w[tap] . in_act(x[q * stride + tap - left]) (+ res), zeros outside the item;
// transposed (k = 2 * stride): y[p] = bias + the two taps of the untrimmed output at p + left.  wt [k * cin][cout] fp16.
enum SeanetInAct { SEANET_IN_NONE = 0, SEANET_IN_ELU = 1, SEANET_IN_TANH = 2 };
struct SconvArgs {
    const float* x = nullptr;
    const __half* wt = nullptr;
    const float* bias = nullptr;
    const float* res = nullptr;  // indexed like y; the forward convolution only
    float* y = nullptr;
    const int* in_off = nullptr;
    const int* out_off = nullptr;
    int n = 0, longest_out = 0, cin = 0, cout = 0, k = 0, stride = 1, left = 0, in_act = SEANET_IN_NONE;
};
bool sconv_supported(int cin, int cout, int k, int stride);  // the input window of a tile fits 48 KB of LDS
void launch_sconv(const SconvArgs& a, hipStream_t s);
void launch_sconvtr(const SconvArgs& a, hipStream_t s);
// wav[t] = 0.8 * (bias + conv_k(ELU(h)))[t] + tanh(skip[t]) for t < the item's output length; h on the decoder's own length
struct SeanetTailArgs {
    const float* h = nullptr;     // [decoder rows][cin]
    const __half* w = nullptr;    // [k * cin] tap-major
    const float* bias = nullptr;  // [1]
    const float* skip = nullptr;  // packed by out_off
    float* wav = nullptr;         // wav_stride != 0: [n][wav_stride], else packed by out_off
    const int* in_off = nullptr;
    const int* out_off = nullptr;
    int64_t wav_stride = 0;
    int n = 0, longest_out = 0, cin = 0, k = 0;
};
bool seanet_tail_supported(int cin, int k);  // odd k; the weights and a tile's activated rows fit 48 KB of LDS
void launch_seanet_tail(const SeanetTailArgs& a, hipStream_t s);
// mel [n][t_cap][dim] -> out [off[n]][dim] = (mel - mean) / scale on every item's own rows, items back to back
void launch_mel_norm_pack(const float* mel, const float* mean, const float* scale, const int* off, int n, int longest, int t_cap, int dim, float* out,
                          hipStream_t s);
// [d0][d1][k] fp32 (Conv1d: [cout][cin][k]; transposed: ConvTranspose1d's [cin][cout][k]) -> [k * cin][cout] fp16
void launch_pack_sconv_weight(const float* w, __half* dst, int cin, int cout, int k, bool transposed, hipStream_t s);

// ---- decode engine (k_engine.hip, engine.hip) ---------------------------------------------------------------------
// One greedy step chain per GPU shared by every pass in flight.  A ROW STATE r (0 .. rows-1) owns everything that lives as
// long as a hypothesis: K / V cache rows, encoder K / V, token history, captured decoder outputs, position, flags.  A SLOT s
// (0 .. slots-1) is a row of the step's activations; slot_rp[s] = {row state, its position}.  The live slots are packed to
// the front (*d_rows of them); admitting a row or dropping a finished one only rewrites slot_rp - no cache row moves.
struct EngineRows {
    int* tok = nullptr;         // [rows] token fed at the next step
    int* pos = nullptr;         // [rows] position fed at the next step
    int* finished = nullptr;    // [rows]
    int* out_len = nullptr;     // [rows] length of the hypothesis incl. prompt and EOS
    int* limit = nullptr;       // [rows] longest hypothesis of the row's request (forced EOS at position limit - 2)
    int* prefix_len = nullptr;  // [rows] prompt tokens (positions 0 .. prefix_len-2 are fed from hist, nothing is chosen there)
    int* enc_lens = nullptr;    // [rows]
    float* score = nullptr;     // [rows]
    int* hist = nullptr;        // [rows][cap]
    float* hidden = nullptr;    // [rows][cap - 1][M] captured decoder outputs
    int cap = 0, M = 0;
};
// closing launch of an engine step: combines the vocabulary projection's per-group records of every live slot (same
// expressions as argmax_finalize_kernel), applies the row's own forced-EOS / prompt rules, appends the token, and advances the
// row's position (a finished row keeps its position and is fed padding until the host drops it from the live slots)
struct EngineFinalizeArgs {
    const float4* part = nullptr;  // [tiles][slots]
    int tiles = 0, slots = 0;
    const float* eos_logit = nullptr;  // [slots]
    int2* slot_rp = nullptr;
    const int* d_rows = nullptr;
    int pad_idx = 0, eos_idx = 0;
    EngineRows rows;
};
void launch_engine_finalize(const EngineFinalizeArgs& a, hipStream_t s);
// new rows: one record each (uploaded by the host), state initialised on the device
constexpr int ENGINE_MAX_PREFIX = 12;
struct EngineAdmitRec {
    int rid, limit, prefix_len, enc_len;
    int prefix[ENGINE_MAX_PREFIX];
};
void launch_engine_admit(const EngineAdmitRec* d_recs, int n, const EngineRows& rows, int pad_idx, hipStream_t s);
// slot_rp[s] = {rids[s], pos[rids[s]]}, slot_lane[s] = lanes[s] for s < n_live ({0, 0} / 0 behind); *d_rows = n_live.
// d_rids holds the row states followed by the K / V lanes ([2][slots]).
void launch_engine_set_slots(const int* d_rids, int n_live, int slots, int2* slot_rp, int* slot_lane, const int* pos, int* d_rows, hipStream_t s);
// finished rows leave: decoder outputs 0 .. out_len-2 of row state rid -> dst[t][M] (zeros up to dst_rows), and
// {out_len, score bits, hist[0 .. cap)} -> stage[i][2 + cap]
struct EngineRetireRec {
    int rid, dst_rows;
    float* dst;  // nullable
};
void launch_engine_retire(const EngineRetireRec* d_recs, int n, const EngineRows& rows, int* stage, hipStream_t s);

}  // namespace sc
