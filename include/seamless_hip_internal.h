/*
 * seamless_hip_internal.h - entry points of libseamless_hip.so that are NOT part of the drop-in boundary: kernel-level hooks
 * the parity tests drive (tests/test_ops_gpu.py, test_dstep_gpu.py, test_dstep3_gpu.py, test_engine_kernels_gpu.py: every hand-written kernel against a
 * PyTorch restatement and against its own variants, bit for bit where the variants claim it), a dependent-chain
 * micro-benchmark, and the introspection of the decoder-step dispatch.  Nothing here has a reference counterpart and nothing
 * of it is needed to run the model; a binding of the reference uses include/seamless_hip.h only.
 * Signatures may change without an ABI version bump.
 */
#ifndef SEAMLESS_HIP_INTERNAL_H_
#define SEAMLESS_HIP_INTERNAL_H_

#include "seamless_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Introspection: the kernel family a decoder step of `rows` live rows is dispatched to for `caller` (0 greedy text
 * generation, 1 beam search over the text decoder, 2 streaming monotonic decoder, 3 beam search over the v1 unit
 * decoder): 1 general (split-K skinny products up to 64 rows, tiled GEMMs above), 2 packed-fragment
 * products, 3 row-group products with fused LayerNorm / residual, 4 the row-group chain cut into row groups (> 64 rows);
 * negative sc_status when the model has no such decoder.  Decided by the predicates the stages themselves use. */
int sc_decoder_step_family(sc_model* m, int rows, int caller);

/* The value the library sees for switch `name` of its knob table (csrc/common.cpp: one table for every SC_* tuning / debugging
 * variable, read once per process; switches that change results are honoured only with SC_DEBUG_NUMERICS=1), `dflt` when unset
 * or gated off.  No device work. */
int sc_op_knob(const char* name, int dflt);

/* Kernel-level entry points used by the parity tests (tests/test_ops_gpu.py).
 * All pointers are device pointers; weights fp16, activations fp32. */
/* 1: route every dense product to the general MFMA kernel instead of the double-buffered fast path
 * (the two produce identical bits; used by the parity tests and for A/B timing). */
int sc_op_force_general_gemm(int on);
/* Host planning of the vocoder's packed pass (no device work; callable without a GPU).  sc_op_voc_pack_plan: `n` items of
 * h_need unit rows each, in their order, cut into consecutive groups of at most budget_rows rows (a longer item is a group of
 * its own); returns the number of groups and writes at most `cap` of the groups' first items, followed by n.
 * sc_op_voc_tile_first: h_off [n + 1] unit-row offsets, `mul` rows per unit row, tiles of tile_rows rows counted from every
 * item's first row -> h_first [n + 1], the first tile (workgroup) of every item and their number.
 * sc_op_last_vocoder_packed_groups: packed groups of the handle's last sc_vocode* call, 0 when it ran the padded batch or the
 * length buckets (SC_VOC_PACKED=0, unit_lens == NULL, a geometry the packed kernels do not take). */
int32_t sc_op_voc_pack_plan(const int32_t* h_need, int32_t n, int64_t budget_rows, int32_t* h_group_first, int32_t cap);
int32_t sc_op_voc_tile_first(const int32_t* h_off, int32_t n, int32_t mul, int32_t tile_rows, int32_t* h_first);
int32_t sc_op_last_vocoder_packed_groups(sc_model* m);
/* the ResBlock op hooks below (sc_op_resblock_pair, sc_op_resblock_pair_ps, sc_op_mrf_fused) multiply the hi fp16 plane of
 * their activations only - the vocoder's shipped variants - while this is on (default off: the two-plane variants) */
int sc_op_single_plane(int on);
int sc_op_layernorm(const float* d_x, const float* d_gamma, const float* d_beta, float* d_y, int32_t rows, int32_t C,
                    int32_t act);
int sc_op_linear(const float* d_x, const void* d_w_f16, const float* d_bias, const float* d_res, float* d_y,
                 int32_t M, int32_t N, int32_t K, int32_t act, float alpha, int32_t split, int32_t force_gemv);
/* Decoder-step products for 1..64 rows (k_skinny.hip).  sc_op_skinny_linear: y = alpha*act(x.W^T+b)+res.
 * sc_op_skinny_res_ln: x += in.W^T + b computed as `splits` K-range partials (0 = pick automatically)
 * summed in fixed order, then h = LayerNorm(x) (d_h may be NULL). */
int sc_op_skinny_linear(const float* d_x, const void* d_w_f16, const float* d_bias, const float* d_res, float* d_y,
                        int32_t M, int32_t N, int32_t K, int32_t act, float alpha);
int sc_op_skinny_res_ln(const float* d_in, const void* d_w_f16, const float* d_bias, float* d_x_inout,
                        const float* d_gamma, const float* d_beta, float* d_h, int32_t M, int32_t N, int32_t K,
                        int32_t splits);
/* Fused vocabulary projection + arg-max under the generation step rules (PAD never, EOS masked while
 * step < min_step_for_eos, EOS forced at step == force_eos_step, UNK penalty); d_lprob receives the
 * log-softmax value of the winner.  step is a host value here. */
int sc_op_skinny_argmax(const float* d_x, const void* d_w_f16, int32_t M, int32_t N, int32_t K, int32_t step,
                        int32_t min_step_for_eos, int32_t force_eos_step, int32_t pad_idx, int32_t eos_idx,
                        int32_t unk_idx, float unk_penalty, int32_t* d_idx, float* d_lprob);

/* Second-generation decoder-step kernels (k_dstep.hip): weights packed into MFMA fragment order, activations as split
 * fp16 planes; same near-fp32 products, own summation order (results agree with the k_skinny.hip kernels to fp32
 * re-association).  sc_op_dstep_res_ln mirrors sc_op_skinny_res_ln (splits: wanted K ranges, 0 = 4);
 * sc_op_dstep_linear_planes: y = act(x.W^T + b) through the split-plane epilogue (K <= 1024);
 * sc_op_dstep_argmax mirrors sc_op_skinny_argmax (ntl: 32-feature tiles per workgroup, 0 = 4);
 * sc_op_dstep_attention: the single-query attention of the step (see api.hip for the operand layout). */
int sc_op_dstep_res_ln(const float* d_in, const void* d_w_f16, const float* d_bias, float* d_x_inout, const float* d_gamma,
                       const float* d_beta, float* d_h, int32_t M, int32_t N, int32_t K, int32_t splits);
int sc_op_dstep_linear_planes(const float* d_x, const void* d_w_f16, const float* d_bias, float* d_y, int32_t M, int32_t N, int32_t K,
                              int32_t act);
int sc_op_dstep_argmax(const float* d_x, const void* d_w_f16, int32_t M, int32_t N, int32_t K, int32_t step,
                       int32_t min_step_for_eos, int32_t force_eos_step, int32_t pad_idx, int32_t eos_idx, int32_t unk_idx,
                       float unk_penalty, int32_t ntl, int32_t* d_idx, float* d_lprob);
int sc_op_dstep_attention(const float* d_proj, int32_t S, const float* d_bias, float* d_kcache, float* d_vcache, int32_t cap,
                          int32_t pos, const int32_t* d_lens, int32_t cross, int32_t nb, int32_t heads, float* d_out);
/* Third-generation decoder-step kernels (k_dstep3.hip): row-group products that apply the preceding LayerNorm and the
 * bias / residual / ReLU (act = 1) or exact-erf GELU (act = 4, mode 2 only) themselves.  sc_op_dstep3_gemv, rg = rows per row group (0 = default):
 *   mode 0: y = LayerNorm(x; gamma, beta) . W^T + b                         (K <= 1024)
 *   mode 1: y = res + x . W^T + b                                           (K <= 1024, res [M][N])
 *   mode 2: y = act(LayerNorm(x) . W^T + b) through the split-plane epilogue (K <= 1024)
 *   mode 3: y = res + x . W^T + b as K-slice partial sums + the reduce kernel; gamma != null: d_h = LayerNorm(y)
 * shape, bits 0..3: workgroup shape, 0 = 1 tile x 16 waves x 4 k-steps, 1 = 2 tiles x 8 waves x 8 k-steps (K <= 1024), 2 = 2
 * tiles x 8 waves x 4 k-steps (512-wide K slices, mode 3).  M up to 512 rows.  Bits 4..7 pick the kernel of the FFN shapes
 * over several row groups (same bits whichever runs): 0 the launcher decides, 15 one workgroup per row group (gemv3_kernel),
 * 14 tile-owning waves (gemv3t_kernel, mode 3), k in 1..13 weights stationary with k workgroups per tile (gemv3s_kernel).
 * rg, bits 8..: live rows (a device-side row count as the beam search / the decode engine pass it; the rows behind it are
 * neither read nor written), 0 = all M rows.
 * sc_op_dstep3_argmax mirrors sc_op_dstep_argmax on the LDS-staged vocabulary projection. */
int sc_op_dstep3_gemv(int32_t mode, const float* d_x, const void* d_w_f16, const float* d_bias, const float* d_gamma,
                      const float* d_beta, const float* d_res, float* d_y, float* d_h, int32_t M, int32_t N, int32_t K, int32_t act,
                      int32_t rg, int32_t shape);
int sc_op_dstep3_argmax(const float* d_x, const void* d_w_f16, int32_t M, int32_t N, int32_t K, int32_t step,
                        int32_t min_step_for_eos, int32_t force_eos_step, int32_t pad_idx, int32_t eos_idx, int32_t unk_idx,
                        float unk_penalty, int32_t* d_idx, float* d_lprob);
/* Diagnostic: n launches of one decoder-step kernel as a dependent chain in a replayed hipGraph; wall time per launch
 * (kinds: see api.hip). */
int sc_op_chain_bench(int32_t kind, int32_t rows, int32_t n, int32_t reps, float* us_per_kernel);
int sc_op_conv1d(const float* d_x, const void* d_w_f16_packed, const float* d_bias, const float* d_res, float* d_y,
                 int32_t nb, int32_t t_in, int32_t cin, int32_t cout, int32_t k, int32_t stride, int32_t pad,
                 int32_t dil, const int32_t* d_in_lens, int32_t in_act, int32_t act);
int sc_op_pack_conv_weight(const void* d_w_f16, void* d_dst_f16, int32_t cout, int32_t cin, int32_t k);
int sc_op_conv_transpose1d(const float* d_x, const void* d_v_f16, const void* d_g_f16, const float* d_bias,
                           float* d_y, int32_t nb, int32_t t_in, int32_t cin, int32_t cout, int32_t k,
                           int32_t stride, int32_t pad, int32_t in_act);
/* y = alpha*act(x.W^T + b) + res through the PRE-SPLIT product kernel (k_gemm_ps.hip): x is first split into two
 * fp16 planes on the device, the operands then reach LDS by DMA.  d_y (fp32) and/or d_yh/d_yl (the result as two
 * fp16 planes, the format the next product consumes) may be requested.  Same bits as sc_op_linear(split=1). */
int sc_op_linear_presplit(const float* d_x, const void* d_w_f16, const float* d_bias, const float* d_res, float* d_y,
                          void* d_yh_f16, void* d_yl_f16, int32_t M, int32_t N, int32_t K, int32_t act, float alpha);
/* y [M][N / 2] = GLU(x.W^T + b) = value * sigmoid(gate), W [N][K] with the N / 2 value rows first and the gate rows behind them
 * (the first pointwise convolution of the Conformer convolution module).  fused = 1: the rows of W interleaved on the device and
 * the GLU applied in the pre-split product's epilogue (launch_gemm_presplit_glu); fused = 0: sc_op_linear_presplit's product to
 * fp32 followed by the GLU kernel.  The two must be bit-identical (tests/test_encoder_glu_epilogue_gpu.py).  N % 4 == 0. */
int sc_op_linear_presplit_glu(const float* d_x, const void* d_w_f16, const float* d_bias, float* d_y, int32_t M, int32_t N, int32_t K,
                              int32_t fused);
/* d_idx[m] = arg-max over n of (x.W^T + b)[m][n] with the arg-max FUSED into the pre-split product's epilogue (no logits in
 * memory; the unit projection of the NAR T2U, reference models/unity/model.py:438-441 + inference/generator.py:346): equal to
 * the arg-max of sc_op_linear_presplit's d_y, lowest index among equal values. */
int sc_op_linear_presplit_argmax(const float* d_x, const void* d_w_f16, const float* d_bias, int32_t* d_idx, int32_t M, int32_t N,
                                 int32_t K);
/* Log-softmax statistics of v = x.W^T + b per row with NO logits in memory (the vocabulary projection of sc_score_text): the
 * pre-split product's epilogue keeps one {max, sum exp(v - max), sum v, v[target], arg-max} record per row and column range
 * (sc_op_score_record_cols(N) columns, a function of N alone), a finish kernel folds them in column order.  Per row m:
 *   d_lse[m] = log sum_j exp v[m][j];  d_lprob[m] = v[m][target[m]] - d_lse[m]  (0 where target[m] < 0; always <= 0);
 *   d_sum_lprob[m] = sum_j v[m][j] - N d_lse[m];  d_top1[m] = arg-max, lowest column among equal values (inside [0, N) for
 *   every row).  A row's results depend on that row alone, to the bit: not on M, nor on the row group.  A NaN in a row of x
 *   makes that row's three floats NaN and touches no other row.  Any of the four outputs may be NULL (not all).
 * _grouped: rows go through in groups of group_rows (0: as many as 32 MB of record scratch hold, sc_op_score_group_rows(N)). */
int sc_op_linear_presplit_score(const float* d_x, const void* d_w_f16, const float* d_bias, const int32_t* d_target, float* d_lprob,
                                float* d_sum_lprob, float* d_lse, int32_t* d_top1, int32_t M, int32_t N, int32_t K);
int sc_op_linear_presplit_score_grouped(const float* d_x, const void* d_w_f16, const float* d_bias, const int32_t* d_target,
                                        float* d_lprob, float* d_sum_lprob, float* d_lse, int32_t* d_top1, int32_t M, int32_t N,
                                        int32_t K, int32_t group_rows);
/* The candidate-set form (the vocabulary projection of sc_identify_language): h_cand [n_cand] on the host, strictly ascending
 * columns inside [0, N), 1 <= n_cand <= 512 (anything else: SC_ERR_INVALID before any launch).  Each wave of the product also
 * writes v at the candidate columns of its range; the finish kernel gives d_lprob [M][n_cand] = v[m][cand[j]] - lse[m] - bit for
 * bit sc_op_linear_presplit_score's d_lprob with target cand[j] - and d_best [M] = the j of the largest v[m][cand[j]], the lowest
 * j among equal values.  A NaN row: NaN log-probabilities, d_best 0, no other row touched. */
int sc_op_score_candidates(const float* d_x, const void* d_w_f16, const float* d_bias, const int32_t* h_cand, int32_t n_cand, float* d_lprob,
                           int32_t* d_best, int32_t M, int32_t N, int32_t K);
int32_t sc_op_score_record_cols(int32_t N);
int32_t sc_op_score_group_rows(int32_t N);
/* The cross-attention rows of sc_score_text_capture by themselves (k_xattn.hip: xattn_rows_kernel; tests/test_xattn_rows_kernel_gpu.py):
 * d_q [n * s1] query rows (stride ldq floats), d_k [n * s_enc] key rows (stride ldk), head h in columns h * 64 .. h * 64 + 63 of both;
 * h_enc_lens [n] in 1..s_enc, h_tok_lens [n] in 2..s1 + 1 (whole sequence lengths: item b has tok_lens[b] - 1 live rows).
 * d_xattn [n][s1][s_enc] = sum over the heads in head order of softmax_j(q_h . k_h / 8), 0 behind the live rows and keys
 * (written by the kernel).  1..16 heads; q / k 16-byte aligned, ldq / ldk multiples of 4.
 * sc_op_xattn_rows_tile(0): query rows one workgroup owns; (1): key rows staged in LDS at a time. */
int sc_op_xattn_rows(const float* d_q, int64_t ldq, const float* d_k, int64_t ldk, int32_t n, int32_t s1, int32_t s_enc, int32_t heads,
                     const int32_t* h_enc_lens, const int32_t* h_tok_lens, float* d_xattn);
int32_t sc_op_xattn_rows_tile(int32_t which);
/* Conv1d (stride 1) through the pre-split product kernel's implicit-convolution mode: x [nb][t][cin] is split into two
 * fp16 planes, output row (i, t) reads rows t + tap*dil - pad of item i (zeros outside the item), weights packed by
 * sc_op_pack_conv_weight.  d_row_valid (nullable, [nb*t] bytes on the device): rows with 0 are written as exact zeros.
 * Same bits as sc_op_conv1d on the same values. */
int sc_op_conv1d_presplit(const float* d_x, const void* d_w_f16_packed, const float* d_bias, const float* d_res, float* d_y,
                          void* d_yh_f16, void* d_yl_f16, int32_t nb, int32_t t, int32_t cin, int32_t cout, int32_t k, int32_t pad,
                          int32_t dil, const unsigned char* d_row_valid, int32_t act);
/* The same dilation pair as the wide vocoder stages (C >= 128, C % 32 == 0, odd k) run it: LeakyReLU(x) as split fp16 planes,
 * both convolutions on the DMA-fed GEMM in implicit-convolution mode (weights packed by sc_op_pack_conv_weight). */
int sc_op_resblock_pair_ps(const float* d_x, const void* d_w1_packed, const float* d_b1, const void* d_w2_packed, const float* d_b2,
                           float* d_out, int32_t nb, int32_t T, int32_t C, int32_t k, int32_t dil);
/* One HiFi-GAN ResBlock dilation pair (hifigan.py:114-121) fused in one kernel for C in {16, 32, 64}:
 * out = x + conv2_{k,1}(lrelu(conv1_{k,dil}(lrelu(x)) + b1)) + b2, weights packed by sc_op_pack_conv_weight
 * (rows padded to a multiple of 32); with d_avg_a/d_avg_b: out = ((a + b) + that) / 3. */
int sc_op_resblock_pair(const float* d_x, const void* d_w1_packed, const float* d_b1, const void* d_w2_packed,
                        const float* d_b2, float* d_out, int32_t nb, int32_t T, int32_t C, int32_t k, int32_t dil,
                        float slope, const float* d_avg_a, const float* d_avg_b);
/* The whole multi-receptive-field block of a narrow vocoder stage (hifigan.py:186-191: the average of the three ResBlocks,
 * kernel sizes k[0..2], three dilation pairs each, dil[3 * block + pair]) fused in one kernel for C in {16, 32}.  The four
 * pointer tables are HOST arrays of nine device pointers (pair q = 3 * block + pair), weights packed by
 * sc_op_pack_conv_weight.  Same bits as nine sc_op_resblock_pair calls, the last one averaging. */
int sc_op_mrf_fused(const float* d_x, const void* const* d_w1_packed, const float* const* d_b1, const void* const* d_w2_packed,
                    const float* const* d_b2, float* d_out, int32_t nb, int32_t T, int32_t C, const int32_t* k, const int32_t* dil,
                    float slope);
int sc_op_attention(const float* d_q, const float* d_k, const float* d_v, float* d_out, int32_t nb, int32_t heads,
                    int32_t sq, int32_t skv, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                    const int32_t* d_kv_lens, int32_t causal, const float* d_rel_k, int32_t rel_left,
                    int32_t rel_right);
/* sc_op_attention with every field of the kernel's argument block (kernels.h: AttnArgs); a null pointer turns its
 * feature off.  d_row_off: packed rows, item n at rows d_row_off[n] .. + d_kv_lens[n].  d_rp_table [2*skv-1][rp_ld] with
 * d_q_bias_u / d_q_bias_v [heads*64]: Transformer-XL relative positions.  d_out_hi / d_out_lo (fp16, row stride ldoh):
 * the result as two fp16 planes instead of d_out. */
int sc_op_attention_ex(const float* d_q, const float* d_k, const float* d_v, float* d_out, int32_t nb, int32_t heads,
                       int32_t sq, int32_t skv, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo,
                       const int32_t* d_kv_lens, int32_t causal, const float* d_rel_k, int32_t rel_left,
                       int32_t rel_right, const int32_t* d_row_off, const float* d_rp_table, int64_t rp_ld,
                       const float* d_q_bias_u, const float* d_q_bias_v, void* d_out_hi, void* d_out_lo, int64_t ldoh);
int sc_op_glu_dwconv(const float* d_x, const float* d_w, float* d_y, int32_t nb, int32_t T, int32_t C, int32_t k,
                     const int32_t* d_lens);
/* Fused element-wise passes of the Conformer stack (k_norm.hip); fused = 0 runs the separate launches they replace, the
 * results must be bit-identical.  sc_op_glu_dwconv_ln: x [nb*T][2C] -> split fp16 planes [nb*T][C] of
 * act(LayerNorm(causal_dwconv_k(GLU(x)))) (k = 31, C % 64 == 0, C <= 1024).  sc_op_layernorm2: y = LN_a(x) [rows][C] fp32
 * and the planes of LN_b(y). */
int sc_op_glu_dwconv_ln(const float* d_x, const float* d_w, const float* d_gamma, const float* d_beta, int32_t act, void* d_yh_f16,
                        void* d_yl_f16, int32_t nb, int32_t T, int32_t C, int32_t k, const int32_t* d_lens, int32_t fused);
/* fused = 2 above: the gated form of the fused kernel, x [nb*T][C] already holds GLU(.).
 * sc_op_glu_dwconv_ln_packed: the same kernel on packed rows (the ragged speech encoder) - item i owns rows h_row_off[i] ..
 * h_row_off[i] + h_lens[i] of x ([rows][2C], gated: [rows][C]) and of the planes; the work table is built here from the two host
 * lists.  An item's rows must equal sc_op_glu_dwconv_ln on the item alone bit for bit; rows no item owns are not written. */
int sc_op_glu_dwconv_ln_packed(const float* d_x, const float* d_w, const float* d_gamma, const float* d_beta, int32_t act, void* d_yh_f16,
                               void* d_yl_f16, int32_t n, const int32_t* h_row_off, const int32_t* h_lens, int32_t C, int32_t k, int32_t gated);
int sc_op_layernorm2(const float* d_x, const float* d_ga, const float* d_ba, const float* d_gb, const float* d_bb, float* d_y,
                     void* d_yh_f16, void* d_yl_f16, int32_t rows, int32_t C, int32_t fused);
int sc_op_argmax(const float* d_logits, int32_t rows, int32_t V, int32_t* d_idx, float* d_lprob);

/* Beam-search step kernels (k_beam.hip) through the launchers the text decoder's beam search calls (tests/test_beam_kernels_gpu.py).
 * sc_op_beam_candidates: best K candidates (d_cand_val / d_cand_idx [n_utt][K], flattened beam * V + token) of each utterance's
 * `beams` logit rows [n_utt*beams][ld] under the step rules; chunked = 1 runs the four-kernel search and fails unless the shape
 * is one it takes, 0 the single-workgroup kernel.  d_seqs [n_utt*beams][seq_ld] (nullable): S tokens per row for the n-gram
 * blocker of size G (logits of blocked tokens are overwritten with -inf).  d_rows (chunked only) / d_slots: live rows / slots
 * (device counts, nullable).
 * sc_op_beam_select: one candidate walk (kernels.h: BeamSelectArgs, n slots); sc_op_beam_compact: BeamCompactArgs;
 * sc_op_gather_cache: dst[l][r][t] = src[l][src_row[r]][t] for t < len; sc_op_row_token_lprob: log-softmax value of `token` in
 * rows 0, row_stride, 2 * row_stride, ... */
int sc_op_beam_candidates(float* d_logits, int64_t ld, int32_t n_utt, int32_t beams, int32_t V, const float* d_cum, int32_t first_step,
                          int32_t no_eos, int32_t force_eos, int32_t pad_idx, int32_t eos_idx, int32_t unk_idx, float unk_penalty, int32_t K,
                          float* d_cand_val, int32_t* d_cand_idx, const int32_t* d_seqs, int32_t seq_ld, int32_t S, int32_t G,
                          const int32_t* d_rows, const int32_t* d_slots, int32_t chunked);
/* sc_op_beam_candidates plus a banned-sequence list in DEVICE memory (CSR: d_banned_tokens, d_banned_offsets [n_banned + 1];
 * tests/test_banned_gpu.py): runs beam_candidates_banned_kernel / step_processors_kernel.  Needs d_seqs; the list is read
 * back and checked against the limits of sc_generate_text_banned before the launch.  n_banned == 0 is sc_op_beam_candidates. */
int sc_op_beam_candidates_banned(float* d_logits, int64_t ld, int32_t n_utt, int32_t beams, int32_t V, const float* d_cum,
                                 int32_t first_step, int32_t no_eos, int32_t force_eos, int32_t pad_idx, int32_t eos_idx, int32_t unk_idx,
                                 float unk_penalty, int32_t K, float* d_cand_val, int32_t* d_cand_idx, const int32_t* d_seqs,
                                 int32_t seq_ld, int32_t S, int32_t G, const int32_t* d_rows, const int32_t* d_slots, int32_t chunked,
                                 const int32_t* d_banned_tokens, const int32_t* d_banned_offsets, int32_t n_banned);
/* sc_op_beam_candidates_banned plus a boost phrase list in DEVICE memory (CSR, any order; tests/test_boost_gpu.py): the list is
 * read back, checked against the limits of sc_generate_text_boosted (pad_idx / eos_idx are the call's) and sorted on the host,
 * then beam_candidates_boost_kernel / step_processors_boost_kernel run.  Needs d_seqs.  n_boost == 0 or boost == 0 is
 * sc_op_beam_candidates_banned. */
int sc_op_beam_candidates_boost(float* d_logits, int64_t ld, int32_t n_utt, int32_t beams, int32_t V, const float* d_cum,
                                int32_t first_step, int32_t no_eos, int32_t force_eos, int32_t pad_idx, int32_t eos_idx, int32_t unk_idx,
                                float unk_penalty, int32_t K, float* d_cand_val, int32_t* d_cand_idx, const int32_t* d_seqs,
                                int32_t seq_ld, int32_t S, int32_t G, const int32_t* d_rows, const int32_t* d_slots, int32_t chunked,
                                const int32_t* d_banned_tokens, const int32_t* d_banned_offsets, int32_t n_banned,
                                const int32_t* d_boost_tokens, const int32_t* d_boost_offsets, int32_t n_boost, float boost);
/* The sampling step of sc_generate_text_sampled (k_sample.hip; tests/test_sample_kernel_gpu.py, restated in tests/sample_oracle.py):
 * one top-k / top-p draw per logit row [rows][ld] under the step rules, a pure function of (row, options, seed, d_stream[r],
 * d_gen[r], d_position[r]).  temperature > 0; top_k 0 = off; 0 < top_p <= 1.  d_seqs (nullable) with S, G and the banned list as
 * sc_op_beam_candidates_banned (blocked logits are overwritten with -inf; not on a forced-EOS step).  Per row: d_tok the drawn
 * token, d_lprob its value v_t (log-softmax of logits / temperature under the rules), d_kept the size of the kept set and
 * d_z_kept its integer mass (sum of floor(exp(v) * 2^36)). */
int sc_op_sample_rows(float* d_logits, int64_t ld, int32_t rows, int32_t V, const uint64_t* d_stream, const int32_t* d_gen,
                      const int32_t* d_position, float temperature, int32_t top_k, float top_p, uint64_t seed, int32_t no_eos, int32_t force_eos,
                      int32_t pad_idx, int32_t eos_idx, int32_t unk_idx, float unk_penalty, const int32_t* d_seqs, int32_t seq_ld, int32_t S,
                      int32_t G, const int32_t* d_banned_tokens, const int32_t* d_banned_offsets, int32_t n_banned, int32_t* d_tok,
                      float* d_lprob, int32_t* d_kept, uint64_t* d_z_kept);
int sc_op_beam_select(const float* d_cand_val, const int32_t* d_cand_idx, const int32_t* d_seqs_cur, int32_t* d_seqs_new, float* d_fin_score,
                      int32_t* d_fin_len, int32_t* d_fin_seq, int32_t* d_fin_count, int32_t* d_done, int32_t* d_remaining, int32_t* d_tok,
                      int32_t* d_src_row, float* d_cum, int32_t* d_anc, int32_t anc_ld, const int32_t* d_slot_utt, const int32_t* d_slots,
                      int32_t n, int32_t beams, int32_t K, int32_t V, int32_t max_len, int32_t step, int32_t eos_idx, int32_t pad_idx,
                      int32_t normalize, float len_penalty);
int sc_op_beam_compact(const int32_t* d_done, int32_t* d_slot_utt, int32_t* d_slots, int32_t* d_rows, int32_t* d_seqs, float* d_cum,
                       int32_t* d_tok, int32_t* d_enc_lens, int32_t* d_anc, int32_t n, int32_t beams, int32_t max_len, int32_t anc_ld,
                       int32_t seq_len, int32_t anc_len);
/* The score history of sc_generate_text_nbest (tests/test_nbest_kernels_gpu.py).  sc_op_beam_select_hist is sc_op_beam_select with
 * d_hist_cur / d_hist_new [n*beams][max_len] and d_fin_hist [n][beams][max_len] (fp32; beam_select_kernel<true>): history rows follow
 * their parents as the sequence rows do, the new candidate's score lands at step + 1, a finished hypothesis keeps its parent's
 * history and the raw score of its EOS candidate at step + 1, 0 behind it.  sc_op_beam_compact_hist is sc_op_beam_compact with
 * d_hist [n*beams][max_len], moved with the slots (seq_len positions).  sc_op_beam_nbest (beam_nbest_kernel): the fin_count[u]
 * finished hypotheses of utterance u ranked NaN first, then by the higher score, ties to the earlier slot; the first nbest
 * (<= beams <= 8) packed into d_out_ids / d_out_step [n][nbest][max_len], d_out_lens / d_out_scores [n][nbest], d_out_counts [n];
 * step[0] = 0, step[t] = hist[t] - hist[t-1]; pad_idx / 0 behind lengths and counts. */
int sc_op_beam_select_hist(const float* d_cand_val, const int32_t* d_cand_idx, const int32_t* d_seqs_cur, int32_t* d_seqs_new,
                           float* d_fin_score, int32_t* d_fin_len, int32_t* d_fin_seq, int32_t* d_fin_count, int32_t* d_done,
                           int32_t* d_remaining, int32_t* d_tok, int32_t* d_src_row, float* d_cum, int32_t* d_anc, int32_t anc_ld,
                           const int32_t* d_slot_utt, const int32_t* d_slots, int32_t n, int32_t beams, int32_t K, int32_t V, int32_t max_len,
                           int32_t step, int32_t eos_idx, int32_t pad_idx, int32_t normalize, float len_penalty, const float* d_hist_cur,
                           float* d_hist_new, float* d_fin_hist);
int sc_op_beam_compact_hist(const int32_t* d_done, int32_t* d_slot_utt, int32_t* d_slots, int32_t* d_rows, int32_t* d_seqs, float* d_cum,
                            int32_t* d_tok, int32_t* d_enc_lens, int32_t* d_anc, int32_t n, int32_t beams, int32_t max_len, int32_t anc_ld,
                            int32_t seq_len, int32_t anc_len, float* d_hist);
int sc_op_beam_nbest(const int32_t* d_fin_seq, const int32_t* d_fin_len, const float* d_fin_score, const float* d_fin_hist,
                     const int32_t* d_fin_count, int32_t n, int32_t beams, int32_t nbest, int32_t max_len, int32_t pad_idx, int32_t* d_out_ids,
                     int32_t* d_out_lens, float* d_out_scores, int32_t* d_out_counts, float* d_out_step);
int sc_op_gather_cache(const float* d_src, float* d_dst, const int32_t* d_src_row, int32_t rows, int32_t len, int32_t cap, int32_t M,
                       int32_t layers, int64_t layer_stride);
int sc_op_row_token_lprob(const float* d_logits, int64_t ld, int32_t rows, int32_t V, int32_t row_stride, int32_t token, float* d_out);

/* Decode-engine and beam modes of the decoder-step kernels, the engine's bookkeeping (k_engine.hip) and the greedy bookkeeping
 * (k_misc.hip) through the launchers the model calls (tests/test_engine_kernels_gpu.py).  A slot table d_slot_rp is [slots][2]
 * ints {row state, position}.  Every hook reads its index tables back and refuses an entry outside the buffers the caller
 * described (n_states row states, cache_rows cache rows, ...) before it launches anything.
 * sc_op_dstep_attention_ex: sc_op_dstep_attention with the remaining fields of the kernel's argument block (kernels.h:
 * DAttnArgs) as nullable device pointers, nb up to 512 (output planes of the row slots a step of that width uses) and caches
 * of cache_rows rows: d_slot_rp / d_slot_lane (engine: caches and d_lens by row state / lane, q and d_out by slot, `pos`
 * unused), d_anc [nb][cap] (beam self-attention), kv_row_div / d_kv_item (beam cross-attention), d_rows (live rows).  Rows the
 * kernel skips read back as NaN in d_out.
 * sc_op_engine_step_close: the closing pair of an engine step, launch_vocab3 with the per-slot step rules (x [M][K], W [N][K]
 * fp16) + launch_engine_finalize on the caller's EngineRows arrays (hist [n_states][cap]).
 * sc_op_engine_admit: d_recs [n][4 + 12] ints {row state, limit, prefix_len, enc_len, prefix tokens} (EngineAdmitRec).
 * sc_op_engine_set_slots: d_rids [2][slots] row states, then lanes.  sc_op_engine_retire: record i = {h_rid[i], h_dst_rows[i],
 * h_dst[i]} from HOST arrays (h_dst: device pointers, NULL allowed), d_hidden [n_states][cap - 1][M], d_stage [n][2 + cap].
 * sc_op_dstep3_embed_ex: launch_embed3 -> x [rows][C] (NaN where the kernel wrote nothing); d_tok [n_states], embedding
 * [vocab][C] fp16, position table [n_pos][C]; without d_slot_rp every row at `pos`.
 * sc_op_dstep3_reduce_capture_ex: launch_reduce3 as the last launch of a step: x += bias + partials [S][rows][C], d_h =
 * LayerNorm(x), captured row -> d_hrow[owner * hrow_bs + position * C] for position < hrow_rows (owner / position from the slot
 * table, the row itself at `pos` without it).
 * sc_op_step_update / sc_op_row_swap: launch_step_update at host position `pos`; launch_row_swap on d_k / d_v
 * [layers][n_rows][cap][M], d_cross [layers][n_rows][s_enc][2M], pairs from the host arrays h_src / h_dst. */
int sc_op_dstep_attention_ex(const float* d_proj, int32_t S, const float* d_bias, float* d_kcache, float* d_vcache, int32_t cap,
                             int32_t cache_rows, int32_t pos, const int32_t* d_lens, int32_t cross, int32_t nb, int32_t heads,
                             const int32_t* d_slot_rp, const int32_t* d_slot_lane, const int32_t* d_anc, const int32_t* d_kv_item,
                             int32_t kv_row_div, const int32_t* d_rows, float* d_out);
int sc_op_engine_step_close(const float* d_x, const void* d_w_f16, int32_t M, int32_t N, int32_t K, int32_t min_step_for_eos, int32_t pad_idx,
                            int32_t eos_idx, int32_t unk_idx, float unk_penalty, int32_t* d_slot_rp, const int32_t* d_rows, int32_t n_states,
                            int32_t cap, int32_t* d_tok, int32_t* d_pos, int32_t* d_finished, int32_t* d_out_len, const int32_t* d_limit,
                            const int32_t* d_prefix_len, float* d_score, int32_t* d_hist);
int sc_op_engine_admit(const int32_t* d_recs, int32_t n, int32_t n_states, int32_t cap, int32_t pad_idx, int32_t* d_tok, int32_t* d_pos,
                       int32_t* d_finished, int32_t* d_out_len, int32_t* d_limit, int32_t* d_prefix_len, int32_t* d_enc_lens, float* d_score,
                       int32_t* d_hist);
int sc_op_engine_set_slots(const int32_t* d_rids, int32_t n_live, int32_t slots, int32_t n_states, int32_t* d_slot_rp, int32_t* d_slot_lane,
                           const int32_t* d_pos, int32_t* d_rows);
int sc_op_engine_retire(const int32_t* h_rid, const int32_t* h_dst_rows, float* const* h_dst, int32_t n, int32_t n_states, int32_t cap, int32_t M,
                        const int32_t* d_out_len, const float* d_score, const int32_t* d_hist, const float* d_hidden, int32_t* d_stage);
int sc_op_dstep3_embed_ex(const int32_t* d_tok, const void* d_embed_f16, float scale, const float* d_pos_table, int32_t pos,
                          const int32_t* d_slot_rp, const int32_t* d_rows, int32_t rows, int32_t C, int32_t n_states, int32_t n_pos, int32_t vocab,
                          float* d_x);
int sc_op_dstep3_reduce_capture_ex(const float* d_partial, int32_t S, const float* d_bias, float* d_x_inout, const float* d_gamma, const float* d_beta,
                                   float* d_h, float* d_hrow, int64_t hrow_bs, int32_t hrow_rows, int32_t pos, const int32_t* d_slot_rp,
                                   const int32_t* d_rows, int32_t rows, int32_t C, int32_t n_states);
int sc_op_step_update(int32_t* d_next_tok, int32_t* d_hist, int32_t hist_ld, int32_t* d_finished, int32_t* d_out_len, const float* d_lprob,
                      float* d_score, int32_t nb, int32_t pos, int32_t pad_idx, int32_t eos_idx, int32_t* d_n_unfinished);
int sc_op_row_swap(float* d_k, float* d_v, float* d_cross, int32_t layers, int32_t pairs, const int32_t* h_src, const int32_t* h_dst, int32_t n_rows,
                   int32_t M, int32_t cap, int32_t s_enc, int32_t filled, int32_t* d_tok, int32_t* d_finished, int32_t* d_out_len,
                   int32_t* d_enc_lens, float* d_lprob, float* d_score, int32_t* d_hist, float* d_hidden);
/* The row kernels between the products by themselves (k_norm.hip, k_misc.hip; tests/test_row_kernels_gpu.py).  Each hook is
 * the launcher the models call with the caller's strides.
 * sc_op_layernorm_ex: d_y only: launch_layernorm; planes only: launch_layernorm_split; both: launch_layernorm_both (the length
 * mask d_lens [rows / t_per_batch] then zeroes the planes, not the fp32 rows).  d_lens NULL: no mask.
 * sc_op_embed_tokens: out[r] = emb[tok[r]] * scale + pos_table[*d_pos + r % t_per_batch] (d_pos NULL: 0; t_per_batch 0: no row term).
 * sc_op_gather_rows: dst[r] = src[idx[r]] (+ add[r / rows_per_item] when d_add is given), zeros where idx[r] < 0.
 * sc_op_char_embed_add / sc_op_pos_add: the NAR decoder front end's positional terms in place; d_row_t [rows] picks the table row
 * per row (launch_pos_add_rows) instead of r % t_per_batch.
 * sc_op_durations: d_durations [rows] of the variance adaptor's rule; d_lens NULL: every row live.
 * sc_op_vocoder_embed: rows [lang | unit | spkr] -> d_out [rows][Lg + E + Sp]; d_item_off [nb + 1] (packed items, rows_total rows)
 * or NULL (nb items of T rows).  sc_op_item_row_pos: d_row_pos [rows][2] = {row inside its item, rows of the item}.
 * sc_op_scatter_items: dst[item_of[i] * dst_stride + t] = src[item_off[i] * mul + t]; `longest` = rows of the longest item * mul.
 * sc_op_glu_dwconv_ex: sc_op_glu_dwconv with `left` taps before the output position (< 0: k - 1, causal) and, when the four
 * BatchNorm vectors are given, SiLU(BatchNorm(.)) behind the convolution through launch_bn_fold (eps 1e-5).
 * sc_op_relpos_table: d_out [2S - 1][M], the v1 encoder's relative position table. */
int sc_op_layernorm_ex(const float* d_x, int64_t ldx, const float* d_gamma, const float* d_beta, float* d_y, int64_t ldy, void* d_yh_f16,
                       void* d_yl_f16, int64_t ldh, int32_t rows, int32_t C, int32_t act, const int32_t* d_lens, int32_t t_per_batch);
int sc_op_embed_tokens(const int32_t* d_tok, int32_t rows, const void* d_emb_f16, int32_t M, float scale, const float* d_pos_table,
                       const int32_t* d_pos, int32_t t_per_batch, float* d_out, int64_t ldo);
int sc_op_gather_rows(const float* d_src, int64_t lds, const int32_t* d_idx, const float* d_add, int64_t ld_add, int32_t rows_per_item,
                      float* d_dst, int64_t ldd, int32_t rows, int32_t C);
int sc_op_char_embed_add(float* d_seqs, int64_t ld, const int32_t* d_char_ids, const void* d_embed_f16, const float* d_pos_table,
                         int32_t t_per_batch, float alpha, float scale, int32_t rows, int32_t M);
int sc_op_pos_add(float* d_seqs, int64_t ld, const float* d_pos_table, int32_t t_per_batch, const int32_t* d_row_t, float alpha, int32_t rows,
                  int32_t M);
int sc_op_durations(const float* d_h, int64_t ld, const float* d_w, const float* d_b, int32_t rows, int32_t H, int32_t t_per_batch,
                    const int32_t* d_lens, float duration_factor, int32_t min_dur, int32_t* d_durations);
int sc_op_vocoder_embed(const int32_t* d_units, int32_t nb, int32_t T, const void* d_dict_f16, int32_t E, const void* d_lang_f16, int32_t Lg,
                        const int32_t* d_lang_idx, const void* d_spkr_f16, int32_t Sp, const int32_t* d_spkr_idx, float* d_out,
                        const int32_t* d_item_off, int32_t rows_total);
int sc_op_item_row_pos(const int32_t* d_item_off, int32_t n_items, int32_t mul, int32_t rows, int32_t* d_row_pos);
int sc_op_scatter_items(const float* d_src, const int32_t* d_item_off, const int32_t* d_item_of, int32_t n_items, int32_t mul, int32_t longest,
                        int64_t dst_stride, float* d_dst);
int sc_op_glu_dwconv_ex(const float* d_x, const float* d_w, float* d_y, int32_t nb, int32_t T, int32_t C, int32_t k, const int32_t* d_lens,
                        int32_t left, const float* d_bn_g, const float* d_bn_b, const float* d_bn_mean, const float* d_bn_var);
int sc_op_relpos_table(int32_t S, int32_t M, float* d_out);
/* Forced aligner kernels by themselves (k_align.hip; tests/test_aligner_gpu.py).  sc_op_align_lprob: encoder states in
 * (d_text [n][s_text][C], d_feat [n][s_feat][C] fp32, C % 32 == 0; lengths on the host), d_lprob [n][s_feat][s_text] out: the
 * masked log-softmax of -temperature * L2 distance.  sc_op_mas: d_lprob [n][s_feat][s_text] and the lengths in, h_durations
 * [n][s_text] out (zeros behind the text length): the monotonic alignment search with the reference's arithmetic (float32
 * values added into a double Q, ties to the upper row).  Items above 2048 text positions or 8192 frames: SC_ERR_INVALID. */
int sc_op_align_lprob(const float* d_text, const float* d_feat, int32_t n, int32_t s_text, int32_t s_feat, int32_t C,
                      const int32_t* h_text_lens, const int32_t* h_feat_lens, float temperature, float* d_lprob);
int sc_op_mas(const float* d_lprob, int32_t n, int32_t s_text, int32_t s_feat, const int32_t* h_text_lens, const int32_t* h_feat_lens,
              int32_t* h_durations);
/* UnitExtractor kernels by themselves (k_attn_hd.hip at head_dim 80, k_w2v2.hip; tests/test_unit_extractor_gpu.py).
 * sc_op_attention_hd: plain attention with a key-length mask at head_dim 64 (the kernel of sc_op_attention) or 80.
 * sc_op_w2v2_frontend: utterance statistics (d_stats [nb][2] = mean, 1/sqrt(var + 1e-5); odd lengths count one more sample of
 *   1.0) and the first extractor layer with its LayerNorm + GELU fused: d_w [C][k], d_out [nb][t_rows][C].
 * sc_op_w2v2_pos_conv: d_y = d_x + GELU(grouped Conv1d_k(d_x) + bias), last step dropped; d_w [C][C / groups][k] fp32.
 * sc_op_kmeans: d_idx[r] = argmin_j |x_r - c_j|^2 for d_centroids [C][K] fp32 (lowest j among equal distances). */
int sc_op_attention_hd(const float* d_q, const float* d_k, const float* d_v, float* d_out, int32_t nb, int32_t heads, int32_t sq, int32_t skv,
                       int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, const int32_t* d_kv_lens, int32_t head_dim);
int sc_op_w2v2_frontend(const float* d_wav, int64_t wav_stride, const int32_t* h_num_samples, int32_t nb, const float* d_w, const float* d_bias,
                        const float* d_gamma, const float* d_beta, int32_t C, int32_t k, int32_t stride, float* d_out, int32_t t_rows,
                        float* d_stats);
int sc_op_w2v2_pos_conv(const float* d_x, const float* d_w, const float* d_bias, float* d_y, int32_t nb, int32_t T, int32_t C, int32_t groups,
                        int32_t k, const int32_t* d_lens);
int sc_op_kmeans(const float* d_x, const float* d_centroids, int32_t rows, int32_t C, int32_t K, int32_t* d_idx);

/* ProsodyEncoder kernels by themselves (k_ecapa.hip; tests/test_prosody_encoder_gpu.py).  Lengths are host arrays (NULL: every
 * item has T frames); a length outside 1..T is refused before anything is launched.
 * sc_op_ecapa_chain: the fused Res2Net chain of one SE-Res2Net block: d_x / d_out [nb][T][scale * chunk]; d_w [scale - 1][chunk]
 *   [chunk][3] fp16 (Conv1d layout, packed here), d_bias / d_gamma / d_beta [scale - 1][chunk].  sc_op_ecapa_chain_tile: frames
 *   a workgroup stores at this scale and dilation (<= 0: unsupported).
 * sc_op_ecapa_relu_ln: y = act(LayerNorm(relu(x + item_bias[row / t_per_item]))), eps 1e-12, act 0 or 3 (tanh); d_item_bias nullable.
 * sc_op_ecapa_se_gate: d_gate [nb][C] = sigmoid(W2 relu(W1 mean_t(x) + b1) + b2); w1 [S][C], w2 [C][S] fp16.
 * sc_op_ecapa_pool: d_gstats [nb][2C] (nullable) = masked mean | std of d_x [nb][T][C]; d_pooled [nb][2C] (nullable, needs
 *   d_logits [nb][T][C]) = attentive mean | std under the masked softmax over time.
 * sc_op_ecapa_tail: d_out [nb][E] = normalize(W LayerNorm(pooled) + b); d_w [E][C2] fp16.
 * sc_op_prosody_last_launches: kernel launches of the handle's last sc_prosody_encode call. */
int sc_op_ecapa_chain(const float* d_x, const void* d_w_f16, const float* d_bias, const float* d_gamma, const float* d_beta, float* d_out, int32_t nb,
                      int32_t T, int32_t chunk, int32_t scale, int32_t dil);
int32_t sc_op_ecapa_chain_tile(int32_t chunk, int32_t scale, int32_t dil);
int sc_op_ecapa_relu_ln(const float* d_x, const float* d_item_bias, int32_t t_per_item, const float* d_gamma, const float* d_beta, float* d_y,
                        int32_t rows, int32_t C, int32_t act);
int sc_op_ecapa_se_gate(const float* d_x, int32_t nb, int32_t T, const int32_t* h_lens, int32_t C, int32_t S, const void* d_w1_f16, const float* d_b1,
                        const void* d_w2_f16, const float* d_b2, float* d_gate);
int sc_op_ecapa_pool(const float* d_x, const float* d_logits, int32_t nb, int32_t T, int32_t C, const int32_t* h_lens, float* d_pooled, float* d_gstats);
int sc_op_ecapa_tail(const float* d_pooled, int32_t nb, int32_t C2, const float* d_gamma, const float* d_beta, const void* d_w_f16, const float* d_bias,
                     int32_t E, float* d_out);
int32_t sc_op_prosody_last_launches(sc_prosody_encoder* p);

/* PRETSSEL kernels by themselves (k_attn_hd.hip at head_dim 128, k_pretssel.hip; tests/test_pretssel_gpu.py).  Device pointers unless named h_.
 * sc_op_attention128: launch_attention at head_dim 128: q / k / v rows with strides ld*, d_kv_lens (nullable), d_row_off (nullable:
 *   packed rows, needs d_kv_lens and sq == skv), fp32 rows d_out (ldo) or the planes d_out_hi / d_out_lo (ldoh) when those are given.
 * sc_op_pretssel_film: d_out [n][N] = mul * (W [N][P + Lg] fp16 . [pros_i | lang] + bias) + add.
 * sc_op_pretssel_film_ln: LayerNorm -> FiLM -> mask (kernels.h: PretsselLnArgs); d_film / d_row_item / d_y / the planes nullable.
 * sc_op_pretssel_var_tail: kernels.h: PretsselTailArgs; d_x [rows][C] is updated in place, d_vals [rows][3] nullable.
 * sc_op_pretssel_upsample: h_tok_lens [n], h_dur: the items' durations back to back; d_x the tokens back to back [sum lens][C];
 *   d_y [sum frames][C]; d_pos_table nullable; d_wsum [sum frames] nullable.  sc_op_pretssel_ups_cutoff: the energy cut-off.
 * sc_op_pretssel_postnet: the post-net of a loaded handle on d_proj (packed frames [sum lens][mel], h_frame_lens [n]) -> d_mel
 *   [n][t_cap][mel] (de-normalised, zeros behind the frames).  sc_op_pretssel_postnet_tile(rows, dim): rows of the product tile.
 * sc_op_pretssel_last_launches: kernel launches of the handle's last sc_pretssel_mel call (the memset of the output and the
 *   uploads of the row tables are copies, not kernels, and are not counted). */
int sc_op_attention128(const float* d_q, const float* d_k, const float* d_v, float* d_out, int32_t nb, int32_t heads, int32_t sq, int32_t skv,
                       int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, const int32_t* d_kv_lens, const int32_t* d_row_off, void* d_out_hi,
                       void* d_out_lo, int64_t ldoh);
int sc_op_pretssel_film(const float* d_pros, int32_t P, const float* d_lang, int32_t Lg, const void* d_w_f16, const float* d_bias, const float* d_mul,
                        const float* d_add, int32_t n, int32_t N, float* d_out);
int sc_op_pretssel_film_ln(const float* d_x, const float* d_gamma, const float* d_beta, const float* d_film, int32_t film_ld, int32_t film_off,
                           const int32_t* d_row_item, float* d_y, void* d_yh_f16, void* d_yl_f16, int32_t rows, int32_t C, int32_t groups);
int sc_op_pretssel_var_tail(const float* d_f, const float* d_pw, const float* d_pb, const float* d_wp, const float* d_bp, const float* d_we,
                            const float* d_be, float* d_x, float* d_vals, int32_t rows, int32_t H, int32_t C);
int sc_op_pretssel_upsample(const float* d_x, const int32_t* h_tok_lens, const int32_t* h_dur, int32_t n, int32_t C, float delta,
                            const float* d_pos_table, float pos_alpha, float* d_y, void* d_yh_f16, void* d_yl_f16, float* d_wsum);
float sc_op_pretssel_ups_cutoff(void);
int sc_op_pretssel_postnet(sc_pretssel* p, const float* d_proj, int32_t n, const int32_t* h_frame_lens, float* d_mel, int32_t t_cap);
int32_t sc_op_pretssel_postnet_tile(int32_t rows, int32_t dim);
int32_t sc_op_pretssel_last_launches(sc_pretssel* p);
/* launch calls of the handle's last sc_t2u_nar / sc_t2u_nar_cond call behind the T2U encoder (decoder front end, duration predictor,
 * packed FFT decoder, projection; every product / convolution / row-pass call counts once); 0 when the length buckets ran */
int32_t sc_op_t2u_last_launches(sc_model* m);
/* The T2U encoder by itself (run_t2u_encoder, the first stage of sc_t2u_nar / sc_t2u_ar): d_dec_hidden and d_out are
 * [n][s_text][model_dim] fp32 on the device, h_text_lens [n] on the host.  *out_rows (nullable) = rows the call computed: the sum
 * of the lengths on the packed pass (which returns exact zeros at and behind an item's length), n * s_text on the padded one
 * (SC_T2U_ENC_PACKED=0, read per call; tests/test_t2u_encoder_packed_gpu.py). */
int sc_op_t2u_encoder(sc_model* m, const float* d_dec_hidden, int32_t n, int32_t s_text, const int32_t* h_text_lens, float* d_out,
                      int64_t* out_rows);

/* Kernels of the PRETSSEL waveform generator's SEANet half by themselves (k_seanet.hip; tests/test_pretssel_wave_gpu.py).  Packed
 * items: the rows [time][C] of item i follow those of item i - 1, h_lens [n] on the host.
 * sc_op_lstm2: y = LSTM(x) + x, 2 layers, weights [4H][H] fp16 in torch.nn.LSTM's layout (gates i, f, g, o), biases fp32; one
 *   input product and longest + 1 step launches (*h_launches_or_null); *d_max_pre_or_null: largest |gate pre-activation|.
 * sc_op_seanet_resblock: y = x + conv_k1(ELU(conv_k3(ELU(x)))), d_w1 [C/2][C][3], d_w2 [C][C/2][1] fp16, C = 32 / 64;
 *   sc_op_seanet_resblock_tile: rows of one workgroup's tile.
 * sc_op_sconv: the "streamable" convolution, padding_total = k - stride split (total - total / 2) left / (total / 2) right plus
 *   the zeros the last window needs; d_w fp32 [cout][cin][k].  transposed != 0: k = 2 * stride, d_w [cin][cout][k], the output
 *   trimmed by the same split (stride * len rows out).  in_act 0 none / 1 ELU / 2 Tanh.  h_out_lens [n] receives the lengths.
 * sc_op_seanet_tail: d_wav = 0.8 * conv_k(ELU(h)) + tanh(skip) on the first h_out_lens[i] samples of every item; d_h packed by
 *   h_dec_lens [rows][cin], d_w [1][cin][k] fp16, d_skip packed by h_out_lens; wav_stride != 0: d_wav [n][wav_stride]. */
/* sc_op_pretssel_wave_probe: the stage outputs of the handle's NEXT sc_pretssel_wave call (one group only), packed item after
 * item, into device buffers of the caller's (each nullable): d_hifi [sum samples] the HiFi-GAN's output, d_lstm_enc / d_lstm_dec
 * [sum steps][16 * n_filters], d_dec [sum decoder samples][n_filters] the decoder's last residual block.
 * sc_op_pretssel_wave_lens: steps and decoder samples of an item of `frames` frames.  sc_op_pretssel_wave_last_launches: kernel
 * launches of the SEANet half in the last call (the LSTMs: steps + 2 each).  sc_op_pretssel_wave_stage_ms: h_ms6 receives the last
 * call's device time per stage from events on the handle's stream: normalisation + HiFi-GAN, encoder, encoder LSTM, the two
 * convolutions around the bottleneck, decoder LSTM, decoder + tail. */
int sc_op_pretssel_wave_probe(sc_pretssel_wave_model* p, float* d_hifi, float* d_lstm_enc, float* d_lstm_dec, float* d_dec);
int sc_op_pretssel_wave_lens(sc_pretssel_wave_model* p, int32_t frames, int32_t* h_steps, int32_t* h_dec_len);
int32_t sc_op_pretssel_wave_last_launches(sc_pretssel_wave_model* p);
int sc_op_pretssel_wave_stage_ms(sc_pretssel_wave_model* p, float* h_ms6);
int sc_op_lstm2(const float* d_x, const int32_t* h_lens, int32_t n, int32_t H, const void* d_wih0_f16, const void* d_whh0_f16, const float* d_b_ih0,
                const float* d_b_hh0, const void* d_wih1_f16, const void* d_whh1_f16, const float* d_b_ih1, const float* d_b_hh1, float* d_y,
                float* d_max_pre_or_null, int32_t* h_launches_or_null);
int32_t sc_op_seanet_resblock_tile(void);
int sc_op_seanet_resblock(const float* d_x, const int32_t* h_lens, int32_t n, int32_t C, const void* d_w1_f16, const float* d_b1, const void* d_w2_f16,
                          const float* d_b2, float* d_y);
int sc_op_sconv(const float* d_x, const int32_t* h_lens, int32_t n, int32_t cin, int32_t cout, int32_t k, int32_t stride, int32_t transposed,
                int32_t in_act, const float* d_w, const float* d_bias, const float* d_res_or_null, float* d_y, int32_t* h_out_lens);
int sc_op_seanet_tail(const float* d_h, const int32_t* h_dec_lens, const int32_t* h_out_lens, int32_t n, int32_t cin, int32_t k, const void* d_w_f16,
                      const float* d_bias, const float* d_skip, float* d_wav, int64_t wav_stride);


/* The resampler's host side by itself (k_resample.hip; tests/test_resample_cpu.py, test_resample_gpu.py): no device work, callable
 * without a GPU.  sc_op_resample_bank: the compact bank sc_resample multiplies with - *width, *S (taps kept per phase: the
 * longest support rounded up to a multiple of 4), h_k0 [new] the first tap of every phase's support, h_taps [new][S] fp32, zeros
 * behind a phase's own support (which the kernel does not read: a sample under a padding tap reaches no output).  h_k0 / h_taps
 * may both be NULL (sizes only); cap counts the floats h_taps can hold, SC_ERR_CAPACITY below new * S.  orig == new has no bank
 * (width = S = 0).
 * sc_op_resample_plan: h_plan6 = {orig, new, F, F * new, F * orig, LDS bytes}: the reduced rates, the frames one workgroup
 * owns, its outputs and input samples, and the LDS it asks for. */
int sc_op_resample_bank(int32_t orig_freq, int32_t new_freq, const sc_resample_opts* opts, int32_t* width, int32_t* S, int32_t* h_k0,
                        float* h_taps, int64_t cap);
int sc_op_resample_plan(int32_t orig_freq, int32_t new_freq, const sc_resample_opts* opts, int32_t* h_plan6);

/* The search stage of sc_t2u_nar_fit on GIVEN values e = exp(x) - 1 (k_dub.hip; tests/test_fit_durations_gpu.py): d_e
 * [n][s_char] fp32 on the device (rows behind h_char_lens[b] are never read), targets / bounds as sc_t2u_nar_fit takes them,
 * min_dur the lower clamp (0..1000000; the model's is 1).  -> h_durations [n][s_char] (0 behind an item's characters), h_factor
 * [n], h_total [n] int64 (the item's unit total at its factor), h_flags [n].  No handle, current device, default stream. */
int sc_op_fit_durations(const float* d_e, int32_t n, int32_t s_char, const int32_t* h_char_lens, const int32_t* h_target,
                        const float* h_lo, const float* h_hi, int32_t min_dur, int32_t* h_durations, float* h_factor,
                        int64_t* h_total, int32_t* h_flags);

/* The search stage of sc_time_stretch by itself (k_tsm.hip; tests/test_tsm_gpu.py, scripts/tsm_bench.py): the peak, the
 * quantisation and the frame walk of every item, no overlap-add.  Arguments and refusals as sc_time_stretch takes them (there is
 * no output buffer).  -> h_centres [n][m_stride] int32: item i's M_i = ceil(Lo_i / Hs) + 1 centres c_0 .. c_{M_i - 1}; what lies
 * behind them is left as it was.  m_stride below the largest M_i is SC_ERR_INVALID.  No handle, current device, default stream. */
int sc_op_tsm_centres(const float* d_in, int32_t n, int64_t in_stride, const int64_t* h_in_len, const int64_t* h_out_len,
                      const sc_tsm_opts* opts, int32_t* h_centres, int64_t m_stride);

#ifdef __cplusplus
}
#endif
#endif /* SEAMLESS_HIP_INTERNAL_H_ */
