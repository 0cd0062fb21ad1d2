// Kernels of the UnitY2 forced aligner (reference models/aligner/model.py:146-277): embedding gather, the distance +
// log-softmax score matrix, and the monotonic alignment search with its back-track.
#include <cmath>

#include "device_util.h"

namespace sc {

namespace {

// ---- embedding gather (StandardEmbedding, no scale, no positions) ----------------------------------------------- //
__global__ __launch_bounds__(256) void align_embed_kernel(const int* __restrict__ ids, const __half* __restrict__ table, int C,
                                                          float* __restrict__ out) {
    const int row = blockIdx.x;
    const __half* e = table + (int64_t)ids[row] * C;
    for (int c = threadIdx.x; c < C; c += 256) out[(int64_t)row * C + c] = __half2float(e[c]);
}

// ---- score[b][f][t] = -temperature * || feat[b][f] - text[b][t] ||_2 -------------------------------------------------- //
// Computed on DIFFERENCES (sum of (f - t)^2), not as |f|^2 + |t|^2 - 2 f.t: where a unit frame is close to its character -
// the cells that decide the path - the expanded form cancels to a few digits.  A workgroup owns a 64 x 64 tile of
// (feature row, text position) pairs; 32-channel slabs of both operands go through LDS (rows padded to 36 floats: the
// 16-byte reads of the 16 lanes that differ in their row then fall on 16 different bank groups), every lane keeps a 4 x 4
// register tile of pairs (rows ty + 16 i, columns tx + 16 j), so one slab costs it 8 x 8 LDS reads of 16 bytes for 512
// subtract + multiply-add pairs.  Per pair the squares of a slab are summed first and the slab sums then added up: the
// rounding error grows with 32 + C / 32 terms instead of C.  Tiles wholly behind an item's lengths are skipped (nobody reads
// them: the log-softmax kernel writes those cells itself).
constexpr int DT = 64, DK = 32, DLD = DK + 4;

__global__ __launch_bounds__(256) void align_dist_kernel(const float* __restrict__ text, const float* __restrict__ feat, int St, int Sf,
                                                         int C, const int* __restrict__ text_lens, const int* __restrict__ feat_lens,
                                                         float temperature, float* __restrict__ score) {
    __shared__ __attribute__((aligned(16))) float Fs[DT * DLD];
    __shared__ __attribute__((aligned(16))) float Ts[DT * DLD];
    const int b = blockIdx.z, f0 = blockIdx.y * DT, t0 = blockIdx.x * DT;
    if (f0 >= feat_lens[b] || t0 >= text_lens[b]) return;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const float* fb = feat + (int64_t)b * Sf * C;
    const float* tb = text + (int64_t)b * St * C;
    float acc[4][4] = {};
    for (int k0 = 0; k0 < C; k0 += DK) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int idx = tid + q * 256, r = idx >> 3, c4 = (idx & 7) * 4;
            float4 vf = make_float4(0.f, 0.f, 0.f, 0.f), vt = vf;
            if (f0 + r < Sf) vf = *reinterpret_cast<const float4*>(fb + (int64_t)(f0 + r) * C + k0 + c4);
            if (t0 + r < St) vt = *reinterpret_cast<const float4*>(tb + (int64_t)(t0 + r) * C + k0 + c4);
            *reinterpret_cast<float4*>(&Fs[r * DLD + c4]) = vf;
            *reinterpret_cast<float4*>(&Ts[r * DLD + c4]) = vt;
        }
        __syncthreads();
        float part[4][4] = {};
#pragma unroll
        for (int kk = 0; kk < DK; kk += 4) {
            float4 a[4], t[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a[i] = *reinterpret_cast<const float4*>(&Fs[(ty + 16 * i) * DLD + kk]);
                t[i] = *reinterpret_cast<const float4*>(&Ts[(tx + 16 * i) * DLD + kk]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float dx = a[i].x - t[j].x, dy = a[i].y - t[j].y, dz = a[i].z - t[j].z, dw = a[i].w - t[j].w;
                    part[i][j] = fmaf(dw, dw, fmaf(dz, dz, fmaf(dy, dy, fmaf(dx, dx, part[i][j]))));
                }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] += part[i][j];
        __syncthreads();
    }
    float* ob = score + (int64_t)b * Sf * St;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int f = f0 + ty + 16 * i;
        if (f >= Sf) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = t0 + tx + 16 * j;
            if (t < St) ob[(int64_t)f * St + t] = -temperature * sqrtf(acc[i][j]);
        }
    }
}

__device__ __forceinline__ float wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// In-place masked log-softmax over the text positions of one (item, feature row): positions behind the text length become
// -inf (model.py:177-181), rows behind the feature length are written as zeros.
__global__ __launch_bounds__(256) void align_lsm_kernel(float* __restrict__ x, int St, int Sf, const int* __restrict__ text_lens,
                                                        const int* __restrict__ feat_lens) {
    __shared__ float red[4];
    const int b = blockIdx.y, f = blockIdx.x, tid = threadIdx.x;
    float* row = x + ((int64_t)b * Sf + f) * St;
    if (f >= feat_lens[b]) {
        for (int t = tid; t < St; t += 256) row[t] = 0.f;
        return;
    }
    const int Tt = text_lens[b];
    float mx = -INFINITY;
    for (int t = tid; t < Tt; t += 256) mx = fmaxf(mx, row[t]);
    mx = wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sum = 0.f;
    for (int t = tid; t < Tt; t += 256) sum += expf(row[t] - mx);
    sum = wave_sum(sum);
    if ((tid & 63) == 0) red[tid >> 6] = sum;
    __syncthreads();
    const float lse = mx + logf((red[0] + red[1]) + (red[2] + red[3]));
    for (int t = tid; t < St; t += 256) row[t] = t < Tt ? row[t] - lse : -INFINITY;
}

// ---- monotonic alignment search (model.py:212-277) ---------------------------------------------------------------------- //
// One item per workgroup.  Column 0 of Q is Q[0][0] = lprob[0][0] and -inf below; column j (all text positions i at feature
// frame j) follows from column j - 1:
//     Q[i][j] = max(Q[i-1][j-1], Q[i][j-1]) + lprob[j][i],   Q[-1][.] = -inf
// which is the reference's recurrence with its row 0 (a running sum, added up in frame order) and its -inf triangle i > j
// falling out of the same expression.  Q is DOUBLE and the fp32 log-probability is converted and added as numpy does, so the comparisons are the
// reference's bit for bit.  A lane owns MAS_R = 4 consecutive text positions: the i - 1 neighbour is a register or one
// __shfl_up, and an item of up to 64 x 4 = 256 characters is one wave that never meets a barrier in the column loop.  Wider
// items (up to MAS_MAX_WAVES = 8 waves: 2048 characters) hand the last value of every wave to the next one through LDS,
// double-buffered: one barrier per column that waits for LDS only, so the prefetched log-probabilities stay in flight.
// The loads of column j + MAS_PF are issued while column j is computed: they do not depend on Q.
// Only the decision bit Q[i-1][j-1] >= Q[i][j-1] (ties: the upper row, as the reference's back-track picks) of every cell
// is kept: word ((j * W + wave) * 4 + r) holds the bits of positions (wave * 64 + lane) * 4 + r, lane = bit number.  After
// the forward pass the same workgroup walks back from (T_text - 1, T_feat - 1), 64 columns of bits staged in LDS at a time,
// and writes the run lengths (np.bincount of the path) as the durations.
constexpr int MAS_R = 4, MAS_PF = 4, MAS_MAX_WAVES = 8;

__device__ __forceinline__ void lds_barrier() {
    // waits for this wave's LDS traffic only (not for the global loads in flight), then the workgroup barrier
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

__global__ __launch_bounds__(64 * MAS_MAX_WAVES) void mas_kernel(const float* __restrict__ lprob, int64_t item_stride, int St,
                                                                 const int* __restrict__ text_lens, const int* __restrict__ feat_lens,
                                                                 unsigned long long* __restrict__ bits, int64_t bits_stride,
                                                                 int* __restrict__ dur) {
    __shared__ double hand[2][MAS_MAX_WAVES];
    __shared__ unsigned long long sb[64 * 8];
    __shared__ int s_wc;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, W = blockDim.x >> 6;
    const int Tt = text_lens[b], Tf = feat_lens[b];
    const float* lp = lprob + (int64_t)b * item_stride;
    unsigned long long* bw = bits + (int64_t)b * bits_stride;
    int* d = dur + (int64_t)b * St;
    for (int i = tid; i < St; i += blockDim.x) d[i] = 0;
    if (tid < MAS_MAX_WAVES) hand[0][tid] = hand[1][tid] = -INFINITY;
    __syncthreads();

    const int i0 = tid * MAS_R;
    int col[MAS_R];  // clamped: lanes behind the text length compute values nobody uses, from addresses inside the item
#pragma unroll
    for (int r = 0; r < MAS_R; ++r) col[r] = min(i0 + r, Tt - 1);
    double q[MAS_R];
#pragma unroll
    for (int r = 0; r < MAS_R; ++r) q[r] = -INFINITY;
    if (tid == 0) q[0] = (double)lp[0];
    float pf[MAS_PF][MAS_R];  // columns 1 .. MAS_PF to start with; slot (j - 1) % MAS_PF holds column j
#pragma unroll
    for (int u = 0; u < MAS_PF; ++u) {
        const float* rowp = lp + (int64_t)min(1 + u, Tf - 1) * St;
#pragma unroll
        for (int r = 0; r < MAS_R; ++r) pf[u][r] = rowp[col[r]];
    }
    for (int j0 = 1; j0 < Tf; j0 += MAS_PF) {
#pragma unroll
        for (int u = 0; u < MAS_PF; ++u) {
            const int j = j0 + u;
            if (j >= Tf) break;  // uniform over the workgroup
            float cur[MAS_R];
            const float* rowp = lp + (int64_t)min(j + MAS_PF, Tf - 1) * St;
#pragma unroll
            for (int r = 0; r < MAS_R; ++r) {
                cur[r] = pf[u][r];
                pf[u][r] = rowp[col[r]];
            }
            double up = __shfl_up(q[MAS_R - 1], 1);
            if (lane == 0) up = w > 0 ? hand[(j + 1) & 1][w - 1] : -INFINITY;
            bool bt[MAS_R];
            double nq[MAS_R];
            bt[0] = up >= q[0];
            nq[0] = (bt[0] ? up : q[0]) + (double)cur[0];
#pragma unroll
            for (int r = 1; r < MAS_R; ++r) {
                bt[r] = q[r - 1] >= q[r];
                nq[r] = (bt[r] ? q[r - 1] : q[r]) + (double)cur[r];
            }
#pragma unroll
            for (int r = 0; r < MAS_R; ++r) {
                q[r] = nq[r];
                const unsigned long long m = __ballot(bt[r]);
                if (lane == r) bw[((int64_t)j * W + w) * MAS_R + r] = m;
            }
            if (W > 1) {
                if (lane == 63) hand[j & 1][w] = q[MAS_R - 1];
                lds_barrier();
            }
        }
    }
    __syncthreads();  // every decision word is in memory and visible to the workgroup

    int i = Tt - 1, run = 1;  // thread 0 walks; column T_feat - 1 belongs to the last text position
    for (int jhi = Tf - 1; jhi >= 1; jhi -= 64) {
        if (tid == 0) s_wc = i / (64 * MAS_R);
        __syncthreads();
        // the path climbs at most one position per column: over 64 columns it stays inside the wave of i and the one above
        const int wc = s_wc, jlo = max(jhi - 63, 1), ncol = jhi - jlo + 1;
        for (int idx = tid; idx < ncol * 8; idx += blockDim.x) {
            const int c = idx >> 3, k = idx & 7, ww = wc - (k >> 2);
            sb[idx] = ww >= 0 ? bw[((int64_t)(jlo + c) * W + ww) * MAS_R + (k & 3)] : 0ull;
        }
        __syncthreads();
        if (tid == 0) {
            for (int j = jhi; j >= jlo; --j) {
                if (i > 0) {
                    const int k = (wc - i / (64 * MAS_R)) * 4 + (i & 3);
                    if ((sb[(j - jlo) * 8 + k] >> ((i & (64 * MAS_R - 1)) >> 2)) & 1ull) {
                        d[i] = run;
                        run = 0;
                        --i;
                    }
                }
                ++run;
            }
        }
    }
    if (tid == 0) d[i] = run;
}

}  // namespace

void launch_align_embed(const int* ids, int rows, const __half* table, int C, float* out, hipStream_t s) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(align_embed_kernel, dim3(rows), dim3(256), 0, s, ids, table, C, out);
    SC_LAUNCH_CHECK();
}

void launch_align_lprob(const float* text, const float* feat, int n, int St, int Sf, int C, const int* d_text_lens, const int* d_feat_lens,
                        float temperature, float* lprob, hipStream_t s) {
    SC_CHECK(n > 0 && St > 0 && Sf > 0 && C > 0 && C % DK == 0, "align_lprob: bad geometry (n=%d s_text=%d s_feat=%d C=%d, C %% 32 == 0)", n,
             St, Sf, C);
    SC_CHECK(n <= 65535 && cdiv(Sf, DT) <= 65535 && (int64_t)Sf * St < (1ll << 31), "align_lprob: batch of %d items of %d x %d cells is too large",
             n, Sf, St);
    {
        // reads: both operands once per tile of the other side; writes: the scores
        prof::Scope scope("align_dist", 3.0 * n * (double)Sf * St * C, 4.0 * n * ((double)Sf * St + (double)(Sf + St) * C), s);
        hipLaunchKernelGGL(align_dist_kernel, dim3(cdiv(St, DT), cdiv(Sf, DT), n), dim3(256), 0, s, text, feat, St, Sf, C, d_text_lens,
                           d_feat_lens, temperature, lprob);
        SC_LAUNCH_CHECK();
    }
    prof::Scope scope("align_lsm", 4.0 * n * (double)Sf * St, 8.0 * n * (double)Sf * St, s);
    hipLaunchKernelGGL(align_lsm_kernel, dim3(Sf, n), dim3(256), 0, s, lprob, St, Sf, d_text_lens, d_feat_lens);
    SC_LAUNCH_CHECK();
}

int mas_max_text() { return 64 * MAS_R * MAS_MAX_WAVES; }
int mas_max_feat() { return 8192; }
size_t mas_bits_words(int max_text_len, int Sf) { return (size_t)Sf * cdiv(max_text_len, 64 * MAS_R) * MAS_R; }

void launch_mas(const float* lprob, int n, int St, int Sf, const int* d_text_lens, const int* d_feat_lens, int max_text_len,
                int max_feat_len, unsigned long long* bits, int* dur, hipStream_t s) {
    SC_CHECK(n > 0 && St > 0 && Sf > 0 && max_text_len >= 1 && max_text_len <= St && max_feat_len >= 1 && max_feat_len <= Sf,
             "mas: bad geometry (n=%d s_text=%d s_feat=%d)", n, St, Sf);
    SC_CHECK(max_text_len <= mas_max_text(), "mas: %d text positions exceed the limit of %d (64 lanes x %d positions x %d waves)", max_text_len,
             mas_max_text(), MAS_R, MAS_MAX_WAVES);
    SC_CHECK(max_feat_len <= mas_max_feat(), "mas: %d feature frames exceed the limit of %d", max_feat_len, mas_max_feat());
    const int W = cdiv(max_text_len, 64 * MAS_R);
    prof::Scope scope("mas", 2.0 * n * (double)Sf * St, n * (double)Sf * St * (4.0 + 0.125), s);  // fp32 log-probability read + one decision bit written per cell
    hipLaunchKernelGGL(mas_kernel, dim3(n), dim3(64 * W), 0, s, lprob, (int64_t)Sf * St, St, d_text_lens, d_feat_lens, bits,
                       (int64_t)mas_bits_words(max_text_len, Sf), dur);
    SC_LAUNCH_CHECK();
}

}  // namespace sc
