// Device-side vocabulary shared by the k_*.hip files: the MFMA operand types, the fp32 -> (hi, lo) fp16 split, the wave
// reduction, the raw-buffer resource and the activation rules.  Every numeric rule of the project that a kernel applies to a
// single value lives here, once.  Device code only: kernels.h (which host translation units include) does not include this.
#pragma once

#include "kernels.h"

namespace sc {

typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef float float16_t __attribute__((ext_vector_type(16)));  // the accumulator of v_mfma_f32_32x32x16_f16
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef int i32x4_t __attribute__((ext_vector_type(4)));

// The split: x = hi + lo to about 22 bits, hi = fp16(x), lo = fp16(x - hi).  A product of a split operand with fp16 weights
// (or the three terms hi.hi + hi.lo + lo.hi of two split operands) accumulated in fp32 is the project's near-fp32 product.
__device__ __forceinline__ void split1(float x, _Float16& hi, _Float16& lo) {
    const _Float16 h = (_Float16)x;
    hi = h;
    lo = (_Float16)(x - (float)h);
}

__device__ __forceinline__ void split8(const float* x, half8_t& hi, half8_t& lo) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const _Float16 h = (_Float16)x[e];
        hi[e] = h;
        lo[e] = (_Float16)(x[e] - (float)h);
    }
}

__device__ __forceinline__ float wave_sum(float v) {  // over the 64 lanes, result in every lane
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Raw buffer resource over [base, base + bytes): stride 0, dword 3 as for every gfx9 raw buffer.  A load at offset OOB
// (>= num_records of every buffer used with it, all below 2 GB) returns zeros.
constexpr uint32_t OOB = 0x80000000u;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t raw_buffer_rsrc(const void* base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}

// ACT_GELU (kernels.h): the exact erf form of torch.nn.GELU(); erff(NaN) is NaN, so a NaN stays NaN.
__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f)); }

// ReLU that keeps NaN (fmaxf would answer 0): an overflowed row must stay visible.  -0 -> +0.
__device__ __forceinline__ float relu_keep_nan(float v) { return !(v <= 0.f) ? v : 0.f; }

// The activation switch (enum Act, kernels.h), compile-time and run-time.
template <int ACT>
__device__ __forceinline__ float act(float v) {
    if (ACT == ACT_RELU) return relu_keep_nan(v);
    if (ACT == ACT_SILU) return v / (1.f + expf(-v));
    if (ACT == ACT_TANH) return tanhf(v);
    if (ACT == ACT_GELU) return gelu_erf(v);
    return v;
}

__device__ __forceinline__ float act(float v, int a) {
    if (a == ACT_RELU) return relu_keep_nan(v);
    if (a == ACT_SILU) return v / (1.f + expf(-v));
    if (a == ACT_TANH) return tanhf(v);
    if (a == ACT_GELU) return gelu_erf(v);
    return v;
}

// The greedy step rules on the logits of one row (ArgmaxEpi, kernels.h), once for the three fused vocabulary projections and
// the finalize kernels.  A row's state is {best tweaked logit, its lowest index idx} and the online log-sum-exp {m, s} of the
// raw logits, empty as {-inf, 0x7fffffff, -inf, 0}; as a float4 record it is (best, idx bits, m, s).
// One logit v of feature `feat` (bias added; the caller keeps the raw EOS logit).  no_eos: the step is before
// min_step_for_eos; force: it is the forced-EOS step.
__device__ __forceinline__ void argmax_push(float& best, int& idx, float& m, float& s, float v, int feat, const ArgmaxEpi& e, bool no_eos,
                                            bool force) {
    if (v > m) {
        s = s * expf(m - v) + 1.f;
        m = v;
    } else {
        s += expf(v - m);
    }
    float tv = v;
    if (feat == e.unk_idx) tv -= e.unk_penalty;
    if (feat == e.pad_idx) tv = -INFINITY;
    if (no_eos && feat == e.eos_idx) tv = -INFINITY;
    if (force && feat != e.eos_idx) tv = -INFINITY;
    if (tv > best || (tv == best && feat < idx)) {
        best = tv;
        idx = feat;
    }
}
// another state (ob, oi, om, os) of the same row: by value then lower index; (max, sumexp) with the -inf guard
__device__ __forceinline__ void argmax_merge(float& best, int& idx, float& m, float& s, float ob, int oi, float om, float os) {
    if (ob > best || (ob == best && oi < idx)) {
        best = ob;
        idx = oi;
    }
    const float nm = fmaxf(m, om);
    const float a = (m == -INFINITY) ? 0.f : s * expf(m - nm);
    const float b = (om == -INFINITY) ? 0.f : os * expf(om - nm);
    s = a + b;
    m = nm;
}
__device__ __forceinline__ void argmax_merge_lane(float& best, int& idx, float& m, float& s, int o) {  // the lane at distance o
    const float ob = __shfl_xor(best, o);
    const int oi = __shfl_xor(idx, o);
    const float om = __shfl_xor(m, o);
    const float os = __shfl_xor(s, o);
    argmax_merge(best, idx, m, s, ob, oi, om, os);
}
// The records part[t * stride + b], t < tiles, of row b combined over a workgroup of 256 threads: valid in thread 0.
__device__ __forceinline__ void argmax_combine_records(const float4* __restrict__ part, int tiles, int stride, int b, float& best,
                                                       int& idx, float& m, float& s) {
    __shared__ float4 s_rec[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    best = -INFINITY, idx = 0x7fffffff, m = -INFINITY, s = 0.f;
    for (int t = tid; t < tiles; t += 256) {
        const float4 r = part[(int64_t)t * stride + b];
        argmax_merge(best, idx, m, s, r.x, __float_as_int(r.y), r.z, r.w);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) argmax_merge_lane(best, idx, m, s, o);
    if (lane == 0) s_rec[wave] = make_float4(best, __int_as_float(idx), m, s);
    __syncthreads();
    if (tid == 0)
        for (int w = 1; w < 4; ++w) argmax_merge(best, idx, m, s, s_rec[w].x, __float_as_int(s_rec[w].y), s_rec[w].z, s_rec[w].w);
}

}  // namespace sc
