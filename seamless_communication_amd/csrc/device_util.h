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

}  // namespace sc
