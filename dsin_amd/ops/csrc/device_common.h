// Torch-free device helpers shared by the dsin_amd CDNA4 (gfx950) kernels.
// common.h adds the torch-side macros on top; kernel headers that must
// compile standalone (ncc_kernels.h) include this file alone.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

namespace dsin {

using bf16 = __hip_bfloat16;

__device__ __forceinline__ float b2f(bf16 v) { return __bfloat162float(v); }
__device__ __forceinline__ bf16 f2b(float v) { return __float2bfloat16(v); }

constexpr int WAVE = 64;

// MFMA operand / accumulator vectors and the 16-byte run of eight bf16 bits
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;
using u16x8 = __attribute__((ext_vector_type(8))) unsigned short;

// order-preserving encode of a float into uint32 (for packed atomic argmax)
__device__ __forceinline__ unsigned int float_flip(float f) {
  unsigned int u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float wave_reduce_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

}  // namespace dsin
