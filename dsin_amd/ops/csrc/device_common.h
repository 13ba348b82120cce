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

// one lane of a u16x8 run as a float, and back
__device__ __forceinline__ float b2f(unsigned short u) {
  return b2f(*reinterpret_cast<bf16*>(&u));
}
__device__ __forceinline__ unsigned short f2bits(float v) {
  bf16 h = f2b(v);
  return *reinterpret_cast<unsigned short*>(&h);
}

// element load / store in fp32 for kernels templated on fp32 or bf16 data
__device__ __forceinline__ float ld_f32(const float* p, long long i) {
  return p[i];
}
__device__ __forceinline__ float ld_f32(const bf16* p, long long i) {
  return b2f(p[i]);
}
__device__ __forceinline__ void st_f32(float* p, long long i, float v) {
  p[i] = v;
}
__device__ __forceinline__ void st_f32(bf16* p, long long i, float v) {
  p[i] = f2b(v);
}

constexpr int WAVE = 64;
// workgroup size of the pointwise and reduction kernels
constexpr int BLOCK_THREADS = 256;
constexpr int BLOCK_WAVES = BLOCK_THREADS / WAVE;

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

// Block sum of n <= N values over a BLOCK_THREADS workgroup, up to the last
// step: wave reduce, one LDS slot per wave and value, one barrier. Returns
// the slots, s[k * BLOCK_WAVES + w] = sum of v[k] over wave w, readable by
// every thread. The caller adds the four wave values with sum4_serial or
// sum4_pairwise and writes the result with a plain store: the order is
// part of the result's bits, and fixed (docs/KERNELS.md, determinism).
template <int N>
__device__ __forceinline__ const float* block_wave_sums(const float (&v)[N],
                                                        int n = N) {
  __shared__ float slots[N * BLOCK_WAVES];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    if (k >= n) break;
    const float w = wave_reduce_sum(v[k]);
    if ((threadIdx.x & (WAVE - 1)) == 0)
      slots[k * BLOCK_WAVES + (threadIdx.x / WAVE)] = w;
  }
  __syncthreads();
  return slots;
}

static_assert(BLOCK_WAVES == 4, "sum4_* add exactly four wave values");
__device__ __forceinline__ float sum4_serial(const float* w) {
  return w[0] + w[1] + w[2] + w[3];
}
__device__ __forceinline__ float sum4_pairwise(const float* w) {
  return (w[0] + w[1]) + (w[2] + w[3]);
}

// Activation codes of the BN and conv epilogues: 0 none, 1 ReLU, 2 leaky 0.2
__device__ __forceinline__ float act_fwd(float v, int act) {
  if (act == 1) return fmaxf(v, 0.f);
  if (act == 2) return fmaxf(v, 0.2f * v);
  return v;
}

// g * act'(.), read off the sign of the post-activation output
__device__ __forceinline__ float act_grad(float g, float out, int act) {
  if (act == 1) return out > 0.f ? g : 0.f;
  if (act == 2) return out > 0.f ? g : 0.2f * g;
  return g;
}

}  // namespace dsin
