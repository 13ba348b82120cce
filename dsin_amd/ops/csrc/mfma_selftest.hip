// MFMA fragment-layout self-checks used by the GPU tests: one wave computes
// C = A @ B from fp32 operands rounded to bf16, with the lane/register
// mapping the kernels assume. 16x16x32 is the shape of the conv family
// (conv_kernels.h), 32x32x16 that of the NCC search (ncc_kernels.h).

#include "common.h"

namespace dsin {

// C = A(16x32) @ B(32x16)
__global__ void mfma_selftest_kernel(const float* __restrict__ A,
                                     const float* __restrict__ B,
                                     float* __restrict__ C) {
  int lane = threadIdx.x & 63;
  bf16x8 a, b;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    int k = (lane >> 4) * 8 + e;
    bf16 av = f2b(A[(lane & 15) * 32 + k]);   // A[row][k]
    bf16 bv = f2b(B[k * 16 + (lane & 15)]);   // B[k][col]
    a[e] = *reinterpret_cast<__bf16*>(&av);
    b[e] = *reinterpret_cast<__bf16*>(&bv);
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    int row = (lane >> 4) * 4 + reg, col = lane & 15;
    C[row * 16 + col] = acc[reg];
  }
}

torch::Tensor mfma_selftest(torch::Tensor A, torch::Tensor B) {
  CHECK_CUDA_CONTIG(A);
  CHECK_CUDA_CONTIG(B);
  auto C = torch::empty({16, 16}, A.options());
  hipLaunchKernelGGL(mfma_selftest_kernel, dim3(1), dim3(64), 0,
                     at::cuda::getCurrentCUDAStream(), A.data_ptr<float>(),
                     B.data_ptr<float>(), C.data_ptr<float>());
  return C;
}

// C = A(32x16) @ B(16x32)
__global__ void mfma32_selftest_kernel(const float* __restrict__ A,
                                       const float* __restrict__ B,
                                       float* __restrict__ C) {
  int lane = threadIdx.x & 63;
  bf16x8 a, b;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    int k = (lane >> 5) * 8 + e;
    bf16 av = f2b(A[(lane & 31) * 16 + k]);   // A[row][k]
    bf16 bv = f2b(B[k * 32 + (lane & 31)]);   // B[k][col]
    a[e] = *reinterpret_cast<__bf16*>(&av);
    b[e] = *reinterpret_cast<__bf16*>(&bv);
  }
  f32x16 acc = {};
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    int row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
    int col = lane & 31;
    C[row * 32 + col] = acc[reg];
  }
}

torch::Tensor mfma32_selftest(torch::Tensor A, torch::Tensor B) {
  CHECK_CUDA_CONTIG(A);
  CHECK_CUDA_CONTIG(B);
  auto C = torch::empty({32, 32}, A.options());
  hipLaunchKernelGGL(mfma32_selftest_kernel, dim3(1), dim3(64), 0,
                     at::cuda::getCurrentCUDAStream(), A.data_ptr<float>(),
                     B.data_ptr<float>(), C.data_ptr<float>());
  return C;
}

}  // namespace dsin
