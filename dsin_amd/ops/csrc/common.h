// Shared helpers for the dsin_amd CDNA4 (gfx950) kernels.
#pragma once

#include "device_common.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#define DSIN_CHECK_HIP(expr)                                                   \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    TORCH_CHECK(_e == hipSuccess, "HIP error: ", hipGetErrorString(_e));       \
  } while (0)

#define CHECK_CUDA_CONTIG(t)                                                   \
  TORCH_CHECK((t).is_cuda() && (t).is_contiguous(), #t " must be contiguous on GPU")

namespace dsin {

inline dim3 grid1d(int64_t n, int block) {
  return dim3(static_cast<unsigned int>((n + block - 1) / block));
}

}  // namespace dsin
