// Shared helpers for the dsin_amd CDNA4 (gfx950) kernels.
#pragma once

#include "device_common.h"
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#define CHECK_CUDA_CONTIG(t)                                                   \
  TORCH_CHECK((t).is_cuda() && (t).is_contiguous(), #t " must be contiguous on GPU")

namespace dsin {

inline dim3 grid1d(int64_t n, int block) {
  return dim3(static_cast<unsigned int>((n + block - 1) / block));
}

// grid of a grid-stride elementwise kernel: one BLOCK_THREADS block per 256
// elements, at most `cap` blocks
inline int ew_grid(int64_t total, int cap = 4096) {
  return (int)std::min<int64_t>((total + BLOCK_THREADS - 1) / BLOCK_THREADS,
                                cap);
}

// What an entry point asks of a tensor before it takes a pointer from it: on
// the GPU, contiguous, of this dtype. `what` is "op: argument".
inline void check_arg(const torch::Tensor& t, const char* what,
                      torch::ScalarType dtype) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous(), what,
              " must be contiguous on GPU");
  TORCH_CHECK(t.scalar_type() == dtype, what, " must be ", dtype, ", got ",
              t.scalar_type());
}
// ... and of this element count
inline void check_arg_numel(const torch::Tensor& t, const char* what,
                            torch::ScalarType dtype, int64_t numel) {
  check_arg(t, what, dtype);
  TORCH_CHECK(t.numel() == numel, what, " must have ", numel,
              " elements, got ", t.numel());
}
// ... or of this shape
inline void check_arg_shape(const torch::Tensor& t, const char* what,
                            torch::ScalarType dtype, c10::IntArrayRef shape) {
  check_arg(t, what, dtype);
  TORCH_CHECK(t.sizes() == shape, what, " must have shape ", shape, ", got ",
              t.sizes());
}

// Calls f with a value of the tensor's element type, float or bf16:
//   dispatch_f32_bf16(x, "op: x", [&](auto tag) { using T = decltype(tag); });
// Any other dtype is an error naming `what`. Nest it for two tensors.
template <typename F>
inline void dispatch_f32_bf16(const torch::Tensor& t, const char* what,
                              F&& f) {
  if (t.scalar_type() == torch::kFloat32) {
    f(float{});
  } else {
    TORCH_CHECK(t.scalar_type() == torch::kBFloat16, what,
                " must be fp32 or bf16, got ", t.scalar_type());
    f(bf16{});
  }
}

// typed pointer of a tensor already checked or dispatched on
template <typename T>
inline T* ptr(const torch::Tensor& t) {
  return static_cast<T*>(t.data_ptr());
}

}  // namespace dsin
