// Fused pad / zero-stuff / quantize launch of the fp8 conv path: builds the
// e4m3 conv input buffer (zero border, optional stride-S zero-stuffing for
// transposed convs) in ONE pass from an fp32 or bf16 NCHW tensor (kernel in
// conv_fp8.h). The bf16 convs pad virtually and need no buffer.
// The output buffer carries 16 elements of tail slack for the conv staging
// vector reads (see ops/conv.py).

#include "common.h"
#include "conv_fp8.h"

namespace dsin {

torch::Tensor pad_stuff_e4m3(torch::Tensor x, int64_t pt, int64_t pb,
                             int64_t pl, int64_t pr, int64_t stride) {
  CHECK_CUDA_CONTIG(x);
  TORCH_CHECK(x.dim() == 4, "pad_stuff_e4m3 expects NCHW");
  const int B = (int)x.size(0), C = (int)x.size(1);
  const int H = (int)x.size(2), W = (int)x.size(3);
  const int Hs = (H - 1) * (int)stride + 1, Ws = (W - 1) * (int)stride + 1;
  const int Hp = Hs + (int)(pt + pb), Wp = Ws + (int)(pl + pr);
  const long long n_img = (long long)C * Hp * Wp;
  auto store = torch::empty({(int64_t)B * n_img + 16},
                            x.options().dtype(torch::kByte));
  auto out = store.narrow(0, 0, B * n_img).view({B, C, Hp, Wp});
  long long total = (long long)B * n_img;
  auto stream = at::cuda::getCurrentCUDAStream();
  dispatch_f32_bf16(x, "pad_stuff_e4m3: x", [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((pad_stuff_fp8_kernel<T>), dim3(ew_grid(total, 8192)),
                       dim3(256), 0, stream, ptr<const T>(x), ptr<f8>(out), C,
                       H, W, Hp, Wp, (int)pt, (int)pl, (int)stride, n_img,
                       (long long)C * H * W, B);
  });
  return out;
}

}  // namespace dsin
