// Fused elementwise/reduction kernels for the eager-torch remainder
// (round-1 verdict item 6): heatmap construction +
// bottleneck masking, L1-distortion partial sums, and the H_real/H_mask
// rate-term sums. Each replaces a 3-8 kernel torch chain (with full-tensor
// temporaries) by one kernel + one ordered partial-sum reduce, and every
// reduction is deterministic (plain per-block partial stores, host-side
// at::sum in fixed order).

#include "common.h"

namespace dsin {

// ---------------------------------------------------------------- heatmap
// Reference src/autoencoder_imgcomp.py:172-201:
//   heatmap2D = sigmoid(b[:,0]) * C;  h3[.,c] = clamp(heatmap2D - c, 0, 1)
//   z = h3 * b[:, 1:]
// One thread per (n, h, w): computes the sigmoid once, loops the C channels.
template <typename T>
__global__ void heatmap_mask_fwd_kernel(const T* __restrict__ b,
                                        T* __restrict__ z,
                                        T* __restrict__ h3,
                                        int C, long long HW, int N) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = (long long)N * HW;
  const long long gstride = (long long)gridDim.x * blockDim.x;
  for (; i < total; i += gstride) {
    const long long n = i / HW, hw = i % HW;
    const T* bn = b + (n * (C + 1)) * HW + hw;
    const float h2 = (1.f / (1.f + __expf(-ld_f32(bn, 0)))) * (float)C;
    T* zn = z + (n * C) * HW + hw;
    T* hn = h3 + (n * C) * HW + hw;
    for (int c = 0; c < C; ++c) {
      const float h = fminf(fmaxf(h2 - (float)c, 0.f), 1.f);
      st_f32(hn, (long long)c * HW, h);
      st_f32(zn, (long long)c * HW, h * ld_f32(bn, (long long)(c + 1) * HW));
    }
  }
}

// backward: g_b[:,0] = C * s * (1 - s) * sum_c (g_z[c]*b[c+1] + g_h3[c])
//                     * 1{0 <= h2 - c <= 1}   (torch clamp grad semantics)
//           g_b[:,c+1] = g_z[c] * h3[c]
template <typename T>
__global__ void heatmap_mask_bwd_kernel(const T* __restrict__ b,
                                        const T* __restrict__ gz,
                                        const T* __restrict__ gh3,
                                        T* __restrict__ gb,
                                        int C, long long HW, int N) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = (long long)N * HW;
  const long long gstride = (long long)gridDim.x * blockDim.x;
  for (; i < total; i += gstride) {
    const long long n = i / HW, hw = i % HW;
    const T* bn = b + (n * (C + 1)) * HW + hw;
    const T* gzn = gz + (n * C) * HW + hw;
    const T* ghn = gh3 ? gh3 + (n * C) * HW + hw : nullptr;
    T* gbn = gb + (n * (C + 1)) * HW + hw;
    const float s = 1.f / (1.f + __expf(-ld_f32(bn, 0)));
    const float h2 = s * (float)C;
    float acc = 0.f;
    for (int c = 0; c < C; ++c) {
      const float v = h2 - (float)c;
      const float h = fminf(fmaxf(v, 0.f), 1.f);
      const float gzc = ld_f32(gzn, (long long)c * HW);
      st_f32(gbn, (long long)(c + 1) * HW, gzc * h);
      if (v >= 0.f && v <= 1.f) {
        float g = gzc * ld_f32(bn, (long long)(c + 1) * HW);
        if (ghn) g += ld_f32(ghn, (long long)c * HW);
        acc += g;
      }
    }
    st_f32(gbn, 0, acc * (float)C * s * (1.f - s));
  }
}

// ---------------------------------------------------------------- L1 mean
// Per-image |y - x| partial sums: parts[n][s] (plain stores, one ordered
// at::sum per image on the host). x and y may differ in dtype.
template <typename TX, typename TY>
__global__ void l1_part_kernel(const TX* __restrict__ x,
                               const TY* __restrict__ y,
                               float* __restrict__ parts,
                               long long CHW, int S) {
  const int n = blockIdx.y;
  const int s = blockIdx.x;
  const TX* xn = x + (long long)n * CHW;
  const TY* yn = y + (long long)n * CHW;
  float a[1] = {0.f};
  for (long long i = (long long)s * blockDim.x + threadIdx.x; i < CHW;
       i += (long long)S * blockDim.x)
    a[0] += fabsf(ld_f32(yn, i) - ld_f32(xn, i));
  const float* ws = block_wave_sums(a);
  if (threadIdx.x == 0) parts[(long long)n * S + s] = sum4_serial(ws);
}

// backward: g per image scalar; gx = -sign(y-x)*g, gy = +sign(y-x)*g
template <typename TX, typename TY>
__global__ void l1_bwd_kernel(const TX* __restrict__ x,
                              const TY* __restrict__ y,
                              const float* __restrict__ g,  // (N,)
                              TX* __restrict__ gx,          // nullable
                              TY* __restrict__ gy,          // nullable
                              long long CHW, int N) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = (long long)N * CHW;
  const long long gstride = (long long)gridDim.x * blockDim.x;
  for (; i < total; i += gstride) {
    const long long n = i / CHW;
    const float d = ld_f32(y, i) - ld_f32(x, i);
    const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    const float gv = sg * g[n];
    if (gy) st_f32(gy, i, gv);
    if (gx) st_f32(gx, i, -gv);
  }
}

// ------------------------------------------------------------- rate terms
// parts[s] = (sum bc, sum bc*heat) over slice s — one pass instead of two
// full-tensor reads (H_real and H_mask, Distortions_imgcomp.py:118-124).
__global__ void hterms_part_kernel(const float* __restrict__ bc,
                                   const bf16* __restrict__ heat,
                                   float* __restrict__ parts,  // (S, 2)
                                   long long n, int S) {
  const int s = blockIdx.x;
  float acc[2] = {0.f, 0.f};
  for (long long i = (long long)s * blockDim.x + threadIdx.x; i < n;
       i += (long long)S * blockDim.x) {
    const float v = bc[i];
    acc[0] += v;
    acc[1] += v * ld_f32(heat, i);
  }
  const float* ws = block_wave_sums(acc);
  if (threadIdx.x == 0) {
    parts[(long long)s * 2] = sum4_serial(ws);
    parts[(long long)s * 2 + 1] = sum4_serial(ws + BLOCK_WAVES);
  }
}

// backward: g_bc = g1/n + g2/n * heat ; g_heat = g2/n * bc
__global__ void hterms_bwd_kernel(const float* __restrict__ bc,
                                  const bf16* __restrict__ heat,
                                  const float* __restrict__ g2v,  // (2,)
                                  float* __restrict__ gbc,
                                  bf16* __restrict__ gheat,
                                  long long n, float invn) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long gstride = (long long)gridDim.x * blockDim.x;
  const float g1 = g2v[0] * invn, g2 = g2v[1] * invn;
  for (; i < n; i += gstride) {
    gbc[i] = g1 + g2 * ld_f32(heat, i);
    if (gheat) st_f32(gheat, i, g2 * bc[i]);
  }
}

// ------------------------------------------------------------------ hosts

std::vector<torch::Tensor> heatmap_mask_fwd(torch::Tensor b) {
  CHECK_CUDA_CONTIG(b);
  TORCH_CHECK(b.dim() == 4 && b.size(1) >= 1,
              "heatmap_mask_fwd: b must be (N, C+1, H, W)");
  const int N = (int)b.size(0), C1 = (int)b.size(1);
  const long long HW = (long long)b.size(2) * b.size(3);
  auto z = torch::empty({N, C1 - 1, b.size(2), b.size(3)}, b.options());
  auto h3 = torch::empty_like(z);
  const int grid = ew_grid((long long)N * HW);
  auto stream = at::cuda::getCurrentCUDAStream();
  dispatch_f32_bf16(b, "heatmap_mask_fwd: b", [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((heatmap_mask_fwd_kernel<T>), dim3(grid),
                       dim3(BLOCK_THREADS), 0, stream, ptr<const T>(b),
                       ptr<T>(z), ptr<T>(h3), C1 - 1, HW, N);
  });
  return {z, h3};
}

torch::Tensor heatmap_mask_bwd(torch::Tensor b, torch::Tensor gz,
                               c10::optional<torch::Tensor> gh3) {
  CHECK_CUDA_CONTIG(b);
  TORCH_CHECK(b.dim() == 4 && b.size(1) >= 1,
              "heatmap_mask_bwd: b must be (N, C+1, H, W)");
  const int N = (int)b.size(0), C1 = (int)b.size(1);
  const long long HW = (long long)b.size(2) * b.size(3);
  // the kernel reads gz and gh3 in the dtype of b
  const std::vector<int64_t> zshape = {N, C1 - 1, b.size(2), b.size(3)};
  check_arg_shape(gz, "heatmap_mask_bwd: gz", b.scalar_type(), zshape);
  if (gh3.has_value())
    check_arg_shape(*gh3, "heatmap_mask_bwd: gh3", b.scalar_type(), zshape);
  auto gb = torch::empty_like(b);
  const int grid = ew_grid((long long)N * HW);
  auto stream = at::cuda::getCurrentCUDAStream();
  dispatch_f32_bf16(b, "heatmap_mask_bwd: b", [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((heatmap_mask_bwd_kernel<T>), dim3(grid),
                       dim3(BLOCK_THREADS), 0, stream, ptr<const T>(b),
                       ptr<const T>(gz),
                       gh3.has_value() ? ptr<const T>(*gh3) : nullptr,
                       ptr<T>(gb), C1 - 1, HW, N);
  });
  return gb;
}

static int _l1_slices(long long CHW) {
  return (int)std::min<long long>(std::max<long long>(CHW / (256 * 16), 1),
                                  64);
}

torch::Tensor l1_part(torch::Tensor x, torch::Tensor y) {
  CHECK_CUDA_CONTIG(x);
  CHECK_CUDA_CONTIG(y);
  TORCH_CHECK(x.dim() >= 1 && x.sizes() == y.sizes(),
              "l1_part: x and y must have one shape");
  const int N = (int)x.size(0);
  const long long CHW = x.numel() / N;
  const int S = _l1_slices(CHW);
  auto parts = torch::empty({N, S}, x.options().dtype(torch::kFloat32));
  auto stream = at::cuda::getCurrentCUDAStream();
  dispatch_f32_bf16(x, "l1_part: x", [&](auto tx) {
    dispatch_f32_bf16(y, "l1_part: y", [&](auto ty) {
      using TX = decltype(tx);
      using TY = decltype(ty);
      hipLaunchKernelGGL((l1_part_kernel<TX, TY>), dim3(S, N),
                         dim3(BLOCK_THREADS), 0, stream, ptr<const TX>(x),
                         ptr<const TY>(y), parts.data_ptr<float>(), CHW, S);
    });
  });
  return parts;
}

std::vector<torch::Tensor> l1_bwd(torch::Tensor x, torch::Tensor y,
                                  torch::Tensor g, bool need_gx,
                                  bool need_gy) {
  CHECK_CUDA_CONTIG(x);
  CHECK_CUDA_CONTIG(y);
  TORCH_CHECK(x.dim() >= 1 && x.sizes() == y.sizes(),
              "l1_bwd: x and y must have one shape");
  const int N = (int)x.size(0);
  check_arg_numel(g, "l1_bwd: g", torch::kFloat32, N);
  const long long CHW = x.numel() / N;
  auto gx = need_gx ? torch::empty_like(x) : torch::Tensor();
  auto gy = need_gy ? torch::empty_like(y) : torch::Tensor();
  const int grid = ew_grid(x.numel());
  auto stream = at::cuda::getCurrentCUDAStream();
  dispatch_f32_bf16(x, "l1_bwd: x", [&](auto tx) {
    dispatch_f32_bf16(y, "l1_bwd: y", [&](auto ty) {
      using TX = decltype(tx);
      using TY = decltype(ty);
      hipLaunchKernelGGL((l1_bwd_kernel<TX, TY>), dim3(grid),
                         dim3(BLOCK_THREADS), 0, stream, ptr<const TX>(x),
                         ptr<const TY>(y), g.data_ptr<float>(),
                         need_gx ? ptr<TX>(gx) : nullptr,
                         need_gy ? ptr<TY>(gy) : nullptr, CHW, N);
    });
  });
  return {gx, gy};
}

torch::Tensor hterms_part(torch::Tensor bc, torch::Tensor heat) {
  check_arg(bc, "hterms_part: bc", torch::kFloat32);
  check_arg_numel(heat, "hterms_part: heat", torch::kBFloat16, bc.numel());
  const long long n = bc.numel();
  const int S = _l1_slices(n);
  auto parts = torch::empty({S, 2}, bc.options());
  hipLaunchKernelGGL(hterms_part_kernel, dim3(S), dim3(BLOCK_THREADS), 0,
                     at::cuda::getCurrentCUDAStream(), bc.data_ptr<float>(),
                     ptr<const bf16>(heat), parts.data_ptr<float>(), n, S);
  return parts;
}

std::vector<torch::Tensor> hterms_bwd(torch::Tensor bc, torch::Tensor heat,
                                      torch::Tensor g2, bool need_gheat) {
  check_arg(bc, "hterms_bwd: bc", torch::kFloat32);
  check_arg_numel(heat, "hterms_bwd: heat", torch::kBFloat16, bc.numel());
  check_arg_numel(g2, "hterms_bwd: g2", torch::kFloat32, 2);
  const long long n = bc.numel();
  auto gbc = torch::empty_like(bc);
  auto gheat = need_gheat ? torch::empty_like(heat) : torch::Tensor();
  hipLaunchKernelGGL(hterms_bwd_kernel, dim3(ew_grid(n)),
                     dim3(BLOCK_THREADS), 0, at::cuda::getCurrentCUDAStream(),
                     bc.data_ptr<float>(), ptr<const bf16>(heat),
                     g2.data_ptr<float>(), gbc.data_ptr<float>(),
                     need_gheat ? ptr<bf16>(gheat) : nullptr, n,
                     1.f / (float)n);
  return {gbc, gheat};
}

}  // namespace dsin
