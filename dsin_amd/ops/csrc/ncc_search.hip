// Streaming side-information NCC search for CDNA4 (gfx950) — host wrapper.
//
// Reference semantics (/root/reference/src/siFinder.py:7-135,
// src/siFull_img.py:5-68, mask from src/AE.py:49,193-220): every
// non-overlapping (ph, pw) patch of the decoded image x is Pearson-correlated
// against every location of the decoded side image y (both fixed-normalized
// and H1H2H3-decorrelated), the correlation is weighted by a per-patch
// Gaussian location prior, the argmax location is found, and the winning
// patches are gathered FROM THE ORIGINAL y and scattered into y_syn.
//
// The reference materializes the (Hc, Wc, P) correlation volume and an
// equally-sized mask constant (~722 MB each at 320x960). This implementation
// streams: the correlation xy[p,i,j] is an implicit GEMM
// (M = P patches, N = Hc*Wc locations, K = 3*ph*pw) on bf16 MFMA
// (32x32x16, fp32 accumulate); Pearson normalization, the Gaussian prior
// (evaluated inline, never materialized) and a packed-u64 atomic argmax with
// TF tie semantics (smallest index wins) live in the epilogue. Device code in
// ncc_kernels.h (torch-free, compilable standalone for .s inspection).
//
// L2+LAB mode (use_L2andLAB; reference src/siFinder.py:13-31, 102-103,
// 145-195): the operands are the CIELAB transform of the raw images (bf16),
// the score is the squared distance sum_x2 - 2*xy + sum_y2 times the same
// prior, and the winner is the argmin, first index on ties. Same pipeline;
// only the transform kernel and the main-kernel instantiation differ.
//
// The batch is the only form below the Python API: B images of one geometry
// go through one launch per stage (one image is B = 1), every intermediate is
// one allocation with a leading B, and the image index is a grid dimension
// (strides at the head of ncc_kernels.h). Scores, keys and ties are per image
// and do not depend on B.

#include "common.h"
#include "ncc_kernels.h"

namespace dsin {

// gridDim.y and gridDim.z hold at most 65535 blocks
constexpr int64_t NCC_GRID_YZ_MAX = 65535;

template <bool L2>
static std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> ncc_search_impl(
    torch::Tensor x_dec, torch::Tensor y_dec, torch::Tensor y_orig,
    int64_t ph_, int64_t pw_, bool use_mask) {
  CHECK_CUDA_CONTIG(x_dec);
  CHECK_CUDA_CONTIG(y_dec);
  CHECK_CUDA_CONTIG(y_orig);
  TORCH_CHECK(x_dec.dim() == 4 && x_dec.size(0) >= 1 && x_dec.size(1) == 3,
              "x_dec must be (B,3,H,W) with B >= 1");
  TORCH_CHECK(x_dec.sizes() == y_dec.sizes() && x_dec.sizes() == y_orig.sizes(),
              "x/y size mismatch (equal sizes required)");
  const int ph = (int)ph_, pw = (int)pw_;
  const int64_t B = x_dec.size(0);
  const int H = (int)x_dec.size(2), W = (int)x_dec.size(3);
  TORCH_CHECK(H % ph == 0 && W % pw == 0, "image must tile by the patch size");
  const int gh = H / ph, gw = W / pw, P = gh * gw;
  // The image is blockIdx.y of the small kernels and the slow part of the
  // main kernels' blockIdx.z, next to the patch tiles.
  const int64_t ptiles = (P + NCC_TP - 1) / NCC_TP;
  const int64_t maxB = NCC_GRID_YZ_MAX / ptiles;
  // blockIdx.z / ptiles as a multiply and a shift (ncc_enter_image)
  const unsigned long long zmagic =
      (1ull << 32) / (unsigned long long)ptiles + 1;
  TORCH_CHECK(B <= maxB, "ncc_search: a batch of ", B, " images of ", P,
              " patches needs ", B * ptiles, " blocks in grid z; at most ",
              NCC_GRID_YZ_MAX, " fit, so the largest batch at this geometry is ",
              maxB);
  const int Hc = H - ph + 1, Wc = W - pw + 1;
  const int K = 3 * ph * pw;
  // v2 (pw % 8 == 0, the default geometry): k-sliced LDS A-tile + direct
  // global B loads — see ncc_main_v2_kernel. The koffs table is laid out for
  // v1's y window in either case.
  const bool v2 = (pw % 8) == 0;
  const NccLdsV1 l1 = ncc_lds_v1(ph, pw);
  const int YR = l1.YR, YCP = l1.YCP;
  const size_t lds = v2 ? ncc_lds_v2(ph, pw).bytes : l1.bytes;
  TORCH_CHECK(lds <= 160 * 1024, "patch size too large for LDS tiling: ", lds);
  TORCH_CHECK(v2 || 3 * YR * YCP < 65536, "y-window exceeds u16 offset range");

  auto optsF = x_dec.options();
  auto stream = at::cuda::getCurrentCUDAStream();

  auto aoffs = torch::empty({K}, optsF.dtype(torch::kUInt32));
  auto koffs = torch::empty({K}, optsF.dtype(torch::kUInt16));
  hipLaunchKernelGGL(ncc_offsets_kernel, grid1d(K, 256), dim3(256), 0, stream,
                     (unsigned int*)aoffs.data_ptr(),
                     (unsigned short*)koffs.data_ptr(), H, W, ph, pw, YR, YCP,
                     K);

  const unsigned int nb = (unsigned int)B;
  // grid of a one-thread-per-element stage: x over the elements of one
  // image, y the image
  const auto grid_img = [nb](int64_t n) {
    return dim3(grid1d(n, 256).x, nb);
  };

  auto t_x = torch::empty({B, 3, H, W}, optsF.dtype(torch::kBFloat16));
  // The images lie back to back, then 192 elements of tail slack: the v2
  // kernel's invalid-column vector loads may overshoot the last row of an
  // image. Past image b < B-1 they land in image b+1, past the last image in
  // the slack; either way the jvalid select of the epilogue discards what
  // they read, so the slack is needed once, not per image.
  auto t_y = torch::empty({B * 3 * H * W + 192},
                          optsF.dtype(torch::kBFloat16));
  int64_t hw = (int64_t)H * W;
  const auto transform = L2 ? lab_transform_kernel : transform_kernel;
  hipLaunchKernelGGL(transform, grid_img(hw), dim3(256), 0, stream,
                     x_dec.data_ptr<float>(), (bf16*)t_x.data_ptr(), hw);
  hipLaunchKernelGGL(transform, grid_img(hw), dim3(256), 0, stream,
                     y_dec.data_ptr<float>(), (bf16*)t_y.data_ptr(), hw);

  auto psum = torch::empty({B, P}, optsF);
  auto psum2 = torch::empty({B, P}, optsF);
  hipLaunchKernelGGL(patch_stats_kernel, dim3(P, nb), dim3(64), 0, stream,
                     (const bf16*)t_x.data_ptr(),
                     (const unsigned int*)aoffs.data_ptr(),
                     psum.data_ptr<float>(), psum2.data_ptr<float>(), H, W, ph,
                     pw, gw, K);

  auto s1 = torch::empty({B, (int64_t)H * Wc}, optsF);
  auto s2 = torch::empty({B, (int64_t)H * Wc}, optsF);
  auto sy = torch::empty({B, (int64_t)Hc * Wc}, optsF);
  auto sy2 = torch::empty({B, (int64_t)Hc * Wc}, optsF);
  hipLaunchKernelGGL(ysum_row_kernel, grid_img((int64_t)H * Wc), dim3(256),
                     0, stream, (const bf16*)t_y.data_ptr(),
                     s1.data_ptr<float>(), s2.data_ptr<float>(), H, W, pw, Wc);
  hipLaunchKernelGGL(ysum_col_kernel, grid_img((int64_t)Hc * Wc), dim3(256),
                     0, stream, s1.data_ptr<float>(), s2.data_ptr<float>(),
                     sy.data_ptr<float>(), sy2.data_ptr<float>(), Hc, Wc, ph);

  auto best = torch::zeros({B, P}, optsF.dtype(torch::kInt64));  // u64 keys
  const int tj = v2 ? NCC_TJ2 : NCC_TJ;
  dim3 grid((Wc + tj - 1) / tj, (Hc + NCC_TI - 1) / NCC_TI,
            (unsigned int)(B * ptiles));
  if (v2) {
    hipLaunchKernelGGL(ncc_main_v2_kernel<L2>, grid, dim3(256), lds, stream,
                       (const bf16*)t_x.data_ptr(),
                       (const bf16*)t_y.data_ptr(),
                       (const unsigned int*)aoffs.data_ptr(),
                       psum.data_ptr<float>(), psum2.data_ptr<float>(),
                       sy.data_ptr<float>(), sy2.data_ptr<float>(),
                       (unsigned long long*)best.data_ptr(), H, W, ph, pw,
                       gw, P, Hc, Wc, use_mask ? 1 : 0, zmagic);
  } else {
    hipLaunchKernelGGL(ncc_main_kernel<L2>, grid, dim3(256), lds, stream,
                       (const bf16*)t_x.data_ptr(),
                       (const bf16*)t_y.data_ptr(),
                       (const unsigned int*)aoffs.data_ptr(),
                       (const unsigned short*)koffs.data_ptr(),
                       psum.data_ptr<float>(), psum2.data_ptr<float>(),
                       sy.data_ptr<float>(), sy2.data_ptr<float>(),
                       (unsigned long long*)best.data_ptr(), H, W, ph, pw,
                       gw, P, Hc, Wc, use_mask ? 1 : 0, zmagic);
  }
  // a refused launch (e.g. the dynamic LDS request) would leave `best` zero,
  // and scatter_kernel would decode index 0xFFFFFFFF from it
  {
    const hipError_t err = hipGetLastError();
    TORCH_CHECK(err == hipSuccess, "ncc_search: launch of ",
                v2 ? "ncc_main_v2_kernel" : "ncc_main_kernel",
                L2 ? "<L2>" : "", " with ", lds,
                " bytes of dynamic LDS failed: ", hipGetErrorString(err));
  }

  auto y_syn = torch::empty_like(y_orig);
  auto rows = torch::empty({B, P}, optsF.dtype(torch::kInt64));
  auto cols = torch::empty({B, P}, optsF.dtype(torch::kInt64));
  hipLaunchKernelGGL(scatter_kernel, dim3(P, nb), dim3(256), 0, stream,
                     (const unsigned long long*)best.data_ptr(),
                     y_orig.data_ptr<float>(), y_syn.data_ptr<float>(),
                     (long long*)rows.data_ptr<int64_t>(),
                     (long long*)cols.data_ptr<int64_t>(), H, W, ph, pw, gw, P,
                     Wc);
  return {y_syn, rows, cols};
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> ncc_search(
    torch::Tensor x_dec, torch::Tensor y_dec, torch::Tensor y_orig,
    int64_t ph, int64_t pw, bool use_mask) {
  return ncc_search_impl<false>(x_dec, y_dec, y_orig, ph, pw, use_mask);
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> ncc_search_l2lab(
    torch::Tensor x_dec, torch::Tensor y_dec, torch::Tensor y_orig,
    int64_t ph, int64_t pw, bool use_mask) {
  return ncc_search_impl<true>(x_dec, y_dec, y_orig, ph, pw, use_mask);
}

// The bf16 LAB operands of the L2+LAB search, fp32 -> bf16 of the same shape,
// (3,H,W) or (B,3,H,W): what the tests' oracle needs (the device powf/cbrtf
// are not bit-identical to the host's).
torch::Tensor ncc_lab_transform(torch::Tensor img) {
  CHECK_CUDA_CONTIG(img);
  const int64_t d = img.dim();
  TORCH_CHECK((d == 3 || d == 4) && img.size(d - 3) == 3,
              "img must be (3,H,W) or (B,3,H,W)");
  TORCH_CHECK(img.scalar_type() == torch::kFloat32, "img must be fp32");
  const int64_t B = d == 4 ? img.size(0) : 1;
  TORCH_CHECK(B <= NCC_GRID_YZ_MAX, "ncc_lab_transform: at most ",
              NCC_GRID_YZ_MAX, " images in one call, got ", B);
  auto out = torch::empty_like(img, img.options().dtype(torch::kBFloat16));
  const int64_t hw = img.size(d - 2) * img.size(d - 1);
  if (hw > 0 && B > 0)
    hipLaunchKernelGGL(lab_transform_kernel,
                       dim3(grid1d(hw, 256).x, (unsigned int)B), dim3(256), 0,
                       at::cuda::getCurrentCUDAStream(),
                       img.data_ptr<float>(), (bf16*)out.data_ptr(), hw);
  return out;
}

}  // namespace dsin
