// Host wrappers for the implicit-GEMM conv family (device code in
// conv_kernels.h). See dsin_amd/ops/conv.py for the autograd layer and the
// geometry-to-table mapping.

#include "common.h"
#include "conv_kernels.h"
#define DSIN_CONV_FP8_KERNELS
#include "conv_fp8.h"

namespace dsin {

std::tuple<torch::Tensor, torch::Tensor> conv_tables(
    int64_t M, int64_t K, int64_t WO, int64_t stride, int64_t dil, int64_t Wp,
    int64_t HpWp, int64_t kh, int64_t kw, torch::Device device) {
  auto opts = torch::TensorOptions().device(device).dtype(torch::kInt32);
  auto mbase = torch::empty({M}, opts);
  auto koff = torch::empty({K}, opts);
  int64_t n = std::max(M, K);
  hipLaunchKernelGGL(conv_tables_kernel, grid1d(n, 256), dim3(256), 0,
                     at::cuda::getCurrentCUDAStream(),
                     mbase.data_ptr<int>(), koff.data_ptr<int>(), (int)M,
                     (int)K, (int)WO, (int)stride, (int)dil, (int)Wp,
                     (int)HpWp, (int)(kh * kw), (int)kw);
  return {mbase, koff};
}

std::tuple<torch::Tensor, torch::Tensor> conv_tables_v2(
    int64_t M, int64_t K, int64_t WO, int64_t stride, int64_t dil, int64_t kh,
    int64_t kw, torch::Device device) {
  auto opts = torch::TensorOptions().device(device).dtype(torch::kInt32);
  auto mpack = torch::empty({M}, opts);
  auto kpack = torch::empty({K}, opts);
  int64_t n = std::max(M, K);
  hipLaunchKernelGGL(conv_tables_v2_kernel, grid1d(n, 256), dim3(256), 0,
                     at::cuda::getCurrentCUDAStream(), mpack.data_ptr<int>(),
                     kpack.data_ptr<int>(), (int)M, (int)K, (int)WO,
                     (int)stride, (int)dil, (int)(kh * kw), (int)kw);
  return {mpack, kpack};
}

// Which instantiation runs is decided by the two functions below: pure host
// arithmetic (no HIP call, no device tensor), bound to Python as well, so
// the tests ask the very functions the launch code asks. Forward: B images
// of M pixels x N channels, WO pixels per output row, conv stride st on an
// input stuffed by sv; flat = flat-offset tables over a pre-padded buffer.
// Returns (TM, VM, VST, VSV) and the run-time stride handed to the kernel.
std::tuple<int64_t, int64_t, int64_t, int64_t, int64_t> conv_fwd_variant(
    int64_t B, int64_t M, int64_t N, int64_t WO, int64_t st, int64_t sv,
    bool flat) {
  if (WO < 8) st = 0;  // generic per-element staging for very narrow outputs
  // TM=64 is the throughput tile; when its grid would underfill 256 CUs
  // (< ~3 workgroups/CU) halve the pixel tile to double parallelism — the
  // small-M resblock convs (40x120) are latency-bound, not FLOP-bound.
  const int64_t wgs64 =
      ((M + CONV_TM - 1) / CONV_TM) * ((N + CONV_TN - 1) / CONV_TN) * B;
  const int64_t TM = (wgs64 < 256 && M > CONV_TM) ? 32 : 64;
  if (flat) return {TM, 0, 0, 1, st};
  if (sv > 2) return {TM, 1, 0, 0, st};  // stuff stride taken at run time
  if (sv == 2) return {TM, 1, st == 1 ? 1 : 0, 2, st};
  return {TM, 1, (st == 1 || st == 2) ? st : 0, 1, st};
}

// (VM, VST) of one weight-gradient launch.
std::tuple<int64_t, int64_t> conv_wrw_variant(int64_t WO, int64_t st,
                                              bool flat) {
  if (flat) return {0, 0};
  return {1, (WO < 8 || (st != 1 && st != 2)) ? 0 : st};
}

// the instantiations, each written once
using FwdKern = decltype(&conv_fwd_kernel<64, 0, 0, 1>);
struct FwdEntry { int VM, VST, VSV; FwdKern tm64, tm32; };
template <int VM, int VST, int VSV>
constexpr FwdEntry fwd_entry() {
  return {VM, VST, VSV, conv_fwd_kernel<64, VM, VST, VSV>,
          conv_fwd_kernel<32, VM, VST, VSV>};
}
static const FwdEntry FWD_TABLE[] = {
    fwd_entry<0, 0, 1>(), fwd_entry<1, 1, 1>(), fwd_entry<1, 2, 1>(),
    fwd_entry<1, 0, 1>(), fwd_entry<1, 1, 2>(), fwd_entry<1, 0, 2>(),
    fwd_entry<1, 0, 0>()};

static const decltype(&conv_wrw_kernel<0, 0>) WRW_TABLE[2][3] = {  // [VM][VST]
    {conv_wrw_kernel<0, 0>, nullptr, nullptr},
    {conv_wrw_kernel<1, 0>, conv_wrw_kernel<1, 1>, conv_wrw_kernel<1, 2>}};

static void check_operands(const torch::Tensor& x, const torch::Tensor& w,
                           bool fp8_ok) {
  CHECK_CUDA_CONTIG(x);
  CHECK_CUDA_CONTIG(w);
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 ||
                  (fp8_ok && x.scalar_type() == torch::kByte),
              "x must be bf16 (flat tables: or e4m3-as-uint8)");
  TORCH_CHECK(w.scalar_type() == x.scalar_type(), "x/w dtype mismatch");
}

static const float* bias_ptr(const c10::optional<torch::Tensor>& bias) {
  if (!bias.has_value()) return nullptr;
  CHECK_CUDA_CONTIG(bias.value());
  return bias->data_ptr<float>();
}

// Direct LDS-halo kernels (virtual pad vpad): ksize 3 is the stride-1 3x3,
// wmat the fragment-major panel of wmat_make mode 6/7; ksize 5 the stride-2
// 5x5, wmat in the mode-2 layout.
torch::Tensor conv_direct(torch::Tensor x, torch::Tensor wmat,
                          c10::optional<torch::Tensor> bias, int64_t N,
                          int64_t HO, int64_t WO, int64_t act, int64_t vpad,
                          int64_t ksize) {
  check_operands(x, wmat, false);
  const int64_t stride = ksize == 3 ? 1 : 2;
  const int64_t B = x.size(0), Ci = x.size(1), Hp = x.size(2), Wp = x.size(3);
  const int64_t KPd = (Ci * ksize * ksize + 63) & ~63;
  TORCH_CHECK((ksize == 3 || ksize == 5) && Ci % 64 == 0,
              "direct conv gate mismatch: ksize 3 or 5, Ci % 64 == 0");
  TORCH_CHECK(ksize != 3 || vpad >= 1,
              "direct 3x3 conv needs a virtual pad of at least 1");
  TORCH_CHECK(wmat.size(1) == KPd + CONV_AP, "direct wmat stride mismatch");
  TORCH_CHECK(wmat.size(0) == (ksize == 3 ? (N + 15) & ~15 : N),
              "direct wmat rows mismatch (3x3: 16-row fragment groups)");
  TORCH_CHECK(HO == (Hp + 2 * vpad - ksize) / stride + 1 &&
                  WO == (Wp + 2 * vpad - ksize) / stride + 1,
              "direct conv size mismatch");
  auto out = torch::empty({B, N, HO, WO}, x.options());
  dim3 grid(((HO + 7) / 8) * ((WO + 7) / 8), (N + 63) / 64, B);
  const size_t lds = ksize == 3 ? (size_t)2 * 10 * 11 * 64 * 2
                                : (size_t)19 * 19 * 64 * 2;
  hipLaunchKernelGGL(
      ksize == 3 ? conv3x3_direct_kernel : conv5x5s2_direct_kernel, grid,
      dim3(256), lds, at::cuda::getCurrentCUDAStream(),
      (const cvbf16*)x.data_ptr(), (const cvbf16*)wmat.data_ptr(),
      bias_ptr(bias), (cvbf16*)out.data_ptr(), (int)Ci, (int)Hp, (int)Wp,
      (int)N, (int)HO, (int)WO, (int)KPd, x.stride(0),
      (long long)N * HO * WO, (int)act, (int)vpad);
  return out;
}

// The gather-GEMM launch behind conv_gather and conv_flat (fp8 is flat).
static torch::Tensor gather_launch(
    torch::Tensor x, torch::Tensor wmat, c10::optional<torch::Tensor> bias,
    torch::Tensor mtab, torch::Tensor ktab, int64_t N, int64_t K, int64_t HO,
    int64_t WO, int64_t act, int64_t st, int64_t sv, int64_t pt, int64_t pl,
    bool flat, c10::optional<torch::Tensor> out_opt, int64_t oh0, int64_t ow0,
    int64_t ostep) {
  check_operands(x, wmat, flat);
  const int64_t B = x.size(0), M = HO * WO;
  const int64_t KP = (K + 63) & ~63;  // 64-chunk padded; wmat zero-padded
  TORCH_CHECK(wmat.size(1) == KP + CONV_AP, "wmat row stride mismatch");
  // phase-strided output: write into a caller-provided full-grid tensor
  torch::Tensor out;
  long long o_chan = M, WOf = WO;  // channel stride and row width of `out`
  if (out_opt.has_value()) {
    out = out_opt.value();
    CHECK_CUDA_CONTIG(out);
    TORCH_CHECK(out.scalar_type() == torch::kBFloat16 && out.dim() == 4 &&
                    out.size(0) == B && out.size(1) == N,
                "phase out tensor mismatch");
    o_chan = (long long)out.size(2) * out.size(3);
    WOf = out.size(3);
  } else {
    TORCH_CHECK(ostep == 1, "strided output needs an out tensor");
    out = torch::empty({B, N, HO, WO},
                       x.options().dtype(torch::kBFloat16));
  }
  if (x.scalar_type() == torch::kByte) {
    dim3 grid((M + CONV_TM - 1) / CONV_TM, (N + CONV_TN - 1) / CONV_TN, B);
    hipLaunchKernelGGL(conv_fwd_fp8_kernel, grid, dim3(256),
                       (size_t)2 * CONV8_TM * (64 + CONV8_AP),
                       at::cuda::getCurrentCUDAStream(),
                       (const f8*)x.data_ptr(), (const f8*)wmat.data_ptr(),
                       bias_ptr(bias), (cvbf16*)out.data_ptr(),
                       mtab.data_ptr<int>(), ktab.data_ptr<int>(), (int)M,
                       (int)N, (int)K, (int)KP, x.stride(0), (long long)N * M,
                       (int)act, (int)WO, (int)(WO < 8 ? 0 : st));
    return out;
  }
  const auto [TM, VM, VST, VSV, kstride] =
      conv_fwd_variant(B, M, N, WO, st, sv, flat);
  FwdKern kern = nullptr;
  for (const FwdEntry& e : FWD_TABLE)
    if (e.VM == VM && e.VST == VST && e.VSV == VSV)
      kern = TM == 32 ? e.tm32 : e.tm64;
  TORCH_CHECK(kern != nullptr, "no conv_fwd_kernel instantiation");
  dim3 grid((M + TM - 1) / TM, (N + CONV_TN - 1) / CONV_TN, B);
  const size_t lds = (size_t)4 * TM * (64 + CONV_AP) * 2;  // 4-buffer pipeline
  hipLaunchKernelGGL(kern, grid, dim3(256), lds,
                     at::cuda::getCurrentCUDAStream(),
                     (const cvbf16*)x.data_ptr(),
                     (const cvbf16*)wmat.data_ptr(), bias_ptr(bias),
                     (cvbf16*)out.data_ptr(), mtab.data_ptr<int>(),
                     ktab.data_ptr<int>(), (int)M, (int)N, (int)K, (int)KP,
                     x.stride(0), (long long)N * o_chan, (int)act, (int)WO,
                     (int)kstride, (int)x.size(2), (int)x.size(3), (int)pt,
                     (int)pl, (int)sv, (int)oh0, (int)ow0, (int)ostep,
                     (int)WOf, o_chan);
  return out;
}

// Packed tables on the raw x, virtual pad (pt, pl) and stuffing sv. With
// `out`, pixel (h, w) lands at (oh0 + ostep*h, ow0 + ostep*w) of it (phases).
torch::Tensor conv_gather(torch::Tensor x, torch::Tensor wmat,
                          c10::optional<torch::Tensor> bias,
                          torch::Tensor mpack, torch::Tensor kpack, int64_t N,
                          int64_t K, int64_t HO, int64_t WO, int64_t act,
                          int64_t st, int64_t sv, int64_t pt, int64_t pl,
                          c10::optional<torch::Tensor> out, int64_t oh0,
                          int64_t ow0, int64_t ostep) {
  TORCH_CHECK(sv >= 1, "conv_gather: stuff stride sv must be >= 1");
  return gather_launch(x, wmat, bias, mpack, kpack, N, K, HO, WO, act, st, sv,
                       pt, pl, false, out, oh0, ow0, ostep);
}

// Flat-offset tables over a pre-padded buffer: bf16 (conv3d, stride 1) or
// e4m3 (stride 1 or 2).
torch::Tensor conv_flat(torch::Tensor xbuf, torch::Tensor wmat,
                        c10::optional<torch::Tensor> bias,
                        torch::Tensor mbase, torch::Tensor koff, int64_t N,
                        int64_t K, int64_t HO, int64_t WO, int64_t act,
                        int64_t stride) {
  TORCH_CHECK(xbuf.scalar_type() == torch::kByte || stride == 1,
              "conv_flat: the bf16 flat staging is stride 1 only");
  return gather_launch(xbuf, wmat, bias, mbase, koff, N, K, HO, WO, act,
                       stride, 1, 0, 0, true, c10::nullopt, 0, 0, 1);
}

// Weight gradient behind conv_wrw_gather and conv_wrw_flat (fp8 is flat).
static torch::Tensor wrw_launch(torch::Tensor x, torch::Tensor dy,
                                torch::Tensor mtab, torch::Tensor ktab,
                                int64_t N, int64_t K, int64_t WO,
                                bool mcontig, int64_t st, int64_t pt,
                                int64_t pl, bool flat) {
  check_operands(x, dy, flat);
  const int64_t B = x.size(0), M = dy.size(2) * dy.size(3);
  // pick pixel chunking so the grid fills the chip (~6 workgroups/CU).
  // Each (tap-tile, cout-tile, chunk) workgroup owns a disjoint 64x64 region
  // of its chunk's PARTIAL-SUM slice — plain stores, no atomics (atomicAdd
  // across ~40 chunks contends on the same dw cache lines and was measured
  // slower). The slices are then reduced with one sum(0); their memory is
  // bounded by the workgroup target: <= 1536 * 64*64*4B = 25 MB.
  const int64_t tiles = ((K + 63) / 64) * ((N + 63) / 64) * B;
  int pix_chunks = (int)std::min<int64_t>(
      std::max<int64_t>(1536 / std::max<int64_t>(tiles, 1), 1),
      std::max<int64_t>(M / 256, 1));
  // every in-range element of every slice is written once: no zero-fill
  auto dwp = torch::empty({(int64_t)B * pix_chunks, N, K},
                          x.options().dtype(torch::kFloat32));
  dim3 grid((K + 63) / 64, (N + 63) / 64, B * pix_chunks);
  if (x.scalar_type() == torch::kByte) {
    hipLaunchKernelGGL(conv_wrw_fp8_kernel, grid, dim3(256),
                       (size_t)4 * 64 * (32 + CONV8_AP),
                       at::cuda::getCurrentCUDAStream(),
                       (const f8*)x.data_ptr(), (const f8*)dy.data_ptr(),
                       dwp.data_ptr<float>(), mtab.data_ptr<int>(),
                       ktab.data_ptr<int>(), (int)M, (int)N, (int)K,
                       x.stride(0), dy.stride(0), pix_chunks, (int)WO,
                       (int)mcontig);
  } else {
    const auto [VM, VST] = conv_wrw_variant(WO, st, flat);
    size_t lds = (size_t)4 * 64 * (32 + CONV_AP) * 2;  // 2 tiles x dbuf
    hipLaunchKernelGGL(WRW_TABLE[VM][VST], grid, dim3(256), lds,
                       at::cuda::getCurrentCUDAStream(),
                       (const cvbf16*)x.data_ptr(),
                       (const cvbf16*)dy.data_ptr(), dwp.data_ptr<float>(),
                       mtab.data_ptr<int>(), ktab.data_ptr<int>(), (int)M,
                       (int)N, (int)K, x.stride(0), dy.stride(0), pix_chunks,
                       (int)WO, (int)st, (int)x.size(2),
                       (int)x.size(3), (int)pt, (int)pl);
  }
  if (B * pix_chunks == 1) return dwp.view({N, K});
  return dwp.sum(0);
}

torch::Tensor conv_wrw_gather(torch::Tensor x, torch::Tensor dy,
                              torch::Tensor mpack, torch::Tensor kpack,
                              int64_t N, int64_t K, int64_t WO, int64_t st,
                              int64_t pt, int64_t pl) {
  return wrw_launch(x, dy, mpack, kpack, N, K, WO, false, st, pt, pl, false);
}

// mcontig: 8 pixels of an output row are contiguous in xbuf. The bf16
// kernel takes that for granted (stride 1); e4m3 may pass false.
torch::Tensor conv_wrw_flat(torch::Tensor xbuf, torch::Tensor dy,
                            torch::Tensor mbase, torch::Tensor koff, int64_t N,
                            int64_t K, int64_t WO, bool mcontig) {
  TORCH_CHECK(xbuf.scalar_type() == torch::kByte || mcontig,
              "conv_wrw_flat: the bf16 flat staging needs mcontig");
  return wrw_launch(xbuf, dy, mbase, koff, N, K, WO, mcontig, 1, 0, 0, true);
}

torch::Tensor panel_gather(torch::Tensor src, torch::Tensor ktab) {
  CHECK_CUDA_CONTIG(src);
  CHECK_CUDA_CONTIG(ktab);
  const int64_t rows = src.size(0);
  const int64_t Kl = ktab.numel();
  const int64_t KPA = ((Kl + 63) & ~63) + CONV_AP;
  auto out = torch::empty({rows, KPA}, src.options().dtype(torch::kBFloat16));
  const long long total = rows * KPA;
  auto stream = at::cuda::getCurrentCUDAStream();
  dispatch_f32_bf16(src, "panel_gather: src", [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((panel_gather_kernel<T>), dim3(ew_grid(total)),
                       dim3(256), 0, stream, ptr<const T>(src),
                       ktab.data_ptr<int>(), ptr<cvbf16>(out), (int)rows,
                       (int)Kl, (int)KPA, (int)src.size(1));
  });
  return out;
}

torch::Tensor act_bwd(torch::Tensor dy, torch::Tensor y, int64_t act) {
  CHECK_CUDA_CONTIG(dy);
  CHECK_CUDA_CONTIG(y);
  const long long n = dy.numel();
  auto out = torch::empty_like(y);  // y is bf16, same shape
  auto stream = at::cuda::getCurrentCUDAStream();
  dispatch_f32_bf16(dy, "act_bwd: dy", [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((act_bwd_kernel<T>), dim3(ew_grid(n)), dim3(256), 0,
                       stream, ptr<const T>(dy), ptr<const cvbf16>(y),
                       ptr<cvbf16>(out), n, (int)act);
  });
  return out;
}

torch::Tensor wmat_make(torch::Tensor w1, int64_t khw, int64_t mode) {
  CHECK_CUDA_CONTIG(w1);
  const int64_t N = w1.size(0), K = w1.size(1);
  const bool rot = (mode & 1) != 0;
  const int64_t nrows = rot ? K / khw : N;
  const int64_t kout = rot ? N * khw : K;
  const int64_t KPA = ((kout + 63) & ~63) + CONV_AP;
  TORCH_CHECK(mode >= 0 && mode <= 7 && mode != 4 && mode != 5,
              "wmat_make: mode 0-3, 6 or 7");
  TORCH_CHECK(!(mode & 4) || kout % 64 == 0,
              "wmat_make: fragment-major panels need K % 64 == 0");
  const int64_t rows = (mode & 4) ? (nrows + 15) & ~15 : nrows;
  auto out = torch::empty({rows, KPA},
                          w1.options().dtype(torch::kBFloat16));
  const long long total = rows * KPA;
  auto stream = at::cuda::getCurrentCUDAStream();
  dispatch_f32_bf16(w1, "wmat_make: w1", [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((wmat_make_kernel<T>), dim3(ew_grid(total)), dim3(256),
                       0, stream, ptr<const T>(w1), ptr<cvbf16>(out),
                       (int)rows, (int)kout, (int)K, (int)khw, (int)KPA,
                       (int)mode, (int)nrows);
  });
  return out;
}

}  // namespace dsin
