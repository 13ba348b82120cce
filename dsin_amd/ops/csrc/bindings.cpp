// Python bindings for the dsin_amd HIP/CDNA4 kernels.
#include <torch/extension.h>

namespace dsin {
std::tuple<torch::Tensor, torch::Tensor> quantize_fwd(torch::Tensor x,
                                                      torch::Tensor centers,
                                                      double sigma);
std::tuple<torch::Tensor, torch::Tensor> quantize_bwd(torch::Tensor g,
                                                      torch::Tensor x,
                                                      torch::Tensor centers,
                                                      double sigma);
torch::Tensor bitcost_ce_fwd(torch::Tensor logits, torch::Tensor symbols);
torch::Tensor bitcost_ce_bwd(torch::Tensor g, torch::Tensor logits,
                             torch::Tensor symbols);
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> ncc_search(
    torch::Tensor x_dec, torch::Tensor y_dec, torch::Tensor y_orig, int64_t ph,
    int64_t pw, bool use_mask);
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> ncc_search_l2lab(
    torch::Tensor x_dec, torch::Tensor y_dec, torch::Tensor y_orig, int64_t ph,
    int64_t pw, bool use_mask);
torch::Tensor ncc_lab_transform(torch::Tensor img);
torch::Tensor mfma_selftest(torch::Tensor A, torch::Tensor B);
torch::Tensor mfma32_selftest(torch::Tensor A, torch::Tensor B);
std::tuple<torch::Tensor, torch::Tensor> conv_tables(
    int64_t M, int64_t K, int64_t WO, int64_t stride, int64_t dil, int64_t Wp,
    int64_t HpWp, int64_t kh, int64_t kw, torch::Device device);
std::tuple<torch::Tensor, torch::Tensor> conv_tables_v2(
    int64_t M, int64_t K, int64_t WO, int64_t stride, int64_t dil, int64_t kh,
    int64_t kw, torch::Device device);
std::tuple<int64_t, int64_t, int64_t, int64_t, int64_t> conv_fwd_variant(
    int64_t B, int64_t M, int64_t N, int64_t WO, int64_t st, int64_t sv,
    bool flat);
std::tuple<int64_t, int64_t> conv_wrw_variant(int64_t WO, int64_t st,
                                              bool flat);
torch::Tensor conv_direct(torch::Tensor x, torch::Tensor wmat,
                          c10::optional<torch::Tensor> bias, int64_t N,
                          int64_t HO, int64_t WO, int64_t act, int64_t vpad,
                          int64_t ksize);
torch::Tensor conv_gather(torch::Tensor x, torch::Tensor wmat,
                          c10::optional<torch::Tensor> bias,
                          torch::Tensor mpack, torch::Tensor kpack, int64_t N,
                          int64_t K, int64_t HO, int64_t WO, int64_t act,
                          int64_t st, int64_t sv, int64_t pt, int64_t pl,
                          c10::optional<torch::Tensor> out, int64_t oh0,
                          int64_t ow0, int64_t ostep);
torch::Tensor conv_flat(torch::Tensor xbuf, torch::Tensor wmat,
                        c10::optional<torch::Tensor> bias,
                        torch::Tensor mbase, torch::Tensor koff, int64_t N,
                        int64_t K, int64_t HO, int64_t WO, int64_t act,
                        int64_t stride);
torch::Tensor panel_gather(torch::Tensor src, torch::Tensor ktab);
torch::Tensor conv_wrw_gather(torch::Tensor x, torch::Tensor dy,
                              torch::Tensor mpack, torch::Tensor kpack,
                              int64_t N, int64_t K, int64_t WO, int64_t st,
                              int64_t pt, int64_t pl);
torch::Tensor conv_wrw_flat(torch::Tensor xbuf, torch::Tensor dy,
                            torch::Tensor mbase, torch::Tensor koff, int64_t N,
                            int64_t K, int64_t WO, bool mcontig);
torch::Tensor act_bwd(torch::Tensor dy, torch::Tensor y, int64_t act);
torch::Tensor wmat_make(torch::Tensor w1, int64_t khw, int64_t mode);
void adam_step(torch::Tensor p, torch::Tensor g, torch::Tensor m,
               torch::Tensor v, torch::Tensor lr, torch::Tensor step,
               c10::optional<torch::Tensor> wd, double b1, double b2,
               double eps);
torch::Tensor pad_stuff_e4m3(torch::Tensor x, int64_t pt, int64_t pb,
                             int64_t pl, int64_t pr, int64_t stride);
std::vector<torch::Tensor> bn_fwd(torch::Tensor y, torch::Tensor gamma,
                                  torch::Tensor beta, torch::Tensor rmean,
                                  torch::Tensor rvar, double momentum,
                                  double eps, bool training, int64_t act,
                                  c10::optional<torch::Tensor> residual);
std::vector<torch::Tensor> bn_bwd(torch::Tensor dy, torch::Tensor y,
                                  torch::Tensor out, torch::Tensor mean,
                                  torch::Tensor rstd, torch::Tensor gamma,
                                  bool training, int64_t act);
std::vector<torch::Tensor> heatmap_mask_fwd(torch::Tensor b);
torch::Tensor heatmap_mask_bwd(torch::Tensor b, torch::Tensor gz,
                               c10::optional<torch::Tensor> gh3);
torch::Tensor l1_part(torch::Tensor x, torch::Tensor y);
std::vector<torch::Tensor> l1_bwd(torch::Tensor x, torch::Tensor y,
                                  torch::Tensor g, bool need_gx,
                                  bool need_gy);
torch::Tensor hterms_part(torch::Tensor bc, torch::Tensor heat);
std::vector<torch::Tensor> hterms_bwd(torch::Tensor bc, torch::Tensor heat,
                                      torch::Tensor g2, bool need_gheat);
torch::Tensor ssim_scale_fwd(torch::Tensor a, torch::Tensor b,
                             torch::Tensor taps, double c1, double c2);
std::vector<torch::Tensor> ssim_scale_bwd(
    torch::Tensor a, torch::Tensor b, torch::Tensor taps,
    c10::optional<torch::Tensor> g_ssim, c10::optional<torch::Tensor> g_cs,
    double c1, double c2, bool need_ga, bool need_gb);
torch::Tensor down2_fwd(torch::Tensor x);
torch::Tensor down2_bwd(torch::Tensor g, int64_t H, int64_t W, bool bf16_out);
std::tuple<torch::Tensor, torch::Tensor> pc_freqs(torch::Tensor q_pad,
                                                  torch::Tensor pos,
                                                  torch::Tensor wts, int64_t k,
                                                  int64_t L, bool portable);
torch::Tensor pc_encode(torch::Tensor q_pad, torch::Tensor pos,
                        torch::Tensor syms, torch::Tensor wts, int64_t k,
                        int64_t L, bool portable);
torch::Tensor pc_decode(torch::Tensor q_pad, torch::Tensor pos,
                        std::vector<int64_t> offsets, torch::Tensor wts,
                        int64_t k, int64_t L, torch::Tensor data,
                        std::vector<int64_t> data_offs, torch::Tensor centers,
                        bool portable);
std::tuple<torch::Tensor, torch::Tensor> pc_freqs_ragged(
    torch::Tensor q, std::vector<int64_t> desc, torch::Tensor items,
    torch::Tensor wts, int64_t k, int64_t L, bool portable);
torch::Tensor pc_encode_ragged(torch::Tensor q, std::vector<int64_t> desc,
                               torch::Tensor items,
                               std::vector<int64_t> starts, torch::Tensor syms,
                               torch::Tensor wts, int64_t k, int64_t L,
                               bool portable);
torch::Tensor pc_decode_ragged(torch::Tensor q, std::vector<int64_t> desc,
                               torch::Tensor items, std::vector<int64_t> seg,
                               torch::Tensor wts, int64_t k, int64_t L,
                               torch::Tensor data,
                               std::vector<int64_t> data_offs,
                               torch::Tensor centers, bool portable);
torch::Tensor rc_encode(torch::Tensor syms, torch::Tensor freqs);
torch::Tensor rc_decode(torch::Tensor data, torch::Tensor freqs);
torch::Tensor rc_encode_host(torch::Tensor syms, torch::Tensor freqs);
torch::Tensor rc_decode_host(torch::Tensor data, torch::Tensor freqs);
bool pc_host_force_libm(bool on);
std::string pc_host_path();
bool pc_host_has_fma();
}  // namespace dsin

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("quantize_fwd", &dsin::quantize_fwd, "fused soft quantizer forward");
  m.def("quantize_bwd", &dsin::quantize_bwd, "fused soft quantizer backward");
  m.def("bitcost_ce_fwd", &dsin::bitcost_ce_fwd, "bitcost cross-entropy fwd");
  m.def("bitcost_ce_bwd", &dsin::bitcost_ce_bwd, "bitcost cross-entropy bwd");
  m.def("ncc_search", &dsin::ncc_search, "streaming NCC side-info search");
  m.def("ncc_search_l2lab", &dsin::ncc_search_l2lab,
        "streaming L2+LAB side-info search (argmin of squared distance)");
  m.def("ncc_lab_transform", &dsin::ncc_lab_transform,
        "bf16 CIELAB operands of the L2+LAB search");
  m.def("mfma_selftest", &dsin::mfma_selftest, "MFMA 16x16x32 layout check");
  m.def("mfma32_selftest", &dsin::mfma32_selftest, "MFMA 32x32x16 layout check");
  m.def("conv_tables", &dsin::conv_tables, "gather-conv offset tables");
  m.def("conv_tables_v2", &dsin::conv_tables_v2,
        "packed-coordinate tables for the virtual-pad gather path");
  // Implicit-GEMM conv family. N = output channels, K = taps (Cin*kh*kw);
  // the two *_variant functions are the launch code's own selection and
  // touch no device, so they answer on a machine without a GPU.
  m.def("conv_fwd_variant", &dsin::conv_fwd_variant,
        "(TM, VM, VST, VSV, run-time stride) of one forward gather launch",
        py::arg("B"), py::arg("M"), py::arg("N"), py::arg("WO"),
        py::arg("st"), py::arg("sv"), py::arg("flat"));
  m.def("conv_wrw_variant", &dsin::conv_wrw_variant,
        "(VM, VST) of one weight-gradient launch", py::arg("WO"),
        py::arg("st"), py::arg("flat"));
  m.def("conv_direct", &dsin::conv_direct,
        "direct LDS-halo conv: ksize 3 (stride 1) or 5 (stride 2)",
        py::arg("x"), py::arg("wmat"), py::arg("bias"), py::arg("N"),
        py::arg("HO"), py::arg("WO"), py::arg("act"), py::arg("vpad"),
        py::arg("ksize"));
  m.def("conv_gather", &dsin::conv_gather,
        "virtual-pad gather conv; with out, a phase written strided into it",
        py::arg("x"), py::arg("wmat"), py::arg("bias"), py::arg("mpack"),
        py::arg("kpack"), py::arg("N"), py::arg("K"), py::arg("HO"),
        py::arg("WO"), py::arg("act"), py::arg("st"), py::arg("sv"),
        py::arg("pt"), py::arg("pl"), py::arg("out") = py::none(),
        py::arg("oh0") = 0, py::arg("ow0") = 0, py::arg("ostep") = 1);
  m.def("conv_flat", &dsin::conv_flat,
        "gather conv over a pre-padded buffer, flat tables (bf16 or e4m3)",
        py::arg("xbuf"), py::arg("wmat"), py::arg("bias"), py::arg("mbase"),
        py::arg("koff"), py::arg("N"), py::arg("K"), py::arg("HO"),
        py::arg("WO"), py::arg("act"), py::arg("stride"));
  m.def("conv_wrw_gather", &dsin::conv_wrw_gather,
        "weight gradient of conv_gather (sv = 1)", py::arg("x"),
        py::arg("dy"), py::arg("mpack"), py::arg("kpack"), py::arg("N"),
        py::arg("K"), py::arg("WO"), py::arg("st"), py::arg("pt"),
        py::arg("pl"));
  m.def("conv_wrw_flat", &dsin::conv_wrw_flat,
        "weight gradient of conv_flat", py::arg("xbuf"), py::arg("dy"),
        py::arg("mbase"), py::arg("koff"), py::arg("N"), py::arg("K"),
        py::arg("WO"), py::arg("mcontig"));
  m.def("act_bwd", &dsin::act_bwd, "fused activation gradient (bf16 out)");
  m.def("wmat_make", &dsin::wmat_make, "padded/rotated bf16 conv W panel");
  m.def("panel_gather", &dsin::panel_gather,
        "column-gather of a W panel (phase-decomposed convs)");
  m.def("adam_step", &dsin::adam_step, "fused flat-buffer Adam step");
  m.def("pad_stuff_e4m3", &dsin::pad_stuff_e4m3,
        "fused pad/zero-stuff/quantize to e4m3 (the fp8 conv input buffer)",
        py::arg("x"), py::arg("pt"), py::arg("pb"), py::arg("pl"),
        py::arg("pr"), py::arg("stride"));
  m.def("bn_fwd", &dsin::bn_fwd, "fused batch-norm(+act) forward");
  m.def("bn_bwd", &dsin::bn_bwd, "fused batch-norm(+act) backward");
  m.def("heatmap_mask_fwd", &dsin::heatmap_mask_fwd,
        "fused heatmap3D + bottleneck mask");
  m.def("heatmap_mask_bwd", &dsin::heatmap_mask_bwd,
        "heatmap3D + mask backward");
  m.def("l1_part", &dsin::l1_part, "per-image |y-x| partial sums");
  m.def("l1_bwd", &dsin::l1_bwd, "L1-mean backward");
  m.def("hterms_part", &dsin::hterms_part,
        "fused (sum bc, sum bc*heatmap) partials");
  m.def("hterms_bwd", &dsin::hterms_bwd, "rate-term backward");
  m.def("ssim_scale_fwd", &dsin::ssim_scale_fwd,
        "fused one-scale SSIM/CS partial sums (fp32)");
  m.def("ssim_scale_bwd", &dsin::ssim_scale_bwd,
        "one-scale SSIM/CS analytic gradient");
  m.def("down2_fwd", &dsin::down2_fwd, "MS-SSIM dyadic downsample");
  m.def("down2_bwd", &dsin::down2_bwd, "MS-SSIM dyadic downsample adjoint");
  // Entropy codec: q_pad is (B, C+4, H+8, W+8) and picks the device (HIP
  // kernels on a GPU tensor, the portable host build on a CPU tensor).
  m.def("pc_freqs", &dsin::pc_freqs,
        "probclass context model per position: (B, n, L) logits and tables",
        py::arg("q_pad"), py::arg("pos"), py::arg("wts"), py::arg("k"),
        py::arg("L"), py::arg("portable") = false);
  m.def("pc_encode", &dsin::pc_encode,
        "context model + range encoder: (B, 8 + 3n + 16) length-prefixed rows",
        py::arg("q_pad"), py::arg("pos"), py::arg("syms"), py::arg("wts"),
        py::arg("k"), py::arg("L"), py::arg("portable") = false);
  m.def("pc_decode", &dsin::pc_decode,
        "wavefront context-model decoder, concatenated payloads",
        py::arg("q_pad"), py::arg("pos"), py::arg("offsets"), py::arg("wts"),
        py::arg("k"), py::arg("L"), py::arg("data"), py::arg("data_offs"),
        py::arg("centers"), py::arg("portable") = false);
  // Ragged form: images of different (C, H, W) in one flat value buffer q
  // (which picks the device), a descriptor table of 5 values per image
  // (C, H, W, volume offset, symbol offset) and items (n, 4) = (b, c, h, w).
  m.def("pc_freqs_ragged", &dsin::pc_freqs_ragged,
        "context model per item: compact (n, L) logits and tables",
        py::arg("q"), py::arg("desc"), py::arg("items"), py::arg("wts"),
        py::arg("k"), py::arg("L"), py::arg("portable") = false);
  m.def("pc_encode_ragged", &dsin::pc_encode_ragged,
        "context model + range encoder: flat length-prefixed rows",
        py::arg("q"), py::arg("desc"), py::arg("items"), py::arg("starts"),
        py::arg("syms"), py::arg("wts"), py::arg("k"), py::arg("L"),
        py::arg("portable") = false);
  m.def("pc_decode_ragged", &dsin::pc_decode_ragged,
        "wavefront decoder over the merged schedule of a ragged batch",
        py::arg("q"), py::arg("desc"), py::arg("items"), py::arg("seg"),
        py::arg("wts"), py::arg("k"), py::arg("L"), py::arg("data"),
        py::arg("data_offs"), py::arg("centers"),
        py::arg("portable") = false);
  m.def("rc_encode", &dsin::rc_encode,
        "device range encoder, one workgroup per image");
  m.def("rc_decode", &dsin::rc_decode, "device range decoder, given tables");
  m.def("rc_encode_host", &dsin::rc_encode_host,
        "host build of the range-encoder step functions");
  m.def("rc_decode_host", &dsin::rc_decode_host,
        "host build of the range-decoder step functions");
  m.def("pc_host_force_libm", &dsin::pc_host_force_libm,
        "force the library-fmaf host path; returns the previous setting");
  m.def("pc_host_path", &dsin::pc_host_path,
        "host path in use: 'fma' (hardware FMA) or 'libm'");
  m.def("pc_host_has_fma", &dsin::pc_host_has_fma,
        "whether this CPU has the hardware-FMA host path");
}
