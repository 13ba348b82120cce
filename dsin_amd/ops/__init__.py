"""Op dispatch layer: HIP/CDNA4 kernels on GPU, pure-torch reference on CPU.

The HIP extension is built IN-TREE (``python setup.py build_ext --inplace`` at
the repo root, or ``__graft_entry__.build()``) into ``dsin_amd/ops/_dsin_hip*.so``
for gfx950 only. On a CUDA(ROCm) tensor the kernel path is mandatory: if the
extension is missing we raise instead of silently falling back to eager, so a
GPU run can never accidentally measure the PyTorch path.

CPU tensors always use the reference implementations in
:mod:`dsin_amd.ops.reference` (also the numerics oracles for the GPU tests).
The one exception is the portable entropy codec (``pc_*(portable=True)``),
whose CPU side is a host build inside the same extension and raises in the
same way when the extension is missing.
"""

from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from . import reference as ref

_EXT = None
_EXT_ERR: Optional[str] = None


def _try_load_ext():
    global _EXT, _EXT_ERR
    if _EXT is not None:
        return _EXT
    try:
        from . import _dsin_hip  # type: ignore  # built in-tree by setup.py
        _EXT = _dsin_hip
    except ImportError as e:  # pragma: no cover - exercised only sans build
        _EXT_ERR = str(e)
        _EXT = None
    return _EXT


def hip_available() -> bool:
    return _try_load_ext() is not None


def _require_ext(opname: str, where: str = "on a GPU tensor"):
    ext = _try_load_ext()
    if ext is None:
        raise RuntimeError(
            f"dsin_amd op {opname!r} called {where} but the HIP extension "
            f"is not built (import error: {_EXT_ERR}). Build it in-tree with "
            f"`python setup.py build_ext --inplace` (PYTORCH_ROCM_ARCH=gfx950).")
    if not hasattr(ext, opname):
        raise RuntimeError(
            f"dsin_amd HIP extension is built but lacks symbol {opname!r} — "
            f"stale build; rebuild with `python setup.py build_ext --inplace`.")
    return getattr(ext, opname)


# ---------------------------------------------------------------------------
# Quantizer: fused soft-to-hard scalar quantization with straight-through
# estimator and analytic backward. HIP kernel: csrc/quantizer.hip.
# ---------------------------------------------------------------------------

class _QuantizeFn(torch.autograd.Function):
    """Forward returns (qbar, symbols); backward implements the qsoft path
    only (the straight-through combine qbar = qsoft + sg(qhard - qsoft),
    reference src/autoencoder_imgcomp.py:131-134): gradients w.r.t. x and
    centers are those of qsoft = sum_l softmax(-(x-c)^2)_l * c_l.
    """

    @staticmethod
    def forward(ctx, x: torch.Tensor, centers: torch.Tensor, sigma: float):
        fwd = _require_ext("quantize_fwd")
        qbar, symbols = fwd(x, centers, sigma)
        ctx.save_for_backward(x, centers)
        ctx.sigma = sigma
        return qbar, symbols

    @staticmethod
    def backward(ctx, g_qbar: torch.Tensor, g_symbols):
        x, centers = ctx.saved_tensors
        bwd = _require_ext("quantize_bwd")
        gx, gc = bwd(g_qbar.contiguous(), x, centers, ctx.sigma)
        return gx, gc, None


def quantize(x: torch.Tensor, centers: torch.Tensor, sigma: float = 1.0
             ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Returns (qbar, symbols). See reference src/quantizer_imgcomp.py:37-100.
    Always computed in fp32 (the bottleneck is tiny; bf16 autocast inputs are
    upcast here and gradients flow back through the cast)."""
    if x.is_cuda:
        return _QuantizeFn.apply(x.float().contiguous(),
                                 centers.float().contiguous(), sigma)
    qbar, _, _, symbols = ref.quantize_ref(x.float(), centers, sigma)
    return qbar, symbols


# ---------------------------------------------------------------------------
# Heatmap + bottleneck masking (reference src/autoencoder_imgcomp.py:172-201).
# GPU: ONE fused kernel (sigmoid + per-channel clamp ramp + mask multiply)
# each way instead of the ~5-kernel torch chain per pass.
# ---------------------------------------------------------------------------

class _HeatmapMaskFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, b: torch.Tensor):
        z, h3 = _require_ext("heatmap_mask_fwd")(b.contiguous())
        ctx.save_for_backward(b)
        ctx.set_materialize_grads(False)
        return z, h3

    @staticmethod
    def backward(ctx, gz, gh3):
        (b,) = ctx.saved_tensors
        if gz is None:
            gz = torch.zeros(b.shape[0], b.shape[1] - 1, b.shape[2],
                             b.shape[3], dtype=b.dtype, device=b.device)
        gh = gh3.contiguous() if gh3 is not None else None
        return _require_ext("heatmap_mask_bwd")(b, gz.contiguous(), gh)


def heatmap_mask(bottleneck: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(N, C+1, H, W) -> (z_masked (N,C,H,W), heatmap3D (N,C,H,W))."""
    if bottleneck.is_cuda and hip_available():
        return _HeatmapMaskFn.apply(bottleneck)
    h3 = ref.heatmap3d_ref(bottleneck)
    return h3 * bottleneck[:, 1:], h3


# ---------------------------------------------------------------------------
# Fused loss reductions: per-image L1 mean and the rate terms
# (H_real, H_mask) — single-pass partial sums + ordered host-side reduce,
# analytic backward kernels. Replaces the sub/abs/mul temporaries and
# multi-stage torch reduces in the loss assembly.
# ---------------------------------------------------------------------------

class _L1MeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, y: torch.Tensor):
        x, y = x.contiguous(), y.contiguous()
        parts = _require_ext("l1_part")(x, y)          # (N, S)
        chw = x.numel() // x.shape[0]
        per = parts.sum(dim=1) / float(chw)            # (N,)
        ctx.save_for_backward(x, y)
        ctx.chw = chw
        return per

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        gs = (g.float() / float(ctx.chw)).contiguous()
        gx, gy = _require_ext("l1_bwd")(x, y, gs, ctx.needs_input_grad[0],
                                        ctx.needs_input_grad[1])
        return (gx if ctx.needs_input_grad[0] else None,
                gy if ctx.needs_input_grad[1] else None)


def l1_mean_per_image(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """mean(|y - x|) over CHW per image, shape (N,). GPU fused; CPU eager."""
    if x.is_cuda and hip_available():
        return _L1MeanFn.apply(x, y)
    return (y.float() - x.float()).abs().mean(dim=(1, 2, 3))


class _HTermsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, bc: torch.Tensor, heat: torch.Tensor):
        bc, heat = bc.contiguous(), heat.contiguous()
        parts = _require_ext("hterms_part")(bc, heat)  # (S, 2)
        sums = parts.sum(dim=0) / float(bc.numel())
        ctx.save_for_backward(bc, heat)
        return sums[0], sums[1]

    @staticmethod
    def backward(ctx, g1, g2):
        bc, heat = ctx.saved_tensors
        g2v = torch.stack([g1, g2]).float().contiguous()
        gbc, gheat = _require_ext("hterms_bwd")(bc, heat, g2v,
                                                ctx.needs_input_grad[1])
        return gbc, (gheat if ctx.needs_input_grad[1] else None)


def rate_terms(bc: torch.Tensor, heat: torch.Tensor):
    """(mean(bc), mean(bc*heat)) in one pass. GPU fused (bc fp32, heat
    bf16); eager otherwise."""
    if (bc.is_cuda and hip_available() and bc.dtype == torch.float32
            and heat.dtype == torch.bfloat16):
        return _HTermsFn.apply(bc, heat)
    return bc.mean(), (bc * heat).mean()


# ---------------------------------------------------------------------------
# Bitcost cross-entropy (reference src/probclass_imgcomp.py:100-106).
# ---------------------------------------------------------------------------

class _BitcostCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits: torch.Tensor, symbols: torch.Tensor):
        fwd = _require_ext("bitcost_ce_fwd")
        bits = fwd(logits, symbols)
        ctx.save_for_backward(logits, symbols)
        return bits

    @staticmethod
    def backward(ctx, g_bits: torch.Tensor):
        logits, symbols = ctx.saved_tensors
        bwd = _require_ext("bitcost_ce_bwd")
        return bwd(g_bits.contiguous(), logits, symbols), None


def bitcost_ce(logits: torch.Tensor, symbols: torch.Tensor) -> torch.Tensor:
    """logits (N, L, C, H, W), symbols (N, C, H, W) -> bits (N, C, H, W).
    fp32 compute (autocast bf16 logits are upcast here)."""
    if logits.is_cuda:
        return _BitcostCEFn.apply(logits.float().contiguous(),
                                  symbols.contiguous())
    return ref.bitcost_ce_ref(logits.float(), symbols)


# ---------------------------------------------------------------------------
# SI search (reference src/siFinder.py + src/siFull_img.py). Non-trainable by
# construction (reference src/siFinder.py:3-5; stop_gradient on y_syn at
# src/AE.py:67), so the GPU path is a forward-only streaming kernel that never
# materializes the (P, Hc, Wc) correlation volume or the Gaussian mask.
# ---------------------------------------------------------------------------

def check_ncc_inputs(x_dec, y_dec, y_orig, ph: int, pw: int, use_mask: bool):
    """Inputs both devices accept, checked before anything is launched."""
    if x_dec.dim() != 3 or x_dec.shape[0] != 3:
        raise ValueError(f"ncc_search: images must be (3, H, W), got "
                         f"{tuple(x_dec.shape)}")
    if x_dec.shape != y_dec.shape or x_dec.shape != y_orig.shape:
        raise ValueError(
            f"ncc_search: the three images must share one shape, got "
            f"{tuple(x_dec.shape)}, {tuple(y_dec.shape)}, "
            f"{tuple(y_orig.shape)}")
    h, w = x_dec.shape[1], x_dec.shape[2]
    if ph < 1 or pw < 1 or h % ph or w % pw:
        raise ValueError(f"ncc_search: a {h}x{w} image does not tile by "
                         f"{ph}x{pw} patches")
    if use_mask and (ph % 2 or pw % 2):
        raise ValueError(
            f"ncc_search: the location prior is defined only for even patch "
            f"sizes, got {ph}x{pw} (pass use_mask=False)")


@torch.no_grad()
def ncc_search(x_dec: torch.Tensor, y_dec: torch.Tensor, y_orig: torch.Tensor,
               ph: int, pw: int, use_mask: bool = True, l2lab: bool = False
               ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Single-image SI search: (3,Hx,Wx)x3 -> (y_syn (3,Hx,Wx), rows, cols).
    l2lab selects the reference's use_L2andLAB mode: CIELAB of the raw
    images, squared L2 distance (times the prior when use_mask), argmin
    with the first index on ties. On the GPU both modes run the streaming
    HIP kernels (bf16 operands, fp32 scores, no (P,Hc,Wc) volume, no host
    sync); on the CPU both run the torch reference in fp32."""
    check_ncc_inputs(x_dec, y_dec, y_orig, ph, pw, use_mask)
    if x_dec.is_cuda:
        # the batch of one: the kernels have no other form
        y_syn, rows, cols = _ncc_search_ext(x_dec[None], y_dec[None],
                                            y_orig[None], ph, pw, use_mask,
                                            l2lab)
        return y_syn[0], rows[0], cols[0]
    return ref.ncc_search_ref(x_dec.float(), y_dec.float(), y_orig.float(),
                              ph, pw, use_mask, l2lab=l2lab)


def _ncc_search_ext(x_dec, y_dec, y_orig, ph, pw, use_mask, l2lab):
    """(B,3,H,W) checked device tensors through the extension."""
    fn = _require_ext("ncc_search_l2lab" if l2lab else "ncc_search")
    return fn(x_dec.contiguous().float(), y_dec.contiguous().float(),
              y_orig.contiguous().float(), ph, pw, use_mask)


def check_ncc_batch_inputs(x_dec, y_dec, y_orig, ph: int, pw: int,
                           use_mask: bool):
    """The batch form of check_ncc_inputs: rank, B >= 1 and one shape here,
    the per-image geometry there."""
    if x_dec.dim() != 4 or x_dec.shape[0] < 1 or x_dec.shape[1] != 3:
        raise ValueError(f"ncc_search_batch: images must be (B, 3, H, W) "
                         f"with B >= 1, got {tuple(x_dec.shape)}")
    if x_dec.shape != y_dec.shape or x_dec.shape != y_orig.shape:
        raise ValueError(
            f"ncc_search_batch: the three batches must share one shape, got "
            f"{tuple(x_dec.shape)}, {tuple(y_dec.shape)}, "
            f"{tuple(y_orig.shape)}")
    check_ncc_inputs(x_dec[0], y_dec[0], y_orig[0], ph, pw, use_mask)


@torch.no_grad()
def ncc_search_batch(x_dec: torch.Tensor, y_dec: torch.Tensor,
                     y_orig: torch.Tensor, ph: int, pw: int,
                     use_mask: bool = True, l2lab: bool = False
                     ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """SI search of B >= 1 images of one size: (B,3,H,W)x3 -> (y_syn
    (B,3,H,W), rows (B,P), cols (B,P)); image b of the result is what
    ncc_search returns for image b, bit for bit. On the GPU the B images
    share one launch per pipeline stage and one allocation per intermediate
    (B times the grid, the launches of one image, no host sync); on the CPU
    the torch reference runs per image."""
    check_ncc_batch_inputs(x_dec, y_dec, y_orig, ph, pw, use_mask)
    if x_dec.is_cuda:
        return _ncc_search_ext(x_dec, y_dec, y_orig, ph, pw, use_mask, l2lab)
    outs = [ref.ncc_search_ref(x_dec[b].float(), y_dec[b].float(),
                               y_orig[b].float(), ph, pw, use_mask,
                               l2lab=l2lab)
            for b in range(x_dec.shape[0])]
    y_syn, rows, cols = (torch.stack(t) for t in zip(*outs))
    return y_syn, rows, cols


@torch.no_grad()
def ncc_lab_transform(img: torch.Tensor) -> torch.Tensor:
    """(3,H,W) raw pixels -> the bf16 CIELAB operands of the l2lab search.
    GPU: the kernel the search itself runs; CPU: rgb_to_lab_ref rounded."""
    if img.is_cuda:
        return _require_ext("ncc_lab_transform")(img.contiguous().float())
    return ref.rgb_to_lab_ref(img.float()).to(torch.bfloat16)


# ---------------------------------------------------------------------------
# MS-SSIM loss: one fused fp32 kernel per scale each way plus
# the dyadic downsample. HIP kernels: csrc/msssim.hip.
# ---------------------------------------------------------------------------

SSIM_C1 = (0.01 * 255.0) ** 2
SSIM_C2 = (0.03 * 255.0) ** 2
SSIM_MAX_TAPS = 11


def check_ssim_taps(ntaps: int, h: int, w: int, what: str = "ssim_scale"):
    """The GPU kernels take an odd filter of at most 11 taps that fits the
    image (the sizes the torch path accepts); anything else is a ValueError
    raised before a kernel is launched."""
    if ntaps % 2 == 0 or not 1 <= ntaps <= SSIM_MAX_TAPS:
        raise ValueError(f"{what}: filter length {ntaps} must be odd and "
                         f"<= {SSIM_MAX_TAPS}")
    if ntaps > min(h, w):
        raise ValueError(f"{what}: a {ntaps}-tap filter does not fit an "
                         f"image of size {h}x{w}")


class _SsimScaleFn(torch.autograd.Function):
    """(mean ssim, mean cs) of one scale. Forward writes per-tile partial
    sums; the ordered host-side sum makes the means bitwise deterministic.
    Backward recomputes the blurred maps (nothing but the inputs is saved)."""

    @staticmethod
    def forward(ctx, a: torch.Tensor, b: torch.Tensor, taps: torch.Tensor,
                c1: float, c2: float):
        parts = _require_ext("ssim_scale_fwd")(a, b, taps, c1, c2)  # (2, S)
        t = taps.numel()
        n = a.shape[0] * a.shape[1] * (a.shape[2] - t + 1) * (a.shape[3] - t + 1)
        means = (parts.sum(dim=1, dtype=torch.float64) / float(n)).float()
        ctx.save_for_backward(a, b, taps)
        ctx.c = (c1, c2)
        ctx.set_materialize_grads(False)
        return means[0], means[1]

    @staticmethod
    def backward(ctx, g_ssim, g_cs):
        a, b, taps = ctx.saved_tensors
        need_a, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if (g_ssim is None and g_cs is None) or not (need_a or need_b):
            return None, None, None, None, None
        gs = g_ssim.float().contiguous() if g_ssim is not None else None
        gc = g_cs.float().contiguous() if g_cs is not None else None
        ga, gb = _require_ext("ssim_scale_bwd")(a, b, taps, gs, gc, ctx.c[0],
                                                ctx.c[1], need_a, need_b)
        return (ga if need_a else None, gb if need_b else None,
                None, None, None)


def ssim_scale(img1: torch.Tensor, img2: torch.Tensor, taps: torch.Tensor,
               c1: float = SSIM_C1, c2: float = SSIM_C2
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """One MS-SSIM scale: (mean ssim, mean cs) of two NCHW images in 0..255
    under the separable VALID blur with the 1-D filter `taps`.

    GPU: fused fp32 kernels (inputs fp32 or bf16, fp32 scalars out), analytic
    backward. CPU: the torch expression in the inputs' dtype."""
    if img1.is_cuda:
        check_ssim_taps(taps.numel(), img1.shape[2], img1.shape[3])
        return _SsimScaleFn.apply(
            img1.contiguous(), img2.contiguous(),
            taps.to(device=img1.device, dtype=torch.float32).contiguous(),
            float(c1), float(c2))
    return ref.ssim_scale_ref(img1, img2, taps, c1, c2)


class _Downsample2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor):
        ctx.hw = (x.shape[2], x.shape[3])
        ctx.bf16 = x.dtype == torch.bfloat16
        return _require_ext("down2_fwd")(x)

    @staticmethod
    def backward(ctx, g: torch.Tensor):
        return _require_ext("down2_bwd")(g.float().contiguous(), ctx.hw[0],
                                         ctx.hw[1], ctx.bf16)


def downsample2(x: torch.Tensor) -> torch.Tensor:
    """MS-SSIM dyadic downsample (N,C,H,W) -> (N,C,ceil(H/2),ceil(W/2)):
    REFLECT pad of one row/column at the end, 2-tap box filter, ::2.
    GPU: one kernel each way, fp32 out (fp32 or bf16 in). CPU: torch."""
    if x.is_cuda:
        return _Downsample2Fn.apply(x.contiguous())
    return ref.downsample2_ref(x)


# ---------------------------------------------------------------------------
# Entropy codec: per-position probclass context model + device range coder.
# HIP kernels: csrc/pc_codec.hip (step functions in csrc/rc_coder.h).
# portable=True selects the backend-id-2 specification (csrc/pc_model.h):
# HIP kernels on GPU tensors, the extension's host build on CPU tensors,
# bit-identical logits, tables and bytes on both.
# ---------------------------------------------------------------------------

PC_MAX_K = 32
PC_MAX_L = 16
PC_FREQ_SCALE = 1 << 16


def pc_live_taps(mask: torch.Tensor) -> torch.Tensor:
    """Flattened (d, kh, kw) indices of the taps a causality mask keeps."""
    return torch.nonzero(mask.reshape(-1), as_tuple=False).reshape(-1)


def check_pc_shape(pc) -> Tuple[int, int]:
    """(k, L) of a ProbClass the codec kernels serve; ValueError otherwise,
    before anything is launched."""
    k, L = int(pc.conv0.weight.shape[0]), int(pc.L)
    if int(pc.K) != 3:
        raise ValueError(f"pc codec: kernel_size must be 3, got {pc.K}")
    if not 1 <= k <= PC_MAX_K:
        raise ValueError(f"pc codec: k={k} outside [1, {PC_MAX_K}]")
    if not 2 <= L <= PC_MAX_L:
        raise ValueError(f"pc codec: L={L} outside [2, {PC_MAX_L}]")
    return k, L


@torch.no_grad()
def pc_pack_weights(pc) -> torch.Tensor:
    """Flat fp32 buffer of the four masked convs with the masked taps
    dropped by index: per layer w[tap][ci][co] over the live taps (13 for
    first_mask, 14 for other_mask) followed by the bias. Output channels of
    the three k-wide layers are zero-padded to a multiple of 8; conv2 keeps
    its L outputs. Layout documented in csrc/pc_codec.hip."""
    k, _ = check_pc_shape(pc)
    kp = (k + 7) // 8 * 8
    parts = []
    for conv, cop in ((pc.conv0, kp), (pc.res_conv1, kp),
                      (pc.res_conv2, kp), (pc.conv2, None)):
        w = conv.weight.detach().float()
        co, ci = w.shape[0], w.shape[1]
        live = pc_live_taps(conv.mask).to(w.device)
        wl = w.reshape(co, ci, -1)[:, :, live].permute(2, 1, 0)  # tap,ci,co
        b = conv.bias.detach().float()
        if cop is not None and cop != co:
            wl = torch.nn.functional.pad(wl, (0, cop - co))
            b = torch.nn.functional.pad(b, (0, cop - co))
        parts += [wl.reshape(-1), b]
    return torch.cat(parts).contiguous()


def pc_logits_packed_ref(packed: torch.Tensor, k: int, L: int,
                         ctx: torch.Tensor) -> torch.Tensor:
    """Torch evaluation of one (5, 9, 9) context from the packed layout, in
    the dtype of `packed`: what the pc_freqs kernel computes per position
    (same live taps, same layer order), used to test the packing."""
    kp = (k + 7) // 8 * 8
    ctx = ctx.to(packed.dtype)

    off = [0]

    def take(n):
        t = packed[off[0]:off[0] + n]
        off[0] += n
        return t

    def layer(x, nt, cin, cop):
        # x: (cin, D, H, W) -> (cop, D-1, H-2, W-2) over the first nt taps
        w = take(nt * cin * cop).reshape(nt, cin, cop)
        b = take(cop)
        D, H, W = x.shape[1] - 1, x.shape[2] - 2, x.shape[3] - 2
        out = b.reshape(cop, 1, 1, 1).expand(cop, D, H, W).clone()
        for t in range(nt):
            d, y, z = t // 9, (t % 9) // 3, t % 3
            win = x[:cin, d:d + D, y:y + H, z:z + W]
            out = out + torch.einsum("idhw,io->odhw", win, w[t])
        return out

    a0 = torch.relu(layer(ctx.reshape(1, 5, 9, 9), 13, 1, kp))
    a1 = torch.relu(layer(a0, 14, k, kp))
    a2 = layer(a1, 14, k, kp) + a0[:, 2:, 2:-2, 2:-2]
    return layer(a2, 14, k, L).reshape(L)


def pc_table_from_probs(p: torch.Tensor) -> torch.Tensor:
    """The hip backend's table rule on fp32 probability rows (n, L):
    f = max(1, floor(p * (65536 - L))), so tot <= 65535."""
    L = p.shape[-1]
    return torch.floor(p.float() * float(PC_FREQ_SCALE - L)).to(
        torch.int32).clamp(min=1)


def pc_host_fma_available() -> bool:
    """Whether this CPU runs the portable host path with hardware FMA."""
    return bool(_require_ext("pc_host_has_fma", "on the CPU")())


def pc_host_force_libm(on: bool) -> bool:
    """Force the portable host path through the C library's fmaf (True) or
    return to the run-time choice (False); returns the previous setting.
    Both paths give the same bits; this exists so a test can compare them."""
    return bool(_require_ext("pc_host_force_libm", "on the CPU")(bool(on)))


# Below this file there is one form, the batch form: B images of one
# symbol-volume shape share the position list and the wave schedule, q_pad is
# (B, C+4, H+8, W+8), and the extension dispatches on the device of q_pad.
# The single-image functions are B = 1 of the batch functions.

PC_MAX_BATCH = 65535  # images per launch: the kernels' gridDim.y


def _pc_args(name: str, pc, q_pad: torch.Tensor, pos: torch.Tensor,
             portable: bool = False):
    """Checks every codec call makes, then the extension entry `name` (a
    missing extension is a RuntimeError on either device); -> (entry, k, L,
    fp32 contiguous q_pad, int32 positions on its device)."""
    k, L = check_pc_shape(pc)
    if not q_pad.is_cuda and not portable:
        raise ValueError("pc codec: the hip backend needs GPU tensors")
    if q_pad.dim() != 4 or q_pad.shape[0] < 1 or min(
            q_pad.shape[1] - 4, q_pad.shape[2] - 8, q_pad.shape[3] - 8) < 1:
        raise ValueError(f"pc codec: a batched q_pad must be "
                         f"(B>=1, C+4, H+8, W+8), got {tuple(q_pad.shape)}")
    if q_pad.shape[0] > PC_MAX_BATCH:
        raise ValueError(f"pc codec: a batch of {q_pad.shape[0]} images is "
                         f"above the {PC_MAX_BATCH} one call codes; split it")
    if pos.dim() != 2 or pos.shape[1] != 3:
        raise ValueError("pc codec: positions must be (n, 3)")
    fn = _require_ext(name, "on a GPU tensor" if q_pad.is_cuda else
                      "for the portable codec on CPU tensors")
    return (fn, k, L, q_pad.float().contiguous(),
            pos.to(device=q_pad.device, dtype=torch.int32).contiguous())


def _pc_one(q_pad: torch.Tensor) -> torch.Tensor:
    """The (C+4, H+8, W+8) buffer of a single-image call as a batch of one
    (a view, so a decode still fills the caller's buffer)."""
    if q_pad.dim() != 3:
        raise ValueError(f"pc codec: q_pad must be (C+4, H+8, W+8), got "
                         f"{tuple(q_pad.shape)}")
    return q_pad[None]


def _pc_bytes_tensor(data: bytes, device) -> torch.Tensor:
    """bytes -> uint8 (len,) on device; b"" gives an empty tensor."""
    raw = torch.frombuffer(bytearray(data) if len(data) else bytearray(1),
                           dtype=torch.uint8)[:len(data)]
    return raw.to(device).contiguous()


def _pc_rows_to_bytes(rows: torch.Tensor) -> List[bytes]:
    """(B, 8 + cap) uint8 rows, each a little-endian payload length and the
    payload, -> the B payloads; a length above cap is an overrun."""
    buf = rows.cpu().numpy()
    out = []
    for b in range(buf.shape[0]):
        n = int.from_bytes(buf[b, :8].tobytes(), "little")
        if n > buf.shape[1] - 8:
            raise RuntimeError(
                f"pc_encode_batch: stream {b} of {n} bytes overran its "
                f"{buf.shape[1] - 8}-byte buffer")
        out.append(buf[b, 8:8 + n].tobytes())
    return out


@torch.no_grad()
def pc_freqs_batch(pc, q_pad: torch.Tensor, pos: torch.Tensor,
                   packed: Optional[torch.Tensor] = None,
                   portable: bool = False
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Context model at a list of positions of the padded value buffers:
    q_pad (B, C+4, H+8, W+8), positions (n, 3) shared by all images ->
    (fp32 logits (B, n, L), int32 frequency tables (B, n, L)), one launch on
    the GPU. GPU only, unless portable=True, which also serves CPU tensors.
    [b] does not depend on the other images, bit for bit."""
    fn, k, L, q_pad, pos = _pc_args("pc_freqs", pc, q_pad, pos, portable)
    if packed is None:
        packed = pc_pack_weights(pc)
    return fn(q_pad, pos, packed.to(q_pad.device), k, L, portable)


@torch.no_grad()
def pc_encode_batch(pc, q_pad: torch.Tensor, pos: torch.Tensor,
                    symbols: torch.Tensor, portable: bool = False
                    ) -> List[bytes]:
    """Range-code symbols (B, n) at positions (n, 3) in the given order: one
    stream per image, which does not depend on the other images. GPU: one
    pc_freqs launch over (positions, images), one rc_encode launch with a
    workgroup per image, one device-to-host copy for the whole batch. CPU
    (portable only): the host build, same bytes."""
    fn, k, L, q_pad, pos = _pc_args("pc_encode", pc, q_pad, pos, portable)
    if symbols.dim() != 2 or symbols.shape != (q_pad.shape[0], pos.shape[0]):
        raise ValueError(f"pc_encode_batch: symbols must be (B, n) = "
                         f"{(q_pad.shape[0], pos.shape[0])}, got "
                         f"{tuple(symbols.shape)}")
    syms = symbols.to(device=q_pad.device, dtype=torch.int32).contiguous()
    packed = pc_pack_weights(pc).to(q_pad.device)
    return _pc_rows_to_bytes(fn(q_pad, pos, syms, packed, k, L, portable))


@torch.no_grad()
def pc_decode_batch(pc, q_pad: torch.Tensor, pos: torch.Tensor, offsets,
                    datas: Sequence[bytes], centers: torch.Tensor,
                    portable: bool = False) -> torch.Tensor:
    """Wavefront decode of B streams into q_pad (B, C+4, H+8, W+8), filled
    in place with centers[symbol]; wave i is pos[offsets[i]:offsets[i+1]].
    Returns (B, C, H, W) int64 symbols. The payloads travel concatenated
    with B+1 offsets, and each image's coder reads zeros past the end of its
    own payload. One state init plus two launches per wave for any B, issued
    from C++ without a host sync."""
    fn, k, L, q_pad_c, pos = _pc_args("pc_decode", pc, q_pad, pos, portable)
    if q_pad_c.data_ptr() != q_pad.data_ptr():
        raise ValueError("pc_decode_batch: q_pad must be fp32 and contiguous")
    if len(datas) != q_pad.shape[0]:
        raise ValueError(f"pc_decode_batch: {len(datas)} streams for a batch "
                         f"of {q_pad.shape[0]}")
    data_offs = [0]
    for d in datas:
        data_offs.append(data_offs[-1] + len(d))
    return fn(q_pad, pos, [int(o) for o in offsets],
              pc_pack_weights(pc).to(q_pad.device), k, L,
              _pc_bytes_tensor(b"".join(datas), q_pad.device), data_offs,
              centers.detach().to(q_pad.device).float().contiguous(),
              portable)


@torch.no_grad()
def pc_freqs(pc, q_pad: torch.Tensor, pos: torch.Tensor,
             packed: Optional[torch.Tensor] = None, portable: bool = False
             ) -> Tuple[torch.Tensor, torch.Tensor]:
    """pc_freqs_batch of one image: q_pad (C+4, H+8, W+8) -> (fp32 logits
    (n, L), int32 frequency tables (n, L))."""
    lg, fr = pc_freqs_batch(pc, _pc_one(q_pad), pos, packed, portable)
    return lg[0], fr[0]


@torch.no_grad()
def pc_encode(pc, q_pad: torch.Tensor, pos: torch.Tensor,
              symbols: torch.Tensor, portable: bool = False) -> bytes:
    """pc_encode_batch of one image: symbols (n,) -> its stream."""
    return pc_encode_batch(pc, _pc_one(q_pad), pos, symbols[None],
                           portable)[0]


@torch.no_grad()
def pc_decode(pc, q_pad: torch.Tensor, pos: torch.Tensor, offsets,
              data: bytes, centers: torch.Tensor,
              portable: bool = False) -> torch.Tensor:
    """pc_decode_batch of one image: q_pad (C+4, H+8, W+8) is filled in
    place; returns (C, H, W) int64 symbols."""
    return pc_decode_batch(pc, _pc_one(q_pad), pos, offsets, [data], centers,
                           portable)[0]


# The ragged form: the images of a batch differ in (C, H, W). Their padded
# volumes lie in one flat fp32 value buffer, their symbols in one flat int64
# output; desc holds one row (C, H, W, volume offset, symbol offset) per
# image and positions are items (b, c, h, w). Layouts: csrc/pc_batch_host.h.

def _pc_ragged_args(name: str, pc, q: torch.Tensor, desc, items: torch.Tensor,
                    portable: bool = False):
    """Checks every ragged codec call makes; -> (the extension entry `name`,
    which is looked up when it is called, k, L, fp32 contiguous q, flat descriptor list, int32 items on
    its device, symbols in the batch)."""
    k, L = check_pc_shape(pc)
    if not q.is_cuda and not portable:
        raise ValueError("pc codec: the hip backend needs GPU tensors")
    if q.dim() != 1:
        raise ValueError(f"pc codec: a ragged value buffer must be flat, got "
                         f"{tuple(q.shape)}")
    rows = [tuple(int(v) for v in r) for r in
            (desc.tolist() if isinstance(desc, torch.Tensor) else desc)]
    if not rows or any(len(r) != 5 for r in rows):
        raise ValueError("pc codec: the descriptor table must hold at least "
                         "one row (C, H, W, volume offset, symbol offset)")
    if len(rows) > PC_MAX_BATCH:
        raise ValueError(f"pc codec: a batch of {len(rows)} images is above "
                         f"the {PC_MAX_BATCH} one call codes; split it")
    total = 0
    for b, (C, H, W, qo, so) in enumerate(rows):
        if not (1 <= C <= 0xFFFF and 1 <= H <= 0xFFFF and 1 <= W <= 0xFFFF):
            raise ValueError(f"pc codec: image {b}: C, H, W must be in "
                             f"[1, 65535], got {(C, H, W)}")
        total += C * H * W
    for what, spans, size in (
            ("padded volumes", [(r[3], (r[0] + 4) * (r[1] + 8) * (r[2] + 8))
                                for r in rows], q.numel()),
            ("symbol ranges", [(r[4], r[0] * r[1] * r[2]) for r in rows],
             total)):
        end = 0
        for off, n in sorted(spans):
            if off < end or off + n > size:
                raise ValueError(f"pc codec: the {what} of the descriptor "
                                 f"table must lie inside their buffer of "
                                 f"{size} values without overlap")
            end = off + n
    if items.dim() != 2 or items.shape[1] != 4:
        raise ValueError("pc codec: items must be (n, 4) = (b, c, h, w)")
    where = ("on a GPU tensor" if q.is_cuda else
             "for the portable codec on CPU tensors")

    def fn(*args):  # looked up at the call, after the caller's own checks
        return _require_ext(name, where)(*args)
    return (fn, k, L, q.float().contiguous(),
            [v for r in rows for v in r],
            items.to(device=q.device, dtype=torch.int32).contiguous(), total)


def _pc_offsets(name: str, what: str, offs, count: int, total: int
                ) -> List[int]:
    """count + 1 offsets running from 0 to total without decreasing."""
    offs = [int(o) for o in offs]
    if (len(offs) != count + 1 or offs[0] != 0 or offs[-1] != total
            or any(b < a for a, b in zip(offs, offs[1:]))):
        raise ValueError(f"{name}: {what} must be {count + 1} values running "
                         f"from 0 to {total} without decreasing")
    return offs


@torch.no_grad()
def pc_freqs_ragged(pc, q: torch.Tensor, desc, items: torch.Tensor,
                    packed: Optional[torch.Tensor] = None,
                    portable: bool = False
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Context model at items (n, 4) = (b, c, h, w) of a ragged batch ->
    (fp32 logits (n, L), int32 frequency tables (n, L)), row i for item i,
    one launch on the GPU. Row i is what pc_freqs gives for that position of
    image b alone, bit for bit."""
    fn, k, L, q, desc, items, _ = _pc_ragged_args("pc_freqs_ragged", pc, q,
                                                  desc, items, portable)
    if packed is None:
        packed = pc_pack_weights(pc)
    return fn(q, desc, items, packed.to(q.device), k, L, portable)


@torch.no_grad()
def pc_encode_ragged(pc, q: torch.Tensor, desc, items: torch.Tensor, starts,
                     symbols: torch.Tensor, portable: bool = False
                     ) -> List[bytes]:
    """Range-code a ragged batch: items (n, 4) sorted by (b, t, c, h, w),
    image b owns items and symbols [starts[b], starts[b+1]), symbols (n,) in
    item order. One stream per image, the bytes pc_encode gives for that
    image alone. GPU: one pc_freqs_ragged launch over all items, one
    rc_encode launch with a workgroup per image, one device-to-host copy."""
    fn, k, L, q, desc, items, _ = _pc_ragged_args("pc_encode_ragged", pc, q,
                                                  desc, items, portable)
    B, n = len(desc) // 5, items.shape[0]
    starts = _pc_offsets("pc_encode_ragged", "starts", starts, B, n)
    if symbols.dim() != 1 or symbols.shape[0] != n:
        raise ValueError(f"pc_encode_ragged: symbols must be ({n},), one per "
                         f"item, got {tuple(symbols.shape)}")
    syms = symbols.to(device=q.device, dtype=torch.int32).contiguous()
    flat = fn(q, desc, items, starts, syms, pc_pack_weights(pc).to(q.device),
              k, L, portable).cpu().numpy()
    out = []
    for b in range(B):
        row, cap = 24 * b + 3 * starts[b], 3 * (starts[b + 1] - starts[b]) + 16
        m = int.from_bytes(flat[row:row + 8].tobytes(), "little")
        if m > cap:
            raise RuntimeError(f"pc_encode_ragged: stream {b} of {m} bytes "
                               f"overran its {cap}-byte buffer")
        out.append(flat[row + 8:row + 8 + m].tobytes())
    return out


@torch.no_grad()
def pc_decode_ragged(pc, q: torch.Tensor, desc, items: torch.Tensor, seg,
                     datas: Sequence[bytes], centers: torch.Tensor,
                     portable: bool = False) -> torch.Tensor:
    """Wavefront decode of a ragged batch into the flat value buffer q,
    filled in place with centers[symbol]. items (n, 4) are sorted by (t, b,
    c, h, w) with t = 25c + 5h + w; seg holds T*B + 1 cumulative offsets:
    image b's share of wave t is items[seg[t*B+b]:seg[t*B+b+1]]. Returns the
    flat int64 symbols, image b's C*H*W values at its descriptor's symbol
    offset. One state init plus two launches per non-empty wave of the merged
    schedule, issued from C++ without a host sync; an image with nothing in
    a wave leaves its coder untouched."""
    fn, k, L, q_c, desc, items, _ = _pc_ragged_args("pc_decode_ragged", pc, q,
                                                    desc, items, portable)
    if q_c.data_ptr() != q.data_ptr():
        raise ValueError("pc_decode_ragged: q must be fp32 and contiguous")
    B, n = len(desc) // 5, items.shape[0]
    if len(datas) != B:
        raise ValueError(f"pc_decode_ragged: {len(datas)} streams for a batch "
                         f"of {B}")
    seg = [int(s) for s in seg]
    if len(seg) < B + 1 or (len(seg) - 1) % B:
        raise ValueError(f"pc_decode_ragged: the segment table must hold "
                         f"T*{B} + 1 values, got {len(seg)}")
    seg = _pc_offsets("pc_decode_ragged", "the segment table", seg,
                      len(seg) - 1, n)
    data_offs = [0]
    for d in datas:
        data_offs.append(data_offs[-1] + len(d))
    return fn(q, desc, items, seg, pc_pack_weights(pc).to(q.device), k, L,
              _pc_bytes_tensor(b"".join(datas), q.device), data_offs,
              centers.detach().to(q.device).float().contiguous(), portable)


# re-exports used across the package
kitti_normalize = ref.kitti_normalize
kitti_denormalize = ref.kitti_denormalize
pad_for_probclass = ref.pad_for_probclass_ref
extract_patches = ref.extract_patches
assemble_patches = ref.assemble_patches
