"""Pure-PyTorch reference implementations of every custom op.

These are the numerics oracles for the HIP/CDNA4 kernels (tests compare the
HIP path against these in fp32) and the CPU execution path. Each function
documents the reference-repo semantics it mirrors (file:line cites are into
/root/reference).
"""

from __future__ import annotations

import math
from typing import Tuple

import torch
import torch.nn.functional as F

from ..constants import KITTI_MEAN, KITTI_STD, KITTI_STD_SIFINDER, LOG2_E

__all__ = [
    "quantize_ref",
    "heatmap3d_ref",
    "kitti_normalize",
    "kitti_denormalize",
    "bitcost_ce_ref",
    "ssim_scale_ref",
    "downsample2_ref",
    "pad_for_probclass_ref",
    "ncc_search_ref",
    "assemble_patches",
    "extract_patches",
    "gaussian_mask_value",
]

# ---------------------------------------------------------------------------
# Quantizer (reference src/quantizer_imgcomp.py:37-100 and the straight-through
# combine at src/autoencoder_imgcomp.py:127-134)
# ---------------------------------------------------------------------------

def quantize_ref(x: torch.Tensor, centers: torch.Tensor, sigma: float = 1.0
                 ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Soft-to-hard scalar quantization.

    x: (N, C, H, W) float; centers: (L,) float.
    Returns (qbar, qsoft, qhard, symbols) with qbar = qsoft + sg(qhard - qsoft).
    symbols is int64 argmin over |x - c|^2 (== argmax of softmax(-1e7 d) in the
    reference, src/quantizer_imgcomp.py:82-85).
    """
    assert centers.dim() == 1
    d = (x.unsqueeze(-1) - centers) ** 2           # (N,C,H,W,L)
    phi_soft = F.softmax(-sigma * d, dim=-1)
    qsoft = (phi_soft * centers).sum(-1)
    symbols = d.argmin(dim=-1)
    qhard = centers[symbols]
    qbar = qsoft + (qhard - qsoft).detach()
    return qbar, qsoft, qhard, symbols


# ---------------------------------------------------------------------------
# Heatmap (reference src/autoencoder_imgcomp.py:172-201)
# ---------------------------------------------------------------------------

def heatmap3d_ref(bottleneck: torch.Tensor) -> torch.Tensor:
    """bottleneck: (N, C+1, H, W); channel 0 is the heatmap logit.

    heatmap2D = sigmoid(b[:,0]) * C ; heatmap3D[.,c,.,.] = clip(heatmap2D - c, 0, 1).
    """
    C = bottleneck.shape[1] - 1
    h2d = torch.sigmoid(bottleneck[:, 0]) * C               # (N,H,W)
    c = _cached_const(tuple(float(i) for i in range(C)), bottleneck.device,
                      bottleneck.dtype, (1, C, 1, 1))
    return (h2d.unsqueeze(1) - c).clamp(0.0, 1.0)


# ---------------------------------------------------------------------------
# Fixed KITTI normalization (reference src/AE.py:222-248)
# ---------------------------------------------------------------------------

_CONST_CACHE = {}


def _cached_const(values, device, dtype, shape):
    """Per-(values, device, dtype) cached constant tensor. Avoids a pageable
    host->device copy per call — which is also forbidden inside hipGraph
    capture (hipErrorStreamCaptureUnsupported)."""
    key = (tuple(values), str(device), dtype, tuple(shape))
    t = _CONST_CACHE.get(key)
    if t is None:
        t = torch.tensor(values, device=device, dtype=dtype).view(shape)
        _CONST_CACHE[key] = t
    return t


def _mean_std(device, dtype):
    return (_cached_const(KITTI_MEAN, device, dtype, (1, 3, 1, 1)),
            _cached_const(KITTI_STD, device, dtype, (1, 3, 1, 1)))


def kitti_normalize(x: torch.Tensor) -> torch.Tensor:
    mean, std = _mean_std(x.device, x.dtype)
    return (x - mean) / std


def kitti_denormalize(x: torch.Tensor) -> torch.Tensor:
    mean, std = _mean_std(x.device, x.dtype)
    return x * std + mean


# ---------------------------------------------------------------------------
# Probclass padding + cross-entropy bitcost
# (reference src/probclass_imgcomp.py:63-106,268-292)
# ---------------------------------------------------------------------------

def pad_for_probclass_ref(q: torch.Tensor, pad: int, pad_value: torch.Tensor) -> torch.Tensor:
    """Pad NCHW with `pad` in front of C (not behind: depth_future is unseen)
    and `pad` on all four H/W sides, filled with pad_value (a 0-dim tensor,
    gradients do NOT flow into it — reference uses tf.pad constant_values).
    """
    n, c, h, w = q.shape
    out = q.new_empty(n, c + pad, h + 2 * pad, w + 2 * pad)
    if isinstance(pad_value, torch.Tensor):
        # device-side broadcast fill: no host sync (.item()) in the hot loop
        out.copy_(pad_value.detach().to(out.dtype).expand_as(out))
    else:
        out.fill_(pad_value)
    out[:, pad:, pad:-pad, pad:-pad] = q
    return out


def bitcost_ce_ref(logits: torch.Tensor, symbols: torch.Tensor) -> torch.Tensor:
    """logits: (N, L, C, H, W); symbols: (N, C, H, W) int64.
    Returns bits per symbol (N, C, H, W): softmax-CE in nats * log2(e)
    (reference src/probclass_imgcomp.py:100-106).
    """
    return F.cross_entropy(logits, symbols, reduction="none") * LOG2_E


# ---------------------------------------------------------------------------
# MS-SSIM building blocks (reference src/ms_ssim_imgcomp.py:16-64,81-112):
# one scale's (ssim, cs) means for given Gaussian taps, and the dyadic
# downsample between scales.
# ---------------------------------------------------------------------------

def _conv_valid(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """Per-channel VALID conv with one shared (1, 1, kh, kw) filter."""
    c = x.shape[1]
    return F.conv2d(x, w.expand(c, 1, w.shape[2], w.shape[3]), groups=c)


def blur_sep_ref(x: torch.Tensor, k1d: torch.Tensor) -> torch.Tensor:
    """Per-channel separable VALID conv, rows then cols (reference :31-42)."""
    x = _conv_valid(x, k1d.view(1, 1, 1, -1))
    return _conv_valid(x, k1d.view(1, 1, -1, 1))


def ssim_scale_ref(img1: torch.Tensor, img2: torch.Tensor, taps: torch.Tensor,
                   c1: float, c2: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mean ssim, mean cs) of one scale; taps is the 1-D Gaussian."""
    mu1 = blur_sep_ref(img1, taps)
    mu2 = blur_sep_ref(img2, taps)
    s11 = blur_sep_ref(img1 * img1, taps) - mu1 * mu1
    s22 = blur_sep_ref(img2 * img2, taps) - mu2 * mu2
    s12 = blur_sep_ref(img1 * img2, taps) - mu1 * mu2
    v1 = 2.0 * s12 + c2
    v2 = s11 + s22 + c2
    ssim = (((2.0 * mu1 * mu2 + c1) * v1) / ((mu1 * mu1 + mu2 * mu2 + c1) * v2)).mean()
    cs = (v1 / v2).mean()
    return ssim, cs


def downsample2_ref(x: torch.Tensor) -> torch.Tensor:
    """2-tap box filter, REFLECT pad (0 front, 1 back), separable (width then
    height), then ::2 (reference kernel_blur at :46-64 with pad_w1=0,
    pad_w2=1)."""
    x = F.pad(x, (0, 1, 0, 1), mode="reflect")
    x = _conv_valid(x, x.new_full((1, 1, 1, 2), 0.5))
    x = _conv_valid(x, x.new_full((1, 1, 2, 1), 0.5))
    return x[:, :, ::2, ::2]


# ---------------------------------------------------------------------------
# SI search: normalized cross-correlation of x_dec patches against y_dec
# (reference src/siFinder.py:7-135, src/siFull_img.py:5-68, mask from
#  src/AE.py:193-220)
# ---------------------------------------------------------------------------

def extract_patches(img: torch.Tensor, ph: int, pw: int) -> torch.Tensor:
    """img: (C, H, W) -> (P, C, ph, pw), non-overlapping, row-major patch order
    (patch p covers rows (p // (W//pw))*ph .., cols (p % (W//pw))*pw ..).
    Mirrors tf.extract_image_patches with stride == ksize
    (reference src/siFull_img.py:45-59)."""
    c, h, w = img.shape
    gh, gw = h // ph, w // pw
    p = img.view(c, gh, ph, gw, pw).permute(1, 3, 0, 2, 4).reshape(gh * gw, c, ph, pw)
    return p


def assemble_patches(patches: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """(P, C, ph, pw) -> (C, H, W), inverse of extract_patches (non-overlapping
    scatter; the reference's gradient trick at src/siFull_img.py:62-68 reduces
    to this when stride == patch size)."""
    p, c, ph, pw = patches.shape
    gh, gw = h // ph, w // pw
    assert p == gh * gw
    return patches.view(gh, gw, c, ph, pw).permute(2, 0, 3, 1, 4).reshape(c, h, w)


def _h1h2h3(x: torch.Tensor) -> torch.Tensor:
    """RGB -> (H1,H2,H3) = (R+G, R-G, 0.5(R+B)) decorrelation, channel dim=-3
    (reference src/siFinder.py:138-154; note the code comment says -0.5 but the
    code computes +0.5*(R+B) — we follow the code)."""
    r, g, b = x.unbind(dim=-3)
    return torch.stack((r + g, r - g, 0.5 * (r + b)), dim=-3)


def _sifinder_norm(x: torch.Tensor) -> torch.Tensor:
    """Per-channel fixed normalization used inside the SI search
    (reference src/siFinder.py:56-73: (v - mean) / std with the std values
    stored under the name `variances`)."""
    shape = [1] * x.dim()
    shape[-3] = 3
    mean = _cached_const(KITTI_MEAN, x.device, x.dtype, shape)
    std = _cached_const(KITTI_STD_SIFINDER, x.device, x.dtype, shape)
    return (x - mean) / std


def gaussian_mask_value(num_patches_w: int, ph: int, pw: int, H: int, W: int,
                        device, dtype) -> torch.Tensor:
    """Dense location-prior mask, shape (P, Hc, Wc) with Hc=H-ph+1, Wc=W-pw+1.

    Reference builds it as numpy constant (src/AE.py:193-220): per patch p a
    Gaussian centered at the patch center with sigma (H/2, W/2),
    g = exp(-4 ln2 ((r-cr)^2/sh^2 + (c-cw)^2/sw^2)), then crops rows
    [ph//2-1 : H-ph//2) and cols [pw//2-1 : W-pw//2).
    Only for small tests — the HIP kernel evaluates it inline (never
    materializes the ~722 MB volume at full resolution).
    """
    hc, wc = H - ph + 1, W - pw + 1
    num_p = (H // ph) * (W // pw)
    p = torch.arange(num_p, dtype=dtype)
    cr = (torch.div(p, num_patches_w, rounding_mode="floor") + 0.5) * ph   # (P,)
    cw = (p % num_patches_w + 0.5) * pw
    rows = torch.arange(ph // 2 - 1, H - ph // 2, dtype=dtype)             # (Hc,)
    cols = torch.arange(pw // 2 - 1, W - pw // 2, dtype=dtype)             # (Wc,)
    assert rows.numel() == hc and cols.numel() == wc
    sh, sw = 0.5 * H, 0.5 * W
    g = torch.exp(-4.0 * math.log(2.0)
                  * ((rows.view(1, hc, 1) - cr.view(-1, 1, 1)) ** 2 / sh ** 2
                     + (cols.view(1, 1, wc) - cw.view(-1, 1, 1)) ** 2 / sw ** 2))
    return g.to(device=device, dtype=dtype)


def rgb_to_lab_ref(x: torch.Tensor) -> torch.Tensor:
    """CIELAB transform used by the reference's use_L2andLAB search mode
    (src/siFinder.py:157-195; applied to the tensors AS-IS, i.e. in the
    raw pixel scale the caller passes — the reference does not rescale
    before the sRGB gamma expansion). x: (..., 3, H, W)."""
    px = x.movedim(-3, -1).reshape(-1, 3).float()
    lin = torch.where(px <= 0.04045, px / 12.92,
                      (((px + 0.055) / 1.055).clamp(min=0.0)) ** 2.4)
    rgb_to_xyz = _cached_const(
        ((0.412453, 0.212671, 0.019334),
         (0.357580, 0.715160, 0.119193),
         (0.180423, 0.072169, 0.950227)), x.device, torch.float32, (3, 3))
    xyz = lin @ rgb_to_xyz
    xyz = xyz * _cached_const((1.0 / 0.950456, 1.0, 1.0 / 1.088754),
                              x.device, torch.float32, (1, 3))
    eps3 = (6.0 / 29.0) ** 3
    f = torch.where(xyz <= eps3,
                    xyz / (3 * (6.0 / 29.0) ** 2) + 4.0 / 29.0,
                    xyz.clamp(min=0.0) ** (1.0 / 3.0))
    f_to_lab = _cached_const(
        ((0.0, 500.0, 0.0), (116.0, -500.0, 200.0), (0.0, 0.0, -200.0)),
        x.device, torch.float32, (3, 3))
    lab = f @ f_to_lab + _cached_const((-16.0, 0.0, 0.0), x.device,
                                       torch.float32, (1, 3))
    return lab.reshape(*x.movedim(-3, -1).shape).movedim(-1, -3)


def ncc_search_ref(x_dec: torch.Tensor, y_dec: torch.Tensor, y_orig: torch.Tensor,
                   ph: int, pw: int, use_mask: bool = True,
                   eps: float = 1e-10,
                   l2lab: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Full SI search for ONE image (the reference loops images at batch 1,
    src/siFull_img.py:15-39). All inputs (3, H, W) [y_* may be larger than
    x_dec in general; equal here]. Returns (y_syn (3,Hx,Wx), rows (P,), cols (P,)).

    Pipeline (reference src/siFinder.py:7-53):
      q = H1H2H3(fixed-norm(patches(x_dec)));  r = H1H2H3(fixed-norm(y_dec))
      pearson[p,i,j] over each ph x pw window of r vs patch p   (:76-135)
      * gaussian location prior (src/AE.py:49,193-220)
      argmax over (i,j); patches gathered FROM THE ORIGINAL y at (row, col)
      (exact slicing, the reference's batch>1 branch, src/siFinder.py:43-51);
      y_syn assembled by non-overlapping scatter (src/siFull_img.py:30-34).
    """
    c, hx, wx = x_dec.shape
    _, hy, wy = y_dec.shape
    patches = extract_patches(x_dec, ph, pw)                    # (P,3,ph,pw)
    if l2lab:
        # L2+LAB mode (src/siFinder.py:13-17): LAB transform of the RAW
        # tensors, no fixed-stats normalization
        q = rgb_to_lab_ref(patches)
        r = rgb_to_lab_ref(y_dec).unsqueeze(0)
    else:
        q = _h1h2h3(_sifinder_norm(patches))                    # (P,3,ph,pw)
        r = _h1h2h3(_sifinder_norm(y_dec)).unsqueeze(0)         # (1,3,Hy,Wy)

    n = float(ph * pw * 3)
    xy = F.conv2d(r, q)[0]                                      # (P,Hc,Wc)
    ones = r.new_ones(1, 3, ph, pw)
    sum_y = F.conv2d(r, ones)[0, 0]                             # (Hc,Wc)
    sum_y2 = F.conv2d(r * r, ones)[0, 0]
    sum_x = q.sum(dim=(1, 2, 3))                                # (P,)
    sum_x2 = (q * q).sum(dim=(1, 2, 3))
    if l2lab:
        # squared L2 distance per window (src/siFinder.py:102-103)
        ncc = (sum_x2.view(-1, 1, 1) - 2 * xy + sum_y2.unsqueeze(0))
    else:
        y_mean = sum_y / n
        x_mean = sum_x / n
        num = xy - y_mean.unsqueeze(0) * sum_x.view(-1, 1, 1) \
            - sum_y.unsqueeze(0) * x_mean.view(-1, 1, 1) \
            + n * (x_mean.view(-1, 1, 1) * y_mean.unsqueeze(0))
        den_x = sum_x2 - 2 * x_mean * sum_x + n * x_mean ** 2   # (P,)
        den_y = sum_y2 - 2 * y_mean * sum_y + n * y_mean ** 2   # (Hc,Wc)
        den = den_y.unsqueeze(0) * den_x.view(-1, 1, 1)
        ncc = num / torch.sqrt(den + eps)

    if use_mask:
        mask = gaussian_mask_value(wx // pw, ph, pw, hx, wx, x_dec.device, x_dec.dtype)
        # mask grid is sized for x_dec's extent; when y is larger the reference
        # would broadcast-fail — x and y share a size in every shipped config.
        ncc = ncc * mask

    p_count, hc, wc = ncc.shape
    # L2 mode picks the MINIMUM distance (src/siFinder.py:28-31)
    flat = ncc.view(p_count, -1)
    flat_idx = flat.argmin(dim=1) if l2lab else flat.argmax(dim=1)
    rows = torch.div(flat_idx, wc, rounding_mode="floor")
    cols = flat_idx % wc

    # gather patches from the ORIGINAL y (src/siFinder.py:41-51)
    out_patches = torch.stack(
        [y_orig[:, r0:r0 + ph, c0:c0 + pw] for r0, c0 in zip(rows.tolist(), cols.tolist())])
    y_syn = assemble_patches(out_patches, hx, wx)
    return y_syn, rows, cols
