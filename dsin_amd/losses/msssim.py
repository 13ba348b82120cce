"""Differentiable multi-scale SSIM (training-loss variant).

Mirror of the reference TF implementation (src/ms_ssim_imgcomp.py):
separable 1D Gaussian blur applied per channel with VALID boundary handling
(:16-43: no padding when the image is at least kernel-sized), per-scale
SSIM/CS means (:81-112), 2-tap box [1/2,1/2] separable downsample padded
REFLECT (0 before, 1 after) then ::2 decimation (:46-64,179-181), 5 scales
with the paper weights [0.0448, 0.2856, 0.3001, 0.2363, 0.1333] combined as
prod(cs[:4]**w[:4]) * ssim[4]**w[4] (:164-186). Inputs NCHW in 0..255.

The per-scale statistics and the downsample are ops (ops.ssim_scale,
ops.downsample2): fused fp32 HIP kernels with an analytic backward on GPU
tensors, the torch expressions on CPU tensors. Only the five-weight
combination is left to autograd.
"""

from __future__ import annotations

from typing import Dict, Tuple

import torch

from .. import ops

_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def _gauss_kernel1d(sigma: float, size: int, device, dtype) -> torch.Tensor:
    n = size // 2
    x = torch.arange(-n, n + 1, device=device, dtype=dtype)
    g = torch.exp(-x * x / (2.0 * sigma * sigma))
    return g / g.abs().sum()


_DEVICE_TAPS: Dict[tuple, torch.Tensor] = {}


def _device_taps(sigma: float, size: int, device) -> torch.Tensor:
    """fp32 taps for the GPU kernels: built once on the host and kept on the
    device, so a loss evaluation does no host-to-device copy (and can be
    graph-captured once warmed up)."""
    key = (float(sigma), int(size), str(device))
    taps = _DEVICE_TAPS.get(key)
    if taps is None:
        taps = _gauss_kernel1d(sigma, size, "cpu", torch.float32).to(device)
        _DEVICE_TAPS[key] = taps
    return taps


def _scale_filter(h: int, w: int, filter_size: int, filter_sigma: float
                  ) -> Tuple[int, float]:
    size = min(filter_size, h, w)
    return size, size * filter_sigma / filter_size


def _ssim_scale(img1: torch.Tensor, img2: torch.Tensor, max_val: float,
                filter_size: int, filter_sigma: float, k1: float, k2: float
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    _, _, h, w = img1.shape
    size, sigma = _scale_filter(h, w, filter_size, filter_sigma)
    if img1.is_cuda:
        k = _device_taps(sigma, size, img1.device)
    else:
        k = _gauss_kernel1d(sigma, size, img1.device, img1.dtype)
    c1 = (k1 * max_val) ** 2
    c2 = (k2 * max_val) ** 2
    return ops.ssim_scale(img1, img2, k, c1, c2)


def _check_gpu_sizes(h: int, w: int, filter_size: int, filter_sigma: float):
    """The GPU path supports exactly the sizes the torch path accepts: at
    every scale the (odd) filter length must fit the image. Checked for all
    scales up front, so nothing is launched for an unsupported size."""
    for scale in range(len(_WEIGHTS)):
        size, _ = _scale_filter(h, w, filter_size, filter_sigma)
        ops.check_ssim_taps(2 * (size // 2) + 1, h, w,
                            what=f"multiscale_ssim scale {scale}")
        h, w = (h + 1) // 2, (w + 1) // 2


def multiscale_ssim(img1: torch.Tensor, img2: torch.Tensor, max_val: float = 255.0,
                    filter_size: int = 11, filter_sigma: float = 1.5,
                    k1: float = 0.01, k2: float = 0.03) -> torch.Tensor:
    assert img1.shape == img2.shape and img1.dim() == 4
    if img1.is_cuda:
        _check_gpu_sizes(img1.shape[2], img1.shape[3], filter_size, filter_sigma)
    im1, im2 = img1, img2
    mssim = []
    mcs = []
    last = len(_WEIGHTS) - 1
    for scale in range(len(_WEIGHTS)):
        ssim, cs = _ssim_scale(im1, im2, max_val, filter_size, filter_sigma, k1, k2)
        mssim.append(ssim)
        mcs.append(cs)
        if scale < last:
            im1, im2 = ops.downsample2(im1), ops.downsample2(im2)
    out = img1.new_ones(())
    for w, cs in zip(_WEIGHTS[:-1], mcs[:-1]):
        out = out * cs ** w
    return out * mssim[-1] ** _WEIGHTS[-1]
