"""CPU contract of the MS-SSIM ops: ops.ssim_scale / ops.downsample2 on CPU
tensors compute exactly what losses/msssim.py computed before the ops
existed, and multiscale_ssim on CPU is unchanged.

`_old_*` below is a frozen copy of that earlier torch implementation, kept
here so the comparison is against fixed code and not against whatever the
package currently delegates to."""

import pytest
import torch
import torch.nn.functional as F

from dsin_amd import ops
from dsin_amd.losses import multiscale_ssim
from dsin_amd.losses.msssim import _gauss_kernel1d

_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def _old_conv_valid(x, w):
    c = x.shape[1]
    return F.conv2d(x, w.expand(c, 1, w.shape[2], w.shape[3]), groups=c)


def _old_blur_sep(x, k1d):
    x = _old_conv_valid(x, k1d.view(1, 1, 1, -1))
    return _old_conv_valid(x, k1d.view(1, 1, -1, 1))


def _old_ssim_scale(img1, img2, max_val=255.0, filter_size=11,
                    filter_sigma=1.5, k1=0.01, k2=0.03):
    _, _, h, w = img1.shape
    size = min(filter_size, h, w)
    sigma = size * filter_sigma / filter_size
    k = _gauss_kernel1d(sigma, size, img1.device, img1.dtype)
    mu1 = _old_blur_sep(img1, k)
    mu2 = _old_blur_sep(img2, k)
    s11 = _old_blur_sep(img1 * img1, k) - mu1 * mu1
    s22 = _old_blur_sep(img2 * img2, k) - mu2 * mu2
    s12 = _old_blur_sep(img1 * img2, k) - mu1 * mu2
    c1 = (k1 * max_val) ** 2
    c2 = (k2 * max_val) ** 2
    v1 = 2.0 * s12 + c2
    v2 = s11 + s22 + c2
    ssim = (((2.0 * mu1 * mu2 + c1) * v1) / ((mu1 * mu1 + mu2 * mu2 + c1) * v2)).mean()
    cs = (v1 / v2).mean()
    return ssim, cs


def _old_downsample2(x):
    x = F.pad(x, (0, 1, 0, 1), mode="reflect")
    x = _old_conv_valid(x, x.new_full((1, 1, 1, 2), 0.5))
    x = _old_conv_valid(x, x.new_full((1, 1, 2, 1), 0.5))
    return x[:, :, ::2, ::2]


def _old_multiscale_ssim(img1, img2):
    im1, im2 = img1, img2
    mssim, mcs = [], []
    for _ in range(len(_WEIGHTS)):
        ssim, cs = _old_ssim_scale(im1, im2)
        mssim.append(ssim)
        mcs.append(cs)
        im1, im2 = _old_downsample2(im1), _old_downsample2(im2)
    out = img1.new_ones(())
    for w, cs in zip(_WEIGHTS[:-1], mcs[:-1]):
        out = out * cs ** w
    return out * mssim[-1] ** _WEIGHTS[-1]


def _pair(h, w, seed, b=2, c=3):
    g = torch.Generator().manual_seed(seed)
    img1 = torch.rand(b, c, h, w, generator=g) * 255
    img2 = (img1 + torch.randn(b, c, h, w, generator=g) * 10).clamp(0, 255)
    return img1, img2


@pytest.mark.parametrize("h,w", [(35, 69), (72, 104)])
def test_ssim_scale_cpu_equals_previous_torch_code(h, w):
    img1, img2 = _pair(h, w, seed=h)
    size = min(11, h, w)
    taps = _gauss_kernel1d(size * 1.5 / 11, size, img1.device, img1.dtype)
    ssim, cs = ops.ssim_scale(img1, img2, taps)
    ssim_old, cs_old = _old_ssim_scale(img1, img2)
    assert torch.equal(ssim, ssim_old)
    assert torch.equal(cs, cs_old)


@pytest.mark.parametrize("h,w", [(35, 69), (72, 104)])
def test_downsample2_cpu_equals_previous_torch_code(h, w):
    img1, _ = _pair(h, w, seed=w)
    out = ops.downsample2(img1)
    assert out.shape == (2, 3, (h + 1) // 2, (w + 1) // 2)
    assert torch.equal(out, _old_downsample2(img1))


def test_multiscale_ssim_cpu_unchanged():
    torch.manual_seed(1234)
    base = torch.rand(1, 3, 23, 23)
    img1 = F.interpolate(base, size=(176, 176), mode="bilinear") * 255
    img2 = (img1 + torch.randn_like(img1) * 10).clamp(0, 255)
    v = multiscale_ssim(img1, img2)
    # bit-identical to the earlier implementation evaluated alongside ...
    assert torch.equal(v, _old_multiscale_ssim(img1, img2))
    # ... and equal to the value it produced when this test was written
    # (0x1.f978dap-1), up to conv rounding differences between CPU builds
    assert abs(float(v) - 0.9872501492500305) <= 1e-6


def test_gpu_size_check_is_a_value_error():
    with pytest.raises(ValueError, match="11-tap"):
        ops.check_ssim_taps(11, 10, 40)
    with pytest.raises(ValueError, match="odd"):
        ops.check_ssim_taps(10, 40, 40)
    ops.check_ssim_taps(11, 11, 200)
