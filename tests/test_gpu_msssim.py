"""GPU tests of the fused fp32 MS-SSIM kernels (csrc/msssim.hip).

Oracle: the torch path in fp64 on the CPU, on identical data (inputs are
generated in fp64 and cast). The bound is self-calibrating: on each input
the error e32 of the fp32 CPU torch path against fp64 is measured, and the
GPU result must satisfy

    value:     |gpu - fp64|      <= 4 * e32      + 1e-6
    gradient:  relL2(gpu, fp64)  <= 4 * e32_grad + 1e-5

The factor 4 covers the different summation order of tiled partial sums;
the floors are about 8 fp32 ulp at 1.0 (and the same relative to the
gradient norm).
"""

import functools
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from dsin_amd import ops
from dsin_amd.losses import Distortions, multiscale_ssim
from dsin_amd.losses.msssim import _gauss_kernel1d
from dsin_amd.ops import reference as ref

BF16_EPS = 2.0 ** -9  # round-to-nearest relative error of a bf16 store


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _pair64(shape, sigma, seed=0):
    """Seeded smooth fp64 image in 0..255 and a noisy, clamped copy."""
    b, c, h, w = shape
    g = torch.Generator().manual_seed(seed + 1000 * int(sigma))
    base = torch.rand(b, c, h // 4 + 2, w // 4 + 2, generator=g,
                      dtype=torch.float64) * 255
    a = F.interpolate(base, size=(h, w), mode="bilinear", align_corners=False)
    n = torch.randn(a.shape, generator=g, dtype=torch.float64) * sigma
    return a, (a + n).clamp(0, 255)


def _rel_l2(x, ref64):
    return float((x.double().cpu() - ref64).norm() / ref64.norm())


def _value_and_grads(fn, a, b):
    a = a.clone().requires_grad_(True)
    b = b.clone().requires_grad_(True)
    v = fn(a, b)
    ga, gb = torch.autograd.grad(v, (a, b))
    return v.detach(), ga, gb


@functools.lru_cache(maxsize=None)
def _full_ref(shape, sigma):
    """fp64 oracle and the fp32-CPU error e32 for the full loss (computed
    once per input, shared by the tests, never modified)."""
    a, b = _pair64(shape, sigma)
    v64, ga64, gb64 = _value_and_grads(multiscale_ssim, a, b)
    v32, ga32, gb32 = _value_and_grads(multiscale_ssim, a.float(), b.float())
    return dict(a=a, b=b, v=float(v64), ga=ga64, gb=gb64,
                e_v=abs(float(v32) - float(v64)),
                e_ga=_rel_l2(ga32, ga64), e_gb=_rel_l2(gb32, gb64))


FULL_SHAPES = [(1, 3, 35, 69), (2, 3, 72, 104), (2, 3, 176, 200),
               (7, 1, 200, 240)]


# ------------------------------------------------------------ 1. full value

@pytest.mark.parametrize("sigma", [3.0, 15.0])
@pytest.mark.parametrize("shape", FULL_SHAPES)
def test_full_value_matches_fp64(dev, shape, sigma):
    r = _full_ref(shape, sigma)
    v = multiscale_ssim(r["a"].float().to(dev), r["b"].float().to(dev))
    assert v.dtype == torch.float32 and v.dim() == 0
    err, bound = abs(float(v) - r["v"]), 4 * r["e_v"] + 1e-6
    print(f"msssim {shape} sigma={sigma}: gpu {float(v):.9f} fp64 "
          f"{r['v']:.9f} err {err:.3e} e32 {r['e_v']:.3e} bound {bound:.3e}")
    assert err <= bound


# ------------------------------------------------------ 2. per-scale op

W_SSIM, W_CS = 0.7, 1.3  # upstream weights, so both gradient paths are live

# (shape, T): one-row output map; output width 33 = tile width + 1; the
# shrunken filters of the small scales; more than one tile each way
SCALE_CASES = [((1, 1, 11, 200), 11), ((1, 2, 30, 43), 11),
               ((2, 3, 70, 75), 11), ((1, 3, 23, 41), 9),
               ((2, 1, 18, 37), 5), ((1, 3, 9, 5), 3)]


def _scale_ref(a, b, taps64):
    """(ssim, cs, grad_a, grad_b) in fp64 and the fp32-CPU errors."""
    def run(dt):
        x = a.to(dt).requires_grad_(True)
        y = b.to(dt).requires_grad_(True)
        s, c = ref.ssim_scale_ref(x, y, taps64.to(dt), ops.SSIM_C1, ops.SSIM_C2)
        gx, gy = torch.autograd.grad(W_SSIM * s + W_CS * c, (x, y))
        return float(s.detach()), float(c.detach()), gx, gy
    s64, c64, ga64, gb64 = run(torch.float64)
    s32, c32, ga32, gb32 = run(torch.float32)
    return dict(s=s64, c=c64, ga=ga64, gb=gb64, e_s=abs(s32 - s64),
                e_c=abs(c32 - c64), e_ga=_rel_l2(ga32, ga64),
                e_gb=_rel_l2(gb32, gb64))


@pytest.mark.parametrize("sigma", [3.0, 15.0])
@pytest.mark.parametrize("shape,T", SCALE_CASES)
def test_ssim_scale_matches_fp64(dev, shape, T, sigma):
    a, b = _pair64(shape, sigma, seed=T)
    taps64 = _gauss_kernel1d(T * 1.5 / 11, T, "cpu", torch.float64)
    r = _scale_ref(a, b, taps64)
    ag = a.float().to(dev).requires_grad_(True)
    bg = b.float().to(dev).requires_grad_(True)
    s, c = ops.ssim_scale(ag, bg, taps64.float().to(dev))
    ga, gb = torch.autograd.grad(W_SSIM * s + W_CS * c, (ag, bg))
    s, c = float(s.detach()), float(c.detach())
    print(f"ssim_scale {shape} T={T} sigma={sigma}: "
          f"ssim err {abs(s - r['s']):.3e} (e32 {r['e_s']:.3e}) "
          f"cs err {abs(c - r['c']):.3e} (e32 {r['e_c']:.3e}) "
          f"ga {_rel_l2(ga, r['ga']):.3e} (e32 {r['e_ga']:.3e}) "
          f"gb {_rel_l2(gb, r['gb']):.3e} (e32 {r['e_gb']:.3e})")
    assert abs(s - r["s"]) <= 4 * r["e_s"] + 1e-6
    assert abs(c - r["c"]) <= 4 * r["e_c"] + 1e-6
    assert _rel_l2(ga, r["ga"]) <= 4 * r["e_ga"] + 1e-5
    assert _rel_l2(gb, r["gb"]) <= 4 * r["e_gb"] + 1e-5


@pytest.mark.parametrize("first_bf16", [False, True])
def test_ssim_scale_bf16_inputs(dev, first_bf16):
    """bf16 images (the reconstruction, or both): the oracle gets the
    bf16-rounded values in fp64. Values obey the usual bound. A gradient
    returned in bf16 carries the store's rounding on top: each element is
    off by at most 2^-9 relative, hence at most 2^-9 in relative L2."""
    shape, T = (2, 3, 40, 75), 11
    a, b = _pair64(shape, 15.0, seed=5)
    b = b.to(torch.bfloat16).double()
    if first_bf16:
        a = a.to(torch.bfloat16).double()
    taps64 = _gauss_kernel1d(1.5, T, "cpu", torch.float64)
    r = _scale_ref(a, b, taps64)
    ag = a.to(device=dev, dtype=torch.bfloat16 if first_bf16 else torch.float32)
    ag.requires_grad_(True)
    bg = b.to(device=dev, dtype=torch.bfloat16).requires_grad_(True)
    s, c = ops.ssim_scale(ag, bg, taps64.float().to(dev))
    assert s.dtype == torch.float32 and c.dtype == torch.float32
    ga, gb = torch.autograd.grad(W_SSIM * s + W_CS * c, (ag, bg))
    assert gb.dtype == torch.bfloat16 and ga.dtype == ag.dtype
    assert abs(float(s.detach()) - r["s"]) <= 4 * r["e_s"] + 1e-6
    assert abs(float(c.detach()) - r["c"]) <= 4 * r["e_c"] + 1e-6
    assert _rel_l2(gb, r["gb"]) <= 4 * r["e_gb"] + 1e-5 + BF16_EPS
    assert _rel_l2(ga, r["ga"]) <= (4 * r["e_ga"] + 1e-5
                                    + (BF16_EPS if first_bf16 else 0.0))


# ------------------------------------------------------- 3. downsample

@pytest.mark.parametrize("shape", [(2, 3, 35, 69), (2, 3, 72, 104),
                                   (1, 3, 2, 2)])
def test_downsample2_fwd_bwd_match_torch(dev, shape):
    g = torch.Generator().manual_seed(shape[2])
    x = torch.rand(shape, generator=g) * 255
    xc = x.clone().requires_grad_(True)
    yc = ref.downsample2_ref(xc)
    up = torch.randn(yc.shape, generator=g)
    (gc,) = torch.autograd.grad(yc, xc, up)
    xg = x.to(dev).requires_grad_(True)
    yg = ops.downsample2(xg)
    (gg,) = torch.autograd.grad(yg, xg, up.to(dev))
    assert yg.shape == yc.shape
    torch.testing.assert_close(yg.cpu(), yc.detach(), rtol=1e-6, atol=1e-5)
    torch.testing.assert_close(gg.cpu(), gc, rtol=1e-6, atol=1e-5)


def test_downsample2_bf16_input(dev):
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(1, 2, 35, 69, generator=g) * 255).to(torch.bfloat16)
    y = ops.downsample2(x.to(dev))
    assert y.dtype == torch.float32
    torch.testing.assert_close(y.cpu(), ref.downsample2_ref(x.float()),
                               rtol=1e-6, atol=1e-5)


# ------------------------------------------- 4. gradient of the full loss

@pytest.mark.parametrize("sigma", [3.0, 15.0])
@pytest.mark.parametrize("shape", [(2, 3, 72, 104), (1, 3, 176, 200)])
def test_full_gradient_matches_fp64(dev, shape, sigma):
    r = _full_ref(shape, sigma)
    # the usual case: only the reconstruction requires grad
    a_nograd = r["a"].float().to(dev)
    b = r["b"].float().to(dev).requires_grad_(True)
    multiscale_ssim(a_nograd, b).backward()
    assert a_nograd.grad is None
    e1 = _rel_l2(b.grad, r["gb"])
    # both inputs
    a = r["a"].float().to(dev).requires_grad_(True)
    b2 = r["b"].float().to(dev).requires_grad_(True)
    ga, gb = torch.autograd.grad(multiscale_ssim(a, b2), (a, b2))
    print(f"msssim grad {shape} sigma={sigma}: gb {e1:.3e} / "
          f"{_rel_l2(gb, r['gb']):.3e} (e32 {r['e_gb']:.3e}) "
          f"ga {_rel_l2(ga, r['ga']):.3e} (e32 {r['e_ga']:.3e})")
    assert e1 <= 4 * r["e_gb"] + 1e-5
    assert _rel_l2(gb, r["gb"]) <= 4 * r["e_gb"] + 1e-5
    assert _rel_l2(ga, r["ga"]) <= 4 * r["e_ga"] + 1e-5
    assert torch.equal(gb, b.grad)


# ------------------------------------------------------ 5. determinism

def _value_and_grad_gpu(a, b):
    b = b.detach().requires_grad_(True)
    v = multiscale_ssim(a, b)
    (g,) = torch.autograd.grad(v, b)
    return v.detach(), g


def test_two_evaluations_are_bitwise_equal(dev):
    r = _full_ref((2, 3, 176, 200), 3.0)
    a, b = r["a"].float().to(dev), r["b"].float().to(dev)
    v1, g1 = _value_and_grad_gpu(a, b)
    v2, g2 = _value_and_grad_gpu(a, b)
    assert torch.equal(v1, v2) and torch.equal(g1, g2)


# ----------------------------------------------------- 6. graph capture

def test_graph_capture_replay_equals_eager(dev):
    shape = (1, 3, 176, 200)
    r1, r2 = _full_ref(shape, 3.0), _full_ref(shape, 15.0)
    a1, b1 = r1["a"].float().to(dev), r1["b"].float().to(dev)
    a2, b2 = r2["a"].float().to(dev), r2["b"].float().to(dev)
    v1, g1 = _value_and_grad_gpu(a1, b1)
    v2, g2 = _value_and_grad_gpu(a2, b2)

    sa = a1.clone()
    sb = b1.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            torch.autograd.grad(multiscale_ssim(sa, sb), sb)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sv = multiscale_ssim(sa, sb)
        (sg,) = torch.autograd.grad(sv, sb)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(sv, v1) and torch.equal(sg, g1)
    with torch.no_grad():
        sa.copy_(a2)
        sb.copy_(b2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(sv, v2) and torch.equal(sg, g2)


# --------------------------------------------------- 7. unsupported size

def test_unsupported_size_raises_value_error(dev):
    x = torch.rand(1, 3, 64, 96, device=dev) * 255
    with pytest.raises(ValueError, match="scale 3"):
        multiscale_ssim(x, x.clone())
    with pytest.raises(ValueError):
        ops.ssim_scale(x[:, :, :10], x[:, :, :10],
                       torch.full((11,), 1 / 11.0, device=dev))


# ------------------------------------------------------- 8. loss wiring

def test_distortions_ms_ssim_on_gpu(dev, ae_config):
    cfg = ae_config.clone()
    cfg.distortion_to_minimize = "ms_ssim"
    r = _full_ref((1, 3, 200, 240), 15.0)
    x, x_out = r["a"].float().to(dev), r["b"].float().to(dev)
    d = Distortions(cfg, x, x_out, is_training=True)
    expect = cfg.K_ms_ssim * (1.0 - r["v"])
    bound = cfg.K_ms_ssim * (4 * r["e_v"] + 1e-6)
    print(f"d_loss_scaled {float(d.d_loss_scaled):.6f} expect {expect:.6f} "
          f"bound {bound:.3e}")
    assert abs(float(d.d_loss_scaled) - expect) <= bound


def test_train_steps_with_ms_ssim_distortion(dev):
    from dsin_amd import config as cm
    from dsin_amd.models import DSIN
    from dsin_amd.training import Trainer
    from dsin_amd.data import SyntheticStereo
    here = os.path.dirname(os.path.abspath(__file__))
    ae, _ = cm.parse(os.path.join(here, "..", "run_configs", "ae_run_configs"))
    pc, _ = cm.parse(os.path.join(here, "..", "run_configs", "pc_run_configs"))
    ae.crop_size = (200, 240)
    ae.distortion_to_minimize = "ms_ssim"
    torch.manual_seed(0)
    model = DSIN(ae, pc).to(dev)
    tr = Trainer(model, ae, pc, num_training_imgs=1576, device=dev,
                 autocast_bf16=True)
    gen = SyntheticStereo(200, 240, device=str(dev))
    for _ in range(2):
        x, y = gen.next_batch()
        loss, bpp = tr.train_step(x, y)
        assert torch.isfinite(loss) and torch.isfinite(bpp)


# ------------------------------------- 9. the remaining dispatch paths

MIX_SHAPE, MIX_T = (1, 2, 13, 45), 11  # 3 x 35 outputs: two tiles in x


def _mix_inputs(dev, first_bf16):
    """One image bf16, the other fp32; fp64 copies of the rounded values."""
    a, b = _pair64(MIX_SHAPE, 15.0, seed=9)
    if first_bf16:
        a = a.to(torch.bfloat16).double()
    else:
        b = b.to(torch.bfloat16).double()
    adt = torch.bfloat16 if first_bf16 else torch.float32
    bdt = torch.float32 if first_bf16 else torch.bfloat16
    taps64 = _gauss_kernel1d(1.5, MIX_T, "cpu", torch.float64)
    return (a, b, a.to(device=dev, dtype=adt), b.to(device=dev, dtype=bdt),
            taps64)


def test_ssim_scale_first_bf16_second_fp32(dev):
    """The (bf16, fp32) instantiation of both kernels, which
    test_ssim_scale_bf16_inputs does not reach; same bounds."""
    a, b, ag, bg, taps64 = _mix_inputs(dev, True)
    r = _scale_ref(a, b, taps64)
    ag.requires_grad_(True)
    bg.requires_grad_(True)
    s, c = ops.ssim_scale(ag, bg, taps64.float().to(dev))
    ga, gb = torch.autograd.grad(W_SSIM * s + W_CS * c, (ag, bg))
    assert ga.dtype == torch.bfloat16 and gb.dtype == torch.float32
    print(f"ssim err {abs(float(s) - r['s']):.3e} (e32 {r['e_s']:.3e}) "
          f"cs err {abs(float(c) - r['c']):.3e} (e32 {r['e_c']:.3e}) "
          f"ga {_rel_l2(ga, r['ga']):.3e} (e32 {r['e_ga']:.3e}) "
          f"gb {_rel_l2(gb, r['gb']):.3e} (e32 {r['e_gb']:.3e})")
    assert abs(float(s.detach()) - r["s"]) <= 4 * r["e_s"] + 1e-6
    assert abs(float(c.detach()) - r["c"]) <= 4 * r["e_c"] + 1e-6
    assert _rel_l2(ga, r["ga"]) <= 4 * r["e_ga"] + 1e-5 + BF16_EPS
    assert _rel_l2(gb, r["gb"]) <= 4 * r["e_gb"] + 1e-5


@pytest.mark.parametrize("first_bf16", [False, True])
def test_ssim_scale_single_gradient_equals_joint(dev, first_bf16):
    """Only one image requires grad: the backward launches once, and for the
    first image with the two images (and element types) swapped. The
    gradient is the one the joint call returns, bit for bit."""
    _, _, ag, bg, taps64 = _mix_inputs(dev, first_bf16)
    taps = taps64.float().to(dev)

    def grads(need_a, need_b):
        x = ag.clone().requires_grad_(need_a)
        y = bg.clone().requires_grad_(need_b)
        s, c = ops.ssim_scale(x, y, taps)
        wrt = [t for t in (x, y) if t.requires_grad]
        return torch.autograd.grad(W_SSIM * s + W_CS * c, wrt)

    ga, gb = grads(True, True)
    (ga1,) = grads(True, False)
    (gb1,) = grads(False, True)
    assert ga1.dtype == ga.dtype and torch.equal(ga1, ga)
    assert gb1.dtype == gb.dtype and torch.equal(gb1, gb)


def test_downsample2_bwd_bf16_input(dev):
    """bf16 input, both sides odd (both reflected taps live): the gradient
    comes back in bf16, each element within 2^-9 relative of the fp32
    gradient of downsample2_ref.

    The upstream gradient holds integers in -4..4, so every element of the
    fp32 gradient is k/4 with |k| <= 16, a bf16 number: 2^-9 is half of what
    one correct bf16 rounding may cost (half an ulp of an 8-bit significand
    is up to 2^-8 of the value), so it can be held elementwise only where
    the store has nothing to round, and then a wrong tap, weight or index
    shows in full. With a normal upstream (first version of this test) a
    correctly rounded store measured 2.846e-3 = 1.46 * 2^-9 worst, at the
    parent and here alike. That store is checked second, under the bound of
    the format: 2^-8 relative, plus 8 * 2^-24 of the largest upstream value
    for the fp32 sums (three additions of at most four such values, scaled
    by 1/4, on each side)."""
    g = torch.Generator().manual_seed(57)
    x = (torch.rand(1, 2, 5, 7, generator=g) * 255).to(torch.bfloat16)
    xg = x.to(dev).requires_grad_(True)
    yg = ops.downsample2(xg)
    ups = (torch.randint(-4, 5, yg.shape, generator=g).float(),
           torch.randn(yg.shape, generator=g))
    for up, rel, floor in ((ups[0], BF16_EPS, 0.0),
                           (ups[1], 2 * BF16_EPS,
                            8 * 2.0 ** -24 * float(ups[1].abs().max()))):
        xc = x.float().requires_grad_(True)
        (gc,) = torch.autograd.grad(ref.downsample2_ref(xc), xc, up)
        (gg,) = torch.autograd.grad(yg, xg, up.to(dev), retain_graph=True)
        assert gg.dtype == torch.bfloat16 and gg.shape == x.shape
        err = (gg.float().cpu() - gc).abs()
        print(f"down2 bwd bf16: worst err {float(err.max()):.3e}, bound "
              f"{rel:.3e}*|ref| + {floor:.1e}")
        assert bool((err <= rel * gc.abs() + floor).all()), float(err.max())
