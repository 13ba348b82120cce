"""GPU tests of the pointwise and reduction kernels (csrc/quantizer.hip,
bitcost.hip, fused.hip, adam.hip) against fp64 oracles on identical data.

House rule of tests/test_gpu_msssim.py: inputs are generated on the CPU with
a seeded generator and rounded to the dtype the kernel reads; the oracle is
the torch expression in fp64; e32 is the measured error of the same
expression in fp32 on the CPU; the kernel must satisfy

    |gpu - fp64| <= 4*e32 + floor

with a floor of a few fp32 ulp of the result's scale, stated per test. Where
a result is a difference of larger terms, the scale is that of the terms.
A sum of n terms gets depth*2^-24*sum|t_i| for the longest chain of
additions a summand passes through; a bf16 store adds 2^-8*|ref|.

The fast exponential: __expf(a) is exp2(a*log2(e)) with the product rounded
in fp32, so its relative error is about |a|*2^-24 plus an ulp. A softmax
term with a < -16 is below 2^-23 of the largest, so 16*2^-24 bounds the
relative error of every term that matters (U_EXP below).
"""

import math

import pytest
import torch
import torch.nn.functional as F

import _oracles as O
from dsin_amd import ops
from dsin_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

U32, U16 = O.U32, O.U16
U_EXP = 16 * U32
LOG2E = 1.4426950408889634


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _report(name, err, bound, e32):
    ratio = float((err / bound).max())
    print(f"{name}: max err {float(err.max()):.3e} e32 {e32:.3e} min bound "
          f"{float(bound.min()):.3e} worst err/bound {ratio:.3f}")
    return ratio


def _e(a32, a64):
    return float((a32.double() - a64).abs().max())


# ---------------------------------------------------------------- quantizer

def _quantizer_depth(n):
    """quantize_bwd_kernel: the thread's own elements, 6 shuffle steps, 3
    additions over the 4 waves, at most grid-1 in the sum over the blocks;
    plus 16 for the rounding of the summand itself (U_EXP)."""
    grid = min(-(-n // 256), 2048)
    return -(-n // (grid * 256)) + 6 + 3 + (grid - 1) + 16


def _check_quantizer(dev, x, centers, g, sigma, backward=True, name="quant"):
    r64 = O.quantize_oracle(x, centers, sigma, g, torch.float64)
    r32 = O.quantize_oracle(x, centers, sigma, g, torch.float32)
    xg = x.to(dev).requires_grad_(True)
    cg = centers.to(dev).requires_grad_(True)
    qbar, sym = ops.quantize(xg, cg, sigma)
    ok = r64["relgap"] > 1e-6
    assert float(ok.float().mean()) >= 0.99
    assert torch.equal(sym.cpu()[ok], r64["sym"][ok])
    # qbar = qsoft + (qhard - qsoft): a few ulp of the centers' scale
    q32 = ref_qbar32(x, centers, sigma)
    cmax = float(centers.abs().max())
    bound = 4 * _e(q32, r64["qhard"]) + 4 * 2 * U32 * cmax + 0 * x.double()
    err = (qbar.detach().cpu().double() - r64["qhard"]).abs()
    worst = _report(f"{name} qbar", err[ok], bound[ok], _e(q32, r64["qhard"]))
    assert worst <= 1.0
    if not backward:
        return
    gx, gc = torch.autograd.grad(qbar, (xg, cg), g.to(dev))
    assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gc).all())
    # gx = g*(sum_l c_l phi_l w_l - qsoft*sum_l phi_l w_l), w = -2 sigma
    # (x - c_l): the scale is that of the two terms, each off by U_EXP
    x64, c64 = x.double().unsqueeze(-1), centers.double()
    phi = F.softmax(-sigma * (x64 - c64) ** 2, dim=-1)
    w = (2 * sigma * (x64 - c64)).abs()
    qsoft = (phi * c64).sum(-1)
    scale = g.double().abs() * ((c64.abs() * phi * w).sum(-1)
                                + qsoft.abs() * (phi * w).sum(-1))
    e_gx = _e(r32["gx"], r64["gx"])
    bound = 4 * e_gx + U_EXP * scale + 1e-30
    err = (gx.cpu().double() - r64["gx"]).abs()
    assert _report(f"{name} gx", err, bound, e_gx) <= 1.0
    e_gc = _e(r32["gc"], r64["gc"])
    bound = 4 * e_gc + _quantizer_depth(x.numel()) * U32 * r64["gc_abs"]
    err = (gc.cpu().double() - r64["gc"]).abs()
    assert _report(f"{name} gc", err, bound, e_gc) <= 1.0


def ref_qbar32(x, centers, sigma):
    x, c = x.float(), centers.float()
    d = (x.unsqueeze(-1) - c) ** 2
    qsoft = (F.softmax(-sigma * d, dim=-1) * c).sum(-1)
    qhard = c[d.argmin(dim=-1)]
    return qsoft + (qhard - qsoft)


@pytest.mark.parametrize("sigma", [0.5, 1.0, 4.0])
@pytest.mark.parametrize("L", [1, 6, 16])
def test_quantizer_matches_fp64(dev, L, sigma):
    x, centers, g = O.quantizer_inputs(3 * 7 * 11 * 13, L, seed=L)
    _check_quantizer(dev, x, centers, g, sigma, name=f"quant L={L} s={sigma}")


@pytest.mark.parametrize("n,backward", [(1048576 + 771, False),
                                        (524288 + 771, True)])
def test_quantizer_grid_stride(dev, n, backward):
    """The grid-stride loops: past 4096*256 elements forward, past 2048*256
    backward."""
    x, centers, g = O.quantizer_inputs(n, 6, seed=3)
    _check_quantizer(dev, x, centers, g, 1.0, backward, name=f"quant n={n}")


def test_quantizer_exact_ties(dev):
    """x halfway between two centers (both distances 0.25 or 2.25, exact in
    fp32): the symbol is the lower index, as argmin gives, qbar is that
    center exactly, and the gradient is finite and matches."""
    centers = torch.tensor([-2.0, -1.0, 0.0, 1.0, 2.0])
    x = torch.tensor([-1.5, -0.5, 0.5, 1.5]).repeat(75)
    g = torch.randn(x.numel(), generator=torch.Generator().manual_seed(5))
    want = torch.tensor([0, 1, 2, 3]).repeat(75)
    assert torch.equal(((x.unsqueeze(-1) - centers) ** 2).argmin(-1), want)
    xg = x.to(dev).requires_grad_(True)
    cg = centers.to(dev).requires_grad_(True)
    qbar, sym = ops.quantize(xg, cg, 1.0)
    assert torch.equal(sym.cpu(), want)
    assert torch.equal(qbar.detach().cpu(), centers[want])
    gx, gc = torch.autograd.grad(qbar, (xg, cg), g.to(dev))
    r64 = O.quantize_oracle(x, centers, 1.0, g, torch.float64)
    r32 = O.quantize_oracle(x, centers, 1.0, g, torch.float32)
    assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gc).all())
    # |dq/dx| <= 2 sigma * sum |c phi (x - c)| < 16 here
    bound = 4 * _e(r32["gx"], r64["gx"]) + U_EXP * 16 * g.double().abs() + 1e-30
    assert bool(((gx.cpu().double() - r64["gx"]).abs() <= bound).all())
    bound = (4 * _e(r32["gc"], r64["gc"])
             + _quantizer_depth(x.numel()) * U32 * r64["gc_abs"])
    assert bool(((gc.cpu().double() - r64["gc"]).abs() <= bound).all())


def test_quantizer_rejects_more_than_16_centers(dev):
    x = torch.zeros(8, device=dev)
    with pytest.raises(RuntimeError, match="at most"):
        ops.quantize(x, torch.linspace(-2, 2, 17, device=dev))


# ------------------------------------------------------------------ bitcost

@pytest.mark.parametrize("chw", [(5, 7, 9), (32, 40, 60)])
@pytest.mark.parametrize("L", [2, 6, 16])
def test_bitcost_matches_fp64(dev, L, chw):
    """N=3 (so the image index of a site goes above 0), logits scaled by 30
    and on half of the sites one class at +80. Floors: bits = (lse -
    logit[sym])*log2e, a difference of two terms of the logits' scale:
    8 ulp of |lse| + |logit[sym]|; dlogits = g*log2e*(softmax - onehot):
    U_EXP of g*log2e (the softmax is at most 1)."""
    n = 3
    gen = torch.Generator().manual_seed(L * 100 + chw[0])
    logits = torch.randn(n, L, *chw, generator=gen) * 30
    hot = torch.randint(0, L, (n, 1, *chw), generator=gen)
    on = torch.rand(n, 1, *chw, generator=gen) < 0.5
    logits = torch.where(on & (torch.arange(L).view(1, L, 1, 1, 1) == hot),
                         torch.full_like(logits, 80.0), logits)
    sym = torch.randint(0, L, (n, *chw), generator=gen)
    g = torch.rand(n, *chw, generator=gen)

    def run(dt):
        lg = logits.clone().to(dt).requires_grad_(True)
        bits = F.cross_entropy(lg, sym, reduction="none") * LOG2E
        (gl,) = torch.autograd.grad(bits, lg, g.to(dt))
        return bits.detach(), gl
    b64, gl64 = run(torch.float64)
    b32, gl32 = run(torch.float32)
    lgd = logits.to(dev).requires_grad_(True)
    bits = ops.bitcost_ce(lgd, sym.to(dev))
    (gl,) = torch.autograd.grad(bits, lgd, g.to(dev))
    l64 = logits.double()
    scale = (torch.logsumexp(l64, dim=1).abs()
             + l64.gather(1, sym.unsqueeze(1)).squeeze(1).abs()) * LOG2E
    err = (bits.detach().cpu().double() - b64).abs()
    bound = 4 * _e(b32, b64) + 8 * U32 * scale + 8 * U32
    assert _report(f"bitcost L={L} {chw} bits", err, bound, _e(b32, b64)) <= 1
    err = (gl.cpu().double() - gl64).abs()
    bound = 4 * _e(gl32, gl64) + U_EXP * LOG2E * g.double().unsqueeze(1) + 1e-30
    bound = bound.expand_as(err)
    assert _report(f"bitcost L={L} {chw} dlogits", err, bound,
                   _e(gl32, gl64)) <= 1


# ------------------------------------------------------- l1_mean_per_image

def _l1_depth(chw):
    """l1_part_kernel: the thread's own elements, 6 shuffle steps, 3 over the
    4 waves, S-1 over the slices; 2 more for the subtraction and the final
    division."""
    s = min(max(chw // 4096, 1), 64)
    return -(-chw // (s * 256)) + 6 + 3 + (s - 1) + 2


@pytest.mark.parametrize("xdt", [torch.float32, torch.bfloat16], ids=str)
@pytest.mark.parametrize("ydt", [torch.float32, torch.bfloat16], ids=str)
@pytest.mark.parametrize("shape,need", [((3, 3, 64, 96), "xy"),
                                        ((3, 4, 33, 47), "xy"),
                                        ((3, 4, 33, 47), "x"),
                                        ((3, 4, 33, 47), "y")])
def test_l1_mean_matches_fp64(dev, shape, need, xdt, ydt):
    """CHW = 3*64*96 gives S=4 slices, 4*33*47 one. Every tenth entry has
    x == y exactly: the gradient there is 0. The gradient is -+sign(y-x)*
    g/CHW, one fp32 division: 2 ulp, plus 2^-8 where it is stored in bf16."""
    gen = torch.Generator().manual_seed(shape[2])
    x = (torch.randn(shape, generator=gen) * 50).to(xdt)
    y = (torch.randn(shape, generator=gen) * 50).to(ydt)
    same = torch.zeros(shape, dtype=torch.bool)
    same.view(-1)[::10] = True
    common = x.to(torch.bfloat16)
    x = torch.where(same, common.to(xdt), x)
    y = torch.where(same, common.to(ydt), y)
    gout = torch.randn(shape[0], generator=gen)
    chw = x[0].numel()

    def run(dt):
        a = x.clone().to(dt).requires_grad_(True)
        b = y.clone().to(dt).requires_grad_(True)
        m = (b - a).abs().mean(dim=(1, 2, 3))
        ga, gb = torch.autograd.grad(m, (a, b), gout.to(dt))
        return m.detach(), ga, gb
    m64, gx64, gy64 = run(torch.float64)
    m32, gx32, gy32 = run(torch.float32)
    xg = x.to(dev).requires_grad_("x" in need)
    yg = y.to(dev).requires_grad_("y" in need)
    m = ops.l1_mean_per_image(xg, yg)
    assert m.dtype == torch.float32
    m.backward(gout.to(dev))
    err = (m.detach().cpu().double() - m64).abs()
    bound = 4 * _e(m32, m64) + _l1_depth(chw) * U32 * m64  # m64 = sum|t|/CHW
    assert _report(f"l1 {shape} {xdt}/{ydt} mean", err, bound,
                   _e(m32, m64)) <= 1
    for t, g64, g32, dt, want in ((xg, gx64, gx32, xdt, "x" in need),
                                  (yg, gy64, gy32, ydt, "y" in need)):
        if not want:
            assert t.grad is None
            continue
        assert t.grad.dtype == dt
        got = t.grad.cpu().double()
        assert bool((got[same] == 0).all())
        rel = 2 * U32 + (U16 if dt == torch.bfloat16 else 0.0)
        assert bool(((got - g64).abs() <= 4 * _e(g32, g64)
                     + rel * g64.abs()).all())


# --------------------------------------------------------------- rate_terms

@pytest.mark.parametrize("heat_grad", [False, True])
@pytest.mark.parametrize("shape", [(1, 4, 10, 12), (1, 7, 33, 47)])
def test_rate_terms_match_fp64(dev, shape, heat_grad):
    """n = 480 (below 4096: one slice) and n = 10857 (two slices, not a
    multiple of 256). Sums take the depth bound (own elements, 6 shuffle
    steps, 3 over the waves, S-1 slices, 2 for the product and the
    division); gradients are g1/n + g2/n*heat and g2/n*bc: 4 ulp of the
    terms, plus 2^-8 for the bf16 store of the heat gradient."""
    gen = torch.Generator().manual_seed(shape[1])
    bc = torch.rand(shape, generator=gen) * 3
    heat = torch.rand(shape, generator=gen).to(torch.bfloat16)
    n = bc.numel()
    s = min(max(n // 4096, 1), 64)
    depth = -(-n // (s * 256)) + 6 + 3 + (s - 1) + 2
    w1, w2 = 2.0, 3.0

    def run(dt):
        a = bc.clone().to(dt).requires_grad_(True)
        h = heat.clone().to(dt).requires_grad_(True)
        hr, hm = a.mean(), (a * h).mean()
        ga, gh = torch.autograd.grad(w1 * hr + w2 * hm, (a, h))
        return hr.detach(), hm.detach(), ga, gh
    hr64, hm64, ga64, gh64 = run(torch.float64)
    hr32, hm32, ga32, gh32 = run(torch.float32)
    a = bc.to(dev).requires_grad_(True)
    h = heat.to(dev).requires_grad_(heat_grad)
    hr, hm = ops.rate_terms(a, h)
    (w1 * hr + w2 * hm).backward()
    for name, got, r64, r32, scale in (
            ("H_real", hr, hr64, hr32, bc.double().abs().mean()),
            ("H_mask", hm, hm64, hm32,
             (bc.double() * heat.double()).abs().mean())):
        err = (got.detach().cpu().double() - r64).abs().reshape(1)
        bound = (4 * _e(r32, r64) + depth * U32 * scale).reshape(1)
        assert _report(f"rate {shape} {name}", err, bound, _e(r32, r64)) <= 1
    err = (a.grad.cpu().double() - ga64).abs()
    bound = 4 * _e(ga32, ga64) + 4 * U32 * (w1 + w2 * heat.double()) / n
    assert _report(f"rate {shape} g_bc", err, bound, _e(ga32, ga64)) <= 1
    if heat_grad:
        assert h.grad.dtype == torch.bfloat16
        err = (h.grad.cpu().double() - gh64).abs()
        bound = 4 * _e(gh32, gh64) + (U16 + 4 * U32) * gh64.abs() + 1e-30
        assert _report(f"rate {shape} g_heat", err, bound, _e(gh32, gh64)) <= 1
    else:
        assert h.grad is None


# ------------------------------------------------------------- heatmap_mask

@pytest.mark.parametrize("which", ["both", "z", "h3"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
def test_heatmap_mask_matches_fp64(dev, dtype, which):
    """h2 = C*sigmoid(b0) with the fast exponential: the relative error of
    exp(-b0) is (|b0| + 2) ulp, the sigmoid's slope is at most 1/4, and the
    division, the product with C and the subtraction of c add 3 ulp of C:

        floor_h = C * 2^-24 * ((|b0| + 2)/4 + 3)

    bounds h3; z = h3*b[c+1] and g_b[c+1] = g_z*h3 carry it times the
    factor plus 2 ulp of the result; g_b0 = acc*C*s*(1-s) (acc has at most
    two terms) carries |acc|*floor_h plus 8 ulp. bf16 outputs add
    2^-8*|ref|. On every 7th pixel b0 = 0, so h2 - c is exactly 1 at c = 15
    and exactly 0 at c = 16: both edges count as inside for the gradient,
    as torch's clamp does. Pixels where a rounding decides the branch
    (O.heatmap_inputs, under 1%) are left out of the g_b0 comparison."""
    b, edge = O.heatmap_inputs(dtype)
    C = b.shape[1] - 1
    gen = torch.Generator().manual_seed(12)
    gz = torch.randn(b.shape[0], C, *b.shape[2:], generator=gen).to(dtype).float()
    gh = torch.randn(b.shape[0], C, *b.shape[2:], generator=gen).to(dtype).float()
    bf = U16 if dtype == torch.bfloat16 else 0.0

    def outs_and_grad(z, h3, bb, cast):
        if which == "both":
            return torch.autograd.grad((z, h3), bb, (cast(gz), cast(gh)))[0]
        if which == "z":
            return torch.autograd.grad(z, bb, cast(gz))[0]
        return torch.autograd.grad(h3, bb, cast(gh))[0]

    def run(dt):
        bb = b.clone().to(dt).requires_grad_(True)
        h2 = torch.sigmoid(bb[:, 0]) * C
        h3 = (h2.unsqueeze(1) - torch.arange(C, dtype=dt).view(1, C, 1, 1)
              ).clamp(0.0, 1.0)
        z = h3 * bb[:, 1:]
        gb = outs_and_grad(z, h3, bb, lambda t: t.to(dt))
        return z.detach(), h3.detach(), gb
    z64, h64, gb64 = run(torch.float64)
    z32, h32, gb32 = run(torch.float32)
    bg = b.to(dev, dtype).requires_grad_(True)
    z, h3 = ops.heatmap_mask(bg)
    assert z.dtype == dtype and h3.dtype == dtype
    gb = outs_and_grad(z, h3, bg, lambda t: t.to(dev, dtype))
    z, h3, gb = (t.detach().cpu().double() for t in (z, h3, gb))

    b64 = b.double()
    floor_h = (C * U32 * ((b64[:, 0].abs() + 2) / 4 + 3)).unsqueeze(1)
    name = f"heatmap {dtype} {which}"
    # the exact pixels: h3 is exactly 1 up to c = 15 and 0 from c = 16
    exact = (b[:, 0] == 0).unsqueeze(1).expand_as(h3)
    assert bool((h3[exact] == h64[exact]).all())
    bound = 4 * _e(h32, h64) + floor_h + bf * h64
    assert _report(f"{name} h3", (h3 - h64).abs(), bound.expand_as(h64),
                   _e(h32, h64)) <= 1
    bound = (4 * _e(z32, z64) + floor_h * b64[:, 1:].abs()
             + (bf + 2 * U32) * z64.abs() + 1e-30)
    assert _report(f"{name} z", (z - z64).abs(), bound, _e(z32, z64)) <= 1
    # g_b[c+1] = g_z * h3
    e_g = _e(gb32, gb64)
    bound = (4 * e_g + floor_h * gz.double().abs()
             + (bf + 2 * U32) * gb64[:, 1:].abs() + 1e-30)
    assert _report(f"{name} g_b[1:]", (gb[:, 1:] - gb64[:, 1:]).abs(), bound,
                   e_g) <= 1
    # g_b0 = acc * C*s*(1-s)
    s = torch.sigmoid(b64[:, 0])
    acc = gb64[:, 0] / (C * s * (1 - s))
    bound = (4 * e_g + acc.abs() * floor_h[:, 0]
             + (bf + 8 * U32) * gb64[:, 0].abs() + 1e-30)
    err = (gb[:, 0] - gb64[:, 0]).abs()
    assert float(edge.float().mean()) < 0.01
    assert _report(f"{name} g_b0", err[~edge], bound[~edge], e_g) <= 1


# --------------------------------------------------------------- adam_step

@pytest.mark.parametrize("use_wd", [False, True])
@pytest.mark.parametrize("sizes", O.ADAM_SMALL_SIZES + [O.ADAM_LARGE_SIZES],
                         ids=lambda s: "n=%d" % sum(math.prod(t) for t in s))
def test_fused_adam_matches_fp64(dev, sizes, use_wd):
    """Flat n in {1, 3, 4, 5, 7, 46} (n < 4 and every n % 4) and one buffer
    of 2,097,152 + 1027 elements (the grid-stride loop), with and without
    weight decay on the last parameter; three steps, lr changed on the
    device in between. Bound derived in O.run_adam_case."""
    worst = O.run_adam_case(sizes, use_wd, dev)
    print(f"adam {sizes} wd={use_wd}: worst err/bound {worst:.3f}")


# ------------------------------------- against the fp32 torch reference
# The older per-op checks, kept as they were: each kernel against the
# pure-torch fp32 expression in dsin_amd.ops.reference or in eager torch.

def test_quantize_fwd_matches_ref(dev):
    torch.manual_seed(1)
    x = torch.randn(1, 32, 40, 120, device=dev) * 2
    centers = torch.linspace(-2, 2, 6, device=dev)
    qbar, symbols = ops.quantize(x, centers)
    qref, _, qhard, sref = ref.quantize_ref(x, centers)
    assert torch.equal(symbols, sref)
    torch.testing.assert_close(qbar, qref, rtol=1e-5, atol=1e-6)


def test_quantize_bwd_matches_autograd(dev):
    torch.manual_seed(2)
    x = torch.randn(1, 8, 10, 12, device=dev, requires_grad=True)
    centers = torch.linspace(-2, 2, 6, device=dev, requires_grad=True)
    qbar, _ = ops.quantize(x, centers)
    g = torch.randn_like(qbar)
    gx, gc = torch.autograd.grad(qbar, (x, centers), g)

    x2 = x.detach().clone().requires_grad_(True)
    c2 = centers.detach().clone().requires_grad_(True)
    qref, _, _, _ = ref.quantize_ref(x2, c2)
    gx2, gc2 = torch.autograd.grad(qref, (x2, c2), g)
    torch.testing.assert_close(gx, gx2, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(gc, gc2, rtol=1e-4, atol=1e-4)


def test_bitcost_fwd_matches_ref(dev):
    torch.manual_seed(3)
    logits = torch.randn(1, 6, 32, 40, 60, device=dev)
    symbols = torch.randint(0, 6, (1, 32, 40, 60), device=dev)
    bits = ops.bitcost_ce(logits, symbols)
    expect = ref.bitcost_ce_ref(logits, symbols)
    torch.testing.assert_close(bits, expect, rtol=1e-5, atol=1e-5)


def test_bitcost_bwd_matches_autograd(dev):
    torch.manual_seed(4)
    logits = torch.randn(1, 6, 8, 10, 12, device=dev, requires_grad=True)
    symbols = torch.randint(0, 6, (1, 8, 10, 12), device=dev)
    bits = ops.bitcost_ce(logits, symbols)
    g = torch.rand_like(bits)
    (gl,) = torch.autograd.grad(bits, logits, g)

    l2 = logits.detach().clone().requires_grad_(True)
    expect = ref.bitcost_ce_ref(l2, symbols)
    (gl2,) = torch.autograd.grad(expect, l2, g)
    torch.testing.assert_close(gl, gl2, rtol=1e-4, atol=1e-6)


def test_heatmap_mask_matches_eager(dev):
    from dsin_amd import ops
    from dsin_amd.ops import reference as ref
    torch.manual_seed(5)
    for dtype in (torch.float32, torch.bfloat16):
        b = torch.randn(2, 33, 10, 12, device=dev, dtype=dtype) * 3
        b1 = b.clone().requires_grad_(True)
        z, h3 = ops.heatmap_mask(b1)
        b2 = b.clone().float().requires_grad_(True)
        h3r = ref.heatmap3d_ref(b2)
        zr = h3r * b2[:, 1:]
        torch.testing.assert_close(z.float(), zr, rtol=2e-2, atol=2e-2)
        torch.testing.assert_close(h3.float(), h3r, rtol=2e-2, atol=2e-2)
        gz = torch.randn_like(zr)
        gh = torch.randn_like(h3r)
        (z.float() * gz + h3.float() * gh).sum().backward()
        (zr * gz + h3r * gh).sum().backward()
        torch.testing.assert_close(b1.grad.float(), b2.grad, rtol=5e-2,
                                   atol=5e-2)


def test_l1_mean_matches_eager(dev):
    from dsin_amd import ops
    torch.manual_seed(6)
    x = torch.randn(3, 4, 33, 47, device=dev) * 50
    y = (torch.randn(3, 4, 33, 47, device=dev) * 50).to(torch.bfloat16)
    x1 = x.clone().requires_grad_(True)
    y1 = y.clone().requires_grad_(True)
    m = ops.l1_mean_per_image(x1, y1)
    x2 = x.clone().requires_grad_(True)
    y2 = y.clone().requires_grad_(True)
    mr = (y2.float() - x2).abs().mean(dim=(1, 2, 3))
    torch.testing.assert_close(m, mr, rtol=1e-4, atol=1e-4)
    g = torch.randn(3, device=dev)
    (m * g).sum().backward()
    (mr * g).sum().backward()
    torch.testing.assert_close(x1.grad, x2.grad, rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(y1.grad.float(), y2.grad.float(), rtol=1e-2,
                               atol=1e-2)


def test_rate_terms_match_eager(dev):
    from dsin_amd import ops
    torch.manual_seed(7)
    bc = (torch.rand(1, 32, 40, 60, device=dev) * 3).requires_grad_(True)
    heat = torch.rand(1, 32, 40, 60, device=dev).to(torch.bfloat16)
    heat.requires_grad_(True)
    hr, hm = ops.rate_terms(bc, heat)
    bc2 = bc.detach().clone().requires_grad_(True)
    h2 = heat.detach().clone().requires_grad_(True)
    hr2 = bc2.mean()
    hm2 = (bc2 * h2).mean()
    torch.testing.assert_close(hr, hr2, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(hm, hm2, rtol=1e-3, atol=1e-4)
    (2.0 * hr + 3.0 * hm).backward()
    (2.0 * hr2 + 3.0 * hm2).backward()
    torch.testing.assert_close(bc.grad, bc2.grad, rtol=1e-3, atol=1e-6)
    torch.testing.assert_close(heat.grad.float(), h2.grad.float(), rtol=1e-2,
                               atol=1e-5)


def test_fused_adam_matches_tf_semantics(dev):
    """FusedAdam vs a hand-rolled TF AdamOptimizer reference:
    p -= lr sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + eps)."""
    from dsin_amd.ops.adam import FusedAdam
    torch.manual_seed(0)
    shapes = [(3, 5), (7,), (2, 3, 4)]
    init = [torch.randn(s, device=dev) for s in shapes]
    params = [torch.nn.Parameter(t.clone()) for t in init]
    opt = FusedAdam(params, lr=1e-2)

    ref_p = [t.clone() for t in init]
    ref_m = [torch.zeros_like(t) for t in init]
    ref_v = [torch.zeros_like(t) for t in init]
    b1, b2, eps, lr = 0.9, 0.999, 1e-8, 1e-2

    for t_step in range(1, 4):
        grads = [torch.randn_like(t) for t in init]
        opt.zero_grad()
        for p, g in zip(params, grads):
            p.grad = g.clone()   # autograd "steals" grads in the new flow
        opt.gather_grads()
        opt.step()
        for i in range(len(ref_p)):
            ref_m[i] = b1 * ref_m[i] + (1 - b1) * grads[i]
            ref_v[i] = b2 * ref_v[i] + (1 - b2) * grads[i] ** 2
            corr = lr * (1 - b2 ** t_step) ** 0.5 / (1 - b1 ** t_step)
            ref_p[i] -= corr * ref_m[i] / (ref_v[i].sqrt() + eps)
        for p, r in zip(params, ref_p):
            torch.testing.assert_close(p.data, r, rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------- refusals

def _refusals(dev):
    """(entry, arguments, the argument the error must name): raw extension
    entries given one tensor of the wrong dtype, shape or element count."""
    f32 = dict(device=dev, dtype=torch.float32)
    b16 = dict(device=dev, dtype=torch.bfloat16)
    y = torch.zeros(1, 2, 2, 2, **b16)
    c2 = torch.ones(2, **f32)
    return [
        ("heatmap_mask_bwd", (torch.zeros(1, 3, 2, 2, **b16),
                              torch.zeros(1, 2, 2, 2, **f32), None), "gz"),
        ("l1_bwd", (torch.zeros(2, 3, **f32), torch.zeros(2, 3, **f32),
                    torch.zeros(2, **b16), True, True), "g"),
        ("bn_bwd", (y, y, torch.zeros(1, 2, 2, 3, **b16), c2, c2, c2, True,
                    0), "out"),
        ("bn_fwd", (y, torch.ones(2, **b16), c2, c2.clone(), c2.clone(), 0.1,
                    1e-5, True, 0, None), "gamma"),
        ("bitcost_ce_bwd", (torch.zeros(1, 1, 2, 2, **f32),
                            torch.zeros(1, 3, 1, 2, 2, **f32),
                            torch.zeros(1, 1, 2, 2, device=dev,
                                        dtype=torch.int32)), "symbols"),
        ("quantize_bwd", (torch.zeros(4, **b16), torch.zeros(4, **f32),
                          torch.linspace(-1, 1, 3, **f32), 1.0), "g"),
        ("hterms_bwd", (torch.zeros(4, **f32), torch.zeros(4, **b16),
                        torch.zeros(3, **f32), False), "g2"),
    ]


@pytest.mark.parametrize("i", range(7))
def test_entry_point_refuses_unchecked_tensor(dev, i):
    """Each of these dereferenced the tensor without looking at it; now the
    call raises before anything is launched and names op and argument."""
    from dsin_amd.ops import _dsin_hip as ext
    name, args, arg = _refusals(dev)[i]
    with pytest.raises(RuntimeError, match=rf"{name}: {arg}\b"):
        getattr(ext, name)(*args)
