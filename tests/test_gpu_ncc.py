"""GPU tests of the NCC side-information search (csrc/ncc_kernels.h,
csrc/ncc_search.hip) against the fp64 score map of tests/_oracles.py.

The oracle sees the operands the kernel uses (H1H2H3 rounded to bf16), so
only fp32 rounding separates the two: with e32 = max|map32 - map64| measured
on the CPU and bound = 4*e32 + 1e-5 (the floor covers the 1-ulp rsq and the
__expf of the epilogue on scores of magnitude <= 1, with a decade to spare),
a patch whose fp64 top-2 gap exceeds the bound is "decided" and the kernel
must return exactly the fp64 argmax; on any other patch its location must
score within the bound of the maximum. tests/test_oracles.py asserts on the
CPU that at least 90% of the patches of every case are decided.

Cases (H, W, ph, pw, mask), noise 8, the first of each kernel also at 25:

  v1 (pw % 8 != 0, ncc_main_kernel)
    24x80   6x10  mask   P=32, one partial column tile
    36x160  6x20  mask   Wc=141: two column tiles; P=48
    42x135  14x15        odd pw, KP > K, 61,536 B of dynamic LDS
  v2 (pw % 8 == 0, ncc_main_v2_kernel)
    21x96   3x8          pw=8 advance(), K=72, K%16=8, nkt=5 odd tail, P=84
    27x72   9x8          pw=8, K=216, one partial slice
    48x112  16x8  mask   K=384, exactly one slice; Hc=33: one row in the
                         last row block, empty second wave group; P=42
    40x144  5x24         K=360, nkt=23 odd
    64x96   16x16 mask   K=768, exactly two slices
    60x168  10x24 mask   two slices, the second with 21 chunks
    80x120  20x24 mask   the default patch, four slices
    44x200  22x40 mask   seven slices, the last odd; P=10

Every v1 case stays under 65,536 bytes of dynamic LDS by the formula of
ncc_search.hip (asserted in tests/test_oracles.py): larger v1 launches have
never been run and are not run here.

The last section holds the older checks against the fp32 torch reference
(planted shift, random images, self-match, the default 320x960 geometry).
"""

import pytest
import torch

import _oracles as O
from dsin_amd import ops
from dsin_amd.ops import reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _search(d, ph, pw, use_mask, dev):
    y_syn, rows, cols = ops.ncc_search(d["x"].to(dev), d["y_dec"].to(dev),
                                       d["y_orig"].to(dev), ph, pw, use_mask)
    return y_syn.cpu(), rows.cpu(), cols.cpu()


def _check_locations(d, rows, cols, label):
    same = (rows == d["rows"]) & (cols == d["cols"])
    dec = d["decided"]
    score = d["m64"][torch.arange(rows.numel()), rows, cols]
    short = d["vmax"] - score
    print(f"ncc {label}: P {rows.numel()} decided {int(dec.sum())} agree "
          f"{int(same.sum())} e32 {d['e32']:.2e} bound {d['bound']:.2e} "
          f"min gap {float(d['gaps'].min()):.2e} worst shortfall "
          f"{float(short.max()):.2e}")
    assert bool(same[dec].all()), torch.nonzero(dec & ~same).flatten().tolist()
    assert bool((short[~dec] <= d["bound"]).all())


# ------------------------------------------------------- 1. MFMA layout

def test_mfma_32x32x16_layout(dev):
    """Asymmetric operands: catches any A/B/C fragment-layout or transpose
    error of the 32x32x16 MFMA both main kernels use. bf16 x bf16 products
    are exact in fp32, so only the 16-term fp32 accumulation rounds:
    |C - exact| <= 16 * 2^-24 * (|A| @ |B|)."""
    from dsin_amd.ops import _dsin_hip as ext
    g = torch.Generator().manual_seed(0)
    a = torch.randn(32, 16, generator=g)
    b = torch.randn(16, 32, generator=g)
    c = ext.mfma32_selftest(a.to(dev).contiguous(), b.to(dev).contiguous())
    a64 = a.to(torch.bfloat16).double()
    b64 = b.to(torch.bfloat16).double()
    err = (c.cpu().double() - a64 @ b64).abs()
    bound = 16 * O.U32 * (a64.abs() @ b64.abs())
    print(f"mfma32: max err {float(err.max()):.2e} min bound "
          f"{float(bound.min()):.2e}")
    assert bool((err <= bound).all())


# ------------------------------- 2. + 3. exact agreement, gather invariant

@pytest.mark.parametrize("case", O.NCC_CASES, ids=str)
def test_ncc_exact_agreement_and_gather(dev, case):
    h, w, ph, pw, use_mask, noise = case
    d = O.ncc_reference(*case)
    y_syn, rows, cols = _search(d, ph, pw, use_mask, dev)
    O.ncc_check_gather(y_syn, rows, cols, d["y_orig"], ph, pw)
    _check_locations(d, rows, cols, str(case))


# ------------------------------------------------------------ 4. real ties

@pytest.mark.parametrize("tie", O.NCC_TIE_CASES, ids=str)
def test_ncc_real_ties_first_maximum_wins(dev, tie):
    """A block tiled periodically, x = y_dec = y_orig, no mask: every
    periodic copy of a patch's own location scores the same bit for bit, in
    other lanes, waves and workgroups. The packed key and the atomicMax
    must return the first copy in flat order."""
    ty, tx, ny, nx, ph, pw = tie
    y = O.ncc_tie_case(ty, tx, ny, nx)
    yg = y.to(dev)
    y_syn, rows, cols = ops.ncc_search(yg, yg, yg, ph, pw, False)
    gw = y.shape[2] // pw
    p = torch.arange(rows.numel())
    want_r = (torch.div(p, gw, rounding_mode="floor") * ph) % ty
    want_c = ((p % gw) * pw) % tx
    assert torch.equal(rows.cpu(), want_r), (rows.cpu(), want_r)
    assert torch.equal(cols.cpu(), want_c), (cols.cpu(), want_c)
    assert torch.equal(y_syn.cpu(), y)


# --------------------------------------------------------- 5. flat patches

@pytest.mark.parametrize("use_mask", [False, True])
def test_ncc_flat_patches(dev, use_mask):
    """Patches 0 and 1 are saturated in both images: their score is rounding
    noise in the reference too, so only what is defined is asserted: range
    and gather for all patches, two calls bitwise equal, and the oracle's
    location for the other, decided patches."""
    d = O.ncc_flat_case(use_mask)
    y_syn, rows, cols = _search(d, 8, 8, use_mask, dev)
    O.ncc_check_gather(y_syn, rows, cols, d["y_orig"], 8, 8)
    y2, r2, c2 = _search(d, 8, 8, use_mask, dev)
    assert torch.equal(rows, r2) and torch.equal(cols, c2)
    assert torch.equal(y_syn, y2)
    keep = torch.ones(rows.numel(), dtype=torch.bool)
    keep[:2] = False
    sub = dict(d, rows=d["rows"][keep], cols=d["cols"][keep],
               decided=d["decided"][keep], m64=d["m64"][keep],
               vmax=d["vmax"][keep], gaps=d["gaps"][keep])
    _check_locations(sub, rows[keep], cols[keep], f"flat mask={use_mask}")


# ---------------------------------------------------------- 6. determinism

@pytest.mark.parametrize("case", [O.NCC_CASES[1], O.NCC_CASES[8]], ids=str)
def test_ncc_two_calls_are_equal(dev, case):
    h, w, ph, pw, use_mask, noise = case
    d = O.ncc_reference(*case)
    y1, r1, c1 = _search(d, ph, pw, use_mask, dev)
    y2, r2, c2 = _search(d, ph, pw, use_mask, dev)
    assert torch.equal(r1, r2) and torch.equal(c1, c2) and torch.equal(y1, y2)


# ----------------------------------------------------- 7. input validation

@pytest.mark.parametrize("match,shapes,ph,pw,use_mask", [
    ("tile", [(3, 24, 80)] * 3, 5, 10, False),
    ("tile", [(3, 24, 80)] * 3, 6, 9, False),
    ("share one shape", [(3, 24, 80), (3, 24, 70), (3, 24, 80)], 6, 10, False),
    ("share one shape", [(3, 24, 80), (3, 24, 80), (3, 18, 80)], 6, 10, False),
    ("even patch sizes", [(3, 24, 80)] * 3, 3, 10, True),
    ("even patch sizes", [(3, 24, 80)] * 3, 6, 5, True),
])
def test_ncc_search_rejects_bad_inputs_on_gpu(dev, match, shapes, ph, pw,
                                              use_mask):
    imgs = [torch.zeros(s, device=dev) for s in shapes]
    with pytest.raises(ValueError, match=match):
        ops.ncc_search(*imgs, ph, pw, use_mask)


# ------------------------- 8. the older checks against the fp32 reference

def _agree_or_tied(ncc_map, kernel_rows, kernel_cols, ref_rows, ref_cols, tol):
    """Kernel argmax must equal ref argmax OR land on a near-tie (bf16 MFMA
    vs fp32 reference rounding)."""
    P = ncc_map.shape[0]
    ok = 0
    for p in range(P):
        if int(kernel_rows[p]) == int(ref_rows[p]) and int(kernel_cols[p]) == int(ref_cols[p]):
            ok += 1
            continue
        vmax = ncc_map[p].max()
        vk = ncc_map[p, int(kernel_rows[p]), int(kernel_cols[p])]
        assert vk >= vmax - tol, (p, float(vk), float(vmax))
        ok += 1
    assert ok == P


def _ref_ncc_map(x, y_dec, ph, pw, use_mask=True):
    """Dense reference correlation map (P, Hc, Wc) for tie checking."""
    import torch.nn.functional as F
    patches = ref.extract_patches(x, ph, pw)
    q = ref._h1h2h3(ref._sifinder_norm(patches))
    r = ref._h1h2h3(ref._sifinder_norm(y_dec)).unsqueeze(0)
    n = float(ph * pw * 3)
    xy = F.conv2d(r, q)[0]
    ones = r.new_ones(1, 3, ph, pw)
    sum_y = F.conv2d(r, ones)[0, 0]
    sum_y2 = F.conv2d(r * r, ones)[0, 0]
    y_mean = sum_y / n
    sum_x = q.sum(dim=(1, 2, 3))
    sum_x2 = (q * q).sum(dim=(1, 2, 3))
    x_mean = sum_x / n
    num = xy - y_mean.unsqueeze(0) * sum_x.view(-1, 1, 1) \
        - sum_y.unsqueeze(0) * x_mean.view(-1, 1, 1) \
        + n * (x_mean.view(-1, 1, 1) * y_mean.unsqueeze(0))
    den_x = sum_x2 - 2 * x_mean * sum_x + n * x_mean ** 2
    den_y = sum_y2 - 2 * y_mean * sum_y + n * y_mean ** 2
    ncc = num / torch.sqrt(den_y.unsqueeze(0) * den_x.view(-1, 1, 1) + 1e-10)
    if use_mask:
        c, hx, wx = x.shape
        mask = ref.gaussian_mask_value(wx // pw, ph, pw, hx, wx, x.device, x.dtype)
        ncc = ncc * mask
    return ncc


def test_ncc_planted_shift(dev):
    torch.manual_seed(5)
    h, w, ph, pw, shift = 80, 120, 20, 24, 12
    base = torch.rand(3, h, w + shift, device=dev) * 255
    x = base[:, :, shift:].contiguous()
    y = base[:, :, :w].contiguous()
    y_syn, rows, cols = ops.ncc_search(x, y, y, ph, pw, True)
    gw = w // pw
    for p in range((h // ph) * gw):
        gr, gc = divmod(p, gw)
        if gc * pw + shift + pw <= w:
            assert int(rows[p]) == gr * ph
            assert int(cols[p]) == gc * pw + shift


def test_ncc_matches_reference_random(dev):
    torch.manual_seed(6)
    h, w, ph, pw = 80, 120, 20, 24
    base = torch.rand(3, h // 8 + 1, w // 8 + 1, device=dev)
    x = torch.nn.functional.interpolate(base[None], size=(h, w),
                                        mode="bilinear")[0] * 255
    ydec = (x + torch.randn_like(x) * 8).clamp(0, 255)
    yorig = (ydec + torch.randn_like(x) * 2).clamp(0, 255)
    y_syn_k, rows_k, cols_k = ops.ncc_search(x, ydec, yorig, ph, pw, True)
    y_syn_r, rows_r, cols_r = ref.ncc_search_ref(x.cpu(), ydec.cpu(),
                                                 yorig.cpu(), ph, pw, True)
    ncc_map = _ref_ncc_map(x.cpu().float(), ydec.cpu().float(), ph, pw)
    _agree_or_tied(ncc_map, rows_k.cpu(), cols_k.cpu(), rows_r, cols_r, 5e-3)
    same = (rows_k.cpu() == rows_r) & (cols_k.cpu() == cols_r)
    assert same.float().mean() > 0.8  # most patches bit-agree with fp32 ref
    # wherever argmax agrees, the gathered output must match exactly
    gw = w // pw
    for p in torch.nonzero(same).flatten().tolist():
        gr, gc = divmod(p, gw)
        sl = (slice(None), slice(gr * ph, gr * ph + ph), slice(gc * pw, gc * pw + pw))
        torch.testing.assert_close(y_syn_k.cpu()[sl], y_syn_r[sl])


def test_ncc_nomask(dev):
    torch.manual_seed(7)
    h, w, ph, pw = 64, 96, 16, 16
    x = torch.rand(3, h, w, device=dev) * 255
    y_syn, rows, cols = ops.ncc_search(x, x, x, ph, pw, False)
    # identical images, no mask: each patch finds itself
    gw = w // pw
    for p in range((h // ph) * gw):
        gr, gc = divmod(p, gw)
        assert int(rows[p]) == gr * ph and int(cols[p]) == gc * pw
    torch.testing.assert_close(y_syn, x)


def test_ncc_default_patch_shapes(dev):
    """Full default-config geometry: 320x960, 20x24 patches, 640 patches."""
    torch.manual_seed(8)
    base = torch.rand(3, 41, 121, device=dev)
    x = torch.nn.functional.interpolate(base[None], size=(320, 960),
                                        mode="bilinear")[0] * 255
    y = (x + torch.randn_like(x) * 5).clamp(0, 255)
    y_syn, rows, cols = ops.ncc_search(x.contiguous(), y.contiguous(),
                                       y.contiguous(), 20, 24, True)
    assert y_syn.shape == (3, 320, 960)
    assert rows.numel() == 640
    assert int(rows.max()) <= 300 and int(cols.max()) <= 936
