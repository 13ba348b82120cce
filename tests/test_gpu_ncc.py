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
"""

import pytest
import torch

import _oracles as O
from dsin_amd import ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _search(d, ph, pw, use_mask, dev):
    y_syn, rows, cols = ops.ncc_search(d["x"].to(dev), d["y_dec"].to(dev),
                                       d["y_orig"].to(dev), ph, pw, use_mask)
    return y_syn.cpu(), rows.cpu(), cols.cpu()


def _check_gather(y_syn, rows, cols, y_orig, ph, pw):
    """Range of the locations, and y_syn == the y_orig windows bit for bit."""
    _, h, w = y_orig.shape
    assert rows.dtype == torch.int64 and cols.dtype == torch.int64
    assert int(rows.min()) >= 0 and int(rows.max()) <= h - ph
    assert int(cols.min()) >= 0 and int(cols.max()) <= w - pw
    gw = w // pw
    for p, (r0, c0) in enumerate(zip(rows.tolist(), cols.tolist())):
        gr, gc = divmod(p, gw)
        got = y_syn[:, gr * ph:(gr + 1) * ph, gc * pw:(gc + 1) * pw]
        assert torch.equal(got, y_orig[:, r0:r0 + ph, c0:c0 + pw]), p


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
    _check_gather(y_syn, rows, cols, d["y_orig"], ph, pw)
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
    _check_gather(y_syn, rows, cols, d["y_orig"], 8, 8)
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
