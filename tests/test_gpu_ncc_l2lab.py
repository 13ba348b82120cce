"""GPU tests of the L2+LAB mode of the side-information search
(lab_transform_kernel and the L2 instantiations of the two main kernels in
csrc/ncc_kernels.h) against the fp64 oracle of tests/_oracles_l2lab.py.

The oracle is given the bf16 LAB operands the device really used
(ops.ncc_lab_transform), so only fp32 rounding separates the two; its
pointwise bounds and the meaning of "decided" are in that module's
docstring, and tests/test_ncc_l2lab_oracle.py checks them on the CPU.

Search cases: every entry of O.NCC_CASES with its own mask flag (what each
reaches in the two kernels is tabulated in tests/test_gpu_ncc.py), and
24x80 6x10, 48x112 16x8 and 80x120 20x24 again with the mask flipped.
"""

import warnings

import pytest
import torch

import _oracles as O
import _oracles_l2lab as L
from dsin_amd import ops
from dsin_amd.ops import reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _search(x, y_dec, y_orig, ph, pw, use_mask, dev):
    y_syn, rows, cols = ops.ncc_search(x.to(dev), y_dec.to(dev),
                                       y_orig.to(dev), ph, pw, use_mask,
                                       l2lab=True)
    return y_syn.cpu(), rows.cpu(), cols.cpu()


# ------------------------------------------------------------ 1. transform

def _transform_input():
    """16x24 image: the thresholds and their fp32 neighbours, negatives, the
    ends of the pixel range and beyond, in every channel combination that a
    row of specials shifted per channel gives; the rest random 0..255."""
    g = torch.Generator().manual_seed(3)
    img = torch.rand(3, 16, 24, generator=g) * 255
    t = torch.tensor(0.04045)
    inf = torch.tensor(float("inf"))
    specials = torch.stack([
        torch.tensor(0.0), t, torch.nextafter(t, inf),
        torch.nextafter(t, -inf), torch.tensor(-1e-3), torch.tensor(-7.5),
        torch.tensor(255.0), torch.tensor(300.0), torch.tensor(1e-3),
        torch.tensor(1.0)])
    n = specials.numel()
    img[:, 0, :n] = specials            # gray pixels
    for c in range(3):                  # one special channel, two random
        img[c, 1 + c, :n] = specials
    return img.contiguous()


def test_lab_transform_against_fp64(dev):
    """|t - lab64| <= 2^-8*|lab64| + 4*e32 + 1e-6 elementwise: the bf16
    store, 4 x the error e32 of the fp32 rgb_to_lab_ref against fp64 on the
    same input (max over the image), and a floor of a few fp32 ulp at 1."""
    img = _transform_input()
    want = L.lab64(img)
    e32 = float((ref.rgb_to_lab_ref(img).double() - want).abs().max())
    got = ops.ncc_lab_transform(img.to(dev))
    assert got.dtype == torch.bfloat16 and got.shape == img.shape
    again = ops.ncc_lab_transform(img.to(dev))
    assert torch.equal(got.view(torch.int16), again.view(torch.int16))
    err = (got.cpu().double() - want).abs()
    bound = O.U16 * want.abs() + 4 * e32 + 1e-6
    print(f"lab transform: e32 {e32:.3e} worst err/bound "
          f"{float((err / bound).max()):.3f}")
    assert bool(torch.isfinite(got.float()).all())
    assert bool((err <= bound).all())


# --------------------------------------------------------------- 2. search

@pytest.mark.parametrize("case", L.L2_GPU_CASES, ids=str)
def test_l2lab_search_against_oracle(dev, case):
    h, w, ph, pw, use_mask, noise = case
    x, y_dec, y_orig = L.lab_case(h, w, ph, pw, noise)
    tx = ops.ncc_lab_transform(x.to(dev)).cpu()
    ty = ops.ncc_lab_transform(y_dec.to(dev)).cpu()
    d = L.l2_decide(tx, ty, ph, pw, use_mask)
    y_syn, rows, cols = _search(x, y_dec, y_orig, ph, pw, use_mask, dev)
    O.ncc_check_gather(y_syn, rows, cols, y_orig, ph, pw)
    L.l2_check(d, rows, cols, str(case))
    _, r32, c32 = ref.ncc_search_ref(x, y_dec, y_orig, ph, pw, use_mask,
                                     l2lab=True)
    same = (rows == r32) & (cols == c32)
    print(f"l2lab {case}: equals the CPU fp32 path on {int(same.sum())}/"
          f"{same.numel()} patches")


# ----------------------------------------------------------------- 3. ties

@pytest.mark.parametrize("tie", O.NCC_TIE_CASES, ids=str)
def test_l2lab_real_ties_first_minimum_wins(dev, tie):
    """A block tiled periodically, x = y_dec = y_orig, no mask: every
    periodic copy of a patch's own location has the same operands in the
    same order, hence the same distance bit for bit (whatever its rounding
    noise around 0), in other lanes, waves and workgroups; every other
    location is farther by many orders of magnitude. The key of 0 - d and
    the atomicMax must return the first copy in flat order."""
    ty, tx, ny, nx, ph, pw = tie
    y = O.ncc_tie_case(ty, tx, ny, nx)
    yg = y.to(dev)
    y_syn, rows, cols = ops.ncc_search(yg, yg, yg, ph, pw, False, l2lab=True)
    gw = y.shape[2] // pw
    p = torch.arange(rows.numel())
    want_r = (torch.div(p, gw, rounding_mode="floor") * ph) % ty
    want_c = ((p % gw) * pw) % tx
    assert torch.equal(rows.cpu(), want_r), (rows.cpu(), want_r)
    assert torch.equal(cols.cpu(), want_c), (cols.cpu(), want_c)
    assert torch.equal(y_syn.cpu(), y)


# ---------------------------------------------------------- 4. determinism

@pytest.mark.parametrize("case", [O.NCC_CASES[1], O.NCC_CASES[8]], ids=str)
def test_l2lab_two_calls_are_equal(dev, case):
    h, w, ph, pw, use_mask, noise = case
    imgs = L.lab_case(h, w, ph, pw, noise)
    y1, r1, c1 = _search(*imgs, ph, pw, use_mask, dev)
    y2, r2, c2 = _search(*imgs, ph, pw, use_mask, dev)
    assert torch.equal(r1, r2) and torch.equal(c1, c2) and torch.equal(y1, y2)


# ------------------------------------------------------------ 5. no volume

def test_l2lab_search_allocates_no_volume(dev):
    """80x240 with 20x24 patches: one (P, Hc, Wc) fp32 volume is 2.1 MB; the
    search's own buffers (operands, window sums, y_syn) are a third of it."""
    h, w, ph, pw = 80, 240, 20, 24
    x, y_dec, y_orig = (t.to(dev) for t in O.ncc_case(h, w, 9, 8))
    ops.ncc_search(x, y_dec, y_orig, ph, pw, True, l2lab=True)  # load code
    torch.cuda.synchronize()
    volume = (h // ph) * (w // pw) * (h - ph + 1) * (w - pw + 1) * 4
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.max_memory_allocated(dev)
    out = ops.ncc_search(x, y_dec, y_orig, ph, pw, True, l2lab=True)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(dev) - before
    print(f"l2lab peak rise {rise} B, one volume {volume} B")
    assert out[0].shape == x.shape
    assert rise < volume


# --------------------------------------------------------------- 6. capture

def test_l2lab_search_is_graph_capturable(dev):
    """No host sync in the op: one search is captured into a graph and
    replayed on new inputs copied into the static buffers."""
    h, w, ph, pw = 48, 112, 16, 8
    first = [t.to(dev) for t in O.ncc_case(h, w, 21, 8)]
    new = [t.to(dev) for t in O.ncc_case(h, w, 22, 8)]
    static = [t.clone() for t in first]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            ops.ncc_search(*static, ph, pw, True, l2lab=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.ncc_search(*static, ph, pw, True, l2lab=True)
    for s, t in zip(static, new):
        s.copy_(t)
    graph.replay()
    torch.cuda.synchronize()
    want = ops.ncc_search(*new, ph, pw, True, l2lab=True)
    for a, b in zip(out, want):
        assert torch.equal(a, b)
    # and it is not the answer to the inputs it was captured with
    assert not torch.equal(want[0],
                           ops.ncc_search(*first, ph, pw, True, l2lab=True)[0])


# ----------------------------------------------------------- 7. module path

def test_sifinder_l2lab_runs_the_op_without_warning(dev, small_ae_config):
    from dsin_amd.models.sifinder import SiFinder
    cfg = small_ae_config.clone()
    cfg.use_L2andLAB = True
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        finder = SiFinder(cfg).to(dev)
        imgs = [O.ncc_case(64, 96, 40 + n, 8) for n in range(2)]
        x, y_dec, y_orig = (torch.stack([im[k] for im in imgs]).to(dev)
                            for k in range(3))
        got = finder(x, y_orig, y_dec)
    assert finder.l2lab and got.shape == (2, 3, 64, 96)
    want = torch.stack([
        ops.ncc_search(x[n], y_dec[n], y_orig[n], finder.ph, finder.pw,
                       finder.use_mask, l2lab=True)[0] for n in range(2)])
    assert torch.equal(got, want)


@pytest.mark.parametrize("match,shapes,ph,pw,use_mask", [
    ("tile", [(3, 24, 80)] * 3, 5, 10, False),
    ("tile", [(3, 24, 80)] * 3, 6, 9, False),
    ("share one shape", [(3, 24, 80), (3, 24, 70), (3, 24, 80)], 6, 10, False),
    ("share one shape", [(3, 24, 80), (3, 24, 80), (3, 18, 80)], 6, 10, False),
    ("even patch sizes", [(3, 24, 80)] * 3, 3, 10, True),
    ("even patch sizes", [(3, 24, 80)] * 3, 6, 5, True),
])
def test_l2lab_search_rejects_bad_inputs_on_gpu(dev, match, shapes, ph, pw,
                                                use_mask):
    imgs = [torch.zeros(s, device=dev) for s in shapes]
    with pytest.raises(ValueError, match=match):
        ops.ncc_search(*imgs, ph, pw, use_mask, l2lab=True)


def test_l2lab_bindings_exist():
    from dsin_amd.ops import _dsin_hip as ext
    assert hasattr(ext, "ncc_search_l2lab") and hasattr(ext, "ncc_lab_transform")
