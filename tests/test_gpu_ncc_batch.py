"""GPU tests of the batched side-information search: ops.ncc_search_batch
runs B images through one launch per pipeline stage (csrc/ncc_kernels.h,
the image index a grid dimension; csrc/ncc_search.hip).

What is checked, on images of at most 80x200:

  1. each image of a B = 2 batch against the fp64 score map of
     tests/_oracles.py, by the decided/undecided rule of tests/test_gpu_ncc.py
     (exact fp64 argmax where the top-2 gap exceeds bound = 4*e32 + 1e-5,
     within the bound of the maximum elsewhere), and the gather invariant;
  2. image b of a B = 3 batch bit-equal to the single call on image b, with
     no tolerance (same kernels, same per-image arithmetic, order-independent
     maximum), on geometries that reach every path of both main kernels;
  3. no leakage between the images of a batch (a shared or mis-strided best,
     ty, sy or y_orig makes one image inherit the other's matches);
  4. real ties in every image: the first periodic copy wins in each;
  5. B = 1 equals the single call; two identical calls are bit-equal;
  6. a non-contiguous batch equals its contiguous copy;
  7. SiFinder with N = 3 equals three single calls, bf16 in gives bf16 out;
  8. the ValueErrors of the Python layer on device tensors, and the host's
     check of the grid limit, raised before anything is launched.
"""

from types import SimpleNamespace

import pytest
import torch

import _oracles as O
from dsin_amd import ops
from dsin_amd.models.sifinder import SiFinder
from test_ncc_batch import bad_batch_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _stack(imgs, dev):
    """[(x, y_dec, y_orig), ...] -> three (B,3,H,W) device tensors."""
    return tuple(torch.stack([im[k] for im in imgs]).to(dev) for k in range(3))


def _cpu(out):
    return tuple(t.cpu() for t in out)


def _assert_equals_single_calls(batch, out, ph, pw, use_mask, l2lab):
    x, y_dec, y_orig = batch
    y_syn, rows, cols = out
    b_, _, h, w = x.shape
    p = (h // ph) * (w // pw)
    assert y_syn.shape == x.shape and y_syn.dtype == torch.float32
    assert rows.shape == (b_, p) and cols.shape == (b_, p)
    assert rows.dtype == torch.int64 and cols.dtype == torch.int64
    for b in range(b_):
        want = ops.ncc_search(x[b], y_dec[b], y_orig[b], ph, pw, use_mask,
                              l2lab=l2lab)
        for name, got, w_ in zip(("y_syn", "rows", "cols"),
                                 (y_syn[b], rows[b], cols[b]), want):
            assert torch.equal(got, w_), (b, name)


# ------------------------------------------------- 1. against the fp64 oracle

@pytest.mark.parametrize("geom", [O.NCC_V1_CASES[0], O.NCC_V2_CASES[0]],
                         ids=str)
def test_batch_images_agree_with_fp64_oracle(dev, geom):
    """The geometry's two existing oracle cases (noise 8 and 25) as B = 2."""
    h, w, ph, pw, use_mask = geom
    ds = [O.ncc_reference(*geom, noise) for noise in (8, 25)]
    batch = _stack([(d["x"], d["y_dec"], d["y_orig"]) for d in ds], dev)
    y_syn, rows, cols = _cpu(ops.ncc_search_batch(*batch, ph, pw, use_mask))
    for b, d in enumerate(ds):
        O.ncc_check_gather(y_syn[b], rows[b], cols[b], d["y_orig"], ph, pw)
        same = (rows[b] == d["rows"]) & (cols[b] == d["cols"])
        dec = d["decided"]
        score = d["m64"][torch.arange(rows[b].numel()), rows[b], cols[b]]
        short = d["vmax"] - score
        print(f"ncc batch {geom} image {b}: P {rows[b].numel()} decided "
              f"{int(dec.sum())} agree {int(same.sum())} bound "
              f"{d['bound']:.2e} worst shortfall {float(short.max()):.2e}")
        assert bool(same[dec].all()), (
            b, torch.nonzero(dec & ~same).flatten().tolist())
        assert bool((short[~dec] <= d["bound"]).all()), b


# --------------------------------------------- 2. bit-equal to single calls

# (H, W, ph, pw, mask): v1 P = 32 and a partial column tile; v1 two column
# tiles and P = 48 (patch-tile tail); v2 P = 84 (three patch tiles, tail of
# 20, odd k tail); v2 Hc = 33 (empty second wave group); v2 two slices, the
# batched-codec shape; v2 the default patch, four slices
EQUAL_GEOMS = [(24, 80, 6, 10, True), (36, 160, 6, 20, True),
               (21, 96, 3, 8, False), (48, 112, 16, 8, True),
               (64, 96, 16, 16, True), (80, 120, 20, 24, True)]
# ... and one of them with the mask flag flipped
EQUAL_CASES = EQUAL_GEOMS + [(64, 96, 16, 16, False)]


@pytest.mark.parametrize("l2lab", [False, True], ids=["pearson", "l2lab"])
@pytest.mark.parametrize("geom", EQUAL_CASES, ids=str)
def test_batch_is_bit_equal_to_single_calls(dev, geom, l2lab):
    h, w, ph, pw, use_mask = geom
    batch = _stack([O.ncc_case(h, w, 500 + 7 * h + b, 8) for b in range(3)],
                   dev)
    out = ops.ncc_search_batch(*batch, ph, pw, use_mask, l2lab=l2lab)
    _assert_equals_single_calls(batch, out, ph, pw, use_mask, l2lab)
    # three different answers: a batch that ran one image three times, or
    # only the first, would have passed nothing above but say so here too
    assert not torch.equal(out[0][0], out[0][1])
    assert not torch.equal(out[0][1], out[0][2])


# ------------------------------------------------------------ 3. no leakage

@pytest.mark.parametrize("l2lab", [False, True], ids=["pearson", "l2lab"])
@pytest.mark.parametrize("swap", [False, True], ids=["self-first",
                                                     "self-last"])
def test_no_leakage_between_images(dev, swap, l2lab):
    """One image is (a, a, a) and finds every patch at its own place; the
    other searches a's patches in an unrelated c and must gather only from
    c, exactly as its single call does."""
    h, w, ph, pw = 64, 96, 16, 16
    # the noisy image of each case: per-pixel noise makes the self-match of a
    # patch unique, which the smooth x alone does not promise
    a = O.ncc_case(h, w, 61, 8)[1]
    c = O.ncc_case(h, w, 62, 8)[1]
    imgs = [(a, a, a), (a, c, c)]
    own, other = (1, 0) if swap else (0, 1)
    if swap:
        imgs.reverse()
    batch = _stack(imgs, dev)
    out = ops.ncc_search_batch(*batch, ph, pw, False, l2lab=l2lab)
    _assert_equals_single_calls(batch, out, ph, pw, False, l2lab)
    y_syn, rows, cols = _cpu(out)
    gw = w // pw
    p = torch.arange(rows.shape[1])
    assert torch.equal(rows[own],
                       torch.div(p, gw, rounding_mode="floor") * ph)
    assert torch.equal(cols[own], (p % gw) * pw)
    assert torch.equal(y_syn[own], a)
    O.ncc_check_gather(y_syn[other], rows[other], cols[other], c, ph, pw)
    assert not torch.equal(y_syn[other], a)


# ------------------------------------------------------------ 4. real ties

@pytest.mark.parametrize("tie", O.NCC_TIE_CASES, ids=str)
def test_real_ties_first_maximum_wins_in_every_image(dev, tie):
    ty, tx, ny, nx, ph, pw = tie
    y = torch.stack([O.ncc_tie_case(ty, tx, ny, nx, seed=s)
                     for s in (0, 1, 2)])
    yg = y.to(dev)
    y_syn, rows, cols = _cpu(ops.ncc_search_batch(yg, yg, yg, ph, pw, False))
    gw = y.shape[3] // pw
    p = torch.arange(rows.shape[1])
    want_r = (torch.div(p, gw, rounding_mode="floor") * ph) % ty
    want_c = ((p % gw) * pw) % tx
    for b in range(3):
        assert torch.equal(rows[b], want_r), (b, rows[b], want_r)
        assert torch.equal(cols[b], want_c), (b, cols[b], want_c)
    assert torch.equal(y_syn, y)


# ------------------------------------------------ 5. B = 1 and determinism

@pytest.mark.parametrize("geom", [(36, 160, 6, 20, True),
                                  (64, 96, 16, 16, True)], ids=str)
def test_batch_of_one_and_two_equal_calls(dev, geom):
    h, w, ph, pw, use_mask = geom
    batch = _stack([O.ncc_case(h, w, 70 + b, 8) for b in range(3)], dev)
    one = ops.ncc_search_batch(*(t[:1] for t in batch), ph, pw, use_mask)
    single = ops.ncc_search(*(t[0] for t in batch), ph, pw, use_mask)
    for g, w_ in zip(one, single):
        assert g.shape[0] == 1 and torch.equal(g[0], w_)
    first = ops.ncc_search_batch(*batch, ph, pw, use_mask)
    second = ops.ncc_search_batch(*batch, ph, pw, use_mask)
    for f, s in zip(first, second):
        assert torch.equal(f, s)


# ------------------------------------------------- 6. non-contiguous input

def test_non_contiguous_batch(dev):
    h, w, ph, pw = 48, 112, 16, 8
    big = _stack([O.ncc_case(h, w, 80 + b, 8) for b in range(6)], dev)
    views = tuple(t[::2] for t in big)
    assert not views[0].is_contiguous()
    got = ops.ncc_search_batch(*views, ph, pw, True)
    want = ops.ncc_search_batch(*(v.contiguous() for v in views), ph, pw,
                                True)
    for g, w_ in zip(got, want):
        assert torch.equal(g, w_)
    _assert_equals_single_calls(views, got, ph, pw, True, False)


# ------------------------------------------------------------- 7. SiFinder

@pytest.mark.parametrize("l2lab", [False, True], ids=["pearson", "l2lab"])
def test_sifinder_runs_one_batched_search(dev, l2lab):
    ph, pw = 16, 16
    cfg = SimpleNamespace(y_patch_size=(ph, pw), use_gauss_mask=True,
                          use_L2andLAB=l2lab)
    finder = SiFinder(cfg).to(dev)
    x, y_dec, y_orig = _stack([O.ncc_case(64, 96, 90 + n, 8)
                               for n in range(3)], dev)
    got = finder(x, y_orig, y_dec)
    assert got.dtype == torch.float32 and got.shape == (3, 3, 64, 96)
    want = torch.stack([
        ops.ncc_search(x[n], y_dec[n], y_orig[n], ph, pw, True,
                       l2lab=l2lab)[0] for n in range(3)])
    assert torch.equal(got, want)
    xb, yb, ob = (t.to(torch.bfloat16) for t in (x, y_dec, y_orig))
    got16 = finder(xb, ob, yb)
    assert got16.dtype == torch.bfloat16
    want16 = torch.stack([
        ops.ncc_search(xb[n], yb[n], ob[n], ph, pw, True,
                       l2lab=l2lab)[0] for n in range(3)]).to(torch.bfloat16)
    assert torch.equal(got16, want16)


# ----------------------------------------------------------- 8. validation

@pytest.mark.parametrize("match,shapes,ph,pw,use_mask", bad_batch_inputs())
def test_batch_rejects_bad_inputs_on_gpu(dev, match, shapes, ph, pw,
                                         use_mask):
    imgs = [torch.zeros(s, device=dev) for s in shapes]
    with pytest.raises(ValueError, match=match):
        ops.ncc_search_batch(*imgs, ph, pw, use_mask)


def test_batch_beyond_the_grid_limit_is_refused(dev):
    """The image shares grid z with the patch tiles: at most 65535 blocks.
    An 8x16 image with 8x8 patches has one patch tile, so 65536 images are
    one too many; the error names the largest batch that fits."""
    t = torch.zeros(65536, 3, 8, 16, device=dev)
    with pytest.raises(RuntimeError, match="largest batch.* is 65535"):
        ops.ncc_search_batch(t, t, t, 8, 8, False)
