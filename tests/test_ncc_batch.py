"""CPU tests of the batched side-information search, ops.ncc_search_batch,
and of SiFinder calling it once for the whole batch. The GPU side is in
tests/test_gpu_ncc_batch.py."""

from types import SimpleNamespace

import pytest
import torch

import _oracles as O
from dsin_amd import ops
from dsin_amd.models.sifinder import SiFinder

H, W, PH, PW = 48, 64, 16, 16


def _batch(n, h=H, w=W, seed0=300):
    imgs = [O.ncc_case(h, w, seed0 + b, 8) for b in range(n)]
    return tuple(torch.stack([im[k] for im in imgs]) for k in range(3))


@pytest.mark.parametrize("l2lab", [False, True])
@pytest.mark.parametrize("use_mask", [True, False])
def test_batch_equals_stacked_single_calls_on_cpu(l2lab, use_mask):
    x, y_dec, y_orig = _batch(3)
    y_syn, rows, cols = ops.ncc_search_batch(x, y_dec, y_orig, PH, PW,
                                             use_mask, l2lab=l2lab)
    p = (H // PH) * (W // PW)
    assert y_syn.shape == (3, 3, H, W)
    assert rows.shape == (3, p) and cols.shape == (3, p)
    assert rows.dtype == torch.int64 and cols.dtype == torch.int64
    for b in range(3):
        want = ops.ncc_search(x[b], y_dec[b], y_orig[b], PH, PW, use_mask,
                              l2lab=l2lab)
        for got, w_ in zip((y_syn[b], rows[b], cols[b]), want):
            assert torch.equal(got, w_), b
    # the images differ, so a batch that repeated one image would show
    assert not torch.equal(y_syn[0], y_syn[1])


def test_batch_of_one_on_cpu():
    x, y_dec, y_orig = _batch(1)
    got = ops.ncc_search_batch(x, y_dec, y_orig, PH, PW)
    want = ops.ncc_search(x[0], y_dec[0], y_orig[0], PH, PW)
    for g, w_ in zip(got, want):
        assert g.shape[0] == 1 and torch.equal(g[0], w_)


def bad_batch_inputs():
    """(match, shapes of the three tensors, ph, pw, use_mask): every input
    ops.ncc_search_batch refuses. Shared with the GPU tests."""
    ok = (2, 3, 24, 80)
    return [
        ("B, 3, H, W", [(3, 24, 80)] * 3, 6, 10, False),        # rank 3
        ("B, 3, H, W", [(1, 2, 3, 24, 80)] * 3, 6, 10, False),  # rank 5
        ("B, 3, H, W", [(2, 1, 24, 80)] * 3, 6, 10, False),     # not RGB
        ("B >= 1", [(0, 3, 24, 80)] * 3, 6, 10, False),         # B = 0
        ("share one shape", [ok, (3, 3, 24, 80), ok], 6, 10, False),
        ("share one shape", [ok, ok, (1, 3, 24, 80)], 6, 10, False),
        ("share one shape", [ok, (2, 3, 18, 80), ok], 6, 10, False),
        ("share one shape", [ok, ok, (2, 3, 24, 70)], 6, 10, False),
        ("share one shape", [ok, (2, 3, 24), ok], 6, 10, False),
        ("tile", [ok] * 3, 5, 10, False),
        ("tile", [ok] * 3, 6, 9, False),
        ("tile", [ok] * 3, 0, 10, False),
        ("even patch sizes", [ok] * 3, 3, 10, True),
        ("even patch sizes", [ok] * 3, 6, 5, True),
    ]


@pytest.mark.parametrize("match,shapes,ph,pw,use_mask", bad_batch_inputs())
@pytest.mark.parametrize("l2lab", [False, True])
def test_batch_rejects_bad_inputs_on_cpu(match, shapes, ph, pw, use_mask,
                                         l2lab):
    imgs = [torch.zeros(s) for s in shapes]
    with pytest.raises(ValueError, match=match):
        ops.ncc_search_batch(*imgs, ph, pw, use_mask, l2lab=l2lab)


def test_batch_accepts_odd_patches_without_mask_on_cpu():
    x, y_dec, y_orig = _batch(2, 21, 40)
    y_syn, rows, cols = ops.ncc_search_batch(x, y_dec, y_orig, 7, 5, False)
    for b in range(2):
        O.ncc_check_gather(y_syn[b], rows[b], cols[b], y_orig[b], 7, 5)


@pytest.mark.parametrize("l2lab", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sifinder_equals_the_per_image_loop_on_cpu(l2lab, dtype):
    cfg = SimpleNamespace(y_patch_size=(PH, PW), use_gauss_mask=True,
                          use_L2andLAB=l2lab)
    finder = SiFinder(cfg)
    x, y_dec, y_orig = (t.to(dtype) for t in _batch(3))
    got = finder(x, y_orig, y_dec)
    assert got.dtype == dtype and got.shape == x.shape
    want = torch.stack([
        ops.ncc_search(x[n], y_dec[n], y_orig[n], PH, PW, True,
                       l2lab=l2lab)[0] for n in range(3)]).to(dtype)
    assert torch.equal(got, want)
