"""The conv family (csrc/conv_kernels.h, csrc/conv.hip, ops/conv.py) against
the fp64 oracles of tests/_oracles_conv.py, on every dispatch path.

Each case runs forward and backward once on the kernel's own rounded
operands and compares y, dx, dw and db with the fp64 references under the
derived bounds of the oracle module (no tuned tolerance: U16*|ref| for the
bf16 store plus 2*depth*U32*S for the fp32 accumulation, depth read from
the launch the host really picks). It then checks that the no-grad forward
and a second forward/backward give the same bits. What each case reaches
(instantiation, staging path, phase, slice layout) is computed by
_oracles_conv.dispatch(), asserted complete on the CPU in
tests/test_conv_oracle.py and tabulated in docs/KERNELS.md.

The worst err/bound of every compared tensor goes into the assert message
and, with `pytest -s`, into a line starting with CONV_ORACLE.
"""

import pytest
import torch

import _oracles_conv as O
from dsin_amd.ops import conv as dconv

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _call(c, x, w, b):
    if c.kind == "conv":
        return dconv.conv2d(x, w, b, c.stride, c.pad, c.dil, c.act)
    if c.kind == "convT":
        return dconv.conv_transpose2d(x, w, b, c.stride, c.pad, c.op, c.act)
    return dconv.conv3d_valid(x, w, b, c.act)


def _run(c, r, dev):
    """One forward and backward on fresh leaves: (y, dx, dw, db)."""
    x = r["x"].to(dev).requires_grad_(c.xgrad)
    w = r["w"].to(dev).requires_grad_(True)
    b = r["b"].to(dev).requires_grad_(True) if c.bias else None
    y = _call(c, x, w, b)
    y.backward(r["dy"].to(dev).to(y.dtype))
    return (y.detach(), x.grad, w.grad, b.grad if c.bias else None)


def _check(c, dev, family):
    r = O.conv_reference(c)
    dconv.begin_step()
    y, dx, dw, db = _run(c, r, dev)
    assert y.dtype == torch.bfloat16 and y.shape == r["y"].shape
    assert (dx is not None) == c.xgrad
    q = {"y": O.ratio(y, r["y"], r["bound_y"]),
         "dw": O.ratio(dw, r["dw"], r["bound_dw"])}
    if c.xgrad:
        q["dx"] = O.ratio(dx, r["dx"], r["bound_dx"])
    if c.bias:
        q["db"] = O.ratio(db, r["db"], r["bound_db"])
    print("CONV_ORACLE", family, O.case_id(c),
          " ".join(f"{k}={v:.3f}" for k, v in sorted(q.items())))
    assert all(v <= 1 for v in q.values()), \
        f"worst err/bound {q} on {sorted(O.dispatch(c))}"
    # the no-grad forward takes the same kernels and gives the same bits
    with torch.no_grad():
        y0 = _call(c, r["x"].to(dev), r["w"].to(dev),
                   r["b"].to(dev) if c.bias else None)
    assert torch.equal(y0, y)
    # a second call gives the same bits, gradients included
    for first, again in zip((y, dx, dw, db), _run(c, r, dev)):
        assert (first is None and again is None) or torch.equal(first, again)


def _params(family):
    cases = O.FAMILIES[family]
    return pytest.mark.parametrize("c", cases,
                                   ids=[O.case_id(c) for c in cases])


@_params("gather")
def test_gather(c, dev):
    _check(c, dev, "gather")


@_params("direct3")
def test_direct3(c, dev):
    _check(c, dev, "direct3")


@_params("direct5")
def test_direct5(c, dev):
    _check(c, dev, "direct5")


@_params("convT")
def test_conv_transpose(c, dev):
    _check(c, dev, "convT")


@_params("wrw")
def test_weight_gradient(c, dev):
    _check(c, dev, "wrw")


@_params("conv3d")
def test_conv3d_valid(c, dev):
    _check(c, dev, "conv3d")


def test_entry_points_refuse_what_the_kernels_no_longer_stage(dev):
    """The three calls whose staging paths are gone raise before anything
    is launched: a direct 3x3 without a virtual pad, a bf16 flat gather at
    stride 2, a bf16 flat weight gradient without contiguous pixel runs."""
    from dsin_amd.ops import _require_ext
    bf = dict(dtype=torch.bfloat16, device=dev)
    x = torch.zeros(1, 64, 8, 8, **bf)
    with pytest.raises(RuntimeError, match="virtual pad of at least 1"):
        _require_ext("conv_direct")(x, torch.zeros(16, 64 * 9 + 8, **bf),
                                    None, 16, 6, 6, 0, 0, 3)
    tab = torch.zeros(9, dtype=torch.int32, device=dev)
    x1 = torch.zeros(1, 1, 8, 8, **bf)
    with pytest.raises(RuntimeError, match="stride 1 only"):
        _require_ext("conv_flat")(x1, torch.zeros(1, 64 + 8, **bf), None, tab,
                                  tab, 1, 9, 3, 3, 0, 2)
    with pytest.raises(RuntimeError, match="needs mcontig"):
        _require_ext("conv_wrw_flat")(x1, torch.zeros(1, 1, 3, 3, **bf), tab,
                                      tab, 1, 9, 3, False)
