"""conv3x3_direct_kernel on its fragment-major W panel (wmat_make modes 6
and 7): the panel against the row-major mode-2/3 panel element by element,
and the kernel at the smallest shapes where the panel's 16-row groups can
go wrong, through ops.conv2d against the fp64 oracle and bounds of
tests/_oracles_conv.py (y, dx, dw, db), plus equal bits from the no-grad
forward and from a second forward/backward.

  Co 16, 33, 48, 65, 96, 128: a wave's row group full, partial (zero rows
     fill it), wholly past Co (it reads group 0), or in the second workgroup
  Ci 64, 128, 192: one, two and three chunks (18, 36, 54 k-steps a group)
  input 8x8, 4x5, 9x17, 17x26: one full tile, a tile with four rows
     outside, partial tiles both ways; at pad 2 the output is two larger
  pad 1 and 2 (border, guarded-vector and interior staging), B = 2, bias
  with ReLU and leaky ReLU; Co = 128 sends dx through the kernel too (the
  rotated panel, mode 7).
"""

import pytest
import torch

import _oracles_conv as O
from _oracles_conv import C
from dsin_amd.ops import conv as dconv

pytestmark = pytest.mark.gpu

CASES = [
    C(2, 64, 16, 8, 8, 3, 1, 1),
    C(2, 128, 33, 4, 5, 3, 1, 1, bias=True, act=1),
    C(2, 192, 48, 9, 17, 3, 1, 2, bias=True, act=2),     # output 11x19
    C(2, 64, 65, 17, 26, 3, 1, 1),
    C(2, 128, 96, 9, 17, 3, 1, 1, bias=True, act=2),
    C(2, 192, 33, 17, 26, 3, 1, 2),                      # output 19x28
    C(2, 128, 128, 4, 5, 3, 1, 1),                       # dx direct
    C(2, 64, 96, 8, 8, 3, 1, 2, bias=True, act=1),       # output 10x10
    C(2, 64, 48, 4, 5, 3, 1, 2),                         # output 6x7
    C(2, 192, 65, 8, 8, 3, 1, 1, bias=True, act=1),
    C(2, 64, 128, 17, 26, 3, 1, 1, bias=True, act=2),    # dx direct, 2 chunks
]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _run(c, r, dev):
    x = r["x"].to(dev).requires_grad_(True)
    w = r["w"].to(dev).requires_grad_(True)
    b = r["b"].to(dev).requires_grad_(True) if c.bias else None
    y = dconv.conv2d(x, w, b, c.stride, c.pad, c.dil, c.act)
    y.backward(r["dy"].to(dev).to(y.dtype))
    return (y.detach(), x.grad, w.grad, b.grad if c.bias else None)


@pytest.mark.parametrize("co,cin,rot", [(33, 64, False), (96, 128, False),
                                        (16, 192, False), (128, 65, True)])
def test_fragment_major_panel_is_a_permutation_of_the_row_major(co, cin, rot,
                                                               dev):
    """Mode 6/7 element (group g, k-step s, lane, e) is mode 2/3 element
    (row 16g + lane % 16, k' = 32s + 8(lane / 16) + e); rows past the last
    are zero. rot: the backward-data panel, whose rows are the input
    channels (65 of them here) and whose k runs over the 128 couts."""
    from dsin_amd import ops
    make = ops._require_ext("wmat_make")
    rows = cin if rot else co
    w1 = torch.randn(co, cin * 9, generator=torch.Generator().manual_seed(3))
    w1 = w1.to(dev)
    flat = make(w1, 9, 3 if rot else 2)            # (rows, KP + 8)
    frag = make(w1, 9, 7 if rot else 6)            # (rows16, KP + 8)
    kp = flat.shape[1] - 8
    r16 = (rows + 15) // 16 * 16
    assert flat.shape[0] == rows and frag.shape == (r16, kp + 8)
    want = torch.zeros(r16, kp, dtype=flat.dtype, device=dev)
    want[:rows] = flat[:, :kp]
    # [g][row][s][kgrp][e] -> [g][s][kgrp][row][e]
    want = want.view(r16 // 16, 16, kp // 32, 4, 8).permute(0, 2, 3, 1, 4)
    got = frag.view(r16 // 16, 16 * (kp + 8))[:, :16 * kp]
    assert torch.equal(got, want.reshape(r16 // 16, 16 * kp))


@pytest.mark.parametrize("c", CASES, ids=[O.case_id(c) for c in CASES])
def test_direct3_on_the_fragment_major_panel(c, dev):
    p = O.plan(c)
    assert p["route_f"] == "direct3"
    assert (p["route_b"] == "direct3") == (c.Co % 64 == 0)
    r = O.conv_reference(c)
    dconv.begin_step()
    y, dx, dw, db = _run(c, r, dev)
    assert y.dtype == torch.bfloat16 and y.shape == r["y"].shape
    q = {"y": O.ratio(y, r["y"], r["bound_y"]),
         "dx": O.ratio(dx, r["dx"], r["bound_dx"]),
         "dw": O.ratio(dw, r["dw"], r["bound_dw"])}
    if c.bias:
        q["db"] = O.ratio(db, r["db"], r["bound_db"])
    print("DIRECT3_PANEL", O.case_id(c),
          " ".join(f"{k}={v:.3f}" for k, v in sorted(q.items())))
    assert all(v <= 1 for v in q.values()), f"worst err/bound {q}"
    with torch.no_grad():
        y0 = dconv.conv2d(r["x"].to(dev), r["w"].to(dev),
                          r["b"].to(dev) if c.bias else None, c.stride, c.pad,
                          c.dil, c.act)
    assert torch.equal(y0, y)
    for first, again in zip((y, dx, dw, db), _run(c, r, dev)):
        assert (first is None and again is None) or torch.equal(first, again)
