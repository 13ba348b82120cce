"""CPU tests of tests/_oracles_conv.py: the conditions the GPU conv tests
(tests/test_gpu_conv_oracle.py) rely on, and the geometry check of
ops/conv.py. Nothing here needs a GPU."""

import pytest
import torch

import _oracles_conv as O
from dsin_amd.ops import conv as dconv

IDS = [O.case_id(c) for c in O.ALL_CASES]


def test_case_ids_unique():
    assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("c", O.ALL_CASES, ids=IDS)
def test_cpu_fp32_within_bounds(c):
    """The CPU fp32 conv on the same operands, stored to bf16, passes
    bound_y, and its fp32 dw passes bound_dw: the bounds leave room for an
    honest fp32 accumulation."""
    r = O.conv_reference(c)
    y32, dw32 = O.cpu_fp32(c)
    qy = O.ratio(y32, r["y"], r["bound_y"])
    qw = O.ratio(dw32, r["dw"], r["bound_dw"])
    assert qy <= 1 and qw <= 1, (qy, qw)


@pytest.mark.parametrize("c", O.ALL_CASES, ids=IDS)
def test_one_dropped_tap_is_seen(c):
    """One tap zeroed over one 64-channel chunk violates bound_y on at
    least 90 % of the outputs it reaches."""
    r = O.conv_reference(c)
    yd = O.defect_forward(c)
    err = (yd - r["y"]).abs()
    reached = err > 0
    assert int(reached.sum()) > 0
    seen = (err > r["bound_y"])[reached].double().mean()
    assert float(seen) >= 0.9, float(seen)


@pytest.mark.parametrize("c", [c for c in O.ALL_CASES if c.act],
                         ids=[O.case_id(c) for c in O.ALL_CASES if c.act])
def test_masked_share(c):
    r = O.conv_reference(c)
    assert r["masked"] < 0.05, r["masked"]
    # the gradient the kernels see is a bf16 value
    assert torch.equal(r["g"], r["g"].bfloat16().float())


def test_wrw_chunks_named_cases():
    big, one, b3 = O.WRW_CASES
    pc, pchunk, p0s = O.wrw_chunks(1, 46 * 56, 8 * 9, 16)
    assert (pc, pchunk) == (10, 288) and p0s[-1] >= 46 * 56
    assert {"wrw:chunks>1", "wrw:p0>=M"} <= O.dispatch(big)
    assert O.wrw_chunks(1, 15 * 17, 72, 16)[0] == 1
    assert {"wrw:view", "wrw:tail%8"} <= O.dispatch(one)
    assert "wrw:view" not in O.dispatch(b3)
    # every slice but the empty one holds a whole number of 32-pixel steps
    # or ends at M
    for c in O.ALL_CASES:
        for ln in O.plan(c)["dw"]:
            assert ln["PCHUNK"] % 32 == 0
            assert ln["PCHUNK"] * ln["pix_chunks"] >= ln["M"]


def test_dispatch_covers_every_reachable_path():
    reached = set()
    for c in O.ALL_CASES:
        reached |= O.dispatch(c)
    assert not (O.REQUIRED - reached), sorted(O.REQUIRED - reached)


def test_dispatch_of_the_named_cases():
    """The cases the issue names reach what it says they reach."""
    g = O.GATHER_CASES
    for i, n in enumerate(range(1, 6)):
        assert f"fwd<64,1,1,1>:nchunks={n}" in O.dispatch(g[i])
        assert f"fwd<32,1,1,1>:nchunks={n}" in O.dispatch(g[5 + i])
    assert "fwd:fwd<64,1,1,1>" in O.dispatch(g[10])   # M = 64
    assert "fwd:fwd<32,1,1,1>" in O.dispatch(g[11])
    assert "fwd:fwd<64,1,0,1>" in O.dispatch(g[12])
    assert "fwd:fwd<32,1,0,1>" in O.dispatch(g[13])
    assert "fwd:fwd<64,1,2,1>" in O.dispatch(g[14])
    assert "phase:empty" in O.dispatch(g[17])
    assert {"fwd:fwd<64,1,0,1>", "dx:fwd<32,1,0,0>"} <= O.dispatch(g[18])
    assert "dx:fwd<64,1,0,0>" in O.dispatch(g[19])
    d3 = O.DIRECT3_CASES
    assert {"fwd:direct3", "dx:direct3"} <= O.dispatch(d3[0])
    assert "dx:direct3" not in O.dispatch(d3[1])
    assert {"dx:direct3", "direct3:dx:vp=2"} <= O.dispatch(d3[6])
    assert "fwd:direct3" not in O.dispatch(d3[6])
    for c in O.DIRECT5_CASES:
        assert {"fwd:direct5"} <= O.dispatch(c)
        assert not c.xgrad or "phase" in O.dispatch(c)
    assert "phase:TM64" in O.dispatch(O.CONVT_CASES[3])
    assert "fwd:fwd<64,0,0,1>" in O.dispatch(O.CONV3D_CASES[0])
    assert "fwd:fwd<32,0,0,1>" in O.dispatch(O.CONV3D_CASES[2])


def test_phase_list_matches_ops():
    """The mirror of the phase decomposition agrees with ops/conv.py."""
    dev = torch.device("cpu")
    for args in [(6, 6, 3, 3, 8, 1, 1), (10, 18, 5, 5, 4, 2, 2),
                 (9, 11, 1, 1, 16, 0, 0), (10, 18, 4, 4, 8, 2, 2),
                 (11, 13, 3, 5, 16, 1, 3)]:
        mine = O.phase_list(*args)
        theirs = dconv._phase_plans(dev, *args)
        assert len(mine) == len(theirs)
        for m, t in zip(mine, theirs):
            assert (m["a"], m["b"], m["nh"], m["nw"], m["Kp"]) == \
                (t["a"], t["b"], t["nh"], t["nw"], t["Kp"])
            assert torch.equal(m["ktab"], t["ktab64"])


# ------------------------------------------------- geometry check (CPU only)

def _conv(ci, co, h, w, k, **kw):
    return dconv.conv2d(torch.zeros(1, ci, h, w), torch.zeros(co, ci, k, k),
                        None, **kw)


def test_geometry_refused():
    with pytest.raises(ValueError, match="reach"):
        _conv(1, 1, 4, 4, 3, padding=512, dilation=512)
    with pytest.raises(ValueError, match="channels"):
        _conv(2048, 1, 1, 1, 1)
    with pytest.raises(ValueError, match="channels"):
        _conv(1, 2048, 1, 1, 1)
    with pytest.raises(ValueError, match="row"):
        _conv(1, 1, 65537, 1, 1, stride=2)      # 32769 output rows
    with pytest.raises(ValueError, match="column"):
        _conv(1, 1, 1, 65537, 1)
    xt, wt = torch.zeros(1, 2048, 1, 1), torch.zeros(2048, 1, 3, 3)
    with pytest.raises(ValueError, match="channels"):
        dconv.conv_transpose2d(xt, wt, None, 2, 1, 1)
    with pytest.raises(ValueError, match="channels"):
        dconv.conv_transpose2d(torch.zeros(1, 1, 1, 1),
                               torch.zeros(1, 2048, 3, 3), None, 2, 1, 1)
    with pytest.raises(ValueError, match="row"):
        dconv.conv_transpose2d(torch.zeros(1, 1, 16385, 1),
                               torch.zeros(1, 1, 3, 3), None, 2, 1, 1)


def test_geometry_accepted():
    # the limits themselves
    assert _conv(1, 1, 4, 4, 3, padding=511, dilation=511).shape[-1] == 4
    assert _conv(2047, 1, 1, 1, 1).shape == (1, 1, 1, 1)
    assert _conv(1, 2047, 1, 1, 1).shape == (1, 2047, 1, 1)
    assert _conv(1, 1, 32768, 1, 1).shape[2] == 32768
    assert _conv(1, 1, 32767, 1, 1, stride=2).shape[2] == 16384
    # the model's own geometries (320x960 and 1024x2048 crops): encoder
    # 5x5/s2, resblock 3x3, siNet dilations up to 128, decoder 5x5 convT
    for h, w in ((320, 960), (1024, 2048)):
        for ci, co, k, st, d in [(3, 64, 5, 2, 1), (64, 128, 5, 2, 1),
                                 (128, 128, 3, 1, 1), (6, 32, 3, 1, 1),
                                 (32, 32, 3, 1, 128), (32, 3, 1, 1, 1)]:
            ho = (h + 2 * (k // 2) * d - (k - 1) * d - 1) // st + 1
            wo = (w + 2 * (k // 2) * d - (k - 1) * d - 1) // st + 1
            dconv.check_conv_geometry("conv2d", ci, co, h, w, ho, wo, k, k,
                                      st, 1, d)
        dconv.check_conv_geometry("conv_transpose2d", 128, 64, h // 8, w // 8,
                                  h // 4, w // 4, 5, 5, 1, 2, 1)
    y = dconv.conv2d(torch.randn(1, 2, 20, 20), torch.randn(3, 2, 3, 3),
                     None, 1, 128, 128)
    assert y.shape == (1, 3, 20, 20)
