"""CPU tests of tests/_oracles_conv.py: the conditions the GPU conv tests
(tests/test_gpu_conv_oracle.py) rely on, and the geometry check of
ops/conv.py. Nothing here needs a GPU."""

import pytest
import torch

import _oracles_conv as O
from dsin_amd import ops
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


# ------------------------------------- the mirror against what it mirrors

def _ext():
    ext = ops._try_load_ext()
    assert ext is not None, "the extension must be built for these tests"
    return ext


def _geometry(c):
    """(Cin, _Geom, direct_ok) of a 2D case's forward gather, from the case
    alone, as conv2d / conv_transpose2d build it."""
    kh, kw = c.k
    if c.kind == "convT":
        return c.Ci, dconv._Geom(1, c.stride, 1, kh, kw, kh - 1 - c.pad,
                                 kw - 1 - c.pad), False
    return c.Ci, dconv._Geom(c.stride, 1, c.dil, kh, kw, c.pad, c.pad), True


@pytest.mark.parametrize("c", O.ALL_CASES, ids=IDS)
def test_mirror_routes_as_ops_route(c):
    """The kind of the forward and of the backward-data launches in plan()
    (direct3 / direct5 / phase / gather, flat for conv3d) is what _route
    answers for the case's geometry and for its transposed geometry."""
    p = O.plan(c)
    if c.kind == "conv3d":      # no routing: always the flat tables
        assert (p["route_f"], p["route_b"]) == ("flat", "flat")
        return
    cin, g, direct_ok = _geometry(c)
    assert p["route_f"] == dconv._route(cin, g, False, direct_ok)
    assert p["route_b"] == dconv._route(c.Co, g.transposed(), True, True)
    for route, launches in ((p["route_f"], p["fwd"]), (p["route_b"], p["dx"])):
        for ln in launches:
            assert ln["kern"] == route if route.startswith("direct") \
                else ln["kern"].startswith("fwd<")
            assert bool(ln.get("phase")) == (route == "phase")


def test_route_asymmetries(monkeypatch):
    """The choices of _route that no case of the table pins down alone,
    asked directly; each decides which kernel a model layer runs."""
    G, route = dconv._Geom, dconv._route
    g3, g5 = G(1, 1, 1, 3, 3, 1, 1), G(2, 1, 1, 5, 5, 2, 2)
    assert route(64, g3, False, True) == "direct3"
    assert route(64, g3, True, True) == "direct3"       # backward-data too
    assert route(64, g3, False, False) == "gather"      # conv-transpose fwd
    assert route(65, g3, False, True) == "gather"       # Cin % 64
    assert route(64, g3._replace(pt=0, pl=0), False, True) == "gather"
    assert route(64, g3._replace(pt=2, pl=2), False, True) == "direct3"
    assert route(64, g3._replace(pt=1, pl=2), True, True) == "gather"
    assert route(64, g3._replace(dil=2), False, True) == "gather"
    assert route(64, g5, False, True) == "direct5"
    assert route(64, g5._replace(pt=0, pl=0), False, True) == "direct5"
    assert route(64, g5, True, True) == "gather"        # never rotated
    assert route(64, g5, False, False) == "gather"
    assert route(32, g5, False, True) == "gather"
    monkeypatch.setattr(dconv, "_DIRECT5", False)
    assert route(64, g5, False, True) == "gather"
    # phases: stuffed by 2 without dilation, whatever else holds
    assert route(64, G(1, 2, 1, 3, 3, 1, 1), False, False) == "phase"
    assert route(64, G(1, 2, 1, 3, 3, 1, 1), True, True) == "phase"
    assert route(8, G(1, 2, 2, 3, 3, 2, 2), True, True) == "gather"
    assert route(8, G(1, 3, 1, 3, 3, 1, 1), True, True) == "gather"
    # the transposed geometry of backward-data
    assert G(2, 1, 2, 3, 5, 1, 3).transposed() == G(1, 2, 2, 3, 5, 3, 5)


@pytest.mark.parametrize("c", O.ALL_CASES, ids=IDS)
def test_mirror_picks_the_extensions_instantiations(c):
    """Every gather, phase and flat launch of plan() names the instantiation
    and the run-time stride that conv_fwd_variant, the launch code's own
    selection, returns for the same (B, M, N, WO, st, sv, flat); every
    weight-gradient launch likewise against conv_wrw_variant."""
    ext, p = _ext(), O.plan(c)
    asked = 0
    for ln in p["fwd"] + p["dx"]:
        if ln["kern"].startswith("direct"):
            continue
        *inst, stride = ext.conv_fwd_variant(*ln["ask"])
        assert ln["kern"] == "fwd<%d,%d,%d,%d>" % tuple(inst), ln["ask"]
        assert ln["stride"] == stride, ln["ask"]
        asked += 1
    for ln in p["dw"]:
        assert ln["kern"] == "wrw<%d,%d>" % ext.conv_wrw_variant(*ln["ask"])
        asked += 1
    assert asked >= 1


def test_tile_rule_boundaries():
    """The edges of the selection, asked of the extension directly."""
    fv = _ext().conv_fwd_variant
    # (B, M, N, WO, st, sv, flat) -> (TM, VM, VST, VSV, run-time stride)
    assert fv(1, 64, 16, 8, 1, 1, False) == (64, 1, 1, 1, 1)   # M == 64
    assert fv(1, 65, 16, 13, 1, 1, False)[0] == 32             # small grid
    assert fv(1, 256 * 64, 64, 128, 1, 1, False)[0] == 64      # 256 groups
    assert fv(1, 255 * 64, 64, 128, 1, 1, False)[0] == 32      # 255 groups
    assert fv(4, 64 * 64, 64, 64, 1, 1, False)[0] == 64        # B counts
    assert fv(1, 64 * 64, 4 * 64, 64, 1, 1, False)[0] == 64    # N tiles count
    assert fv(1, 70, 16, 7, 1, 1, False) == (32, 1, 0, 1, 0)   # WO == 7
    assert fv(1, 80, 16, 8, 1, 1, False) == (32, 1, 1, 1, 1)   # WO == 8
    assert fv(1, 70, 16, 7, 2, 1, True) == (32, 0, 0, 1, 0)    # flat, WO < 8
    assert fv(1, 80, 16, 8, 2, 1, True) == (32, 0, 0, 1, 2)
    for tm, m in ((64, 64), (32, 4096)):
        assert fv(1, m, 16, 64, 1, 3, False) == (tm, 1, 0, 0, 1)   # sv == 3
        assert fv(1, m, 16, 64, 1, 2, False) == (tm, 1, 1, 2, 1)
        assert fv(1, m, 16, 64, 2, 2, False) == (tm, 1, 0, 2, 2)
        assert fv(1, m, 16, 64, 3, 1, False) == (tm, 1, 0, 1, 3)
    wv = _ext().conv_wrw_variant
    assert wv(8, 1, False) == (1, 1) and wv(7, 1, False) == (1, 0)
    assert wv(8, 2, False) == (1, 2) and wv(8, 3, False) == (1, 0)
    assert wv(8, 1, True) == (0, 0)


def test_extension_has_the_named_conv_entry_points():
    """The conv family is reached through entry points whose arguments all
    mean something; the positional catch-alls are gone."""
    ext = _ext()
    for name in ("conv_direct", "conv_gather", "conv_flat", "conv_wrw_gather",
                 "conv_wrw_flat", "conv_fwd_variant", "conv_wrw_variant",
                 "pad_stuff_e4m3"):
        assert hasattr(ext, name), name
    for name in ("conv_fwd", "conv_wrw", "pad_stuff"):
        assert not hasattr(ext, name), name


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
