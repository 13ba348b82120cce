"""fp64 oracles, derived bounds and a dispatch mirror for the conv family.

Plain helper module (not a conftest), CPU only, in the style of
tests/_oracles.py. tests/test_conv_oracle.py checks on the CPU the conditions
the GPU tests (tests/test_gpu_conv_oracle.py) rely on.

Operands. x and the upstream gradient dy are bf16 values held in fp32; the
weight is fp32 and is rounded to bf16 here exactly as wmat_make /
panel_gather round it (round to nearest even). The gradient the kernels see
is g = bf16(fp32(dy) * act'(y)), act_bwd_kernel's own expression; dy is
zeroed wherever |pre64| <= 2*bound_y so that rounding never decides the
activation branch.

Bounds (U16 = 2^-8, U32 = 2^-24, S = the same expression on absolute
values):
  y, dx (bf16 stores)  U16*|ref| + 2*depth*U32*S + 1e-12,
                       depth = 32 + KP/32 + 2
  dw (fp32)            2*depth_w*U32*S_dw,
                       depth_w = 32 + PCHUNK/32 + (B*pix_chunks - 1)
  db                   (B*M)*U32*S_db
32 is one MFMA's products in any order, KP/32 the accumulate chain over the
K steps, 2 the bias add and the leaky multiply; the factor 2 allows the
matrix unit's internal additions to truncate. KP is what the launch really
uses: the 64-padded K of a gather launch, a phase's own Kp padded to 64,
Ci*khw for the direct kernels. plan() mirrors the host-side selection of
ops/conv.py (_route, _gather) and csrc/conv.hip (conv_fwd_variant,
conv_wrw_variant) to find it; the mirror stays independent Python, and
tests/test_conv_oracle.py compares it with the code it mirrors for every
launch of every case.
"""

import functools
import math
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as F

from _oracles import U16, U32

SLOPE = float(torch.tensor(0.2, dtype=torch.float32))  # the kernels' 0.2f

Case = namedtuple("Case", "kind B Ci Co size k stride pad dil bias act op "
                          "xgrad")


def C(B, Ci, Co, H, W, k, stride=1, pad=0, dil=1, bias=False, act=0,
      xgrad=True):
    """conv2d case in the issue's notation (B, Ci, Co, H, W, k, s, p, d)."""
    k = (k, k) if isinstance(k, int) else tuple(k)
    return Case("conv", B, Ci, Co, (H, W), k, stride, pad, dil, bias, act, 0,
                xgrad)


def T(B, Ci, Co, H, W, k, stride, pad, op, bias=False, act=0, xgrad=True):
    """conv_transpose2d case."""
    return Case("convT", B, Ci, Co, (H, W), (k, k), stride, pad, 1, bias, act,
                op, xgrad)


def V(B, Ci, Co, D, H, W, act=0, xgrad=True):
    """conv3d_valid case, kernel (2, 3, 3), always with bias."""
    return Case("conv3d", B, Ci, Co, (D, H, W), (2, 3, 3), 1, 0, 1, True, act,
                0, xgrad)


def case_id(c):
    s = "x".join(str(v) for v in c.size)
    k = "x".join(str(v) for v in c.k)
    t = f"{c.kind}-b{c.B}-ci{c.Ci}-co{c.Co}-{s}-k{k}-s{c.stride}-p{c.pad}"
    if c.dil != 1:
        t += f"-d{c.dil}"
    if c.op:
        t += f"-op{c.op}"
    if c.bias and c.kind != "conv3d":
        t += "-bias"
    if c.act:
        t += f"-act{c.act}"
    if not c.xgrad:
        t += "-nodx"
    return t


# --------------------------------------------------------------- case tables
# What each case reaches is computed by dispatch() and tabulated in
# docs/KERNELS.md.

GATHER_CASES = (
    # TM=64, VST=1: KP/64 = 1..5, K % 64 != 0, one live column in N tile 2
    [C(2, ci, 65, 64, 64, 3, 1, 1) for ci in (5, 8, 15, 24, 33)]
    # TM=32: M = 117, runs crossing rows at every offset
    + [C(1, ci, 16, 9, 13, 3, 1, 1) for ci in (5, 8, 15, 24, 33)]
    + [C(2, 16, 16, 8, 8, 3, 1, 1),        # M = 64, WO = 8
       C(2, 16, 16, 9, 9, 3, 1, 1),        # WO = 9
       C(1, 8, 16, 7, 7, 3, 1, 1),         # generic staging, TM=64
       C(1, 8, 16, 20, 6, 3, 1, 1),        # generic staging, TM=32
       C(2, 3, 65, 128, 128, 5, 2, 2),     # stride 2, TM=64
       C(1, 3, 64, 33, 47, 5, 2, 2),
       C(1, 16, 16, 18, 18, 3, 2, 1),      # the wv0 + 16 <= W edge
       C(1, 8, 16, 9, 11, 1, 2, 0),        # backward phases without taps
       C(1, 8, 16, 20, 26, 3, 3, 1),       # stride 3
       C(1, 8, 16, 8, 8, 3, 3, 1),         # stride 3, dx at TM=64
       C(1, 6, 32, 24, 40, 3, 1, 2, 2, bias=True, act=2),
       C(2, 6, 32, 24, 40, 3, 1, 4, 4, bias=True, act=2),
       C(1, 6, 32, 24, 40, 3, 1, 16, 16, bias=True, act=2),
       C(2, 32, 3, 24, 40, 1, 1, 0, bias=True),
       C(1, 16, 16, 12, 14, 3, 1, 0),      # pad 0
       C(1, 8, 16, 10, 14, (3, 5), 1, 2),  # ptb = 0, plb = 2
       C(1, 8, 16, 10, 14, (5, 3), 1, 1),  # ptb = 3, plb = 1
       C(1, 8, 16, 11, 13, (3, 5), 2, 1),  # non-square phases
       # stride 2 with dilation: dx is the stuffed (VSV=2) gather
       C(2, 65, 8, 64, 64, 3, 2, 2, 2),
       C(1, 8, 16, 21, 19, 3, 2, 2, 2),
       C(1, 8, 16, 12, 7, 3, 2, 2, 2),
       C(1, 8, 16, 8, 7, 3, 2, 2, 2),
       # activations on one TM=64 and one TM=32 case
       C(2, 8, 65, 64, 64, 3, 1, 1, bias=True, act=1),
       C(2, 8, 65, 64, 64, 3, 1, 1, bias=True, act=2),
       C(1, 8, 16, 9, 13, 3, 1, 1, bias=True, act=1),
       C(1, 8, 16, 9, 13, 3, 1, 1, bias=True, act=2),
       C(1, 15, 16, 9, 13, 3, 1, 1, xgrad=False)])

DIRECT3_CASES = [
    C(2, 64, 64, 8, 8, 3, 1, 1),                       # both ways direct
    C(2, 64, 48, 19, 29, 3, 1, 1, bias=True, act=2),   # dx by the gather
    C(2, 128, 65, 17, 26, 3, 1, 1),
    C(2, 192, 80, 19, 29, 3, 1, 2),                    # vp = 2, restage
    C(2, 256, 64, 17, 26, 3, 1, 1, bias=True, act=1),
    C(2, 64, 128, 17, 26, 3, 1, 1),                    # dx with two chunks
    C(2, 16, 64, 19, 29, 3, 1, 0),                     # dx direct, vp = 2
    C(2, 128, 48, 8, 8, 3, 1, 2),
    C(2, 64, 64, 17, 26, 3, 1, 1, xgrad=False)]

DIRECT5_CASES = [
    C(2, 64, 33, 8, 8, 5, 2, 2),
    C(1, 128, 64, 37, 45, 5, 2, 2, bias=True, act=2),
    C(1, 192, 65, 40, 48, 5, 2, 0),
    C(2, 64, 65, 37, 45, 5, 2, 0),
    C(1, 128, 33, 40, 48, 5, 2, 2),
    C(1, 64, 64, 8, 8, 5, 2, 0, xgrad=False)]

CONVT_CASES = [
    T(1, 8, 16, 3, 3, 3, 2, 1, 1),                     # nw < 8
    T(1, 64, 3, 4, 8, 3, 2, 1, 0),
    T(1, 128, 16, 5, 9, 5, 2, 2, 1, bias=True, act=1),
    T(2, 8, 65, 64, 64, 5, 2, 2, 1),                   # phases at TM=64
    T(1, 8, 16, 5, 9, 4, 2, 1, 0, bias=True, act=2),
    T(1, 64, 65, 4, 8, 3, 2, 1, 1, bias=True),
    T(1, 8, 64, 4, 8, 3, 1, 1, 0),                     # sv = 1, dx direct
    T(2, 128, 3, 5, 9, 3, 1, 1, 0, bias=True),
    T(1, 8, 16, 5, 9, 3, 2, 1, 1, xgrad=False)]

WRW_CASES = [
    C(1, 8, 16, 46, 56, 3, 1, 1),   # pix_chunks 10, PCHUNK 288, p0 >= M
    C(1, 8, 16, 15, 17, 3, 1, 1),   # pix_chunks 1: the view return, M%8 != 0
    C(3, 8, 16, 15, 17, 3, 1, 1)]

CONV3D_CASES = [
    V(1, 1, 24, 18, 34, 34), V(1, 1, 24, 18, 34, 34, act=1),
    V(1, 24, 24, 6, 9, 16), V(1, 24, 24, 6, 9, 16, act=1),
    V(2, 3, 6, 4, 6, 8), V(2, 3, 6, 4, 6, 8, act=1),
    V(1, 24, 6, 5, 7, 15), V(1, 24, 6, 5, 7, 15, act=1, xgrad=False)]

FAMILIES = {"gather": GATHER_CASES, "direct3": DIRECT3_CASES,
            "direct5": DIRECT5_CASES, "convT": CONVT_CASES,
            "wrw": WRW_CASES, "conv3d": CONV3D_CASES}
ALL_CASES = [c for f in FAMILIES.values() for c in f]


# ------------------------------------------------------------ host mirrors

def _cdiv(a, b):
    return -(-a // b)


def _kp64(k):
    return (k + 63) & ~63


def out_size(c):
    if c.kind == "conv3d":
        return tuple(n - k + 1 for n, k in zip(c.size, c.k))
    if c.kind == "convT":
        return tuple((n - 1) * c.stride - 2 * c.pad + k + c.op
                     for n, k in zip(c.size, c.k))
    return tuple((n + 2 * c.pad - (k - 1) * c.dil - 1) // c.stride + 1
                 for n, k in zip(c.size, c.k))


def wrw_chunks(B, M, K, Co):
    """(pix_chunks, PCHUNK, [p0 of every slice]) of one weight-gradient
    launch: the host formula of csrc/conv.hip (wrw_launch) and the kernel's
    own slice start."""
    tiles = _cdiv(K, 64) * _cdiv(Co, 64) * B
    pix_chunks = min(max(1536 // max(tiles, 1), 1), max(M // 256, 1))
    pchunk = (_cdiv(M, pix_chunks) + 31) & ~31
    return pix_chunks, pchunk, [pc * pchunk for pc in range(pix_chunks)]


def phase_list(HO, WO, kh, kw, Cin, pt, pl):
    """The live phases of a (st=1, sv=2, dil=1) gather, as ops/conv.py
    decomposes it: dicts with a, b, nh, nw, Kp and the tap columns ktab."""
    out = []
    for a in (0, 1):
        for b in (0, 1):
            rs = list(range((pt + a) & 1, kh, 2))
            ss = list(range((pl + b) & 1, kw, 2))
            nh, nw = len(range(a, HO, 2)), len(range(b, WO, 2))
            if not rs or not ss or nh == 0 or nw == 0:
                continue
            ktab = [ci * kh * kw + r * kw + s
                    for ci in range(Cin) for r in rs for s in ss]
            out.append(dict(a=a, b=b, nh=nh, nw=nw, Kp=len(ktab),
                            ktab=torch.tensor(ktab)))
    return out


def _fwd_launch(B, M, N, K, WO, stride, vm, vsv, sel=None):
    """The instantiation and run-time stride of one gather launch: a mirror
    of conv_fwd_variant in csrc/conv.hip, whose arguments are kept in
    "ask"."""
    st = 0 if WO < 8 else stride
    tm = 32 if (_cdiv(M, 64) * _cdiv(N, 64) * B < 256 and M > 64) else 64
    if not vm:
        inst = (tm, 0, 0, 1)
    elif vsv > 2:
        inst = (tm, 1, 0, 0)
    elif vsv == 2:
        inst = (tm, 1, 1 if st == 1 else 0, 2)
    else:
        inst = (tm, 1, st if st in (1, 2) else 0, 1)
    return dict(kern="fwd<%d,%d,%d,%d>" % inst, KP=_kp64(K), WO=WO, M=M,
                sel=sel, tm=tm, vst=inst[2], stride=st,
                ask=(B, M, N, WO, stride, vsv, not vm))


def _wrw_launch(B, M, K, N, WO, st, vm, cols=None):
    """Mirror of conv_wrw_variant (arguments in "ask") and the chunking."""
    if not vm:
        kern = "wrw<0,0>"
    elif WO < 8 or st not in (1, 2):
        kern = "wrw<1,0>"
    else:
        kern = "wrw<1,%d>" % st
    pix_chunks, pchunk, p0s = wrw_chunks(B, M, K, N)
    return dict(kern=kern, B=B, M=M, K=K, pix_chunks=pix_chunks,
                PCHUNK=pchunk, p0s=p0s, cols=cols, ask=(WO, st, not vm))


def _direct3_staging(Hp, Wp, HO, WO, vp, Ci):
    """Which staging paths of conv3x3_direct_kernel a launch takes."""
    paths = set()
    nelem = Ci * Hp * Wp
    for oy0 in range(0, HO, 8):
        for ox0 in range(0, WO, 8):
            if (vp > 0 and oy0 >= vp and oy0 + 10 - vp <= Hp and ox0 >= vp
                    and ox0 + 16 - vp <= Wp):
                paths.add("tile_int")
                continue
            cbase = ox0 - vp
            for y in range(10):
                gy = oy0 + y - vp
                rowin = 0 <= gy < Hp
                off = (rowin and gy or 0) * Wp + cbase  # channel 0
                if rowin and cbase >= 0 and cbase + 10 <= Wp \
                        and off + 40 <= nelem:
                    paths.add("guarded_vec")
                else:
                    paths.add("border")
    return paths


def _direct5_staging(Hp, Wp, HO, WO, vp):
    paths = set()
    for oy0 in range(0, HO, 8):
        for ox0 in range(0, WO, 8):
            gy0, cbase = 2 * oy0 - vp, 2 * ox0 - vp
            inside = (gy0 >= 0 and gy0 + 19 <= Hp and cbase >= 0
                      and cbase + 24 <= Wp)
            paths.add("tile_int" if inside else "border")
    return paths


@functools.lru_cache(maxsize=None)
def plan(c):
    """Every launch of one case's forward, backward-data and weight
    gradient, as ops/conv.py and csrc/conv.hip select them. route_f and
    route_b name the kind of the forward and backward-data launches:
    direct3, direct5, phase, gather, or flat (conv3d)."""
    B, Ci, Co = c.B, c.Ci, c.Co
    if c.kind == "conv3d":
        Dp, Hp, Wp = c.size
        Do, Ho, Wo = out_size(c)
        K = Ci * 18
        return dict(
            fwd=[_fwd_launch(B, Do * Ho * Wo, Co, K, Wo, 1, 0, 1)],
            dx=[_fwd_launch(B, Dp * Hp * Wp, Ci, Co * 18, Wp, 1, 0, 1)],
            dw=[_wrw_launch(B, Do * Ho * Wo, K, Co, Wo, 1, 0)],
            route_f="flat", route_b="flat")
    H, W = c.size
    kh, kw = c.k
    HO, WO = out_size(c)
    K = Ci * kh * kw
    if c.kind == "convT":
        st, sv, dil = 1, c.stride, 1
        pt, pl = kh - 1 - c.pad, kw - 1 - c.pad
        direct = 0
    else:
        st, sv, dil = c.stride, 1, c.dil
        pt = pl = c.pad
        direct = 0
        if st == 1 and dil == 1 and (kh, kw) == (3, 3) and Ci % 64 == 0 \
                and c.pad >= 1:
            direct = 1
        elif st == 2 and dil == 1 and (kh, kw) == (5, 5) and Ci % 64 == 0:
            direct = 2
    phases_f = None
    route_f = {2: "direct5", 1: "direct3"}.get(direct, "gather")
    if direct == 2:
        fwd = [dict(kern="direct5", KP=Ci * 25, vp=pt, sel=None,
                    staging=_direct5_staging(H, W, HO, WO, pt))]
    elif direct == 1:
        fwd = [dict(kern="direct3", KP=Ci * 9, vp=pt, sel=None,
                    staging=_direct3_staging(H, W, HO, WO, pt, Ci))]
    elif sv == 2 and dil == 1:
        route_f = "phase"
        phases_f = phase_list(HO, WO, kh, kw, Ci, pt, pl)
        fwd = [dict(_fwd_launch(B, p["nh"] * p["nw"], Co, p["Kp"], p["nw"],
                                1, 1, 1, sel=(p["a"], p["b"])), phase=True)
               for p in phases_f]
    else:
        fwd = [_fwd_launch(B, HO * WO, Co, K, WO, st, 1, sv)]
    ptb, plb = (kh - 1) * dil - pt, (kw - 1) * dil - pl
    phases_b = None
    route_b = "gather"
    if sv == 1 and st == 1 and dil == 1 and (kh, kw) == (3, 3) \
            and Co % 64 == 0 and ptb == plb and ptb >= 1:
        route_b = "direct3"
        dx = [dict(kern="direct3", KP=Co * 9, vp=ptb, sel=None,
                   staging=_direct3_staging(HO, WO, H, W, ptb, Co))]
    elif st == 2 and dil == 1:
        route_b = "phase"
        phases_b = phase_list(H, W, kh, kw, Co, ptb, plb)
        dx = [dict(_fwd_launch(B, p["nh"] * p["nw"], Ci, p["Kp"], p["nw"],
                               1, 1, 1, sel=(p["a"], p["b"])), phase=True)
              for p in phases_b]
    else:
        dx = [_fwd_launch(B, H * W, Ci, Co * kh * kw, W, sv, 1, st)]
    if sv == 2 and dil == 1:
        dw = [_wrw_launch(B, p["nh"] * p["nw"], p["Kp"], Co, p["nw"], 1, 1,
                          cols=p["ktab"]) for p in phases_f]
    else:
        dw = [_wrw_launch(B, HO * WO, K, Co, WO, st, 1)]
    return dict(fwd=fwd, dx=dx, dw=dw, route_f=route_f, route_b=route_b,
                nphase_f=None if phases_f is None else len(phases_f),
                nphase_b=None if phases_b is None else len(phases_b))


def dispatch(c):
    """Names of the instantiations and branches one case reaches: a mirror
    of the TM / VST / direct selection, read from plan()."""
    p = plan(c)
    f = set()
    roles = [("fwd", p["fwd"])] + ([("dx", p["dx"])] if c.xgrad else [])
    for role, launches in roles:
        for ln in launches:
            k = ln["kern"]
            f.update({k, f"{role}:{k}"})
            if k.startswith("fwd"):
                f.add(f"{k}:nchunks={min(ln['KP'] // 64, 6)}")
                if ln["vst"] != 0 and ln["WO"] in (8, 9):
                    f.add(f"{role}:WO=={ln['WO']}")
                if ln.get("phase"):
                    f.add("phase")
                    if ln["WO"] < 8:
                        f.add("phase:nw<8")
                    if ln["tm"] == 64 and ln["M"] > 64:
                        f.add("phase:TM64")
                    if role == "fwd" and c.bias and c.act:
                        f.add("phase:bias_act")
            else:
                f.add(f"{k}:{role}:vp={ln['vp']}")
                f.update(f"{k}:{s}" for s in ln["staging"])
                nch = ln["KP"] // (64 * (9 if k == "direct3" else 25))
                if nch >= 3:
                    f.add(f"{k}:chunks>=3")
                if nch > 1:
                    f.add(f"{k}:chunks>1")
                if role == "fwd" and c.bias and c.act:
                    f.add(f"{k}:bias_act")
    for key, role in (("nphase_f", "fwd"), ("nphase_b", "dx")):
        if p.get(key) is not None and p[key] < 4 and (role == "fwd"
                                                      or c.xgrad):
            f.add("phase:empty")
    for ln in p["dw"]:
        f.add(ln["kern"])
        if c.B * ln["pix_chunks"] == 1:
            f.add("wrw:view")
        if ln["pix_chunks"] > 1:
            f.add("wrw:chunks>1")
        for p0 in ln["p0s"]:
            if p0 >= ln["M"]:
                f.add("wrw:p0>=M")
            elif (min(p0 + ln["PCHUNK"], ln["M"]) - p0) % 8:
                f.add("wrw:tail%8")
    if c.kind == "conv" and c.stride not in (1, 2):
        f.add("stride3")
    if c.k[-2] != c.k[-1]:
        f.add("kh!=kw")
    if not c.xgrad:
        f.add("dx:off")
    return f


FWD_INSTANTIATIONS = {"fwd<%d,%d,%d,%d>" % ((tm,) + v)
                      for tm in (32, 64)
                      for v in ((0, 0, 1), (1, 1, 1), (1, 2, 1), (1, 0, 1),
                                (1, 1, 2), (1, 0, 2), (1, 0, 0))}
WRW_INSTANTIATIONS = {"wrw<0,0>", "wrw<1,0>", "wrw<1,1>", "wrw<1,2>"}
# every kernel ops/conv.py can launch on the bf16 path, and every branch
# docs/KERNELS.md lists as covered
REQUIRED = (
    FWD_INSTANTIATIONS | WRW_INSTANTIATIONS | {"direct3", "direct5"}
    | {"fwd<%d,1,1,1>:nchunks=%d" % (tm, n) for tm in (32, 64)
       for n in range(1, 6)}
    | {"fwd:WO==8", "fwd:WO==9", "stride3", "kh!=kw", "dx:off",
       "direct3:fwd:vp=1", "direct3:fwd:vp=2", "direct3:dx:vp=1",
       "direct3:dx:vp=2", "direct3:chunks>=3", "direct3:tile_int",
       "direct3:guarded_vec", "direct3:border", "direct3:bias_act",
       "direct5:chunks>1", "direct5:chunks>=3", "direct5:fwd:vp=0",
       "direct5:fwd:vp=2", "direct5:bias_act", "direct5:tile_int",
       "direct5:border", "phase", "phase:nw<8", "phase:empty",
       "phase:bias_act", "phase:TM64", "wrw:view", "wrw:p0>=M",
       "wrw:tail%8", "wrw:chunks>1"})


# ------------------------------------------------------------------ oracle

def _fn(c):
    if c.kind == "conv":
        return lambda x, w: F.conv2d(x, w, None, c.stride, c.pad, c.dil)
    if c.kind == "convT":
        return lambda x, w: F.conv_transpose2d(x, w, None, c.stride, c.pad,
                                               c.op)
    return lambda x, w: F.conv3d(x, w)


def _w_shape(c):
    return ((c.Ci, c.Co) if c.kind == "convT" else (c.Co, c.Ci)) + c.k


def operands(c):
    """(x, w, b, dy) of a case: x and dy are bf16 values in fp32, w and b
    fp32. Outputs have a standard deviation of about 1."""
    g = torch.Generator().manual_seed(zlib.crc32(case_id(c).encode()))
    x = torch.randn((c.B, c.Ci) + c.size, generator=g).bfloat16().float()
    fan = c.Ci * math.prod(c.k) / (c.stride ** 2 if c.kind == "convT" else 1)
    w = torch.randn(_w_shape(c), generator=g) / math.sqrt(fan)
    b = torch.randn(c.Co, generator=g) if c.bias else None
    dy = torch.randn((c.B, c.Co) + out_size(c),
                     generator=g).bfloat16().float()
    return x, w, b, dy


def _grads(fn, x, w, g):
    x = x.clone().requires_grad_(True)
    w = w.clone().requires_grad_(True)
    return torch.autograd.grad(fn(x, w), (x, w), g)


def _bshape(c):
    return (1, c.Co) + (1,) * len(c.size)


def _act(pre, act):
    if act == 1:
        return pre.clamp_min(0)
    if act == 2:
        return torch.where(pre > 0, pre, SLOPE * pre)
    return pre


def depth_maps(c):
    """depth of y and dx (broadcastable to them) and depth_w in the layout
    of the weight, from the launches plan() predicts."""
    p = plan(c)

    def pix_depth(launches, shape):
        if launches[0]["sel"] is None:
            return torch.tensor(float(32 + launches[0]["KP"] // 32 + 2),
                                dtype=torch.float64)
        # phases that run no launch hold bias alone: KP = 0
        d = torch.full(shape, 34.0, dtype=torch.float64)
        for ln in launches:
            a, b = ln["sel"]
            d[a::2, b::2] = 32 + ln["KP"] // 32 + 2
        return d

    dy_ = pix_depth(p["fwd"], out_size(c))
    dx_ = pix_depth(p["dx"], c.size)

    def wdepth(ln):
        return float(32 + ln["PCHUNK"] // 32 + c.B * ln["pix_chunks"] - 1)

    if p["dw"][0]["cols"] is None:
        dw_ = torch.tensor(wdepth(p["dw"][0]), dtype=torch.float64)
    else:   # conv-transpose: per phase, in the columns of w1 = (Co, K)
        kh, kw = c.k
        d1 = torch.zeros(c.Co, c.Ci * kh * kw, dtype=torch.float64)
        for ln in p["dw"]:
            d1[:, ln["cols"]] = wdepth(ln)
        dw_ = d1.view(c.Co, c.Ci, kh, kw).permute(1, 0, 2, 3).flip(2, 3)
    return dy_, dx_, dw_


def bound16(ref, S, depth):
    return U16 * ref.abs() + 2 * depth * U32 * S + 1e-12


def forward64(c, x, wb, b):
    """(pre, S_y) in fp64 on the rounded operands."""
    fn = _fn(c)
    pre = fn(x.double(), wb.double())
    S = fn(x.double().abs(), wb.double().abs())
    if b is not None:
        pre = pre + b.double().view(_bshape(c))
        S = S + b.double().abs().view(_bshape(c))
    return pre, S


@functools.lru_cache(maxsize=None)
def conv_reference(c):
    """Operands, fp64 references, S terms and bounds of one case (computed
    once, shared by the tests, never modified)."""
    x, w, b, dy = operands(c)
    wb = w.bfloat16().float()
    fn = _fn(c)
    d_y, d_dx, d_dw = depth_maps(c)
    pre, S_y = forward64(c, x, wb, b)
    y = _act(pre, c.act)
    bound_y = bound16(y, S_y, d_y)
    masked = 0.0
    if c.act:
        undecided = pre.abs() <= 2 * bound16(pre, S_y, d_y)
        masked = float(undecided.double().mean())
        dy = torch.where(undecided, torch.zeros(()), dy)
    # g = bf16(fp32(dy) * act'(y)), the expression of act_bwd_kernel
    if c.act == 1:
        g = torch.where(pre > 0, dy, torch.zeros(()))
    elif c.act == 2:
        g = torch.where(pre > 0, dy,
                        dy * torch.tensor(0.2, dtype=torch.float32))
        g = g.bfloat16().float()
    else:
        g = dy
    dx, dw = _grads(fn, x.double(), wb.double(), g.double())
    S_dx, S_dw = _grads(fn, x.double().abs(), wb.double().abs(),
                        g.double().abs())
    red = (0,) + tuple(range(2, g.dim()))
    r = dict(case=c, x=x, w=w, wb=wb, b=b, dy=dy, g=g, pre=pre, y=y, S_y=S_y,
             bound_y=bound_y, masked=masked, dx=dx, S_dx=S_dx,
             bound_dx=bound16(dx, S_dx, d_dx), dw=dw, S_dw=S_dw,
             bound_dw=2 * d_dw * U32 * S_dw)
    if c.bias:
        n = g.numel() // c.Co
        r.update(db=g.double().sum(red),
                 bound_db=n * U32 * g.double().abs().sum(red))
    return r


def cpu_fp32(c):
    """The CPU fp32 result on the same operands: y stored to bf16, dw."""
    r = conv_reference(c)
    fn = _fn(c)
    pre = fn(r["x"], r["wb"])
    if r["b"] is not None:
        pre = pre + r["b"].view(_bshape(c))
    y = _act(pre, c.act).bfloat16()
    _, dw = _grads(fn, r["x"], r["wb"], r["g"])
    return y, dw


def defect_forward(c):
    """The fp64 forward with one tap (the middle one) zeroed over the first
    64-channel chunk, all channels when Ci < 64: the smallest defect a
    chunked kernel can have."""
    r = conv_reference(c)
    wd = r["wb"].clone()
    mid = tuple(k // 2 for k in c.k)
    if c.kind == "convT":
        wd[(slice(0, 64), slice(None)) + mid] = 0
    else:
        wd[(slice(None), slice(0, 64)) + mid] = 0
    pre, _ = forward64(c, r["x"], wd, r["b"])
    return _act(pre, c.act)


def ratio(got, ref, bound):
    """Worst err/bound of one tensor (0/0 counts as 0)."""
    err = (got.double().cpu() - ref).abs()
    q = err / bound.expand_as(err).clamp_min(1e-300)
    return float(q.max())
