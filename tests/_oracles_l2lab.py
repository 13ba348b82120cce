"""fp64 oracle of the L2+LAB side-information search (use_L2andLAB).

Plain helper module, as tests/_oracles.py: everything runs on the CPU. The
scores of this mode are squared distances of LAB values in the thousands,
not correlations of magnitude <= 1, so the bounds are pointwise instead of
one number per case. With the operands tx, ty the search really used (LAB
rounded to bf16):

    d64, d32   sum_x2 - 2*xy + sum_y2 by F.conv2d in fp64 and in fp32
    e32[p]     max over locations of |d32 - d64|
    g          the location prior in fp64, from the kernel's inline formula
               (1 without the mask)
    m64        d64 * g
    b          4*e32[p]*g + 1e-5*|m64|

4 x the CPU's fp32 error is the project's margin for another summation
order, and 1e-5 relative is NCC_FLOOR of tests/_oracles.py, the allowance
for __expf. With l* the fp64 argmin, a patch is decided when

    min over l != l* of (m64[l] - b[l])  >  m64[l*] + b[l*]

A decided patch must come back at exactly l*; any other patch at a
location l with m64[l] - b[l] <= m64[l*] + b[l*].
"""

import functools
import math

import torch
import torch.nn.functional as F

import _oracles as O
from dsin_amd.ops import reference as ref

# the three shapes also run with the mask flipped (one v1, two v2)
L2_FLIPPED = [(24, 80, 6, 10), (48, 112, 16, 8), (80, 120, 20, 24)]
L2_GPU_CASES = list(O.NCC_CASES) + [
    (h, w, ph, pw, not m, n) for (h, w, ph, pw, m, n) in O.NCC_CASES
    if (h, w, ph, pw) in L2_FLIPPED and n == 8]
# every entry of NCC_CASES without the mask, and with it where the patch is
# even (the prior is defined for even patches only)
L2_CPU_CASES = sorted(set(
    [c[:4] + (False,) + c[5:] for c in O.NCC_CASES]
    + [c[:4] + (True,) + c[5:] for c in O.NCC_CASES
       if c[2] % 2 == 0 and c[3] % 2 == 0]))


def lab64(x):
    """rgb_to_lab_ref in fp64 (that function forces fp32): x (3, H, W) in
    any dtype -> (3, H, W) fp64. Same branches, matrices and white point."""
    px = x.double().movedim(-3, -1).reshape(-1, 3)
    lin = torch.where(px <= 0.04045, px / 12.92,
                      ((px + 0.055) / 1.055).clamp(min=0.0) ** 2.4)
    m = torch.tensor(((0.412453, 0.212671, 0.019334),
                      (0.357580, 0.715160, 0.119193),
                      (0.180423, 0.072169, 0.950227)), dtype=torch.float64)
    xyz = (lin @ m) * torch.tensor((1.0 / 0.950456, 1.0, 1.0 / 1.088754),
                                   dtype=torch.float64)
    eps3 = (6.0 / 29.0) ** 3
    f = torch.where(xyz <= eps3, xyz / (3 * (6.0 / 29.0) ** 2) + 4.0 / 29.0,
                    xyz.clamp(min=0.0) ** (1.0 / 3.0))
    t = torch.tensor(((0.0, 500.0, 0.0), (116.0, -500.0, 200.0),
                      (0.0, 0.0, -200.0)), dtype=torch.float64)
    lab = f @ t + torch.tensor((-16.0, 0.0, 0.0), dtype=torch.float64)
    return lab.reshape(*x.movedim(-3, -1).shape).movedim(-1, -3)


def lab_case(h, w, ph, pw, noise):
    """Inputs of one search case: the images of the Pearson case of the
    same shape (same seed)."""
    return O.ncc_case(h, w, 100 * h + w + ph + int(noise), noise)


def lab_operands_cpu(x, y_dec):
    """What the CPU could give the kernel: rgb_to_lab_ref rounded to bf16."""
    return (ref.rgb_to_lab_ref(x).to(torch.bfloat16),
            ref.rgb_to_lab_ref(y_dec).to(torch.bfloat16))


def _dist(tx, ty, ph, pw, dtype):
    q = ref.extract_patches(tx.to(dtype), ph, pw)
    r = ty.to(dtype).unsqueeze(0)
    xy = F.conv2d(r, q)[0]
    sy2 = F.conv2d(r * r, r.new_ones(1, 3, ph, pw))[0, 0]
    sx2 = (q * q).sum(dim=(1, 2, 3)).view(-1, 1, 1)
    return sx2 - 2 * xy + sy2.unsqueeze(0)


def _prior64(h, w, ph, pw):
    gw = w // pw
    p = torch.arange((h // ph) * gw, dtype=torch.float64)
    cr = (torch.div(p, gw, rounding_mode="floor") + 0.5) * ph
    cw = (p % gw + 0.5) * pw
    di = torch.arange(h - ph + 1, dtype=torch.float64) + (ph // 2 - 1)
    dj = torch.arange(w - pw + 1, dtype=torch.float64) + (pw // 2 - 1)
    dd = (di.view(1, -1, 1) - cr.view(-1, 1, 1)) ** 2 * (4.0 / (h * h))
    dw = (dj.view(1, 1, -1) - cw.view(-1, 1, 1)) ** 2 * (4.0 / (w * w))
    return torch.exp(-4.0 * math.log(2.0) * (dd + dw))


def l2_decide(tx, ty, ph, pw, use_mask):
    """Decision data of one case from the operands tx, ty (3, H, W): m64
    and b as (P, Hc*Wc), the fp64 argmin as rows/cols/best, and the decided
    mask."""
    _, h, w = tx.shape
    d64 = _dist(tx, ty, ph, pw, torch.float64)
    d32 = _dist(tx, ty, ph, pw, torch.float32)
    p, hc, wc = d64.shape
    e32 = (d32.double() - d64).abs().amax(dim=(1, 2)).view(-1, 1, 1)
    g = _prior64(h, w, ph, pw) if use_mask else torch.ones_like(d64)
    m64 = d64 * g
    b = (4 * e32 * g + O.NCC_FLOOR * m64.abs()).reshape(p, -1)
    m64 = m64.reshape(p, -1)
    best = m64.argmin(dim=1)
    thr = (m64 + b).gather(1, best[:, None])[:, 0]
    rest = m64 - b
    rest.scatter_(1, best[:, None], float("inf"))
    return dict(m64=m64, b=b, thr=thr, best=best, wc=wc,
                rows=torch.div(best, wc, rounding_mode="floor"),
                cols=best % wc, decided=rest.min(dim=1).values > thr,
                e32=float(e32.max()))


def l2_check(d, rows, cols, label):
    """Asserts the oracle's conditions on returned locations and the 90%
    cap. Returns the worst ratio (m64[l] - m64[l*]) / (b[l] + b[l*]) over
    all patches (0 where l = l*); the condition on an undecided patch is
    that its ratio is at most 1."""
    flat = (rows * d["wc"] + cols)[:, None]
    same = flat[:, 0] == d["best"]
    dec = d["decided"]
    m, b = d["m64"].gather(1, flat)[:, 0], d["b"].gather(1, flat)[:, 0]
    m0 = d["m64"].gather(1, d["best"][:, None])[:, 0]
    ratio = (m - m0) / (b + d["thr"] - m0).clamp_min(1e-300)
    share = float(dec.double().mean())
    print(f"l2lab {label}: P {rows.numel()} decided {int(dec.sum())} agree "
          f"{int(same.sum())} e32 {d['e32']:.3e} worst ratio "
          f"{float(ratio.max()):.3f}")
    assert share >= 0.9, share
    assert bool(same[dec].all()), torch.nonzero(dec & ~same).flatten().tolist()
    assert bool((m - b <= d["thr"])[~dec].all())
    return float(ratio.max())


@functools.lru_cache(maxsize=None)
def l2_cpu_reference(h, w, ph, pw, use_mask, noise):
    """Inputs and decision data of one case on the CPU's bf16 operands
    (computed once, shared, never modified)."""
    x, y_dec, y_orig = lab_case(h, w, ph, pw, noise)
    tx, ty = lab_operands_cpu(x, y_dec)
    d = l2_decide(tx, ty, ph, pw, use_mask)
    d.update(x=x, y_dec=y_dec, y_orig=y_orig)
    return d
