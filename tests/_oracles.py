"""Shared high-precision oracles for the GPU kernel tests.

Plain helper module (not a conftest): every function runs on the CPU and
takes the dtype to compute in, so the same expression gives the fp64 oracle
and the fp32 result whose error e32 calibrates the bounds
(|gpu - fp64| <= 4*e32 + floor, the rule of tests/test_gpu_msssim.py).
tests/test_oracles.py checks, on the CPU alone, the conditions the GPU tests
rely on (decided patches, masked shares, ...).
"""

import functools
import math

import torch
import torch.nn.functional as F

from dsin_amd.ops import reference as ref

U32 = 2.0 ** -24   # unit roundoff of fp32
U16 = 2.0 ** -8    # unit roundoff of bf16 (8 significand bits)


# ------------------------------------------------------------------- NCC

# (H, W, ph, pw, use_mask), noise 8; what each reaches is tabulated in
# tests/test_gpu_ncc.py and docs/KERNELS.md
NCC_V1_CASES = [(24, 80, 6, 10, True), (36, 160, 6, 20, True),
                (42, 135, 14, 15, False)]
NCC_V2_CASES = [(21, 96, 3, 8, False), (27, 72, 9, 8, False),
                (48, 112, 16, 8, True), (40, 144, 5, 24, False),
                (64, 96, 16, 16, True), (60, 168, 10, 24, True),
                (80, 120, 20, 24, True), (44, 200, 22, 40, True)]
# every case at noise 8, the first case of each kernel again at noise 25
NCC_CASES = ([c + (8,) for c in NCC_V1_CASES + NCC_V2_CASES]
             + [NCC_V1_CASES[0] + (25,), NCC_V2_CASES[0] + (25,)])

NCC_FLOOR = 1e-5  # 1-ulp rsq and __expf of the epilogue on |score| <= 1,
                  # about 2e-7 each, with a decade to spare


def ncc_v1_lds_bytes(ph, pw):
    """Dynamic LDS of ncc_main_kernel, the formula of ncc_lds_v1 in
    ncc_kernels.h, written out again."""
    tp, tj, ti, apad = 32, 128, 8, 8
    k = 3 * ph * pw
    kp = (k + 15) & ~15
    yr, ycp = ti + ph - 1, (tj + pw - 1 + 8) & ~7
    return (tp * (kp + apad) * 2 + 3 * yr * ycp * 2 + ((kp + 7) & ~7) * 2
            + 5 * tp * 4)


def ncc_case(h, w, seed, noise):
    """Smooth random x in 0..255, a noisy decoded side image and its
    'original' (fp32, CPU)."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(3, h // 8 + 1, w // 8 + 1, generator=g)
    x = F.interpolate(base[None], size=(h, w), mode="bilinear")[0] * 255
    y_dec = (x + noise * torch.randn(x.shape, generator=g)).clamp(0, 255)
    y_orig = (y_dec + 2 * torch.randn(x.shape, generator=g)).clamp(0, 255)
    return x.contiguous(), y_dec.contiguous(), y_orig.contiguous()


def ncc_map(x, y_dec, ph, pw, use_mask, dtype, round_bf16=True):
    """Dense (P, Hc, Wc) score map on the operands the kernel really uses:
    fixed normalization and H1H2H3 in fp32, rounded to bf16, everything
    after that in `dtype`, with the kernel's algebra (max(den, 1e-10) under
    the root, the location prior from its inline formula, valid for any
    patch size). round_bf16=False keeps the fp32 operands, as the CPU path
    ref.ncc_search_ref does."""
    _, h, w = x.shape
    gw = w // pw
    q = ref._h1h2h3(ref._sifinder_norm(ref.extract_patches(x.float(), ph, pw)))
    r = ref._h1h2h3(ref._sifinder_norm(y_dec.float()))
    if round_bf16:
        q, r = q.to(torch.bfloat16), r.to(torch.bfloat16)
    q, r = q.to(dtype), r.to(dtype).unsqueeze(0)
    k = float(3 * ph * pw)
    xy = F.conv2d(r, q)[0]
    ones = r.new_ones(1, 3, ph, pw)
    sy = F.conv2d(r, ones)[0, 0]
    sy2 = F.conv2d(r * r, ones)[0, 0]
    sx = q.sum(dim=(1, 2, 3)).view(-1, 1, 1)
    sx2 = (q * q).sum(dim=(1, 2, 3)).view(-1, 1, 1)
    xm, ym = sx / k, sy / k
    denx = sx2 - 2 * xm * sx + k * xm * xm
    deny = sy2 - 2 * ym * sy + k * ym * ym
    num = xy - ym * sx - xm * sy + k * xm * ym
    val = num / torch.sqrt((denx * deny).clamp_min(1e-10))
    if use_mask:
        p = torch.arange(q.shape[0], dtype=dtype)
        cr = (torch.div(p, gw, rounding_mode="floor") + 0.5) * ph
        cw = (p % gw + 0.5) * pw
        di = torch.arange(h - ph + 1, dtype=dtype) + (ph // 2 - 1)
        dj = torch.arange(w - pw + 1, dtype=dtype) + (pw // 2 - 1)
        dd = (di.view(1, -1, 1) - cr.view(-1, 1, 1)) ** 2 * (4.0 / (h * h))
        dw = (dj.view(1, 1, -1) - cw.view(-1, 1, 1)) ** 2 * (4.0 / (w * w))
        val = val * torch.exp(-4.0 * math.log(2.0) * (dd + dw))
    return val


def ncc_decide(m64, m32):
    """(bound, argmax rows, cols, decided mask, top-2 gaps) of one case."""
    p, hc, wc = m64.shape
    e32 = float((m32.double() - m64).abs().max())
    bound = 4 * e32 + NCC_FLOOR
    top = m64.reshape(p, -1).topk(2, dim=1)
    gaps = top.values[:, 0] - top.values[:, 1]
    idx = top.indices[:, 0]
    return dict(e32=e32, bound=bound, gaps=gaps, decided=gaps > bound,
                rows=torch.div(idx, wc, rounding_mode="floor"),
                cols=idx % wc, vmax=top.values[:, 0])


@functools.lru_cache(maxsize=None)
def ncc_reference(h, w, ph, pw, use_mask, noise):
    """Inputs, fp64 map and decision data of one case (computed once,
    shared by the tests, never modified)."""
    x, y_dec, y_orig = ncc_case(h, w, 100 * h + w + ph + int(noise), noise)
    m64 = ncc_map(x, y_dec, ph, pw, use_mask, torch.float64)
    m32 = ncc_map(x, y_dec, ph, pw, use_mask, torch.float32)
    d = ncc_decide(m64, m32)
    d.update(x=x, y_dec=y_dec, y_orig=y_orig, m64=m64)
    return d


def ncc_flat_case(use_mask):
    """32x64 image whose top-left 8x16 is saturated in x and y: the 8x8
    patches 0 and 1 have zero variance."""
    x, y_dec, y_orig = ncc_case(32, 64, 77, 8)
    for t in (x, y_dec, y_orig):
        t[:, :8, :16] = 255.0
    m64 = ncc_map(x, y_dec, 8, 8, use_mask, torch.float64)
    m32 = ncc_map(x, y_dec, 8, 8, use_mask, torch.float32)
    d = ncc_decide(m64, m32)
    d.update(x=x, y_dec=y_dec, y_orig=y_orig, m64=m64)
    d["decided"] = d["decided"].clone()
    d["decided"][:2] = False  # zero-variance patches: score is rounding noise
    return d


# (block h, block w, tiles y, tiles x, ph, pw)
NCC_TIE_CASES = [(16, 24, 3, 4, 8, 8), (12, 20, 3, 5, 6, 10),
                 (20, 48, 2, 3, 20, 24)]


def ncc_tie_case(ty, tx, ny, nx, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    block = torch.rand(3, ty, tx, generator=g) * 255
    return block.repeat(1, ny, nx).contiguous()


def ncc_check_gather(y_syn, rows, cols, y_orig, ph, pw):
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


# ------------------------------------------------------------ batch norm

BN_SHAPES = [(2, 32, 20, 24), (3, 5, 7, 9), (2, 3, 1, 5), (2, 3, 65, 67),
             (1, 2, 220, 300), (2, 8, 20, 24)]
BN_SHIFTED = (2, 8, 20, 24)  # run with the mean shifted by 8 std


def bn_cases():
    """(id, bn_case keyword arguments) of every BN case of the GPU tests."""
    out = []
    for shape in BN_SHAPES:
        for act in (0, 1, 2):
            out.append(dict(shape=shape, act=act,
                            shifted=shape == BN_SHIFTED))
    out.append(dict(shape=(3, 5, 7, 9), act=1, momentum=0.25))
    for shape in ((3, 5, 7, 9), (2, 3, 65, 67)):
        for act in (0, 2):
            out.append(dict(shape=shape, act=act, training=False))
        out.append(dict(shape=shape, act=0, residual=True))
    ids = ["-".join(f"{k}={v}".replace(" ", "") for k, v in kw.items())
           for kw in out]
    return ids, out


BN_ACT_EDGE = 1e-3


def bn_spatial_chunks(hw):
    """S of bn.hip (_spatial_chunks)."""
    return min(max(hw // 2048, 1), 32)


def bn_depth(b, hw):
    """Longest chain of fp32 additions one summand passes through in
    bn_stats_part / bn_bwd_part plus the sum over the S slices: the
    thread's own elements (per image ceil(vectors / (S*256)) vectors of 8,
    plus one tail element in slice 0), 6 shuffle steps, the 3 additions
    over the 4 waves, and S-1 over the slices."""
    s = bn_spatial_chunks(hw)
    iters = -(-(hw // 8) // (s * 256))
    per_thread = b * (8 * iters + (1 if hw % 8 else 0))
    return per_thread + 6 + 3 + (s - 1)


def _act(z, act):
    if act == 1:
        return z.clamp_min(0)
    if act == 2:
        return torch.maximum(z, 0.2 * z)
    return z


def _bn_eval(dt, x, gamma, beta, res, act, training, rmean, rvar, momentum,
             eps, dy):
    x, gamma, beta, rmean, rvar = (t.to(dt) for t in
                                   (x, gamma, beta, rmean, rvar))
    b, c, h, w = x.shape
    n = b * h * w
    v = lambda t: t.view(1, -1, 1, 1)
    if training:
        # the kernel's form: E[x^2] - m^2, biased; unbiased for the EMA
        m = x.sum(dim=(0, 2, 3)) / n
        var = (x.square().sum(dim=(0, 2, 3)) / n - m * m).clamp_min(0)
        unb = var * n / (n - 1) if n > 1 else var
        new_rm = (1 - momentum) * rmean + momentum * m
        new_rv = (1 - momentum) * rvar + momentum * unb
    else:
        m, var, new_rm, new_rv = rmean, rvar, rmean, rvar
    rs = torch.rsqrt(var + eps)
    sc = gamma * rs
    pre = x * v(sc) + v(beta - m * sc)
    if res is not None:
        pre = pre + res.to(dt)
    out = _act(pre, act)
    r = dict(pre=pre, out=out, running_mean=new_rm, running_var=new_rv)
    if dy is None:
        return r
    g = dy.to(dt)
    if act == 1:
        g = torch.where(pre > 0, g, torch.zeros_like(g))
    elif act == 2:
        g = torch.where(pre > 0, g, 0.2 * g)
    xh = (x - v(m)) * v(rs)
    t_beta, t_gamma = g, g * xh
    dbeta, dgamma = t_beta.sum(dim=(0, 2, 3)), t_gamma.sum(dim=(0, 2, 3))
    if training:
        dx = v(gamma * rs) * (g - v(dbeta) / n - xh * v(dgamma) / n)
    else:
        dx = v(gamma * rs) * g
    r.update(dx=dx, dgamma=dgamma, dbeta=dbeta,
             dres=dy.to(dt) if res is not None else None,
             abs_beta=t_beta.abs().sum(dim=(0, 2, 3)),
             abs_gamma=t_gamma.abs().sum(dim=(0, 2, 3)))
    return r


def bn_oracle(x, gamma, beta, res, act, training, rmean, rvar, momentum, eps,
              dy=None):
    """Fused BN(+residual)(+act) forward and backward, in fp64 and in fp32.
    x, res and dy hold bf16 values (in any dtype). Returns (r64, r32), dicts
    of out, dx, dgamma, dbeta, dres, running_mean, running_var, the
    pre-activation, and abs_gamma / abs_beta: the sums of the absolute
    summands of dgamma / dbeta per channel."""
    args = (x, gamma, beta, res, act, training, rmean, rvar, momentum, eps, dy)
    return _bn_eval(torch.float64, *args), _bn_eval(torch.float32, *args)


def bn_case(shape, act, seed=0, shifted=False, residual=False, training=True,
            momentum=0.1, eps=1e-5):
    """Seeded inputs of one BN case (bf16 values held in fp32, CPU). For act
    1 and 2, dy is zeroed wherever the fp64 pre-activation is within
    BN_ACT_EDGE of zero, so that neither side's rounding decides the branch
    of the activation gradient; `masked` is that share."""
    b, c, h, w = shape
    g = torch.Generator().manual_seed(seed + 17 * h + w + 1000 * act)
    bf = lambda t: t.to(torch.bfloat16).float()
    x = 2 * torch.randn(shape, generator=g) + 1
    if shifted:
        x = x + 8 * 2.0
    x = bf(x)
    gamma = torch.rand(c, generator=g) + 0.5
    beta = 0.3 * torch.randn(c, generator=g)
    rmean = torch.rand(c, generator=g) * 2 - 1
    rvar = torch.rand(c, generator=g) * 1.5 + 0.5
    if not training:  # eval: statistics near the data's
        rmean, rvar = rmean + 1, rvar * 4
    res = bf(torch.randn(shape, generator=g)) if residual else None
    dy = bf(torch.randn(shape, generator=g))
    pre64 = _bn_eval(torch.float64, x, gamma, beta, res, act, training, rmean,
                     rvar, momentum, eps, None)["pre"]
    masked = 0.0
    if act in (1, 2):
        edge = pre64.abs() < BN_ACT_EDGE
        dy = torch.where(edge, torch.zeros_like(dy), dy)
        masked = float(edge.float().mean())
    return dict(x=x, gamma=gamma, beta=beta, res=res, act=act,
                training=training, rmean=rmean, rvar=rvar, momentum=momentum,
                eps=eps, dy=dy, masked=masked)


def bn_case_oracle(case):
    keys = ("x", "gamma", "beta", "res", "act", "training", "rmean", "rvar",
            "momentum", "eps", "dy")
    return bn_oracle(*(case[k] for k in keys))


# ------------------------------------------------------------- pointwise

def quantize_oracle(x, centers, sigma, g, dt):
    """(qsoft-path forward, symbols, gx, gc, per-center sum of |summands|,
    relative gap of the two smallest distances) in dtype dt."""
    x = x.clone().to(dt).requires_grad_(True)
    c = centers.clone().to(dt).requires_grad_(True)
    d = (x.unsqueeze(-1) - c) ** 2
    phi = F.softmax(-sigma * d, dim=-1)
    qsoft = (phi * c).sum(-1)
    sym = d.argmin(dim=-1)
    gx, gc = torch.autograd.grad(qsoft, (x, c), g.to(dt))
    with torch.no_grad():
        # d qsoft / d c_j = phi_j + 2 sigma (x - c_j) phi_j (c_j - qsoft)
        dq = phi + 2 * sigma * (x.unsqueeze(-1) - c) * phi * (
            c - qsoft.unsqueeze(-1))
        gc_abs = (g.to(dt).unsqueeze(-1) * dq).abs().reshape(-1, c.numel()).sum(0)
        if c.numel() > 1:
            two = d.topk(2, dim=-1, largest=False).values
            relgap = (two[..., 1] - two[..., 0]) / two[..., 1].clamp_min(1e-30)
        else:
            relgap = torch.ones_like(x)
    return dict(qhard=c.detach()[sym], sym=sym, gx=gx, gc=gc, gc_abs=gc_abs,
                relgap=relgap.detach())


def adam_oracle(p, grads, lrs, wd, b1=0.9, b2=0.999, eps=1e-8,
                dt=torch.float64):
    """TF-semantics Adam over flat buffers, written out independently of
    FusedAdam: one step per entry of grads / lrs; wd is None or per-element
    L2 factors. Returns the parameter after every step."""
    p = p.to(dt).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    out = []
    for t, (g, lr) in enumerate(zip(grads, lrs), start=1):
        g = g.to(dt)
        if wd is not None:
            g = g + wd.to(dt) * p
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        corr = lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
        p = p - corr * m / (v.sqrt() + eps)
        out.append(p.clone())
    return out


def bn_bounds(case, r64, r32):
    """Bounds of the BN tests against the fp64 oracle r64; e32 is the max
    error of the unrounded fp32 CPU result r32.

    out, dx (bf16 stores), elementwise:
        2^-8*|ref| + 4*e32 + 1e-6   (bf16 term; floor about 8 fp32 ulp at 1)
    dgamma, dbeta (fp32 sums), per channel:
        4*e32 + depth*2^-24*sum|t_i|  (worst case of any summation in which
        a summand passes through at most `depth` additions, bn_depth())
    running_var / running_mean: the kernel forms E[x^2] - m^2 from two such
    sums, so
        4*e32 + momentum*depth*2^-24*(mean(x^2) + mean(x)^2)*n/(n-1)
        4*e32 + momentum*depth*2^-24*mean|x|
    Returns {name: (bound tensor, e32)}."""
    x = case["x"].double()
    b, c, h, w = x.shape
    n = b * h * w
    depth = bn_depth(b, h * w)
    e = lambda k: float((r32[k].double() - r64[k]).abs().max())
    out = {}
    for k in ("out", "dx"):
        if k in r64:
            out[k] = (U16 * r64[k].abs() + 4 * e(k) + 1e-6, e(k))
    if "dgamma" in r64:
        out["dgamma"] = (4 * e("dgamma") + depth * U32 * r64["abs_gamma"],
                         e("dgamma"))
        out["dbeta"] = (4 * e("dbeta") + depth * U32 * r64["abs_beta"],
                        e("dbeta"))
    if case["training"]:
        mom = case["momentum"]
        mx2 = x.square().mean(dim=(0, 2, 3))
        mx = x.mean(dim=(0, 2, 3))
        out["running_var"] = (
            4 * e("running_var")
            + mom * depth * U32 * (mx2 + mx * mx) * n / (n - 1),
            e("running_var"))
        out["running_mean"] = (
            4 * e("running_mean")
            + mom * depth * U32 * x.abs().mean(dim=(0, 2, 3)),
            e("running_mean"))
    return out


def quantizer_inputs(n, L, seed=0):
    """(x, centers, g): x = 2*randn with 64 elements moved more than 40
    away from every center (the softmax underflows there), slightly uneven
    centers."""
    gen = torch.Generator().manual_seed(seed)
    centers = torch.linspace(-2, 2, L) + 0.05 * torch.randn(L, generator=gen)
    x = 2 * torch.randn(n, generator=gen)
    far = 44 + torch.rand(64, generator=gen)
    far[::2] *= -1
    x[:64] = far
    return x, centers, torch.randn(n, generator=gen)


def heatmap_inputs(dtype, shape=(2, 33, 10, 12)):
    """Bottleneck (values of `dtype`, held in fp32) whose heatmap logit is
    exactly 0 on every 7th pixel: sigmoid(0) = 0.5 and C = 32 are exact, so
    h2 - c lands exactly on 1 (c = 15) and on 0 (c = 16) there. Also the
    mask of pixels where some h2 - c comes within 1e-4 of a clamp edge
    without sitting on it; the gradient of the logit is not compared there
    (rounding decides the clamp's branch)."""
    gen = torch.Generator().manual_seed(11)
    b = (torch.randn(shape, generator=gen) * 3).to(dtype).float()
    n, _, h, w = shape
    zero = (torch.arange(n * h * w) % 7 == 0).view(n, h, w)
    b[:, 0] = torch.where(zero, torch.zeros(()), b[:, 0])
    c = shape[1] - 1
    v = (torch.sigmoid(b[:, 0].double()) * c).unsqueeze(1) - torch.arange(
        c, dtype=torch.float64).view(1, -1, 1, 1)
    near = torch.minimum(v.abs(), (v - 1).abs()).min(dim=1).values < 1e-4
    return b, near & (b[:, 0] != 0)


ADAM_SMALL_SIZES = [[(1,)], [(3,)], [(2, 2)], [(5,)], [(3,), (4,)],
                    [(3, 5), (7,), (2, 3, 4)]]          # flat n 1,3,4,5,7,46
ADAM_LARGE_SIZES = [(1027,), (2097152,)]  # grid-stride loop, n % 4 == 3
ADAM_LRS = (1e-2, 5e-3, 2e-2)


def run_adam_case(sizes, use_wd, device):
    """Three FusedAdam steps on `device` (lr changed on the device between
    them, weight decay on the last parameter if use_wd) against adam_oracle
    in fp64. With e32 the error of the same oracle in fp32,

        |p - p64| <= 4*e32 + sum_steps (2^-16*|step| + 4*2^-24*|p64|)

    2^-16 of the step: b2 = 0.999 held in fp32 is off by 1.3e-8, that is
    1.3e-5 of 1 - b2, which enters the step through sqrt(1 - b2^t) and
    sqrt(v) (6.5e-6 each); the rest is a few ulp of the parameter."""
    from dsin_amd.ops.adam import FusedAdam
    gen = torch.Generator().manual_seed(sum(sum(s) for s in sizes))
    init = [torch.randn(s, generator=gen) for s in sizes]
    grads = [[torch.randn(s, generator=gen) for s in sizes] for _ in ADAM_LRS]
    params = [torch.nn.Parameter(t.clone().to(device)) for t in init]
    opt = FusedAdam(params, lr=ADAM_LRS[0])
    wd = None
    if use_wd:
        assert opt.set_weight_decay(params[-1], 0.05)
        wd = torch.cat([torch.full((t.numel(),), 0.05 if i == len(init) - 1
                                   else 0.0) for i, t in enumerate(init)])
    flat = lambda ts: torch.cat([t.reshape(-1) for t in ts])
    p0 = flat(init)
    r64 = adam_oracle(p0, [flat(g) for g in grads], ADAM_LRS, wd)
    r32 = adam_oracle(p0, [flat(g) for g in grads], ADAM_LRS, wd,
                      dt=torch.float32)
    prev, floor = p0.double(), torch.zeros_like(p0, dtype=torch.float64)
    worst = 0.0
    for t, lr in enumerate(ADAM_LRS):
        opt.lr_t.fill_(lr)
        opt.zero_grad()
        for p, g in zip(params, grads[t]):
            p.grad = g.clone().to(device)
        opt.gather_grads()
        opt.step()
        floor = floor + 2.0 ** -16 * (r64[t] - prev).abs() + 4 * U32 * r64[t].abs()
        prev = r64[t]
        e32 = float((r32[t].double() - r64[t]).abs().max())
        err = (opt.flat_p.detach().double().cpu() - r64[t]).abs()
        worst = max(worst, float((err / (4 * e32 + floor)).max()))
        assert bool((err <= 4 * e32 + floor).all()), (sizes, t, float(err.max()))
        # the parameters are views of the flat buffer
        assert torch.equal(flat([p.detach() for p in params]), opt.flat_p)
    return worst
