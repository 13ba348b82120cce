"""Time and check losses.multiscale_ssim forward+backward on the GPU.

    python tools/bench_msssim.py [--iters 50] [--warmup 10]
                                 [--shapes 320x960,1024x2048] [--no-errors]

For every shape (batch 1, 3 channels) it prints one JSON line with
* the median / min / max time in ms of one forward + backward (gradient
  w.r.t. the second argument only) from device events, one pair per
  iteration, after a warm-up, all in this one process;
* the error of the value and the relative-L2 error of the gradient against
  an fp64 evaluation of the same inputs on the CPU.

Only the public function is used, so the tool runs unchanged on any commit
that has it. For a kernel count per evaluation run it under a kernel trace
with --warmup 0 --no-errors and divide the calls by --iters.
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from dsin_amd.losses import multiscale_ssim


def make_pair(h, w, sigma=3.0, seed=0):
    """Smooth seeded fp64 image in 0..255 plus Gaussian noise, clamped."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(1, 3, h // 4 + 2, w // 4 + 2, generator=g,
                      dtype=torch.float64) * 255
    a = F.interpolate(base, size=(h, w), mode="bilinear", align_corners=False)
    n = torch.randn(a.shape, generator=g, dtype=torch.float64) * sigma
    return a, (a + n).clamp(0, 255)


def fwd_bwd(a, b):
    b = b.detach().requires_grad_(True)
    v = multiscale_ssim(a, b)
    (g,) = torch.autograd.grad(v, b)
    return v.detach(), g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--shapes", default="320x960,1024x2048")
    ap.add_argument("--sigma", type=float, default=3.0)
    ap.add_argument("--no-errors", action="store_true",
                    help="skip the fp64 CPU oracle")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_msssim: needs a GPU")
    dev = torch.device("cuda:0")

    for spec in args.shapes.split(","):
        h, w = (int(s) for s in spec.split("x"))
        a64, b64 = make_pair(h, w, args.sigma)
        a, b = a64.float().to(dev), b64.float().to(dev)
        for _ in range(args.warmup):
            fwd_bwd(a, b)
        torch.cuda.synchronize()
        times = []
        for _ in range(args.iters):
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            v, g = fwd_bwd(a, b)
            t1.record()
            t1.synchronize()
            times.append(t0.elapsed_time(t1))
        out = {"shape": [1, 3, h, w], "sigma": args.sigma,
               "iters": args.iters, "warmup": args.warmup,
               "ms_median": round(statistics.median(times), 4),
               "ms_min": round(min(times), 4),
               "ms_max": round(max(times), 4),
               "value": float(v)}
        if not args.no_errors:
            v64, g64 = fwd_bwd(a64, b64)
            out["value_fp64"] = float(v64)
            out["value_err"] = abs(float(v) - float(v64))
            out["grad_rel_l2"] = float((g.double().cpu() - g64).norm()
                                       / g64.norm())
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
