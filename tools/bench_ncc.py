"""Time the side-information search on the GPU, both modes.

    python tools/bench_ncc.py [--iters 50] [--warmup 10] [--shape 320x960]
                              [--patch 20x24] [--torch-iters 3] [--cpu]
                              [--batch 1]

For one image of the given shape it prints one JSON line per run, in one
process, interleaved over --rounds rounds:
* pearson / l2lab, each with and without the location prior: median / min /
  max time in ms of one ops.ncc_search call from device events (one pair per
  call, after a warm-up), and the rise of torch's peak allocated memory over
  one call;
* with --batch B, in the same modes: pearson-batch / l2lab-batch, the same
  timing and memory figures for one ops.ncc_search_batch call on B distinct
  images (make_case with seeds 0..B-1); each line carries "batch": B;
* torch-l2lab (unless --torch-iters 0): the same for
  ops.reference.ncc_search_ref(l2lab=True) run on the GPU tensors, which is
  what the GPU served this mode with before the L2 kernels, and the share
  of patches where the kernel's location equals its location;
* with --cpu, the share of patches where the kernel's location equals that
  of the fp32 CPU path (slow: a dense fp32 correlation on the host).
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from dsin_amd import ops
from dsin_amd.ops import reference as ref


def make_case(h, w, noise=8.0, seed=0):
    """Smooth seeded x in 0..255, a noisy decoded side image, its original."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(3, h // 8 + 1, w // 8 + 1, generator=g)
    x = F.interpolate(base[None], size=(h, w), mode="bilinear")[0] * 255
    y_dec = (x + noise * torch.randn(x.shape, generator=g)).clamp(0, 255)
    y_orig = (y_dec + 2 * torch.randn(x.shape, generator=g)).clamp(0, 255)
    return x.contiguous(), y_dec.contiguous(), y_orig.contiguous()


def timed(fn, iters, warmup, dev):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.max_memory_allocated(dev)
    out = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(dev) - before
    times = []
    for _ in range(iters):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    return out, dict(iters=iters, ms_median=round(statistics.median(times), 4),
                     ms_min=round(min(times), 4), ms_max=round(max(times), 4),
                     peak_rise_bytes=int(rise))


def share(a, b):
    same = (a[1].cpu() == b[1].cpu()) & (a[2].cpu() == b[2].cpu())
    return round(float(same.double().mean()), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--shape", default="320x960")
    ap.add_argument("--patch", default="20x24")
    ap.add_argument("--torch-iters", type=int, default=3)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--batch", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ncc: needs a GPU")
    dev = torch.device("cuda:0")
    h, w = (int(s) for s in args.shape.split("x"))
    ph, pw = (int(s) for s in args.patch.split("x"))
    cpu_imgs = make_case(h, w)
    imgs = [t.to(dev) for t in cpu_imgs]
    p = (h // ph) * (w // pw)
    head = dict(shape=[3, h, w], patch=[ph, pw], patches=p,
                volume_bytes=p * (h - ph + 1) * (w - pw + 1) * 4,
                batch=args.batch)
    cases = [make_case(h, w, seed=b) for b in range(args.batch)]
    batch = [torch.stack([c[k] for c in cases]).to(dev) for k in range(3)]

    kernel = {}
    for rnd in range(args.rounds):
        for l2lab in (False, True):
            for mask in (True, False):
                out, t = timed(lambda: ops.ncc_search(*imgs, ph, pw, mask,
                                                      l2lab=l2lab),
                               args.iters, args.warmup, dev)
                kernel[(l2lab, mask)] = out
                print(json.dumps(dict(head, run="l2lab" if l2lab else "pearson",
                                      mask=mask, round=rnd, **t)), flush=True)
                _, t = timed(lambda: ops.ncc_search_batch(*batch, ph, pw, mask,
                                                          l2lab=l2lab),
                             args.iters, args.warmup, dev)
                print(json.dumps(dict(head, run=("l2lab" if l2lab else
                                                 "pearson") + "-batch",
                                      mask=mask, round=rnd, **t)), flush=True)
    for mask in (True, False):
        if args.torch_iters:
            out, t = timed(lambda: ref.ncc_search_ref(*imgs, ph, pw, mask,
                                                      l2lab=True),
                           args.torch_iters, 1, dev)
            print(json.dumps(dict(head, run="torch-l2lab", mask=mask, **t,
                                  kernel_equals_torch=share(
                                      kernel[(True, mask)], out))), flush=True)
        if args.cpu:
            out = ref.ncc_search_ref(*cpu_imgs, ph, pw, mask, l2lab=True)
            print(json.dumps(dict(head, run="cpu-l2lab", mask=mask,
                                  kernel_equals_cpu=share(
                                      kernel[(True, mask)], out))), flush=True)


if __name__ == "__main__":
    main()
