"""Time the entropy codec (encode_symbols / decode_symbols).

    python tools/bench_codec.py [--backend hip|torch|portable] [--device cpu]
                                [--runs 5] [--warmup 1]
                                [--shapes 32x8x12,32x40x120] [--zero-frac 0.5]

--device defaults to the GPU; --device cpu times the portable backend's host
build (or the torch backend) and reports the thread count.

For every symbol-volume shape CxHxW it prints one JSON line with the median
/ min / max wall time in ms of one encode and of one decode (host clock
around the call, device synchronised before and after), the stream size,
the number of waves and the number of kernel launches the hip backend
issues (encode: pc_freqs + rc_encode; decode: one state init plus pc_freqs
+ rc_decode_wave per wave). The probclass has the shipped shape (k=24,
L=6) with seeded random weights; every decode is checked against the
symbols.

--backend torch calls encode_symbols / decode_symbols without the backend
argument, so the tool also runs on a commit that predates it.
"""

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from dsin_amd import config as config_mod
from dsin_amd.coding import decode_symbols, encode_symbols
from dsin_amd.coding.entropy import _wave_order
from dsin_amd.models.probclass import ProbClass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(fn, dev):
    sync = torch.cuda.synchronize if dev.type == "cuda" else (lambda: None)
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return out, (time.perf_counter() - t0) * 1e3


def stats(ts):
    return {"median": round(statistics.median(ts), 3),
            "min": round(min(ts), 3), "max": round(max(ts), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", default="hip",
                    choices=["hip", "torch", "portable"])
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default="32x8x12,32x40x120")
    ap.add_argument("--zero-frac", type=float, default=0.5)
    args = ap.parse_args()
    dev = torch.device(args.device)
    if dev.type == "cuda" and not torch.cuda.is_available():
        sys.exit("bench_codec: needs a GPU (or --device cpu)")
    if dev.type != "cuda" and args.backend == "hip":
        sys.exit("bench_codec: the hip backend needs a GPU")
    kw = {} if args.backend == "torch" else {"backend": args.backend}

    pcc, _ = config_mod.parse(os.path.join(ROOT, "run_configs",
                                           "pc_run_configs"))
    L = 6
    torch.manual_seed(0)
    pc = ProbClass(pcc, num_centers=L).to(dev).eval()
    centers = torch.linspace(-2, 2, L, device=dev)

    for spec in args.shapes.split(","):
        shape = tuple(int(s) for s in spec.split("x"))
        g = torch.Generator().manual_seed(1)
        sym = torch.randint(0, L, shape, generator=g)
        sym[torch.rand(shape, generator=g) < args.zero_frac] = 0
        sym = sym.to(dev)
        waves = len(_wave_order(*shape, pc.context_size() // 2))
        enc_t, dec_t = [], []
        for i in range(args.warmup + args.runs):
            data, te = timed(lambda: encode_symbols(pc, centers, sym, **kw),
                             dev)
            out, td = timed(lambda: decode_symbols(pc, centers, data, shape,
                                                   **kw), dev)
            if not torch.equal(out, sym):
                sys.exit(f"bench_codec: roundtrip failed at {shape}")
            if i >= args.warmup:
                enc_t.append(te)
                dec_t.append(td)
        out = {"backend": args.backend, "device": dev.type,
               "shape": list(shape),
               "symbols": sym.numel(), "zero_frac": args.zero_frac,
               "runs": args.runs, "warmup": args.warmup, "waves": waves,
               "stream_bytes": len(data), "encode_ms": stats(enc_t),
               "decode_ms": stats(dec_t)}
        if dev.type != "cuda":
            out["threads"] = torch.get_num_threads()
        elif args.backend in ("hip", "portable"):
            out["encode_launches"] = 2
            out["decode_launches"] = 1 + 2 * waves
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
