"""Time the entropy codec (encode_symbols / decode_symbols).

    python tools/bench_codec.py [--backend hip|torch|portable] [--device cpu]
                                [--runs 5] [--warmup 1]
                                [--shapes 32x8x12,32x40x120] [--zero-frac 0.5]
                                [--batch 1,2,4,8,16]
                                [--ragged 32x46x155,32x46x153,..]

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

With the hip and portable backends encode_symbols / decode_symbols are a
batch of one through the batch functions (ops.pc_encode_batch /
pc_decode_batch and the extension's pc_encode / pc_decode, which take
(B, ...) only), so the single-image lines time that path at B = 1.

--backend torch calls encode_symbols / decode_symbols without the backend
argument, so the tool also runs on a commit that predates it.

--batch B1,B2,.. times the batched codec instead: for every shape and every
B one JSON line with the time of ONE encode_symbols_batch /
decode_symbols_batch call over B different symbol volumes ("batched") next
to the time of B sequential encode_symbols / decode_symbols calls on the
same volumes ("sequential"), taken alternately in the same process, their
ratio (sequential median / batched median), the batched cost per image and
the launch counts computed from the wave schedule (encode 2, decode
1 + 2 * waves, whatever B is; nothing counts them at run time, the C++ wave
loop issues exactly these and a kernel trace confirms it). Every
decode, batched and sequential, is checked against the symbols, and the
batched streams against the sequential ones.

--ragged SHAPE,SHAPE,.. times a batch of symbol volumes of different shapes
(a shape may repeat; --shapes and --batch are ignored) three ways,
alternately in one process: "ragged", one encode_symbols_ragged /
decode_symbols_ragged call over all the volumes; "grouped", one
encode_symbols_batch / decode_symbols_batch call per group of equal shapes
(the best the uniform batch path can do); "single", one encode_symbols /
decode_symbols call per volume. One JSON line with the three times for
encode and for decode, the ratios against ragged, and the launch counts
computed from the schedules (ragged decode: one state init plus two per
non-empty wave of the merged schedule). Every run compares the three sets of
streams byte for byte and every decode against the symbols.
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


def bench_batch(args, dev, pc, centers, L, shape, B):
    """One JSON line: a batched call against B sequential calls."""
    from dsin_amd.coding import decode_symbols_batch, encode_symbols_batch
    kw = {"backend": args.backend}
    g = torch.Generator().manual_seed(1)
    sym = torch.randint(0, L, (B,) + shape, generator=g)
    sym[torch.rand(sym.shape, generator=g) < args.zero_frac] = 0
    sym = sym.to(dev)
    waves = len(_wave_order(*shape, pc.context_size() // 2))
    t = {"eb": [], "es": [], "db": [], "ds": []}
    for i in range(args.warmup + args.runs):
        datas, eb = timed(lambda: encode_symbols_batch(pc, centers, sym,
                                                       **kw), dev)
        seq, es = timed(lambda: [encode_symbols(pc, centers, s, **kw)
                                 for s in sym], dev)
        if datas != seq:
            sys.exit(f"bench_codec: batched streams differ at {shape}, B={B}")
        out, db = timed(lambda: decode_symbols_batch(pc, centers, datas,
                                                     shape, **kw), dev)
        outs, ds = timed(lambda: [decode_symbols(pc, centers, d, shape, **kw)
                                  for d in datas], dev)
        if not (torch.equal(out, sym) and torch.equal(torch.stack(outs), sym)):
            sys.exit(f"bench_codec: roundtrip failed at {shape}, B={B}")
        if i >= args.warmup:
            for k, v in zip(("eb", "es", "db", "ds"), (eb, es, db, ds)):
                t[k].append(v)
    med = {k: statistics.median(v) for k, v in t.items()}
    out = {"backend": args.backend, "device": dev.type, "shape": list(shape),
           "batch": B, "symbols_per_image": sym[0].numel(),
           "zero_frac": args.zero_frac, "runs": args.runs,
           "warmup": args.warmup, "waves": waves,
           "stream_bytes": sum(len(d) for d in datas),
           "encode_batched_ms": stats(t["eb"]),
           "encode_sequential_ms": stats(t["es"]),
           "encode_ratio": round(med["es"] / med["eb"], 3),
           "encode_ms_per_image": round(med["eb"] / B, 3),
           "decode_batched_ms": stats(t["db"]),
           "decode_sequential_ms": stats(t["ds"]),
           "decode_ratio": round(med["ds"] / med["db"], 3),
           "decode_ms_per_image": round(med["db"] / B, 3)}
    if dev.type != "cuda":
        out["threads"] = torch.get_num_threads()
    else:
        # from the schedule, not counted: what the C++ loops issue
        out["encode_launches_computed"] = {"batched": 2, "sequential": 2 * B}
        out["decode_launches_computed"] = {"batched": 1 + 2 * waves,
                                           "sequential": B * (1 + 2 * waves)}
    print(json.dumps(out), flush=True)


def bench_ragged(args, dev, pc, centers, L, shapes):
    """One JSON line: one ragged call against one batched call per group of
    equal shapes and against one call per volume."""
    from dsin_amd.coding import (decode_symbols_batch, decode_symbols_ragged,
                                 encode_symbols_batch, encode_symbols_ragged)
    kw = {"backend": args.backend}
    g = torch.Generator().manual_seed(1)
    syms = []
    for shape in shapes:
        s = torch.randint(0, L, shape, generator=g)
        s[torch.rand(shape, generator=g) < args.zero_frac] = 0
        syms.append(s.to(dev))
    groups = {}
    for i, shape in enumerate(shapes):
        groups.setdefault(shape, []).append(i)
    stacked = {shape: torch.stack([syms[i] for i in idx])
               for shape, idx in groups.items()}
    pad = pc.context_size() // 2
    wave_t = {shape: {25 * w[0][0] + 5 * w[0][1] + w[0][2]
                      for w in _wave_order(*shape, pad)} for shape in groups}
    merged = len(set().union(*wave_t.values()))

    def enc_grouped():
        out = [None] * len(shapes)
        for shape, idx in groups.items():
            for i, d in zip(idx, encode_symbols_batch(pc, centers,
                                                      stacked[shape], **kw)):
                out[i] = d
        return out

    def dec_grouped(datas):
        out = [None] * len(shapes)
        for shape, idx in groups.items():
            dec = decode_symbols_batch(pc, centers, [datas[i] for i in idx],
                                       shape, **kw)
            for i, o in zip(idx, dec):
                out[i] = o
        return out

    names = ("ragged", "grouped", "single")
    t = {f"{op}_{n}": [] for op in ("encode", "decode") for n in names}
    for it in range(args.warmup + args.runs):
        enc = [timed(lambda: encode_symbols_ragged(pc, centers, syms, **kw),
                     dev),
               timed(enc_grouped, dev),
               timed(lambda: [encode_symbols(pc, centers, s, **kw)
                              for s in syms], dev)]
        datas = enc[0][0]
        if not (enc[1][0] == datas and enc[2][0] == datas):
            sys.exit(f"bench_codec: ragged streams differ at {shapes}")
        dec = [timed(lambda: decode_symbols_ragged(pc, centers, datas, shapes,
                                                   **kw), dev),
               timed(lambda: dec_grouped(datas), dev),
               timed(lambda: [decode_symbols(pc, centers, d, sh, **kw)
                              for d, sh in zip(datas, shapes)], dev)]
        for outs, _ in dec:
            if not all(torch.equal(o, s) for o, s in zip(outs, syms)):
                sys.exit(f"bench_codec: ragged roundtrip failed at {shapes}")
        if it >= args.warmup:
            for n, (_, te), (_, td) in zip(names, enc, dec):
                t[f"encode_{n}"].append(te)
                t[f"decode_{n}"].append(td)
    med = {k: statistics.median(v) for k, v in t.items()}
    out = {"backend": args.backend, "device": dev.type,
           "ragged_shapes": [list(s) for s in shapes],
           "images": len(shapes), "size_groups": len(groups),
           "symbols": sum(s.numel() for s in syms),
           "zero_frac": args.zero_frac, "runs": args.runs,
           "warmup": args.warmup, "merged_waves": merged,
           "stream_bytes": sum(len(d) for d in datas)}
    for k, v in t.items():
        out[k + "_ms"] = stats(v)
    for op in ("encode", "decode"):
        for n in names[1:]:
            out[f"{op}_{n}_over_ragged"] = round(
                med[f"{op}_{n}"] / med[f"{op}_ragged"], 3)
    if dev.type != "cuda":
        out["threads"] = torch.get_num_threads()
    else:
        # from the schedules, not counted: what the C++ loops issue
        out["encode_launches_computed"] = {
            "ragged": 2, "grouped": 2 * len(groups), "single": 2 * len(shapes)}
        out["decode_launches_computed"] = {
            "ragged": 1 + 2 * merged,
            "grouped": sum(1 + 2 * len(wave_t[s]) for s in groups),
            "single": sum(1 + 2 * len(wave_t[s]) for s in shapes)}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", default="hip",
                    choices=["hip", "torch", "portable"])
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default="32x8x12,32x40x120")
    ap.add_argument("--zero-frac", type=float, default=0.5)
    ap.add_argument("--batch", default=None,
                    help="comma-separated batch sizes: time one batched call "
                         "against B sequential single-image calls")
    ap.add_argument("--ragged", default=None,
                    help="comma-separated CxHxW volumes of one mixed batch: "
                         "time one ragged call against one batched call per "
                         "size group and one call per volume")
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

    if args.ragged:
        if args.backend == "torch":
            sys.exit("bench_codec: --ragged times the hip and portable "
                     "backends (torch loops over the images)")
        bench_ragged(args, dev, pc, centers, L,
                     [tuple(int(s) for s in spec.split("x"))
                      for spec in args.ragged.split(",")])
        return

    for spec in args.shapes.split(","):
        shape = tuple(int(s) for s in spec.split("x"))
        if args.batch:
            if args.backend == "torch":
                sys.exit("bench_codec: --batch times the hip and portable "
                         "backends (torch loops over the images)")
            for B in (int(b) for b in args.batch.split(",")):
                bench_batch(args, dev, pc, centers, L, shape, B)
            continue
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
