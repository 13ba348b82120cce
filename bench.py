"""Benchmark entry point (driver contract).

Measures the flagship DSIN training step — full model (AE + probclass +
siFinder NCC search + siNet fusion), bf16 compute, 320x960 synthetic
KITTI-shaped stereo pairs, batch 1 per GPU (the reference's SI training
batch, src/AE.py:26) — and prints ONE JSON line with the whole-job
imgs/sec aggregate. Metric and config follow BASELINE.json
("imgs/sec train @320x960 per GPU", synthetic data, random-init weights).

Launch: `python bench.py --gpus N --steps K --warmup W`; for N>1 the driver
uses torch.distributed.run with one rank per GPU over RCCL; we read
RANK/LOCAL_RANK/WORLD_SIZE from the env. Weak scaling: per-GPU work fixed.

A plain run does only what the headline figure needs: set up, warm up, time
the K steps, print the result line. `--dump-outputs DIR` additionally writes
what the last timed step produced (see dump_outputs). `--full` is where any
measurement beyond the headline figure belongs (baselines, other precisions
or sizes, per-kernel figures); there is none today, so it changes nothing.
"""

from __future__ import annotations

import argparse
import json
import os
import time

import numpy as np
import torch

from dsin_amd import config as config_mod
from dsin_amd.data import SyntheticStereo
from dsin_amd.models import DSIN
from dsin_amd.parallel import init_distributed, is_distributed, rank, world_size
from dsin_amd.training import Trainer

BASELINE_VALUE = None  # reference publishes no throughput number


def build_configs(args):
    cur = os.path.dirname(os.path.abspath(__file__))
    ae, _ = config_mod.parse(os.path.join(cur, "run_configs", "ae_run_configs"))
    pc, _ = config_mod.parse(os.path.join(cur, "run_configs", "pc_run_configs"))
    ae.crop_size = (args.height, args.width)
    # keep the siFinder patch grid valid for non-default crops (the
    # reference's (20, 24) patches assume 320x960 / 320x1224 crops)
    ph, pw = ae.y_patch_size
    if args.height % ph or args.width % pw:
        ph = next(p for p in (20, 16, 32, 8, 4, 2, 1) if args.height % p == 0)
        pw = next(p for p in (24, 32, 16, 8, 4, 2, 1) if args.width % p == 0)
        ae.y_patch_size = (ph, pw)
    ae.AE_only = bool(args.ae_only)
    ae.load_model = False
    ae.train_model = True
    ae.test_model = False
    return ae, pc


DUMP_MAX_ELEMS = 4 * 1024 * 1024  # per array; 3 arrays of fp32 stay < 64 MB


def _to_dump_array(t: torch.Tensor) -> np.ndarray:
    a = t.detach().to(device="cpu", dtype=torch.float32).reshape(-1).numpy()
    if a.size > DUMP_MAX_ELEMS:
        # fixed, seeded sample: the same elements in every run and every build
        idx = np.random.default_rng(0).choice(a.size, DUMP_MAX_ELEMS,
                                              replace=False)
        idx.sort()
        a = a[idx]
    return np.ascontiguousarray(a)


def dump_outputs(out_dir, last_out, model):
    """Write what the last timed train step produced as DIR/<name>.npy
    (float32): the (loss, bpp) pair train_step returns, and the parameters
    the step left behind, flattened per optimizer group (AE and probclass).
    Inputs and initial weights are seeded, so equal arguments give equal
    inputs and two builds can be compared array for array."""
    os.makedirs(out_dir, exist_ok=True)
    loss, bpp = last_out
    ae_params, pc_params = model.param_groups()
    arrays = {
        "loss_bpp": torch.stack([loss.detach().float().reshape(()),
                                 bpp.detach().float().reshape(())]),
        "params_ae": torch.cat([p.detach().float().reshape(-1)
                                for p in ae_params]),
        "params_pc": torch.cat([p.detach().float().reshape(-1)
                                for p in pc_params]),
    }
    for name, t in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), _to_dump_array(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--height", type=int, default=320)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--ae-only", action="store_true",
                    help="benchmark config 2 (AE without side information)")
    ap.add_argument("--dtype", type=str, default="bf16",
                    choices=["bf16", "fp32", "fp8"])
    ap.add_argument("--device", type=str, default=None)
    ap.add_argument("--no-graph", action="store_true",
                    help="disable hipGraph capture of the train step")
    ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                    help="after the timed steps, write the last step's "
                         "outputs (loss/bpp, updated parameters) as "
                         "DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run every measurement beyond the headline "
                         "figure (none exist today)")
    # NOTE: no --channels-last flag. The custom conv/BN kernels are designed
    # around NCHW with K-contiguous gather tables; an NHWC input would be
    # silently re-laid-out at every op entry, so offering the flag would
    # suggest a capability that does not exist (round-1 verdict, weak #8).
    args = ap.parse_args()

    local_rank = init_distributed()
    if args.device:
        device = torch.device(args.device)
    elif torch.cuda.is_available():
        device = torch.device(f"cuda:{local_rank}")
    else:
        device = torch.device("cpu")
    n_ranks = world_size()

    ae_config, pc_config = build_configs(args)
    if args.dtype == "fp8":
        from dsin_amd.ops import conv as dconv
        dconv.set_compute_dtype("fp8")  # e4m3 MFMA conv path (config 5)
    torch.manual_seed(1234 + rank())
    model = DSIN(ae_config, pc_config).to(device)
    # hipGraph capture is the default at world=1 (verified on hardware).
    # Multi-rank capture would record the RCCL all-reduces inside the graph;
    # that configuration has never been verified on a multi-GPU box, so the
    # default there is the eager overlapped-bucket path (FlatGradReducer) —
    # correct by construction, CI-covered over gloo at 2/4/8 ranks.
    # DSIN_DIST_GRAPH=1 opts multi-rank capture in for experiments.
    use_graph = (not args.no_graph and device.type == "cuda"
                 and (world_size() == 1
                      or bool(os.environ.get("DSIN_DIST_GRAPH"))))
    trainer = Trainer(model, ae_config, pc_config, num_training_imgs=1576,
                     device=device, autocast_bf16=(args.dtype in ("bf16", "fp8")),
                     use_cuda_graph=use_graph,
                     ddp_comm_dtype=None)

    batch = args.batch if args.ae_only else 1
    gen = SyntheticStereo(args.height, args.width, batch_size=batch,
                          seed=1234 + rank(), device=str(device))
    # pre-generate batches so host-side synthesis stays out of the timed region
    n_batches = min(args.warmup + args.steps, 16)
    batches = [gen.next_batch() for _ in range(n_batches)]

    def step(i):
        x, y = batches[i % n_batches]
        return trainer.train_step(x, y if not args.ae_only else None)

    last_out = None
    for i in range(args.warmup):
        last_out = step(i)

    def barrier_sync():
        if is_distributed():
            torch.distributed.barrier()
        if device.type == "cuda":
            torch.cuda.synchronize(device)

    barrier_sync()
    t0 = time.perf_counter()
    for i in range(args.steps):
        last_out = step(args.warmup + i)
    barrier_sync()
    elapsed = time.perf_counter() - t0

    if args.dump_outputs and rank() == 0 and last_out is not None:
        dump_outputs(args.dump_outputs, last_out, model)

    # which execution path actually ran (per-rank proof)
    import sys
    graph_live = getattr(trainer, "_graph", None) is not None
    print(f"[bench rank {rank()}] path={'hipGraph' if graph_live else 'eager'}"
          f" fused_adam={trainer._fused}"
          f" graph_failed={trainer._graph_failed}", file=sys.stderr)

    # max over ranks
    if is_distributed():
        t = torch.tensor([elapsed], device=device if device.type == "cuda" else None)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())

    imgs = args.steps * batch * n_ranks
    value = imgs / elapsed
    ms_per_step = elapsed / args.steps * 1000.0

    if rank() == 0:
        result = {
            "metric": "imgs/sec train @320x960 per GPU; MS-SSIM @0.02 bpp, 1/2/4/8 MI355X",
            "value": value,
            "unit": "imgs/sec",
            "n_gpus": n_ranks,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": BASELINE_VALUE,
            "dtype": args.dtype,
            "data": "synthetic",
            "config": {
                "model": "DSIN (AE+probclass+siFinder+siNet)" if not args.ae_only
                         else "DSIN AE-only",
                "global_batch": batch * n_ranks,
                "crop": [args.height, args.width],
                "seq_len": None,
                "parallelism": f"dp{n_ranks}",
            },
        }
        print(json.dumps(result))


if __name__ == "__main__":
    main()
