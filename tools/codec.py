"""Compress a PNG to a .dsin byte stream and back.

    python tools/codec.py compress   [--backend portable] <checkpoint> <x.png> <out.dsin>
    python tools/codec.py decompress <checkpoint> <in.dsin> [--side y.png] <out.png>

    python tools/codec.py compress-batch   [--backend portable] --out-dir DIR <checkpoint> <a.png> <b.png> ..
    python tools/codec.py decompress-batch --out-dir DIR [--side ya.png --side yb.png ..] <checkpoint> <a.dsin> <b.dsin> ..

    python tools/codec.py compress-many   [--backend portable] --out FILE.dsna <checkpoint> <a.png> <b.png> ..
    python tools/codec.py decompress-many --out-dir DIR [--side ya.png --side yb.png ..] <checkpoint> FILE.dsna

compress-many takes images of any sizes (each a multiple of 8 in both
dimensions) and codes them in one compress_many call: one encoder pass per
distinct size and one ragged entropy-coder call over all of them. It writes
one archive FILE.dsna (magic DSNA, see dsin_amd/coding/bitstream.py) that
holds an ordinary single-image stream per image together with the image's
file name. decompress-many opens such an archive, decodes all streams in one
decompress_many call and writes DIR/<name>.png per image (one --side per
image, in the archive's order, or none). The model is size-agnostic apart
from the side-information patch: with --side the patch (--patch HxW, default
from the config) must tile every image of the archive, otherwise the tool
exits with a message that names the image.

compress-batch takes several images of one size and codes them in one
compress_batch call (the entropy coder runs them as one batch on the GPU),
writing DIR/<name>.dsin per image, each an ordinary single-image stream that
decompress opens; decompress-batch takes several such streams of one size,
decodes them in one decompress_batch call and writes DIR/<name>.png per
stream (one --side per stream, in order, or none).

<checkpoint> is a directory written by training (it holds model.pt). The
model runs on the GPU when there is one (hip codec backend) and on the CPU
otherwise (torch backend); a stream is decoded by the backend that wrote
it (see dsin_amd/coding/bitstream.py). compress --backend portable writes a
stream that decodes on a GPU and on the CPU alike; decompress needs no flag,
the stream names its backend. With --side the decoder also runs
the side-information search and fusion and writes x_with_si; without it,
x_dec. Image height and width must be multiples of 8, and with --side they
must tile by the patch size (--patch HxW, default from the config or the
largest of 20/16/8.. x 24/32/16.. that divides the image).
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from dsin_amd import config as config_mod
from dsin_amd.coding import (compress, compress_batch, compress_many,
                             decompress, decompress_batch, decompress_many,
                             pack_archive, unpack_archive)
from dsin_amd.coding.bitstream import parse_container
from dsin_amd.data.png import read_png, write_png
from dsin_amd.models import DSIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_image(path: str, device) -> torch.Tensor:
    img = read_png(path)
    if img.shape[2] == 1:
        img = np.repeat(img, 3, axis=2)
    img = img[:, :, :3]
    if img.shape[0] % 8 or img.shape[1] % 8:
        sys.exit(f"{path}: {img.shape[0]}x{img.shape[1]} is not a multiple "
                 f"of 8 in both dimensions")
    return torch.from_numpy(img.copy()).permute(2, 0, 1).float().to(device)


def save_image(path: str, x: torch.Tensor) -> None:
    img = x.detach().float().clamp(0, 255).round().to(torch.uint8)
    write_png(path, img[0].permute(1, 2, 0).cpu().numpy())


def build_model(args, height: int, width: int, device) -> DSIN:
    ae, _ = config_mod.parse(args.ae_config)
    pc, _ = config_mod.parse(args.pc_config)
    ae.crop_size = (height, width)
    if args.patch:
        ph, pw = (int(v) for v in args.patch.split("x"))
    else:
        ph, pw = ae.y_patch_size
        if height % ph or width % pw:
            ph = next(p for p in (20, 16, 32, 8, 4, 2, 1) if height % p == 0)
            pw = next(p for p in (24, 32, 16, 8, 4, 2, 1) if width % p == 0)
    ae.y_patch_size = (ph, pw)
    model = DSIN(ae, pc)
    blob = torch.load(os.path.join(args.checkpoint, "model.pt"),
                      map_location="cpu", weights_only=False)
    for name, mod in model.state_groups().items():
        if name not in blob:
            sys.exit(f"{args.checkpoint}: checkpoint has no {name!r} group")
        mod.load_state_dict(blob[name])
    return model.to(device).eval()


def out_paths(out_dir: str, paths, ext: str):
    names = [os.path.splitext(os.path.basename(p))[0] + ext for p in paths]
    if len(set(names)) != len(names):
        sys.exit("inputs of one batch need different file names")
    os.makedirs(out_dir, exist_ok=True)
    return [os.path.join(out_dir, n) for n in names]


def run_batch(args, device, cast) -> None:
    """All inputs in one compress_batch / decompress_batch call."""
    if args.cmd == "compress-batch":
        xs = [load_image(p, device) for p in args.paths]
        if len(set(tuple(x.shape) for x in xs)) != 1:
            sys.exit("images of one batch must have the same size")
        outs = out_paths(args.out_dir, args.paths, ".dsin")
        x = torch.stack(xs)
        model = build_model(args, x.shape[2], x.shape[3], device)
        with cast:
            datas = compress_batch(model, x, backend=args.backend)
        for path, data in zip(outs, datas):
            with open(path, "wb") as f:
                f.write(data)
            bpp = 8.0 * len(data) / (x.shape[2] * x.shape[3])
            print(f"{path}: {len(data)} bytes, {bpp:.4f} bpp")
        return
    datas = []
    for p in args.paths:
        with open(p, "rb") as f:
            datas.append(f.read())
    try:
        _, (_, hb, wb), _, _, _ = parse_container(datas[0])
    except ValueError as e:
        sys.exit(f"{args.paths[0]}: {e}")
    if args.side and len(args.side) != len(datas):
        sys.exit(f"{len(datas)} streams need {len(datas)} --side images, "
                 f"got {len(args.side)}")
    outs = out_paths(args.out_dir, args.paths, ".png")
    model = build_model(args, hb * 8, wb * 8, device)
    y = (torch.stack([load_image(p, device) for p in args.side])
         if args.side else None)
    try:
        with cast:
            x_dec, x_si = decompress_batch(model, datas, y)
    except ValueError as e:
        sys.exit(f"{args.out_dir}: {e}")
    res = x_si if x_si is not None else x_dec
    for b, path in enumerate(outs):
        save_image(path, res[b:b + 1])
        print(f"{path}: {hb * 8}x{wb * 8}, "
              f"{'x_with_si' if x_si is not None else 'x_dec'}")


def run_many(args, device, cast) -> None:
    """Images of different sizes: one compress_many / decompress_many call,
    one archive."""
    if args.cmd == "compress-many":
        xs = [load_image(p, device) for p in args.paths]
        names = [os.path.basename(p) for p in args.paths]
        if len(set(os.path.splitext(n)[0] for n in names)) != len(names):
            sys.exit("inputs of one archive need different file names")
        model = build_model(args, xs[0].shape[1], xs[0].shape[2], device)
        with cast:
            datas = compress_many(model, xs, backend=args.backend)
        with open(args.out, "wb") as f:
            f.write(pack_archive(datas, names))
        for name, x, data in zip(names, xs, datas):
            bpp = 8.0 * len(data) / (x.shape[1] * x.shape[2])
            print(f"{name}: {x.shape[1]}x{x.shape[2]}, {len(data)} bytes, "
                  f"{bpp:.4f} bpp")
        print(f"{args.out}: {len(datas)} images, "
              f"{os.path.getsize(args.out)} bytes")
        return
    with open(args.archive, "rb") as f:
        blob = f.read()
    try:
        datas, names = unpack_archive(blob)
        sizes = [tuple(8 * v for v in parse_container(d)[1][1:])
                 for d in datas]
    except ValueError as e:
        sys.exit(f"{args.archive}: {e}")
    if not datas:
        sys.exit(f"{args.archive}: the archive holds no image")
    names = [n or f"image{i:04d}" for i, n in enumerate(names)]
    if args.side and len(args.side) != len(datas):
        sys.exit(f"{len(datas)} images need {len(datas)} --side images, got "
                 f"{len(args.side)}")
    outs = out_paths(args.out_dir, names, ".png")
    model = build_model(args, sizes[0][0], sizes[0][1], device)
    ys = None
    if args.side:
        ph, pw = model.ae_config.y_patch_size
        for name, (h, w) in zip(names, sizes):
            if h % ph or w % pw:
                sys.exit(f"{name}: the {ph}x{pw} side-information patch does "
                         f"not tile its {h}x{w} pixels; choose --patch so "
                         f"that it tiles every image of the archive")
        ys = [load_image(p, device) for p in args.side]
    try:
        with cast:
            res = decompress_many(model, datas, ys)
    except ValueError as e:
        sys.exit(f"{args.archive}: {e}")
    for path, (h, w), (x_dec, x_si) in zip(outs, sizes, res):
        save_image(path, x_si if x_si is not None else x_dec)
        print(f"{path}: {h}x{w}, "
              f"{'x_with_si' if x_si is not None else 'x_dec'}")


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ae-config", default=os.path.join(
        ROOT, "run_configs", "ae_run_configs"))
    ap.add_argument("--pc-config", default=os.path.join(
        ROOT, "run_configs", "pc_run_configs"))
    ap.add_argument("--device", default=None)
    ap.add_argument("--bf16", action="store_true",
                    help="bf16 autocast for the autoencoder (GPU); use the "
                         "same setting on both sides")
    ap.add_argument("--patch", default=None, help="side-info patch size HxW")
    sub = ap.add_subparsers(dest="cmd", required=True)
    c = sub.add_parser("compress")
    c.add_argument("--backend", default=None,
                   choices=["torch", "hip", "portable"],
                   help="codec backend (default: hip on a GPU, torch on the "
                        "CPU); portable streams decode on any device")
    c.add_argument("checkpoint")
    c.add_argument("image")
    c.add_argument("out")
    d = sub.add_parser("decompress")
    d.add_argument("checkpoint")
    d.add_argument("stream")
    d.add_argument("--side", default=None, help="side image y.png")
    d.add_argument("out")
    cb = sub.add_parser("compress-batch",
                        help="code several images of one size as one batch")
    cb.add_argument("--backend", default=None,
                    choices=["torch", "hip", "portable"])
    cb.add_argument("--out-dir", required=True,
                    help="receives one <name>.dsin per image")
    cb.add_argument("checkpoint")
    cb.add_argument("paths", nargs="+", metavar="image")
    db = sub.add_parser("decompress-batch",
                        help="decode several streams of one size as one batch")
    db.add_argument("--out-dir", required=True,
                    help="receives one <name>.png per stream")
    db.add_argument("--side", action="append", default=None,
                    help="side image y.png, once per stream and in their "
                         "order, or not at all")
    db.add_argument("checkpoint")
    db.add_argument("paths", nargs="+", metavar="stream")
    cm_ = sub.add_parser("compress-many",
                         help="code images of any sizes into one archive")
    cm_.add_argument("--backend", default=None,
                     choices=["torch", "hip", "portable"])
    cm_.add_argument("--out", required=True, help="the archive FILE.dsna")
    cm_.add_argument("checkpoint")
    cm_.add_argument("paths", nargs="+", metavar="image")
    dm = sub.add_parser("decompress-many",
                        help="decode every image of an archive")
    dm.add_argument("--out-dir", required=True,
                    help="receives one <name>.png per image")
    dm.add_argument("--side", action="append", default=None,
                    help="side image y.png, once per image and in the "
                         "archive's order, or not at all")
    dm.add_argument("checkpoint")
    dm.add_argument("archive")
    args = ap.parse_args()

    device = torch.device(args.device or (
        "cuda:0" if torch.cuda.is_available() else "cpu"))
    cast = torch.autocast("cuda", dtype=torch.bfloat16, cache_enabled=False,
                          enabled=args.bf16 and device.type == "cuda")
    if args.cmd.endswith("-many"):
        run_many(args, device, cast)
    elif args.cmd.endswith("-batch"):
        run_batch(args, device, cast)
    elif args.cmd == "compress":
        x = load_image(args.image, device)
        model = build_model(args, x.shape[1], x.shape[2], device)
        with cast:
            data = compress(model, x, backend=args.backend)
        with open(args.out, "wb") as f:
            f.write(data)
        bpp = 8.0 * len(data) / (x.shape[1] * x.shape[2])
        print(f"{args.out}: {len(data)} bytes, {bpp:.4f} bpp")
    else:
        with open(args.stream, "rb") as f:
            data = f.read()
        try:
            _, (_, hb, wb), _, _, _ = parse_container(data)
        except ValueError as e:
            sys.exit(f"{args.stream}: {e}")
        model = build_model(args, hb * 8, wb * 8, device)
        y = load_image(args.side, device) if args.side else None
        try:
            with cast:
                x_dec, x_si = decompress(model, data, y)
        except ValueError as e:
            sys.exit(f"{args.stream}: {e}")
        save_image(args.out, x_si if x_si is not None else x_dec)
        print(f"{args.out}: {hb * 8}x{wb * 8}, "
              f"{'x_with_si' if x_si is not None else 'x_dec'}")


if __name__ == "__main__":
    main()
