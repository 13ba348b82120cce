"""Image <-> bytes: the container around the entropy-coded symbol volume.

    data = compress(model, x)               # x: (3,H,W) or (1,3,H,W), 0..255
    x_dec, x_with_si = decompress(model, data, y)

Both run the model in eval mode, as ``DSIN.reconstruct`` does, and produce
the same ``x_dec`` / ``x_with_si`` as ``reconstruct`` under the same autocast
setting: the decoder input is ``centers[symbols]``, which is what the
quantizer's ``qbar`` equals.

Container (little-endian, 22-byte header, then the payload):

    4s  magic  b"DSIN"
    B   version (1)
    B   backend id (0 torch, 1 hip, 2 portable)
    H   C   bottleneck channels
    H   Hb  bottleneck height
    H   Wb  bottleneck width
    H   L   number of centers
    I   CRC32 of the probclass weights, biases and the centers (fp32 bytes)
    I   payload length in bytes
    ..  payload: range-coded symbols in wave order

Without a ``backend`` argument ``compress`` picks hip when the model is on a
GPU and torch on the CPU. Those two do NOT decode each other's streams: the
hip kernels evaluate the context model in fp32 with their own ``expf`` and
scale tables by 65536-L, the torch path uses the torch convs (bf16 panels on
a GPU) and a 65536 scale, so the frequency tables differ. A stream records
its backend and ``decompress`` refuses one it cannot reproduce: id 0 on a
GPU model, id 1 on a CPU model.

``compress(model, x, backend="portable")`` writes id 2, the stream to use
when encoder and decoder are different machines. Its tables come from
correctly rounded fp32 operations and integer arithmetic only
(``ops/csrc/pc_model.h``, specified in ``docs/KERNELS.md``), which a gfx950
kernel and the extension's host build evaluate to the same bits, so a
portable stream written on a GPU decodes on a CPU model and the reverse.
``decompress`` accepts id 2 on any device. (Only the symbols are portable:
the decoder network's ``x_dec`` still differs in the last bits between a GPU
and a CPU.)

Batches: ``compress_batch(model, x)`` takes ``x`` of shape (B,3,H,W) and
returns a list of B byte strings, each a complete version-1 container of one
image that ``decompress`` opens on its own (the archive below holds several
of them in one file). ``decompress_batch(model, datas, y)`` takes such a list (from
``compress_batch`` or from B ``compress`` calls) and returns batched
``x_dec`` / ``x_with_si``. The containers of one batch must agree in backend
id, ``(C, Hb, Wb)`` and ``L``. With the hip and portable backends the B
symbol volumes are entropy-coded together by the batched kernels
(``encode_symbols_batch`` / ``decode_symbols_batch``): the images share one
wave loop and each has a range coder of its own.

Images of different sizes: ``compress_many(model, xs)`` takes a list of
(3,H_b,W_b) images whose sizes may all differ and returns one ordinary
version-1 single-image container per image, in input order;
``decompress_many(model, datas, ys)`` takes such containers, which may
differ in ``(Hb, Wb)`` but must agree in backend id, ``C`` and ``L``, and
returns one ``(x_dec, x_with_si)`` pair per image. With the hip and portable
backends all symbol volumes go through one ragged call
(``encode_symbols_ragged`` / ``decode_symbols_ragged``): the images walk one
wave counter and the smaller ones finish early. The networks run once per
size group.

Archive, the multi-image container (little-endian), written by
``pack_archive(datas, names)`` and read by ``unpack_archive(data)``:

    4s  magic  b"DSNA"
    B   version (1)
    I   count  number of entries
    per entry:
      I   container length in bytes
      H   name length in bytes
      ..  name, UTF-8 (may be empty)
    ..  the containers back to back, in entry order

Each container is a complete version-1 single-image stream. A bad magic or
version, a truncated table, a truncated container and trailing bytes are
ValueErrors.
"""

from __future__ import annotations

import struct
import zlib
from typing import List, Optional, Sequence, Tuple

import torch

from .entropy import (decode_symbols, decode_symbols_batch,
                      decode_symbols_ragged, encode_symbols_batch,
                      encode_symbols_ragged)

MAGIC = b"DSIN"
VERSION = 1
BACKEND_IDS = {"torch": 0, "hip": 1, "portable": 2}
_HEADER = struct.Struct("<4sBBHHHHII")
HEADER_SIZE = _HEADER.size
ARCHIVE_MAGIC = b"DSNA"
ARCHIVE_VERSION = 1
_ARCHIVE_HEADER = struct.Struct("<4sBI")
_ARCHIVE_ENTRY = struct.Struct("<IH")


def model_backend(model) -> str:
    """hip on a GPU, torch on the CPU."""
    dev = model.encoder.quantizer.centers.device
    return "hip" if dev.type == "cuda" else "torch"


def probclass_crc(model) -> int:
    """CRC32 over the fp32 bytes of every probclass weight and bias (layer
    order conv0, res_conv1, res_conv2, conv2) and of the centers."""
    pc = model.probclass
    crc = 0
    tensors = []
    for m in (pc.conv0, pc.res_conv1, pc.res_conv2, pc.conv2):
        tensors += [m.weight, m.bias]
    tensors.append(model.encoder.quantizer.centers)
    for t in tensors:
        raw = t.detach().float().cpu().contiguous().numpy().tobytes()
        crc = zlib.crc32(raw, crc)
    return crc & 0xFFFFFFFF


def pack_container(backend: str, shape, L: int, crc: int,
                   payload: bytes) -> bytes:
    C, Hb, Wb = (int(v) for v in shape)
    if max(C, Hb, Wb, L) > 0xFFFF:
        raise ValueError(f"container: dimension too large in {shape}, L={L}")
    return _HEADER.pack(MAGIC, VERSION, BACKEND_IDS[backend], C, Hb, Wb,
                        int(L), crc, len(payload)) + payload


def parse_container(data: bytes):
    """-> (backend id, (C, Hb, Wb), L, crc, payload). ValueError on a bad
    magic or version or a truncated stream."""
    if len(data) < HEADER_SIZE:
        raise ValueError(f"container: {len(data)} bytes is shorter than the "
                         f"{HEADER_SIZE}-byte header")
    magic, ver, bid, C, Hb, Wb, L, crc, n = _HEADER.unpack_from(data)
    if magic != MAGIC:
        raise ValueError(f"container: bad magic {magic!r}")
    if ver != VERSION:
        raise ValueError(f"container: version {ver}, this build reads "
                         f"{VERSION}")
    if bid not in BACKEND_IDS.values():
        raise ValueError(f"container: unknown backend id {bid}")
    if min(C, Hb, Wb, L) < 1:
        raise ValueError(f"container: empty volume {(C, Hb, Wb)}, L={L}")
    payload = data[HEADER_SIZE:HEADER_SIZE + n]
    if len(payload) != n:
        raise ValueError(f"container: payload truncated, header says {n} "
                         f"bytes, {len(payload)} present")
    return bid, (C, Hb, Wb), L, crc, payload


def _as_batch(x: torch.Tensor, what: str) -> torch.Tensor:
    if x.dim() == 3:
        x = x.unsqueeze(0)
    if x.dim() != 4 or x.shape[0] != 1 or x.shape[1] != 3:
        raise ValueError(f"{what} must be (3,H,W) or (1,3,H,W), got "
                         f"{tuple(x.shape)}")
    return x


@torch.no_grad()
def compress(model, x: torch.Tensor, backend: Optional[str] = None) -> bytes:
    """Encode one image to a self-describing byte string: compress_batch of
    a batch of one. backend None is the model's own (hip on a GPU, torch on
    the CPU); "portable" writes a stream that any device decodes."""
    return compress_batch(model, _as_batch(x, "x"), backend)[0]


def _check_header(model, bid: int, shape, L: int, crc: int) -> str:
    """The checks decompress makes on a parsed header; -> the backend that
    decodes the stream on this model."""
    backend = model_backend(model)
    if bid == BACKEND_IDS["portable"]:
        backend = "portable"
    if bid != BACKEND_IDS[backend]:
        names = {v: k for k, v in BACKEND_IDS.items()}
        raise ValueError(
            f"container: stream was written by the {names[bid]} backend, "
            f"this model runs the {backend} backend (hip on a GPU, torch on "
            f"the CPU); the two do not decode each other's streams")
    centers = model.encoder.quantizer.centers.detach()
    if L != centers.numel():
        raise ValueError(f"container: stream has L={L}, the model has "
                         f"{centers.numel()} centers")
    if shape[0] != int(model.ae_config.num_chan_bn):
        raise ValueError(f"container: stream has {shape[0]} channels, the "
                         f"model has {model.ae_config.num_chan_bn}")
    if crc != probclass_crc(model):
        raise ValueError("container: CRC mismatch, the stream was written "
                         "with other probclass weights or centers")
    return backend


def _reconstruct(model, symbols: torch.Tensor, y: Optional[torch.Tensor]
                 ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Decoded symbols (B,C,Hb,Wb) and an optional side image (B,3,H,W) ->
    (x_dec, x_with_si): the decoder on centers[symbols], then the
    side-information search and the SI network."""
    from .. import ops
    centers = model.encoder.quantizer.centers.detach()
    x_dec = model.decoder(centers.float()[symbols])
    if y is None or model.ae_only:
        return x_dec, None
    y_dec = model.create_y_dec(y)
    y_syn = model.sifinder(x_dec.float(), y.float(), y_dec.float())
    cat = torch.cat([ops.kitti_normalize(x_dec),
                     ops.kitti_normalize(y_syn.to(x_dec.dtype))], dim=1)
    return x_dec, ops.kitti_denormalize(model.sinet(cat))


@torch.no_grad()
def decompress(model, data: bytes, y: Optional[torch.Tensor] = None
               ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """-> (x_dec, x_with_si). x_with_si is None without a side image y or
    for an AE-only model. Every header problem is a ValueError raised
    before any network or kernel runs."""
    from ..ops import conv as _conv
    bid, shape, L, crc, payload = parse_container(data)
    backend = _check_header(model, bid, shape, L, crc)
    centers = model.encoder.quantizer.centers.detach()
    if y is not None:
        y = _as_batch(y, "y")
    _conv.begin_step()
    model.eval()
    symbols = decode_symbols(model.probclass, centers, payload, shape,
                             device=centers.device, backend=backend)
    return _reconstruct(model, symbols[None], y)


def _as_images(x: torch.Tensor, what: str) -> torch.Tensor:
    if x.dim() != 4 or x.shape[0] < 1 or x.shape[1] != 3:
        raise ValueError(f"{what} must be (B,3,H,W) with B >= 1, got "
                         f"{tuple(x.shape)}")
    return x


@torch.no_grad()
def compress_batch(model, x: torch.Tensor, backend: Optional[str] = None
                   ) -> List[bytes]:
    """Encode B images (B,3,H,W) to B self-describing byte strings, each a
    single-image container that decompress opens. One encoder pass over the
    batch and one encode_symbols_batch call."""
    if backend is not None and backend not in BACKEND_IDS:
        raise ValueError(f"backend must be one of {tuple(BACKEND_IDS)}, got "
                         f"{backend!r}")
    from ..ops import conv as _conv
    x = _as_images(x, "x")
    _conv.begin_step()
    model.eval()
    symbols = model.encoder(x).symbols
    centers = model.encoder.quantizer.centers.detach()
    if backend is None:
        backend = model_backend(model)
    payloads = encode_symbols_batch(model.probclass, centers, symbols,
                                    backend=backend)
    crc = probclass_crc(model)
    return [pack_container(backend, symbols.shape[1:], centers.numel(), crc,
                           p) for p in payloads]


@torch.no_grad()
def decompress_batch(model, datas: Sequence[bytes],
                     y: Optional[torch.Tensor] = None
                     ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """-> (x_dec (B,3,H,W), x_with_si or None) from B single-image
    containers; y is (B,3,H,W) when given. Every header problem, containers
    that differ in backend id, (C, Hb, Wb) or L, and a y of another batch
    size are ValueErrors raised before any network or kernel runs."""
    from ..ops import conv as _conv
    datas = list(datas)
    if len(datas) < 1:
        raise ValueError("decompress_batch: empty batch")
    parsed = [parse_container(d) for d in datas]
    bid, shape, L = parsed[0][:3]
    backend = _check_header(model, *parsed[0][:4])
    for i, (bid_i, shape_i, L_i, crc_i, _) in enumerate(parsed[1:], 1):
        _check_header(model, bid_i, shape_i, L_i, crc_i)
        if (bid_i, shape_i, L_i) != (bid, shape, L):
            raise ValueError(
                f"container {i}: backend id {bid_i}, volume {shape_i}, "
                f"L={L_i} differ from container 0 (backend id {bid}, volume "
                f"{shape}, L={L}); one batch holds one kind of stream")
    if y is not None:
        y = _as_images(y, "y")
        if y.shape[0] != len(datas):
            raise ValueError(f"decompress_batch: {len(datas)} streams but y "
                             f"holds {y.shape[0]} images")
    centers = model.encoder.quantizer.centers.detach()
    _conv.begin_step()
    model.eval()
    symbols = decode_symbols_batch(model.probclass, centers,
                                   [p[4] for p in parsed], shape,
                                   device=centers.device, backend=backend)
    return _reconstruct(model, symbols, y)


def _size_groups(keys) -> List[List[int]]:
    """Indices grouped by equal key, groups in order of first appearance."""
    groups = {}
    for i, k in enumerate(keys):
        groups.setdefault(k, []).append(i)
    return list(groups.values())


@torch.no_grad()
def compress_many(model, xs: Sequence[torch.Tensor],
                  backend: Optional[str] = None) -> List[bytes]:
    """Encode images (3,H_b,W_b) whose sizes may differ to single-image
    containers, in input order. One encoder pass per distinct size (the
    images of a size stacked, sizes in order of first appearance) and one
    encode_symbols_ragged call over all symbol volumes."""
    if backend is not None and backend not in BACKEND_IDS:
        raise ValueError(f"backend must be one of {tuple(BACKEND_IDS)}, got "
                         f"{backend!r}")
    from ..ops import conv as _conv
    xs = list(xs)
    if len(xs) < 1:
        raise ValueError("compress_many: empty list")
    for i, x in enumerate(xs):
        if x.dim() != 3 or x.shape[0] != 3:
            raise ValueError(f"compress_many: image {i} must be (3,H,W), got "
                             f"{tuple(x.shape)}")
    _conv.begin_step()
    model.eval()
    symbols: List[Optional[torch.Tensor]] = [None] * len(xs)
    for group in _size_groups(tuple(x.shape) for x in xs):
        sym = model.encoder(torch.stack([xs[i] for i in group])).symbols
        for i, s in zip(group, sym):
            symbols[i] = s
    centers = model.encoder.quantizer.centers.detach()
    if backend is None:
        backend = model_backend(model)
    payloads = encode_symbols_ragged(model.probclass, centers, symbols,
                                     backend=backend)
    crc = probclass_crc(model)
    return [pack_container(backend, s.shape, centers.numel(), crc, p)
            for s, p in zip(symbols, payloads)]


@torch.no_grad()
def decompress_many(model, datas: Sequence[bytes],
                    ys: Optional[Sequence[torch.Tensor]] = None
                    ) -> List[Tuple[torch.Tensor, Optional[torch.Tensor]]]:
    """-> one (x_dec (1,3,H_b,W_b), x_with_si or None) per container; ys,
    when given, holds one side image (3,H_b,W_b) per container. The
    containers may differ in (Hb, Wb); backend id, C, L and CRC must agree
    with the model and with each other. Every header problem, a ys of
    another length and a side image of another size than its container are
    ValueErrors raised before any network or kernel runs. One
    decode_symbols_ragged call, then the networks once per size group."""
    from ..ops import conv as _conv
    datas = list(datas)
    if len(datas) < 1:
        raise ValueError("decompress_many: empty list")
    parsed = [parse_container(d) for d in datas]
    bid, _, L = parsed[0][:3]
    backend = _check_header(model, *parsed[0][:4])
    for i, (bid_i, shape_i, L_i, crc_i, _) in enumerate(parsed[1:], 1):
        _check_header(model, bid_i, shape_i, L_i, crc_i)
        if (bid_i, L_i) != (bid, L):
            raise ValueError(
                f"container {i}: backend id {bid_i}, L={L_i} differ from "
                f"container 0 (backend id {bid}, L={L}); one call holds one "
                f"kind of stream")
    if ys is not None:
        ys = list(ys)
        if len(ys) != len(datas):
            raise ValueError(f"decompress_many: {len(datas)} streams but "
                             f"{len(ys)} side images")
        for i, (y, p) in enumerate(zip(ys, parsed)):
            want = (3, p[1][1] * 8, p[1][2] * 8)
            if tuple(y.shape) != want:
                raise ValueError(f"decompress_many: side image {i} must be "
                                 f"{want}, got {tuple(y.shape)}")
    centers = model.encoder.quantizer.centers.detach()
    _conv.begin_step()
    model.eval()
    shapes = [p[1] for p in parsed]
    symbols = decode_symbols_ragged(model.probclass, centers,
                                    [p[4] for p in parsed], shapes,
                                    device=centers.device, backend=backend)
    out: List[Optional[Tuple[torch.Tensor, Optional[torch.Tensor]]]] = \
        [None] * len(datas)
    for group in _size_groups(shapes):
        y = None if ys is None else torch.stack([ys[i] for i in group])
        x_dec, x_si = _reconstruct(
            model, torch.stack([symbols[i] for i in group]), y)
        for j, i in enumerate(group):
            out[i] = (x_dec[j:j + 1],
                      None if x_si is None else x_si[j:j + 1])
    return out


def pack_archive(datas: Sequence[bytes],
                 names: Optional[Sequence[str]] = None) -> bytes:
    """Containers (and optional names, one per container) -> one archive
    (layout in the module docstring)."""
    datas = [bytes(d) for d in datas]
    names = [""] * len(datas) if names is None else list(names)
    if len(names) != len(datas):
        raise ValueError(f"archive: {len(datas)} containers but {len(names)} "
                         f"names")
    table = [_ARCHIVE_HEADER.pack(ARCHIVE_MAGIC, ARCHIVE_VERSION, len(datas))]
    for d, name in zip(datas, names):
        raw = name.encode("utf-8")
        if len(raw) > 0xFFFF or len(d) > 0xFFFFFFFF:
            raise ValueError(f"archive: entry {name!r} is too large")
        table.append(_ARCHIVE_ENTRY.pack(len(d), len(raw)) + raw)
    return b"".join(table + datas)


def unpack_archive(data: bytes) -> Tuple[List[bytes], List[str]]:
    """-> (containers, names). ValueError on a bad magic or version, a
    truncated table, a truncated container or trailing bytes."""
    if len(data) < _ARCHIVE_HEADER.size:
        raise ValueError(f"archive: {len(data)} bytes is shorter than the "
                         f"{_ARCHIVE_HEADER.size}-byte header")
    magic, ver, count = _ARCHIVE_HEADER.unpack_from(data)
    if magic != ARCHIVE_MAGIC:
        raise ValueError(f"archive: bad magic {magic!r}")
    if ver != ARCHIVE_VERSION:
        raise ValueError(f"archive: version {ver}, this build reads "
                         f"{ARCHIVE_VERSION}")
    pos = _ARCHIVE_HEADER.size
    sizes, names = [], []
    for i in range(count):
        if len(data) - pos < _ARCHIVE_ENTRY.size:
            raise ValueError(f"archive: table truncated at entry {i} of "
                             f"{count}")
        n, m = _ARCHIVE_ENTRY.unpack_from(data, pos)
        pos += _ARCHIVE_ENTRY.size
        if len(data) - pos < m:
            raise ValueError(f"archive: table truncated in the name of entry "
                             f"{i}")
        try:
            names.append(data[pos:pos + m].decode("utf-8"))
        except UnicodeDecodeError:
            raise ValueError(f"archive: the name of entry {i} is not UTF-8")
        pos += m
        sizes.append(n)
    datas = []
    for i, n in enumerate(sizes):
        if len(data) - pos < n:
            raise ValueError(f"archive: container {i} truncated, the table "
                             f"says {n} bytes, {len(data) - pos} present")
        datas.append(bytes(data[pos:pos + n]))
        pos += n
    if pos != len(data):
        raise ValueError(f"archive: {len(data) - pos} trailing bytes")
    return datas, names
