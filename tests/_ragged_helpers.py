"""Shared by test_ragged_codec.py (CPU) and test_gpu_ragged_codec.py: the
batches of symbol volumes of different shapes and the checks both devices
repeat. The oracle throughout is the single-image path (encode_symbols /
decode_symbols / ops.pc_freqs), never the ragged code itself, and every
comparison is exact."""

import struct

import numpy as np
import pytest
import torch

import _batch_helpers as H
import _portable_helpers as P
from dsin_amd import ops
from dsin_amd.coding import (decode_symbols, decode_symbols_ragged,
                             encode_symbols, encode_symbols_batch,
                             encode_symbols_ragged)
from dsin_amd.coding import bitstream as bs

# (1,1,1) finishes in wave 0; (2,1,7) is idle for waves 7..24 and comes back
# (an empty segment in the middle of a live image); two different C; a
# repeated shape; the batch ends long after its smallest member does.
MIX = [(3, 5, 6), (1, 1, 1), (2, 1, 7), (3, 10, 12), (3, 5, 6)]
ORDERS = {"mix": MIX, "reversed": MIX[::-1], "rotated": MIX[2:] + MIX[:2]}
ONE = [(2, 1, 7)]
ALT17 = [(3, 5, 6) if b % 2 == 0 else (2, 1, 7) for b in range(17)]
BATCHES = dict(ORDERS, one=ONE, alt17=ALT17)
LK = H.LK
PAD = P.PAD


def volumes(shapes, L, seed=0):
    """One volume per shape with mixed_symbols' mix: image b is all zeros,
    uniform random or 90 % zeros in turn (a batch of one gets the random
    one)."""
    B = len(shapes)
    return [H.mixed_symbols(s, L, B, seed=seed)[b]
            for b, s in enumerate(shapes)]


_SINGLES = {}


def singles(key, pc, centers, symbols, backend):
    """The single-image streams of a batch, computed once per key and
    shared by the tests that compare against them."""
    if key not in _SINGLES:
        _SINGLES[key] = [encode_symbols(pc, centers, s, backend=backend)
                         for s in symbols]
    return _SINGLES[key]


def layout(pc, centers, symbols):
    """-> (flat value buffer, descriptor rows, items (n, 4) image after
    image in wave order, the per-image (q_pad, positions)), built from the
    single-image helpers on the CPU."""
    qs, desc, items, per = [], [], [], []
    q_off = s_off = 0
    for b, sym in enumerate(symbols):
        C, Hh, W = sym.shape
        q = P.q_pad_of(pc, centers, sym)
        pos = P.positions((C, Hh, W))
        desc.append((C, Hh, W, q_off, s_off))
        items.append(torch.cat([torch.full((pos.shape[0], 1), b,
                                           dtype=torch.int32), pos], dim=1))
        qs.append(q.reshape(-1))
        per.append((q, pos))
        q_off += q.numel()
        s_off += sym.numel()
    return torch.cat(qs), desc, torch.cat(items), per


def check_tables(pc_cpu, centers_cpu, pc, shapes, portable, device):
    """Test 1: rows of ops.pc_freqs_ragged == ops.pc_freqs of each image
    alone, logits bit for bit. pc_cpu / centers_cpu build the buffers, pc
    lives on `device`."""
    L = centers_cpu.numel()
    symbols = volumes(shapes, L, seed=4)
    q, desc, items, per = layout(pc_cpu, centers_cpu, symbols)
    # shuffled: a row depends on its item alone, not on the order
    perm = torch.randperm(items.shape[0],
                          generator=torch.Generator().manual_seed(3))
    lg, fr = ops.pc_freqs_ragged(pc, q.to(device), desc,
                                 items[perm].to(device), portable=portable)
    n = items.shape[0]
    assert lg.shape == (n, L) and fr.shape == (n, L)
    assert lg.device.type == device.type
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(n)
    lg, fr = lg.cpu()[inv], fr.cpu()[inv]
    at = 0
    for b, (qb, pos) in enumerate(per):
        lg1, fr1 = ops.pc_freqs(pc, qb.to(device), pos.to(device),
                                portable=portable)
        m = pos.shape[0]
        assert torch.equal(P.bits(lg[at:at + m]), P.bits(lg1.cpu())), b
        assert torch.equal(fr[at:at + m], fr1.cpu()), b
        at += m
    assert at == n


def check_bytes(key, pc, centers, symbols, backend):
    """Test 2: ragged stream b == the single-image stream of image b."""
    got = encode_symbols_ragged(pc, centers, symbols, backend=backend)
    want = singles(key, pc, centers, symbols, backend)
    assert isinstance(got, list) and len(got) == len(symbols)
    for b, data in enumerate(got):
        assert isinstance(data, bytes)
        assert data == want[b], b
    return got


def check_roundtrip(key, pc, centers, symbols, backend):
    """Test 3: ragged decode of ragged streams and of single-image streams;
    decode_symbols opens each ragged stream."""
    shapes = [tuple(s.shape) for s in symbols]
    ragged = encode_symbols_ragged(pc, centers, symbols, backend=backend)
    for datas in (ragged, singles(key, pc, centers, symbols, backend)):
        out = decode_symbols_ragged(pc, centers, datas, shapes,
                                    backend=backend)
        assert isinstance(out, list) and len(out) == len(symbols)
        for b, (o, s) in enumerate(zip(out, symbols)):
            assert o.dtype == torch.int64 and o.device == s.device
            assert o.shape == s.shape and torch.equal(o, s), b
    for b, data in enumerate(ragged):
        out = decode_symbols(pc, centers, data, shapes[b], backend=backend)
        assert torch.equal(out, symbols[b]), b


def check_stream_bounds(pc, centers, symbols, backend):
    """Test 4: the payload of a middle image truncated to 0 bytes, 3 bytes
    and half its length decodes as decode_symbols decodes those bytes; every
    other image is untouched."""
    shapes = [tuple(s.shape) for s in symbols]
    datas = encode_symbols_ragged(pc, centers, symbols, backend=backend)
    mid = len(symbols) // 2
    assert 0 < mid < len(symbols) - 1
    for cut in (0, 3, len(datas[mid]) // 2):
        short = list(datas)
        short[mid] = datas[mid][:cut]
        out = decode_symbols_ragged(pc, centers, short, shapes,
                                    backend=backend)
        want = decode_symbols(pc, centers, short[mid], shapes[mid],
                              backend=backend)
        for b, (o, s) in enumerate(zip(out, symbols)):
            assert torch.equal(o, want if b == mid else s), (cut, b)


def check_equal_sizes(pc, centers, backend):
    """Test 6: a ragged call on B volumes of one shape gives the bytes of
    encode_symbols_batch."""
    L = centers.numel()
    for shape, B in (((3, 5, 6), 3), ((2, 1, 7), 4)):
        sym = H.mixed_symbols(shape, L, B, seed=6).to(centers.device)
        assert encode_symbols_ragged(pc, centers, list(sym), backend=backend) \
            == encode_symbols_batch(pc, centers, sym, backend=backend)


def check_symbol_level_rejected(pc, centers, backend, monkeypatch):
    """Test 7, symbol level: ValueError, and the extension is not touched."""
    L = centers.numel()
    dev = centers.device
    sym = P.symbols_of((2, 1, 7), L, seed=1).to(dev)
    data = encode_symbols(pc, centers, sym, backend=backend)

    def boom(*a, **k):
        raise AssertionError("the extension was touched by a bad request")
    monkeypatch.setattr(ops, "_require_ext", boom)
    with pytest.raises(ValueError):
        encode_symbols_ragged(pc, centers, [], backend=backend)
    with pytest.raises(ValueError):  # a 4-D volume
        encode_symbols_ragged(pc, centers, [sym, sym[None]], backend=backend)
    with pytest.raises(ValueError):  # a 2-D volume
        encode_symbols_ragged(pc, centers, [sym[0]], backend=backend)
    with pytest.raises(ValueError):
        decode_symbols_ragged(pc, centers, [], [], backend=backend)
    with pytest.raises(ValueError):  # two streams, one shape
        decode_symbols_ragged(pc, centers, [data, data], [(2, 1, 7)],
                              backend=backend)
    with pytest.raises(ValueError):  # a shape that is not (C, H, W)
        decode_symbols_ragged(pc, centers, [data], [(1, 2, 1, 7)],
                              backend=backend)
    if backend == "torch":
        return
    portable = backend == "portable"
    with pytest.raises(ValueError):  # an empty volume
        decode_symbols_ragged(pc, centers, [data], [(2, 0, 7)],
                              backend=backend)
    # the ops wrappers: descriptor table, items, segment table, payloads
    n1, n2 = 6 * 9 * 15, 5 * 9 * 9
    q = torch.zeros(n1 + n2, device=dev)
    good = [(2, 1, 7, 0, 0), (1, 1, 1, n1, 14)]
    items = torch.tensor([[0, 0, 0, 0], [1, 0, 0, 0]], dtype=torch.int32,
                         device=dev)
    for desc in ([],                                        # no image
                 [(2, 1, 7, 0)],                            # short row
                 [(0, 1, 7, 0, 0), good[1]],                # C = 0
                 [good[0], (1, 1, 1, n1 + 1, 14)],          # past the buffer
                 [good[0], (1, 1, 1, n1 - 1, 14)],          # volumes overlap
                 [good[0], (1, 1, 1, n1, 13)],              # symbols overlap
                 [good[0], (1, 1, 1, n1, 15)]):             # past the output
        with pytest.raises(ValueError):
            ops.pc_freqs_ragged(pc, q, desc, items, portable=portable)
    with pytest.raises(ValueError):  # a 2-D value buffer
        ops.pc_freqs_ragged(pc, q[None], good, items, portable=portable)
    with pytest.raises(ValueError):  # items are (n, 4)
        ops.pc_freqs_ragged(pc, q, good, items[:, :3], portable=portable)
    s2 = torch.zeros(2, dtype=torch.int64, device=dev)
    for starts in ([0, 2], [0, 1, 1], [1, 1, 2], [0, 2, 1]):
        with pytest.raises(ValueError):
            ops.pc_encode_ragged(pc, q, good, items, starts, s2,
                                 portable=portable)
    with pytest.raises(ValueError):  # one symbol for two items
        ops.pc_encode_ragged(pc, q, good, items, [0, 1, 2], s2[:1],
                             portable=portable)
    for seg in ([0, 2], [0, 1, 2, 2], [0, 1, 1], [1, 1, 2], [0, 2, 1, 2, 2]):
        with pytest.raises(ValueError):
            ops.pc_decode_ragged(pc, q, good, items, seg, [data, data],
                                 centers, portable=portable)
    with pytest.raises(ValueError):  # one stream for two images
        ops.pc_decode_ragged(pc, q, good, items, [0, 1, 2], [data], centers,
                             portable=portable)
    assert not q.any()  # nothing was decoded into the buffer


def check_archive():
    """Test 7, the multi-image container."""
    datas = [b"DSIN" + bytes(range(40)), b"", b"\x00" * 7]
    for names in (None, ["a.png", "", "ü/猫"]):
        blob = bs.pack_archive(datas, names)
        assert blob[:4] == b"DSNA" and blob[4] == 1
        assert struct.unpack_from("<I", blob, 5)[0] == 3
        got, got_names = bs.unpack_archive(blob)
        assert got == datas
        assert got_names == (names or ["", "", ""])
    assert bs.unpack_archive(bs.pack_archive([])) == ([], [])
    blob = bs.pack_archive(datas, ["a", "b", "c"])
    table_end = 9 + 3 * 6 + 3
    for bad in (b"DSNX" + blob[4:],            # magic
                blob[:4] + b"\x02" + blob[5:],  # version
                blob[:3],                       # shorter than the header
                blob[:9 + 4],                   # table cut inside an entry
                blob[:9 + 6],                   # table cut inside a name
                blob[:table_end + 10],          # first container cut
                blob[:-1],                      # last container cut
                blob + b"\x00"):                # trailing bytes
        with pytest.raises(ValueError):
            bs.unpack_archive(bad)
    with pytest.raises(ValueError):  # two containers, one name
        bs.pack_archive(datas[:2], ["a"])


SIZES = [(64, 96), (32, 48), (64, 96)]


def images_many(device):
    g = torch.Generator().manual_seed(1)
    xs = [torch.rand(3, *s, generator=g) * 255 for s in SIZES]
    ys = [(x + torch.randn(x.shape, generator=g) * 4).clamp(0, 255)
          for x in xs]
    return [x.to(device) for x in xs], [y.to(device) for y in ys]


def check_compress_many(model, backend, other_backend_id, monkeypatch):
    """Test 8 and the image-level part of test 7. The images are 64x96,
    32x48 and 64x96 again on the model's device."""
    from dsin_amd.coding import compress, compress_many, decompress_many
    centers = model.encoder.quantizer.centers.detach()
    xs, ys = images_many(centers.device)
    datas = compress_many(model, xs, backend=backend)
    assert isinstance(datas, list) and len(datas) == 3
    name = backend or bs.model_backend(model)
    groups = [[0, 2], [1]]
    with torch.no_grad():
        sym_g = [model.encoder(torch.stack([xs[i] for i in g])).symbols
                 for g in groups]
        want_g = [model.decoder(centers.float()[s]) for s in sym_g]
    for g, sym, want in zip(groups, sym_g, want_g):
        for j, i in enumerate(g):
            bid, shape, L, crc, payload = bs.parse_container(datas[i])
            assert bid == bs.BACKEND_IDS[name]
            assert shape == tuple(sym.shape[1:]) and L == centers.numel()
            assert shape[1:] == (SIZES[i][0] // 8, SIZES[i][1] // 8)
            assert crc == bs.probclass_crc(model)
            out = decode_symbols(model.probclass, centers, payload, shape,
                                 backend=name)
            assert torch.equal(out, sym[j]), i
    # not asserted (the encoder's conv and BN kernels are not known to be
    # bit-invariant to the batch size): do single-image containers match?
    same = [datas[i] == compress(model, xs[i], backend=backend)
            for i in range(3)]
    print(f"compress_many[b] == compress(x[b]) on {centers.device.type}: "
          f"{same}")

    outs_y = decompress_many(model, datas, ys)
    assert isinstance(outs_y, list) and len(outs_y) == 3
    # without side images; the torch codec is slow (a network call per wave
    # and image), so there only the small image goes through a second time
    again = [1] if name == "torch" else [0, 1, 2]
    outs = dict(zip(again, decompress_many(model, [datas[i] for i in again])))
    assert len(outs) == len(again)
    for g, want in zip(groups, want_g):
        for j, i in enumerate(g):
            x_dec, x_si = outs_y[i]
            assert torch.equal(x_dec, want[j:j + 1]), i
            assert x_si.shape == (1, 3) + SIZES[i]
            if i in outs:
                x_dec2, none = outs[i]
                assert none is None
                assert torch.equal(x_dec2, want[j:j + 1]), i
    # an archive carries the containers through
    back, names = bs.unpack_archive(bs.pack_archive(datas, ["a", "b", "c"]))
    assert back == datas and names == ["a", "b", "c"]

    def boom(*a, **k):  # no network may run, nothing may be coded
        raise AssertionError("work started despite a bad request")
    from dsin_amd.ops import conv as _conv
    monkeypatch.setattr(bs, "decode_symbols_ragged", boom)
    monkeypatch.setattr(bs, "encode_symbols_ragged", boom)
    monkeypatch.setattr(_conv, "begin_step", boom)
    monkeypatch.setattr(model.encoder, "forward", boom)
    monkeypatch.setattr(model.decoder, "forward", boom)
    monkeypatch.setattr(model, "create_y_dec", boom)
    crc = struct.unpack_from("<I", datas[1], 14)[0]
    for bad in (H.rebuild(datas[1], backend=other_backend_id),
                H.rebuild(datas[1], crc=crc ^ 0x100),
                H.rebuild(datas[1], C=31),
                H.rebuild(datas[1], L=centers.numel() + 1),
                H.rebuild(datas[1], version=2),
                datas[1][:-1]):
        with pytest.raises(ValueError):
            decompress_many(model, [datas[0], bad, datas[2]])
    with pytest.raises(ValueError):
        decompress_many(model, [])
    with pytest.raises(ValueError):  # three streams, two side images
        decompress_many(model, datas, ys[:2])
    with pytest.raises(ValueError):  # side image 1 has the size of image 0
        decompress_many(model, datas, [ys[0], ys[0], ys[2]])
    with pytest.raises(ValueError):
        compress_many(model, [], backend=backend)
    with pytest.raises(ValueError):  # a batched tensor is not an image
        compress_many(model, [xs[0][None]], backend=backend)
    with pytest.raises(ValueError):
        compress_many(model, xs, backend="nope")
