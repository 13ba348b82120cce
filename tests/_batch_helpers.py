"""Shared by test_batch_codec.py (CPU) and test_gpu_batch_codec.py: the
mixed batches of symbol volumes and the checks both devices repeat."""

import os
import struct

import pytest
import torch

import _portable_helpers as P
from dsin_amd import config as cm
from dsin_amd.coding import (decode_symbols, decode_symbols_batch,
                             encode_symbols, encode_symbols_batch)
from dsin_amd.coding import bitstream as bs

SHAPES = [(3, 5, 6), (1, 1, 1), (2, 1, 7), (3, 10, 12)]
BATCHES = [1, 3, 17]
LK = [(2, 8), (6, 24), (16, 24)]


def mixed_symbols(shape, L, B, seed=0):
    """(B, C, H, W): image b is all zeros, uniform random or 90 % zeros in
    turn (B = 1 gets the random one), so the streams of a batch differ in
    length and the coders' positions diverge."""
    out = []
    for b in range(B):
        kind = (b + 1) % 3 if B > 1 else 1
        if kind == 1:
            out.append(P.symbols_of(shape, L, seed=seed + b))
        elif kind == 2:
            out.append(P.symbols_of(shape, L, seed=seed + b, zero_frac=0.9))
        else:
            out.append(torch.zeros(shape, dtype=torch.int64))
    return torch.stack(out)


def check_bytes(pc, centers, symbols, backend):
    """Test 2: batched stream b == the single-image stream of image b."""
    got = encode_symbols_batch(pc, centers, symbols, backend=backend)
    assert isinstance(got, list) and len(got) == symbols.shape[0]
    for b, data in enumerate(got):
        assert isinstance(data, bytes)
        assert data == encode_symbols(pc, centers, symbols[b],
                                      backend=backend), b
    return got


def check_roundtrip(pc, centers, symbols, backend):
    """Test 3: batched decode of batched streams and of single-image
    streams, single-image decode of each batched stream."""
    shape = tuple(symbols.shape[1:])
    batched = encode_symbols_batch(pc, centers, symbols, backend=backend)
    singles = [encode_symbols(pc, centers, s, backend=backend)
               for s in symbols]
    for datas in (batched, singles):
        out = decode_symbols_batch(pc, centers, datas, shape, backend=backend)
        assert out.dtype == torch.int64 and out.device == symbols.device
        assert torch.equal(out, symbols)
    for b, data in enumerate(batched):
        out = decode_symbols(pc, centers, data, shape, backend=backend)
        assert torch.equal(out, symbols[b]), b


def check_stream_bounds(pc, centers, symbols, backend):
    """Test 4: the middle payload of three truncated to 0 bytes, 3 bytes and
    half its length decodes as decode_symbols decodes those bytes (zeros
    past the end, never the next image's bytes); its neighbours are
    untouched."""
    assert symbols.shape[0] == 3
    shape = tuple(symbols.shape[1:])
    datas = encode_symbols_batch(pc, centers, symbols, backend=backend)
    for cut in (0, 3, len(datas[1]) // 2):
        short = datas[1][:cut]
        out = decode_symbols_batch(pc, centers, [datas[0], short, datas[2]],
                                   shape, backend=backend)
        want = decode_symbols(pc, centers, short, shape, backend=backend)
        assert torch.equal(out[1], want), cut
        assert torch.equal(out[0], symbols[0]), cut
        assert torch.equal(out[2], symbols[2]), cut


def check_rejected(pc, centers, backend):
    """Test 6, the symbol-level part: B = 0 and a 3-D volume."""
    L = centers.numel()
    sym = P.symbols_of((2, 1, 7), L, seed=1).to(centers.device)
    with pytest.raises(ValueError):
        encode_symbols_batch(pc, centers, sym[None][:0], backend=backend)
    with pytest.raises(ValueError):
        encode_symbols_batch(pc, centers, sym, backend=backend)
    with pytest.raises(ValueError):
        decode_symbols_batch(pc, centers, [], (2, 1, 7), backend=backend)


def small_dsin(crop=(64, 96)):
    """Seeded DSIN at small_ae_config (crop 64x96 -> bottleneck (32,8,12))
    or a smaller crop."""
    from dsin_amd.models import DSIN
    cfg = os.path.join(P.HERE, "..", "run_configs")
    ae, _ = cm.parse(os.path.join(cfg, "ae_run_configs"))
    pcc, _ = cm.parse(os.path.join(cfg, "pc_run_configs"))
    ae.crop_size = crop
    ae.y_patch_size = (16, 16)
    torch.manual_seed(0)
    return DSIN(ae, pcc).eval()


def images(B, crop, device):
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, 3, *crop, generator=g) * 255
    y = (x + torch.randn(x.shape, generator=g) * 4).clamp(0, 255)
    return x.to(device), y.to(device)


def rebuild(data, **kw):
    f = list(struct.unpack_from("<4sBBHHHHII", data))
    names = ["magic", "version", "backend", "C", "Hb", "Wb", "L", "crc", "n"]
    for k, v in kw.items():
        f[names.index(k)] = v
    return struct.pack("<4sBBHHHHII", *f) + data[bs.HEADER_SIZE:]


def check_compress_batch(model, x, y, backend, other_backend_id, monkeypatch):
    """Test 7. x, y: (2, 3, H, W) on the model's device."""
    from dsin_amd.coding import compress, compress_batch, decompress_batch
    B, _, H, W = x.shape
    datas = compress_batch(model, x, backend=backend)
    assert isinstance(datas, list) and len(datas) == B
    centers = model.encoder.quantizer.centers.detach()
    with torch.no_grad():
        symbols = model.encoder(x).symbols
    name = backend or bs.model_backend(model)
    for b, data in enumerate(datas):
        bid, shape, L, crc, payload = bs.parse_container(data)
        assert bid == bs.BACKEND_IDS[name]
        assert shape == tuple(symbols.shape[1:]) and L == centers.numel()
        assert crc == bs.probclass_crc(model)
        out = decode_symbols(model.probclass, centers, payload, shape,
                             backend=name)
        assert torch.equal(out, symbols[b]), b
    # not asserted (the encoder's conv and BN kernels are not known to be
    # bit-invariant to the batch size): do single-image containers match?
    same = [datas[b] == compress(model, x[b:b + 1], backend=backend)
            for b in range(B)]
    print(f"compress_batch[b] == compress(x[b]) on {x.device.type}: {same}")

    x_dec, none = decompress_batch(model, datas)
    assert none is None
    with torch.no_grad():
        want = model.decoder(centers.float()[symbols])
    assert torch.equal(x_dec, want)
    x_dec2, x_si = decompress_batch(model, datas, y)
    assert torch.equal(x_dec2, want)
    assert x_si.shape == (B, 3, H, W)

    def boom(*a, **k):  # no network may run, nothing may be decoded
        raise AssertionError("work started despite a bad request")
    from dsin_amd.ops import conv as _conv
    monkeypatch.setattr(bs, "decode_symbols_batch", boom)
    monkeypatch.setattr(_conv, "begin_step", boom)
    monkeypatch.setattr(model.decoder, "forward", boom)
    monkeypatch.setattr(model, "create_y_dec", boom)
    wb = bs.parse_container(datas[1])[1][2]
    crc = struct.unpack_from("<I", datas[1], 14)[0]
    for bad in (rebuild(datas[1], Wb=wb + 1),
                rebuild(datas[1], backend=other_backend_id),
                rebuild(datas[1], crc=crc ^ 0x100)):
        with pytest.raises(ValueError):
            decompress_batch(model, [datas[0], bad])
    with pytest.raises(ValueError):  # len(datas) against the batch of y
        decompress_batch(model, datas, y[:1])
    with pytest.raises(ValueError):
        decompress_batch(model, [])
    with pytest.raises(ValueError):
        compress_batch(model, x[0], backend=backend)
