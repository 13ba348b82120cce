"""Batched entropy codec on the CPU: encode_symbols_batch /
decode_symbols_batch through the portable backend's host build and through
the torch backend, and compress_batch / decompress_batch on a CPU model.
Every comparison is exact: stream b of a batch is the single-image stream of
image b, and either decoder reads either."""

import pytest
import torch

import _batch_helpers as H
import _portable_helpers as P
from dsin_amd import ops
from dsin_amd.coding import (decode_symbols_batch, encode_symbols,
                             encode_symbols_batch)

@pytest.fixture(params=[False, True], ids=["fma", "libm"])
def host_path(request):
    """Both host paths of the portable model: run-time choice and forced
    library fmaf."""
    prev = ops.pc_host_force_libm(request.param)
    yield request.param
    ops.pc_host_force_libm(prev)


@pytest.mark.parametrize("L,k", H.LK)
def test_portable_freqs_independent_of_the_batch(L, k):
    """Host build: batched logits and tables [b] are bitwise those of image
    b alone."""
    pc, centers = P.make_pc(L, k, seed=1), P.centers_of(L)
    shape = (3, 5, 6)
    symbols = H.mixed_symbols(shape, L, 3, seed=4)
    q = torch.stack([P.q_pad_of(pc, centers, s) for s in symbols])
    pos = P.positions(shape)
    lg, fr = ops.pc_freqs_batch(pc, q, pos, portable=True)
    assert lg.shape == (3, pos.shape[0], L) and fr.shape == lg.shape
    for b in range(3):
        lg1, fr1 = ops.pc_freqs(pc, q[b], pos, portable=True)
        assert torch.equal(P.bits(lg[b]), P.bits(lg1))
        assert torch.equal(fr[b], fr1)


@pytest.mark.parametrize("B", H.BATCHES)
@pytest.mark.parametrize("L,k", H.LK)
def test_portable_bytes(L, k, B):
    pc, centers = P.make_pc(L, k, seed=1), P.centers_of(L)
    for shape in H.SHAPES:
        H.check_bytes(pc, centers, H.mixed_symbols(shape, L, B, seed=B),
                      "portable")


@pytest.mark.parametrize("L,k", H.LK)
def test_portable_roundtrip_and_cross_decoding(L, k):
    pc, centers = P.make_pc(L, k, seed=2), P.centers_of(L)
    for shape in H.SHAPES:
        for B in (1, 3):
            H.check_roundtrip(pc, centers,
                              H.mixed_symbols(shape, L, B, seed=7),
                              "portable")


def test_portable_roundtrip_saturated():
    """Table entries of 1: the streams of a batch differ widely in length."""
    L = 6
    pc, centers = P.saturate(P.make_pc(L, seed=4)), P.centers_of(L)
    symbols = H.mixed_symbols((3, 10, 12), L, 3, seed=8)
    datas = H.check_bytes(pc, centers, symbols, "portable")
    assert len(set(len(d) for d in datas)) > 1
    H.check_roundtrip(pc, centers, symbols, "portable")


@pytest.mark.parametrize("L,k", H.LK)
def test_portable_stream_bounds(L, k):
    pc, centers = P.make_pc(L, k, seed=3), P.centers_of(L)
    for shape in H.SHAPES:
        H.check_stream_bounds(pc, centers,
                              H.mixed_symbols(shape, L, 3, seed=5),
                              "portable")


def test_portable_golden_stream_in_a_batch(host_path):
    """The golden symbols at index 1 of 3 give the golden stream there."""
    pc, centers, symbols, stream = P.load_golden()
    batch = torch.stack([P.symbols_of((3, 5, 6), 6, seed=1), symbols,
                         torch.zeros(3, 5, 6, dtype=torch.int64)])
    datas = encode_symbols_batch(pc, centers, batch, backend="portable")
    assert datas[1] == stream
    out = decode_symbols_batch(pc, centers, datas, (3, 5, 6),
                               backend="portable")
    assert torch.equal(out, batch)


def test_portable_rejected_requests():
    H.check_rejected(P.make_pc(6, 8), P.centers_of(6), "portable")
    pc, centers = P.make_pc(6, 8), P.centers_of(6)
    q = torch.zeros(2, 6, 9, 15)
    pos = P.positions((2, 1, 7))
    with pytest.raises(ValueError):  # one stream for a batch of two
        ops.pc_decode_batch(pc, q, pos, [0, pos.shape[0]], [b"\0" * 4],
                            centers, portable=True)
    with pytest.raises(ValueError):  # a 3-D buffer is the single-image call
        ops.pc_freqs_batch(pc, q[0], pos, portable=True)
    many = torch.zeros(1, 6, 9, 15).expand(ops.PC_MAX_BATCH + 1, -1, -1, -1)
    with pytest.raises(ValueError):  # above the images one call codes
        ops.pc_freqs_batch(pc, many, pos, portable=True)
    with pytest.raises(ValueError):  # hip needs GPU tensors
        encode_symbols_batch(pc, centers, torch.zeros(1, 2, 1, 7).long(),
                             backend="hip")


@pytest.mark.parametrize("shape", [(2, 1, 7), (1, 1, 1)])
def test_torch_backend_bytes_and_roundtrip(shape):
    """The torch backend loops over the images: same bytes, same symbols."""
    L = 6
    pc, centers = P.make_pc(L, 8, seed=1), P.centers_of(L)
    symbols = H.mixed_symbols(shape, L, 3, seed=2)
    H.check_bytes(pc, centers, symbols, "torch")
    H.check_roundtrip(pc, centers, symbols, "torch")
    one = H.mixed_symbols(shape, L, 1, seed=3)
    assert encode_symbols_batch(pc, centers, one) == [
        encode_symbols(pc, centers, one[0])]  # default backend = torch


def test_torch_backend_rejected_requests():
    H.check_rejected(P.make_pc(6, 8), P.centers_of(6), "torch")


def test_compress_batch_cpu_torch_backend(monkeypatch):
    """compress_batch / decompress_batch on a CPU model (torch backend) at a
    32x48 crop, bottleneck (32, 4, 6): the container and error-path checks
    do not depend on the size and the torch codec is slow."""
    crop = (32, 48)
    model = H.small_dsin(crop)
    x, y = H.images(2, crop, "cpu")
    # a portable id (2) opens on a CPU model by itself: only the comparison
    # between the containers of the batch can refuse it
    H.check_compress_batch(model, x, y, None, 2, monkeypatch)
