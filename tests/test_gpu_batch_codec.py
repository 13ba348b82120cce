"""Batched entropy codec on the GPU (hip and portable backends): B images
share one pc_freqs launch per wave and have a range-coder workgroup each.
Every comparison is exact. The single-image calls are the reference: a
position's tables must not depend on which other images are in the launch,
stream b of a batch is the single-image stream of image b, and a workgroup's
byte window ends where its own image's payload ends."""

import copy

import pytest
import torch

import _batch_helpers as H
import _portable_helpers as P
from dsin_amd import ops
from dsin_amd.coding import decode_symbols_batch, encode_symbols_batch

pytestmark = pytest.mark.gpu

BACKENDS = ["hip", "portable"]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _on(dev, pc, centers, symbols=None):
    out = (copy.deepcopy(pc).to(dev), centers.to(dev))
    return out if symbols is None else out + (symbols.to(dev),)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("L,k", H.LK)
def test_launch_independence_across_images(dev, backend, L, k):
    """Test 1: batched logits and tables [b] == ops.pc_freqs of image b."""
    pc, centers = P.make_pc(L, k, seed=1), P.centers_of(L)
    shape = (3, 5, 6)
    symbols = H.mixed_symbols(shape, L, 3, seed=4)
    q = torch.stack([P.q_pad_of(pc, centers, s) for s in symbols]).to(dev)
    pos = P.positions(shape).to(dev)
    pcd = copy.deepcopy(pc).to(dev)
    portable = backend == "portable"
    lg, fr = ops.pc_freqs_batch(pcd, q, pos, portable=portable)
    assert lg.is_cuda and lg.shape == (3, pos.shape[0], L)
    assert fr.shape == lg.shape
    for b in range(3):
        lg1, fr1 = ops.pc_freqs(pcd, q[b], pos, portable=portable)
        assert torch.equal(P.bits(lg[b].cpu()), P.bits(lg1.cpu())), b
        assert torch.equal(fr[b], fr1), b


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("B", H.BATCHES)
@pytest.mark.parametrize("L,k", H.LK)
def test_bytes(dev, backend, L, k, B):
    """Test 2."""
    pc, centers = _on(dev, P.make_pc(L, k, seed=1), P.centers_of(L))
    for shape in H.SHAPES:
        H.check_bytes(pc, centers,
                      H.mixed_symbols(shape, L, B, seed=B).to(dev), backend)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("L,k", H.LK)
def test_roundtrip_and_cross_decoding(dev, backend, L, k):
    """Test 3."""
    pc, centers = _on(dev, P.make_pc(L, k, seed=2), P.centers_of(L))
    for shape in H.SHAPES:
        for B in (1, 3):
            H.check_roundtrip(pc, centers,
                              H.mixed_symbols(shape, L, B, seed=7).to(dev),
                              backend)


@pytest.mark.parametrize("backend", BACKENDS)
def test_roundtrip_saturated_and_largest_volume(dev, backend):
    """Table entries of 1 (streams of very different lengths), B = 17 at
    (3, 10, 12), and one batch at the largest volume (32, 8, 12)."""
    L = 6
    pc, centers = _on(dev, P.saturate(P.make_pc(L, seed=4)), P.centers_of(L))
    symbols = H.mixed_symbols((3, 10, 12), L, 17, seed=8).to(dev)
    datas = H.check_bytes(pc, centers, symbols, backend)
    assert len(set(len(d) for d in datas)) > 1
    H.check_roundtrip(pc, centers, symbols, backend)
    pc, centers = _on(dev, P.make_pc(L, seed=5), P.centers_of(L))
    H.check_roundtrip(pc, centers,
                      H.mixed_symbols((32, 8, 12), L, 3, seed=9).to(dev),
                      backend)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("L,k", H.LK)
def test_stream_bounds(dev, backend, L, k):
    """Test 4: a short middle stream is defined behaviour (zeros past the
    end) and must not read the next image's bytes."""
    pc, centers = _on(dev, P.make_pc(L, k, seed=3), P.centers_of(L))
    for shape in H.SHAPES:
        H.check_stream_bounds(pc, centers,
                              H.mixed_symbols(shape, L, 3, seed=5).to(dev),
                              backend)


def test_portable_across_devices(dev):
    """Test 5: golden stream at index 1 of a GPU batch; GPU batch decodes
    with the host build and the reverse."""
    pc, centers, symbols, stream = P.load_golden()
    batch = torch.stack([P.symbols_of((3, 5, 6), 6, seed=1), symbols,
                         torch.zeros(3, 5, 6, dtype=torch.int64)])
    pcd, cend, batchd = _on(dev, pc, centers, batch)
    datas_d = encode_symbols_batch(pcd, cend, batchd, backend="portable")
    assert datas_d[1] == stream
    out_h = decode_symbols_batch(pc, centers, datas_d, (3, 5, 6),
                                 backend="portable")
    assert not out_h.is_cuda and torch.equal(out_h, batch)
    datas_h = encode_symbols_batch(pc, centers, batch, backend="portable")
    assert datas_h == datas_d
    out_d = decode_symbols_batch(pcd, cend, datas_h, (3, 5, 6),
                                 backend="portable")
    assert out_d.is_cuda and torch.equal(out_d.cpu(), batch)


@pytest.mark.parametrize("backend", BACKENDS)
def test_rejected_requests(dev, backend):
    """Test 6: raised before any launch."""
    pc, centers = _on(dev, P.make_pc(6, 8), P.centers_of(6))
    H.check_rejected(pc, centers, backend)
    q = torch.zeros(2, 6, 9, 15, device=dev)
    pos = P.positions((2, 1, 7)).to(dev)
    with pytest.raises(ValueError):  # one stream for a batch of two
        ops.pc_decode_batch(pc, q, pos, [0, pos.shape[0]], [b"\0" * 4],
                            centers, portable=backend == "portable")
    assert not q.any()  # nothing was decoded into the buffer


@pytest.mark.parametrize("backend", [None, "portable"])
def test_compress_batch_decompress_batch(dev, backend, monkeypatch):
    """Test 7 at small_ae_config (crop 64x96, bottleneck (32, 8, 12)),
    B = 2, with the model's own backend (hip) and with portable."""
    crop = (64, 96)
    model = H.small_dsin(crop).to(dev)
    x, y = H.images(2, crop, dev)
    # an id that opens on this model by itself, so that only the comparison
    # between the containers of the batch can refuse it
    other = 2 if backend is None else 1
    H.check_compress_batch(model, x, y, backend, other, monkeypatch)
