"""Ragged entropy codec on the GPU (hip and portable backends): symbol
volumes of different shapes share one wave counter, one pc_freqs workgroup
per item and a range-coder workgroup per image. The oracle is the
single-image path; every comparison is exact."""

import copy

import pytest
import torch

import _batch_helpers as H
import _portable_helpers as P
import _ragged_helpers as R
from dsin_amd.coding import (decode_symbols_ragged, encode_symbols_ragged)

pytestmark = pytest.mark.gpu

BACKENDS = ["hip", "portable"]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _setup(dev, L, k, shapes, seed, saturated=False):
    pc, centers = P.make_pc(L, k, seed=1), P.centers_of(L)
    if saturated:
        P.saturate(pc)
    symbols = [s.to(dev) for s in R.volumes(shapes, L, seed=seed)]
    return copy.deepcopy(pc).to(dev), centers.to(dev), symbols


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("L,k", R.LK)
def test_tables_equal_the_single_image_ones(dev, backend, L, k):
    """Test 1."""
    pc, centers = P.make_pc(L, k, seed=1), P.centers_of(L)
    pcd = copy.deepcopy(pc).to(dev)
    for shapes in (R.MIX, R.ONE):
        R.check_tables(pc, centers, pcd, shapes, backend == "portable", dev)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("batch", list(R.BATCHES))
@pytest.mark.parametrize("L,k", R.LK)
def test_bytes_and_roundtrip(dev, backend, L, k, batch):
    """Tests 2 and 3: every ordering, a batch of one, 17 alternating."""
    pc, centers, symbols = _setup(dev, L, k, R.BATCHES[batch], seed=7)
    key = ("gpu", backend, L, k, batch)
    R.check_bytes(key, pc, centers, symbols, backend)
    R.check_roundtrip(key, pc, centers, symbols, backend)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("L,k", R.LK)
def test_stream_bounds(dev, backend, L, k):
    """Test 4: a short middle stream reads zeros past its own end, never the
    next image's bytes."""
    for shapes in R.ORDERS.values():
        pc, centers, symbols = _setup(dev, L, k, shapes, seed=5)
        R.check_stream_bounds(pc, centers, symbols, backend)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("order", list(R.ORDERS))
def test_saturated(dev, backend, order):
    """Test 5."""
    pc, centers, symbols = _setup(dev, 6, 24, R.ORDERS[order], seed=8,
                                  saturated=True)
    key = ("gpu", backend + "-saturated", order)
    datas = R.check_bytes(key, pc, centers, symbols, backend)
    assert len(set(len(d) for d in datas)) > 1
    R.check_roundtrip(key, pc, centers, symbols, backend)


@pytest.mark.parametrize("backend", BACKENDS)
def test_equal_sizes_give_the_batch_bytes(dev, backend):
    """Test 6."""
    R.check_equal_sizes(P.make_pc(6, 8, seed=1).to(dev),
                        P.centers_of(6).to(dev), backend)


@pytest.mark.parametrize("order", list(R.ORDERS))
def test_portable_across_devices(dev, order):
    """Test 3, across devices: a portable ragged batch written on the GPU
    decodes through the host build and the reverse; same bytes on both."""
    L, k = 6, 24
    shapes = R.ORDERS[order]
    pc, centers = P.make_pc(L, k, seed=1), P.centers_of(L)
    symbols = R.volumes(shapes, L, seed=9)
    pcd, cend = copy.deepcopy(pc).to(dev), centers.to(dev)
    datas_d = encode_symbols_ragged(pcd, cend, [s.to(dev) for s in symbols],
                                    backend="portable")
    datas_h = encode_symbols_ragged(pc, centers, symbols, backend="portable")
    assert datas_d == datas_h
    out_h = decode_symbols_ragged(pc, centers, datas_d, shapes,
                                  backend="portable")
    out_d = decode_symbols_ragged(pcd, cend, datas_h, shapes,
                                  backend="portable")
    for b, s in enumerate(symbols):
        assert not out_h[b].is_cuda and torch.equal(out_h[b], s), b
        assert out_d[b].is_cuda and torch.equal(out_d[b].cpu(), s), b


@pytest.mark.parametrize("backend", BACKENDS)
def test_rejected_requests(dev, backend, monkeypatch):
    """Test 7, symbol level: raised before the extension is touched."""
    R.check_symbol_level_rejected(P.make_pc(6, 8).to(dev),
                                  P.centers_of(6).to(dev), backend,
                                  monkeypatch)


@pytest.mark.parametrize("backend", [None, "portable"])
def test_compress_many_decompress_many(dev, backend, monkeypatch):
    """Test 8 with the model's own backend (hip) and with portable."""
    model = H.small_dsin((64, 96)).to(dev)
    # an id that opens on this model by itself, so that only the comparison
    # between the containers can refuse it
    other = 2 if backend is None else 1
    R.check_compress_many(model, backend, other, monkeypatch)
