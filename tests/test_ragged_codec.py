"""Ragged entropy codec on the CPU: symbol volumes of different shapes in one
batch, through the portable backend's host build and through the torch
backend, compress_many / decompress_many on a CPU model and the multi-image
archive. The oracle is the single-image path; every comparison is exact."""

import pytest
import torch

import _batch_helpers as H
import _portable_helpers as P
import _ragged_helpers as R
from dsin_amd import ops

CPU = torch.device("cpu")


@pytest.fixture(params=[False, True], ids=["fma", "libm"])
def host_path(request):
    """Both host paths of the portable model: run-time choice and forced
    library fmaf."""
    prev = ops.pc_host_force_libm(request.param)
    yield request.param
    ops.pc_host_force_libm(prev)


def _setup(L, k, shapes, seed, saturated=False):
    pc, centers = P.make_pc(L, k, seed=1), P.centers_of(L)
    if saturated:
        P.saturate(pc)
    return pc, centers, R.volumes(shapes, L, seed=seed)


@pytest.mark.parametrize("L,k", R.LK)
def test_portable_tables_equal_the_single_image_ones(L, k, host_path):
    """Test 1 on both host paths."""
    pc, centers = P.make_pc(L, k, seed=1), P.centers_of(L)
    for shapes in (R.MIX, R.ONE):
        R.check_tables(pc, centers, pc, shapes, True, CPU)


@pytest.mark.parametrize("batch", list(R.BATCHES))
@pytest.mark.parametrize("L,k", R.LK)
def test_portable_bytes_and_roundtrip(L, k, batch):
    """Tests 2 and 3: every ordering, a batch of one, 17 alternating."""
    pc, centers, symbols = _setup(L, k, R.BATCHES[batch], seed=7)
    key = ("cpu", "portable", L, k, batch)
    R.check_bytes(key, pc, centers, symbols, "portable")
    R.check_roundtrip(key, pc, centers, symbols, "portable")


@pytest.mark.parametrize("order", list(R.ORDERS))
def test_torch_bytes_and_roundtrip(order):
    """Tests 2 and 3, torch backend: a loop over the images."""
    pc, centers, symbols = _setup(6, 8, R.ORDERS[order], seed=2)
    key = ("cpu", "torch", 6, 8, order)
    R.check_bytes(key, pc, centers, symbols, "torch")
    R.check_roundtrip(key, pc, centers, symbols, "torch")


@pytest.mark.parametrize("L,k", R.LK)
def test_portable_stream_bounds(L, k):
    """Test 4."""
    for shapes in R.ORDERS.values():
        pc, centers, symbols = _setup(L, k, shapes, seed=5)
        R.check_stream_bounds(pc, centers, symbols, "portable")


@pytest.mark.parametrize("order", list(R.ORDERS))
def test_portable_saturated(order):
    """Test 5: table entries of 1, stream lengths differ widely."""
    pc, centers, symbols = _setup(6, 24, R.ORDERS[order], seed=8,
                                  saturated=True)
    key = ("cpu", "portable-saturated", order)
    datas = R.check_bytes(key, pc, centers, symbols, "portable")
    assert len(set(len(d) for d in datas)) > 1
    R.check_roundtrip(key, pc, centers, symbols, "portable")


@pytest.mark.parametrize("backend", ["portable", "torch"])
def test_equal_sizes_give_the_batch_bytes(backend):
    """Test 6."""
    R.check_equal_sizes(P.make_pc(6, 8, seed=1), P.centers_of(6), backend)


@pytest.mark.parametrize("backend", ["portable", "torch"])
def test_rejected_requests(backend, monkeypatch):
    """Test 7, symbol level."""
    R.check_symbol_level_rejected(P.make_pc(6, 8), P.centers_of(6), backend,
                                  monkeypatch)


def test_hip_backend_needs_a_gpu():
    pc, centers = P.make_pc(6, 8), P.centers_of(6)
    sym = P.symbols_of((2, 1, 7), 6, seed=1)
    with pytest.raises(ValueError):
        R.encode_symbols_ragged(pc, centers, [sym], backend="hip")


def test_extension_rejects_what_the_wrappers_would():
    """The host validation of the entry points themselves, reached past the
    Python wrappers: descriptor table, items, segment table, payload
    offsets."""
    ext = ops._require_ext("pc_decode_ragged", "on the CPU")
    pc, centers = P.make_pc(6, 8), P.centers_of(6)
    k, L = ops.check_pc_shape(pc)
    wts = ops.pc_pack_weights(pc)
    n1, n2 = 6 * 9 * 15, 5 * 9 * 9
    q = torch.zeros(n1 + n2)
    good = [2, 1, 7, 0, 0, 1, 1, 1, n1, 14]
    items = torch.tensor([[0, 0, 0, 0], [1, 0, 0, 0]], dtype=torch.int32)
    data = torch.zeros(8, dtype=torch.uint8)

    def call(desc=good, items=items, seg=(0, 1, 2), offs=(0, 4, 8)):
        return ext(q, list(desc), items, list(seg), wts, k, L, data,
                   list(offs), centers, True)
    call()
    q.zero_()
    for kw in (dict(desc=[0, 1, 7, 0, 0, 1, 1, 1, n1, 14]),
               dict(desc=[2, 1, 7, 0, 0, 1, 1, 1, n1 + 1, 14]),
               dict(desc=[2, 1, 7, 0, 0, 1, 1, 1, n1 - 1, 14]),
               dict(desc=[2, 1, 7, 0, 0, 1, 1, 1, n1, 13]),
               dict(desc=good[:9]),
               dict(items=torch.tensor([[0, 0, 0, 7], [1, 0, 0, 0]],
                                       dtype=torch.int32)),
               dict(items=torch.tensor([[0, 0, 0, 0], [2, 0, 0, 0]],
                                       dtype=torch.int32)),
               dict(items=torch.tensor([[1, 0, 0, 0], [0, 0, 0, 0]],
                                       dtype=torch.int32)),
               dict(seg=(0, 2)), dict(seg=(0, 1, 1)), dict(seg=(0, 2, 1, 2, 2)),
               dict(offs=(0, 4)), dict(offs=(0, 9, 8)), dict(offs=(0, 4, 7))):
        with pytest.raises(RuntimeError):
            call(**kw)
    assert not q.any()


def test_archive():
    """Test 7, archive parsing and round trips."""
    R.check_archive()


@pytest.mark.parametrize("backend", [None, "portable"])
def test_compress_many_decompress_many(backend, monkeypatch):
    """Test 8 on a CPU model: torch (the model's own backend) and
    portable."""
    model = H.small_dsin((64, 96))
    # an id that opens on a CPU model by itself, so that only the comparison
    # between the containers can refuse it
    other = 2 if backend is None else 0
    R.check_compress_many(model, backend, other, monkeypatch)
