"""Portable codec backend (container id 2) on the CPU: the host build of
csrc/pc_model.h + csrc/rc_coder.h in the extension.

Logits are held to the bound the hip backend's test uses, 4*e32 + 1e-5
against an fp64 evaluation of the same fp32 weights (e32: error of the fp32
CPU torch path on the same input); tables to within 1 of the fp64 table of
the fp32 logits, with min >= 1 and tot <= 65535. Then the degenerate rows,
the two fmaf paths, the thread count, roundtrips, the container and the
golden stream."""

import struct

import pytest
import torch

import _portable_helpers as P
from dsin_amd import ops
from dsin_amd.coding import (compress, decode_symbols, decompress,
                             encode_symbols)
from dsin_amd.coding import bitstream as bs


def _roundtrip(pc, centers, symbols):
    data = encode_symbols(pc, centers, symbols, backend="portable")
    out = decode_symbols(pc, centers, data, tuple(symbols.shape),
                         backend="portable")
    assert out.dtype == torch.int64 and out.device.type == "cpu"
    assert torch.equal(out, symbols)
    return data


@pytest.mark.parametrize("centers_pad", [True, False])
@pytest.mark.parametrize("k", P.KS)
@pytest.mark.parametrize("L", P.LS)
def test_host_logits_and_tables_against_fp64(L, k, centers_pad):
    pc = P.make_pc(L, k, centers_pad, seed=1)
    centers = P.centers_of(L)
    packed = ops.pc_pack_weights(pc)
    for shape in P.SHAPES:
        q = P.q_pad_of(pc, centers, P.symbols_of(shape, L, seed=sum(shape)))
        pos = P.positions(shape)
        ref64 = P.ref_logits(pc, q, pos, torch.float64)
        ref32 = P.ref_logits(pc, q, pos, torch.float32)
        e32 = float((ref32.double() - ref64).abs().max())
        lg, fr = ops.pc_freqs(pc, q, pos, packed, portable=True)
        assert lg.shape == (len(pos), L) and lg.dtype == torch.float32
        assert fr.shape == (len(pos), L) and fr.dtype == torch.int32
        err, bound = float((lg.double() - ref64).abs().max()), 4 * e32 + 1e-5
        fr = fr.long()
        diff = int((fr - P.fp64_table(lg)).abs().max())
        print(f"L={L} k={k} pad={centers_pad} {shape}: err {err:.3e} "
              f"e32 {e32:.3e} bound {bound:.3e} table diff {diff}")
        assert err <= bound
        assert diff <= 1
        assert int(fr.min()) >= 1
        assert int(fr.sum(dim=1).max()) <= 65535


def test_saturated_tables_roundtrip():
    L = 6
    pc = P.saturate(P.make_pc(L, seed=4))
    centers = P.centers_of(L)
    symbols = P.symbols_of((4, 8, 10), L, seed=8)
    lg, fr = ops.pc_freqs(pc, P.q_pad_of(pc, centers, symbols),
                          P.positions(symbols.shape), portable=True)
    assert int((fr == 1).sum()) >= 1
    assert int(fr.min()) >= 1 and int(fr.sum(dim=1).max()) <= 65535
    assert int((fr.long() - P.fp64_table(lg)).abs().max()) <= 1
    _roundtrip(pc, centers, symbols)


def test_non_finite_logit_gives_uniform_table_and_roundtrips():
    L = 6
    pc = P.make_pc(L, seed=5)
    with torch.no_grad():
        pc.conv2.bias[2] = float("inf")
    centers = P.centers_of(L)
    symbols = P.symbols_of((3, 5, 6), L, seed=9)
    lg, fr = ops.pc_freqs(pc, P.q_pad_of(pc, centers, symbols),
                          P.positions(symbols.shape), portable=True)
    assert torch.isinf(lg[:, 2]).all()
    assert torch.equal(fr, torch.full_like(fr, (65536 - L) // L))
    _roundtrip(pc, centers, symbols)


def test_libm_and_hardware_fma_paths_give_equal_bits():
    if not ops.pc_host_fma_available():
        pytest.skip("this CPU has no FMA: only the libm path exists")
    L = 6
    centers = P.centers_of(L)
    symbols = P.symbols_of((3, 5, 6), L, seed=10)
    pos = P.positions(symbols.shape)
    path = ops._require_ext("pc_host_path")
    for pc in (P.make_pc(L, 24, seed=6), P.make_pc(L, 20, seed=6),
               P.saturate(P.make_pc(L, 8, seed=6)),
               P.make_subnormal(P.make_pc(L, 8, seed=6))):
        q = P.q_pad_of(pc, centers, symbols)
        assert path() == "fma"
        lg_hw, fr_hw = ops.pc_freqs(pc, q, pos, portable=True)
        data_hw = encode_symbols(pc, centers, symbols, backend="portable")
        prev = ops.pc_host_force_libm(True)
        try:
            assert path() == "libm"
            lg_lm, fr_lm = ops.pc_freqs(pc, q, pos, portable=True)
            data_lm = encode_symbols(pc, centers, symbols, backend="portable")
        finally:
            ops.pc_host_force_libm(prev)
        assert torch.equal(P.bits(lg_hw), P.bits(lg_lm))
        assert torch.equal(fr_hw, fr_lm)
        assert data_hw == data_lm


def test_thread_count_does_not_change_results():
    L = 6
    pc = P.make_pc(L, seed=7)
    centers = P.centers_of(L)
    symbols = P.symbols_of((4, 8, 10), L, seed=11)
    q = P.q_pad_of(pc, centers, symbols)
    pos = P.positions(symbols.shape)
    before = torch.get_num_threads()
    got = {}
    try:
        for n in (1, 4):
            torch.set_num_threads(n)
            lg, fr = ops.pc_freqs(pc, q, pos, portable=True)
            data = encode_symbols(pc, centers, symbols, backend="portable")
            out = decode_symbols(pc, centers, data, symbols.shape,
                                 backend="portable")
            got[n] = (P.bits(lg), fr, data, out)
    finally:
        torch.set_num_threads(before)
    assert torch.equal(got[1][0], got[4][0])
    assert torch.equal(got[1][1], got[4][1])
    assert got[1][2] == got[4][2]
    assert torch.equal(got[1][3], symbols) and torch.equal(got[4][3], symbols)


@pytest.mark.parametrize("shape", [(4, 8, 10), (32, 8, 12)])
def test_roundtrip(shape):
    L = 6
    pc = P.make_pc(L, seed=5)
    centers = P.centers_of(L)
    symbols = P.symbols_of(shape, L, seed=9, zero_frac=0.5)
    data = _roundtrip(pc, centers, symbols)
    assert data == encode_symbols(pc, centers, symbols, backend="portable")


def test_compress_portable_decompress_equals_reconstruct(small_ae_config,
                                                         pc_config):
    from dsin_amd.models import DSIN
    torch.manual_seed(0)
    model = DSIN(small_ae_config, pc_config).eval()
    g = torch.Generator().manual_seed(1)
    x = torch.rand(1, 3, 64, 96, generator=g) * 255
    y = (x + torch.randn(x.shape, generator=g) * 4).clamp(0, 255)
    data = compress(model, x, backend="portable")
    bid, shape, L, _, payload = bs.parse_container(data)
    assert bid == 2 == bs.BACKEND_IDS["portable"]
    assert shape == (32, 8, 12) and L == 6 and len(payload) > 4
    x_dec, x_si = decompress(model, data, y)
    _, _, r_dec, r_si, _ = model.reconstruct(x, y)
    assert torch.equal(x_dec, r_dec)
    assert torch.equal(x_si, r_si)
    # the default is still the torch backend on the CPU, and a hip stream is
    # still refused there
    assert bs.parse_container(compress(model, x))[0] == 0
    f = list(struct.unpack_from("<4sBBHHHHII", data))
    f[2] = 1
    with pytest.raises(ValueError):
        decompress(model, struct.pack("<4sBBHHHHII", *f)
                   + data[bs.HEADER_SIZE:], y)
    with pytest.raises(ValueError):
        compress(model, x, backend="cuda")


def test_golden_stream():
    pc, centers, symbols, stream = P.load_golden()
    assert symbols.shape == (3, 5, 6) and len(stream) > 4
    out = decode_symbols(pc, centers, stream, (3, 5, 6), backend="portable")
    assert torch.equal(out, symbols)
    assert encode_symbols(pc, centers, symbols, backend="portable") == stream


def test_extension_has_one_set_of_codec_entry_points():
    """The context model is reached through three entry points that take a
    batch and dispatch on the device; no per-device or single-image twin of
    them is left in the built extension."""
    ext = ops._try_load_ext()
    assert ext is not None
    for name in ("pc_freqs", "pc_encode", "pc_decode"):
        assert hasattr(ext, name), name
    for name in ("pc_freqs_batch", "rc_encode_batch", "pc_encode_batch",
                 "pc_decode_batch", "pc_freqs_batch_host",
                 "pc_encode_batch_host", "pc_decode_batch_host",
                 "pc_freqs_host", "pc_encode_host", "pc_decode_host"):
        assert not hasattr(ext, name), name


def test_cpu_without_extension_raises_runtime_error(monkeypatch):
    pc = P.make_pc(6, 8)
    centers = P.centers_of(6)
    symbols = P.symbols_of((1, 1, 1), 6, seed=1)
    monkeypatch.setattr(ops, "_try_load_ext", lambda: None)
    with pytest.raises(RuntimeError, match="build_ext"):
        encode_symbols(pc, centers, symbols, backend="portable")
