"""Container format, compress/decompress on the torch backend, the packed
live-tap weights and table rule of the hip backend, and the host build of
the device coder's step functions (all CPU)."""

import struct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dsin_amd import ops
from dsin_amd.coding import (compress, decode_symbols, decode_with_freqs,
                             decompress, encode_symbols, encode_with_freqs)
from dsin_amd.coding import bitstream as bs
from dsin_amd.models import DSIN
from dsin_amd.models.probclass import ProbClass


def _make_pc(pc_config, L=6, k=None, seed=0):
    cfg = pc_config.clone()
    if k is not None:
        cfg.arch_param__k = k
    torch.manual_seed(seed)
    pc = ProbClass(cfg, num_centers=L)
    with torch.no_grad():  # biases are zero at init; make them count
        for m in (pc.conv0, pc.res_conv1, pc.res_conv2, pc.conv2):
            m.bias.uniform_(-0.2, 0.2)
    return pc


class _TinyModel:
    """The part of a DSIN that the container code looks at."""

    def __init__(self, pc, centers):
        self.probclass = pc

        class _Q:
            pass

        class _E:
            pass
        self.encoder = _E()
        self.encoder.quantizer = _Q()
        self.encoder.quantizer.centers = centers


@pytest.fixture(scope="module")
def small_model_and_stream():
    """One compress() at small_ae_config on the CPU, shared by the tests."""
    from dsin_amd import config as cm
    import os
    root = os.path.join(os.path.dirname(__file__), "..", "run_configs")
    ae, _ = cm.parse(os.path.join(root, "ae_run_configs"))
    pc, _ = cm.parse(os.path.join(root, "pc_run_configs"))
    ae.crop_size = (64, 96)
    ae.y_patch_size = (16, 16)
    torch.manual_seed(0)
    model = DSIN(ae, pc).eval()
    g = torch.Generator().manual_seed(1)
    x = torch.rand(1, 3, 64, 96, generator=g) * 255
    y = (x + torch.randn(x.shape, generator=g) * 4).clamp(0, 255)
    return model, x, y, compress(model, x)


def test_container_roundtrip_symbols(pc_config):
    """Header + payload survive pack/parse and the payload decodes back, at
    symbols (3, 5, 6) through the torch backend."""
    pc = _make_pc(pc_config)
    centers = torch.linspace(-2, 2, 6)
    torch.manual_seed(2)
    symbols = torch.randint(0, 6, (3, 5, 6))
    payload = encode_symbols(pc, centers, symbols, backend="torch")
    assert payload == encode_symbols(pc, centers, symbols)  # default = torch
    crc = bs.probclass_crc(_TinyModel(pc, centers))
    data = bs.pack_container("torch", symbols.shape, 6, crc, payload)
    assert data[:4] == b"DSIN" and len(data) == bs.HEADER_SIZE + len(payload)
    bid, shape, L, crc2, payload2 = bs.parse_container(data)
    assert (bid, shape, L, crc2, payload2) == (0, (3, 5, 6), 6, crc, payload)
    out = decode_symbols(pc, centers, payload2, shape, backend="torch")
    assert torch.equal(out, symbols)


def test_compress_decompress_small_config(small_model_and_stream):
    """decompress(compress(x), y) equals DSIN.reconstruct(x, y) bitwise on
    the CPU torch backend at small_ae_config."""
    model, x, y, data = small_model_and_stream
    assert isinstance(data, bytes)
    bid, shape, L, _, payload = bs.parse_container(data)
    assert bid == 0 and shape == (32, 8, 12) and L == 6 and len(payload) > 4
    x_dec, x_si = decompress(model, data, y)
    _, _, r_dec, r_si, bpp = model.reconstruct(x, y)
    assert torch.equal(x_dec, r_dec)
    assert torch.equal(x_si, r_si)
    # the real stream is close to the estimate reconstruct reports
    est_bits = float(bpp) * 64 * 96
    assert 8 * len(payload) < 1.05 * est_bits + 64
    # (3,H,W) input and no side image
    assert compress(model, x[0]) == data
    x_dec2, none = decompress(model, data)
    assert none is None and torch.equal(x_dec2, r_dec)


def _rebuild(data, **kw):
    f = list(struct.unpack_from("<4sBBHHHHII", data))
    names = ["magic", "version", "backend", "C", "Hb", "Wb", "L", "crc", "n"]
    for k, v in kw.items():
        f[names.index(k)] = v
    return struct.pack("<4sBBHHHHII", *f) + data[bs.HEADER_SIZE:]


@pytest.mark.parametrize("what", ["magic", "version", "truncated", "short",
                                  "backend", "crc", "L"])
def test_header_errors_raise(small_model_and_stream, what, monkeypatch):
    model, _, _, data = small_model_and_stream
    bad = {
        "magic": lambda: _rebuild(data, magic=b"DSIM"),
        "version": lambda: _rebuild(data, version=2),
        "truncated": lambda: data[:-1],
        "short": lambda: data[:10],
        "backend": lambda: _rebuild(data, backend=1),
        "crc": lambda: _rebuild(
            data, crc=struct.unpack_from("<I", data, 14)[0] ^ 1),
        "L": lambda: _rebuild(data, L=7),
    }[what]()

    def boom(*a, **k):  # nothing may be decoded or launched
        raise AssertionError("decode started despite a bad header")
    monkeypatch.setattr(bs, "decode_symbols", boom)
    with pytest.raises(ValueError):
        decompress(model, bad)


def test_crc_tracks_probclass_weights(pc_config):
    pc = _make_pc(pc_config)
    centers = torch.linspace(-2, 2, 6)
    m = _TinyModel(pc, centers)
    c0 = bs.probclass_crc(m)
    assert c0 == bs.probclass_crc(m)
    with torch.no_grad():
        pc.res_conv1.weight[3, 2, 0, 1, 1] += 1e-3
    c1 = bs.probclass_crc(m)
    assert c1 != c0
    m.encoder.quantizer.centers = centers.clone()
    m.encoder.quantizer.centers[2] += 1e-3
    assert bs.probclass_crc(m) != c1


def test_unknown_backend_and_hip_on_cpu_raise(pc_config):
    pc = _make_pc(pc_config)
    centers = torch.linspace(-2, 2, 6)
    symbols = torch.zeros(1, 1, 1, dtype=torch.int64)
    with pytest.raises(ValueError):
        encode_symbols(pc, centers, symbols, backend="cuda")
    with pytest.raises(ValueError):
        encode_symbols(pc, centers, symbols, backend="hip")
    with pytest.raises(ValueError):
        decode_symbols(pc, centers, b"\0" * 8, (1, 1, 1), backend="hip")


def test_unsupported_probclass_shapes_raise(pc_config):
    with pytest.raises(ValueError):
        ops.check_pc_shape(_make_pc(pc_config, L=17))
    with pytest.raises(ValueError):
        ops.check_pc_shape(_make_pc(pc_config, k=33))
    cfg = pc_config.clone()
    cfg.kernel_size = 5
    with pytest.raises(ValueError):
        ops.check_pc_shape(ProbClass(cfg, num_centers=6))
    assert ops.check_pc_shape(_make_pc(pc_config, L=16, k=32)) == (32, 16)


def _logits64(pc, ctx):
    """fp64 logits of one (5,9,9) context with the masked convs as
    ProbClass.logits orders them."""
    def conv(x, m, relu):
        w = (m.weight * m.mask).double()
        y = F.conv3d(x, w, m.bias.double())
        return torch.relu(y) if relu else y
    x = ctx.double().reshape(1, 1, 5, 9, 9)
    a0 = conv(x, pc.conv0, True)
    a1 = conv(a0, pc.res_conv1, True)
    a2 = conv(a1, pc.res_conv2, False) + a0[:, :, 2:, 2:-2, 2:-2]
    return conv(a2, pc.conv2, False).reshape(-1)


@pytest.mark.parametrize("L,k", [(6, 24), (2, 8), (16, 32), (5, 20)])
def test_packed_live_taps_match_logits(pc_config, L, k):
    """A pure-torch evaluation of one 5x9x9 context from the packed layout
    equals the masked-conv logits in fp64. Non-causal context entries are
    NaN: a packed tap that read one would poison the result."""
    pc = _make_pc(pc_config, L=L, k=k, seed=3)
    packed = ops.pc_pack_weights(pc)
    kp = (k + 7) // 8 * 8
    assert packed.dtype == torch.float32
    assert packed.numel() == (13 * kp + kp + 2 * (14 * k * kp + kp)
                              + 14 * k * L + L)
    assert ops.pc_live_taps(pc.conv0.mask).tolist() == list(range(13))
    assert ops.pc_live_taps(pc.conv2.mask).tolist() == list(range(14))
    g = torch.Generator().manual_seed(4)
    ctx = torch.randn(5, 9, 9, generator=g, dtype=torch.float64)
    want = _logits64(pc, ctx)
    also = pc.double().logits(ctx.reshape(1, 1, 5, 9, 9)).reshape(-1)
    pc.float()
    assert torch.allclose(want, also, rtol=0, atol=1e-12)
    poisoned = ctx.clone()
    poisoned[4, 4, 4:] = float("nan")
    poisoned[4, 5:, :] = float("nan")
    got = ops.pc_logits_packed_ref(packed.double(), k, L, poisoned)
    assert torch.isfinite(got).all()
    assert torch.allclose(got, want, rtol=0, atol=1e-11)


def test_hip_table_rule_bounds():
    """f = max(1, floor(p*(65536-L))): every f >= 1 and tot <= 65535, on
    random fp32 softmax rows, near-one-hot rows and exact one-hot rows."""
    g = torch.Generator().manual_seed(0)
    for L in (2, 6, 16):
        rows = [torch.softmax(torch.randn(4096, L, generator=g) * s, dim=1)
                for s in (0.1, 1.0, 10.0, 100.0)]
        rows.append(torch.eye(L))
        rows.append(torch.full((1, L), 1.0 / L))
        p = torch.cat(rows).float()
        f = ops.pc_table_from_probs(p)
        assert f.dtype == torch.int32 and f.shape == p.shape
        assert int(f.min()) >= 1
        assert int(f.sum(dim=1).max()) <= 65535
        onehot = ops.pc_table_from_probs(torch.eye(L))
        assert int(onehot.max()) == 65536 - L
        assert int(onehot.sum(dim=1).max()) == 65535


def _host_coder():
    if not ops.hip_available():
        pytest.skip("HIP extension does not import here")
    return ops._require_ext("rc_encode_host"), ops._require_ext("rc_decode_host")


@pytest.mark.parametrize("seed,n,L,fmax", [(0, 1, 2, 1), (1, 400, 6, 10000),
                                           (2, 3000, 16, 4095), (3, 700, 3, 3),
                                           (4, 2000, 6, 65535 // 6)])
def test_host_step_functions_match_python_coder(seed, n, L, fmax):
    """The host build of the device coder's step functions against
    encode_with_freqs / decode_with_freqs, byte for byte, on adaptive
    tables (table i is rotated by symbol i-1) with freq=1 tails."""
    enc, dec = _host_coder()
    rng = np.random.default_rng(seed)
    base = rng.integers(1, fmax + 1, size=(n, L)).astype(np.int64)
    base[rng.random((n, L)) < 0.3] = 1
    syms, tables = [], []
    for i in range(n):
        t = np.roll(base[i], syms[-1] if syms else 0)
        tables.append(t)
        syms.append(int(rng.choice(L, p=t / t.sum())))
    want = encode_with_freqs(syms, iter(tables))
    tt = torch.from_numpy(np.stack(tables).astype(np.int32))
    got = enc(torch.tensor(syms, dtype=torch.int32), tt)
    assert bytes(got.numpy().tobytes()) == want
    out = dec(got, tt)
    assert out.tolist() == syms
    py = decode_with_freqs(
        want, n, lambda i, prev: np.roll(base[i], prev[-1] if prev else 0))
    assert py == syms


def test_host_decoder_matches_python_on_garbage():
    """Random bytes, short of what the symbols need: both decoders read
    zeros past the end and return the same in-range symbols."""
    _, dec = _host_coder()
    rng = np.random.default_rng(7)
    n, L = 500, 6
    tables = rng.integers(1, 9000, size=(n, L)).astype(np.int64)
    data = rng.integers(0, 256, size=40, dtype=np.uint8).tobytes()
    want = decode_with_freqs(data, n, lambda i, prev: tables[i])
    got = dec(torch.frombuffer(bytearray(data), dtype=torch.uint8),
              torch.from_numpy(tables.astype(np.int32)))
    assert got.tolist() == want
    assert 0 <= min(want) and max(want) < L
