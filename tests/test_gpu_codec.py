"""Device-resident entropy codec (csrc/pc_codec.hip) on the GPU.

Logits are compared against an fp64 torch evaluation of the same fp32
weights; the bound is 4*e32 + 1e-5, e32 being the measured error of the
fp32 CPU torch path on the same input against fp64. Tables, launch
independence, causality, the coder against the Python range coder, and
roundtrips up to the shipped bottleneck (32, 40, 120)."""

import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dsin_amd import config as cm
from dsin_amd import ops
from dsin_amd.coding import (ProbclassTesting, compress, decode_symbols,
                             decompress, encode_symbols, encode_with_freqs)
from dsin_amd.coding import bitstream as bs
from dsin_amd.coding.entropy import _pad_value, _wave_order
from dsin_amd.models.probclass import ProbClass

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CFG = os.path.join(HERE, "..", "run_configs")
PAD = 4


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _make_pc(L=6, k=24, centers_pad=True, seed=0):
    cfg, _ = cm.parse(os.path.join(CFG, "pc_run_configs"))
    cfg.arch_param__k = k
    cfg.use_centers_for_padding = centers_pad
    torch.manual_seed(seed)
    pc = ProbClass(cfg, num_centers=L)
    with torch.no_grad():
        for m in (pc.conv0, pc.res_conv1, pc.res_conv2, pc.conv2):
            m.bias.uniform_(-0.2, 0.2)
    return pc


def _centers(L):
    return torch.linspace(-2, 2, L)


def _symbols(shape, L, seed, zero_frac=0.0):
    g = torch.Generator().manual_seed(seed)
    s = torch.randint(0, L, shape, generator=g)
    if zero_frac:
        s[torch.rand(shape, generator=g) < zero_frac] = 0
    return s


def _q_pad(pc, centers, symbols):
    """The padded fp32 value buffer (C+4, H+8, W+8) of a symbol volume."""
    C, H, W = symbols.shape
    q = torch.full((C + PAD, H + 2 * PAD, W + 2 * PAD),
                   float(_pad_value(pc, centers)), dtype=torch.float32)
    q[PAD:, PAD:H + PAD, PAD:W + PAD] = centers.float()[symbols]
    return q


def _positions(shape):
    waves = _wave_order(*shape, PAD)
    pos = torch.from_numpy(np.concatenate(waves).astype(np.int32))
    offs = np.concatenate([[0], np.cumsum([len(w) for w in waves])])
    return pos, offs


def _ref_logits(pc, q_pad, dtype):
    """(C, H, W, L) logits of every position: the masked convs run fully
    convolutionally over the padded buffer on the CPU in `dtype`."""
    def conv(x, m, relu):
        y = F.conv3d(x, (m.weight * m.mask).to(dtype), m.bias.to(dtype))
        return torch.relu(y) if relu else y
    x = q_pad.to(dtype)[None, None]
    a0 = conv(x, pc.conv0, True)
    a1 = conv(a0, pc.res_conv1, True)
    a2 = conv(a1, pc.res_conv2, False) + a0[:, :, 2:, 2:-2, 2:-2]
    return conv(a2, pc.conv2, False)[0].permute(1, 2, 3, 0).contiguous()


def _at(vol, pos):
    p = pos.long()
    return vol[p[:, 0], p[:, 1], p[:, 2]]


@pytest.mark.parametrize("centers_pad", [True, False])
@pytest.mark.parametrize("k", [8, 24])
@pytest.mark.parametrize("L", [2, 6, 16])
def test_logits_and_tables_against_fp64(dev, L, k, centers_pad):
    pc = _make_pc(L, k, centers_pad, seed=1)
    centers = _centers(L)
    pcd = pc.to(dev)
    packed = ops.pc_pack_weights(pcd)
    pc = _make_pc(L, k, centers_pad, seed=1)  # CPU twin, same weights
    for shape in [(3, 5, 6), (1, 1, 1), (2, 1, 7)]:
        q = _q_pad(pc, centers, _symbols(shape, L, seed=sum(shape)))
        pos, _ = _positions(shape)
        with torch.no_grad():
            ref64 = _at(_ref_logits(pc, q, torch.float64), pos)
            ref32 = _at(_ref_logits(pc, q, torch.float32), pos)
        e32 = float((ref32.double() - ref64).abs().max())
        lg, fr = ops.pc_freqs(pcd, q.to(dev), pos, packed)
        assert lg.shape == (len(pos), L) and lg.dtype == torch.float32
        assert fr.shape == (len(pos), L) and fr.dtype == torch.int32
        lg, fr = lg.cpu(), fr.cpu().long()
        err, bound = float((lg.double() - ref64).abs().max()), 4 * e32 + 1e-5
        print(f"L={L} k={k} pad={centers_pad} {shape}: err {err:.3e} "
              f"e32 {e32:.3e} bound {bound:.3e}")
        assert err <= bound
        want = torch.floor(torch.softmax(lg.double(), dim=1)
                           * (65536 - L)).long().clamp(min=1)
        assert int((fr - want).abs().max()) <= 1
        assert int(fr.min()) >= 1
        assert int(fr.sum(dim=1).max()) <= 65535


def test_launch_independence(dev):
    """One launch over all positions, per-wave launches and single-position
    launches give bitwise equal logits and tables."""
    pc = _make_pc().to(dev)
    centers = _centers(6)
    shape = (3, 5, 6)
    q = _q_pad(pc.cpu(), centers, _symbols(shape, 6, seed=5)).to(dev)
    pc = pc.to(dev)
    packed = ops.pc_pack_weights(pc)
    pos, offs = _positions(shape)
    pos = pos.to(dev)
    lg_all, fr_all = ops.pc_freqs(pc, q, pos, packed)
    parts = [ops.pc_freqs(pc, q, pos[a:b], packed)
             for a, b in zip(offs[:-1], offs[1:])]
    assert torch.equal(torch.cat([p[1] for p in parts]), fr_all)
    assert torch.equal(torch.cat([p[0] for p in parts]), lg_all)
    n = len(pos)
    for i in (0, n // 2, n - 1):
        lg1, fr1 = ops.pc_freqs(pc, q, pos[i:i + 1], packed)
        assert torch.equal(fr1[0], fr_all[i])
        assert torch.equal(lg1[0], lg_all[i])


def test_causality_nan_fill(dev):
    """With every non-causal entry of q_pad set to NaN for the queried
    position, its table does not change, bit for bit."""
    pc = _make_pc(seed=2)
    centers = _centers(6)
    shape = (3, 5, 6)
    q = _q_pad(pc, centers, _symbols(shape, 6, seed=6)).to(dev)
    pc = pc.to(dev)
    packed = ops.pc_pack_weights(pc)
    pos, _ = _positions(shape)
    pos = pos.to(dev)
    lg_all, fr_all = ops.pc_freqs(pc, q, pos, packed)
    assert torch.isfinite(lg_all).all()
    for i, (c, h, w) in enumerate(pos.tolist()):
        qn = q.clone()
        qn[c + PAD + 1:] = float("nan")
        qn[c + PAD, h + PAD + 1:] = float("nan")
        qn[c + PAD, h + PAD, w + PAD:] = float("nan")
        lg1, fr1 = ops.pc_freqs(pc, qn, pos[i:i + 1], packed)
        assert torch.equal(fr1[0], fr_all[i]), (c, h, w)
        assert torch.equal(lg1[0], lg_all[i]), (c, h, w)


def test_device_coder_matches_python_coder(dev):
    """rc_encode on the kernel's own tables for (32, 8, 12) gives the bytes
    of encode_with_freqs on the copied tables; the device decoder fed those
    bytes and tables returns the symbols."""
    pc = _make_pc(seed=3)
    centers = _centers(6)
    shape = (32, 8, 12)
    symbols = _symbols(shape, 6, seed=7)
    q = _q_pad(pc, centers, symbols).to(dev)
    pc = pc.to(dev)
    pos, _ = _positions(shape)
    _, fr = ops.pc_freqs(pc, q, pos)
    syms = _at(symbols, pos).to(torch.int32)
    rows = ops._require_ext("rc_encode")(syms.to(dev)[None], fr[None])
    assert rows.shape == (1, 8 + 3 * len(syms) + 16)
    buf = rows[0].cpu().numpy()
    n = int.from_bytes(buf[:8].tobytes(), "little")
    got = buf[8:8 + n].tobytes()
    want = encode_with_freqs(syms.tolist(), iter(fr.cpu().numpy().astype(np.int64)))
    assert got == want
    assert ops.pc_encode(pc, q, pos, syms) == want
    raw = torch.frombuffer(bytearray(got), dtype=torch.uint8).to(dev)
    out = ops._require_ext("rc_decode")(raw, fr)
    assert torch.equal(out.cpu(), syms.long())


def _roundtrip(pc, centers, symbols, dev):
    data = encode_symbols(pc, centers.to(dev), symbols.to(dev), backend="hip")
    out = decode_symbols(pc, centers.to(dev), data, tuple(symbols.shape),
                         backend="hip")
    assert out.dtype == torch.int64 and out.device.type == "cuda"
    assert torch.equal(out.cpu(), symbols)
    return data


def test_saturated_tables_roundtrip(dev):
    """conv2 scaled by 40 with a steep bias saturates the softmax: some
    table entries sit at the floor of 1 and the stream still decodes."""
    L = 6
    pc = _make_pc(L, seed=4)
    with torch.no_grad():
        pc.conv2.weight.mul_(40.0)
        pc.conv2.bias.copy_(torch.linspace(8, -8, L))
    centers = _centers(L)
    shape = (4, 8, 10)
    symbols = _symbols(shape, L, seed=8)
    q = _q_pad(pc, centers, symbols).to(dev)
    pc = pc.to(dev)
    pos, _ = _positions(shape)
    _, fr = ops.pc_freqs(pc, q, pos)
    assert int((fr == 1).sum()) >= 1
    assert int(fr.min()) >= 1 and int(fr.sum(dim=1).max()) <= 65535
    _roundtrip(pc, centers, symbols, dev)


@pytest.mark.parametrize("zero_frac", [0.0, 0.9])
@pytest.mark.parametrize("shape", [(4, 8, 10), (1, 1, 1), (32, 8, 12),
                                   (32, 40, 120)])
def test_roundtrip(dev, shape, zero_frac):
    L = 6
    pc = _make_pc(L, seed=5)
    centers = _centers(L)
    symbols = _symbols(shape, L, seed=9, zero_frac=zero_frac)
    if shape == (4, 8, 10):
        est = ProbclassTesting(pc, centers).total_bit_cost(symbols)
    data = _roundtrip(pc.to(dev), centers, symbols, dev)
    if shape == (4, 8, 10):
        print(f"{shape} zero_frac={zero_frac}: {8 * len(data)} bits, "
              f"estimate {est:.1f}")
        assert 8 * len(data) < 1.05 * est + 64


def test_random_payload_decodes_in_range(dev):
    L = 6
    pc = _make_pc(L, seed=6).to(dev)
    centers = _centers(L).to(dev)
    shape = (4, 8, 10)
    symbols = _symbols(shape, L, seed=10)
    n = len(encode_symbols(pc, centers, symbols.to(dev), backend="hip"))
    junk = np.random.default_rng(0).integers(0, 256, n, dtype=np.uint8)
    out = decode_symbols(pc, centers, junk.tobytes(), shape, backend="hip")
    assert out.shape == shape
    assert int(out.min()) >= 0 and int(out.max()) < L
    out0 = decode_symbols(pc, centers, b"", shape, backend="hip")
    assert int(out0.min()) >= 0 and int(out0.max()) < L


def test_two_decodes_bitwise_equal(dev):
    L = 6
    pc = _make_pc(L, seed=7).to(dev)
    centers = _centers(L).to(dev)
    shape = (32, 8, 12)
    symbols = _symbols(shape, L, seed=11, zero_frac=0.5).to(dev)
    data = encode_symbols(pc, centers, symbols, backend="hip")
    assert data == encode_symbols(pc, centers, symbols, backend="hip")
    a = decode_symbols(pc, centers, data, shape, backend="hip")
    b = decode_symbols(pc, centers, data, shape, backend="hip")
    assert torch.equal(a, b) and torch.equal(a, symbols)


def test_unsupported_shapes_raise_before_launch(dev):
    centers = _centers(6).to(dev)
    symbols = torch.zeros(1, 1, 1, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError):
        encode_symbols(_make_pc(6, k=40).to(dev), centers, symbols,
                       backend="hip")
    with pytest.raises(ValueError):
        encode_symbols(_make_pc(17).to(dev), _centers(17).to(dev), symbols,
                       backend="hip")
    with pytest.raises(ValueError):  # CPU tensors
        encode_symbols(_make_pc(), _centers(6), symbols.cpu(), backend="hip")


@pytest.mark.parametrize("autocast", [True, False])
def test_compress_decompress_equals_reconstruct(dev, autocast):
    """decompress(compress(x), y) returns x_dec and x_with_si bitwise equal
    to DSIN.reconstruct(x, y) under the same autocast setting, at
    small_ae_config (64x96, patches 16x16)."""
    from dsin_amd.data import SyntheticStereo
    from dsin_amd.models import DSIN
    ae, _ = cm.parse(os.path.join(CFG, "ae_run_configs"))
    pcc, _ = cm.parse(os.path.join(CFG, "pc_run_configs"))
    ae.crop_size = (64, 96)
    ae.y_patch_size = (16, 16)
    torch.manual_seed(0)
    model = DSIN(ae, pcc).to(dev).eval()
    x, y = SyntheticStereo(64, 96, batch_size=1, device=dev).next_batch()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16,
                                         enabled=autocast,
                                         cache_enabled=False):
        data = compress(model, x)
        x_dec, x_si = decompress(model, data, y)
        _, _, r_dec, r_si, bpp = model.reconstruct(x, y)
    bid, shape, L, _, payload = bs.parse_container(data)
    assert bid == 1 and shape == (32, 8, 12) and L == 6
    print(f"autocast={autocast}: {len(payload)} payload bytes, "
          f"bpp estimate {float(bpp):.4f}")
    assert x_dec.dtype == r_dec.dtype and torch.equal(x_dec, r_dec)
    assert x_si.dtype == r_si.dtype and torch.equal(x_si, r_si)
    # a torch-backend stream is refused on the GPU model
    import struct
    f = list(struct.unpack_from("<4sBBHHHHII", data))
    f[2] = 0
    with pytest.raises(ValueError):
        decompress(model, struct.pack("<4sBBHHHHII", *f)
                   + data[bs.HEADER_SIZE:], y)
