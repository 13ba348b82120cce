"""Portable codec backend (container id 2) on the GPU against its host build.

The PORTABLE instantiation of pc_freqs_kernel and the host functions of
csrc/pc_model.h must agree bit for bit: logits (compared as int32), tables,
stream bytes. Each side decodes the other's stream, the golden stream
decodes on the device, and a container written on a GPU model opens on a
CPU copy of it."""

import copy
import os
import struct

import pytest
import torch

import _portable_helpers as P
from dsin_amd import config as cm
from dsin_amd import ops
from dsin_amd.coding import (compress, decode_symbols, decompress,
                             encode_symbols)
from dsin_amd.coding import bitstream as bs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _assert_bitwise(pc, centers, shape, dev, seed):
    """Device and host pc_freqs(portable=True) at every position of a
    volume; returns the host (logits, tables)."""
    L = centers.numel()
    q = P.q_pad_of(pc, centers, P.symbols_of(shape, L, seed=seed))
    pos = P.positions(shape)
    lg_h, fr_h = ops.pc_freqs(pc, q, pos, portable=True)
    pcd = copy.deepcopy(pc).to(dev)
    lg_d, fr_d = ops.pc_freqs(pcd, q.to(dev), pos.to(dev), portable=True)
    assert lg_d.is_cuda and fr_d.is_cuda
    assert torch.equal(P.bits(lg_d.cpu()), P.bits(lg_h)), shape
    assert torch.equal(fr_d.cpu(), fr_h), shape
    return lg_h, fr_h


@pytest.mark.parametrize("k", P.KS)
@pytest.mark.parametrize("L", P.LS)
def test_device_and_host_agree_bitwise(dev, L, k):
    pc = P.make_pc(L, k, seed=1)
    centers = P.centers_of(L)
    for shape in P.SHAPES:
        lg, fr = _assert_bitwise(pc, centers, shape, dev, seed=sum(shape))
        assert torch.isfinite(lg).all()
        assert int(fr.min()) >= 1 and int(fr.sum(dim=1).max()) <= 65535


def test_saturated_case_agrees_bitwise(dev):
    L = 6
    pc = P.saturate(P.make_pc(L, seed=4))
    _, fr = _assert_bitwise(pc, P.centers_of(L), (4, 8, 10), dev, seed=8)
    assert int((fr == 1).sum()) >= 1


def test_subnormal_case_agrees_bitwise(dev):
    """Subnormal conv0 weights and activations, subnormal logits: both sides
    keep fp32 subnormals, neither flushes them."""
    L = 6
    pc = P.make_subnormal(P.make_pc(L, 8, seed=2))
    tiny = torch.finfo(torch.float32).tiny
    w0 = pc.conv0.weight.detach().abs()
    assert bool(((w0 > 0) & (w0 < tiny)).any())
    lg, _ = _assert_bitwise(pc, P.centers_of(L), (3, 5, 6), dev, seed=3)
    assert bool(((lg.abs() > 0) & (lg.abs() < tiny)).any())


@pytest.mark.parametrize("shape", [(4, 8, 10), (32, 8, 12)])
def test_streams_equal_and_cross_decode(dev, shape):
    L = 6
    pc = P.make_pc(L, seed=5)
    pcd = copy.deepcopy(pc).to(dev)
    centers = P.centers_of(L)
    symbols = P.symbols_of(shape, L, seed=9, zero_frac=0.5)
    data_h = encode_symbols(pc, centers, symbols, backend="portable")
    data_d = encode_symbols(pcd, centers.to(dev), symbols.to(dev),
                            backend="portable")
    assert data_d == data_h
    out_d = decode_symbols(pcd, centers.to(dev), data_h, shape,
                           backend="portable")
    assert out_d.is_cuda and torch.equal(out_d.cpu(), symbols)
    out_h = decode_symbols(pc, centers, data_d, shape, backend="portable")
    assert not out_h.is_cuda and torch.equal(out_h, symbols)


def test_golden_stream_decodes_on_device(dev):
    pc, centers, symbols, stream = P.load_golden()
    pc, centers = pc.to(dev), centers.to(dev)
    out = decode_symbols(pc, centers, stream, (3, 5, 6), backend="portable")
    assert torch.equal(out.cpu(), symbols)
    assert encode_symbols(pc, centers, symbols.to(dev),
                          backend="portable") == stream


def test_gpu_container_opens_on_cpu_model(dev):
    """compress(backend="portable") on a GPU model; decompress on a CPU copy
    of it. The symbols are what is portable: x_dec comes from the decoder
    network, which is not bitwise the same on the two devices."""
    from dsin_amd.data import SyntheticStereo
    from dsin_amd.models import DSIN
    cfg = os.path.join(P.HERE, "..", "run_configs")
    ae, _ = cm.parse(os.path.join(cfg, "ae_run_configs"))
    pcc, _ = cm.parse(os.path.join(cfg, "pc_run_configs"))
    ae.crop_size = (64, 96)
    ae.y_patch_size = (16, 16)
    torch.manual_seed(0)
    model = DSIN(ae, pcc).to(dev).eval()
    x, y = SyntheticStereo(64, 96, batch_size=1, device=dev).next_batch()
    with torch.no_grad():
        data = compress(model, x, backend="portable")
        symbols = model.encoder(x).symbols[0]
    bid, shape, L, _, payload = bs.parse_container(data)
    assert bid == 2 and shape == (32, 8, 12) and L == 6

    cpu_model = copy.deepcopy(model).cpu().eval()
    cen_c = cpu_model.encoder.quantizer.centers.detach()
    cen_d = model.encoder.quantizer.centers.detach()
    sym_c = decode_symbols(cpu_model.probclass, cen_c, payload, shape,
                           backend="portable")
    sym_d = decode_symbols(model.probclass, cen_d, payload, shape,
                           backend="portable")
    assert torch.equal(sym_c, symbols.cpu())
    assert torch.equal(sym_d, symbols)
    x_dec_c, x_si_c = decompress(cpu_model, data, y.cpu())
    assert not x_dec_c.is_cuda and x_dec_c.shape == x.shape
    assert x_si_c.shape == x.shape
    # the GPU model takes the portable stream too, and still refuses id 0
    x_dec_d, _ = decompress(model, data, y)
    assert x_dec_d.is_cuda and x_dec_d.shape == x.shape
    f = list(struct.unpack_from("<4sBBHHHHII", data))
    f[2] = 0
    with pytest.raises(ValueError):
        decompress(model, struct.pack("<4sBBHHHHII", *f)
                   + data[bs.HEADER_SIZE:], y)
    # and a CPU-written portable container opens on the GPU model
    data_c = compress(cpu_model, x.cpu(), backend="portable")
    bid_c, shape_c, _, _, payload_c = bs.parse_container(data_c)
    assert bid_c == 2
    sym_back = decode_symbols(model.probclass, cen_d, payload_c, shape_c,
                              backend="portable")
    with torch.no_grad():
        want = cpu_model.encoder(x.cpu()).symbols[0]
    assert torch.equal(sym_back.cpu(), want)
