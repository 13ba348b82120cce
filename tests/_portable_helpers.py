"""Shared by test_portable_codec.py (CPU) and test_gpu_portable_codec.py:
seeded probclasses in the style of test_gpu_codec._make_pc, the padded value
buffer, wave-ordered positions, the fp64 conv reference and the golden
fixture."""

import os

import numpy as np
import torch
import torch.nn.functional as F

from dsin_amd import config as cm
from dsin_amd.coding.entropy import _pad_value, _wave_order
from dsin_amd.models.probclass import ProbClass

HERE = os.path.dirname(os.path.abspath(__file__))
CFG = os.path.join(HERE, "..", "run_configs")
GOLDEN = os.path.join(HERE, "golden", "portable_k8_L6.npz")
PAD = 4
LS = [2, 6, 16]
KS = [8, 20, 24, 32]
SHAPES = [(3, 5, 6), (1, 1, 1), (2, 1, 7)]
LAYERS = ("conv0", "res_conv1", "res_conv2", "conv2")


def make_pc(L=6, k=24, centers_pad=True, seed=0):
    cfg, _ = cm.parse(os.path.join(CFG, "pc_run_configs"))
    cfg.arch_param__k = k
    cfg.use_centers_for_padding = centers_pad
    torch.manual_seed(seed)
    pc = ProbClass(cfg, num_centers=L)
    with torch.no_grad():
        for name in LAYERS:
            getattr(pc, name).bias.uniform_(-0.2, 0.2)
    return pc


def saturate(pc):
    """conv2 scaled by 40 with a steep bias: some table entries reach 1."""
    with torch.no_grad():
        pc.conv2.weight.mul_(40.0)
        pc.conv2.bias.copy_(torch.linspace(8, -8, pc.conv2.bias.numel()))
    return pc


def make_subnormal(pc):
    """conv0 weights scaled into the fp32 subnormal range (bias zero, so its
    activations are subnormal too), conv2 scaled so the logits are."""
    with torch.no_grad():
        pc.conv0.weight.mul_(1e-38)
        pc.conv0.bias.zero_()
        pc.conv2.weight.mul_(1e-38)
        pc.conv2.bias.mul_(1e-38)
    return pc


def centers_of(L):
    return torch.linspace(-2, 2, L)


def symbols_of(shape, L, seed, zero_frac=0.0):
    g = torch.Generator().manual_seed(seed)
    s = torch.randint(0, L, shape, generator=g)
    if zero_frac:
        s[torch.rand(shape, generator=g) < zero_frac] = 0
    return s


def q_pad_of(pc, centers, symbols):
    """The padded fp32 value buffer (C+4, H+8, W+8) of a symbol volume."""
    C, H, W = symbols.shape
    q = torch.full((C + PAD, H + 2 * PAD, W + 2 * PAD),
                   float(_pad_value(pc, centers)), dtype=torch.float32)
    q[PAD:, PAD:H + PAD, PAD:W + PAD] = centers.float()[symbols]
    return q


def positions(shape):
    waves = _wave_order(*shape, PAD)
    return torch.from_numpy(np.concatenate(waves).astype(np.int32))


def ref_logits(pc, q_pad, pos, dtype):
    """(n, L) logits at pos: the masked convs run fully convolutionally over
    the padded buffer on the CPU in `dtype`."""
    def conv(x, m, relu):
        y = F.conv3d(x, (m.weight * m.mask).to(dtype), m.bias.to(dtype))
        return torch.relu(y) if relu else y
    with torch.no_grad():
        x = q_pad.to(dtype)[None, None]
        a0 = conv(x, pc.conv0, True)
        a1 = conv(a0, pc.res_conv1, True)
        a2 = conv(a1, pc.res_conv2, False) + a0[:, :, 2:, 2:-2, 2:-2]
        vol = conv(a2, pc.conv2, False)[0].permute(1, 2, 3, 0)
    p = pos.long()
    return vol[p[:, 0], p[:, 1], p[:, 2]].contiguous()


def fp64_table(logits):
    L = logits.shape[1]
    return torch.floor(torch.softmax(logits.double(), dim=1)
                       * (65536 - L)).long().clamp(min=1)


def bits(t):
    return t.contiguous().view(torch.int32)


def load_golden():
    """-> (pc, centers, symbols (3,5,6) int64, stream bytes)."""
    z = np.load(GOLDEN)
    pc = make_pc(L=6, k=8, centers_pad=True, seed=0)
    with torch.no_grad():
        for name in LAYERS:
            m = getattr(pc, name)
            m.weight.copy_(torch.from_numpy(z[name + "_weight"]))
            m.bias.copy_(torch.from_numpy(z[name + "_bias"]))
    return (pc, torch.from_numpy(z["centers"]),
            torch.from_numpy(z["symbols"]), z["stream"].tobytes())
