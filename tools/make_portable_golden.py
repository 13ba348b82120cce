"""Write tests/golden/portable_k8_L6.npz, the fixture that pins the portable
codec stream (container backend id 2) across commits and machines.

    python tools/make_portable_golden.py [out.npz]

It holds a seeded probclass (k=8, L=6: weight and bias of conv0, res_conv1,
res_conv2 and conv2), the centers, a (3, 5, 6) symbol volume and the bytes
the portable backend's host build (CPU) writes for it. Run it only when the
format is changed on purpose: tests/test_portable_codec.py requires the
committed stream to decode and to be reproduced byte for byte, on the CPU
and on the GPU.
"""

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from dsin_amd import config as config_mod
from dsin_amd.coding import decode_symbols, encode_symbols
from dsin_amd.models.probclass import ProbClass

K, L, SHAPE = 8, 6, (3, 5, 6)
LAYERS = ("conv0", "res_conv1", "res_conv2", "conv2")


def make_pc(k: int = K, num_centers: int = L) -> ProbClass:
    cfg, _ = config_mod.parse(os.path.join(ROOT, "run_configs",
                                           "pc_run_configs"))
    cfg.arch_param__k = k
    cfg.use_centers_for_padding = True
    return ProbClass(cfg, num_centers=num_centers)


def main() -> None:
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(
        ROOT, "tests", "golden", "portable_k8_L6.npz")
    torch.manual_seed(2024)
    pc = make_pc()
    with torch.no_grad():
        for name in LAYERS:
            getattr(pc, name).bias.uniform_(-0.2, 0.2)
    centers = torch.linspace(-2, 2, L)
    g = torch.Generator().manual_seed(7)
    symbols = torch.randint(0, L, SHAPE, generator=g)
    data = encode_symbols(pc, centers, symbols, backend="portable")
    back = decode_symbols(pc, centers, data, SHAPE, backend="portable")
    assert torch.equal(back, symbols)
    arrays = {"centers": centers.numpy(),
              "symbols": symbols.numpy().astype(np.int64),
              "stream": np.frombuffer(data, dtype=np.uint8)}
    for name in LAYERS:
        m = getattr(pc, name)
        arrays[name + "_weight"] = m.weight.detach().numpy()
        arrays[name + "_bias"] = m.bias.detach().numpy()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, **arrays)
    print(f"{out}: {os.path.getsize(out)} bytes, stream of {len(data)} bytes")


if __name__ == "__main__":
    main()
