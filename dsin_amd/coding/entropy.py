"""Entropy-coding bridge between the probclass network and the range coder.

Re-provides (and completes) the reference's arithmetic-coding hooks
(/root/reference/src/probclass_imgcomp.py:361-482):

* :class:`ProbclassTesting` — total bit cost computed fully convolutionally
  from a symbol volume (mirror of ProbclassNetworkTesting, :393-421);
* :class:`PredictionNetwork` — per-position next-symbol frequency tables
  from a causal context block (mirror of :425-482);
* :func:`encode_symbols` / :func:`decode_symbols` — an actual working codec
  the reference never shipped.

Codec design (beyond the reference's anticipated per-pixel loop): the causal
mask admits a *skewed wavefront* schedule. Position (c, h, w) depends only on
positions with strictly smaller t = 25c + 5h + w (the skew constants follow
from the context half-width pad=4: within a plane the farthest same-row-above
dependency is (h-1, w+4), so the h-skew must exceed 4; across planes the
farthest is (c-1, h+4, w+4), so the c-skew must exceed 5*4+4). All positions
sharing one t are conditionally independent given earlier symbols, so the
autoregressive decode batches each wave through ONE network call —
O(25C + 5H + W) calls instead of O(C*H*W). The encoder runs the *identical*
per-wave batched computation (same batch shapes, same block contents at every
causal position; non-causal positions differ but are multiplied by
exactly-0.0 masked weights), so encoder and decoder frequency tables are
bit-identical by construction — no cross-pass float-equality assumption.

Padding: contexts are gathered from a *value* buffer initialized to the
configured pad value (centers[0] when use_centers_for_padding, else 0.0 —
reference :59-61, pc_run_configs:23), so both paths see identical borders in
either config.
"""

from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..models.probclass import ProbClass
from .range_coder import RangeDecoder, RangeEncoder, _cumulate

FREQ_RESOLUTION = 1 << 16


def _pad_value(pc: ProbClass, centers: torch.Tensor) -> torch.Tensor:
    """Scalar pad value per config (reference probclass_imgcomp.py:59-61)."""
    if pc.config.use_centers_for_padding:
        return centers[0]
    return torch.zeros((), device=centers.device, dtype=centers.dtype)


class ProbclassTesting:
    """Total bit cost from a symbol volume, fully convolutionally
    (reference :393-421: q = centers[symbols], then the standard bitcost)."""

    def __init__(self, pc: ProbClass, centers: torch.Tensor):
        self.pc = pc
        self.centers = centers

    @torch.no_grad()
    def total_bit_cost(self, symbols: torch.Tensor) -> float:
        if symbols.dim() == 3:
            symbols = symbols.unsqueeze(0)
        q = self.centers[symbols]
        bc = self.pc.bitcost(q.float(), symbols,
                             _pad_value(self.pc, self.centers))
        return float(bc.sum())


class PredictionNetwork:
    """Per-pixel next-symbol frequencies for the range coder
    (reference :425-482). Context is a (D, H, W) = context_shape block; the
    center-front position is the one being predicted."""

    def __init__(self, pc: ProbClass, centers: torch.Tensor,
                 freqs_resolution: int = FREQ_RESOLUTION):
        self.pc = pc
        self.centers = centers
        self.res = freqs_resolution
        cs = pc.context_size()
        self.context_shape = (cs // 2 + 1, cs, cs)

    @torch.no_grad()
    def probs_q(self, q_blocks: torch.Tensor) -> torch.Tensor:
        """q_blocks: (B, D, H, W) float value contexts -> (B, L) probs."""
        logits = self.pc.logits(q_blocks.unsqueeze(1))      # (B,L,1,1,1)
        return torch.softmax(logits[:, :, 0, 0, 0].float(), dim=1)

    @torch.no_grad()
    def freqs_q(self, q_blocks: torch.Tensor) -> np.ndarray:
        """(B, D, H, W) value contexts -> (B, L) integer frequency tables."""
        f = (self.probs_q(q_blocks) * self.res).long().clamp(min=1)
        return f.cpu().numpy()

    @torch.no_grad()
    def probs(self, ctx_symbols: torch.Tensor) -> torch.Tensor:
        """ctx_symbols: (D, H, W) int64 context -> (L,) probabilities.
        Symbol-context variant; caller guarantees pad positions hold the
        symbol whose center equals the configured pad value."""
        q = self.centers[ctx_symbols].float()
        return self.probs_q(q.unsqueeze(0))[0]

    @torch.no_grad()
    def freqs(self, ctx_symbols: torch.Tensor) -> np.ndarray:
        f = (self.probs(ctx_symbols) * self.res).long().clamp(min=1)
        return f.cpu().numpy()


def _wave_order(C: int, H: int, W: int, pad: int
                ) -> List[np.ndarray]:
    """Positions grouped by wave t = Kc*c + Kh*h + w with Kh = pad+1 and
    Kc = Kh*pad + pad + 1; each group is an (n, 3) int array sorted by
    (c, h, w). Every dependency of a position lands in a strictly earlier
    wave (see module docstring)."""
    Kh = pad + 1
    Kc = Kh * pad + pad + 1
    c, h, w = np.meshgrid(np.arange(C), np.arange(H), np.arange(W),
                          indexing="ij")
    pos = np.stack([c.ravel(), h.ravel(), w.ravel()], axis=1)
    t = Kc * pos[:, 0] + Kh * pos[:, 1] + pos[:, 2]
    # sort by (t, c, h, w) -> stable wave-major order
    order = np.lexsort((pos[:, 2], pos[:, 1], pos[:, 0], t))
    pos, t = pos[order], t[order]
    cuts = np.flatnonzero(np.diff(t)) + 1
    return np.split(pos, cuts)


def _gather_blocks(q_pad: torch.Tensor, wave: np.ndarray,
                   Dc: int, Hc: int, Wc: int) -> torch.Tensor:
    """(B, Dc, Hc, Wc) context blocks at the padded-buffer offsets of one
    wave. q_pad is (C+Dc-1, H+Hc-1, W+Wc-1); position (c,h,w)'s block starts
    at (c, h, w) in the padded buffer."""
    blocks = [q_pad[c:c + Dc, h:h + Hc, w:w + Wc] for c, h, w in wave]
    return torch.stack(blocks)


BACKENDS = ("torch", "hip", "portable")


def _check_backend(backend: str) -> None:
    if backend not in BACKENDS:
        raise ValueError(f"backend must be one of {BACKENDS}, got {backend!r}")


def _torch_backend_cache_reset(device: torch.device) -> None:
    """The torch backend on a GPU runs four masked convs per wave, each on a
    fresh weight*mask temporary that the W-panel cache would pin; drop the
    cache around a call so a decode does not grow it without bound."""
    if device.type == "cuda":
        from ..ops import conv as _conv
        _conv.begin_step()


def _hip_setup(pc: ProbClass, centers: torch.Tensor, B: int, shape, device,
               portable: bool = False):
    """Checks + the pad-filled value buffers (B, C+4, H+8, W+8), wave-ordered
    positions and wave offsets shared by the hip / portable encoder and
    decoder."""
    from .. import ops
    ops.check_pc_shape(pc)
    name = "portable" if portable else "hip"
    if device.type != "cuda" and not portable:
        raise ValueError("backend='hip' needs the model and symbols on a GPU")
    C, H, W = (int(v) for v in shape)
    if min(C, H, W) < 1:
        raise ValueError(f"backend={name!r}: empty symbol volume {shape}")
    pad = pc.context_size() // 2
    waves = _wave_order(C, H, W, pad)
    pos = torch.from_numpy(np.concatenate(waves).astype(np.int32)).to(device)
    offsets = np.concatenate([[0], np.cumsum([len(w) for w in waves])])
    q_pad = torch.full((B, C + pad, H + 2 * pad, W + 2 * pad),
                       float(_pad_value(pc, centers)),
                       dtype=torch.float32, device=device)
    return ops, pad, pos, offsets, q_pad


def _encode_symbols_hip_batch(pc, centers, symbols,
                              portable=False) -> List[bytes]:
    dev = centers.device
    B, C, H, W = symbols.shape
    ops, pad, pos, _, q_pad = _hip_setup(pc, centers, B, (C, H, W), dev,
                                         portable)
    sym = symbols.to(dev)
    q_pad[:, pad:, pad:H + pad, pad:W + pad] = centers.float()[sym]
    p = pos.long()
    return ops.pc_encode_batch(pc, q_pad, pos,
                               sym[:, p[:, 0], p[:, 1], p[:, 2]],
                               portable=portable)


def _decode_symbols_hip_batch(pc, centers, datas, shape, device,
                              portable=False) -> torch.Tensor:
    ops, _, pos, offsets, q_pad = _hip_setup(pc, centers, len(datas), shape,
                                             device, portable)
    return ops.pc_decode_batch(pc, q_pad, pos, offsets, datas, centers,
                               portable=portable)


@torch.no_grad()
def encode_symbols_batch(pc: ProbClass, centers: torch.Tensor,
                         symbols: torch.Tensor, backend: str = "torch"
                         ) -> List[bytes]:
    """symbols: (B, C, H, W) int64 -> B byte streams; element b is what
    encode_symbols gives for symbols[b] with the same backend, so either
    decoder reads it. "hip" and "portable" code the whole batch in one pass
    of the batched kernels (ops.pc_encode_batch): the images share the wave
    schedule and each has a range coder of its own. "torch" loops over the
    images. An empty batch is a ValueError."""
    _check_backend(backend)
    if symbols.dim() != 4:
        raise ValueError(f"encode_symbols_batch: symbols must be (B, C, H, "
                         f"W), got {tuple(symbols.shape)}")
    if symbols.shape[0] < 1:
        raise ValueError("encode_symbols_batch: empty batch")
    if backend in ("hip", "portable"):
        return _encode_symbols_hip_batch(pc, centers, symbols,
                                         portable=backend == "portable")
    return [encode_symbols(pc, centers, s, backend=backend) for s in symbols]


@torch.no_grad()
def decode_symbols_batch(pc: ProbClass, centers: torch.Tensor,
                         datas: Sequence[bytes],
                         shape: Tuple[int, int, int],
                         device: Optional[torch.device] = None,
                         backend: str = "torch") -> torch.Tensor:
    """Inverse of encode_symbols_batch: B streams of one (C, H, W) shape ->
    (B, C, H, W) int64. The streams may come from encode_symbols_batch or
    from B encode_symbols calls. "hip" and "portable" decode all images in
    one wave loop (ops.pc_decode_batch: one state init plus two launches per
    wave for any B); "torch" loops over the images. A short stream decodes
    as decode_symbols decodes it, reading zeros past its own end."""
    _check_backend(backend)
    datas = list(datas)
    if len(datas) < 1:
        raise ValueError("decode_symbols_batch: empty batch")
    if len(shape) != 3:
        raise ValueError(f"decode_symbols_batch: shape must be (C, H, W), "
                         f"got {tuple(shape)}")
    device = torch.device(device or centers.device)
    if backend in ("hip", "portable"):
        return _decode_symbols_hip_batch(pc, centers, datas, shape, device,
                                         portable=backend == "portable")
    return torch.stack([decode_symbols(pc, centers, d, shape, device=device,
                                       backend=backend) for d in datas])


def _ragged_setup(pc: ProbClass, centers: torch.Tensor, shapes, device,
                  portable: bool):
    """Checks + what the hip / portable ragged encoder and decoder share:
    the wave-ordered positions and wave numbers of every distinct shape
    (_wave_order runs once per shape), the descriptor rows (C, H, W, volume
    offset, symbol offset) and the pad-filled flat value buffer."""
    from .. import ops
    ops.check_pc_shape(pc)
    name = "portable" if portable else "hip"
    if device.type != "cuda" and not portable:
        raise ValueError("backend='hip' needs the model and symbols on a GPU")
    pad = pc.context_size() // 2
    Kh = pad + 1
    Kc = Kh * pad + pad + 1
    orders, desc, q_off, s_off = {}, [], 0, 0
    for shape in shapes:
        C, H, W = shape
        if min(C, H, W) < 1:
            raise ValueError(f"backend={name!r}: empty symbol volume {shape}")
        if shape not in orders:
            pos = np.concatenate(_wave_order(C, H, W, pad)).astype(np.int32)
            orders[shape] = (pos, Kc * pos[:, 0] + Kh * pos[:, 1] + pos[:, 2])
        desc.append((C, H, W, q_off, s_off))
        q_off += (C + pad) * (H + 2 * pad) * (W + 2 * pad)
        s_off += C * H * W
    q = torch.full((q_off,), float(_pad_value(pc, centers)),
                   dtype=torch.float32, device=device)
    return ops, pad, orders, desc, q


def _ragged_items(shapes, orders) -> np.ndarray:
    """(n, 4) int32 items (b, c, h, w): image after image, each in its own
    wave order, which is the encoder's order (b, t, c, h, w)."""
    return np.concatenate([
        np.concatenate([np.full((len(orders[s][0]), 1), b, np.int32),
                        orders[s][0]], axis=1)
        for b, s in enumerate(shapes)])


def _encode_symbols_hip_ragged(pc, centers, symbols, portable) -> List[bytes]:
    dev = centers.device
    shapes = [tuple(int(v) for v in s.shape) for s in symbols]
    ops, pad, orders, desc, q = _ragged_setup(pc, centers, shapes, dev,
                                              portable)
    cen = centers.float()
    index = {s: torch.from_numpy(o[0]).to(dev).long()
             for s, o in orders.items()}
    syms, starts = [], [0]
    for sym, shape, (C, H, W, q_off, _) in zip(symbols, shapes, desc):
        sym = sym.to(dev)
        vol = q[q_off:q_off + (C + pad) * (H + 2 * pad) * (W + 2 * pad)]
        vol.view(C + pad, H + 2 * pad, W + 2 * pad)[
            pad:, pad:H + pad, pad:W + pad] = cen[sym]
        p = index[shape]
        syms.append(sym[p[:, 0], p[:, 1], p[:, 2]])
        starts.append(starts[-1] + p.shape[0])
    items = torch.from_numpy(_ragged_items(shapes, orders)).to(dev)
    return ops.pc_encode_ragged(pc, q, desc, items, starts, torch.cat(syms),
                                portable=portable)


def _decode_symbols_hip_ragged(pc, centers, datas, shapes, device,
                               portable) -> List[torch.Tensor]:
    ops, _, orders, desc, q = _ragged_setup(pc, centers, shapes, device,
                                            portable)
    B = len(shapes)
    items = _ragged_items(shapes, orders)
    t = np.concatenate([orders[s][1] for s in shapes]).astype(np.int64)
    # images are in order and each is sorted by (t, c, h, w): a stable sort
    # by t gives (t, b, c, h, w)
    order = np.argsort(t, kind="stable")
    items, t = items[order], t[order]
    T = int(t[-1]) + 1
    counts = np.bincount(t * B + items[:, 0], minlength=T * B)
    seg = np.concatenate([[0], np.cumsum(counts)])
    out = ops.pc_decode_ragged(pc, q, desc, torch.from_numpy(items).to(device),
                               seg.tolist(), datas, centers,
                               portable=portable)
    return [out[so:so + C * H * W].view(C, H, W)
            for C, H, W, _, so in desc]


def _ragged_shapes(what: str, shapes) -> List[Tuple[int, int, int]]:
    out = []
    for s in shapes:
        if len(s) != 3:
            raise ValueError(f"{what}: every volume must be (C, H, W), got "
                             f"{tuple(s)}")
        out.append(tuple(int(v) for v in s))
    if not out:
        raise ValueError(f"{what}: empty batch")
    return out


@torch.no_grad()
def encode_symbols_ragged(pc: ProbClass, centers: torch.Tensor,
                          symbols: Sequence[torch.Tensor],
                          backend: str = "torch") -> List[bytes]:
    """symbols: B int64 volumes (C_b, H_b, W_b) whose shapes may all differ
    -> B byte streams; element b is what encode_symbols gives for symbols[b]
    with the same backend. "hip" and "portable" code the whole list in one
    pass of the ragged kernels (ops.pc_encode_ragged, two launches); "torch"
    loops over the images. An empty list or a volume that is not 3-D is a
    ValueError."""
    _check_backend(backend)
    symbols = list(symbols)
    _ragged_shapes("encode_symbols_ragged", [s.shape for s in symbols])
    if backend in ("hip", "portable"):
        return _encode_symbols_hip_ragged(pc, centers, symbols,
                                          portable=backend == "portable")
    return [encode_symbols(pc, centers, s, backend=backend) for s in symbols]


@torch.no_grad()
def decode_symbols_ragged(pc: ProbClass, centers: torch.Tensor,
                          datas: Sequence[bytes],
                          shapes: Sequence[Tuple[int, int, int]],
                          device: Optional[torch.device] = None,
                          backend: str = "torch") -> List[torch.Tensor]:
    """Inverse of encode_symbols_ragged: stream b holds a (C, H, W) =
    shapes[b] volume -> B int64 tensors. The streams may come from
    encode_symbols_ragged, encode_symbols_batch or encode_symbols. "hip" and
    "portable" decode all images in one wave loop over the merged schedule
    (ops.pc_decode_ragged: the images walk one wave counter, the smaller
    ones finish early); "torch" loops over the images. A short stream
    decodes as decode_symbols decodes it. An empty list, a shape that is not
    (C, H, W) or len(datas) != len(shapes) is a ValueError."""
    _check_backend(backend)
    datas = list(datas)
    shapes = _ragged_shapes("decode_symbols_ragged", list(shapes))
    if len(datas) != len(shapes):
        raise ValueError(f"decode_symbols_ragged: {len(datas)} streams for "
                         f"{len(shapes)} shapes")
    device = torch.device(device or centers.device)
    if backend in ("hip", "portable"):
        return _decode_symbols_hip_ragged(pc, centers, datas, shapes, device,
                                          portable=backend == "portable")
    return [decode_symbols(pc, centers, d, s, device=device, backend=backend)
            for d, s in zip(datas, shapes)]


@torch.no_grad()
def encode_symbols(pc: ProbClass, centers: torch.Tensor,
                   symbols: torch.Tensor, backend: str = "torch") -> bytes:
    """symbols: (C, H, W) int64 -> range-coded byte stream, wave order.

    backend="torch" (default): the per-wave torch path below, on any device.
    backend="hip": the device-resident codec (a batch of one through
    ops.pc_encode_batch; GPU only). The
    two backends do not decode each other's streams: their tables differ
    (fp32 kernels and a 65536-L table scale against the torch convs and a
    65536 scale).
    backend="portable": the specification of ops/csrc/pc_model.h, run by the
    HIP kernels when centers are on a GPU and by the extension's host build
    when they are on the CPU. Both give the same bytes and each decodes the
    other's stream; "torch" and "hip" streams stay apart from it.

    Frequencies are computed through the SAME per-wave batched network
    calls the decoder runs — same batch shapes, same block contents at
    every causal position — so the roundtrip is bit-exact by construction.
    (A one-conv-pass "fast" encoder was measured to disagree with the
    per-wave decoder floats by +-1 freq even on a deterministic CPU
    backend — different reduction shapes — and was removed: a codec whose
    streams sometimes fail to decode is worse than no fast path.)
    """
    _check_backend(backend)
    if backend in ("hip", "portable"):
        return _encode_symbols_hip_batch(pc, centers, symbols[None],
                                         portable=backend == "portable")[0]
    sym = symbols.cpu().numpy()
    C, H, W = sym.shape
    pad = pc.context_size() // 2
    Dc, Hc, Wc = pad + 1, 2 * pad + 1, 2 * pad + 1
    enc = RangeEncoder()
    pred = PredictionNetwork(pc, centers)
    dev = centers.device
    _torch_backend_cache_reset(dev)
    # ground-truth value buffer: causal reads see the same values the
    # decoder will have reconstructed; non-causal positions hold ground
    # truth here vs the pad value on the decoder side, but every non-causal
    # tap is multiplied by an exactly-0.0 masked weight, so the per-wave
    # network outputs are bit-identical anyway (module docstring).
    q_pad = torch.full((C + Dc - 1, H + Hc - 1, W + Wc - 1),
                       float(_pad_value(pc, centers)),
                       dtype=torch.float32, device=dev)
    q_pad[Dc - 1:, pad:H + pad, pad:W + pad] = \
        centers.float()[symbols.to(dev)]
    for wave in _wave_order(C, H, W, pad):
        fr = pred.freqs_q(_gather_blocks(q_pad, wave, Dc, Hc, Wc))
        for (c, h, w), f in zip(wave, fr):
            cum = _cumulate(f)
            s = int(sym[c, h, w])
            enc.encode(int(cum[s]), int(f[s]), int(cum[-1]))
    _torch_backend_cache_reset(dev)
    return enc.finish()


@torch.no_grad()
def decode_symbols(pc: ProbClass, centers: torch.Tensor, data: bytes,
                   shape: Tuple[int, int, int],
                   device: Optional[torch.device] = None,
                   backend: str = "torch") -> torch.Tensor:
    """Wavefront autoregressive decode of a (C, H, W) symbol volume. Exact
    inverse of encode_symbols with the same backend: one batched network
    call per skewed wave (O(25C + 5H + W) calls), then the wave's symbols
    are range-decoded sequentially against the batch's frequency tables.
    backend="hip" keeps both steps on the GPU (ops.pc_decode_batch, B = 1);
    backend="portable" does the same on a GPU and runs the host build on
    the CPU, and decodes a portable stream written on either."""
    _check_backend(backend)
    C, H, W = shape
    device = torch.device(device or centers.device)
    if backend in ("hip", "portable"):
        return _decode_symbols_hip_batch(pc, centers, [data], shape, device,
                                         portable=backend == "portable")[0]
    _torch_backend_cache_reset(device)
    pred = PredictionNetwork(pc, centers)
    pad = pc.context_size() // 2
    Dc, Hc, Wc = pad + 1, 2 * pad + 1, 2 * pad + 1
    q_pad = torch.full((C + Dc - 1, H + Hc - 1, W + Wc - 1),
                       float(_pad_value(pc, centers)),
                       dtype=torch.float32, device=device)
    out = torch.zeros(C, H, W, dtype=torch.int64)
    centers_f = centers.float().cpu().numpy()
    dec = RangeDecoder(data)
    for wave in _wave_order(C, H, W, pad):
        fr = pred.freqs_q(_gather_blocks(q_pad, wave, Dc, Hc, Wc))
        for (c, h, w), f in zip(wave, fr):
            cum = _cumulate(f)
            tot = int(cum[-1])
            target = dec.decode_cum(tot)
            s = int(np.searchsorted(cum, target, side="right") - 1)
            dec.decode_update(int(cum[s]), int(f[s]), tot)
            out[c, h, w] = s
            q_pad[c + Dc - 1, h + pad, w + pad] = float(centers_f[s])
    _torch_backend_cache_reset(device)
    return out.to(device)
