"""fp8 inference path (BASELINE config 5): OCP e4m3 activations and weights on
the fp8 MFMA conv kernel, ij encoding for the 1-channel layers; and the pin
list that keeps cached fp8 operands alive for a captured HIP graph (shared
with the fused e4m3 kernel of ``fused``)."""
from __future__ import annotations

import numpy as np
import torch
import torch.utils.weak as _weak

from .. import _ext
from ..packing import ij_groups, ij_in_weights, ij_out_weights, pack_w16, pack_w16_planes
from .layers import _pad_bias, _std, ijpack, symmetric_1ch

FP8 = torch.float8_e4m3fn


def _fp8_weights(packed_bf16: torch.Tensor):
    """Packed bf16 fragments -> (fp8 fragments scaled into the e4m3 range, 1/scale)."""
    amax = float(packed_bf16.abs().max())
    e = 0 if amax == 0 else int(np.floor(np.log2(240.0 / amax)))
    e = max(-8, min(12, e))
    return (packed_bf16.float() * 2.0 ** e).to(FP8), 2.0 ** -e


# weight tensor -> {kind: (version, shape, (fp8 fragments, 1/scale))}.  Keyed by
# the tensor OBJECT (entries die with it), never by its address: a new weight
# tensor the caching allocator places where a freed one lived must not inherit
# its fp8 weights.
_FP8_W_CACHE = _weak.WeakIdKeyDictionary()
# rebound by pin_fp8_weights: every reader goes through pin() below
_FP8_PINS: list | None = None


class pin_fp8_weights:
    """Collects every cached fp8 weight tensor used inside the block (returned
    by ``__enter__``): a HIP graph captured there replays those exact buffers,
    so its owner keeps them alive for as long as the graph exists
    (eval/inloc.py PairMatcher)."""

    def __enter__(self):
        global _FP8_PINS
        self._prev, _FP8_PINS = _FP8_PINS, []
        return _FP8_PINS

    def __exit__(self, *exc):
        global _FP8_PINS
        _FP8_PINS = self._prev
        return False


def pin(tensors) -> None:
    """Hand cached fp8 operands that a launch is about to read to the
    enclosing ``pin_fp8_weights`` block, if there is one."""
    if _FP8_PINS is not None:
        _FP8_PINS.extend(tensors)


def _fp8_weights_of(w_ref: torch.Tensor, kind: str):
    """Quantised fp8 fragments of one layer's weights, cached per weight tensor
    and version: the amax -> scale step reads the max on the host, which must
    not happen per pair (it serialises the stream and is illegal inside the
    InLoc PairMatcher HIP-graph capture).  Pass the weight Parameter itself
    (``Conv4d.weight`` with ``pre_permuted_filters=True``, the default) for the
    cache to hit across calls; a fresh tensor per call is re-quantised."""
    per = _FP8_W_CACHE.get(w_ref)
    if per is None:
        per = _FP8_W_CACHE[w_ref] = {}
    ent = per.get(kind)
    ver = 0 if w_ref.is_inference() else w_ref._version      # inference tensors are immutable
    if ent is None or ent[0] != ver or ent[1] != tuple(w_ref.shape):
        w = _std(w_ref)
        packed = {"1in": lambda: pack_w16_planes(ij_in_weights(w)), "16": lambda: pack_w16(w),
                  "1out": lambda: pack_w16_planes(ij_out_weights(w))}[kind]()
        ent = per[kind] = (ver, tuple(w_ref.shape), _fp8_weights(packed))
    pin((ent[2][0],))
    return ent[2]


def _stack_fwd_fp8(x0: torch.Tensor, ws, bs, kinds) -> torch.Tensor:
    """x0 [V,I,J,K,L] bf16 -> last layer output fp32 [V,I,J,K,L] (ReLU'd), fp8 inside."""
    C = _ext.ext()
    V, I, J, K, L = x0.shape
    h = x0
    for li, (w_ref, b, kind) in enumerate(zip(ws, bs, kinds)):
        ks = w_ref.shape[0]
        wq, osc = _fp8_weights_of(w_ref, kind)
        if kind == "1in":
            xs = ijpack(C, h, ks, 1, FP8)
            y = torch.empty((V, I, J, K, L, 16), dtype=FP8, device=x0.device)
            C.conv16f8_fwd(xs, wq, _pad_bias(b, 16), y, ks, 1, osc)
        elif kind == "16":
            y = torch.empty((V, I, J, K, L, 16), dtype=FP8, device=x0.device)
            C.conv16f8_fwd(h, wq, _pad_bias(b, 16), y, ks, 1, osc)
        else:  # "1out"
            G, nq = ij_groups(ks), ks * ks
            z = torch.empty((nq, V, I, J, K, L), dtype=torch.float32, device=x0.device)
            hx = h.unsqueeze(0)
            for gi in range(G):
                C.conv16f8_fwd(hx, wq[gi:gi + 1], None, z[16 * gi:min(nq, 16 * gi + 16)], ks, 4, osc)
            y = torch.empty((V, I, J, K, L), dtype=torch.float32, device=x0.device)
            C.ijsum(z, _pad_bias(b, 1), y, ks, 1, 1)
            del z
            if li != len(kinds) - 1:
                raise RuntimeError("fp8 NC path: the 1-channel output layer must be last")
        h = y
    return h


def neigh_consensus_fp8(x: torch.Tensor, weights, biases, kinds, symmetric: bool = True) -> torch.Tensor:
    """Inference-only NeighConsensus with fp8 operands (no autograd)."""
    def run(xb):
        return _stack_fwd_fp8(xb, weights, biases, kinds)

    if symmetric:
        return symmetric_1ch(x, run)
    V, _, I, J, K, L = x.shape
    return run(x.reshape(V, I, J, K, L).to(torch.bfloat16).contiguous()).reshape(V, 1, I, J, K, L)
