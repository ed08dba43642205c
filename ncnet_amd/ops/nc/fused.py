"""Fused InLoc NC (csrc/nc_fused.hip): kernel sizes (3, 3), channels (<=16, 1),
inference.  The hidden activation stays in LDS; HBM sees the input and the
output volume once.  bf16 / float16 operands (``nc_fused_k3``) or e4m3
(``nc_fused_k3_f8``).  NCNET_NC_FUSED=0 falls back to the layer-by-layer path."""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.utils.weak as _weak

from .. import _ext
from ..packing import ij_in_weights, ij_out_weights, pack_w16_planes
from . import fp8 as _fp8
from .layers import _pad_bias, _std, combine_1ch, symmetric_1ch

_FUSED_LDS = 80 * 1024          # two workgroups per CU (160 KB LDS)


def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


@functools.lru_cache(maxsize=64)
def fused_tiles(V: int, I: int, J: int, K: int, L: int):
    """(TK, TL, R, IR) of nc_fused_k3: a (k, l) tile within the kernel's limits
    ((TK+2)(TL+2) <= 512, TK*TL <= 384, (TK+4)(TL+4) <= 512) minimising the
    padded layer-1 + layer-2 work, then R output planes per workgroup (as many
    as the LDS ring allows) and row segments of IR rows until the grid has
    ~2 workgroups per CU."""
    best = None
    for tk in range(1, min(K, 28) + 1):
        for tl in range(1, min(L, 28) + 1):
            if (tk + 2) * (tl + 2) > 512 or tk * tl > 384 or (tk + 4) * (tl + 4) > 512:
                continue
            n = _cdiv(K, tk) * _cdiv(L, tl)
            cost = n * (_cdiv((tk + 2) * (tl + 2), 16) + _cdiv(tk * tl, 16))
            if best is None or cost < best[0]:
                best = (cost, tk, tl)
    _, tk, tl = best
    fixed = (tk + 4) * (tl + 10) * 32 + (tk + 2) * (tl + 8) * 32 + 2 * 5 * 64 * 16 + 268   # + ring trash / alignment
    rps = tk * tl + (16 - (tk * tl) % 32) % 32        # ring plane stride (csrc/nc_fused.hip ncf_ring_stride)
    r_max = max(1, (_FUSED_LDS - fixed) // (12 * rps))
    base = V * _cdiv(K, tk) * _cdiv(L, tl)

    def nwg(r, ir):
        return base * _cdiv(J, r) * _cdiv(I, ir)

    # the kernel is latency-bound (two barriers per hidden plane): prefer >= ~500
    # workgroups (two per CU), first by splitting rows (halo (IR+2)/IR), then
    # planes ((R+2)/R).  Measured at 3200 px: 500 workgroups (R=10, IR=75)
    # 4.3 ms vs 6.4 ms for 1000 (IR=37); at 1600 px R=4, IR=5 0.55 ms.
    R, IR = min(J, r_max), I
    while nwg(R, IR) < 500 and IR > 5:
        IR = max(5, IR // 2)
    while nwg(R, IR) < 500 and R > 4:
        R -= 1
    return tk, tl, R, IR


def _layer2_rows(w2: torch.Tensor) -> torch.Tensor:
    """Layer-2 MFMA rows: row 4 * dj + di <- ij combo di * 3 + dj (nc_fused.hip: a
    lane's four rows then share dj and one output plane); other rows zero."""
    wo = ij_out_weights(w2)
    wr = torch.zeros_like(wo)
    for di in range(3):
        for dj in range(3):
            wr[:, 4 * dj + di] = wo[:, 3 * di + dj]
    return wr


def _fused_weights(weights, biases, dtype=torch.bfloat16):
    """Packed fused-kernel weights in the operand dtype (bf16, or float16 for the
    IEEE-half kernel of half_precision models)."""
    w1, w2 = _std(weights[0]), _std(weights[1])
    W1p = pack_w16_planes(ij_in_weights(w1), dtype)[0].contiguous()
    W2p = pack_w16_planes(_layer2_rows(w2), dtype)[0].contiguous()
    return W1p, _pad_bias(biases[0], 16), W2p, _pad_bias(biases[1], 1)


def _run_fused(xb: torch.Tensor, wts) -> torch.Tensor:
    V, I, J, K, L = xb.shape
    y = torch.empty((V, I, J, K, L), dtype=torch.float32, device=xb.device)
    tk, tl, R, IR = fused_tiles(V, I, J, K, L)
    _ext.ext().nc_fused_k3(xb, *wts, y, R, IR, tk, tl)
    return y


def neigh_consensus_fused_x2(x2: torch.Tensor, weights, biases) -> torch.Tensor:
    """Symmetric fused NC on a prepared [2V, I, J, K, L] bf16 / float16 input (x,
    then its A<->B swap: ops/mutual.py mutual_matching_nc_input) -> [V, 1, I, J, K, L] fp32."""
    V2, I, J, K, L = x2.shape
    z = _run_fused(x2, _fused_weights(weights, biases, x2.dtype))
    return combine_1ch(z, (V2 // 2, I, J, K, L))


def neigh_consensus_fused(x: torch.Tensor, weights, biases, symmetric: bool = True) -> torch.Tensor:
    """Inference NeighConsensus of a (3, 3) / (<=16, 1) stack on the fused kernel."""
    wts = _fused_weights(weights, biases)
    if symmetric:
        return symmetric_1ch(x, lambda xb: _run_fused(xb, wts))
    V, _, I, J, K, L = x.shape
    return _run_fused(x.reshape(V, I, J, K, L).to(torch.bfloat16).contiguous(), wts).reshape(V, 1, I, J, K, L)


# fused fp8 kernel (csrc/nc_fused.hip nc_fused_k3_f8_kernel): x0 (in [0, 1]
# after MutualMatching) enters e4m3 times this power of two
FP8_NC_X_SCALE = 256.0


def _pow2_scale(bound: float, target: float) -> float:
    """2^e with bound * 2^e <= target (e clamped to [-10, 12]); 1 for bound 0."""
    if not bound > 0:
        return 1.0
    return 2.0 ** max(-10, min(12, int(np.floor(np.log2(target / bound)))))


def _mx_frags(dense: torch.Tensor):
    """[16 rows, 9 taps, 16 ch] -> (A fragments of taps 0-7 for
    v_mfma_scale_f32_16x16x128_f8f6f4: [64 lanes, 32] with lane fr + 16 fq
    holding row fr, taps 2fq, 2fq + 1; tap-8 fragments for
    v_mfma_f32_16x16x32_fp8_fp8: [64, 8], lane groups fq = 0, 1 channels
    0-7 / 8-15, fq = 2, 3 zero)."""
    a = dense[:, :8, :].reshape(16, 4, 32).permute(1, 0, 2).reshape(64, 32)
    b = dense.new_zeros((4, 16, 8))
    b[:2] = dense[:, 8, :].reshape(16, 2, 8).permute(1, 0, 2)
    return a.contiguous(), b.reshape(64, 8).contiguous()


def _fused_weights_f8_build(weights, biases):
    w1, w2 = _std(weights[0]).float(), _std(weights[1]).float()
    d1 = ij_in_weights(w1)[0].reshape(16, 16, 9).permute(0, 2, 1)          # [hidden co, tap, combo]
    d2 = _layer2_rows(w2)[0].reshape(16, 16, 9).permute(0, 2, 1)           # [combo row, tap, hidden ci]
    b1, b2 = _pad_bias(biases[0], 16), _pad_bias(biases[1], 1)
    sw1 = _pow2_scale(float(d1.abs().max()), 240.0)
    sw2 = _pow2_scale(float(d2.abs().max()), 240.0)
    # hidden bound: x0 <= 1, so h[co] <= sum |W1[co]| + max(b1[co], 0)
    hb = float((d1.abs().sum((1, 2)) + b1.clamp(min=0)).max())
    sh = _pow2_scale(hb, 440.0)
    sx = FP8_NC_X_SCALE
    w1a, w1b = _mx_frags(d1 * sw1)
    w2a, w2b = _mx_frags(d2 * sw2)
    tens = tuple(t.to(_fp8.FP8) for t in (w1a, w1b)) + (b1,) + tuple(t.to(_fp8.FP8) for t in (w2a, w2b)) + (b2,)
    return tens, (sx, 1.0 / (sw1 * sx), sh, 1.0 / (sw2 * sh))


_F8_FUSED_CACHE = _weak.WeakIdKeyDictionary()


def _fused_weights_f8(weights, biases):
    """Quantised fused-kernel operands, cached per layer-1 weight tensor and the
    versions of all four parameters (the amax / bound reads are host syncs,
    illegal inside the InLoc pair-graph capture).  Handed to the enclosing
    ``pin_fp8_weights`` block: a captured pair graph replays these buffers."""
    def ver(t):
        return 0 if t.is_inference() else t._version
    key = tuple((ver(t), tuple(t.shape)) for t in (*weights, *biases))
    ent = _F8_FUSED_CACHE.get(weights[0])
    if ent is None or ent[0] != key or ent[1] is not weights[1]:
        ent = _F8_FUSED_CACHE[weights[0]] = (key, weights[1], _fused_weights_f8_build(weights, biases))
    _fp8.pin(ent[2][0])
    return ent[2]


def neigh_consensus_fused_x2_fp8(x2: torch.Tensor, weights, biases) -> torch.Tensor:
    """Symmetric fused NC on e4m3 operands (nc_fused_k3_f8) on a prepared
    [2V, I, J, K, L] bf16 input -> [V, 1, I, J, K, L] fp32."""
    V2, I, J, K, L = x2.shape
    tens, scales = _fused_weights_f8(weights, biases)
    z = torch.empty((V2, I, J, K, L), dtype=torch.float32, device=x2.device)
    tk, tl, R, IR = fused_tiles(V2, I, J, K, L)
    _ext.ext().nc_fused_k3_f8(x2, *tens, z, R, IR, tk, tl, *scales)
    return combine_1ch(z, (V2 // 2, I, J, K, L))
