"""Weak-supervision score (train.py:110-156) with a fused HIP forward/backward.

All three normalisations of the reference (train.py:111-116) run on the same
single-pass HIP statistics (max, first argmax, and a sum) plus one
closed-form backward kernel:

* ``'softmax'`` (default): ``max_j softmax(x)_j = 1 / sum_j exp(x_j - max x)``,
  ``ds/dx_j = s (delta_{j, argmax} - softmax_j)``;
* ``'l1'``: ``max_j x_j / (sum x + eps) = max x / (sum x + eps)`` (eps 1e-4;
  the volumes are non-negative -- ReLU'd NC outputs after MutualMatching -- so
  the positive denominator keeps the argmax), ``ds/dx_j = delta_{j, argmax} / D - max / D^2``;
* ``None``: ``max x``, ``ds/dx_j = delta_{j, argmax}``.

``strong_loss_from_corr`` is the keypoint-supervised objective (an extension
beyond the reference; ``reference.keypoint_ce``) on the fused forward /
closed-form backward kernels of csrc/kploss.hip.

``warp_loss_from_corr`` is the dense correspondence objective of two warped
views of one image (``reference.dense_ce``) on the kernels of csrc/densece.hip
and the same single-pass statistics.

``LOSSES`` (at the end) describes the three as plain data for engine/trainer.py.
"""
from __future__ import annotations

import collections

import torch

from .. import config as _config
from . import _ext
from . import reference as ref


_NORM = {"softmax": 1, "l1": 2, None: 0}


def _row_col_stats(x3: torch.Tensor, norm: int):
    C = _ext.ext()
    V, R, Cc = x3.shape
    f = dict(dtype=torch.float32, device=x3.device)
    rmax, rse = torch.empty((V, R), **f), torch.empty((V, R), **f)
    cmax, cse = torch.empty((V, Cc), **f), torch.empty((V, Cc), **f)
    rarg = torch.empty((V, R), dtype=torch.int32, device=x3.device)
    carg = torch.empty((V, Cc), dtype=torch.int32, device=x3.device)
    sum_kind = {1: 1, 2: 2, 0: 0}[norm]
    # one pass for both directions (stats2d: any row length and alignment, scalar loads where 16-byte ones cannot be used)
    if not (_config.RUNTIME.stats2d and C.stats2d(x3, rmax, rarg, rse, cmax, carg, cse, sum_kind)):
        C.stats_rows(x3, rmax, rarg, rse if sum_kind else None, sum_kind)
        C.stats_cols(x3, cmax, carg, cse if sum_kind else None, sum_kind)
    if not sum_kind:
        rse.zero_()
        cse.zero_()
    return rmax, rarg, rse, cmax, carg, cse


class SoftmaxMaxScoreFn(torch.autograd.Function):
    """sum_v wr[v] * sum_rows s_row + wc[v] * sum_cols s_col, s = the max of the
    normalised row / column (norm 1 softmax, 2 l1, 0 None)."""

    @staticmethod
    def forward(ctx, x3, wr, wc, norm=1):
        x3 = x3.float().contiguous()
        st = _row_col_stats(x3, norm)
        rmax, rarg, rse, cmax, carg, cse = st
        # one launch for the weighted score sum (was 7 small PyTorch kernels on the step's critical path)
        val = torch.empty((), dtype=torch.float32, device=x3.device)
        _ext.ext().score_sum(rmax, rse, cmax, cse, wr.float().contiguous(), wc.float().contiguous(), val, norm,
                             ref.L1_EPS)
        ctx.norm = norm
        ctx.save_for_backward(x3, wr, wc, *st)
        return val

    @staticmethod
    def backward(ctx, g):
        x3, wr, wc, rmax, rarg, rse, cmax, carg, cse = ctx.saved_tensors
        gx = torch.empty_like(x3)
        # the incoming gradient scales inside the kernel (no extra pass over the volume)
        _ext.ext().softmax_max_bwd(x3, rmax, rarg, rse, cmax, carg, cse, wr.float().contiguous(),
                                   wc.float().contiguous(), gx, ctx.norm, ref.L1_EPS, g.float().contiguous().reshape(1))
        return gx, None, None, None


_WEIGHTS: dict = {}


def _loss_weights(b: int, R: int, Cc: int, device):
    """Per-volume weights of score_neg - score_pos: -1/(2bR), -1/(2bCc) for the
    b positive volumes, + for the b negatives.  Built on the device by fill
    kernels (no pageable host->device copy per step) and cached per shape."""
    key = (b, R, Cc, str(device))
    w = _WEIGHTS.get(key)
    if w is None:
        sign = torch.ones(2 * b, dtype=torch.float32, device=device)
        sign[:b] = -1.0
        w = (sign / (2.0 * b * R), sign / (2.0 * b * Cc))
        if not (sign.is_cuda and torch.cuda.is_current_stream_capturing()):
            _WEIGHTS[key] = w
    return w


def weak_loss_from_corr(corr4d: torch.Tensor, n_pos: int, normalization: str | None = "softmax") -> torch.Tensor:
    """loss = score_neg - score_pos for a [2B,1,I,J,K,L] volume whose first B
    entries are the positive pairs and last B the negatives."""
    V = corr4d.shape[0]
    b = n_pos
    assert V == 2 * b
    i, j, k, l = corr4d.shape[2:]
    R, Cc = i * j, k * l
    if normalization not in _NORM:
        raise ValueError(f"normalization must be 'softmax', 'l1' or None, got {normalization!r}")
    if _ext.use_hip(corr4d):
        x3 = corr4d.reshape(V, R, Cc)
        wr, wc = _loss_weights(b, R, Cc, corr4d.device)
        return SoftmaxMaxScoreFn.apply(x3, wr, wc, _NORM[normalization])
    pos = ref.match_score(corr4d[:b], normalization)
    neg = ref.match_score(corr4d[b:], normalization)
    return neg - pos


class KeypointCEFn(torch.autograd.Function):
    """ops/reference.py keypoint_ce on the HIP kernels of csrc/kploss.hip: the
    forward builds the keypoint table on the device and saves it with the
    log-sum-exps; the backward is the closed form, scaled by the incoming
    gradient and 1 / (2 Nvalid) inside the kernel (no host sync)."""

    @staticmethod
    def forward(ctx, x3, sp, tp, ssz, tsz, grid):
        x3 = x3.float().contiguous()
        B, N = x3.shape[0], sp.shape[2]
        dev = x3.device
        cells = torch.empty((B, N, 8), dtype=torch.int32, device=dev)
        wts = torch.empty((B, N, 8), dtype=torch.float32, device=dev)
        valid = torch.empty((B, N), dtype=torch.int32, device=dev)
        lse = torch.empty((B, N, 2), dtype=torch.float32, device=dev)
        term = torch.empty((B, N, 2), dtype=torch.float32, device=dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)
        _ext.ext().kploss_fwd(x3, sp, tp, ssz, tsz, *grid, cells, wts, valid, lse, term, out)
        ctx.save_for_backward(x3, cells, wts, valid, lse, out)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        x3, cells, wts, valid, lse, out = ctx.saved_tensors
        gx = torch.empty_like(x3)
        _ext.ext().kploss_bwd(x3, cells, wts, valid, lse, out[1:], gx, g.float().contiguous().reshape(1))
        return gx, None, None, None, None, None


# THE keypoint fields of a batch (the loss table below and engine/trainer.py take them from here)
KEYPOINT_FIELDS = ("source_points", "target_points", "source_im_size", "target_im_size")


def strong_loss_from_corr(corr4d: torch.Tensor, batch) -> torch.Tensor:
    """Keypoint-supervised loss (ops/reference.py keypoint_ce) of a
    [B,1,hA,wA,hB,wB] volume against the batch's ``source_points`` /
    ``target_points`` [B,2,N] and ``*_im_size`` [B,3].  The keypoint tensors are
    used as they are when they already are contiguous fp32 on the volume's
    device (the trainer moves the batch once); nothing is copied per step."""
    missing = [k for k in KEYPOINT_FIELDS if k not in batch]
    if missing:
        raise KeyError(f"strong loss: the batch has no {missing} (use a dataset with keypoints)")
    if corr4d.dim() != 6 or corr4d.shape[1] != 1:
        raise ValueError(f"strong loss: expected a [B,1,hA,wA,hB,wB] volume, got {tuple(corr4d.shape)}")
    sp, tp, ssz, tsz = (batch[k] for k in KEYPOINT_FIELDS)
    if _ext.use_hip(corr4d):
        b = corr4d.shape[0]
        ha, wa, hb, wb = corr4d.shape[2:]
        if sp.shape[2] > 64:
            raise ValueError(f"strong loss: at most 64 keypoints per image on the GPU (got {sp.shape[2]})")
        sp, tp, ssz, tsz = (t.to(device=corr4d.device, dtype=torch.float32).contiguous() for t in (sp, tp, ssz, tsz))
        _ext.count("kploss")
        return KeypointCEFn.apply(corr4d.reshape(b, ha * wa, hb * wb), sp, tp, ssz, tsz, (ha, wa, hb, wb))
    return ref.keypoint_ce(corr4d, sp, tp, ssz, tsz)


class DenseCEFn(torch.autograd.Function):
    """ops/reference.py dense_ce on the HIP kernels of csrc/densece.hip: the
    forward builds the target table on the device, takes the row / column
    log-sum-exps from the one-pass stats2d statistics and reduces the terms in
    a fixed order; it saves the table, the log-sum-exps (+inf for an invalid
    line: the backward then needs no flag) and ``out`` = (loss, 1 / (2 N_A),
    1 / (2 N_B)).  The backward is the closed form, one pass over
    the volume, scaled by the incoming gradient inside the kernel (no host sync)."""

    @staticmethod
    def forward(ctx, x3, maps, grid):
        x3 = x3.float().contiguous()
        C = _ext.ext()
        B, R, Cc = x3.shape
        n = max(R, Cc)
        dev = x3.device
        cells = torch.empty((B, 2, 4, n), dtype=torch.int32, device=dev)
        wts = torch.empty((B, 2, 4, n), dtype=torch.float32, device=dev)
        valid = torch.empty((B, 2, n), dtype=torch.int32, device=dev)
        lse = torch.empty((B, 2, n), dtype=torch.float32, device=dev)
        term = torch.empty((B, 2, n), dtype=torch.float32, device=dev)
        out = torch.empty(3, dtype=torch.float32, device=dev)
        C.densece_table(maps, *grid, cells, wts, valid)
        rmax, _, rse, cmax, _, cse = _row_col_stats(x3, 1)
        C.densece_fwd(x3, cells, wts, valid, rmax, rse, cmax, cse, lse, term)
        C.densece_reduce(term, valid, out)
        ctx.save_for_backward(x3, cells, wts, lse, out)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        x3, cells, wts, lse, out = ctx.saved_tensors
        gx = torch.empty_like(x3)
        _ext.ext().densece_bwd(x3, cells, wts, lse, out, gx, g.float().contiguous().reshape(1))
        return gx, None, None


def warp_loss_from_corr(corr4d: torch.Tensor, batch) -> torch.Tensor:
    """Dense correspondence loss (ops/reference.py dense_ce) of a
    [B,1,hA,wA,hB,wB] volume whose two views are warps of one image, against
    the batch's ``warp_maps`` [B, 2, 12] fp64 (data/augment.py view_maps).  The
    maps are used as they are when they already are contiguous fp64 on the
    volume's device (the trainer moves the batch once)."""
    if "warp_maps" not in batch:
        raise KeyError("warp loss: the batch has no 'warp_maps' (use the two-view input path, gpu_view_batch)")
    if corr4d.dim() != 6 or corr4d.shape[1] != 1:
        raise ValueError(f"warp loss: expected a [B,1,hA,wA,hB,wB] volume, got {tuple(corr4d.shape)}")
    maps = batch["warp_maps"]
    b = corr4d.shape[0]
    if maps.dim() != 3 or tuple(maps.shape) != (b, 2, 12):
        raise ValueError(f"warp loss: warp_maps must be [{b}, 2, 12], got {tuple(maps.shape)}")
    if _ext.use_hip(corr4d):
        ha, wa, hb, wb = corr4d.shape[2:]
        maps = maps.to(device=corr4d.device, dtype=torch.float64).contiguous()
        _ext.count("densece")
        return DenseCEFn.apply(corr4d.reshape(b, ha * wa, hb * wb), maps, (ha, wa, hb, wb))
    return ref.dense_ce(corr4d, maps)


def match_score(corr4d: torch.Tensor, normalization: str | None = "softmax") -> torch.Tensor:
    """mean(scores_A + scores_B) / 2 of one batch (train.py:125-134)."""
    V = corr4d.shape[0]
    i, j, k, l = corr4d.shape[2:]
    R, Cc = i * j, k * l
    if normalization not in _NORM:
        raise ValueError(f"normalization must be 'softmax', 'l1' or None, got {normalization!r}")
    if _ext.use_hip(corr4d):
        wr = torch.full((V,), 1.0 / (2.0 * V * R), device=corr4d.device)
        wc = torch.full((V,), 1.0 / (2.0 * V * Cc), device=corr4d.device)
        return SoftmaxMaxScoreFn.apply(corr4d.reshape(V, R, Cc), wr, wc, _NORM[normalization])
    return ref.match_score(corr4d, normalization)


# The training losses as data, for engine/trainer.py.  negatives: reads the rolled negative volumes
# after the positives; fields: the batch tensors a step reads besides the images (kept alive on the
# main stream); from_corr: (volumes, batch, normalization) -> loss; pck_fields: evaluation also
# scores PCK when the batch has all of these (None: never).
LossSpec = collections.namedtuple("LossSpec", "negatives fields from_corr pck_fields")

LOSSES = {
    "weak": LossSpec(True, (), lambda corr4d, batch, normalization:
                     weak_loss_from_corr(corr4d, corr4d.shape[0] // 2, normalization), None),
    "strong": LossSpec(False, KEYPOINT_FIELDS + ("L_pck",), lambda corr4d, batch, normalization:
                       strong_loss_from_corr(corr4d, batch), ("L_pck",)),
    "warp": LossSpec(False, ("warp_maps",) + KEYPOINT_FIELDS + ("L_pck",), lambda corr4d, batch, normalization:
                     warp_loss_from_corr(corr4d, batch), ("L_pck", "source_points")),
}
