"""Geometric + photometric augmentation of uint8 pair batches, with the
keypoints carried through the same transforms.

The GPU side is ONE kernel (csrc/dataprep.hip ``warp_norm_u8``): it resizes,
warps, jitters and normalises the packed batch in the pass that already
resized and normalised it.  This module is the host side: it draws one
parameter row per image, and moves the keypoints through the same map.

A row is ``(a0, a1, a2, a3, a4, a5, gain, bias)``: output pixel ``p_o = (ox,
oy)`` (0-based, x right, y down) shows the source position ``A p_o + t`` with
``A = [[a0, a1], [a3, a4]]``, ``t = (a2, a5)``, clamped to the image; the
normalised value is scaled by ``gain`` and shifted by ``bias``.

Frames.  Keypoints are (x, y) in 1-based pixels of the image they belong to
(the PF-Pascal annotation convention; ``eval/point_tnf.normalize_axis`` maps
1 -> -1 and L -> +1), so pixel position = keypoint - 1.  A keypoint ``p`` of
the decoded image becomes ``A^-1 (p - 1 - t) + 1`` in the output frame.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch


@dataclass(frozen=True)
class PairAugment:
    """Ranges of the random similarity + photometric jitter.

    ================  ===========  ===================================================
    field             default      sampling
    ================  ===========  ===================================================
    ``rot_deg``       15           rotation, uniform in +-rot_deg
    ``scale``         (0.8, 1.25)  zoom factor z, log-uniform; z < 1 zooms in (the
                                   output shows z times the source extent)
    ``shift``         0.1          uniform in +-shift, as a fraction of the source
                                   extent (W - 1, H - 1), per axis
    ``flip``          0.5          probability of a horizontal flip; drawn once per
                                   PAIR and applied to both of its images
    ``gain``          (0.8, 1.2)   contrast about the ImageNet mean, log-uniform
    ``bias``          0.2          brightness in normalised units, uniform in +-bias
    ================  ===========  ===================================================

    Everything but the flip is drawn per image.  Order of the draws
    (``draw_params``): first ``torch.rand(B)`` for the B flips, then
    ``torch.rand(2B, 6)`` whose row n holds image n's (rotation, zoom, shift x,
    shift y, gain, bias) uniforms -- sources are rows 0..B-1, targets B..2B-1.
    """
    rot_deg: float = 15.0
    scale: tuple = (0.8, 1.25)
    shift: float = 0.1
    flip: float = 0.5
    gain: tuple = (0.8, 1.2)
    bias: float = 0.2

    def __post_init__(self):
        for name in ("scale", "gain"):
            lo, hi = getattr(self, name)
            if not (0 < lo <= hi and math.isfinite(hi)):
                raise ValueError(f"{name} must be a range 0 < lo <= hi, got {(lo, hi)}")
        if not 0 <= self.flip <= 1:
            raise ValueError(f"flip is a probability, got {self.flip}")
        for name in ("rot_deg", "shift", "bias"):
            v = getattr(self, name)
            if not (v >= 0 and math.isfinite(v)):
                raise ValueError(f"{name} must be finite and >= 0, got {v}")


def _ratio32(n_in: torch.Tensor, n_out: int) -> torch.Tensor:
    """float32(n_in - 1) / float32(n_out - 1), 0 when n_out == 1: the
    align_corners=True source step exactly as resize_norm_u8_kernel forms it."""
    if n_out <= 1:
        return torch.zeros(n_in.shape, dtype=torch.float32)
    return (n_in - 1).to(torch.float32) / torch.tensor(float(n_out - 1), dtype=torch.float32)


def resize_params(meta: torch.Tensor, oh: int, ow: int) -> torch.Tensor:
    """[N, 8] rows ``(rx, 0, 0, 0, ry, 0, 1, 0)`` of the plain resize of
    ``meta`` [N, 3] = (byte offset, H, W) to ``oh`` x ``ow``, built directly in
    fp32: with them ``warp_norm_u8`` reproduces ``resize_norm_u8`` bit for bit."""
    meta = meta.cpu()
    out = torch.zeros((meta.shape[0], 8), dtype=torch.float32)
    out[:, 0] = _ratio32(meta[:, 2], ow)
    out[:, 4] = _ratio32(meta[:, 1], oh)
    out[:, 6] = 1.0
    return out


def _uniform(u, lo, hi):
    return lo + u * (hi - lo)


def _log_uniform(u, lo, hi):
    return torch.exp(_uniform(u, math.log(lo), math.log(hi)))


def draw_params(meta: torch.Tensor, oh: int, ow: int, aug: PairAugment, generator: torch.Generator) -> torch.Tensor:
    """One random row per image of a pair batch: ``meta`` [2B, 3] = (byte
    offset, H, W), sources first, then targets (``collate_uint8_pairs``).
    Returns float32 [2B, 8], composed in fp64 and then cast.

    With ``c_o = ((ow-1)/2, (oh-1)/2)``, ``c_s = ((W-1)/2, (H-1)/2)`` and
    ``S = diag((W-1)/(ow-1), (H-1)/(oh-1))``:

        A = S . R(theta) . z . diag(+-1, 1)        t = c_s + shift o (W-1, H-1) - A c_o

    i.e. rotation, zoom and flip act about the centre of the OUTPUT frame (on
    the resized image), S maps that frame onto the source, and the shift moves
    the sampled window by a fraction of the source extent.  ``generator`` must
    be a CPU generator (the draws are host-side and reproducible from its
    seed); see ``PairAugment`` for the order of the draws."""
    if generator is None or generator.device.type != "cpu":
        raise ValueError("draw_params needs a CPU torch.Generator")
    meta = meta.cpu()
    n = meta.shape[0]
    if n % 2:
        raise ValueError(f"a pair batch has an even number of images, got {n}")
    b = n // 2
    flip = torch.rand(b, generator=generator, dtype=torch.float64) < aug.flip
    u = torch.rand(n, 6, generator=generator, dtype=torch.float64)
    theta = _uniform(u[:, 0], -aug.rot_deg, aug.rot_deg) * (math.pi / 180.0)
    z = _log_uniform(u[:, 1], *aug.scale)
    shift = _uniform(u[:, 2:4], -aug.shift, aug.shift)
    gain = _log_uniform(u[:, 4], *aug.gain)
    bias = _uniform(u[:, 5], -aug.bias, aug.bias)
    sign = 1.0 - 2.0 * torch.cat((flip, flip)).to(torch.float64)

    ext = torch.stack((meta[:, 2] - 1, meta[:, 1] - 1), 1).to(torch.float64)          # (W-1, H-1)
    s = torch.stack((ext[:, 0] / (ow - 1) if ow > 1 else torch.zeros(n, dtype=torch.float64),
                     ext[:, 1] / (oh - 1) if oh > 1 else torch.zeros(n, dtype=torch.float64)), 1)
    c, sn = torch.cos(theta) * z, torch.sin(theta) * z
    A = torch.stack((torch.stack((s[:, 0] * c * sign, -s[:, 0] * sn), 1),
                     torch.stack((s[:, 1] * sn * sign, s[:, 1] * c), 1)), 1)           # [n, 2, 2]
    c_o = torch.tensor([(ow - 1) / 2.0, (oh - 1) / 2.0], dtype=torch.float64)
    t = ext / 2.0 + shift * ext - A @ c_o
    out = torch.stack((A[:, 0, 0], A[:, 0, 1], t[:, 0], A[:, 1, 0], A[:, 1, 1], t[:, 1], gain, bias), 1)
    out = out.to(torch.float32)
    if not bool(torch.isfinite(out).all()):
        raise ValueError("non-finite augmentation parameters (check the PairAugment ranges and the image sizes)")
    return out


def transform_points(points: torch.Tensor, params: torch.Tensor, oh: int, ow: int) -> torch.Tensor:
    """Keypoints of the decoded images -> the output frame of ``params``.

    ``points`` [B, 2, n]: (x, y) in 1-based pixels, ``-1`` padded; ``params``
    [B, 8], row i belonging to the image of ``points[i]``.  In fp64:
    ``p_o = A^-1 (p - 1 - t)``, new point ``p_o + 1``.  A point stays valid when
    ``0 <= p_o <= (ow - 1, oh - 1)``; every other column (padding included)
    comes back as ``(-1, -1)``.  Returns the dtype of ``points``.

    An image whose map is singular -- one with ``H < 2`` or ``W < 2``, or any
    image when ``oh < 2`` or ``ow < 2``: all output pixels then show one source
    row or column -- cannot carry keypoints: ``ValueError``."""
    p = points.detach().cpu().to(torch.float64)
    q = params.detach().cpu().to(torch.float64)
    valid = (p != -1).all(1)                                                          # [B, n]
    A = torch.stack((q[:, [0, 1]], q[:, [3, 4]]), 1)                                  # [B, 2, 2]
    t = q[:, [2, 5]]
    det = A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0]
    bad = (det == 0) & valid.any(1)
    if bool(bad.any()):
        raise ValueError(f"image {int(torch.nonzero(bad)[0])} of the batch has keypoints but a singular sampling "
                         f"map: an image with H < 2 or W < 2, or an output of {oh} x {ow} with oh < 2 or ow < 2, has "
                         "no pixel frame to move keypoints in")
    det = torch.where(det == 0, torch.ones_like(det), det)
    inv = torch.stack((torch.stack((A[:, 1, 1], -A[:, 0, 1]), 1),
                       torch.stack((-A[:, 1, 0], A[:, 0, 0]), 1)), 1) / det.view(-1, 1, 1)
    po = inv @ (p - 1.0 - t.unsqueeze(2))                                             # [B, 2, n]
    hi = torch.tensor([ow - 1.0, oh - 1.0], dtype=torch.float64).view(1, 2, 1)
    valid = valid & ((po >= 0) & (po <= hi)).all(1)
    out = torch.where(valid.unsqueeze(1), po + 1.0, torch.full_like(po, -1.0))
    return out.to(points.dtype)


def transform_pair_points(source_points, target_points, params, oh: int, ow: int):
    """Both point sets of a pair batch through ``params`` [2B, 8] (sources
    first, then targets).  Index k of BOTH sets becomes ``-1`` when either of
    its two points leaves its output frame (a correspondence needs both ends)."""
    b = source_points.shape[0]
    sp = transform_points(source_points, params[:b], oh, ow)
    tp = transform_points(target_points, params[b:], oh, ow)
    keep = ((sp != -1).all(1) & (tp != -1).all(1)).unsqueeze(1)
    return (torch.where(keep, sp, torch.full_like(sp, -1.0)),
            torch.where(keep, tp, torch.full_like(tp, -1.0)))


def view_maps(params: torch.Tensor, meta: torch.Tensor, oh: int, ow: int) -> torch.Tensor:
    """``warp_maps`` [B, 2, 12] fp64 of a two-view batch (the table of
    ``ops/reference.py dense_ce``): ``params`` [2B, 8] and ``meta`` [2B, 3] =
    (byte offset, H, W) hold view A of image b in row b and view B in row
    B + b, both views sampling the SAME source image.

    With ``p -> A_v p + t_v`` the pixel map of view v (output pixel -> source
    position), ``D_o = diag(ow - 1, oh - 1)`` and ``D_s = diag(W - 1, H - 1)``,
    on unit coordinates (pixel / (extent - 1)):

        view -> source:   u -> D_s^-1 (A_v D_o u + t_v)                 entries 6..11
        A -> B:           u -> D_o^-1 A_b^-1 (A_a D_o u + t_a - t_b)    entries 0..5, row [b, 0]
        B -> A:           likewise with a and b swapped                 entries 0..5, row [b, 1]

    Each map is stored as (m00, m01, c0, m10, m11, c1).  Composed in fp64 on
    the host.  A singular view map (an image with H < 2 or W < 2, or oh < 2 or
    ow < 2) has no inverse: ``ValueError``, as ``transform_points``."""
    q = params.detach().cpu().to(torch.float64)
    meta = meta.cpu()
    n = q.shape[0]
    if n % 2 or meta.shape[0] != n:
        raise ValueError(f"a two-view batch has 2B parameter and meta rows, got {n} and {meta.shape[0]}")
    b = n // 2
    if not torch.equal(meta[:b, 1:], meta[b:, 1:]):
        raise ValueError("the two views of an image must share its size")
    A = torch.stack((q[:, [0, 1]], q[:, [3, 4]]), 1)                                  # [2B, 2, 2]
    t = q[:, [2, 5]]
    det = A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0]
    d_s = torch.stack((meta[:, 2] - 1, meta[:, 1] - 1), 1).to(torch.float64)          # (W-1, H-1)
    bad = (det == 0) | (d_s == 0).any(1)
    if oh < 2 or ow < 2 or bool(bad.any()):
        which = f"view {int(torch.nonzero(bad)[0])}" if bool(bad.any()) else f"an output of {oh} x {ow}"
        raise ValueError(f"{which} of the batch has a singular sampling map: an image with H < 2 or W < 2, or an "
                         "output with oh < 2 or ow < 2, has no pixel frame to map cells in")
    inv = torch.stack((torch.stack((A[:, 1, 1], -A[:, 0, 1]), 1),
                       torch.stack((-A[:, 1, 0], A[:, 0, 0]), 1)), 1) / det.view(-1, 1, 1)
    d_o = torch.tensor([ow - 1.0, oh - 1.0], dtype=torch.float64)
    other = torch.cat((torch.arange(b, n), torch.arange(0, b)))                       # the other view of each row
    # into the other view: D_o^-1 inv_o (A D_o u + t - t_o)
    M = (inv[other] @ A) * d_o.view(1, 1, 2) / d_o.view(1, 2, 1)
    c = (inv[other] @ (t - t[other]).unsqueeze(2)).squeeze(2) / d_o
    # into the source image: D_s^-1 (A D_o u + t)
    Ms = A * d_o.view(1, 1, 2) / d_s.unsqueeze(2)
    cs = t / d_s
    rows = torch.stack((M[:, 0, 0], M[:, 0, 1], c[:, 0], M[:, 1, 0], M[:, 1, 1], c[:, 1],
                        Ms[:, 0, 0], Ms[:, 0, 1], cs[:, 0], Ms[:, 1, 0], Ms[:, 1, 1], cs[:, 1]), 1)   # [2B, 12]
    out = torch.stack((rows[:b], rows[b:]), 1).contiguous()
    if not bool(torch.isfinite(out).all()):
        raise ValueError("non-finite view maps (check the augmentation parameters)")
    return out
