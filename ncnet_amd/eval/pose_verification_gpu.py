"""Batched dense pose verification on the GPU (csrc/pv.hip) for the InLoc back end.

``pv_scores_batch`` scores all (query image, pose) candidates of ONE scan: the
scan is uploaded once and traversed once per group of equally sized targets
(``pv_render``: every point is read once for all poses of a launch), the image
stages of ``pose_verification.pv_score`` (grey conversion, masked
normalisation, in-painting, dense SIFT up to the pooled orientation maps) run
as batched torch on ``[B, ...]`` tensors with the same formulas and constants,
and one fused kernel (``pv_desc_err``) turns the pooled maps of both sides into
the per-keypoint RootSIFT distance without writing a descriptor.  The score is
``1 / nanmedian`` per candidate, copied to the host once per call.

``device='cpu'``, or a machine without a GPU, runs ``pv_score(device='cpu')``
per candidate: today's results bit for bit.  On a GPU machine the HIP
extension is required (``ops/_ext.py``): there is no silent fallback.

Neighbourhood sums (the in-painting stencil, the Gaussian and the triangular
windows of dense SIFT) are written as sums of shifted slices: every output
element sees the same operations whatever the batch size, so a candidate's
result does not depend on what else is in its batch.
"""
from __future__ import annotations

import math

import numpy as np

from . import pose_verification as pv
from .localization_gpu import _use_gpu
from .pose_verification import DS_LEVEL

INPAINT_ITERS = 50          # pose_verification.inpaint_nans(iters=50)
GROW_CHECK = 4              # in-painting grow phase: look for completion every GROW_CHECK steps


def _target_size(img, ds):
    return max(1, int(round(img.shape[0] * ds))), max(1, int(round(img.shape[1] * ds)))


def _valid_pose(P) -> bool:
    return P is not None and bool(np.all(np.isfinite(np.asarray(P, np.float64))))


# ---------------------------------------------------------------------------
# batched image stages ([B, h, w] tensors; formulas of pose_verification.py)
def _nb4(x):
    """4-neighbour sum with replicated borders (inpaint_nans' stencil)."""
    import torch.nn.functional as F
    p = F.pad(x[:, None], (1, 1, 1, 1), mode="replicate")[:, 0]
    return p[:, :-2, 1:-1] + p[:, 2:, 1:-1] + p[:, 1:-1, :-2] + p[:, 1:-1, 2:]


def inpaint_nans_batch(img, iters: int = INPAINT_ITERS):
    """``inpaint_nans`` on [B, h, w].  The grow phase is a host loop of at most
    h + w steps (a step past an image's completion changes nothing in it);
    completion is looked at every GROW_CHECK steps only."""
    import torch
    known = ~torch.isnan(img)
    m = known.to(img.dtype)
    x = torch.where(known, img, torch.zeros_like(img))
    filled = m.clone()
    h, w = img.shape[-2:]
    for step in range(h + w):
        if step % GROW_CHECK == 0 and bool((filled > 0).all()):
            break
        s, c = _nb4(x * filled), _nb4(filled)
        grow = (filled == 0) & (c > 0)
        x = torch.where(grow, s / c.clamp_min(1e-12), x)
        filled = torch.where(grow, torch.ones_like(filled), filled)
    for _ in range(iters):
        x = torch.where(known, x, _nb4(x) / 4.0)
    return x


def image_normalization_batch(img, mask):
    """``image_normalization`` on [B, h, w] with one mask per image."""
    import torch
    n = mask.flatten(1).sum(1).to(img.dtype)[:, None, None]
    mf = mask.to(img.dtype)
    mean = (img * mf).flatten(1).sum(1)[:, None, None] / n.clamp_min(1)
    d = (img - mean) * mf
    std = torch.sqrt((d * d).flatten(1).sum(1)[:, None, None] / (n - 1).clamp_min(1))
    x = (img - mean) / std.clamp_min(1e-6)
    inf = torch.full_like(x, float("inf"))
    lo = torch.where(mask, x, inf).flatten(1).amin(1)[:, None, None]
    hi = torch.where(mask, x, -inf).flatten(1).amax(1)[:, None, None]
    out = ((x - lo) / (hi - lo).clamp_min(1e-6)).clamp(0, 1)
    return torch.where(n >= 2, out, torch.zeros_like(out))


def _window(x, k, dim, mode):
    """Correlation of [B, C, H, W] with the 1-D window k along dim (-1 or -2),
    'replicate' or zero padding of len(k) // 2, as a sum of shifted slices."""
    import torch.nn.functional as F
    r = len(k) // 2
    pad = (r, r, 0, 0) if dim == -1 else (0, 0, r, r)
    p = F.pad(x, pad, mode="replicate") if mode == "replicate" else F.pad(x, pad)
    n = x.shape[dim]
    out = None
    for i, wgt in enumerate(k):
        s = p.narrow(dim, i, n) * wgt
        out = s if out is None else out + s
    return out


def pooled_orientation_maps(img, size: int = 8, magnif: float = 6.0, nori: int = 8):
    """The first half of ``dense_sift`` on [B, H, W] images in [0, 1]: Gaussian
    pre-smoothing, gradients, linear orientation binning, triangular spatial
    pooling -> [B, nori, H, W] (dense_sift's ``o``)."""
    import torch
    import torch.nn.functional as F
    dt = torch.float32
    x = img.to(dt)[:, None]
    sigma = size / magnif
    r = max(1, int(math.ceil(3 * sigma)))
    t = torch.arange(-r, r + 1, dtype=dt)
    gk = torch.exp(-0.5 * (t / sigma) ** 2)
    gk = (gk / gk.sum()).tolist()
    x = _window(x, gk, -1, "replicate")
    x = _window(x, gk, -2, "replicate")
    xp = F.pad(x, (1, 1, 1, 1), mode="replicate")
    gx = 0.5 * (xp[..., 1:-1, 2:] - xp[..., 1:-1, :-2])
    gy = 0.5 * (xp[..., 2:, 1:-1] - xp[..., :-2, 1:-1])
    mag = torch.sqrt(gx * gx + gy * gy)                      # [B, 1, H, W]
    ang = torch.atan2(gy, gx) % (2 * math.pi)
    fb = ang / (2 * math.pi) * nori
    b0 = torch.floor(fb).long() % nori
    w1 = fb - torch.floor(fb)
    # a pixel votes into bins b0 and b0 + 1: dense_sift's two scatter_add_ calls, written as selections
    bins = torch.arange(nori, device=img.device)[None, :, None, None]
    zero = torch.zeros((), device=img.device, dtype=dt)
    omap = torch.where(b0 == bins, mag * (1 - w1), zero) + torch.where((b0 + 1) % nori == bins, mag * w1, zero)
    tri = (1 - (torch.arange(-size + 1, size, dtype=dt).abs() / size)).tolist()
    o = _window(omap, tri, -1, "zeros")
    return _window(o, tri, -2, "zeros").contiguous()


# ---------------------------------------------------------------------------
def pv_scores_batch(query_imgs, rgb, xyz, poses, focal: float, device=None, ds: float = DS_LEVEL,
                    return_maps: bool = False):
    """Dense-PV scores of the candidates (query_imgs[i], poses[i]) of one scan.

    query_imgs: [H, W, 3] (or [H, W]) arrays at full resolution; the same array
    may appear many times and is downsampled once.  rgb / xyz [N, 3]: the scan
    (xyz in the global frame).  poses: [3, 4] arrays or None.  focal: full-res
    pixels.  Returns the list of scores; with return_maps also a list of
    (synth [h, w, 3], flag [h, w], errmap [ny, nx]) per candidate, with None
    where ``pv_score`` returns None."""
    query_imgs, poses = list(query_imgs), list(poses)
    if len(query_imgs) != len(poses):
        raise ValueError(f"{len(query_imgs)} query images for {len(poses)} poses")
    B = len(poses)
    if not _use_gpu(device):
        res = [pv.pv_score(q, rgb, xyz, P, focal, device="cpu", ds=ds) for q, P in zip(query_imgs, poses)]
        scores = [float(r[0]) for r in res]
        return (scores, [tuple(r[1:]) for r in res]) if return_maps else scores

    import torch
    import torch.nn.functional as F
    from ..ops import _ext
    ext = _ext.ext()                                       # raises when the extension is missing
    dev = torch.device("cuda" if device is None or str(device) == "gpu" else device)
    scores = [0.0] * B
    maps = [(None, None, None)] * B
    live = [i for i in range(B) if _valid_pose(poses[i])]
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    rgb = np.asarray(rgb, np.float32).reshape(-1, 3)
    if xyz.shape[0] == 0:
        if return_maps:
            for i in live:
                h, w = _target_size(np.asarray(query_imgs[i]), ds)
                maps[i] = (np.full((h, w, 3), np.nan, np.float32), np.zeros((h, w), bool), None)
        return (scores, maps) if return_maps else scores
    if not live:
        return (scores, maps) if return_maps else scores

    xyz_d = torch.from_numpy(np.ascontiguousarray(xyz)).to(dev)      # the scan: one upload per call
    rgb_d = torch.from_numpy(np.ascontiguousarray(rgb)).to(dev)

    groups = {}
    for i in live:
        groups.setdefault(_target_size(np.asarray(query_imgs[i]), ds), []).append(i)
    qcache = {}                                            # id(query array) -> (grey / scale) [h, w] on the device

    def query_grey(img, hq, wq):
        key = id(img)
        if key not in qcache:
            q = torch.as_tensor(np.asarray(img, np.float32), device=dev)
            if q.ndim == 2:
                q = q[..., None].repeat(1, 1, 3)
            qs = F.interpolate(q.permute(2, 0, 1)[None], size=(hq, wq), mode="bilinear", align_corners=False,
                               antialias=True)[0].permute(1, 2, 0)
            scale = torch.where(qs.max() > 1.5, 255.0, 1.0).to(qs.dtype)
            qcache[key] = pv.rgb2gray(qs) / scale
        return qcache[key]

    pending = []                                           # (candidate indices, medians on the device)
    for (hq, wq), idx in sorted(groups.items()):
        fl = focal * ds
        K = torch.tensor([[fl, 0, wq / 2.0], [0, fl, hq / 2.0], [0, 0, 1]], dtype=torch.float64)
        KP = torch.stack([K @ torch.as_tensor(np.asarray(poses[i], np.float64)) for i in idx]).contiguous().to(dev)
        synth, flag, _ = ext.pv_render(xyz_d, rgb_d, KP, hq, wq)
        _ext.count("pv_render")
        keep = flag.flatten(1).any(1).cpu().numpy()        # candidates that see nothing leave the batch here
        if return_maps:
            synth_h, flag_h = synth.cpu().numpy(), flag.cpu().numpy()
            for j, i in enumerate(idx):
                maps[i] = (synth_h[j], flag_h[j], None)
        sel = [j for j in range(len(idx)) if keep[j]]
        if not sel:
            continue
        if len(sel) < len(idx):
            t = torch.as_tensor(sel, device=dev)
            synth, flag = synth[t], flag[t]
        idx = [idx[j] for j in sel]
        gq = torch.stack([query_grey(query_imgs[i], hq, wq) for i in idx])
        iq = image_normalization_batch(gq, flag)
        smax = torch.nan_to_num(synth).flatten(1).amax(1)[:, None, None]
        gs = pv.rgb2gray(synth) / torch.where(smax > 1.5, 255.0, 1.0).to(synth.dtype)
        gs = torch.where(flag, gs, torch.full_like(gs, float("nan")))
        isyn = image_normalization_batch(inpaint_nans_batch(gs), flag)
        oq, osy = pooled_orientation_maps(iq), pooled_orientation_maps(isyn)
        err = ext.pv_desc_err(oq, osy, flag.contiguous())
        _ext.count("pv_desc_err")
        if err.shape[1] == 0:
            continue
        pending.append((idx, torch.nanquantile(err, 0.5, dim=1)))
        if return_maps:
            ny = (hq - 27) // 4
            err_h = err.cpu().numpy()
            for j, i in enumerate(idx):
                if not np.isnan(err_h[j]).all():
                    maps[i] = (maps[i][0], maps[i][1], err_h[j].reshape(ny, -1))
    if pending:
        med = torch.cat([m for _, m in pending]).cpu().numpy()        # the one copy of the scores
        order = [i for idx, _ in pending for i in idx]
        for i, m in zip(order, med):
            m = float(m)
            scores[i] = 0.0 if math.isnan(m) else (1.0 / m if m > 0 else float("inf"))
    return (scores, maps) if return_maps else scores
