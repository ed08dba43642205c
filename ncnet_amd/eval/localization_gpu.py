"""Batched P3P LO-RANSAC on the GPU (csrc/pnp.hip) for the InLoc back end.

``p3p_ransac_batch`` solves many independent (rays, X) problems with one
host->device copy, one kernel launch and one device->host copy: one workgroup
per problem, every lane one minimal sample per round, all of a problem's points
scored from LDS (see the header of csrc/pnp.hip and docs/ARCHITECTURE.md).
The semantics are those of ``localization.p3p_ransac`` (angular inlier test,
adaptive stop, hard cap, local optimisation on the inliers); the hypothesis
sequence is the kernel's own counter-based stream, so a problem's result
depends on its data and its key only.

``device='cpu'``, or a machine without a GPU, runs the numpy ``p3p_ransac`` per
problem with ``np.random.default_rng(key)``.  On a GPU machine the HIP
extension is required (``ops/_ext.py``): there is no silent fallback.
"""
from __future__ import annotations

import numpy as np

from .localization import p3p_ransac


def key_to_int64(key) -> int:
    """The kernel's 64-bit key of a problem: an int as it is, anything else
    ``np.random.default_rng`` accepts (e.g. the [seed, q, jj] of a pair) through
    numpy's SeedSequence."""
    if isinstance(key, (int, np.integer)):
        k = int(key) & 0xFFFFFFFFFFFFFFFF
    else:
        k = int(np.random.SeedSequence(key).generate_state(1, np.uint64)[0])
    return k - (1 << 64) if k >= (1 << 63) else k


def _use_gpu(device) -> bool:
    import torch
    if device is not None and str(device) != "gpu" and torch.device(device).type == "cpu":
        return False
    if not torch.cuda.is_available():
        return False
    return True


def p3p_ransac_batch(problems, thr_rad: float, max_iters: int = 10000, confidence: float = 0.999, lo_iters: int = 20,
                     keys=None, device=None, return_rounds: bool = False):
    """problems: list of (rays [3, n], X [3, n]) numpy pairs (the convention of
    ``p3p_ransac``) -> list of (P 3x4 or None, inlier mask [n] bool), in order.

    keys: one per problem (default: the problem's index); an int, or a sequence
    of ints as ``np.random.default_rng`` takes.  return_rounds (GPU only) adds
    the int array of sampling rounds every problem ran."""
    problems = [(np.asarray(r, np.float64).reshape(3, -1), np.asarray(x, np.float64).reshape(3, -1))
                for r, x in problems]
    for r, x in problems:
        if r.shape != x.shape:
            raise ValueError(f"rays {r.shape} and X {x.shape} differ")
    keys = list(range(len(problems))) if keys is None else list(keys)
    if len(keys) != len(problems):
        raise ValueError(f"{len(keys)} keys for {len(problems)} problems")
    if max_iters < 0:
        raise ValueError("max_iters must be non-negative")
    if not _use_gpu(device):
        if return_rounds:
            raise ValueError("return_rounds needs the GPU path")
        return [p3p_ransac(r, x, thr_rad, max_iters, confidence, lo_iters, rng=np.random.default_rng(k))
                for (r, x), k in zip(problems, keys)]
    if not problems:
        return ([], np.zeros(0, np.int32)) if return_rounds else []

    import torch
    from ..ops import _ext
    dev = torch.device("cuda" if device is None or str(device) == "gpu" else device)
    ext = _ext.ext()                                   # raises when the extension is missing
    B = len(problems)
    sizes = np.array([r.shape[1] for r, _ in problems], np.int64)
    offsets = np.zeros(B + 1, np.int64)
    np.cumsum(sizes, out=offsets[1:])
    N = int(offsets[-1])
    if N >= 2 ** 31:
        raise ValueError("too many tentatives for one batch")
    # one host buffer = one H2D copy: rays [N, 3] | X [N, 3] | keys [B] | offsets [B + 1] (int32 pairs in 8-byte words)
    n_off = (B + 2) // 2
    buf = np.empty(6 * N + B + n_off, np.float64)
    pts = buf[: 6 * N].reshape(2, N, 3)
    for (r, x), o in zip(problems, offsets[:-1]):
        n = r.shape[1]
        pts[0, o:o + n] = r.T
        pts[1, o:o + n] = x.T
    buf[6 * N: 6 * N + B].view(np.int64)[:] = [key_to_int64(k) for k in keys]
    off32 = buf[6 * N + B:].view(np.int32)
    off32[: B + 1] = offsets
    off32[B + 1:] = 0
    d = torch.from_numpy(buf).to(dev)
    d_rays, d_X = d[: 3 * N].view(N, 3), d[3 * N: 6 * N].view(N, 3)
    d_keys = d[6 * N: 6 * N + B].view(torch.int64)
    d_off = d[6 * N + B:].view(torch.int32)[: B + 1]
    rounds = torch.zeros(B, dtype=torch.int32, device=dev) if return_rounds else None
    P, ninl, mask = ext.p3p_ransac_batch(d_rays, d_X, d_off, d_keys, float(thr_rad), int(max_iters), float(confidence),
                                         int(lo_iters), rounds)
    _ext.count("p3p_ransac_batch")
    # one D2H copy: P [B, 12] fp64 | n_inliers | rounds | mask, packed as bytes
    parts = [P.view(-1).view(torch.uint8), ninl.view(torch.uint8)]
    if return_rounds:
        parts.append(rounds.view(torch.uint8))
    host = torch.cat(parts + [mask]).cpu().numpy()
    hP = host[: 96 * B].view(np.float64).reshape(B, 3, 4)
    hn = host[96 * B: 100 * B].view(np.int32)
    hr = host[100 * B: 104 * B].view(np.int32).copy() if return_rounds else None
    hm = host[(104 if return_rounds else 100) * B:].astype(bool)
    out = []
    for b in range(B):
        m = hm[offsets[b]: offsets[b + 1]].copy()
        if np.isnan(hP[b]).any() or hn[b] == 0:
            out.append((None, np.zeros(m.size, dtype=bool)))
        else:
            out.append((hP[b].copy(), m))
    if return_rounds:
        return out, hr
    return out


def p3p_solve(rays, X, device="cuda"):
    """Test entry point of the kernel's minimal solver: rays / X [M, 3, 3]
    (row k = k-th bearing vector / world point) -> (P [M, 4, 3, 4] with the
    valid poses first, NaN after them; nsol [M])."""
    import torch
    from ..ops import _ext
    r = torch.as_tensor(np.ascontiguousarray(rays, np.float64), device=device)
    x = torch.as_tensor(np.ascontiguousarray(X, np.float64), device=device)
    P, nsol = _ext.ext().p3p_solve(r, x)
    return P.cpu().numpy(), nsol.cpu().numpy()
