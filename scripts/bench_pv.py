#!/usr/bin/env python
"""Time the batched GPU dense pose verification (eval/pose_verification_gpu.py,
csrc/pv.hip) against the per-candidate torch path (eval/pose_verification.py
pv_score, what inloc_localize.py --pv_device cuda / cpu runs) on one synthetic
scan sized like an InLoc scan.

Scene (seeded): --points random points on a wavy textured surface that fills the
view of a --query_size camera (default 3024 x 4032, the iPhone 7 queries, focal
4032 * 28 / 36); the query image is the surface's texture evaluated per pixel.
--candidates poses: the true one, then small rotations and shifts of growing
size.  At ds = 1/8 the targets are 378 x 504.

Three ways of scoring the same candidates, each timed as the whole call from
host arrays to host scores (scan upload included), after one warm-up call,
median of --reps with a device synchronise inside the window:

* batch:      pv_scores_batch(device='gpu'), one call;
* loop_cuda:  pv_score(device='cuda') per candidate;
* loop_cpu:   pv_score(device='cpu') per candidate on --threads torch threads
              (--cpu_reps repetitions, no warm-up: nothing to warm).

--breakdown also times the scan upload and pv_render alone.

    python scripts/bench_pv.py [--points 2000000] [--candidates 10] [--skip_cpu]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ncnet_amd.eval import pose_verification as pv  # noqa: E402
from ncnet_amd.eval import pose_verification_gpu as pvg  # noqa: E402


def _depth(u, v, wq):
    s = wq / 320.0
    return 4.0 + 0.5 * np.sin(u / (40.0 * s)) + 0.3 * np.cos(v / (25.0 * s))


def _texture(X):
    return (np.sin(3 * X[..., 0]) + np.cos(4 * X[..., 1]) + 2) / 4 * 255


def make_scene(n_points, hq, wq, focal, seed):
    """-> (query image [hq, wq, 3] uint8, rgb [N, 3] float32, xyz [N, 3] float64)."""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(0, wq, n_points), rng.uniform(0, hq, n_points)
    z = _depth(u, v, wq) + rng.uniform(0, 0.05, n_points)
    xyz = np.stack([(u - wq / 2.0) / focal * z, (v - hq / 2.0) / focal * z, z], 1)
    rgb = np.repeat(_texture(xyz)[:, None], 3, 1).astype(np.float32)
    vv, uu = np.meshgrid(np.arange(hq) + 0.5, np.arange(wq) + 0.5, indexing="ij")
    zz = _depth(uu, vv, wq) + 0.025
    img = _texture(np.stack([(uu - wq / 2.0) / focal * zz, (vv - hq / 2.0) / focal * zz, zz], -1))
    return np.repeat(img[..., None], 3, 2).astype(np.uint8), rgb, np.ascontiguousarray(xyz)


def make_poses(n):
    """The true pose, then pitched / yawed / shifted poses of growing size."""
    poses = []
    for k in range(n):
        a, b = math.radians(0.7 * k), math.radians(-0.4 * k)
        Ry = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
        Rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
        poses.append(np.hstack([Ry @ Rx, np.array([[0.03 * k], [0.01 * k], [0.0]])]))
    return poses


def _timed(fn, reps, sync=None):
    times, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        if sync is not None:
            sync()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), [round(t, 4) for t in times], out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", type=int, default=2_000_000)
    ap.add_argument("--candidates", type=int, default=10)
    ap.add_argument("--query_size", type=int, nargs=2, default=[3024, 4032])
    ap.add_argument("--focal", type=float, default=4032 * 28.0 / 36.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu_reps", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--skip_cpu", action="store_true")
    ap.add_argument("--skip_gpu", action="store_true")
    ap.add_argument("--breakdown", action="store_true")
    a = ap.parse_args(argv)
    import torch
    hq, wq = a.query_size
    q, rgb, xyz = make_scene(a.points, hq, wq, a.focal, a.seed)
    poses = make_poses(a.candidates)
    h, w = max(1, int(round(hq * pv.DS_LEVEL))), max(1, int(round(wq * pv.DS_LEVEL)))
    res = {"points": a.points, "candidates": a.candidates, "target": [h, w]}

    if not a.skip_gpu:
        assert torch.cuda.is_available(), "the GPU parts need a GPU (--skip_gpu times the CPU loop only)"
        sync = torch.cuda.synchronize
        batch = lambda: pvg.pv_scores_batch([q] * len(poses), rgb, xyz, poses, a.focal, device="gpu")   # noqa: E731
        loop = lambda: [pv.pv_score(q, rgb, xyz, P, a.focal, device="cuda")[0] for P in poses]           # noqa: E731
        batch(), sync()                                    # warm-up: code objects, allocator
        res["batch_s"], res["batch_s_all"], s_batch = _timed(batch, a.reps, sync)
        loop(), sync()
        res["loop_cuda_s"], res["loop_cuda_s_all"], s_loop = _timed(loop, a.reps, sync)
        res["batch_scores"] = [round(s, 4) for s in s_batch]
        res["loop_cuda_scores"] = [round(s, 4) for s in s_loop]
        res["speedup_vs_loop_cuda"] = res["loop_cuda_s"] / res["batch_s"]
        if a.breakdown:
            from ncnet_amd.ops import _ext
            ext = _ext.ext()
            up = lambda: (torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda())                    # noqa: E731
            res["upload_s"], _, (xyz_d, rgb_d) = _timed(up, a.reps, sync)
            fl = a.focal * pv.DS_LEVEL
            K = torch.tensor([[fl, 0, w / 2.0], [0, fl, h / 2.0], [0, 0, 1]], dtype=torch.float64)
            KP = torch.stack([K @ torch.as_tensor(P) for P in poses]).contiguous().cuda()
            res["render_s"], _, _ = _timed(lambda: ext.pv_render(xyz_d, rgb_d, KP, h, w), a.reps, sync)

    if not a.skip_cpu:
        torch.set_num_threads(a.threads)
        cpu = lambda: [pv.pv_score(q, rgb, xyz, P, a.focal, device="cpu")[0] for P in poses]             # noqa: E731
        res["cpu_threads"] = a.threads
        res["loop_cpu_s"], res["loop_cpu_s_all"], s_cpu = _timed(cpu, a.cpu_reps)
        res["loop_cpu_scores"] = [round(s, 4) for s in s_cpu]
        if "batch_s" in res:
            res["speedup_vs_loop_cpu"] = res["loop_cpu_s"] / res["batch_s"]
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
