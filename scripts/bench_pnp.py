#!/usr/bin/env python
"""Time the batched GPU P3P LO-RANSAC (eval/localization_gpu.py, csrc/pnp.hip)
against the numpy back end (eval/localization.py p3p_ransac on worker
processes, what inloc_localize.py --pnp_device cpu runs) on a synthetic problem
set sized like an InLoc run.

Problem set (seeded): --problems pairs (default 3560 = 356 queries x 10
cutouts), each with uniform[--min_pts, --max_pts] tentatives.  A fraction
--consensus of them (default 0.1: about one cutout of a shortlist shows the
query's place) holds a true pose with 50-90 % outliers and 1e-4 ray noise; the
others are mismatches (rays and points unrelated), which never reach consensus
and run all --max_iters hypotheses.  Threshold 0.2 degrees, confidence 0.999,
20 local-optimisation samples: the defaults of inloc_localize.py.

The GPU time is the whole call (packing, one H2D copy, one launch, one D2H
copy, unpacking), median of --reps.  The numpy path takes seconds per mismatch
problem, so it is timed on the first --cpu_problems problems of the same set on
--workers processes and scaled to the whole set by the problem count.

    python scripts/bench_pnp.py [--problems 3560] [--cpu_problems 64] [--workers 16] [--skip_cpu]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ncnet_amd.eval.localization import p3p_ransac  # noqa: E402
from ncnet_amd.eval.localization_gpu import p3p_ransac_batch  # noqa: E402


def make_problems(n_problems, min_pts, max_pts, consensus, seed):
    rng = np.random.default_rng(seed)
    problems, has_pose = [], []
    for _ in range(n_problems):
        n = int(rng.integers(min_pts, max_pts + 1))
        Xc = np.stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.uniform(3, 8, n)])
        Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(Q) < 0:
            Q[:, 0] *= -1
        t = rng.normal(size=3)
        Xw = Q.T @ (Xc - t[:, None])
        good = rng.random() < consensus
        rays = Xc / np.linalg.norm(Xc, axis=0) + rng.normal(scale=1e-4, size=Xc.shape)
        out = rng.random(n) < (rng.uniform(0.5, 0.9) if good else 1.0)
        rays[:, out] = rng.normal(size=(3, int(out.sum())))
        rays[2, out] = np.abs(rays[2, out])
        problems.append((rays, Xw))
        has_pose.append(good)
    return problems, np.array(has_pose)


def _cpu_one(task):
    rays, X, key, thr, max_iters = task
    P, inl = p3p_ransac(rays, X, thr, max_iters, rng=np.random.default_rng(key))
    return int(inl.sum())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--problems", type=int, default=3560)
    ap.add_argument("--min_pts", type=int, default=1000)
    ap.add_argument("--max_pts", type=int, default=4000)
    ap.add_argument("--consensus", type=float, default=0.1)
    ap.add_argument("--max_iters", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu_problems", type=int, default=64)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--skip_cpu", action="store_true")
    ap.add_argument("--skip_gpu", action="store_true")
    a = ap.parse_args(argv)
    thr = np.radians(0.2)
    problems, has_pose = make_problems(a.problems, a.min_pts, a.max_pts, a.consensus, a.seed)
    keys = list(range(a.problems))
    res = {"problems": a.problems, "tentatives": int(sum(r.shape[1] for r, _ in problems)),
           "with_consensus": int(has_pose.sum()), "max_iters": a.max_iters}

    if not a.skip_gpu:
        import torch
        assert torch.cuda.is_available(), "the GPU half needs a GPU (--skip_gpu times numpy only)"
        p3p_ransac_batch(problems[:8], thr, a.max_iters, keys=keys[:8])          # load + warm up
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out, rounds = p3p_ransac_batch(problems, thr, a.max_iters, keys=keys, return_rounds=True)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        found = np.array([P is not None and inl.sum() >= 0.05 * inl.size for P, inl in out])
        res.update(gpu_s=float(np.median(times)), gpu_s_all=[round(t, 4) for t in times],
                   gpu_consensus_found=int((found & has_pose).sum()), gpu_false_consensus=int((found & ~has_pose).sum()),
                   gpu_full_length_problems=int((rounds == -(-a.max_iters // 256)).sum()))

    if not a.skip_cpu:
        import multiprocessing as mp
        from concurrent.futures import ProcessPoolExecutor
        k = min(a.cpu_problems, a.problems)
        tasks = [(r, x, key, thr, a.max_iters) for (r, x), key in zip(problems[:k], keys[:k])]
        with ProcessPoolExecutor(max_workers=a.workers, mp_context=mp.get_context("spawn")) as ex:
            list(ex.map(_cpu_one, [t[:4] + (1,) for t in tasks[: a.workers]]))     # start the workers (1 hypothesis)
            t0 = time.perf_counter()
            list(ex.map(_cpu_one, tasks))
            dt = time.perf_counter() - t0
        res.update(cpu_workers=a.workers, cpu_problems=k, cpu_with_consensus=int(has_pose[:k].sum()), cpu_s=dt,
                   cpu_s_scaled_to_all=dt * a.problems / k)
        if "gpu_s" in res:
            res["speedup_vs_cpu_workers"] = res["cpu_s_scaled_to_all"] / res["gpu_s"]
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
