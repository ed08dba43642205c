#!/usr/bin/env python
"""Time the fused keypoint-supervised loss (csrc/kploss.hip) on fixed data.

Per batch size, at the 25^4 training plane with N keypoints per image:
  fused      forward + backward through strong_loss_from_corr (autograd)
  fused_fwd  the kploss_fwd binding alone (table, log-sum-exps, reduction)
  fused_bwd  the kploss_bwd binding alone (writes the volume once)
  oracle     ops/reference.py keypoint_ce forward + backward on the same GPU
  weak_bwd   softmax_max_bwd at the same shape with V = B: it also writes the
             volume exactly once -- the natural floor of the backward
The cases run interleaved for ``--rounds`` rounds after a warm-up; each sample
is the mean of ``--iters`` back-to-back calls between two events.  Prints one
JSON line per batch size: median and min / max (the spread) in microseconds.

    python scripts/bench_strong_loss.py --batch 16 256 --rounds 7
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ncnet_amd.ops import _ext  # noqa: E402
from ncnet_amd.ops import loss as loss_ops  # noqa: E402
from ncnet_amd.ops import reference as ref  # noqa: E402


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / iters


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[16, 256])
    ap.add_argument("--grid", type=int, default=25)
    ap.add_argument("--points", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args(argv)
    dev = "cuda"
    C = _ext.ext()
    g, n = a.grid, a.points
    for B in a.batch:
        torch.manual_seed(0)
        x = (torch.rand(B, 1, g, g, g, g, device=dev) * 3).requires_grad_(True)
        size = 16.0 * g
        sp = 1 + torch.rand(B, 2, n, device=dev) * (size - 1)
        tp = 1 + torch.rand(B, 2, n, device=dev) * (size - 1)
        sz = torch.tensor([size, size, 3.0], device=dev).expand(B, 3).contiguous()
        batch = {"source_points": sp, "target_points": tp, "source_im_size": sz, "target_im_size": sz}
        x3 = x.detach().reshape(B, g * g, g * g)
        i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
        cells, wts, valid = torch.empty((B, n, 8), **i32), torch.empty((B, n, 8), **f32), torch.empty((B, n), **i32)
        lse, term, out = torch.empty((B, n, 2), **f32), torch.empty((B, n, 2), **f32), torch.empty(2, **f32)
        gx = torch.empty_like(x3)
        one = torch.ones(1, **f32)
        st = loss_ops._row_col_stats(x3, 1)
        wr = torch.full((B,), 1.0 / (2.0 * B * g * g), **f32)

        def fused():
            x.grad = None
            loss_ops.strong_loss_from_corr(x, batch).backward()

        def oracle():
            x.grad = None
            ref.keypoint_ce(x, sp, tp, sz, sz).backward()

        cases = {
            "fused": fused,
            "fused_fwd": lambda: C.kploss_fwd(x3, sp, tp, sz, sz, g, g, g, g, cells, wts, valid, lse, term, out),
            "fused_bwd": lambda: C.kploss_bwd(x3, cells, wts, valid, lse, out[1:], gx, one),
            "oracle": oracle,
            "weak_bwd": lambda: C.softmax_max_bwd(x3, st[0], st[1], st[2], st[3], st[4], st[5], wr, wr, gx, 1,
                                                  ref.L1_EPS, one),
        }
        for _ in range(a.warmup):
            for fn in cases.values():
                fn()
        torch.cuda.synchronize()
        samples = {k: [] for k in cases}
        for _ in range(a.rounds):
            for k, fn in cases.items():
                samples[k].append(timed(fn, a.iters))
        rec = {"batch": B, "grid": g, "points": n, "rounds": a.rounds, "iters": a.iters,
               "us": {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                      for k, v in samples.items()}}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
