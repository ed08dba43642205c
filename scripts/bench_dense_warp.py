#!/usr/bin/env python
"""Time the fused dense correspondence loss (csrc/densece.hip) on fixed data.

Per batch size, at the 25^4 training plane with maps drawn by draw_params:
  fused      forward + backward through warp_loss_from_corr (autograd)
  table      densece_table (cells, weights, valid flags from the maps)
  stats2d    the one-pass row + column statistics the forward reads
  fwd        densece_fwd (log-sum-exps and terms: four gathers per cell)
  reduce     densece_reduce (two one-wave launches)
  bwd        densece_bwd (reads and writes the volume once)
  weak_bwd   softmax_max_bwd at the same shape with V = B: it also reads and
             writes the volume exactly once
The cases run interleaved for ``--rounds`` rounds after a warm-up; each sample
is the mean of ``--iters`` back-to-back calls between two events.  Prints one
JSON line per batch size: median and min / max (the spread) in microseconds.

    python scripts/bench_dense_warp.py --batch 16 256 --rounds 7
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ncnet_amd.data.augment import PairAugment, draw_params, view_maps  # noqa: E402
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args(argv)
    dev = "cuda"
    C = _ext.ext()
    g = a.grid
    n = g * g
    for B in a.batch:
        torch.manual_seed(0)
        x = (torch.rand(B, 1, g, g, g, g, device=dev) * 3).requires_grad_(True)
        meta = torch.tensor([[0, 375, 500]] * (2 * B), dtype=torch.int64)
        params = draw_params(meta, 400, 400, PairAugment(), torch.Generator().manual_seed(B))
        maps = view_maps(params, meta, 400, 400).to(dev)
        batch = {"warp_maps": maps}
        x3 = x.detach().reshape(B, n, n)
        i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
        cells, wts = torch.empty((B, 2, 4, n), **i32), torch.empty((B, 2, 4, n), **f32)
        valid = torch.empty((B, 2, n), **i32)
        lse, term, out = torch.empty((B, 2, n), **f32), torch.empty((B, 2, n), **f32), torch.empty(3, **f32)
        gx = torch.empty_like(x3)
        one = torch.ones(1, **f32)
        st = loss_ops._row_col_stats(x3, 1)
        wr = torch.full((B,), 1.0 / (2.0 * B * n), **f32)

        def fused():
            x.grad = None
            loss_ops.warp_loss_from_corr(x, batch).backward()

        cases = {
            "fused": fused,
            "table": lambda: C.densece_table(maps, g, g, g, g, cells, wts, valid),
            "stats2d": lambda: loss_ops._row_col_stats(x3, 1),
            "fwd": lambda: C.densece_fwd(x3, cells, wts, valid, st[0], st[2], st[3], st[5], lse, term),
            "reduce": lambda: C.densece_reduce(term, valid, out),
            "bwd": lambda: C.densece_bwd(x3, cells, wts, lse, out, gx, one),
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
        rec = {"batch": B, "grid": g, "valid_share": round(float(valid.float().mean()), 3), "rounds": a.rounds,
               "iters": a.iters,
               "us": {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                      for k, v in samples.items()}}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
