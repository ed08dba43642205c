#!/usr/bin/env python
"""Timings of the relocalized-training front end at the training shape:
V = 2B volumes (the weak loss's positives + rolled negatives) of 50 x 50 grids,
K = 1024 (--image_size 800, k = 2).

* forward: the mapped fused pool (corr_gemm_pool2 with pair maps) against the
  unfused mapped correlation + maxpool4d;
* backward: corr_pool2_bwd (both directions, transposed operand copies
  included) against the only differentiable alternative without it: scatter g
  into the dense [V, M, N] fp32 volume, then the two fp32 bmm + index_add_ of
  CorrelationFn.backward.

The cases of a group are timed interleaved (A B A B ...), --rounds rounds of
--reps calls each between device events after a warm-up call; the table gives
the median and the min .. max over rounds.  Outputs of the two backward forms
are compared once (rel. L2) on the same inputs.

    python scripts/reloc_bench.py [--batch 16] [--grid 50] [--k 1024] [--rounds 7] [--reps 5] [--json out.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ncnet_amd.ops import _ext  # noqa: E402

co = importlib.import_module("ncnet_amd.ops.correlation")   # the package re-exports the function under this name


def timeit(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def interleaved(cases, rounds, reps):
    for fn in cases.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(rounds):
        for k, fn in cases.items():
            ms[k].append(timeit(fn, reps))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--grid", type=int, default=50)
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", type=str, default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("reloc_bench.py measures on the GPU; none found")
    dev = "cuda"
    B, h, K = a.batch, a.grid, a.k
    M = h * h
    ar = tuple(range(B))
    amap, bmap = ar + ar[1:] + ar[:1], ar + ar
    V = len(amap)
    g0 = torch.Generator(device=dev).manual_seed(1)
    fa = torch.nn.functional.normalize(torch.randn(B, M, K, device=dev, generator=g0), dim=-1).to(torch.bfloat16)
    fb = torch.nn.functional.normalize(torch.randn(B, M, K, device=dev, generator=g0), dim=-1).to(torch.bfloat16)
    am, bm = co._device_map(amap, dev), co._device_map(bmap, dev)

    def fwd_fused():
        return co.correlation_pool2(fa, fb, h, h, h, h, packed=True, amap=amap, bmap=bmap)

    def fwd_unfused():
        return co.maxpool4d(co.correlation(fa, fb, am, bm).view(V, 1, h, h, h, h), 2)

    out = {"shape": {"V": V, "grid": h, "K": K}}
    with torch.no_grad():
        out["forward"] = interleaved({"mapped fused pool": fwd_fused, "correlation + maxpool4d": fwd_unfused},
                                     a.rounds, a.reps)
        pooled, code = fwd_fused()
    g = torch.randn(pooled.shape, device=dev, generator=g0)
    pa = co.block_order_index(h, h, 2, dev)
    ablk, bblk = fa[:, pa].contiguous(), fb[:, pa].contiguous()
    inv = co.block_order_inverse(h, h, 2, dev)
    aml, bml = am.long(), bm.long()
    # natural-order scatter targets of the dense baseline, from the forward's codes
    c = code.reshape(V, h // 2, h // 2, h // 2, h // 2).long()
    rng = lambda pos: torch.arange(h // 2, device=dev).view([h // 2 if i == pos else 1 for i in range(5)])   # noqa: E731
    row_a = (2 * rng(1) + ((c >> 6) & 1)) * h + 2 * rng(2) + ((c >> 4) & 1)
    row_b = (2 * rng(3) + ((c >> 2) & 1)) * h + 2 * rng(4) + (c & 1)
    target = (row_a * M + row_b).reshape(V, -1)

    def bwd_kernel():
        ga, gb = co.corr_pool2_bwd(ablk, bblk, g, code, amap, bmap, h, h, h, h)
        return ga[:, inv], gb[:, inv]

    def bwd_dense():
        full = torch.zeros(V, M * M, device=dev)
        full.scatter_(1, target, g.reshape(V, -1))
        full = full.view(V, M, M)
        ga = torch.zeros(fa.shape, dtype=torch.float32, device=dev)
        ga.index_add_(0, aml, torch.bmm(full, fb.float()[bml]))
        gb = torch.zeros(fb.shape, dtype=torch.float32, device=dev)
        gb.index_add_(0, bml, torch.bmm(full.transpose(1, 2), fa.float()[aml]))
        return ga, gb

    with torch.no_grad():
        ka, kb = bwd_kernel()
        da, db = bwd_dense()
        rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm())   # noqa: E731
        out["backward_rel_l2_kernel_vs_dense"] = {"gA": rel(ka, da), "gB": rel(kb, db)}
        del ka, kb, da, db
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        bwd_kernel()
        out["backward_peak_extra_mb"] = {"corr_pool2_bwd": (torch.cuda.max_memory_allocated() - base) / 2 ** 20}
        torch.cuda.reset_peak_memory_stats()
        bwd_dense()
        out["backward_peak_extra_mb"]["dense scatter + 2 fp32 bmm"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        out["backward"] = interleaved({"corr_pool2_bwd": bwd_kernel, "dense scatter + 2 fp32 bmm": bwd_dense},
                                      a.rounds, a.reps)
    flops = 2 * 2.0 * V * M * M * K            # both directions, as a dense GEMM
    out["backward"]["corr_pool2_bwd"]["dense_equiv_tflops"] = flops / out["backward"]["corr_pool2_bwd"]["median_ms"] / 1e9
    assert _ext.DISPATCH["torch_fallback"] == 0
    for grp in ("forward", "backward"):
        print(f"{grp} (V = {V}, {h} x {h} grids, K = {K}; {a.rounds} rounds x {a.reps} calls, interleaved)")
        for k, v in out[grp].items():
            print(f"  {k:30s} median {v['median_ms']:8.3f} ms   min {v['min_ms']:8.3f}   max {v['max_ms']:8.3f}")
    print("backward, kernel vs dense baseline (g rounded to bf16 in the kernel only): rel. L2", out["backward_rel_l2_kernel_vs_dense"])
    print("backward, peak extra memory (MB):", out["backward_peak_extra_mb"])
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
