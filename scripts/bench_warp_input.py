#!/usr/bin/env python
"""Time the two input kernels of csrc/dataprep.hip on fixed data: N random
images in PF-Pascal size ranges (longest side 300-500 px), packed as
``collate_uint8_pairs`` packs them, to 400 x 400:
  resize     resize_norm_u8
  warp_id    warp_norm_u8 on the plain-resize rows (same pixels read)
  warp_aug   warp_norm_u8 on rows drawn from the default PairAugment
The cases run interleaved for ``--rounds`` rounds after a warm-up; each sample
is the mean of ``--iters`` back-to-back launches between two events.  Prints
one JSON line: median and min / max (the spread) in microseconds, and the bytes
the kernel must move (pixels read once + fp32 output) over the median.

    python scripts/bench_warp_input.py --images 32 --rounds 7
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ncnet_amd.data.augment import PairAugment, draw_params, resize_params  # noqa: E402
from ncnet_amd.data.transforms import IMAGENET_MEAN, IMAGENET_STD  # noqa: E402
from ncnet_amd.ops import _ext  # noqa: E402


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
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args(argv)
    dev = "cuda"
    C = _ext.ext()
    g = torch.Generator().manual_seed(0)
    metas, off = [], 0
    for _ in range(a.images):
        long = int(torch.randint(300, 501, (1,), generator=g))
        short = int(long * (0.75 if float(torch.rand(1, generator=g)) < 0.5 else 1.0))
        h, w = (short, long) if float(torch.rand(1, generator=g)) < 0.6 else (long, short)
        metas.append([off, h, w])
        off += h * w * 3
    meta = torch.tensor(metas, dtype=torch.int64)
    pix = torch.randint(0, 256, (off,), generator=g, dtype=torch.uint8).to(dev)
    meta_d = meta.to(dev)
    p_id = resize_params(meta, a.size, a.size).to(dev)
    p_aug = draw_params(meta, a.size, a.size, PairAugment(), g).to(dev)
    out = torch.empty((a.images, 3, a.size, a.size), dtype=torch.float32, device=dev)
    mean, std = list(IMAGENET_MEAN), list(IMAGENET_STD)
    cases = {
        "resize": lambda: C.resize_norm_u8(pix, meta_d, out, mean, std),
        "warp_id": lambda: C.warp_norm_u8(pix, meta_d, p_id, out, mean, std),
        "warp_aug": lambda: C.warp_norm_u8(pix, meta_d, p_aug, out, mean, std),
    }
    for _ in range(a.warmup):
        for fn in cases.values():
            timed(fn, a.iters)
    torch.cuda.synchronize()
    samples = {k: [] for k in cases}
    for _ in range(a.rounds):
        for k, fn in cases.items():
            samples[k].append(timed(fn, a.iters))
    nbytes = off + out.numel() * 4
    rec = {"images": a.images, "size": a.size, "pixel_bytes": off, "out_bytes": out.numel() * 4, "rounds": a.rounds,
           "iters": a.iters,
           "us": {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2),
                      "GBps_at_median": round(nbytes / statistics.median(v) / 1e3, 1)}
                  for k, v in samples.items()}}
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
