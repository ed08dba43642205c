#!/usr/bin/env python
"""Write N JPEG pairs WITH keypoints in PF-Pascal size ranges (longest side
300-500 px, 4:3 / 3:4 / square) plus train / val CSVs in the ``test_pairs.csv``
layout (``source_image,target_image,class,XA,YA,XB,YB``, ``;``-separated point
lists, 1-based pixels) -- the input of ``train.py --loss strong
--train_pairs_csv ... --val_pairs_csv ...`` when PF-Pascal cannot be
downloaded: the benchmark set of the keypoint input path and the data of its
command-line tests.

The target of a pair is a known similarity warp of its source: target pixel
``p_t`` (0-based) shows source position ``p_s = s R(theta) (p_t - c_t) + c_s +
d`` (border replicated), where ``s`` also maps the target's size onto the
source's.  Each pair gets 8-20 keypoints drawn in the target whose
correspondences ``p_s`` lie inside the source.  Seeded; nothing is downloaded.

    python scripts/make_keypoint_pairs.py --out /tmp/kp_pairs --pairs 640
"""
import argparse
import os

import numpy as np
from PIL import Image


def _size(rng, lo, hi):
    long = int(rng.integers(lo, hi + 1))
    short = int(long * rng.choice([0.75, 1.0]))
    return (short, long) if rng.random() < 0.6 else (long, short)          # (h, w)


def _photo(rng, h, w):
    """Smooth colour field + noise: JPEG decode cost like a photo, not like flat colour."""
    base = rng.integers(0, 256, size=(h // 16 + 2, w // 16 + 2, 3), dtype=np.uint8)
    im = Image.fromarray(base).resize((w, h), Image.BICUBIC)
    arr = np.asarray(im).astype(np.int16) + rng.integers(-20, 21, size=(h, w, 3))
    return np.clip(arr, 0, 255).astype(np.uint8)


def _sample(src, sx, sy):
    """Bilinear samples of ``src`` [h, w, 3] uint8 at float positions (border replicated)."""
    h, w, _ = src.shape
    sx, sy = np.clip(sx, 0, w - 1), np.clip(sy, 0, h - 1)
    x0, y0 = np.minimum(sx.astype(np.int64), w - 1), np.minimum(sy.astype(np.int64), h - 1)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = (sx - x0)[..., None].astype(np.float32), (sy - y0)[..., None].astype(np.float32)
    v = (1 - fy) * ((1 - fx) * src[y0, x0] + fx * src[y0, x1]) + fy * ((1 - fx) * src[y1, x0] + fx * src[y1, x1])
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def make_pair(rng, lo=300, hi=500):
    """(source uint8 [hs, ws, 3], target uint8 [ht, wt, 3], source points [n, 2],
    target points [n, 2]) with 0-based (x, y) points, 8 <= n <= 20."""
    hs, ws = _size(rng, lo, hi)
    ht, wt = _size(rng, lo, hi)
    src = _photo(rng, hs, ws)
    theta = np.deg2rad(rng.uniform(-20, 20))
    s = rng.uniform(0.8, 1.1) * min((ws - 1) / (wt - 1), (hs - 1) / (ht - 1))
    A = s * np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])
    c_t = np.array([(wt - 1) / 2, (ht - 1) / 2])
    t = np.array([(ws - 1) / 2, (hs - 1) / 2]) + rng.uniform(-0.05, 0.05, 2) * np.array([ws - 1, hs - 1]) - A @ c_t
    ys, xs = np.mgrid[0:ht, 0:wt].astype(np.float64)
    tgt = _sample(src, A[0, 0] * xs + A[0, 1] * ys + t[0], A[1, 0] * xs + A[1, 1] * ys + t[1])
    n = int(rng.integers(8, 21))
    pt, ps = np.zeros((0, 2)), np.zeros((0, 2))
    while len(pt) < n:                       # the centre of the target always maps inside: this ends
        cand = rng.uniform(0.05, 0.95, (4 * n, 2)) * np.array([wt - 1, ht - 1])
        cs = cand @ A.T + t
        ok = ((cs >= 0) & (cs <= np.array([ws - 1, hs - 1]))).all(1)
        pt, ps = np.concatenate((pt, cand[ok])), np.concatenate((ps, cs[ok]))
    return src, tgt, ps[:n], pt[:n]


def _join(v):
    return ";".join(f"{x:.4f}" for x in v)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--pairs", type=int, default=640)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--min_side", type=int, default=300, help="range of the longest side (tests use tiny images)")
    ap.add_argument("--max_side", type=int, default=500)
    a = ap.parse_args(argv)
    rng = np.random.default_rng(a.seed)
    img_dir = os.path.join(a.out, "images")
    os.makedirs(img_dir, exist_ok=True)
    os.makedirs(os.path.join(a.out, "image_pairs"), exist_ok=True)
    rows = []
    for i in range(a.pairs):
        src, tgt, ps, pt = make_pair(rng, a.min_side, a.max_side)
        names = [f"images/pair_{i:05d}_{side}.jpg" for side in "ab"]
        for name, im in zip(names, (src, tgt)):
            Image.fromarray(im).save(os.path.join(a.out, name), quality=90)
        # the CSV is 1-based, as the PF-Pascal annotations
        rows.append(f"{names[0]},{names[1]},{i % 20 + 1},{_join(ps[:, 0] + 1)},{_join(ps[:, 1] + 1)},"
                    f"{_join(pt[:, 0] + 1)},{_join(pt[:, 1] + 1)}")
    nval = max(1, a.pairs // 10)
    for fn, part in (("train_pairs.csv", rows[nval:]), ("val_pairs.csv", rows[:nval])):
        with open(os.path.join(a.out, "image_pairs", fn), "w") as f:
            f.write("source_image,target_image,class,XA,YA,XB,YB\n" + "\n".join(part) + "\n")
    print(f"wrote {a.pairs} keypoint pairs to {a.out}")


if __name__ == "__main__":
    main()
