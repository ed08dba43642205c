"""Shared cases of the augmentation tests (tests/test_augment_cpu.py on the fp64
oracle, tests/test_gpu_warp_input.py on the HIP kernel)."""
import math

import torch

from ncnet_amd.data.augment import PairAugment, draw_params, transform_points
from ncnet_amd.data.transforms import IMAGENET_MEAN, IMAGENET_STD

# the ranges of the "pixels and keypoints move together" check
BLOB_AUG = PairAugment(rot_deg=30.0, scale=(0.7, 1.4), shift=0.1, flip=0.5, gain=(1.0, 1.0), bias=0.0)
BLOB_SIGMA = 2.0
BLOB_DRAWS = 24


def pack(images):
    """HWC uint8 images -> (pixels, meta) as collate_uint8_pairs packs them."""
    sizes = [int(x.numel()) for x in images]
    offs = [0]
    for s in sizes[:-1]:
        offs.append(offs[-1] + s)
    meta = torch.tensor([[o, x.shape[0], x.shape[1]] for o, x in zip(offs, images)], dtype=torch.int64)
    return torch.cat([x.reshape(-1) for x in images]), meta


def blob_image(h, w, x, y, sigma=BLOB_SIGMA):
    """[h, w, 3] uint8: one 8-bit Gaussian blob centred on the 0-based position (x, y)."""
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    g = torch.exp(-((xs - x) ** 2 + (ys - y) ** 2) / (2 * sigma ** 2))
    return torch.round(255 * g).to(torch.uint8).unsqueeze(2).expand(h, w, 3).contiguous()


def blob_cases(n=BLOB_DRAWS, seed=11):
    """n pairs of blob images (sources 30-60 px, outputs 24-50 px) with one
    keypoint each, at least 8 px inside its source so that the border the warp
    replicates is black.  Returns a list of dicts: images (2 HWC uint8), points
    [2, 2, 1] (1-based; image 0 = source, 1 = target of the pair), oh, ow,
    params [2, 8]."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))  # noqa: E731
    cases = []
    for _ in range(n):
        ims, pts = [], []
        for _side in range(2):
            h, w = ri(30, 60), ri(30, 60)
            x = 8 + float(torch.rand(1, generator=g, dtype=torch.float64)) * (w - 1 - 16)
            y = 8 + float(torch.rand(1, generator=g, dtype=torch.float64)) * (h - 1 - 16)
            ims.append(blob_image(h, w, x, y))
            pts.append([[x + 1], [y + 1]])
        oh, ow = ri(24, 50), ri(24, 50)
        _, meta = pack(ims)
        cases.append({"images": ims, "points": torch.tensor(pts, dtype=torch.float64), "oh": oh, "ow": ow,
                      "params": draw_params(meta, oh, ow, BLOB_AUG, g)})
    return cases


def centroid(warped):
    """Intensity centroid (x, y), 0-based, of channel 0 of one normalised [3, oh, ow] output."""
    inten = warped[0].double() * IMAGENET_STD[0] + IMAGENET_MEAN[0]
    oh, ow = inten.shape
    tot = inten.sum()
    return (float((inten.sum(0) * torch.arange(ow, dtype=torch.float64)).sum() / tot),
            float((inten.sum(1) * torch.arange(oh, dtype=torch.float64)).sum() / tot))


def blob_errors(cases, warp):
    """``warp(pixels, meta, params, oh, ow)`` -> [2, 3, oh, ow].  Returns
    (distance centroid <-> transformed keypoint in px, keypoint's distance to
    the output border in px) of every image whose keypoint stays in the frame."""
    out = []
    for c in cases:
        pix, meta = pack(c["images"])
        img = warp(pix, meta, c["params"], c["oh"], c["ow"]).cpu()
        new = transform_points(c["points"], c["params"], c["oh"], c["ow"])
        for i in range(2):
            x, y = float(new[i, 0, 0]) - 1, float(new[i, 1, 0]) - 1
            if new[i, 0, 0] == -1:
                continue
            cx, cy = centroid(img[i])
            inside = min(x, y, c["ow"] - 1 - x, c["oh"] - 1 - y)
            out.append((math.hypot(cx - x, cy - y), inside))
    return out
