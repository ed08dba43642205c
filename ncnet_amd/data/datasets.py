"""Pair datasets (lib/im_pair_dataset.py, lib/pf_dataset.py) and synthetic pairs.

CSV formats:
* train / val: ``source_image,target_image,class,flip``
* PF-Pascal test: ``source_image,target_image,class,XA,YA,XB,YB`` with ``;``
  separated point lists.
"""
from __future__ import annotations

import os

import numpy as np
import pandas as pd
import torch
from torch.utils.data import Dataset

from .transforms import read_image, resize_bilinear, to_chw_float

PF_CATEGORIES = ["aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow",
                 "diningtable", "dog", "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train",
                 "tvmonitor"]


class ImagePairDataset(Dataset):
    """Weakly supervised image pairs (lib/im_pair_dataset.py:11-93)."""

    def __init__(self, dataset_csv_path, dataset_csv_file, dataset_image_path, dataset_size=0,
                 output_size=(240, 240), transform=None, random_crop=False, gpu_resize=False):
        """``gpu_resize``: return the decoded (cropped / flipped) images as
        uint8 CHW tensors of their own size and let the consumer resize +
        normalise the batch on the GPU (``gpu_pair_batch``; collate with
        ``collate_uint8_pairs``) -- the DataLoader workers then only decode."""
        self.random_crop = random_crop
        self.gpu_resize = gpu_resize
        self.out_h, self.out_w = output_size
        data = pd.read_csv(os.path.join(dataset_csv_path, dataset_csv_file))
        if dataset_size:
            data = data.iloc[: min(dataset_size, len(data))]
        self.img_A_names = data.iloc[:, 0].tolist()
        self.img_B_names = data.iloc[:, 1].tolist()
        self.set = data.iloc[:, 2].to_numpy()
        self.flip = data.iloc[:, 3].to_numpy().astype("int")
        self.dataset_image_path = dataset_image_path
        self.transform = transform

    def __len__(self):
        return len(self.img_A_names)

    def get_image(self, name, flip):
        image = read_image(os.path.join(self.dataset_image_path, name))
        if self.random_crop:
            h, w, _ = image.shape
            top = np.random.randint(h // 4)
            bottom = int(3 * h / 4 + np.random.randint(h // 4))
            left = np.random.randint(w // 4)
            right = int(3 * w / 4 + np.random.randint(w // 4))
            image = image[top:bottom, left:right, :]
        if flip:
            image = np.flip(image, 1)
        im_size = torch.tensor(image.shape, dtype=torch.float32)
        if self.gpu_resize:          # HWC uint8 as decoded; packed per batch by collate_uint8_pairs
            return torch.from_numpy(np.ascontiguousarray(image)), im_size
        img = resize_bilinear(to_chw_float(image), self.out_h, self.out_w)
        return img, im_size

    def __getitem__(self, idx):
        a, sa = self.get_image(self.img_A_names[idx], self.flip[idx])
        b, sb = self.get_image(self.img_B_names[idx], self.flip[idx])
        sample = {"source_image": a, "target_image": b, "source_im_size": sa, "target_im_size": sb,
                  "set": int(self.set[idx])}
        if self.transform and not self.gpu_resize:
            sample = self.transform(sample)
        return sample


def collate_uint8_pairs(samples):
    """Batch of ``gpu_resize`` samples (runs in the DataLoader workers): the
    decoded HWC uint8 pixels of all 2B images are packed into ONE byte buffer
    ``pixels`` with a table ``pixel_meta`` [2B, 3] = (byte offset, H, W)
    (sources first, then targets) -- one pinned tensor, one host->device copy;
    everything else is stacked."""
    imgs = [s["source_image"] for s in samples] + [s["target_image"] for s in samples]
    sizes = [int(x.numel()) for x in imgs]
    offs = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.int64)
    meta = torch.tensor([[o, x.shape[0], x.shape[1]] for o, x in zip(offs, imgs)], dtype=torch.int64)
    out = {"pixels": torch.cat([x.reshape(-1) for x in imgs]), "pixel_meta": meta}
    for k in samples[0]:
        if k in ("source_image", "target_image"):
            continue
        vals = [s[k] for s in samples]
        out[k] = torch.stack(vals) if torch.is_tensor(vals[0]) else torch.tensor(vals)
    return out


def gpu_pair_batch(batch, device, out_h: int, out_w: int, augment=None, generator=None):
    """Move a ``collate_uint8_pairs`` batch to ``device`` (uint8 pixels: 4x
    fewer bytes than float, one non-blocking copy) and resize + normalise all
    images there in one HIP launch (csrc/dataprep.hip): bilinear with
    align_corners=True as the reference's identity AffineTnf
    (lib/transformation.py), then ImageNet normalisation
    (lib/normalization.py).  On CPU the same math runs through torch.

    ``augment`` (a ``data.augment.PairAugment``, with a CPU ``generator``): the
    launch is ``warp_norm_u8`` instead, which also warps and jitters every
    image by a row of parameters drawn here on the host (``draw_params``) and
    uploaded next to ``pixel_meta``.  If the batch carries keypoints they are
    moved through the same maps on the host first: ``source_points`` /
    ``target_points`` are rewritten in the output frame (index k of BOTH sets
    becomes -1 when either point leaves its frame), ``source_im_size`` /
    ``target_im_size`` become ``(out_h, out_w, 3)``; ``L_pck`` stays."""
    from .transforms import IMAGENET_MEAN, IMAGENET_STD, gpu_normalize_resize
    from ..ops import _ext
    pix, meta = batch["pixels"], batch["pixel_meta"]
    n = meta.shape[0]
    ends = meta[:, 0] + meta[:, 1] * meta[:, 2] * 3
    if int(ends.max()) > pix.numel() or int(meta[:, 1:].min()) < 1:
        raise ValueError("malformed pixel table")
    params = None
    if augment is not None:
        from .augment import draw_params, transform_pair_points
        params = draw_params(meta, out_h, out_w, augment, generator)
        if "source_points" in batch:
            sp, tp = transform_pair_points(batch["source_points"], batch["target_points"], params, out_h, out_w)
            size = torch.tensor([float(out_h), float(out_w), 3.0]).expand(n // 2, 3).contiguous()
            batch = dict(batch, source_points=sp, target_points=tp, source_im_size=size, target_im_size=size.clone())
    res = {k: (v.to(device, non_blocking=True) if torch.is_tensor(v) else v) for k, v in batch.items()
           if k not in ("pixels", "pixel_meta")}
    dev = torch.device(device)
    pix_d = pix.to(dev, non_blocking=True) if dev.type == "cuda" else None   # the batch's ONE pixel copy
    if pix_d is not None and _ext.use_hip(pix_d):
        out = torch.empty((n, 3, out_h, out_w), dtype=torch.float32, device=dev)
        if params is None:
            _ext.ext().resize_norm_u8(pix_d, meta.to(dev, non_blocking=True), out, list(IMAGENET_MEAN),
                                      list(IMAGENET_STD))
        else:
            _ext.ext().warp_norm_u8(pix_d, meta.to(dev, non_blocking=True), params.to(dev, non_blocking=True), out,
                                    list(IMAGENET_MEAN), list(IMAGENET_STD))
    elif params is not None:
        from ..ops.reference import warp_norm_u8
        out = warp_norm_u8(pix, meta, params, out_h, out_w, IMAGENET_MEAN, IMAGENET_STD, dtype=torch.float32).to(dev)
    else:
        ims = []
        for o, h, w in meta.tolist():
            x = pix[o:o + h * w * 3].view(h, w, 3).permute(2, 0, 1).unsqueeze(0).to(dev)
            ims.append(gpu_normalize_resize(x, out_h, out_w))
        out = torch.cat(ims)
    b = n // 2
    res["source_image"], res["target_image"] = out[:b], out[b:]
    return res


class SingleImageDataset(Dataset):
    """Single images for warp-supervised training (``train.py --loss warp``):
    item i is ``{"image": HWC uint8 as decoded}`` of ``names[i]`` under
    ``image_root`` -- the workers only decode; the two views of every image are
    cut on the device (``gpu_view_batch``).  Collate with ``collate_uint8_images``."""

    def __init__(self, image_root, names):
        self.image_root = image_root
        self.names = list(names)

    def __len__(self):
        return len(self.names)

    def __getitem__(self, idx):
        image = read_image(os.path.join(self.image_root, self.names[idx]))
        return {"image": torch.from_numpy(np.ascontiguousarray(image))}


class SyntheticImageDataset(Dataset):
    """Low-pass noise uint8 images of a fixed size (``train.py --loss warp
    --synthetic N``): item i is a sum of upsampled noise octaves, deterministic
    per (seed, index), as ``{"image": HWC uint8}``."""

    def __init__(self, n: int = 64, hw=(400, 400), seed: int = 0):
        self.length = int(n)
        self.h, self.w = (hw, hw) if isinstance(hw, int) else hw
        self.seed = seed

    def __len__(self):
        return self.length

    def __getitem__(self, idx):
        if not 0 <= idx < self.length:
            raise IndexError(idx)
        g = torch.Generator().manual_seed(self.seed * 100003 + int(idx))
        # the octaves are summed on the finest one's 48 x 48 grid and upsampled once: a worker
        # makes an image in about the time it decodes a JPEG of that size
        low = torch.zeros(1, 3, 48, 48)
        for cells, amp in ((6, 1.0), (12, 0.6), (24, 0.35), (48, 0.2)):
            noise = torch.randn(1, 3, cells, cells, generator=g)
            low += amp * torch.nn.functional.interpolate(noise, size=(48, 48), mode="bicubic", align_corners=True)
        low = low / low.std() * 60.0 + 128.0
        out = torch.nn.functional.interpolate(low, size=(self.h, self.w), mode="bilinear", align_corners=True)[0]
        image = out.clamp(0, 255).round().to(torch.uint8)
        return {"image": image.permute(1, 2, 0).contiguous()}


def collate_uint8_images(samples):
    """Batch of single-image samples (runs in the DataLoader workers): the
    decoded HWC uint8 pixels of the B images packed into ONE byte buffer
    ``pixels`` with ``pixel_meta`` [B, 3] = (byte offset, H, W)."""
    imgs = [s["image"] for s in samples]
    sizes = [int(x.numel()) for x in imgs]
    offs = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.int64)
    meta = torch.tensor([[o, x.shape[0], x.shape[1]] for o, x in zip(offs, imgs)], dtype=torch.int64)
    return {"pixels": torch.cat([x.reshape(-1) for x in imgs]), "pixel_meta": meta}


VIEW_POINT_GRID = 25      # gpu_view_batch(with_points=True): the A-cell centres of a 25 x 25 grid


def gpu_view_batch(batch, device, out_h: int, out_w: int, augment, generator, with_points: bool = False):
    """Two random views of every image of a ``collate_uint8_images`` batch,
    with their dense ground-truth correspondence (``train.py --loss warp``).

    The meta rows are duplicated to [2B, 3] with the SAME byte offsets (view A
    of image b is row b, view B row B + b; the pixels are not copied),
    ``draw_params`` draws one row per view (its per-pair flip applies to both
    views of an image, which keeps the correspondence a plain affine map), the
    bytes are uploaded once and ONE ``warp_norm_u8`` launch cuts, resizes,
    jitters and normalises all 2B views (on CPU tensors: the fp32 torch form
    of the same definition).  The launch takes the rows interleaved (A0, B0,
    A1, B1, ...): the kernel's contract, asserted by its bounds-checked build,
    is a table of non-decreasing byte offsets; the two images returned are
    therefore strided views of one [B, 2, 3, out_h, out_w] buffer.  Returns ``source_image`` (view A), ``target_image``
    (view B) [B, 3, out_h, out_w] and ``warp_maps`` [B, 2, 12] fp64
    (``data.augment.view_maps``) on ``device``.

    ``with_points``: also ``source_points`` / ``target_points`` [B, 2, 625] --
    the A-cell centres of a 25 x 25 grid and their images in view B, (x, y) in
    1-based pixels, ``-1`` where the cell is not valid (``dense_targets``) --
    ``source_im_size`` / ``target_im_size`` = (out_h, out_w, 3) and ``L_pck`` =
    max(out_h, out_w): the fields ``engine.trainer.batch_pck`` scores."""
    from .augment import draw_params, view_maps
    from .transforms import IMAGENET_MEAN, IMAGENET_STD
    from ..ops import _ext
    if augment is None:
        raise ValueError("gpu_view_batch needs a PairAugment: the two views differ only by their random maps")
    pix, meta = batch["pixels"], batch["pixel_meta"]
    b = meta.shape[0]
    ends = meta[:, 0] + meta[:, 1] * meta[:, 2] * 3
    if b < 1 or int(ends.max()) > pix.numel() or int(meta[:, 1:].min()) < 1 or int(meta[:, 0].min()) < 0:
        raise ValueError("malformed pixel table")
    meta2 = torch.cat((meta, meta), 0)
    params = draw_params(meta2, out_h, out_w, augment, generator)
    maps = view_maps(params, meta2, out_h, out_w)
    dev = torch.device(device)
    res = {"warp_maps": maps.to(dev, non_blocking=True)}
    if with_points:
        from ..ops.reference import dense_targets
        g = VIEW_POINT_GRID
        _, _, ok, _, _, _ = dense_targets(maps, g, g, g, g)
        i, j = torch.meshgrid(torch.arange(g, dtype=torch.float64), torch.arange(g, dtype=torch.float64),
                              indexing="ij")
        ux, uy = (j / (g - 1)).reshape(1, -1), (i / (g - 1)).reshape(1, -1)
        m = maps[:, 0]
        qx = m[:, 0:1] * ux + m[:, 1:2] * uy + m[:, 2:3]
        qy = m[:, 3:4] * ux + m[:, 4:5] * uy + m[:, 5:6]
        ext = torch.tensor([out_w - 1.0, out_h - 1.0], dtype=torch.float64).view(1, 2, 1)
        sp = torch.stack((ux.expand(b, -1), uy.expand(b, -1)), 1) * ext + 1.0
        tp = torch.stack((qx, qy), 1) * ext + 1.0
        keep = ok.unsqueeze(1)
        size = torch.tensor([float(out_h), float(out_w), 3.0]).expand(b, 3).contiguous()
        pts = {"source_points": torch.where(keep, sp, torch.full_like(sp, -1.0)).float(),
               "target_points": torch.where(keep, tp, torch.full_like(tp, -1.0)).float(),
               "source_im_size": size, "target_im_size": size.clone(),
               "L_pck": torch.full((b, 1), float(max(out_h, out_w)))}
        res.update({k: v.to(dev, non_blocking=True) for k, v in pts.items()})
    order = torch.arange(2 * b).view(2, b).t().reshape(-1)                    # A0, B0, A1, B1, ...
    meta_k, params_k = meta2[order].contiguous(), params[order].contiguous()
    pix_d = pix.to(dev, non_blocking=True) if dev.type == "cuda" else None   # the batch's ONE pixel copy
    if pix_d is not None and _ext.use_hip(pix_d):
        out = torch.empty((2 * b, 3, out_h, out_w), dtype=torch.float32, device=dev)
        _ext.ext().warp_norm_u8(pix_d, meta_k.to(dev, non_blocking=True), params_k.to(dev, non_blocking=True), out,
                                list(IMAGENET_MEAN), list(IMAGENET_STD))
    else:
        from ..ops.reference import warp_norm_u8
        out = warp_norm_u8(pix, meta_k, params_k, out_h, out_w, IMAGENET_MEAN, IMAGENET_STD,
                           dtype=torch.float32).to(dev)
    out = out.view(b, 2, 3, out_h, out_w)
    res["source_image"], res["target_image"] = out[:, 0], out[:, 1]
    return res


class PFPascalDataset(Dataset):
    """PF-Pascal keypoint pairs (lib/pf_dataset.py:11-112)."""

    def __init__(self, csv_file, dataset_path, output_size=(240, 240), transform=None, category=None,
                 pck_procedure="pf", gpu_resize=False):
        """``gpu_resize``: return the decoded images as HWC uint8 tensors of
        their own size and skip ``transform`` (collate with
        ``collate_uint8_pairs``, resize + normalise with ``gpu_pair_batch``);
        points, sizes and ``L_pck`` are the same either way."""
        if gpu_resize and pck_procedure == "scnet":
            raise ValueError("pck_procedure='scnet' rescales the keypoints into a 224 x 224 frame that is not the "
                             "pixel frame of the decoded image; it cannot be combined with gpu_resize")
        self.gpu_resize = gpu_resize
        self.category_names = PF_CATEGORIES
        self.out_h, self.out_w = output_size
        pairs = pd.read_csv(csv_file)
        self.category = pairs.iloc[:, 2].to_numpy().astype("float")
        if category is not None:
            keep = np.nonzero(self.category == category)[0]
            self.category = self.category[keep]
            pairs = pairs.iloc[keep, :]
        self.pairs = pairs
        self.img_A_names = pairs.iloc[:, 0].tolist()
        self.img_B_names = pairs.iloc[:, 1].tolist()
        self.point_A_coords = pairs.iloc[:, 3:5]
        self.point_B_coords = pairs.iloc[:, 5:]
        self.dataset_path = dataset_path
        self.transform = transform
        self.pck_procedure = pck_procedure

    def __len__(self):
        return len(self.pairs)

    def get_image(self, name):
        image = read_image(os.path.join(self.dataset_path, name))
        im_size = torch.tensor(image.shape, dtype=torch.float32)
        if self.gpu_resize:          # HWC uint8 as decoded; packed per batch by collate_uint8_pairs
            return torch.from_numpy(np.ascontiguousarray(image)), im_size
        return resize_bilinear(to_chw_float(image), self.out_h, self.out_w), im_size

    @staticmethod
    def parse_points(xs: str, ys: str, n: int = 20) -> torch.Tensor:
        x = np.array([float(v) for v in str(xs).split(";") if v != ""])
        y = np.array([float(v) for v in str(ys).split(";") if v != ""])
        out = -np.ones((2, n))
        out[0, : len(x)] = x
        out[1, : len(x)] = y
        return torch.tensor(out, dtype=torch.float32)

    def __getitem__(self, idx):
        image_a, size_a = self.get_image(self.img_A_names[idx])
        image_b, size_b = self.get_image(self.img_B_names[idx])
        pa = self.parse_points(self.point_A_coords.iloc[idx, 0], self.point_A_coords.iloc[idx, 1])
        pb = self.parse_points(self.point_B_coords.iloc[idx, 0], self.point_B_coords.iloc[idx, 1])
        n_pts = int(torch.sum(pa[0] != -1))
        if self.pck_procedure == "pf":
            l_pck = torch.tensor([float(torch.max(pa[:, :n_pts].max(1)[0] - pa[:, :n_pts].min(1)[0]))])
        elif self.pck_procedure == "scnet":
            pa[0, :n_pts] *= 224 / size_a[1]
            pa[1, :n_pts] *= 224 / size_a[0]
            pb[0, :n_pts] *= 224 / size_b[1]
            pb[1, :n_pts] *= 224 / size_b[0]
            size_a[0:2] = torch.tensor([224.0, 224.0])
            size_b[0:2] = torch.tensor([224.0, 224.0])
            l_pck = torch.tensor([224.0])
        else:
            raise ValueError(self.pck_procedure)
        sample = {"source_image": image_a, "target_image": image_b, "source_im_size": size_a,
                  "target_im_size": size_b, "source_points": pa, "target_points": pb, "L_pck": l_pck}
        if self.transform and not self.gpu_resize:
            sample = self.transform(sample)
        return sample


class SyntheticPairDataset(Dataset):
    """Random normalised image pairs of a fixed size (benchmarks, smoke tests)."""

    def __init__(self, length: int = 64, image_size=(400, 400), seed: int = 0):
        self.length = length
        self.h, self.w = image_size
        self.seed = seed

    def __len__(self):
        return self.length

    def __getitem__(self, idx):
        g = torch.Generator().manual_seed(self.seed * 100003 + idx)
        a = torch.randn(3, self.h, self.w, generator=g)
        b = torch.randn(3, self.h, self.w, generator=g)
        size = torch.tensor([self.h, self.w, 3], dtype=torch.float32)
        return {"source_image": a, "target_image": b, "source_im_size": size, "target_im_size": size, "set": 0}


class SyntheticCorrespondenceDataset(Dataset):
    """Synthetic pairs WITH keypoints (``train.py --loss strong --synthetic N``):
    item ``i`` is ``synthetic_correspondence_batch(1, size, seed=seed * 100003 + i)``
    without its batch axis, so it is deterministic per index.  Fields as
    ``PFPascalDataset``: images [3, size, size], ``source_points`` /
    ``target_points`` [2, n_points] (-1 padded), ``*_im_size`` [3], ``L_pck`` [1]."""

    def __init__(self, length: int = 64, size: int = 400, seed: int = 0, n_points: int = 20):
        self.length = length
        self.size = int(size)
        self.seed = seed
        self.n_points = n_points

    def __len__(self):
        return self.length

    def __getitem__(self, idx):
        if not 0 <= idx < self.length:
            raise IndexError(idx)
        b = synthetic_correspondence_batch(1, self.size, seed=self.seed * 100003 + int(idx), n_points=self.n_points)
        return {k: v[0].contiguous() for k, v in b.items()}


def synthetic_batch(batch: int, image_size=(400, 400), device="cpu", seed: int = 0):
    """One batch of random normalised pairs generated directly on ``device``."""
    g = torch.Generator(device=device).manual_seed(seed)
    h, w = image_size
    src = torch.randn(batch, 3, h, w, generator=g, device=device)
    tgt = torch.randn(batch, 3, h, w, generator=g, device=device)
    return {"source_image": src, "target_image": tgt}


def _smooth_texture(n: int, size: int, g: torch.Generator, device) -> torch.Tensor:
    """[n, 3, size, size] smooth random colour textures (sum of upsampled noise
    octaves), roughly ImageNet-normalised."""
    out = torch.zeros(n, 3, size, size, device=device)
    for cells, amp in ((6, 1.0), (12, 0.6), (24, 0.35), (48, 0.2)):
        noise = torch.randn(n, 3, cells, cells, generator=g, device=device)
        out += amp * torch.nn.functional.interpolate(noise, size=(size, size), mode="bicubic", align_corners=True)
    return out / out.flatten(1).std(1).view(n, 1, 1, 1)


def synthetic_correspondence_batch(batch: int, size: int, device="cpu", seed: int = 0, n_points: int = 20,
                                   max_shift: float = 0.15, max_rot_deg: float = 10.0, scale_range=(0.9, 1.1)):
    """Image pairs with a KNOWN dense correspondence (training-quality checks).

    A smooth texture is drawn on a 1.5x canvas; the source is its centre crop and
    the target samples the canvas through a random similarity transform
    (rotation, scale, shift), so target pixel p_t shows source pixel
    p_s = A (p_t - c) + c + t.  Keypoints are drawn in the target where p_s
    lands inside the source (PF-Pascal layout: [b, 2, n_points], -1 padded;
    ``L_pck`` = image size).  Everything is generated on ``device``."""
    g = torch.Generator(device=device).manual_seed(seed)
    canvas = int(round(1.5 * size))
    tex = _smooth_texture(batch, canvas, g, device)
    off = (canvas - size) / 2.0
    src = tex[:, :, int(off):int(off) + size, int(off):int(off) + size]
    u = lambda *s: torch.rand(*s, generator=g, device=device)  # noqa: E731
    ang = (u(batch) * 2 - 1) * max_rot_deg * 3.141592653589793 / 180
    sc = scale_range[0] + u(batch) * (scale_range[1] - scale_range[0])
    sh = (u(batch, 2) * 2 - 1) * max_shift * size
    A = torch.stack([torch.stack([sc * torch.cos(ang), -sc * torch.sin(ang)], -1),
                     torch.stack([sc * torch.sin(ang), sc * torch.cos(ang)], -1)], 1)      # [b, 2, 2] on (x, y)
    c = (size - 1) / 2.0
    ys, xs = torch.meshgrid(torch.arange(size, device=device, dtype=torch.float32),
                            torch.arange(size, device=device, dtype=torch.float32), indexing="ij")
    pt = torch.stack((xs, ys), -1).view(1, -1, 2) - c                                    # target pixels, centred
    ps = torch.einsum("bij,bnj->bni", A, pt.expand(batch, -1, -1)) + c + sh.view(batch, 1, 2)
    grid = (ps + off) / (canvas - 1) * 2 - 1                                               # canvas coords (align_corners)
    tgt = torch.nn.functional.grid_sample(tex, grid.view(batch, size, size, 2), mode="bilinear",
                                          padding_mode="border", align_corners=True)
    # keypoints: target points whose source correspondence is inside the source image
    cand = u(batch, 4 * n_points, 2) * (size - 1)
    cs = torch.einsum("bij,bnj->bni", A, cand - c) + c + sh.view(batch, 1, 2)
    ok = ((cs >= 0) & (cs <= size - 1)).all(-1)
    tp = torch.full((batch, 2, n_points), -1.0, device=device)
    sp = torch.full((batch, 2, n_points), -1.0, device=device)
    for i in range(batch):
        idx = torch.nonzero(ok[i]).view(-1)[:n_points]
        tp[i, :, :idx.numel()] = cand[i, idx].t()
        sp[i, :, :idx.numel()] = cs[i, idx].t()
    sz = torch.tensor([float(size), float(size), 3.0], device=device).expand(batch, 3)
    return {"source_image": src.contiguous(), "target_image": tgt.contiguous(), "source_points": sp,
            "target_points": tp, "source_im_size": sz, "target_im_size": sz,
            "L_pck": torch.full((batch, 1), float(size), device=device)}
