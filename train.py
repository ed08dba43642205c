#!/usr/bin/env python
"""Weakly-supervised NC-Net training (reference CLI: train.py:34-47).

Same flags and defaults as the reference, plus:
  --synthetic N        train on N random pairs instead of a CSV dataset
  --num_workers W      data-loader workers per rank (reference: 0 train / 4 test)
  --log_interval L     loss print interval (reference: 1); the values are read
                       back asynchronously (no per-step host sync)
  --sync_log           synchronous per-step loss readback, as the reference
  --resume PATH        real resume: weights + optimizer + epoch + RNG state
  --max_steps S        stop after S training steps (smoke / profiling)
  --loss weak|strong   weak (default): the reference's objective.  strong: the
                       keypoint-supervised cross-entropy (ops/reference.py
                       keypoint_ce) on pairs with annotated correspondences:
                       --synthetic N (synthetic pairs with known keypoints) or
                       --train_pairs_csv / --val_pairs_csv (test_pairs.csv
                       layout); every validation epoch also reports PCK@0.1
  --loss warp          warp-supervised training from plain images, no annotation:
                       every image gives two random views (--aug_* set the
                       ranges) whose dense correspondence is a closed-form affine
                       map; the loss is the dense cross-entropy of
                       ops/reference.py dense_ce (csrc/densece.hip).  Images: the
                       distinct names of train_pairs.csv / val_pairs.csv under
                       --dataset_csv_path, or --image_dir DIR, or --synthetic N.
                       Implies the uint8 input path; validation draws the same
                       views every epoch and reports PCK@0.1 of a 25 x 25 grid
  --image_dir DIR      --loss warp: all .jpg / .jpeg / .png under DIR, sorted; the
                       last tenth (at least one image) is the validation set
  --gpu_input          --loss strong with --train_pairs_csv / --val_pairs_csv:
                       the workers only decode; one uint8 copy and one HIP
                       launch resize + normalise the batch on the GPU (what
                       the weak path does by default on a GPU; with the weak
                       loss the flag only matters on a CPU device, where it
                       selects the same uint8 route through torch)
  --augment            random rotation / zoom / shift / flip / contrast /
                       brightness of the training batches in that same launch
                       (--aug_* set the ranges); keypoints move with the pixels
  --metrics PATH       JSONL metrics (rank 0)
  --dtype bf16|fp32    backbone compute dtype of the default (bf16) NC mode
  --nc_precision bf16|mixed|fp32
                       bf16 (default, the headline benchmark): bf16 MFMA operands,
                       fp32 accumulation.  fp32: fp32-accurate training -- fp32
                       trunk, bf16x3 correlation and a bf16x3 NeighConsensus
                       forward AND backward on the fused kernels (~16 mantissa
                       bits per operand).  mixed: the stages the per-stage
                       ablation found necessary (profiles/r5/ablation): the
                       fp32-accurate trunk and NeighConsensus forward, a bf16
                       correlation and bf16 NeighConsensus backward (fp32-class
                       forward numerics at 2/3 of the fp32 mode's NC work).

Which precision to train with: bf16 unless you need fp32-class numerics.  A
per-stage ablation over 24 seeds in the hardest offline regime (random-init
trunk, per-step loss ~1e-8; profiles/r5/ablation/README.md) found the run
either takes off (PCK ~0.7) or its ReLUs die, at rates within noise of each
other for bf16 (10/24), mixed (12/24) and fp32 (13/24): the earlier few-seed
finding that only fp32 learns there did not hold.  mixed / fp32 keep the
reference's fp32 forward numerics (parity studies, checkpoints compared
bit-closely against fp32 training) at 2.2x / 2.9x the bf16 step time.
"""
from __future__ import annotations

import argparse
import datetime
import os
import sys
import time

# RCCL under torchrun: the ROCm driver only supports dmabuf IPC; must be set
# before any HIP initialisation (bench.py does the same).
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.utils.data import DataLoader, Subset

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ncnet_amd.data import (ImagePairDataset, NormalizeImageDict, PFPascalDataset, SingleImageDataset,  # noqa: E402
                            SyntheticCorrespondenceDataset, SyntheticImageDataset, SyntheticPairDataset)
from ncnet_amd.data.augment import PairAugment  # noqa: E402
from ncnet_amd.data.datasets import (collate_uint8_images, collate_uint8_pairs, gpu_pair_batch,  # noqa: E402
                                     gpu_view_batch)
from ncnet_amd.engine.checkpoint import capture_rng, load_checkpoint, restore_rng, save_checkpoint  # noqa: E402
from ncnet_amd.engine.trainer import AsyncLossLog, Trainer, make_adam  # noqa: E402
from ncnet_amd.models import ImMatchNet  # noqa: E402
from ncnet_amd.parallel.dist import barrier, broadcast_module, destroy, init_distributed, shard_indices  # noqa: E402
from ncnet_amd.utils.timing import SegmentTimer, set_active  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser(description="NC-Net training (MI355X)")
    p.add_argument("--checkpoint", type=str, default="")
    p.add_argument("--image_size", type=int, default=400)
    p.add_argument("--dataset_image_path", type=str, default="datasets/pf-pascal/", help="path to PF Pascal dataset")
    p.add_argument("--dataset_csv_path", type=str, default="datasets/pf-pascal/image_pairs/",
                   help="path to PF Pascal training csv")
    p.add_argument("--num_epochs", type=int, default=5, help="number of training epochs")
    p.add_argument("--batch_size", type=int, default=16, help="training batch size (per GPU)")
    p.add_argument("--lr", type=float, default=0.0005, help="learning rate")
    p.add_argument("--ncons_kernel_sizes", nargs="+", type=int, default=[5, 5, 5], help="kernels sizes in neigh. cons.")
    p.add_argument("--ncons_channels", nargs="+", type=int, default=[16, 16, 1], help="channels in neigh. cons")
    p.add_argument("--result_model_fn", type=str, default="checkpoint_adam", help="trained model filename")
    p.add_argument("--result-model-dir", type=str, default="trained_models", help="path to trained models folder")
    p.add_argument("--fe_finetune_params", type=int, default=0, help="number of layers to finetune")
    # extensions
    p.add_argument("--relocalization_k_size", type=int, default=0, metavar="K",
                   help="max-pool the correlation k x k x k x k before NeighConsensus; with --image_size 800 and K = 2 "
                        "the NC stack runs at the 400 px shape")
    p.add_argument("--synthetic", type=int, default=0)
    p.add_argument("--num_workers", type=int, default=-1,
                   help="DataLoader decode workers per rank (-1: min(8, cpus per rank) on GPU, 0 on CPU)")
    p.add_argument("--cpu_resize", action="store_true",
                   help="resize/normalise in the workers (reference behaviour) instead of on the GPU")
    p.add_argument("--log_interval", type=int, default=1)
    p.add_argument("--sync_log", action="store_true",
                   help="read every logged loss back synchronously (the reference's float(loss) per step); "
                        "default: asynchronous pinned-memory readback, printed when ready")
    p.add_argument("--resume", type=str, default="")
    p.add_argument("--max_steps", type=int, default=0)
    p.add_argument("--metrics", type=str, default="")
    p.add_argument("--dtype", type=str, default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--nc_precision", type=str, default="bf16", choices=["bf16", "mixed", "fp32"],
                   help="fp32: fp32-accurate training (fp32 trunk, bf16x3 correlation + NeighConsensus fwd/bwd on "
                        "the fused kernels); mixed: fp32-accurate trunk + NeighConsensus forward, bf16 correlation "
                        "and backward (fp32-class forward numerics at ~1/3 less NC cost than fp32). Over 24 seeds "
                        "bf16, mixed and fp32 took off at the same rate (profiles/r5/ablation): there is no evidence "
                        "that either learns where bf16 does not; pick them for forward numerics, not for learning")
    p.add_argument("--loss", type=str, default="weak", choices=["weak", "strong", "warp"],
                   help="weak: the reference's weakly-supervised score; strong: keypoint-supervised cross-entropy "
                        "on pairs with annotated correspondences (--synthetic N, or --train_pairs_csv / "
                        "--val_pairs_csv in the test_pairs.csv layout); warp: dense cross-entropy on two random views "
                        "of every image (the images of train_pairs.csv / val_pairs.csv, --image_dir DIR or "
                        "--synthetic N; the --aug_* flags set the view ranges)")
    p.add_argument("--image_dir", type=str, default="",
                   help="--loss warp: train on all .jpg / .jpeg / .png under DIR (sorted; the last tenth, at least "
                        "one image, is the validation set)")
    p.add_argument("--train_pairs_csv", type=str, default="",
                   help="--loss strong: training pairs with keypoints (source,target,class,XA,YA,XB,YB)")
    p.add_argument("--val_pairs_csv", type=str, default="", help="--loss strong: validation pairs with keypoints")
    p.add_argument("--gpu_input", action="store_true",
                   help="--loss strong on pair CSVs: decode in the workers, resize + normalise the packed uint8 batch "
                        "on the GPU; on a CPU device the same math runs through torch. The weak loss takes this route "
                        "by default on a GPU: there the flag changes nothing, and on a CPU device it selects the "
                        "uint8 route (torch) for the weak loss too")
    p.add_argument("--augment", action="store_true",
                   help="augment the training batches on the uint8 input path (implies --gpu_input): per-image random "
                        "rotation, zoom, shift, contrast and brightness and a per-pair horizontal flip, in the same "
                        "launch that resizes and normalises; keypoints are moved with the pixels, and a "
                        "correspondence with a point outside its frame is dropped (-1). Validation batches are not "
                        "augmented. The draws come from one generator per process seeded from (--seed, rank, first "
                        "epoch): ranks differ, and a resumed run does NOT replay the draws of the uninterrupted run")
    p.add_argument("--aug_rot_deg", type=float, default=15.0, help="rotation, uniform in +-DEG")
    p.add_argument("--aug_scale", type=float, nargs=2, default=[0.8, 1.25], metavar=("LO", "HI"),
                   help="zoom factor, log-uniform; below 1 zooms in")
    p.add_argument("--aug_shift", type=float, default=0.1, help="shift, uniform in +-F of the source extent")
    p.add_argument("--aug_flip", type=float, default=0.5, help="probability of a horizontal flip (per pair)")
    p.add_argument("--aug_gain", type=float, nargs=2, default=[0.8, 1.2], metavar=("LO", "HI"),
                   help="contrast about the ImageNet mean, log-uniform")
    p.add_argument("--aug_bias", type=float, default=0.2, help="brightness in normalised units, uniform in +-B")
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--segment_timing", action="store_true")
    p.add_argument("--profile", type=str, default="")
    return p


def warp_image_sets(args):
    """--loss warp: (image root, training names, validation names)."""
    if args.image_dir:
        names = sorted(os.path.relpath(os.path.join(d, f), args.image_dir)
                       for d, _, files in os.walk(args.image_dir) for f in files
                       if f.lower().endswith((".jpg", ".jpeg", ".png")))
        n_val = max(1, len(names) // 10)
        if len(names) < 2:
            raise SystemExit(f"--image_dir {args.image_dir}: found {len(names)} .jpg / .jpeg / .png images, need at "
                             "least 2 (one to train on, one to validate on)")
        return args.image_dir, names[:-n_val], names[-n_val:]
    import pandas as pd
    out = []
    for fn in ("train_pairs.csv", "val_pairs.csv"):
        data = pd.read_csv(os.path.join(args.dataset_csv_path, fn))
        out.append(sorted(set(data.iloc[:, 0].tolist()) | set(data.iloc[:, 1].tolist())))
    return args.dataset_image_path, out[0], out[1]


def augment_seed(seed: int, rank: int, first_epoch: int) -> int:
    """Seed of a process's augmentation generator: a mix of (--seed, rank, first
    epoch) reduced into the range torch.Generator.manual_seed takes, for any
    --seed.  Ranks of one run differ (their mixes differ by a multiple of
    1000003 below 2^63)."""
    return ((seed * 1000003 + rank) * 1000003 + first_epoch) % (1 << 63)


class _Shard(torch.utils.data.Sampler):
    """Per-rank, per-epoch reshuffled shard (DistributedSampler semantics)."""

    def __init__(self, n, ctx, shuffle=True, seed=1):
        self.n, self.ctx, self.shuffle, self.seed, self.epoch = n, ctx, shuffle, seed, 0

    def set_epoch(self, e):
        self.epoch = e

    def __iter__(self):
        return iter(shard_indices(self.n, self.ctx, self.epoch, self.shuffle, self.seed, drop_last=self.ctx.world_size > 1))

    def __len__(self):
        return self.n // self.ctx.world_size if self.ctx.world_size > 1 else self.n


def make_augment(args):
    """The PairAugment of --augment / --loss warp (the ranges of its two views), else None."""
    if not (args.augment or args.loss == "warp"):
        return None
    try:
        return PairAugment(rot_deg=args.aug_rot_deg, scale=tuple(args.aug_scale), shift=args.aug_shift,
                           flip=args.aug_flip, gain=tuple(args.aug_gain), bias=args.aug_bias)
    except ValueError as e:
        raise SystemExit(f"--{'augment' if args.augment else 'loss warp'}: {e}")


def validate_args(args):
    """Reject flag combinations before anything is built (SystemExit)."""
    strong = args.loss == "strong"
    warp = args.loss == "warp"
    if warp and args.cpu_resize:
        raise SystemExit("--loss warp cuts both views of an image from its decoded uint8 pixels on the device (the "
                         "uint8 input path); --cpu_resize, which resizes in the workers, cannot be combined with it")
    if args.image_dir and not warp:
        raise SystemExit("--image_dir is the image source of --loss warp")
    if strong and not args.synthetic and not (args.train_pairs_csv and args.val_pairs_csv):
        raise SystemExit("--loss strong needs pairs with keypoints: give --synthetic N, or --train_pairs_csv and "
                         "--val_pairs_csv (test_pairs.csv layout: source,target,class,XA,YA,XB,YB); "
                         "the shipped train_pairs.csv / val_pairs.csv carry no keypoints")
    for flag in ("augment", "gpu_input"):
        if getattr(args, flag) and ((args.synthetic and not warp) or args.cpu_resize):
            raise SystemExit(f"--{flag} works on the uint8 input path (decoded image files, resized on the device); "
                             f"--{'synthetic' if args.synthetic else 'cpu_resize'} batches carry float images")
    k_reloc = args.relocalization_k_size
    if k_reloc < 0:
        raise SystemExit("--relocalization_k_size must be >= 0")
    if k_reloc > 1:
        if args.image_size % (16 * k_reloc):
            raise SystemExit(f"--relocalization_k_size {k_reloc}: the feature grid (--image_size {args.image_size} / 16 "
                             f"= {args.image_size / 16:g} cells) must be a multiple of K")
        if args.fe_finetune_params > 0 and k_reloc != 2:
            raise SystemExit("--fe_finetune_params > 0 trains through the pooled correlation, whose backward exists "
                             "for --relocalization_k_size 2 (even feature grids) only")
    make_augment(args)


def build_data(args, ctx, model):
    """The per-loss data choices, made once: ``(train_loader, test_loader, tr_sampler, te_sampler,
    to_device, aug_rng, val_rng)`` -- the Trainer's ``batch_to_device`` hook and the generators of
    the training augmentation / --loss warp's validation views (None when unused; seeded by main())."""
    size = (args.image_size, args.image_size)
    n_test = max(2 * args.batch_size, args.synthetic // 8)
    augment = make_augment(args)
    aug_rng = torch.Generator() if augment is not None else None
    val_rng = None
    uint8_input = args.gpu_input or args.augment       # asked for: on any device (CPU: the torch fallback)
    if args.loss == "warp":
        if args.synthetic:
            train_set = SyntheticImageDataset(args.synthetic, size, seed=1)
            test_set = SyntheticImageDataset(n_test, size, seed=2)
        else:
            root, tr_names, va_names = warp_image_sets(args)
            train_set, test_set = SingleImageDataset(root, tr_names), SingleImageDataset(root, va_names)
        collate = collate_uint8_images
        val_rng = torch.Generator()      # re-seeded before every validation epoch: same views each time
        # validation batches also carry the 25 x 25 grid points, for PCK@0.1 of the same volume
        to_device = lambda batch: gpu_view_batch(  # noqa: E731
            batch, ctx.device, size[0], size[1], augment, aug_rng if model.training else val_rng,
            with_points=not model.training)
    else:
        strong = args.loss == "strong"
        # keypoint datasets yield float images unless the uint8 path is asked for
        gpu_resize = uint8_input or (not strong and ctx.device.type == "cuda" and not args.cpu_resize)
        if args.synthetic and strong:
            train_set = SyntheticCorrespondenceDataset(args.synthetic, args.image_size, seed=1)
            test_set = SyntheticCorrespondenceDataset(n_test, args.image_size, seed=2)
        elif args.synthetic:
            train_set = SyntheticPairDataset(args.synthetic, size, seed=1)
            test_set = SyntheticPairDataset(n_test, size, seed=2)
        else:
            kw = dict(output_size=size, transform=NormalizeImageDict(["source_image", "target_image"]),
                      gpu_resize=gpu_resize)
            if strong:
                train_set = PFPascalDataset(args.train_pairs_csv, args.dataset_image_path, **kw)
                test_set = PFPascalDataset(args.val_pairs_csv, args.dataset_image_path, **kw)
            else:
                train_set = ImagePairDataset(args.dataset_csv_path, "train_pairs.csv", args.dataset_image_path, **kw)
                test_set = ImagePairDataset(args.dataset_csv_path, "val_pairs.csv", args.dataset_image_path, **kw)
        collate = to_device = None
        if gpu_resize and not args.synthetic:
            collate = collate_uint8_pairs
            # training batches only (the Trainer sets model.training before it touches a loader): validation
            # keeps the plain resize and its points, so its loss and PCK compare with an un-augmented run
            to_device = lambda batch: gpu_pair_batch(  # noqa: E731
                batch, ctx.device, size[0], size[1], augment=augment if model.training else None, generator=aug_rng)
    tr_sampler = _Shard(len(train_set), ctx, True, args.seed)
    te_sampler = _Shard(len(test_set), ctx, True, args.seed + 7)
    pin = ctx.device.type == "cuda"
    nw = args.num_workers
    if nw < 0:
        nw = min(8, max(1, (os.cpu_count() or 2) // max(1, ctx.world_size) - 1)) if pin else 0
    lkw = dict(batch_size=args.batch_size, num_workers=nw, pin_memory=pin, drop_last=True, collate_fn=collate,
               persistent_workers=nw > 0, prefetch_factor=4 if nw > 0 else None)
    train_loader = DataLoader(train_set, sampler=tr_sampler, **lkw)
    test_loader = DataLoader(test_set, sampler=te_sampler, **lkw)
    return train_loader, test_loader, tr_sampler, te_sampler, to_device, aug_rng, val_rng


def run_max_steps(args, ctx, model, trainer, train_loader, timer):
    """The bounded --max_steps run (smoke / profiling): no validation, no checkpoint."""
    model.train()
    prof = None
    if args.profile and ctx.is_main:
        acts = [torch.profiler.ProfilerActivity.CPU]
        if ctx.device.type == "cuda":
            acts.append(torch.profiler.ProfilerActivity.CUDA)
        prof = torch.profiler.profile(activities=acts)
        prof.__enter__()
    t0 = time.perf_counter()
    t_warm, warm = None, min(10, max(0, args.max_steps - 1))
    steps = 0

    def batches():
        while True:
            for b in train_loader:
                yield b
    it = batches()
    steplog = AsyncLossLog(ctx.device, sync=args.sync_log)

    def show(recs):
        for r in recs:
            msg = f"step {r['step']} loss {r['loss']:.6f}"
            if "segments_ms" in r:
                msg += " " + " ".join(f"{k}={v:.2f}ms" for k, v in r["segments_ms"].items())
            print(msg, flush=True)
    nxt = trainer.to_device(next(it))
    while steps < args.max_steps:
        batch = nxt
        # one batch of lookahead, as Trainer.process_epoch: its backbone overlaps this step
        nxt = trainer.to_device(next(it)) if steps + 1 < args.max_steps else None
        loss = trainer.train_step(batch, nxt)
        steps += 1
        if steps == warm:
            if ctx.device.type == "cuda":
                torch.cuda.synchronize()
            t_warm = time.perf_counter()
        if ctx.is_main and (steps % max(1, args.log_interval) == 0):
            meta = {"step": steps}
            if timer is not None:
                meta["segments_ms"] = timer.collect()
            show(steplog.push(loss, meta))
        elif ctx.is_main:
            show(steplog.poll())
    if ctx.is_main:
        show(steplog.drain())
    if ctx.device.type == "cuda":
        torch.cuda.synchronize()
    if prof is not None:
        prof.__exit__(None, None, None)
        os.makedirs(args.profile, exist_ok=True)
        sort = "cuda_time_total" if ctx.device.type == "cuda" else "cpu_time_total"
        with open(os.path.join(args.profile, "train_profile.txt"), "w") as f:
            f.write(prof.key_averages().table(sort_by=sort, row_limit=60))
        prof.export_chrome_trace(os.path.join(args.profile, "train_trace.json"))
    if ctx.is_main:
        t1 = time.perf_counter()
        dt = t1 - t0
        msg = f"{steps} steps in {dt:.2f}s ({steps * args.batch_size * ctx.world_size / dt:.1f} pairs/s)"
        if t_warm is not None and steps > warm:
            # steady state: excludes DataLoader worker start-up and the first (graph-capturing) steps
            msg += (f"; steady state after {warm} steps: "
                    f"{(steps - warm) * args.batch_size * ctx.world_size / (t1 - t_warm):.1f} pairs/s")
        print(msg)


def main(argv=None):
    args = build_parser().parse_args(argv)
    validate_args(args)
    ctx = init_distributed()
    torch.manual_seed(args.seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(args.seed)
    np.random.seed(args.seed)
    if ctx.is_main:
        print("ImMatchNet training script (ncnet_amd)")
        print(args)

    # --resume rebuilds the NC architecture from the checkpoint's args, like --checkpoint
    model = ImMatchNet(use_cuda=ctx.device.type == "cuda", checkpoint=(args.resume or args.checkpoint) or None,
                       ncons_kernel_sizes=args.ncons_kernel_sizes, ncons_channels=args.ncons_channels,
                       dtype=args.dtype, nc_precision=args.nc_precision,
                       relocalization_k_size=args.relocalization_k_size).to(ctx.device)
    # the saved Namespace must describe the architecture actually built
    args.ncons_kernel_sizes = list(model.NeighConsensus.kernel_sizes)
    args.ncons_channels = list(model.NeighConsensus.channels)
    if args.fe_finetune_params > 0:  # train.py:60-63
        for i in range(args.fe_finetune_params):
            for p in model.FeatureExtraction.model[-1][-(i + 1)].parameters():
                p.requires_grad = True
    broadcast_module(model, ctx)
    params = [p for p in model.parameters() if p.requires_grad]
    if ctx.is_main:
        print("Trainable parameters:")
        for i, p in enumerate(params):
            print(f"{i + 1}: {tuple(p.shape)}")
    optimizer = make_adam(params, args.lr)

    train_loader, test_loader, tr_sampler, te_sampler, to_device, aug_rng, val_rng = build_data(args, ctx, model)

    checkpoint_name = os.path.join(args.result_model_dir,
                                   datetime.datetime.now().strftime("%Y-%m-%d_%H:%M") + "_" + args.result_model_fn +
                                   ".pth.tar")
    train_loss = np.zeros(args.num_epochs)
    test_loss = np.zeros(args.num_epochs)
    best_test_loss = float("inf")
    start_epoch = 1
    if args.resume:
        ck = load_checkpoint(args.resume)
        optimizer.load_state_dict(ck["optimizer"])
        start_epoch = int(ck["epoch"]) + 1
        best_test_loss = float(ck.get("best_test_loss", best_test_loss))
        n = min(len(train_loss), len(ck["train_loss"]))
        train_loss[:n] = ck["train_loss"][:n]
        test_loss[:n] = ck["test_loss"][:n]
        restore_rng(ck.get("rng"))
        checkpoint_name = args.resume
        if ctx.is_main:
            print(f"Resumed from {args.resume} at epoch {start_epoch}")
    if aug_rng is not None:
        aug_rng.manual_seed(augment_seed(args.seed, ctx.rank, start_epoch))
    if val_rng is not None:
        val_rng.manual_seed(augment_seed(args.seed + 7, ctx.rank, 0))
    if ctx.is_main:
        print("Checkpoint name: " + checkpoint_name)

    timer = SegmentTimer(device=ctx.device) if args.segment_timing else None
    set_active(timer)
    trainer = Trainer(model, optimizer, ctx, metrics_path=args.metrics or None, loss=args.loss)
    trainer.batch_to_device = to_device
    if args.max_steps:
        run_max_steps(args, ctx, model, trainer, train_loader, timer)
    else:
        run_epochs(args, ctx, model, optimizer, trainer, (train_loader, test_loader, tr_sampler), val_rng,
                   (start_epoch, train_loss, test_loss, best_test_loss, checkpoint_name))
    set_active(None)
    destroy(ctx)


def run_epochs(args, ctx, model, optimizer, trainer, data, val_rng, state):
    """Train, validate, checkpoint.  ``state``: (first epoch, loss histories, best loss, checkpoint name)."""
    train_loader, test_loader, tr_sampler = data
    start_epoch, train_loss, test_loss, best_test_loss, checkpoint_name = state
    if ctx.is_main:
        print("Starting training...")
    for epoch in range(start_epoch, args.num_epochs + 1):
        tr_sampler.set_epoch(epoch)
        train_loss[epoch - 1] = trainer.process_epoch("train", epoch, train_loader, args.log_interval, args.sync_log)
        if val_rng is not None:                        # the same validation views every epoch: loss and PCK compare
            val_rng.manual_seed(augment_seed(args.seed + 7, ctx.rank, 0))
        test_loss[epoch - 1] = trainer.process_epoch("test", epoch, test_loader, args.log_interval, args.sync_log)
        is_best = test_loss[epoch - 1] < best_test_loss
        best_test_loss = min(test_loss[epoch - 1], best_test_loss)
        if ctx.is_main:
            save_checkpoint({"epoch": epoch, "args": args, "state_dict": model.state_dict(),
                             "best_test_loss": best_test_loss, "optimizer": optimizer.state_dict(),
                             "train_loss": train_loss, "test_loss": test_loss, "rng": capture_rng()},
                            is_best, checkpoint_name)
        barrier(ctx)
    if ctx.is_main:
        print("Done!")


if __name__ == "__main__":
    main()
