#!/usr/bin/env python
"""SHA-256 fingerprints of seeded training steps, for comparing two commits.

A refactor of the route from features to volumes, or of the Trainer's loss
handling, must not change a number.  This script runs a matrix of small seeded
configurations on synthetic data and writes, per configuration, the SHA-256
digest of the loss, of every gradient and of every trained parameter to one
JSON file -- folded into one digest per configuration and mode, or with
``--per-tensor`` each on its own.  Run it on both commits and diff the files
(``--diff A B``).

Two modes per configuration:

* ``features``: seeded unit-norm features -> ``weak_loss_volumes_from_features``
  / ``match_volumes_from_features`` -> the loss -> backward.  No trunk runs, so
  this covers exactly the volume route and the loss.  With a "trainable trunk"
  the features require grad and their gradient is digested too.
* ``steps``: two ``Trainer.train_step`` calls and one ``eval_step`` on the whole
  model.  On a GPU the frozen trunk picks its 1x1-conv implementation per
  process by timing, so these digests may differ between two processes of ONE
  commit: record them, compare them only where the commit agrees with itself.

The matrix: loss in {weak, strong, warp} x relocalization_k_size in {0, 2} x
trunk {frozen, last block trainable} x nc_precision in {bf16, fp32} (fp32 with
a frozen trunk yields split (hi, lo) correlation operands), at 128 px on the
host and 240 px (k = 0) / 256 px (k = 2: an even grid) on a GPU.  A configuration
that raises (the unfused pool has no backward into a trainable trunk) records
the exception text instead of digests: that must not change either.

Where bit-equality is not expected (``index_add_`` in the plain correlation's
backward on a GPU) ``--save-tensors DIR`` keeps the tensors of the ``features``
mode and ``--maxdiff DIR_A DIR_B`` prints the largest absolute difference per
configuration, to set a branch-vs-parent difference against the difference
between two runs of the parent.

    python scripts/step_fingerprint.py --out fp.json [--device cuda] [--image_size 240]
    python scripts/step_fingerprint.py --diff parent.json branch.json
"""
from __future__ import annotations

import argparse
import hashlib
import itertools
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LOSSES = ("weak", "strong", "warp")
B = 2
CHANNELS = 1024          # ResNet-101 layer3, what extract() packs


def digest(t: torch.Tensor) -> str:
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def config_name(loss, k, trainable, prec) -> str:
    return f"{loss}/k{k}/{'trainable' if trainable else 'frozen'}/{prec}"


def build_model(k, trainable, prec, dev, nc):
    from ncnet_amd.models import ImMatchNet
    torch.manual_seed(0)
    model = ImMatchNet(use_cuda=dev.type == "cuda", ncons_kernel_sizes=nc[0], ncons_channels=nc[1],
                       relocalization_k_size=k, nc_precision=prec).to(dev)
    if trainable:                                  # train.py --fe_finetune_params 1
        for p in model.FeatureExtraction.model[-1][-1].parameters():
            p.requires_grad = True
    model.train()
    return model


def make_batch(loss, size, dev, seed):
    """A seeded synthetic batch of B pairs for ``loss``, built on the host."""
    from ncnet_amd.data.augment import PairAugment
    from ncnet_amd.data.datasets import (SyntheticImageDataset, collate_uint8_images, gpu_view_batch,
                                         synthetic_batch, synthetic_correspondence_batch)
    if loss == "weak":
        batch = synthetic_batch(B, (size, size), "cpu", seed=seed)
    elif loss == "strong":
        batch = synthetic_correspondence_batch(B, size, "cpu", seed=seed)
    else:
        ims = SyntheticImageDataset(B, (size + 20, size + 60), seed=seed)
        return gpu_view_batch(collate_uint8_images([ims[i] for i in range(B)]), dev, size, size, PairAugment(),
                              torch.Generator().manual_seed(seed), with_points=True)
    return {k: v.to(dev) for k, v in batch.items()}


def seeded_features(grid, dev, split, requires_grad, seed=11):
    """Unit-norm [2B, grid*grid, C] features as extract() would hand them on:
    (hi, lo) bf16 when ``split``, else bf16 on a GPU / fp32 on the host."""
    g = torch.Generator().manual_seed(seed)
    y = torch.nn.functional.normalize(torch.randn(2 * B, grid * grid, CHANNELS, generator=g), dim=2).to(dev)
    if split:
        hi = y.to(torch.bfloat16)
        return hi, (y - hi.float()).to(torch.bfloat16)
    f = y.to(torch.bfloat16) if dev.type == "cuda" else y
    return f.requires_grad_(True) if requires_grad else f


def loss_from_features(model, f, hw, batch, loss):
    from ncnet_amd.ops.loss import strong_loss_from_corr, warp_loss_from_corr, weak_loss_from_corr
    if loss == "weak":
        return weak_loss_from_corr(model.weak_loss_volumes_from_features(f, hw, B), B, "softmax")
    vol = model.match_volumes_from_features(f, hw, B)
    return (strong_loss_from_corr if loss == "strong" else warp_loss_from_corr)(vol, batch)


def named_trained(model):
    return [(n, p) for n, p in model.named_parameters() if p.requires_grad]


def run_features(cfg, dev, size, nc, keep):
    loss_name, k, trainable, prec = cfg
    model = build_model(k, trainable, prec, dev, nc)
    grid = size // 16
    split = prec == "fp32" and not trainable
    f = seeded_features(grid, dev, split, trainable)
    batch = make_batch(loss_name, size, dev, seed=21)
    loss = loss_from_features(model, f, (grid, grid), batch, loss_name)
    loss.backward()
    tensors = {"loss": loss.detach()}
    for n, p in model.NeighConsensus.named_parameters():
        tensors["grad/NeighConsensus." + n] = p.grad
    if trainable:
        tensors["grad/features"] = f.grad
    if keep is not None:
        keep.update({k_: v.detach().float().cpu() for k_, v in tensors.items()})
    return {k_: digest(v) for k_, v in tensors.items()}


def run_steps(cfg, dev, size, nc):
    from ncnet_amd.engine.trainer import Trainer, make_adam
    from ncnet_amd.parallel.dist import DistContext
    loss_name, k, trainable, prec = cfg
    model = build_model(k, trainable, prec, dev, nc)
    ctx = DistContext(device=torch.device(dev.type, 0) if dev.type == "cuda" else dev)
    trained = named_trained(model)                 # before a step: the trunk registers its folded copy later
    tr = Trainer(model, make_adam([p for _, p in trained], 1e-3), ctx, loss=loss_name)
    batches = [make_batch(loss_name, size, dev, seed=31 + i) for i in range(2)]
    out = {}
    out["step0/loss"] = digest(tr.train_step(batches[0], batches[1]))
    out["step1/loss"] = digest(tr.train_step(batches[1]))
    for n, p in trained:
        if p.grad is not None:
            out["step1/grad/" + n] = digest(p.grad)
        out["step1/param/" + n] = digest(p)
    model.eval()
    out["eval/loss"] = digest(tr.eval_step(batches[0]))
    if tr._pck:
        out["eval/pck"] = digest(tr._pck[-1])
    return out


def fingerprint(args):
    from ncnet_amd.ops import _ext
    dev = torch.device(args.device)
    # 240 px is a 15 x 15 feature grid, which k = 2 does not divide: the pooled configurations of a
    # GPU run take the next size up, 256 px (16 x 16 -> 8 x 8: the fused pool, and its HIP backward)
    sizes = {0: args.image_size or (240 if dev.type == "cuda" else 128),
             2: args.image_size or (256 if dev.type == "cuda" else 128)}
    # the GPU runs the benchmark's NC stack (the compile-time fast kernels); the host a small one
    nc = ([5, 5, 5], [16, 16, 1]) if dev.type == "cuda" else ([3, 3], [16, 1])
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    result = {"device": dev.type, "image_size": {f"k{k}": v for k, v in sizes.items()}, "batch": B,
              "torch": torch.__version__, "configs": {}}
    for cfg in itertools.product(LOSSES, (0, 2), (False, True), ("bf16", "fp32")):
        name = config_name(*cfg)
        if args.only and args.only not in name:
            continue
        rec = {}
        size = sizes[cfg[1]]
        for mode in args.modes:
            n0 = dict(_ext.DISPATCH)
            keep = {} if (args.save_tensors and mode == "features") else None
            try:
                rec[mode] = run_features(cfg, dev, size, nc, keep) if mode == "features" else \
                    run_steps(cfg, dev, size, nc)
            except (ValueError, RuntimeError, NotImplementedError) as e:
                rec[mode] = {"error": f"{type(e).__name__}: {e}"}
            if dev.type == "cuda":
                torch.cuda.synchronize()
            rec[mode + "_dispatch"] = {k: v - n0.get(k, 0) for k, v in sorted(_ext.DISPATCH.items())
                                       if v != n0.get(k, 0)}
            if keep:
                os.makedirs(args.save_tensors, exist_ok=True)
                torch.save(keep, os.path.join(args.save_tensors, name.replace("/", "_") + ".pt"))
        print(name, {m: ("error" if "error" in rec[m] else f"{len(rec[m])} digests") for m in args.modes}, flush=True)
        result["configs"][name] = rec if args.per_tensor else compact(rec)
    write_json(result, args.out)


def compact(rec: dict) -> dict:
    """One digest per mode: the SHA-256 of the mode's sorted (tensor name, digest)
    pairs and their count; errors and dispatch counters are kept as they are."""
    out = {}
    for key, val in rec.items():
        if key.endswith("_dispatch") or "error" in val or "sha256" in val:
            out[key] = val
        else:
            out[key] = {"sha256": hashlib.sha256(json.dumps(sorted(val.items())).encode()).hexdigest(),
                        "tensors": len(val)}
    return out


def write_json(result: dict, path: str) -> None:
    """The header, then one line per configuration (files meant to be diffed and committed)."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    head = {k: v for k, v in result.items() if k != "configs"}
    lines = [f' {json.dumps(n)}: {json.dumps(r, sort_keys=True)}' for n, r in sorted(result["configs"].items())]
    with open(path, "w") as fh:
        fh.write("{" + json.dumps(head, sort_keys=True)[1:-1] + ',\n"configs": {\n' + ",\n".join(lines) + "\n}}\n")


def compact_file(src: str, dst: str) -> None:
    with open(src) as fh:
        result = json.load(fh)
    result["configs"] = {n: compact(r) for n, r in result["configs"].items()}
    write_json(result, dst)


def diff(a_path, b_path) -> int:
    with open(a_path) as fa, open(b_path) as fb:
        a, b = json.load(fa)["configs"], json.load(fb)["configs"]
    bad = 0
    for name in sorted(set(a) | set(b)):
        for mode in sorted(set(a.get(name, {})) | set(b.get(name, {}))):
            ra, rb = a.get(name, {}).get(mode), b.get(name, {}).get(mode)
            if ra == rb:
                print(f"same    {name} {mode}")
                continue
            bad += 1
            keys = [k for k in sorted(set(ra or {}) | set(rb or {})) if (ra or {}).get(k) != (rb or {}).get(k)]
            print(f"DIFFERS {name} {mode}: {keys}")
    print(f"{bad} differing records")
    return bad


def maxdiff(dir_a, dir_b):
    for fn in sorted(os.listdir(dir_a)):
        if not fn.endswith(".pt") or not os.path.exists(os.path.join(dir_b, fn)):
            continue
        ta, tb = torch.load(os.path.join(dir_a, fn)), torch.load(os.path.join(dir_b, fn))
        worst = {k: float((ta[k].double() - tb[k].double()).abs().max()) for k in ta if k in tb}
        scale = {k: float(ta[k].double().abs().max()) for k in worst}
        k = max(worst, key=lambda k_: worst[k_] / (scale[k_] or 1.0))
        print(f"{fn[:-3]}: max |a - b| = {max(worst.values()):.3e}; largest relative to the tensor's max: "
              f"{k} {worst[k]:.3e} / {scale[k]:.3e}", flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="step_fingerprint.json")
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--image_size", type=int, default=0, help="default: 240 (k = 0) / 256 (k = 2) on a GPU, 128 on the host")
    ap.add_argument("--modes", nargs="+", default=["features", "steps"], choices=["features", "steps"])
    ap.add_argument("--only", default="", help="run the configurations whose name contains this")
    ap.add_argument("--save-tensors", default="", metavar="DIR", help="keep the features mode's tensors (for --maxdiff)")
    ap.add_argument("--per-tensor", action="store_true",
                    help="write every tensor's digest instead of one digest per mode (to find which tensor moved)")
    ap.add_argument("--compact", nargs=2, metavar=("IN", "OUT"), help="reduce a --per-tensor file to the default form")
    ap.add_argument("--diff", nargs=2, metavar=("A", "B"))
    ap.add_argument("--maxdiff", nargs=2, metavar=("DIR_A", "DIR_B"))
    args = ap.parse_args(argv)
    if args.diff:
        return 1 if diff(*args.diff) else 0
    if args.maxdiff:
        return maxdiff(*args.maxdiff)
    if args.compact:
        return compact_file(*args.compact)
    return fingerprint(args)


if __name__ == "__main__":
    sys.exit(main())
