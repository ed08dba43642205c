"""Host side of the augmenting input path (ncnet_amd/data/augment.py,
ops/reference.py::warp_norm_u8, PFPascalDataset(gpu_resize=True),
gpu_pair_batch(augment=...), train.py --gpu_input / --augment), on the CPU."""
import math
import os
import sys

import pytest
import torch

from ncnet_amd.data.augment import (PairAugment, draw_params, resize_params, transform_pair_points,
                                    transform_points)
from ncnet_amd.data.datasets import PFPascalDataset, collate_uint8_pairs, gpu_pair_batch
from ncnet_amd.data.transforms import IMAGENET_MEAN, IMAGENET_STD, NormalizeImageDict
from ncnet_amd.ops import reference as ref

from tests import augment_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def kp_files(tmp_path_factory):
    """Six tiny keypoint pairs from scripts/make_keypoint_pairs.py (5 train, 1 val)."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import make_keypoint_pairs
    finally:
        sys.path.pop(0)
    d = tmp_path_factory.mktemp("kp_pairs")
    make_keypoint_pairs.main(["--out", str(d), "--pairs", "6", "--min_side", "40", "--max_side", "64", "--seed", "3"])
    return d


def _forward(points, params):
    """1-based output-frame points -> 1-based source points through (A, t), fp64."""
    q = params.double()
    po = points.double() - 1
    x = q[:, 0, None] * po[:, 0] + q[:, 1, None] * po[:, 1] + q[:, 2, None]
    y = q[:, 3, None] * po[:, 0] + q[:, 4, None] * po[:, 1] + q[:, 5, None]
    return torch.stack((x, y), 1) + 1


def test_transform_points_roundtrip_padding_and_frames():
    g = torch.Generator().manual_seed(0)
    meta = torch.tensor([[0, 50, 70], [0, 61, 43], [0, 33, 90], [0, 48, 48]])
    oh, ow = 40, 56
    params = draw_params(meta, oh, ow, PairAugment(rot_deg=30, scale=(0.7, 1.4)), g)
    pts = torch.full((4, 2, 20), -1.0, dtype=torch.float64)
    n_real = 12
    for i, (_, h, w) in enumerate(meta.tolist()):
        pts[i, 0, :n_real] = 1 + torch.rand(n_real, generator=g, dtype=torch.float64) * (w - 1)
        pts[i, 1, :n_real] = 1 + torch.rand(n_real, generator=g, dtype=torch.float64) * (h - 1)
    new = transform_points(pts, params, oh, ow)
    assert new.dtype == pts.dtype and new.shape == pts.shape
    assert (new[:, :, n_real:] == -1).all()                         # padding stays padding
    valid = (new != -1).all(1)
    assert ((new == -1).all(1) | valid).all()                       # a column is a point or (-1, -1)
    assert 0 < int(valid.sum()) < 4 * n_real                        # the draws push some points out, not all
    back = _forward(new, params)
    assert float((back - pts).abs()[valid.unsqueeze(1).expand_as(pts)].max()) < 1e-6
    # valid <=> inside the output frame, judged independently by solving A p_o = p - 1 - t
    q = params.double()
    A = torch.stack((q[:, [0, 1]], q[:, [3, 4]]), 1)
    po = torch.linalg.solve(A, pts - 1 - q[:, [2, 5]].unsqueeze(2))
    inside = ((po >= 0) & (po <= torch.tensor([ow - 1.0, oh - 1.0]).view(1, 2, 1))).all(1)
    inside[:, n_real:] = False
    assert torch.equal(valid, inside)

    # a pair: index k is -1 in BOTH sets when either point left its frame, and nowhere else
    sp, tp = transform_pair_points(pts[:2], pts[2:], params, oh, ow)
    keep = valid[:2] & valid[2:]
    assert 0 < int(keep.sum()) < int(valid[:2].sum())
    for got, one in ((sp, new[:2]), (tp, new[2:])):
        assert torch.equal((got != -1).all(1), keep) and torch.equal((got == -1).all(1), ~keep)
        assert torch.equal(got[keep.unsqueeze(1).expand_as(got)], one[keep.unsqueeze(1).expand_as(one)])


@pytest.mark.parametrize("h,w", [(1, 30), (30, 1)])
def test_transform_points_degenerate_image_raises(h, w):
    meta = torch.tensor([[0, h, w], [0, 20, 20]])
    pts = torch.full((1, 2, 20), -1.0)
    for params in (resize_params(meta, 16, 16), draw_params(meta, 16, 16, PairAugment(), torch.Generator())):
        assert transform_points(pts, params[:1], 16, 16).eq(-1).all()       # no keypoints: fine
        with_kp = pts.clone()
        with_kp[0, :, 0] = 1.0
        with pytest.raises(ValueError, match="H < 2 or W < 2"):
            transform_points(with_kp, params[:1], 16, 16)


def test_transform_points_one_pixel_output_names_the_output():
    meta = torch.tensor([[0, 20, 30], [0, 20, 20]])
    pts = torch.full((1, 2, 20), -1.0)
    pts[0, :, 0] = 3.0
    with pytest.raises(ValueError, match="16 x 1"):
        transform_points(pts, resize_params(meta, 16, 1)[:1], 16, 1)


def test_plain_resize_keeps_normalised_points():
    """Keypoints pushed through resize_params and normalised with the NEW size
    equal the originals normalised with the OLD size: an un-augmented
    --gpu_input loss is today's loss."""
    from ncnet_amd.eval.point_tnf import normalize_axis
    g = torch.Generator().manual_seed(1)
    meta = torch.tensor([[0, 375, 500], [0, 500, 333], [0, 300, 300], [0, 2, 7]])
    for oh, ow in ((400, 400), (240, 320)):
        params = resize_params(meta, oh, ow)
        assert params.dtype == torch.float32 and params.shape == (4, 8)
        pts = torch.full((4, 2, 20), -1.0, dtype=torch.float64)
        for i, (_, h, w) in enumerate(meta.tolist()):
            pts[i, 0, :15] = 1 + torch.rand(15, generator=g, dtype=torch.float64) * (w - 1)
            pts[i, 1, :15] = 1 + torch.rand(15, generator=g, dtype=torch.float64) * (h - 1)
            pts[i, :, 0] = 1.0                                      # the corners stay in the frame
            pts[i, 0, 1], pts[i, 1, 1] = float(w), float(h)
        new = transform_points(pts, params, oh, ow)
        # fp32 rx may put the far corner 1e-5 px outside; every other point must survive
        assert (new[:, :, [0] + list(range(2, 15))] != -1).all()
        ok = (new != -1).all(1)
        for axis, (old_len, new_len) in enumerate(((meta[:, 2], ow), (meta[:, 1], oh))):
            want = normalize_axis(pts[:, axis], old_len.double().unsqueeze(1))
            got = normalize_axis(new[:, axis], float(new_len))
            assert float((got - want).abs()[ok].max()) < 1e-6


def test_resize_params_are_the_resize_kernel_ratios():
    meta = torch.tensor([[0, 17, 9], [5, 1, 6]])
    p = resize_params(meta, 24, 40)
    f = torch.float32
    assert torch.equal(p[:, 0], torch.tensor([8.0, 5.0], dtype=f) / torch.tensor(39.0, dtype=f))
    assert torch.equal(p[:, 4], torch.tensor([16.0, 0.0], dtype=f) / torch.tensor(23.0, dtype=f))
    assert torch.equal(p[:, [1, 2, 3, 5, 7]], torch.zeros(2, 5)) and torch.equal(p[:, 6], torch.ones(2))
    assert torch.equal(resize_params(meta, 1, 1)[:, [0, 4]], torch.zeros(2, 2))


def test_oracle_with_resize_params_is_the_resize():
    """The oracle is written out, not grid_sample / interpolate: with the
    plain-resize rows it must agree with today's CPU resize path."""
    g = torch.Generator().manual_seed(2)
    ims = [torch.randint(0, 256, s + (3,), generator=g, dtype=torch.uint8) for s in ((17, 9), (40, 33), (1, 6), (6, 1))]
    pix, meta = ac.pack(ims)
    got = ref.warp_norm_u8(pix, meta, resize_params(meta, 24, 40), 24, 40, IMAGENET_MEAN, IMAGENET_STD)
    assert got.dtype == torch.float64
    want = gpu_pair_batch({"pixels": pix, "pixel_meta": meta}, "cpu", 24, 40)
    want = torch.cat((want["source_image"], want["target_image"]))
    assert float((got - want).abs().max()) < 1e-4


def test_oracle_nan_and_far_parameters_stay_in_range():
    ims = [torch.full((3, 4, 3), 200, dtype=torch.uint8), torch.full((2, 2, 3), 10, dtype=torch.uint8)]
    pix, meta = ac.pack(ims)
    params = torch.tensor([[float("nan"), 0, 0, 0, float("inf"), -float("inf"), 1, 0],
                           [1e30, -1e30, 5e8, 0, 0, -7, 1, 0]])
    out = ref.warp_norm_u8(pix, meta, params, 5, 6, (0, 0, 0), (1, 1, 1))
    assert torch.isfinite(out).all()
    assert torch.allclose(out[0], torch.full_like(out[0], 200 / 255)) and torch.allclose(
        out[1], torch.full_like(out[1], 10 / 255))


def test_pixels_and_keypoints_move_together():
    """A blob at a keypoint, warped by the oracle, has its intensity centroid
    within 0.5 px of the transformed keypoint whenever that lies >= 6 px inside
    the output (the fp64 definition stays within 0.21 px over 2000 draws; a
    transposed or inverted matrix misses by pixels)."""
    cases = ac.blob_cases()
    errs = ac.blob_errors(cases, lambda p, m, q, oh, ow: ref.warp_norm_u8(p, m, q, oh, ow, IMAGENET_MEAN,
                                                                          IMAGENET_STD))
    checked = [e for e, inside in errs if inside >= 6]
    print(f"blob centroid error: max {max(checked):.3f} px over {len(checked)} keypoints")
    assert len(checked) >= 20
    assert max(checked) < 0.5
    flips = sum(1 for c in cases if c["params"][0, 0] * c["params"][0, 4] - c["params"][0, 1] * c["params"][0, 3] < 0)
    assert 0 < flips < len(cases)                                   # both orientations are exercised


def _stack(ds, idx):
    from torch.utils.data import default_collate
    return default_collate([ds[i] for i in idx])


def test_fast_path_matches_todays_path(kp_files):
    csv = os.path.join(kp_files, "image_pairs", "train_pairs.csv")
    size = (48, 56)
    old = PFPascalDataset(csv, str(kp_files), output_size=size,
                          transform=NormalizeImageDict(["source_image", "target_image"]))
    new = PFPascalDataset(csv, str(kp_files), output_size=size, gpu_resize=True,
                          transform=NormalizeImageDict(["source_image", "target_image"]))
    assert len(old) == len(new) == 5
    item = new[0]
    assert item["source_image"].dtype == torch.uint8 and item["source_image"].shape[2] == 3
    assert tuple(item["source_image"].shape) == tuple(int(v) for v in item["source_im_size"])
    n_pts = int((item["source_points"][0] != -1).sum())
    assert 8 <= n_pts <= 20
    want = _stack(old, range(5))
    got = gpu_pair_batch(collate_uint8_pairs([new[i] for i in range(5)]), "cpu", *size)
    for k in ("source_image", "target_image"):
        assert got[k].shape == want[k].shape == (5, 3) + size
        assert torch.allclose(got[k], want[k], atol=1e-4, rtol=0)
    for k in ("source_points", "target_points", "source_im_size", "target_im_size", "L_pck"):
        assert torch.equal(got[k], want[k]), k
    with pytest.raises(ValueError, match="scnet"):
        PFPascalDataset(csv, str(kp_files), pck_procedure="scnet", gpu_resize=True)


def test_generated_keypoints_follow_the_warp(kp_files):
    """make_keypoint_pairs.py: the target is a similarity warp of the source and
    the keypoints follow it -- the target patch at a keypoint looks like the
    source patch at its correspondence (and unlike a patch elsewhere)."""
    ds = PFPascalDataset(os.path.join(kp_files, "image_pairs", "val_pairs.csv"), str(kp_files), gpu_resize=True)
    it = ds[0]
    a, b = it["source_image"].double().mean(2), it["target_image"].double().mean(2)
    n = int((it["source_points"][0] != -1).sum())
    good = bad = 0.0
    for k in range(n):
        xa, ya = (int(round(float(v))) - 1 for v in it["source_points"][:, k])
        xb, yb = (int(round(float(v))) - 1 for v in it["target_points"][:, k])
        xo, yo = (int(round(float(v))) - 1 for v in it["source_points"][:, (k + 1) % n])
        good += abs(float(a[ya, xa] - b[yb, xb]))
        bad += abs(float(a[yo, xo] - b[yb, xb]))
    assert good / n < 25 and good < 0.6 * bad, (good / n, bad / n)


def test_hook_determinism_and_keypoints(kp_files):
    csv = os.path.join(kp_files, "image_pairs", "train_pairs.csv")
    ds = PFPascalDataset(csv, str(kp_files), gpu_resize=True)
    batch = collate_uint8_pairs([ds[i] for i in range(4)])
    aug = PairAugment()
    meta = batch["pixel_meta"]
    p1 = draw_params(meta, 32, 40, aug, torch.Generator().manual_seed(5))
    p2 = draw_params(meta, 32, 40, aug, torch.Generator().manual_seed(5))
    p3 = draw_params(meta, 32, 40, aug, torch.Generator().manual_seed(6))
    assert p1.dtype == torch.float32 and p1.shape == (8, 8) and torch.isfinite(p1).all()
    assert torch.equal(p1, p2) and not torch.equal(p1, p3)
    # the flip is per pair: source and target maps share their orientation
    det = p1[:, 0] * p1[:, 4] - p1[:, 1] * p1[:, 3]
    assert torch.equal(det[:4] < 0, det[4:] < 0)
    assert (p1[:, 6] >= 0.8 - 1e-6).all() and (p1[:, 6] <= 1.2 + 1e-6).all() and (p1[:, 7].abs() <= 0.2 + 1e-6).all()
    with pytest.raises(ValueError, match="CPU"):
        draw_params(meta, 32, 40, aug, None)

    keep = {k: v.clone() for k, v in batch.items()}
    run = lambda seed: gpu_pair_batch(batch, "cpu", 32, 40, augment=aug,  # noqa: E731
                                      generator=torch.Generator().manual_seed(seed))
    a, b, c = run(5), run(5), run(6)
    assert all(torch.equal(batch[k], keep[k]) for k in keep)       # the host batch is not modified
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["source_image"], c["source_image"])
    assert not torch.equal(a["source_points"], c["source_points"])
    # what the hook documents: images by the definition in fp32, points through the same rows, sizes rewritten
    want = ref.warp_norm_u8(batch["pixels"], meta, p1, 32, 40, IMAGENET_MEAN, IMAGENET_STD)
    got = torch.cat((a["source_image"], a["target_image"]))
    assert got.dtype == torch.float32 and float((got - want).abs().max()) < 2e-4 * 1.2
    sp, tp = transform_pair_points(batch["source_points"], batch["target_points"], p1, 32, 40)
    assert torch.equal(a["source_points"], sp) and torch.equal(a["target_points"], tp)
    assert a["source_points"].dtype == batch["source_points"].dtype
    holes = (a["source_points"] == -1).all(1)
    assert torch.equal(holes, (a["target_points"] == -1).all(1))
    assert bool((~holes).any())
    for k in ("source_im_size", "target_im_size"):
        assert torch.equal(a[k], torch.tensor([32.0, 40.0, 3.0]).expand(4, 3))
    assert torch.equal(a["L_pck"], batch["L_pck"])
    # without augmentation nothing but the images changes; weak batches just get warped images
    plain = gpu_pair_batch(batch, "cpu", 32, 40)
    assert torch.equal(plain["source_points"], batch["source_points"])
    weak = {k: batch[k] for k in ("pixels", "pixel_meta")}
    w = gpu_pair_batch(weak, "cpu", 32, 40, augment=aug, generator=torch.Generator().manual_seed(5))
    assert set(w) == {"source_image", "target_image"} and torch.equal(w["source_image"], a["source_image"])


def test_pair_augment_rejects_bad_ranges():
    for kw in ({"scale": (0.0, 1.0)}, {"gain": (1.2, 0.8)}, {"flip": 1.5}, {"rot_deg": float("nan")}, {"bias": -1.0}):
        with pytest.raises(ValueError):
            PairAugment(**kw)


def _cli_args(kp_files, *extra):
    return ["--loss", "strong", "--dataset_image_path", str(kp_files),
            "--train_pairs_csv", os.path.join(kp_files, "image_pairs", "train_pairs.csv"),
            "--val_pairs_csv", os.path.join(kp_files, "image_pairs", "val_pairs.csv"),
            "--batch_size", "2", "--image_size", "64", "--ncons_kernel_sizes", "3", "3",
            "--ncons_channels", "4", "1", "--num_workers", "0", *extra]


def test_train_cli_flag_errors(kp_files):
    import train
    a = train.build_parser().parse_args([])
    assert not a.gpu_input and not a.augment
    assert (a.aug_rot_deg, a.aug_scale, a.aug_shift, a.aug_flip, a.aug_gain, a.aug_bias) == (
        15.0, [0.8, 1.25], 0.1, 0.5, [0.8, 1.2], 0.2)
    d = PairAugment()
    assert (d.rot_deg, tuple(d.scale), d.shift, d.flip, tuple(d.gain), d.bias) == (15.0, (0.8, 1.25), 0.1, 0.5,
                                                                                   (0.8, 1.2), 0.2)
    for flags, word in ((["--augment", "--synthetic", "8"], "synthetic"),
                        (["--augment", "--cpu_resize"], "cpu_resize"),
                        (["--gpu_input", "--cpu_resize"], "cpu_resize"),
                        (["--loss", "strong", "--synthetic", "8", "--augment"], "synthetic")):
        with pytest.raises(SystemExit) as e:
            train.main(flags)
        assert word in str(e.value) and "float images" in str(e.value)
    with pytest.raises(SystemExit) as e:
        train.main(_cli_args(kp_files, "--cpu_resize", "--augment"))
    assert "float images" in str(e.value)
    with pytest.raises(SystemExit) as e:
        train.main(_cli_args(kp_files, "--augment", "--aug_scale", "0", "1"))
    assert "scale" in str(e.value)


def test_augment_seed_fits_the_generator_and_separates_ranks():
    import train
    for seed in (1, 12345678, 20000000, 1234567890, 2147483647, 2 ** 32 - 1, 2 ** 63 - 1, -5):
        seeds = [train.augment_seed(seed, rank, 1) for rank in range(8)]
        assert len(set(seeds)) == 8
        for v in seeds:
            assert 0 <= v < 2 ** 63
            torch.Generator().manual_seed(v)                        # raises when out of range
        assert train.augment_seed(seed, 0, 1) != train.augment_seed(seed, 0, 2)
    assert train.augment_seed(1, 0, 1) != train.augment_seed(2, 0, 1)


@pytest.mark.parametrize("seed", ["1234567890", "2147483647"])
def test_train_cli_32_bit_seed(kp_files, seed, monkeypatch, capsys):
    """A large --seed runs in every mode: without the new flags (where no
    augmentation generator exists) and with --augment."""
    import train
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    small = ["--batch_size", "2", "--image_size", "64", "--ncons_kernel_sizes", "3", "3", "--ncons_channels", "4", "1",
             "--max_steps", "1", "--seed", seed]
    train.main(["--synthetic", "4", *small])
    train.main(["--loss", "strong", "--synthetic", "4", *small])
    train.main(_cli_args(kp_files, "--max_steps", "1", "--seed", seed))
    train.main(_cli_args(kp_files, "--augment", "--max_steps", "1", "--seed", seed))
    out = capsys.readouterr().out
    assert out.count("1 steps in") == 4


@pytest.mark.parametrize("flag", ["--gpu_input", "--augment"])
def test_train_cli_strong_uint8_path_cpu(kp_files, flag, monkeypatch, capsys):
    import train
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    calls = []
    real = train.gpu_pair_batch

    def spy(batch, device, oh, ow, augment=None, generator=None):
        calls.append(augment)
        out = real(batch, device, oh, ow, augment=augment, generator=generator)
        assert out["source_image"].shape == (2, 3, 64, 64) and "source_points" in out
        return out
    monkeypatch.setattr(train, "gpu_pair_batch", spy)
    train.main(_cli_args(kp_files, flag, "--max_steps", "2"))
    out = capsys.readouterr().out
    losses = [float(ln.split()[3]) for ln in out.splitlines() if ln.startswith("step ")]
    assert len(losses) == 2 and all(math.isfinite(v) and abs(v) < 1e6 for v in losses), out
    assert len(calls) == 2
    assert all((c is not None) == (flag == "--augment") for c in calls)


def test_train_cli_validation_is_not_augmented(kp_files, monkeypatch, tmp_path):
    """One epoch with --augment: training batches are augmented, validation
    batches take the plain resize with their points untouched."""
    import train
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    calls = []
    real = train.gpu_pair_batch

    def spy(batch, device, oh, ow, augment=None, generator=None):
        out = real(batch, device, oh, ow, augment=augment, generator=generator)
        calls.append((augment is not None, torch.equal(out["source_points"], batch["source_points"])))
        return out
    monkeypatch.setattr(train, "gpu_pair_batch", spy)
    args = _cli_args(kp_files, "--augment", "--num_epochs", "1", "--result-model-dir", str(tmp_path))
    args[args.index("--batch_size") + 1] = "1"
    train.main(args)
    assert calls == [(True, False)] * 5 + [(False, True)]
