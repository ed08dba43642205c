"""The augmenting input kernel on the MI355X (csrc/dataprep.hip warp_norm_u8):
against the fp64 oracle of its definition (ops/reference.py::warp_norm_u8),
bit for bit against resize_norm_u8 on plain-resize rows, through
gpu_pair_batch, on blobs at keypoints, and under train.py --loss strong
--augment."""
import math
import os
import sys

import pytest
import torch

from ncnet_amd.data.augment import PairAugment, draw_params, resize_params
from ncnet_amd.data.datasets import collate_uint8_pairs, gpu_pair_batch
from ncnet_amd.data.transforms import IMAGENET_MEAN, IMAGENET_STD
from ncnet_amd.ops import _ext
from ncnet_amd.ops import reference as ref

from tests import augment_cases as ac

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the bound of test_resize_norm_u8_kernel (tests/test_gpu_kernels.py); the gain scales the error with the value
BOUND = 2e-4
WIDE = PairAugment(rot_deg=180.0, scale=(0.5, 2.0), shift=0.6, flip=0.5, gain=(0.8, 1.25), bias=0.2)
# (H, W); 5 x 3 is 45 bytes, so every later image starts at an odd byte offset
SIZES = ((1, 6), (5, 3), (6, 1), (2, 2), (31, 32), (32, 17), (17, 9), (32, 32))


def _noise(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for h, w in sizes]


def _kernel(pix, meta, params, oh, ow):
    out = torch.full((meta.shape[0], 3, oh, ow), float("nan"), dtype=torch.float32, device=DEV)
    _ext.ext().warp_norm_u8(pix.to(DEV), meta.to(DEV), params.to(DEV), out, list(IMAGENET_MEAN), list(IMAGENET_STD))
    return out


@pytest.mark.parametrize("oh,ow", [(7, 9), (19, 23)])       # less than one 256-thread block; a partial second block
def test_kernel_matches_fp64_oracle(oh, ow):
    ims = _noise(SIZES, seed=oh)
    pix, meta = ac.pack(ims)
    assert any(int(o) % 2 for o in meta[:, 0])
    params = draw_params(meta, oh, ow, WIDE, torch.Generator().manual_seed(100 + oh))
    params[4, 2] += 10 * 32                                  # 31 x 32: every sample right of the image
    # what the parameters cover: images sampled partly outside their border, one wholly outside
    q = params.double()
    oy, ox = torch.meshgrid(torch.arange(oh, dtype=torch.float64), torch.arange(ow, dtype=torch.float64),
                            indexing="ij")
    outside = []
    for i, (_, h, w) in enumerate(meta.tolist()):
        sx = q[i, 0] * ox + q[i, 1] * oy + q[i, 2]
        sy = q[i, 3] * ox + q[i, 4] * oy + q[i, 5]
        outside.append(float(((sx < 0) | (sx > w - 1) | (sy < 0) | (sy > h - 1)).double().mean()))
    assert outside[4] == 1.0 and sum(0 < f < 1 for f in outside) >= 3, outside
    det = q[:, 0] * q[:, 4] - q[:, 1] * q[:, 3]
    assert bool((det < 0).any()) and bool((det > 0).any())  # flipped and unflipped images

    got = _kernel(pix, meta, params, oh, ow)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all()                         # every element written
    want = ref.warp_norm_u8(pix, meta, params, oh, ow, IMAGENET_MEAN, IMAGENET_STD)
    err = float((got.double().cpu() - want).abs().max())
    bound = BOUND * float(params[:, 6].max())
    print(f"warp_norm_u8 {oh}x{ow}: max abs error {err:.3e} (bound {bound:.3e})")
    assert err < bound


def test_nan_and_far_parameters_stay_in_range():
    """No parameter row can form an out-of-range address: NaN / inf / huge
    coefficients clamp onto a border pixel."""
    ims = [torch.full((3, 4, 3), 200, dtype=torch.uint8), torch.full((2, 2, 3), 10, dtype=torch.uint8)]
    pix, meta = ac.pack(ims)
    params = torch.tensor([[float("nan"), 0, 0, 0, float("inf"), -float("inf"), 1, 0],
                           [1e30, -1e30, 5e8, 0, 0, -7, 1, 0]])
    got = _kernel(pix, meta, params, 5, 6).cpu()
    want = ref.warp_norm_u8(pix, meta, params, 5, 6, IMAGENET_MEAN, IMAGENET_STD)
    assert torch.isfinite(got).all() and float((got.double() - want).abs().max()) < BOUND


@pytest.mark.parametrize("oh,ow", [(24, 40), (24, 1)])
def test_plain_resize_rows_reproduce_resize_norm_u8_bit_for_bit(oh, ow):
    # the last two: fp32 (W - 1) / 39 * 39 > W - 1 for W = 6, 12 and (H - 1) / 23 * 23 > H - 1 for H = 16, 31, so
    # the last column / row is sampled a few ulp past the border pixel
    ims = _noise(((17, 9), (40, 33), (8, 5), (16, 6), (31, 12)), seed=7)
    pix, meta = ac.pack(ims)
    if (oh, ow) == (24, 40):
        p = resize_params(meta, oh, ow)
        assert bool((p[3:, 0] * 39 > torch.tensor([5.0, 11.0])).all())
        assert bool((p[3:, 4] * 23 > torch.tensor([15.0, 30.0])).all())
    pix_d, meta_d = pix.to(DEV), meta.to(DEV)
    want = torch.full((len(ims), 3, oh, ow), float("nan"), dtype=torch.float32, device=DEV)
    _ext.ext().resize_norm_u8(pix_d, meta_d, want, list(IMAGENET_MEAN), list(IMAGENET_STD))
    got = _kernel(pix, meta, resize_params(meta, oh, ow), oh, ow)
    assert torch.isfinite(want).all()
    assert torch.equal(got, want)


def _pair_samples(seed=3):
    g = torch.Generator().manual_seed(seed)
    samples = []
    for (h1, w1), (h2, w2) in (((31, 32), (5, 3)), ((32, 17), (17, 9)), ((24, 30), (32, 32))):
        pts = []
        for h, w in ((h1, w1), (h2, w2)):
            p = torch.full((2, 20), -1.0)
            p[0, :9] = 1 + torch.rand(9, generator=g) * (w - 1)
            p[1, :9] = 1 + torch.rand(9, generator=g) * (h - 1)
            pts.append(p)
        samples.append({"source_image": torch.randint(0, 256, (h1, w1, 3), generator=g, dtype=torch.uint8),
                        "target_image": torch.randint(0, 256, (h2, w2, 3), generator=g, dtype=torch.uint8),
                        "source_im_size": torch.tensor([h1, w1, 3.0]), "target_im_size": torch.tensor([h2, w2, 3.0]),
                        "source_points": pts[0], "target_points": pts[1], "L_pck": torch.tensor([float(max(h1, w1))])})
    return samples


def test_whole_hook_gpu_equals_cpu():
    batch = collate_uint8_pairs(_pair_samples())
    aug = PairAugment()
    before = _ext.DISPATCH["torch_fallback"]
    got = gpu_pair_batch(batch, DEV, 19, 23, augment=aug, generator=torch.Generator().manual_seed(9))
    want = gpu_pair_batch(batch, "cpu", 19, 23, augment=aug, generator=torch.Generator().manual_seed(9))
    assert _ext.DISPATCH["torch_fallback"] == before
    assert set(got) == set(want)
    bound = BOUND * aug.gain[1]
    for k in ("source_image", "target_image"):
        assert got[k].is_cuda and got[k].dtype == torch.float32 and got[k].shape == (3, 3, 19, 23)
        err = float((got[k].cpu() - want[k]).abs().max())
        print(f"hook {k}: max |gpu - cpu| {err:.3e} (bound {bound:.3e})")
        assert err < bound
    for k in ("source_points", "target_points", "source_im_size", "target_im_size", "L_pck"):
        assert got[k].is_cuda and torch.equal(got[k].cpu(), want[k]), k
    assert not torch.equal(want["source_points"], batch["source_points"])
    assert bool((want["source_points"] != -1).any())


def test_pixels_and_keypoints_move_together_on_the_kernel():
    cases = ac.blob_cases()
    errs = ac.blob_errors(cases, _kernel)
    checked = [e for e, inside in errs if inside >= 6]
    print(f"blob centroid error (kernel): max {max(checked):.3f} px over {len(checked)} keypoints")
    assert len(checked) >= 20
    assert max(checked) < 0.5


def test_binding_rejects_bad_arguments():
    pix, meta = ac.pack(_noise(((4, 4), (3, 5)), seed=1))
    pix, meta = pix.to(DEV), meta.to(DEV)
    params = resize_params(meta, 6, 6).to(DEV)
    out = torch.empty((2, 3, 6, 6), device=DEV)
    mean, std = list(IMAGENET_MEAN), list(IMAGENET_STD)
    f = _ext.ext().warp_norm_u8
    f(pix, meta, params, out, mean, std)
    for bad in (params.cpu(), params.double(), params[:, :7].contiguous(), params[:1], params.t().contiguous().t(),
                params.view(-1)):
        with pytest.raises(RuntimeError):
            f(pix, meta, bad, out, mean, std)
    with pytest.raises(RuntimeError):
        f(pix.float(), meta, params, out, mean, std)
    with pytest.raises(RuntimeError):
        f(pix, meta.int(), params, out, mean, std)
    with pytest.raises(RuntimeError):
        f(pix, meta, params, out[:, :2].contiguous(), mean, std)
    with pytest.raises(RuntimeError):
        f(pix, meta, params, out, mean[:2], std)
    torch.cuda.synchronize()


def test_train_cli_strong_augment_gpu(tmp_path, monkeypatch, capsys):
    """Three steps of train.py --loss strong --augment on generated keypoint
    files: the release extension runs warp_norm_u8 once per training batch
    (one batch of lookahead), nothing falls back to torch, losses are finite."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import make_keypoint_pairs
    finally:
        sys.path.pop(0)
    import train
    from ncnet_amd import config
    make_keypoint_pairs.main(["--out", str(tmp_path), "--pairs", "10", "--min_side", "100", "--max_side", "140"])
    assert _ext.available()
    variant = config.RUNTIME.ext_variant
    assert _ext.ext().__name__ == ("ncnet_amd._C" if variant in ("", "release") else f"ncnet_amd._C_{variant}")
    launches = []
    real = _ext.ext().warp_norm_u8
    monkeypatch.setattr(_ext.ext(), "warp_norm_u8", lambda *a: (launches.append(a[2].shape), real(*a))[1])
    before = _ext.DISPATCH["torch_fallback"]
    train.main(["--loss", "strong", "--augment", "--dataset_image_path", str(tmp_path),
                "--train_pairs_csv", os.path.join(tmp_path, "image_pairs", "train_pairs.csv"),
                "--val_pairs_csv", os.path.join(tmp_path, "image_pairs", "val_pairs.csv"),
                "--batch_size", "4", "--image_size", "128", "--max_steps", "3", "--num_workers", "0"])
    out = capsys.readouterr().out
    losses = [float(ln.split()[3]) for ln in out.splitlines() if ln.startswith("step ")]
    assert len(losses) == 3 and all(math.isfinite(v) and abs(v) < 1e6 for v in losses), out
    assert launches == [torch.Size([8, 8])] * 3
    assert _ext.DISPATCH["torch_fallback"] == before
