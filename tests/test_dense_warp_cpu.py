"""Warp-supervised training on the CPU: the oracle (ops/reference.py dense_ce),
its closed-form gradient and target table, the view maps, the two-view input
path, the op, the Trainer option and the train.py flag."""
import pytest
import torch

from ncnet_amd.data.augment import PairAugment, draw_params, view_maps
from ncnet_amd.ops import reference as ref
from tests.dense_warp_cases import (CASES, dense_weight_maps, learning_setup, make_case, out_of_frame_maps,
                                    run_learning, shift_maps)


@pytest.mark.parametrize("name", list(CASES))
def test_closed_form_gradient_matches_fp64_autograd(name):
    x, maps = make_case(name)
    xd = x.double().requires_grad_(True)
    loss = ref.dense_ce(xd, maps)
    loss.backward()
    g = ref.dense_ce_grad(xd.detach(), maps)
    loss = loss.detach()
    assert torch.isfinite(loss) and float(loss) > 0
    rel = float((g - xd.grad).abs().max() / xd.grad.abs().max())
    print(f"{name}: loss {float(loss):.6f} closed form vs autograd {rel:.3e}")
    assert rel < 1e-12


def test_all_invalid_batch_is_zero():
    x, _ = make_case("small")
    maps = out_of_frame_maps(x.shape[0])
    xd = x.double().requires_grad_(True)
    loss = ref.dense_ce(xd, maps)
    loss.backward()
    assert float(loss.detach()) == 0.0 and torch.count_nonzero(xd.grad) == 0
    assert torch.count_nonzero(ref.dense_ce_grad(xd.detach(), maps)) == 0


def test_identity_targets_are_one_hot_on_the_same_cell():
    maps = torch.tensor([[[1.0, 0, 0, 0, 1, 0] * 2] * 2], dtype=torch.float64)
    h, w = 5, 9
    ca, wa, oka, cb, wb, okb = ref.dense_targets(maps, h, w, h, w)
    eye = torch.eye(h * w, dtype=torch.float64).unsqueeze(0)
    assert oka.all() and okb.all()
    assert torch.equal(dense_weight_maps(ca, wa, h * w), eye) and torch.equal(dense_weight_maps(cb, wb, h * w), eye)
    # the last cell of an axis sits at i0 = n - 2 with f = 1
    assert ca[0, -1].tolist() == [(h - 2) * w + w - 2, (h - 2) * w + w - 1, (h - 1) * w + w - 2, h * w - 1]
    assert wa[0, -1].tolist() == [0.0, 0.0, 0.0, 1.0]
    # an axis of length 1 takes coordinate 0
    ca, wa, oka, _, _, _ = ref.dense_targets(maps, 1, 4, 1, 4)
    assert oka.all() and torch.equal(dense_weight_maps(ca, wa, 4), torch.eye(4, dtype=torch.float64).unsqueeze(0))


def test_odd_case_contents():
    """The 'odd' case really holds what its tests rely on."""
    _, maps = make_case("odd")
    _, hA, wA, hB, wB = CASES["odd"]
    ca, wa, oka, cb, wb, okb = ref.dense_targets(maps, hA, wA, hB, wB)
    assert oka[0].all() and okb[0].all()                                  # the identity: every cell valid
    assert wa[0, -1].tolist() == [0.0, 0.0, 0.0, 1.0] and int(ca[0, -1, 3]) == hB * wB - 1
    assert not oka[1].any() and not okb[1].any()                          # every cell out of frame
    assert 0 < int(oka[2].sum()) < hA * wA and 0 < int(okb[2].sum()) < hB * wB
    assert float(maps[2, 0, 0]) < 0                                       # flipped
    # part of image 2's cells are excluded by the SOURCE frame alone
    src_only = maps[2:].clone()
    src_only[:, :, 6:] = torch.tensor([1.0, 0, 0, 0, 1, 0], dtype=torch.float64)
    assert int(ref.dense_targets(src_only, hA, wA, hB, wB)[2].sum()) > int(oka[2].sum())
    for v in (dense_weight_maps(ca, wa, hB * wB), dense_weight_maps(cb, wb, hA * wA)):
        s = v.sum(2)
        assert torch.allclose(s[s > 0], torch.ones((), dtype=torch.float64), atol=1e-12)


def _unit_coordinates(maps, h, w, side):
    """The four mapped coordinates [B, h*w, 4] of one side's cell centres."""
    i, j = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    ux = (j / (w - 1) if w > 1 else torch.zeros_like(j)).reshape(1, -1)
    uy = (i / (h - 1) if h > 1 else torch.zeros_like(i)).reshape(1, -1)
    m = maps[:, side]
    return torch.stack([m[:, k:k + 1] * ux + m[:, k + 1:k + 2] * uy + m[:, k + 2:k + 3] for k in (0, 3, 6, 9)], 2)


@pytest.mark.parametrize("name", list(CASES))
def test_no_case_coordinate_sits_on_the_frame_border(name):
    """The valid flags of the cases do not hang on a rounding: no mapped
    coordinate lies within 1e-9 of 0 or 1.  The identity image of 'odd' is
    left out: its coordinates are products with 0 and 1 of the cell centres
    themselves, exact in any evaluation order, and ON the border by design."""
    _, maps = make_case(name)
    _, hA, wA, hB, wB = CASES[name]
    if name == "odd":
        maps = maps[1:]
    for side, (h, w) in enumerate(((hA, wA), (hB, wB))):
        q = _unit_coordinates(maps, h, w, side)
        d = torch.minimum(q.abs(), (q - 1).abs()).min()
        assert float(d) > 1e-9, (name, side, float(d))


def _blob_image(h, w, cx, cy, sigma=6.0):
    y, x = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    v = torch.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * sigma ** 2))
    return (v * 255).round().clamp(0, 255).to(torch.uint8).unsqueeze(2).expand(h, w, 3).contiguous()


def _centroid(img):
    v = img.sum(0).double()
    v = (v - v.min()).clamp(min=0)
    v = torch.where(v > 0.2 * v.max(), v, torch.zeros_like(v))
    y, x = torch.meshgrid(torch.arange(v.shape[0], dtype=torch.float64),
                          torch.arange(v.shape[1], dtype=torch.float64), indexing="ij")
    return float((v * x).sum() / v.sum()), float((v * y).sum() / v.sum())


def test_view_maps_round_trip():
    """A blob drawn in the source where a valid A-cell centre looks appears, in
    view B rendered by ops/reference.py warp_norm_u8, at the position the A -> B
    map gives (the centroid check of test_augment_cpu.py)."""
    H, W, oh, ow, grid = 300, 360, 200, 240, 9
    meta = torch.tensor([[0, H, W]] * 2, dtype=torch.int64)
    checked = 0
    for seed in range(4):
        g = torch.Generator().manual_seed(100 + seed)
        params = draw_params(meta, oh, ow, PairAugment(gain=(1.0, 1.0), bias=0.0), g)
        maps = view_maps(params, meta, oh, ow)
        _, _, ok, _, _, _ = ref.dense_targets(maps, grid, grid, grid, grid)
        q = _unit_coordinates(maps, grid, grid, 0)[0]                    # [cells, 4]: B x, B y, source x, source y
        # a valid A cell whose blob stays clear of both frames' borders
        inner = ok[0] & (q > 0.2).all(1) & (q < 0.8).all(1)
        if not inner.any():
            continue
        cell = int(torch.nonzero(inner)[0])
        sx, sy = float(q[cell, 2]) * (W - 1), float(q[cell, 3]) * (H - 1)
        pix = _blob_image(H, W, sx, sy).reshape(-1)
        out = ref.warp_norm_u8(pix, meta, params, oh, ow, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
        i, j = divmod(cell, grid)
        ax, ay = _centroid(out[0])
        bx, by = _centroid(out[1])
        print(f"seed {seed}: cell ({i}, {j}) A at ({ax:.2f}, {ay:.2f}) B at ({bx:.2f}, {by:.2f}) "
              f"expected B ({float(q[cell, 0]) * (ow - 1):.2f}, {float(q[cell, 1]) * (oh - 1):.2f})")
        assert abs(ax - j / (grid - 1) * (ow - 1)) < 0.5 and abs(ay - i / (grid - 1) * (oh - 1)) < 0.5
        assert abs(bx - float(q[cell, 0]) * (ow - 1)) < 0.5 and abs(by - float(q[cell, 1]) * (oh - 1)) < 0.5
        checked += 1
    assert checked >= 2


def test_view_maps_are_mutually_inverse_and_reject_singular_views():
    meta = torch.tensor([[0, 300, 400], [0, 250, 210]] * 2, dtype=torch.int64)
    params = draw_params(meta, 400, 400, PairAugment(), torch.Generator().manual_seed(3))
    maps = view_maps(params, meta, 400, 400)
    assert maps.shape == (2, 2, 12) and maps.dtype == torch.float64
    for b in range(2):
        for k in (0, 1):
            f, g = maps[b, k, :6], maps[b, 1 - k, :6]
            F, G = f[[0, 1, 3, 4]].view(2, 2), g[[0, 1, 3, 4]].view(2, 2)
            assert torch.allclose(F @ G, torch.eye(2, dtype=torch.float64), atol=1e-12)
            assert torch.allclose(F @ g[[2, 5]] + f[[2, 5]], torch.zeros(2, dtype=torch.float64), atol=1e-12)
    bad = params.clone()
    bad[1, :6] = 0.0
    with pytest.raises(ValueError):
        view_maps(bad, meta, 400, 400)
    with pytest.raises(ValueError):
        view_maps(params, meta, 1, 400)


def test_validity_share_of_default_augmentation():
    """With the default PairAugment, 2000 draws from a generator seeded 7 over
    200-600 px sources at 400 x 400 and a 25 x 25 grid, every image keeps more
    than 0.25 of its A cells (a frame or inverse bug drives the share to ~0)."""
    g = torch.Generator().manual_seed(7)
    B = 2000
    hw = torch.randint(200, 601, (B, 2), generator=g)
    meta = torch.cat((torch.zeros(B, 1, dtype=torch.int64), hw), 1).repeat(2, 1)
    params = draw_params(meta, 400, 400, PairAugment(), g)
    maps = view_maps(params, meta, 400, 400)
    _, _, ok, _, _, _ = ref.dense_targets(maps, 25, 25, 25, 25)
    share = ok.double().mean(1)
    print(f"valid A-cell share: mean {float(share.mean()):.3f} min {float(share.min()):.3f}")
    assert float(share.min()) > 0.25


def _image_batch(n=2, seed=0):
    from ncnet_amd.data.datasets import SyntheticImageDataset, collate_uint8_images
    ds = SyntheticImageDataset(n, (60, 80), seed=seed)
    return collate_uint8_images([ds[i] for i in range(n)])


def test_synthetic_image_dataset_and_collate():
    from ncnet_amd.data.datasets import SyntheticImageDataset
    ds = SyntheticImageDataset(3, (60, 80), seed=4)
    a, b, c = ds[1], ds[1], ds[2]
    assert len(ds) == 3 and a["image"].shape == (60, 80, 3) and a["image"].dtype == torch.uint8
    assert torch.equal(a["image"], b["image"]) and not torch.equal(a["image"], c["image"])
    assert float(a["image"].float().std()) > 20                            # not flat, not saturated noise
    with pytest.raises(IndexError):
        ds[3]
    batch = _image_batch(2)
    assert batch["pixel_meta"].tolist() == [[0, 60, 80], [60 * 80 * 3, 60, 80]]
    assert batch["pixels"].numel() == 2 * 60 * 80 * 3 and batch["pixels"].dtype == torch.uint8


def test_gpu_view_batch_cpu_is_deterministic_per_seed():
    from ncnet_amd.data.datasets import gpu_view_batch
    batch = _image_batch(2)
    run = lambda s, **kw: gpu_view_batch(batch, "cpu", 48, 64, PairAugment(),  # noqa: E731
                                         torch.Generator().manual_seed(s), **kw)
    a, b, c = run(5), run(5), run(6)
    assert set(a) == {"source_image", "target_image", "warp_maps"}
    assert a["source_image"].shape == (2, 3, 48, 64) and a["target_image"].shape == (2, 3, 48, 64)
    assert a["warp_maps"].shape == (2, 2, 12) and a["warp_maps"].dtype == torch.float64
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["warp_maps"], c["warp_maps"]) and not torch.equal(a["source_image"], c["source_image"])
    assert not torch.equal(a["source_image"], a["target_image"])
    # the points of the validation batches: A-cell centres and their images in B
    p = run(5, with_points=True)
    assert torch.equal(p["warp_maps"], a["warp_maps"]) and torch.equal(p["source_image"], a["source_image"])
    sp, tp = p["source_points"], p["target_points"]
    assert sp.shape == (2, 2, 625) and tp.shape == (2, 2, 625) and sp.dtype == torch.float32
    assert p["source_im_size"].tolist() == [[48.0, 64.0, 3.0]] * 2 and p["L_pck"].tolist() == [[64.0]] * 2
    _, _, ok, _, _, _ = ref.dense_targets(a["warp_maps"], 25, 25, 25, 25)
    assert torch.equal((sp != -1).all(1), ok) and torch.equal((tp != -1).all(1), ok) and ok.any()
    keep = ok[0]
    assert float(sp[0, 0, keep].min()) >= 1 and float(sp[0, 0, keep].max()) <= 64
    assert float(tp[0, 1, keep].min()) >= 1 and float(tp[0, 1, keep].max()) <= 48
    with pytest.raises(ValueError):
        gpu_view_batch(batch, "cpu", 48, 64, None, torch.Generator())


def test_warp_loss_from_corr_cpu_is_the_oracle():
    from ncnet_amd.ops.loss import warp_loss_from_corr
    x, maps = make_case("odd")
    xa = x.clone().requires_grad_(True)
    xb = x.clone().requires_grad_(True)
    la = warp_loss_from_corr(xa, {"warp_maps": maps})
    lb = ref.dense_ce(xb, maps)
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(xa.grad, xb.grad)
    with pytest.raises(KeyError):
        warp_loss_from_corr(x, {"source_points": maps})
    with pytest.raises(ValueError):
        warp_loss_from_corr(x[:, 0], {"warp_maps": maps})
    with pytest.raises(ValueError):
        warp_loss_from_corr(torch.cat((x, x), 1), {"warp_maps": maps})


def _tiny_model():
    from ncnet_amd.models import ImMatchNet
    torch.manual_seed(0)
    return ImMatchNet(use_cuda=False, ncons_kernel_sizes=[3, 3], ncons_channels=[4, 1])


def test_trainer_warp_steps_cpu():
    from ncnet_amd.data.datasets import gpu_view_batch
    from ncnet_amd.engine.trainer import Trainer, make_adam, warp_loss
    from ncnet_amd.parallel.dist import DistContext
    model = _tiny_model()
    g = torch.Generator().manual_seed(2)
    batch = gpu_view_batch(_image_batch(2), "cpu", 96, 96, PairAugment(), g, with_points=True)
    ctx = DistContext(device=torch.device("cpu"))
    params = [p for p in model.parameters() if p.requires_grad]
    before = [p.detach().clone() for p in model.NeighConsensus.parameters()]
    tr = Trainer(model, make_adam(params, 1e-3), ctx, loss="warp")
    model.train()
    losses = [tr.train_step(batch), tr.train_step(batch)]
    assert all(torch.isfinite(v) for v in losses) and tr.global_step == 2
    after = list(model.NeighConsensus.parameters())
    assert all(torch.isfinite(p).all() for p in after)
    assert any(not torch.equal(a, b) for a, b in zip(after, before))
    with torch.no_grad():
        f, hw = model.extract(torch.cat((batch["source_image"], batch["target_image"]), 0))
        vol = model.match_volumes_from_features(f, hw, 2)
        assert vol.shape == (2, 1, 6, 6, 6, 6)
        assert torch.allclose(warp_loss(model, batch), ref.dense_ce(vol, batch["warp_maps"]))
    ev = tr.eval_step(batch)
    assert torch.isfinite(ev) and len(tr._pck) == 1 and tr._pck[0].shape == (2,)
    with pytest.raises(KeyError):
        tr.train_step({k: v for k, v in batch.items() if k != "warp_maps"})


def test_train_cli_warp_cpu(monkeypatch, capsys):
    import train
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    train.main(["--loss", "warp", "--synthetic", "8", "--max_steps", "2", "--batch_size", "2", "--image_size", "240"])
    out = capsys.readouterr().out
    assert "loss='warp'" in out and "step 2 loss" in out and "2 steps in" in out
    losses = [float(ln.split()[3]) for ln in out.splitlines() if ln.startswith("step ")]
    assert len(losses) == 2 and all(v == v and 0 < v < 1e6 for v in losses)


def test_train_cli_warp_rejects_cpu_resize():
    import train
    with pytest.raises(SystemExit) as e:
        train.main(["--loss", "warp", "--synthetic", "8", "--cpu_resize"])
    assert "--cpu_resize" in str(e.value) and "uint8" in str(e.value)
    with pytest.raises(SystemExit) as e:
        train.main(["--image_dir", "somewhere"])
    assert "--loss warp" in str(e.value)


def test_train_cli_warp_image_sets(tmp_path):
    """--image_dir: sorted, the last tenth (at least one) validates; the CSV
    route takes the distinct names of the first two columns."""
    import train
    for i in range(12):
        (tmp_path / f"im{i:02d}.{'png' if i % 2 else 'JPG'}").write_bytes(b"")
    (tmp_path / "notes.txt").write_text("x")
    args = train.build_parser().parse_args(["--loss", "warp", "--image_dir", str(tmp_path)])
    root, tr, va = train.warp_image_sets(args)
    assert root == str(tmp_path) and len(tr) == 11 and va == ["im11.png"] and tr == sorted(tr)
    (tmp_path / "train_pairs.csv").write_text("source_image,target_image,class,flip\na.jpg,b.jpg,1,0\nb.jpg,c.jpg,1,1\n")
    (tmp_path / "val_pairs.csv").write_text("source_image,target_image,class,flip\nd.jpg,d.jpg,1,0\n")
    args = train.build_parser().parse_args(["--loss", "warp", "--dataset_csv_path", str(tmp_path),
                                            "--dataset_image_path", "imgs"])
    assert train.warp_image_sets(args) == ("imgs", ["a.jpg", "b.jpg", "c.jpg"], ["d.jpg"])


def test_learning_cpu():
    """The strong loss's bar on the reference path: strong_loss_cases'
    8x8x8x8 volumes (target = source rolled by one cell + 0.3 noise, seed 1),
    the maps 'B = A shifted by one cell', NC (3,3)/(16,1), Adam lr 5e-3, 40
    steps on the fixed batch: the loss must end below half its initial value."""
    model, corr, batch = learning_setup("cpu", seed=1)
    assert torch.equal(batch["warp_maps"], shift_maps(corr.shape[0], 8))
    first, last = run_learning(model, corr, batch)
    print(f"learning (cpu): {first:.4f} -> {last:.4f}")
    assert last < 0.5 * first
