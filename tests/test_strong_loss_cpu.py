"""Keypoint-supervised loss on the CPU: the oracle (ops/reference.py
keypoint_ce), its closed-form gradient, the op, the dataset, the Trainer option
and the train.py flag."""
import pytest
import torch

from ncnet_amd.ops import reference as ref
from tests.strong_loss_cases import learning_setup, make_case, run_learning


@pytest.mark.parametrize("name", ["small", "edge", "train"])
def test_closed_form_gradient_matches_fp64_autograd(name):
    """-1 padding, corner points, an image without keypoints and two keypoints
    in one cell are all in the cases (strong_loss_cases.make_case)."""
    x, kp = make_case(name)
    xd = x.double().requires_grad_(True)
    loss = ref.keypoint_ce(xd, *kp)
    loss.backward()
    g = ref.keypoint_ce_grad(xd.detach(), *kp)
    loss = loss.detach()
    assert torch.isfinite(loss) and float(loss) > 0
    rel = float((g - xd.grad).abs().max() / xd.grad.abs().max())
    print(f"{name}: loss {float(loss):.6f} closed form vs autograd {rel:.3e}")
    assert rel < 1e-12
    # non-zero only on the rows and columns some keypoint touches
    assert 0 < float((xd.grad != 0).double().mean()) < 1


def test_edge_case_contents():
    """The 'edge' case really holds what its tests rely on."""
    x, (sp, tp, ssz, tsz) = make_case("edge")
    valid = ref.keypoint_valid(sp, tp)
    assert not valid[1].any() and valid[0].any() and valid[2].any()       # image 1 has no keypoints
    assert (sp[0, :, -3:] == -1).all() and not valid[0, -3:].any()         # -1 padding
    assert sp[0, :, 0].tolist() == [1.0, 1.0] and sp[0, :, 1].tolist() == [float(ssz[0, 1]), float(ssz[0, 0])]
    assert float(sp[0, 0, 2]) < 0 and float(sp[0, 0, 3]) > float(ssz[0, 1])   # outside the image, still valid
    assert valid[0, 2] and valid[0, 3]
    U = ref.keypoint_weight_maps(sp.double(), ssz.double(), x.shape[2], x.shape[3])
    assert torch.equal(U[0, 4] > 0, U[0, 5] > 0) and not torch.equal(U[0, 4], U[0, 5])   # two keypoints, one cell
    assert torch.allclose(U.sum(2), torch.ones_like(U.sum(2)))
    # corners land on the corner cells with weight 1
    assert float(U[0, 0, 0]) == 1.0 and float(U[0, 1, -1]) == 1.0


def test_all_invalid_batch_is_zero():
    x, (sp, tp, ssz, tsz) = make_case("small")
    sp, tp = torch.full_like(sp, -1.0), torch.full_like(tp, -1.0)
    xd = x.double().requires_grad_(True)
    loss = ref.keypoint_ce(xd, sp, tp, ssz, tsz)
    loss.backward()
    assert float(loss) == 0.0 and torch.count_nonzero(xd.grad) == 0
    assert torch.count_nonzero(ref.keypoint_ce_grad(xd.detach(), sp, tp, ssz, tsz)) == 0


def test_strong_loss_from_corr_cpu_is_the_oracle():
    from ncnet_amd.ops.loss import strong_loss_from_corr
    x, kp = make_case("edge")
    batch = dict(zip(("source_points", "target_points", "source_im_size", "target_im_size"), kp))
    xa = x.clone().requires_grad_(True)
    xb = x.clone().requires_grad_(True)
    la = strong_loss_from_corr(xa, batch)
    lb = ref.keypoint_ce(xb, *kp)
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(xa.grad, xb.grad)
    with pytest.raises(KeyError):
        strong_loss_from_corr(x, {"source_points": kp[0]})


def test_synthetic_correspondence_dataset():
    from ncnet_amd.data import SyntheticCorrespondenceDataset
    from ncnet_amd.data.datasets import synthetic_correspondence_batch
    ds = SyntheticCorrespondenceDataset(4, 64, seed=3)
    assert len(ds) == 4
    a, b, c = ds[1], ds[1], ds[2]
    assert set(a) == {"source_image", "target_image", "source_points", "target_points", "source_im_size",
                      "target_im_size", "L_pck"}
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["source_image"], c["source_image"])
    ref_b = synthetic_correspondence_batch(1, 64, seed=3 * 100003 + 1)
    assert all(torch.equal(a[k], ref_b[k][0]) for k in a)
    assert a["source_image"].shape == (3, 64, 64) and a["target_image"].shape == (3, 64, 64)
    assert a["source_points"].shape == (2, 20) and a["target_points"].shape == (2, 20)
    assert a["source_im_size"].tolist() == [64.0, 64.0, 3.0] and a["L_pck"].shape == (1,)
    with pytest.raises(IndexError):
        ds[4]
    batch = torch.utils.data.default_collate([ds[0], ds[1]])
    assert batch["source_points"].shape == (2, 2, 20) and batch["source_im_size"].shape == (2, 3)


def _tiny_model():
    from ncnet_amd.models import ImMatchNet
    torch.manual_seed(0)
    return ImMatchNet(use_cuda=False, ncons_kernel_sizes=[3, 3], ncons_channels=[4, 1])


def test_trainer_strong_step_cpu():
    from ncnet_amd.data.datasets import synthetic_correspondence_batch
    from ncnet_amd.engine.trainer import Trainer, make_adam, strong_loss
    from ncnet_amd.parallel.dist import DistContext
    model = _tiny_model()
    batch = synthetic_correspondence_batch(2, 96, seed=5)
    ctx = DistContext(device=torch.device("cpu"))
    params = [p for p in model.parameters() if p.requires_grad]
    before = [p.detach().clone() for p in model.NeighConsensus.parameters()]
    tr = Trainer(model, make_adam(params, 1e-3), ctx, loss="strong")
    model.train()
    loss = tr.train_step(batch)
    assert torch.isfinite(loss)
    after = list(model.NeighConsensus.parameters())
    assert all(torch.isfinite(p).all() for p in after)
    assert any(not torch.equal(a, b) for a, b in zip(after, before))
    # the positive volumes only: [B,1,h,w,h,w]
    with torch.no_grad():
        f, hw = model.extract(torch.cat((batch["source_image"], batch["target_image"]), 0))
        vol = model.match_volumes_from_features(f, hw, 2)
        assert vol.shape == (2, 1, 6, 6, 6, 6)
        assert torch.allclose(strong_loss(model, batch), ref.keypoint_ce(
            vol, batch["source_points"], batch["target_points"], batch["source_im_size"], batch["target_im_size"]))
    ev = tr.eval_step(batch)
    assert torch.isfinite(ev) and len(tr._pck) == 1 and tr._pck[0].shape == (2,)
    with pytest.raises(ValueError):
        Trainer(model, make_adam(params, 1e-3), ctx, loss="other")
    assert Trainer(model, make_adam(params, 1e-3), ctx).loss == "weak"


def test_train_cli_strong_cpu(monkeypatch, capsys):
    import train
    assert train.build_parser().parse_args([]).loss == "weak"
    with pytest.raises(SystemExit) as e:
        train.main(["--loss", "strong"])
    assert "keypoints" in str(e.value)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    train.main(["--loss", "strong", "--synthetic", "8", "--max_steps", "2", "--batch_size", "2",
                "--image_size", "240"])
    out = capsys.readouterr().out
    assert "loss='strong'" in out and "step 2 loss" in out and "2 steps in" in out
    losses = [float(ln.split()[3]) for ln in out.splitlines() if ln.startswith("step ")]
    assert len(losses) == 2 and all(v == v and abs(v) < 1e6 for v in losses)


def test_learning_cpu():
    """The bar of the GPU learning test (tests/test_gpu_strong_loss.py), on the
    reference path: 8x8x8x8 volumes from 32-channel unit features (target =
    source rolled by one cell + 0.3 noise), 10 keypoints per image with
    tp = sp + 8 px on 64 px images, NC (3,3)/(16,1), Adam lr 5e-3, 40 steps on
    the fixed batch: the loss must end below half its initial value."""
    first, last = run_learning(*learning_setup("cpu"))
    print(f"learning (cpu): {first:.4f} -> {last:.4f}")
    assert last < 0.5 * first
