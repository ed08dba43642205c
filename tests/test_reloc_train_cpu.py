"""Relocalized training (--relocalization_k_size) on CPU: the backward oracle of
the pooled correlation, the model's pooled training volumes, the CLIs, and the
compiler resources of the HIP backward."""
import glob
import json
import math
import os
import shutil
from pathlib import Path

import pytest
import torch

from ncnet_amd.ops import reference as ref

GRIDS = [(6, 8, 10, 14), (18, 16, 10, 14)]
AMAP, BMAP = [0, 1, 1], [0, 1, 0]


@pytest.mark.parametrize("grid", GRIDS)
def test_oracle_equals_autograd_of_pooled_bmm(grid):
    hA, wA, hB, wB = grid
    torch.manual_seed(3)
    fa = torch.randn(3, hA * wA, 64, dtype=torch.float64, requires_grad=True)
    fb = torch.randn(2, hB * wB, 64, dtype=torch.float64, requires_grad=True)
    corr = torch.bmm(fa[AMAP], fb[BMAP].transpose(1, 2)).view(3, 1, hA, wA, hB, wB)
    pooled, offsets = ref.maxpool4d(corr, 2)
    g = torch.randn_like(pooled)
    want_a, want_b = torch.autograd.grad(pooled, (fa, fb), g)
    ga, gb = ref.corr_pool2_bwd(fa.detach(), fb.detach(), g, offsets, AMAP, BMAP, hA, wA, hB, wB)
    assert ga.dtype == torch.float64 and ga.shape == fa.shape and gb.shape == fb.shape
    assert (ga - want_a).abs().max().item() == 0.0
    assert (gb - want_b).abs().max().item() == 0.0
    assert want_a.abs().max() > 0 and (ga[2] == 0).all()          # image 2 of A is in no volume
    # quantize_g rounds g to bf16 and nothing else
    gq = g.to(torch.bfloat16).to(torch.float64)
    qa, qb = ref.corr_pool2_bwd(fa.detach(), fb.detach(), g, offsets, AMAP, BMAP, hA, wA, hB, wB, quantize_g=True)
    ea, eb = ref.corr_pool2_bwd(fa.detach(), fb.detach(), gq, offsets, AMAP, BMAP, hA, wA, hB, wB)
    assert torch.equal(qa, ea) and torch.equal(qb, eb) and not torch.equal(qa, ga)


def test_backward_table_is_validated_on_the_host():
    from ncnet_amd.ops.correlation import pool2_bwd_table
    aoff, avol, boff, bvol, am, bm = pool2_bwd_table((0, 1, 1, 0), (0, 1, 0, 1), 3, 2, "cpu")
    assert aoff.tolist() == [0, 2, 4, 4] and avol.tolist() == [0, 3, 1, 2]
    assert boff.tolist() == [0, 2, 4] and bvol.tolist() == [0, 2, 1, 3]
    assert am.tolist() == [0, 1, 1, 0] and bm.tolist() == [0, 1, 0, 1] and am.dtype == torch.int32
    with pytest.raises(ValueError):
        pool2_bwd_table((0, 3), (0, 1), 3, 2, "cpu")
    with pytest.raises(ValueError):
        pool2_bwd_table((0, -1), (0, 1), 3, 2, "cpu")
    with pytest.raises(ValueError):
        pool2_bwd_table((0, 1, 1), (0, 1), 3, 2, "cpu")


def _model(k, **kw):
    from ncnet_amd.models import ImMatchNet
    torch.manual_seed(0)
    return ImMatchNet(relocalization_k_size=k, use_cuda=False, ncons_kernel_sizes=[3, 3], ncons_channels=[16, 1], **kw)


def test_model_pools_the_training_volumes():
    m = _model(2)
    m.eval()
    torch.manual_seed(1)
    B = 2
    imgs = torch.randn(2 * B, 3, 128, 128)
    with torch.no_grad():
        f, hw = m.extract(imgs)
        assert tuple(hw) == (8, 8)
        vols, delta = m.weak_loss_volumes_from_features(f, hw, B, return_delta=True)
        assert vols.shape == (2 * B, 1, 4, 4, 4, 4)
        assert torch.equal(m.weak_loss_volumes_from_features(f, hw, B), vols)
        fa, fb = f[:B], f[B:]
        amap, bmap = [0, 1, 1, 0], [0, 1, 0, 1]                    # positives, then sources rolled by -1
        for v in range(2 * B):
            want, wd = m.match_features(fa[amap[v]:amap[v] + 1], hw, fb[bmap[v]:bmap[v] + 1], hw)
            assert (vols[v:v + 1] - want).abs().max() <= 1e-6
            for d, w in zip(delta, wd):
                assert torch.equal(d[v:v + 1].long(), w.long())
        pos, pdelta = m.match_volumes_from_features(f, hw, B, return_delta=True)
        assert pos.shape == (B, 1, 4, 4, 4, 4)
        assert (pos - vols[:B]).abs().max() <= 1e-6
        for d, w in zip(pdelta, delta):
            assert torch.equal(d.long(), w[:B].long())
        assert torch.equal(m.match_volumes_from_features(f, hw, B), pos)

        # k = 3, frozen trunk: the unfused pool of the full volume (12 x 12 features -> 4 x 4 cells)
        m3 = _model(3)
        m3.eval()
        f3 = torch.nn.functional.normalize(torch.randn(2 * B, 144, 64), dim=2)
        v3, d3 = m3.weak_loss_volumes_from_features(f3, (12, 12), B, return_delta=True)
        assert v3.shape == (2 * B, 1, 4, 4, 4, 4) and int(max(d.max() for d in d3)) == 2
        for v in range(2 * B):
            want, wd = m3.match_features(f3[amap[v]:amap[v] + 1], (12, 12), f3[B + bmap[v]:B + bmap[v] + 1], (12, 12))
            assert (v3[v:v + 1] - want).abs().max() <= 1e-6
            for d, w in zip(d3, wd):
                assert torch.equal(d[v:v + 1].long(), w.long())


def test_trainable_trunk_needs_k2():
    m3 = _model(3)
    m3.train()
    f = torch.randn(4, 64, 1024, requires_grad=True)
    with pytest.raises(ValueError, match="k = 2"):
        m3.weak_loss_volumes_from_features(f, (8, 8), 2)
    with pytest.raises(ValueError, match="even grids"):
        m3.match_volumes_from_features(f, (8, 8), 2)
    # k = 2 on CPU is differentiable through the oracle composition
    m2 = _model(2)
    m2.train()
    vols = m2.weak_loss_volumes_from_features(f, (8, 8), 2)
    vols.sum().backward()
    assert f.grad is not None and torch.isfinite(f.grad).all() and f.grad.abs().max() > 0


@pytest.mark.parametrize("k", [0, 2])
def test_trainer_step_reaches_a_trainable_trunk(k):
    """With the last trunk block trainable the step's gradient flows through the
    (pooled) correlation into it: the Trainer runs that trunk under autograd."""
    from ncnet_amd.engine.trainer import Trainer, make_adam
    from ncnet_amd.parallel.dist import DistContext
    m = _model(k)
    trunk = list(m.FeatureExtraction.model[-1][-1].parameters())
    for p in trunk:
        p.requires_grad = True
    m.train()
    params = [p for p in m.parameters() if p.requires_grad]
    tr = Trainer(m, make_adam(params, 1e-4), DistContext(device=torch.device("cpu")))
    torch.manual_seed(5)
    loss = tr.train_step({"source_image": torch.randn(2, 3, 128, 128), "target_image": torch.randn(2, 3, 128, 128)})
    assert torch.isfinite(loss)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in trunk)
    assert any(bool((p.grad != 0).any()) for p in trunk)


def test_k01_is_untouched():
    torch.manual_seed(2)
    imgs = torch.randn(4, 3, 64, 64)
    outs = []
    for k in (0, 1):
        m = _model(k)
        m.eval()
        with torch.no_grad():
            f, hw = m.extract(imgs)
            v, d = m.weak_loss_volumes_from_features(f, hw, 2, return_delta=True)
            assert d is None and v.shape == (4, 1, 4, 4, 4, 4)
            outs.append(v)
    assert torch.equal(outs[0], outs[1])


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("reloc_cli")
    old = os.getcwd()
    os.chdir(d)
    yield d
    os.chdir(old)


_TINY = ["--synthetic", "4", "--batch_size", "2", "--image_size", "128", "--relocalization_k_size", "2",
         "--ncons_kernel_sizes", "3", "3", "--ncons_channels", "16", "1", "--num_epochs", "1"]


@pytest.mark.parametrize("loss", ["weak", "strong", "warp"])
def test_cli_trains_relocalized(workdir, loss):
    import eval_pf_pascal
    import train
    from ncnet_amd.engine.checkpoint import load_checkpoint
    metrics = f"metrics_{loss}.jsonl"
    train.main(_TINY + ["--loss", loss, "--result-model-dir", f"models_{loss}", "--metrics", metrics])
    cks = sorted(glob.glob(f"models_{loss}/2*_checkpoint_adam.pth.tar"))
    assert cks
    ck = load_checkpoint(cks[0])
    assert ck["args"].relocalization_k_size == 2
    assert math.isfinite(float(ck["train_loss"][0])) and math.isfinite(float(ck["test_loss"][0]))
    if loss in ("strong", "warp"):
        recs = [json.loads(ln) for ln in Path(metrics).read_text().splitlines()]
        pcks = [r["pck"] for r in recs if "pck" in r]
        assert pcks and all(math.isfinite(p) and 0.0 <= p <= 1.0 for p in pcks)
    if loss == "weak":
        stats = eval_pf_pascal.main(["--synthetic", "2", "--image_size", "128", "--checkpoint", cks[0]])
        assert stats["point_tnf"]["pck"].shape == (2, 1)


def test_eval_picks_k_from_the_checkpoint(workdir, monkeypatch):
    import eval_pf_pascal
    import train
    from ncnet_amd.eval import point_tnf
    train.main(_TINY + ["--result-model-dir", "models_k"])
    ck = sorted(glob.glob("models_k/2*_checkpoint_adam.pth.tar"))[0]
    seen = []
    real = point_tnf.corr_to_matches

    def spy(corr4d, *a, **kw):
        seen.append((tuple(corr4d.shape[2:]), kw.get("k_size", 1), kw.get("delta4d") is not None))
        return real(corr4d, *a, **kw)

    monkeypatch.setattr(eval_pf_pascal, "corr_to_matches", spy)
    stats = eval_pf_pascal.main(["--synthetic", "2", "--image_size", "128", "--checkpoint", ck])
    assert stats["point_tnf"]["pck"].shape == (2, 1)
    assert seen and all(s == ((4, 4, 4, 4), 2, True) for s in seen)
    seen.clear()
    eval_pf_pascal.main(["--synthetic", "2", "--image_size", "128", "--checkpoint", ck, "--k_size", "0"])
    assert seen and all(s == ((8, 8, 8, 8), 1, False) for s in seen)
    # a grid the checkpoint's k does not divide is rejected up front (80 px: 5 cells)
    seen.clear()
    with pytest.raises(SystemExit, match="multiple of it"):
        eval_pf_pascal.main(["--synthetic", "2", "--image_size", "80", "--checkpoint", ck])
    assert not seen


def test_cli_rejects_a_grid_k_does_not_divide(workdir):
    import train
    with pytest.raises(SystemExit, match="multiple of K"):
        train.main(["--synthetic", "4", "--batch_size", "2", "--image_size", "72", "--relocalization_k_size", "2",
                    "--ncons_kernel_sizes", "3", "3", "--ncons_channels", "16", "1", "--num_epochs", "1",
                    "--result-model-dir", "models_bad"])
    assert not os.path.exists("models_bad")


def _hipcc():
    from ncnet_amd import kernel_resources as kr
    return shutil.which(kr.HIPCC) is not None or os.path.exists(kr.HIPCC)


def test_backward_kernel_source_declares_no_lds():
    from ncnet_amd.build import CSRC
    assert "__shared__" not in (CSRC / "corrpool_bwd.hip").read_text()


@pytest.mark.skipif(not _hipcc(), reason="hipcc not available")
def test_backward_kernel_has_no_scratch():
    from ncnet_amd import kernel_resources as kr
    from ncnet_amd.build import CSRC
    recs = kr.analyse(CSRC / "corrpool_bwd.hip")
    names = sorted(r["name"] for r in recs)
    assert names == ["corr_pool2_bwd_kernel<0>", "corr_pool2_bwd_kernel<1>"], names
    for r in recs:
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r.get("lds", 0) == 0, r
