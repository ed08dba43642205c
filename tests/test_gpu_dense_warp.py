"""The fused HIP dense correspondence loss (csrc/densece.hip) against the fp64
oracle (ops/reference.py dense_ce / dense_targets), the two-view input path on
the GPU, and the model / Trainer / train.py path over them (run on an MI355X).

Bounds: the strong loss's own (tests/test_gpu_strong_loss.py): loss within
1e-5 max(1, |loss|), gradient relative error (max norm) below 1e-4.
"""
import math
import sys

import pytest
import torch

from ncnet_amd.data.augment import PairAugment
from ncnet_amd.ops import _ext
from ncnet_amd.ops import reference as ref
from ncnet_amd.ops.loss import warp_loss_from_corr
from tests.dense_warp_cases import (CASES, dense_weight_maps, learning_setup, make_case, out_of_frame_maps,
                                    run_learning)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


_ORACLE: dict = {}


def oracle(name):
    """fp64 loss, gradient and target table of a case on the CPU, computed once and shared."""
    if name not in _ORACLE:
        x, maps = make_case(name)
        xd = x.double().requires_grad_(True)
        loss = ref.dense_ce(xd, maps)
        loss.backward()
        _ORACLE[name] = (float(loss.detach()), xd.grad.detach(), ref.dense_targets(maps, *CASES[name][1:]))
    return _ORACLE[name]


def gpu_case(name):
    x, maps = make_case(name, DEV)
    return x.requires_grad_(True), {"warp_maps": maps}


def _buffers(B, R, C):
    n = max(R, C)
    i32 = dict(dtype=torch.int32, device=DEV)
    f32 = dict(dtype=torch.float32, device=DEV)
    return {"cells": torch.full((B, 2, 4, n), -7, **i32), "wts": torch.full((B, 2, 4, n), float("nan"), **f32),
            "valid": torch.full((B, 2, n), -7, **i32), "lse": torch.empty((B, 2, n), **f32),
            "term": torch.empty((B, 2, n), **f32), "out": torch.empty(3, **f32)}


def _forward(x3, maps, grid):
    """The four forward launches of ops/loss.py DenseCEFn on explicit buffers."""
    from ncnet_amd.ops.loss import _row_col_stats
    C = _ext.ext()
    o = _buffers(*x3.shape)
    C.densece_table(maps, *grid, o["cells"], o["wts"], o["valid"])
    rmax, _, rse, cmax, _, cse = _row_col_stats(x3, 1)
    C.densece_fwd(x3, o["cells"], o["wts"], o["valid"], rmax, rse, cmax, cse, o["lse"], o["term"])
    C.densece_reduce(o["term"], o["valid"], o["out"])
    return o


@pytest.mark.parametrize("name", list(CASES))
def test_loss_and_gradient_match_fp64_oracle(name):
    lr, gr, _ = oracle(name)
    x, batch = gpu_case(name)
    n0, f0 = _ext.DISPATCH["densece"], _ext.DISPATCH["torch_fallback"]
    loss = warp_loss_from_corr(x, batch)
    loss.backward()
    assert _ext.DISPATCH["densece"] == n0 + 1 and _ext.DISPATCH["torch_fallback"] == f0
    loss = float(loss.detach())
    le, ge = abs(loss - lr), relerr(x.grad, gr)
    print(f"{name}: loss {loss:.7f} oracle {lr:.7f} |diff| {le:.3e}; gradient rel {ge:.3e}")
    assert le < 1e-5 * max(1.0, abs(lr))
    assert ge < 1e-4
    # zero exactly where neither the row nor the column is valid
    assert torch.equal(x.grad.cpu() == 0, gr == 0)


@pytest.mark.parametrize("name", list(CASES))
def test_table_matches_dense_targets(name):
    """The kernel's table, scattered into dense weight maps, against the fp64
    table (functionally: (i0, f ~ 1) and (i0 + 1, f ~ 0) are the same target),
    and its valid flags against the oracle's; everything past a side's cell
    count and every invalid cell is zero."""
    B, hA, wA, hB, wB = CASES[name]
    R, C = hA * wA, hB * wB
    ca, wa, oka, cb, wb, okb = oracle(name)[2]
    x, batch = gpu_case(name)
    o = _forward(x.detach().reshape(B, R, C).contiguous(), batch["warp_maps"], (hA, wA, hB, wB))
    cells, wts, valid = o["cells"].cpu(), o["wts"].cpu(), o["valid"].cpu()
    for side, (ns, no, c_ref, w_ref, ok_ref) in enumerate(((R, C, ca, wa, oka), (C, R, cb, wb, okb))):
        assert torch.equal(valid[:, side, :ns].bool(), ok_ref), (name, side)
        assert int(valid[:, side, ns:].abs().sum()) == 0 and int(cells[:, side, :, ns:].abs().sum()) == 0
        assert float(wts[:, side, :, ns:].abs().sum()) == 0.0
        c, w = cells[:, side, :, :ns].permute(0, 2, 1), wts[:, side, :, :ns].permute(0, 2, 1)
        assert int(c.min()) >= 0 and int(c.max()) < no
        dead = ~ok_ref
        assert int(c[dead].abs().sum()) == 0 and float(w[dead].abs().sum()) == 0.0
        err = float((dense_weight_maps(c, w, no) - dense_weight_maps(c_ref, w_ref, no)).abs().max())
        print(f"{name} side {side}: dense weight maps max |kernel - fp64| {err:.3e}")
        assert err < 1e-6


def test_upstream_gradient_scales_in_the_kernel():
    _, gr, _ = oracle("odd")
    x, batch = gpu_case("odd")
    (3 * warp_loss_from_corr(x, batch)).backward()
    assert relerr(x.grad, 3 * gr) < 1e-4


@pytest.mark.parametrize("name", ["odd", "train"])
def test_backward_writes_every_element(name):
    """The backward binding on a NaN-prefilled gx: no NaN left, exactly 0 where
    the oracle is 0; also on a volume that starts 4 bytes off a 16-byte boundary
    (the scalar kernel), with the same values."""
    _, gr, _ = oracle(name)
    B, hA, wA, hB, wB = CASES[name]
    R, C = hA * wA, hB * wB
    x, batch = gpu_case(name)
    x3 = x.detach().reshape(B, R, C).contiguous()
    o = _forward(x3, batch["warp_maps"], (hA, wA, hB, wB))
    gx = torch.full_like(x3, float("nan"))
    _ext.ext().densece_bwd(x3, o["cells"], o["wts"], o["lse"], o["out"], gx)
    assert not torch.isnan(gx).any()
    assert torch.equal(gx.cpu().reshape(gr.shape) == 0, gr == 0)
    assert relerr(gx.reshape(gr.shape), gr) < 1e-4
    xo = torch.empty(x3.numel() + 1, device=DEV)[1:].view_as(x3).copy_(x3)
    go = torch.full((x3.numel() + 1,), float("nan"), device=DEV)[1:].view_as(x3)
    assert xo.data_ptr() % 16 == 4 and go.data_ptr() % 16 == 4
    _ext.ext().densece_bwd(xo, o["cells"], o["wts"], o["lse"], o["out"], go)
    assert not torch.isnan(go).any() and torch.equal(go == 0, gx == 0)
    assert relerr(go, gx) < 1e-6


def test_all_invalid_batch_is_exactly_zero():
    x, _ = gpu_case("small")
    loss = warp_loss_from_corr(x, {"warp_maps": out_of_frame_maps(x.shape[0]).to(DEV)})
    loss.backward()
    assert float(loss.detach()) == 0.0 and torch.count_nonzero(x.grad) == 0


def test_two_calls_are_bit_identical():
    out = []
    for _ in range(2):
        x, batch = gpu_case("train")
        loss = warp_loss_from_corr(x, batch)
        loss.backward()
        out.append((loss.detach().reshape(1).view(torch.int32), x.grad.view(torch.int32)))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_swapping_the_rows_of_one_image_changes_the_loss():
    """Mutation check: the A and B rows of warp_maps are not interchangeable."""
    lr, _, _ = oracle("small")
    x, batch = gpu_case("small")
    maps = batch["warp_maps"].clone()
    maps[0] = maps[0].flip(0)
    with torch.no_grad():
        good = float(warp_loss_from_corr(x, batch))
        bad = float(warp_loss_from_corr(x, {"warp_maps": maps}))
    want = float(ref.dense_ce(x.detach().double().cpu(), maps.cpu()))
    print(f"loss {good:.6f}, rows of image 0 swapped {bad:.6f} (oracle {want:.6f})")
    assert abs(bad - lr) > 100 * 1e-5 * max(1.0, abs(lr))
    assert abs(bad - want) < 1e-5 * max(1.0, abs(want))


def test_binding_rejects_bad_arguments():
    B, hA, wA, hB, wB = CASES["small"]
    R, C = hA * wA, hB * wB
    x, batch = gpu_case("small")
    maps = batch["warp_maps"]
    x3 = x.detach().reshape(B, R, C).contiguous()
    E = _ext.ext()
    o = _forward(x3, maps, (hA, wA, hB, wB))
    tab = (o["cells"], o["wts"], o["valid"])
    for bad in (maps.float(), maps.cpu(), maps[:, :1].contiguous(), maps[:, :, :11].contiguous(), maps.view(-1)):
        with pytest.raises(RuntimeError):
            E.densece_table(bad, hA, wA, hB, wB, *tab)
    with pytest.raises(RuntimeError):                      # the grid does not match the table
        E.densece_table(maps, hA, wA + 2, hB, wB, *tab)
    with pytest.raises(RuntimeError):
        E.densece_table(maps, 0, wA, hB, wB, *tab)
    with pytest.raises(RuntimeError):
        E.densece_table(maps, hA, wA, hB, wB, o["cells"].float(), o["wts"], o["valid"])
    with pytest.raises(RuntimeError):
        E.densece_table(maps, hA, wA, hB, wB, o["cells"], o["wts"], o["valid"][:, :, :-1].contiguous())
    from ncnet_amd.ops.loss import _row_col_stats
    rmax, _, rse, cmax, _, cse = _row_col_stats(x3, 1)
    with pytest.raises(RuntimeError):                      # row statistics in the column slots
        E.densece_fwd(x3, *tab, cmax, cse, rmax, rse, o["lse"], o["term"])
    with pytest.raises(RuntimeError):
        E.densece_fwd(x3.double(), *tab, rmax, rse, cmax, cse, o["lse"], o["term"])
    with pytest.raises(RuntimeError):
        E.densece_fwd(x3.cpu(), *tab, rmax, rse, cmax, cse, o["lse"], o["term"])
    with pytest.raises(RuntimeError):
        E.densece_reduce(o["term"], o["valid"], torch.empty(2, device=DEV))
    with pytest.raises(RuntimeError):
        E.densece_reduce(o["term"], o["valid"].float(), o["out"])
    gx = torch.empty_like(x3)
    with pytest.raises(RuntimeError):
        E.densece_bwd(x3, *tab[:2], o["lse"], o["out"][1:], gx)
    with pytest.raises(RuntimeError):
        E.densece_bwd(x3, *tab[:2], o["lse"], o["out"], gx[:, :-1].contiguous())
    with pytest.raises(RuntimeError):
        E.densece_bwd(x3, *tab[:2], o["lse"], o["out"], gx.cpu())
    with pytest.raises(RuntimeError):
        E.densece_bwd(x3, *tab[:2], o["lse"], o["out"], gx, torch.ones(2, device=DEV))
    with pytest.raises(KeyError):
        warp_loss_from_corr(x, {})
    with pytest.raises(ValueError):
        warp_loss_from_corr(x[:, 0], batch)
    torch.cuda.synchronize()


def _image_batch(n, hw, seed=0):
    from ncnet_amd.data.datasets import SyntheticImageDataset, collate_uint8_images
    ds = SyntheticImageDataset(n, hw, seed=seed)
    return collate_uint8_images([ds[i] for i in range(n)])


def test_gpu_view_batch_equals_cpu_fallback(monkeypatch):
    from ncnet_amd.data.datasets import gpu_view_batch
    batch = _image_batch(3, (37, 45))
    aug = PairAugment()
    before = _ext.DISPATCH["torch_fallback"]
    tables = []
    real = _ext.ext().warp_norm_u8
    monkeypatch.setattr(_ext.ext(), "warp_norm_u8", lambda *a: (tables.append(a[1].cpu()), real(*a))[1])
    got = gpu_view_batch(batch, DEV, 19, 23, aug, torch.Generator().manual_seed(9), with_points=True)
    # one launch over the 2B views, both views of an image on the same bytes, offsets non-decreasing
    # (the kernel's contract: its bounds-checked build asserts it)
    assert len(tables) == 1 and tables[0].shape == (6, 3)
    assert torch.equal(tables[0][0::2], batch["pixel_meta"]) and torch.equal(tables[0][1::2], batch["pixel_meta"])
    assert bool((tables[0][1:, 0] >= tables[0][:-1, 0]).all())
    want = gpu_view_batch(batch, "cpu", 19, 23, aug, torch.Generator().manual_seed(9), with_points=True)
    assert _ext.DISPATCH["torch_fallback"] == before
    assert set(got) == set(want)
    for k in ("source_image", "target_image"):
        assert got[k].is_cuda and got[k].dtype == torch.float32 and got[k].shape == (3, 3, 19, 23)
        err = float((got[k].cpu() - want[k]).abs().max())
        print(f"view batch {k}: max |gpu - cpu| {err:.3e} (bound 1e-4)")
        assert err < 1e-4
    for k in ("warp_maps", "source_points", "target_points", "source_im_size", "target_im_size", "L_pck"):
        assert got[k].is_cuda and torch.equal(got[k].cpu(), want[k]), k
    assert got["warp_maps"].dtype == torch.float64


@pytest.fixture(scope="module")
def model_and_batch():
    from ncnet_amd.data.datasets import gpu_view_batch
    from ncnet_amd.models import ImMatchNet
    torch.manual_seed(0)
    model = ImMatchNet(ncons_kernel_sizes=[5, 5, 5], ncons_channels=[16, 16, 1]).to(DEV)
    batch = gpu_view_batch(_image_batch(2, (200, 260), seed=3), DEV, 240, 240, PairAugment(),
                           torch.Generator().manual_seed(11), with_points=True)
    return model, batch


def test_trainer_warp_step_matches_oracle_on_its_volume(model_and_batch):
    from ncnet_amd.engine.trainer import Trainer, make_adam, warp_loss
    from ncnet_amd.parallel.dist import DistContext
    model, batch = model_and_batch
    model.train()
    with torch.no_grad():
        loss = warp_loss(model, batch)
        f, hw = model.extract(torch.cat((batch["source_image"], batch["target_image"]), 0))
        vol = model.match_volumes_from_features(f, hw, 2)
    assert vol.shape == (2, 1, 15, 15, 15, 15)
    want = float(ref.dense_ce(vol.double().cpu(), batch["warp_maps"].cpu()))
    print(f"model: warp_loss {float(loss):.7f} oracle on the no-grad volume {want:.7f}")
    assert abs(float(loss) - want) < 1e-5 * max(1.0, abs(want))
    params = [p for p in model.parameters() if p.requires_grad]
    before = [p.detach().clone() for p in model.NeighConsensus.parameters()]
    tr = Trainer(model, make_adam(params, 1e-3), DistContext(device=torch.device(DEV, 0)), loss="warp")
    n0, f0 = _ext.DISPATCH["densece"], _ext.DISPATCH["torch_fallback"]
    step = tr.train_step(batch)
    torch.cuda.synchronize()
    # the step's loss is the loss of the volume before the update
    assert abs(float(step) - want) < 1e-5 * max(1.0, abs(want))
    assert _ext.DISPATCH["densece"] == n0 + 1 and _ext.DISPATCH["torch_fallback"] == f0
    after = list(model.NeighConsensus.parameters())
    assert all(torch.isfinite(p).all() for p in after)
    assert any(not torch.equal(a, b) for a, b in zip(after, before))
    # the evaluation step: the loss and the PCK of the same volume
    model.eval()
    ev = tr.eval_step(batch)
    assert torch.isfinite(ev) and _ext.DISPATCH["torch_fallback"] == f0
    pck = tr._pck[-1]
    assert pck.shape == (2,) and bool(((pck >= 0) & (pck <= 1)).all())


def test_learning_gpu():
    """tests/test_dense_warp_cpu.py::test_learning_cpu through the HIP
    NeighConsensus + MutualMatching + loss path, with the same bar."""
    n0, f0 = _ext.DISPATCH["densece"], _ext.DISPATCH["torch_fallback"]
    first, last = run_learning(*learning_setup(DEV, seed=1))
    print(f"learning (gpu): {first:.4f} -> {last:.4f}")
    assert _ext.DISPATCH["densece"] == n0 + 40 and _ext.DISPATCH["torch_fallback"] == f0
    assert last < 0.5 * first


def test_train_cli_warp_gpu(monkeypatch, capfd):
    """Three steps of train.py --loss warp --synthetic 8 --batch_size 2: one
    warp_norm_u8 launch over the 2B views per training batch (one batch of
    lookahead), the loss on the HIP kernels, nothing falls back to torch.
    (capfd, not capsys: the bounds-checked build's fixture in conftest.py holds
    capfd, and the output read here is written back for it.)"""
    import train
    assert _ext.available()
    launches = []
    real = _ext.ext().warp_norm_u8
    monkeypatch.setattr(_ext.ext(), "warp_norm_u8", lambda *a: (launches.append(a[2].shape), real(*a))[1])
    n0, f0 = _ext.DISPATCH["densece"], _ext.DISPATCH["torch_fallback"]
    train.main(["--loss", "warp", "--synthetic", "8", "--batch_size", "2", "--image_size", "240", "--max_steps", "3",
                "--num_workers", "0"])
    torch.cuda.synchronize()
    out, err = capfd.readouterr()
    sys.stdout.write(out)
    sys.stderr.write(err)
    losses = [float(ln.split()[3]) for ln in out.splitlines() if ln.startswith("step ")]
    assert len(losses) == 3 and all(math.isfinite(v) and 0 < v < 1e6 for v in losses), out
    assert launches == [torch.Size([4, 8])] * 3
    assert _ext.DISPATCH["densece"] == n0 + 3 and _ext.DISPATCH["torch_fallback"] == f0
