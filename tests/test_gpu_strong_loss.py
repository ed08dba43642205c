"""The fused HIP keypoint-supervised loss (csrc/kploss.hip) against the fp64
oracle (ops/reference.py keypoint_ce), and the model / Trainer path over it
(run on an MI355X).

Bounds: loss within 1e-5 max(1, |loss|), gradient relative error (max norm)
below 1e-4 -- what test_gpu_kernels.py::test_weak_loss_scores holds the other
fp32 exp-sum kernels to; the fp32 evaluation of these formulas sits ~50x inside.
"""
import pytest
import torch

from ncnet_amd.ops import _ext
from ncnet_amd.ops import reference as ref
from ncnet_amd.ops.loss import strong_loss_from_corr
from tests.strong_loss_cases import CASES, learning_setup, make_case, run_learning

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIELDS = ("source_points", "target_points", "source_im_size", "target_im_size")


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


_ORACLE: dict = {}


def oracle(name):
    """fp64 loss and gradient of a case on the CPU, computed once and shared."""
    if name not in _ORACLE:
        x, kp = make_case(name)
        xd = x.double().requires_grad_(True)
        loss = ref.keypoint_ce(xd, *kp)
        loss.backward()
        _ORACLE[name] = (float(loss.detach()), xd.grad.detach())
    return _ORACLE[name]


def gpu_case(name):
    x, kp = make_case(name, DEV)
    return x.requires_grad_(True), dict(zip(FIELDS, kp))


@pytest.mark.parametrize("name", list(CASES))
def test_loss_and_gradient_match_fp64_oracle(name):
    lr, gr = oracle(name)
    x, batch = gpu_case(name)
    n0 = _ext.DISPATCH["kploss"]
    loss = strong_loss_from_corr(x, batch)
    loss.backward()
    assert _ext.DISPATCH["kploss"] == n0 + 1
    loss = float(loss.detach())
    le, ge = abs(loss - lr), relerr(x.grad, gr)
    print(f"{name}: loss {loss:.7f} oracle {lr:.7f} |diff| {le:.3e}; gradient rel {ge:.3e}")
    assert le < 1e-5 * max(1.0, abs(lr))
    assert ge < 1e-4
    # zero exactly where no keypoint touches the row or the column
    assert torch.equal(x.grad.cpu() == 0, gr == 0)


def test_upstream_gradient_scales_in_the_kernel():
    lr, gr = oracle("edge")
    x, batch = gpu_case("edge")
    (3 * strong_loss_from_corr(x, batch)).backward()
    assert relerr(x.grad, 3 * gr) < 1e-4


def test_all_invalid_batch_is_exactly_zero():
    x, batch = gpu_case("small")
    batch["source_points"] = torch.full_like(batch["source_points"], -1.0)
    batch["target_points"] = torch.full_like(batch["target_points"], -1.0)
    loss = strong_loss_from_corr(x, batch)
    loss.backward()
    assert float(loss.detach()) == 0.0 and torch.count_nonzero(x.grad) == 0


@pytest.mark.parametrize("name", ["edge", "train"])
def test_backward_writes_every_element(name):
    """The backward binding on a NaN-prefilled gx: no NaN left, exactly 0 where the oracle is 0."""
    _, gr = oracle(name)
    x, batch = gpu_case(name)
    x = x.detach()
    (B, N, hA, wA, hB, wB) = CASES[name][0]
    x3 = x.reshape(B, hA * wA, hB * wB).contiguous()
    i32 = dict(dtype=torch.int32, device=DEV)
    f32 = dict(dtype=torch.float32, device=DEV)
    cells, wts, valid = torch.empty((B, N, 8), **i32), torch.empty((B, N, 8), **f32), torch.empty((B, N), **i32)
    lse, term, out = torch.empty((B, N, 2), **f32), torch.empty((B, N, 2), **f32), torch.empty(2, **f32)
    C = _ext.ext()
    C.kploss_fwd(x3, *(batch[k] for k in FIELDS), hA, wA, hB, wB, cells, wts, valid, lse, term, out)
    gx = torch.full_like(x3, float("nan"))
    C.kploss_bwd(x3, cells, wts, valid, lse, out[1:], gx)
    assert not torch.isnan(gx).any()
    assert torch.equal(gx.cpu().reshape(gr.shape) == 0, gr == 0)
    assert relerr(gx.reshape(gr.shape), gr) < 1e-4
    # the saved table: cells in range, weights of a valid keypoint sum to 1 per grid
    assert int(cells[..., :4].min()) >= 0 and int(cells[..., :4].max()) < hA * wA
    assert int(cells[..., 4:].min()) >= 0 and int(cells[..., 4:].max()) < hB * wB
    assert torch.equal(valid.bool().cpu(), ref.keypoint_valid(batch["source_points"], batch["target_points"]).cpu())
    v = valid.bool()
    assert torch.allclose(wts[..., :4].sum(-1)[v], torch.ones((), device=DEV), atol=1e-6)
    assert torch.allclose(wts[..., 4:].sum(-1)[v], torch.ones((), device=DEV), atol=1e-6)


def test_binding_rejects_bad_arguments():
    x, batch = gpu_case("small")
    big = {k: v for k, v in batch.items()}
    big["source_points"] = torch.ones(2, 2, 65, device=DEV)
    big["target_points"] = torch.ones(2, 2, 65, device=DEV)
    with pytest.raises(ValueError):
        strong_loss_from_corr(x, big)
    (B, N, hA, wA, hB, wB) = CASES["small"][0]
    x3 = x.detach().reshape(B, hA * wA, hB * wB)
    f32 = dict(dtype=torch.float32, device=DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    args = [torch.empty((B, N, 8), **i32), torch.empty((B, N, 8), **f32), torch.empty((B, N), **i32),
            torch.empty((B, N, 2), **f32), torch.empty((B, N, 2), **f32), torch.empty(2, **f32)]
    with pytest.raises(RuntimeError):      # grid does not match the volume
        _ext.ext().kploss_fwd(x3, *(batch[k] for k in FIELDS), hA, wA + 1, hB, wB, *args)
    with pytest.raises(RuntimeError):      # more than 64 keypoints
        _ext.ext().kploss_fwd(x3, big["source_points"], big["target_points"], batch["source_im_size"],
                              batch["target_im_size"], hA, wA, hB, wB, *args)


def test_two_calls_are_bit_identical():
    out = []
    for _ in range(2):
        x, batch = gpu_case("train")
        loss = strong_loss_from_corr(x, batch)
        loss.backward()
        out.append((loss.detach().reshape(1).view(torch.int32), x.grad.view(torch.int32)))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.fixture(scope="module")
def model_and_batch():
    from ncnet_amd.data.datasets import synthetic_correspondence_batch
    from ncnet_amd.models import ImMatchNet
    torch.manual_seed(0)
    model = ImMatchNet(ncons_kernel_sizes=[5, 5, 5], ncons_channels=[16, 16, 1]).to(DEV)
    return model, synthetic_correspondence_batch(2, 240, device=DEV, seed=11)


def test_model_strong_loss_matches_oracle_on_its_volume(model_and_batch):
    from ncnet_amd.engine.trainer import strong_loss
    model, batch = model_and_batch
    model.train()
    loss = strong_loss(model, batch).detach()
    with torch.no_grad():
        f, hw = model.extract(torch.cat((batch["source_image"], batch["target_image"]), 0))
        vol = model.match_volumes_from_features(f, hw, 2)
    assert vol.shape == (2, 1, 15, 15, 15, 15)
    want = float(ref.keypoint_ce(vol.double().cpu(), *(batch[k].double().cpu() for k in FIELDS)))
    print(f"model: strong_loss {float(loss):.7f} oracle on the no-grad volume {want:.7f}")
    assert abs(float(loss) - want) < 1e-5 * max(1.0, abs(want))


def test_trainer_strong_step(model_and_batch):
    from ncnet_amd.engine.trainer import Trainer, make_adam
    from ncnet_amd.parallel.dist import DistContext
    model, batch = model_and_batch
    model.train()
    params = [p for p in model.parameters() if p.requires_grad]
    before = [p.detach().clone() for p in model.NeighConsensus.parameters()]
    tr = Trainer(model, make_adam(params, 1e-3), DistContext(device=torch.device(DEV, 0)), loss="strong")
    n0, f0 = _ext.DISPATCH["kploss"], _ext.DISPATCH["torch_fallback"]
    loss = tr.train_step(batch)
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and _ext.DISPATCH["kploss"] == n0 + 1 and _ext.DISPATCH["torch_fallback"] == f0
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
    """tests/test_strong_loss_cpu.py::test_learning_cpu through the HIP
    NeighConsensus + MutualMatching + loss path, with the same bar."""
    n0, f0 = _ext.DISPATCH["kploss"], _ext.DISPATCH["torch_fallback"]
    first, last = run_learning(*learning_setup(DEV))
    print(f"learning (gpu): {first:.4f} -> {last:.4f}")
    assert _ext.DISPATCH["kploss"] == n0 + 40 and _ext.DISPATCH["torch_fallback"] == f0
    assert last < 0.5 * first
