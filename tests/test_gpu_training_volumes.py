"""ImMatchNet.training_volumes on the GPU: the same kernels, operands and
launch counters as the ops called by hand with explicit pair maps (run on an
MI355X)."""
import pytest
import torch

from ncnet_amd.ops import _ext

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, GRID, CH = 2, 8, 64


@pytest.fixture(scope="module")
def model():
    from ncnet_amd.models import ImMatchNet
    torch.manual_seed(0)
    return ImMatchNet(ncons_kernel_sizes=[5, 5, 5], ncons_channels=[16, 16, 1]).to(DEV).train()


def _counted(fn):
    n0 = dict(_ext.DISPATCH)
    out = fn()
    torch.cuda.synchronize()
    return out, {k: v - n0.get(k, 0) for k, v in _ext.DISPATCH.items() if v != n0.get(k, 0)}


@pytest.mark.parametrize("negatives", [False, True])
@pytest.mark.parametrize("k", [0, 2])
def test_training_volumes_are_the_ops_by_hand(model, k, negatives):
    from ncnet_amd.ops.correlation import correlation, correlation_pool2
    g = torch.Generator().manual_seed(3)
    f = torch.nn.functional.normalize(torch.randn(2 * B, GRID * GRID, CH, generator=g), dim=2).to(DEV, torch.bfloat16)
    fa, fb = f[:B], f[B:]
    amap, bmap = ([0, 1, 1, 0], [0, 1, 0, 1]) if negatives else ([0, 1], [0, 1])

    def by_hand():
        if k == 2:
            corr, delta = correlation_pool2(fa, fb, GRID, GRID, GRID, GRID, amap=amap, bmap=bmap)
        else:
            am = torch.tensor(amap, dtype=torch.int32, device=DEV)
            bm = torch.tensor(bmap, dtype=torch.int32, device=DEV)
            corr, delta = correlation(fa, fb, am, bm).view(len(amap), 1, GRID, GRID, GRID, GRID), None
        return model.process_correlation(corr), delta

    model.relocalization_k_size = k
    try:
        (want, wdelta), want_counts = _counted(by_hand)
        (got, delta), counts = _counted(lambda: model.training_volumes(f, (GRID, GRID), B, negatives, return_delta=True))
    finally:
        model.relocalization_k_size = 0
    out = GRID // 2 if k == 2 else GRID
    assert got.shape == (len(amap), 1, out, out, out, out) and got.requires_grad
    assert torch.isfinite(got).all() and float(got.abs().max()) > 0
    assert torch.equal(got, want)
    assert (delta is None) == (wdelta is None) == (k == 0)
    if k == 2:
        for d, w in zip(delta, wdelta):
            assert torch.equal(d, w)
    assert counts == want_counts
    assert counts.get("torch_fallback", 0) == 0
