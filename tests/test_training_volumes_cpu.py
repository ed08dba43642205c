"""ImMatchNet.training_volumes on CPU: every route of ops/correlation.py
pair_volumes (plain, fused pool, unfused pool, split operands with and
without a pool), with and without the rolled negatives, against
match_features of each single pair."""
import functools

import pytest
import torch

from ncnet_amd.ops.correlation import weak_loss_maps

B = 2
GRID = {0: 8, 2: 8, 3: 12}        # the grids of test_reloc_train_cpu.py: 8 x 8 (k = 0, 2), 12 x 12 (k = 3)


@functools.lru_cache(maxsize=None)
def _model(k):
    from ncnet_amd.models import ImMatchNet
    torch.manual_seed(0)
    return ImMatchNet(relocalization_k_size=k, use_cuda=False, ncons_kernel_sizes=[3, 3], ncons_channels=[16, 1]).eval()


def _features(grid, split):
    g = torch.Generator().manual_seed(7)
    y = torch.nn.functional.normalize(torch.randn(2 * B, grid * grid, 64, generator=g), dim=2)
    if not split:
        return y
    hi = y.to(torch.bfloat16)
    return hi, (y - hi.float()).to(torch.bfloat16)


def _image(f, n):
    """Image n of packed features (a tensor or a (hi, lo) split), batch axis kept."""
    return tuple(t[n:n + 1] for t in f) if isinstance(f, tuple) else f[n:n + 1]


def test_weak_loss_maps():
    assert weak_loss_maps(2) == ((0, 1, 1, 0), (0, 1, 0, 1))
    assert weak_loss_maps(3) == ((0, 1, 2, 1, 2, 0), (0, 1, 2, 0, 1, 2))


@pytest.mark.parametrize("split", [False, True], ids=["bf16style", "split"])
@pytest.mark.parametrize("k", [0, 2, 3])
@pytest.mark.parametrize("negatives", [False, True])
def test_volume_v_is_match_features_of_its_pair(negatives, k, split):
    m = _model(k)
    grid = GRID[k]
    hw = (grid, grid)
    f = _features(grid, split)
    amap, bmap = weak_loss_maps(B) if negatives else (tuple(range(B)), tuple(range(B)))
    out = grid // k if k > 1 else grid
    with torch.no_grad():
        vols, delta = m.training_volumes(f, hw, B, negatives, return_delta=True)
        assert vols.shape == (len(amap), 1, out, out, out, out)
        assert torch.equal(m.training_volumes(f, hw, B, negatives), vols)
        assert (delta is None) == (k <= 1)
        for v in range(len(amap)):
            want = m.match_features(_image(f, amap[v]), hw, _image(f, B + bmap[v]), hw)
            if k > 1:
                want, wd = want
                assert len(delta) == len(wd) == 4
                for d, w in zip(delta, wd):
                    assert torch.equal(d[v:v + 1].long(), w.long())
            assert (vols[v:v + 1] - want).abs().max() <= 1e-6
    # the two delegations are this entry
    with torch.no_grad():
        named = m.weak_loss_volumes_from_features(f, hw, B) if negatives else m.match_volumes_from_features(f, hw, B)
    assert torch.equal(named, vols)
