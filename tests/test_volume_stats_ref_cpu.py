"""The fp64 reference and the input families of tests/volume_stats_ref.py,
checked on the CPU against PyTorch: the GPU tests of the statistics kernels
(tests/test_gpu_volume_stats.py) rest on them."""
import pytest
import torch

from tests import volume_stats_ref as VR

# one small and one multi-tile shape of the kernel tests, plus the consumers' volume
CHECK_SHAPES = [(1, 3, 5), (2, 77, 263), (1, 70, 7500), (1, 2100, 68)]


@pytest.mark.parametrize("family", VR.FAMILIES)
@pytest.mark.parametrize("shape", CHECK_SHAPES)
def test_ref_equals_torch_max(family, shape):
    """max equals torch.max everywhere; the explicit first-argmax equals
    torch.max's index on every line whose max is unique (where no tie rule is
    involved), and holds the max on all lines."""
    x, rows, cols = VR.case(family, shape)
    for dim, st in ((2, rows), (1, cols)):
        mx, idx = torch.max(x.double(), dim=dim)
        assert torch.equal(st["max"], mx)
        unique = (x.double() == mx.unsqueeze(dim)).sum(dim) == 1
        assert torch.equal(st["arg"][unique], idx[unique])
        assert torch.equal(torch.gather(x.double(), dim, st["arg"].unsqueeze(dim)).squeeze(dim), mx)
        # first: nothing before the index holds the max
        n = x.shape[dim]
        view = [1, 1, 1]
        view[dim] = n
        before = torch.arange(n).view(view) < st["arg"].unsqueeze(dim)
        assert not ((x.double() == mx.unsqueeze(dim)) & before).any()
        assert st["sum"].dtype == torch.float64 and torch.equal(st["abs_sum"], x.double().abs().sum(dim))


@pytest.mark.parametrize("family", ["neg", "peaky", "planted"])
@pytest.mark.parametrize("shape", CHECK_SHAPES)
def test_continuous_families_are_nearly_tie_free(family, shape):
    """The continuous families test values, not the tie rule.  ('flat' is left
    out: fp32 has only ~2100 values in [5, 5.001), so its long lines do tie.)"""
    x, _, _ = VR.case(family, shape)
    assert VR.tie_share(x, 2) <= 0.01 and VR.tie_share(x, 1) <= 0.01


@pytest.mark.parametrize("family", VR.FAMILIES)
@pytest.mark.parametrize("shape", CHECK_SHAPES)
def test_ref_se_equals_softmax_max(family, shape):
    """se = sum exp(x - max) is 1 / max softmax(x), to 1e-12 in fp64."""
    x, rows, cols = VR.case(family, shape)
    for dim, st in ((2, rows), (1, cols)):
        want = 1.0 / torch.softmax(x.double(), dim=dim).max(dim=dim)[0]
        assert float(((st["se"] - want).abs() / want).max()) <= 1e-12
        assert float(st["se"].min()) >= 1.0 and float(st["se"].max()) <= x.shape[dim]


@pytest.mark.parametrize("shape", VR.SHAPES + (VR.SCORE_SHAPE, (2, 130, 1852)))
def test_ties_family_has_ties(shape):
    """At least half the rows and half the columns of 'ties' have their max
    more than once, at every shape it is used at; the constant lines are whole."""
    x, rows, cols = VR.case("ties", shape)
    V, R, C = shape
    print(f"ties {shape}: levels {VR.tie_levels(shape)}, tie share rows {VR.tie_share(x, 2):.2f} "
          f"columns {VR.tie_share(x, 1):.2f}")
    assert VR.tie_share(x, 2) >= 0.5
    assert VR.tie_share(x, 1) >= 0.5
    if R >= 8:
        assert (x[:, [1, R - 1], :] == VR.TIES_CONST).all() and (rows["arg"][:, [1, R - 1]] == 0).all()
    if C >= 8:
        assert (x[:, :, [2, C - 1]] == VR.TIES_CONST).all() and (cols["arg"][:, [2, C - 1]] == 0).all()


def test_ties_family_at_the_recorded_shape():
    """(2, 130, 1852) draws from the full 50 levels: 0.79 of the columns and
    every row tie (recorded when the family was written)."""
    shape = (2, 130, 1852)
    assert VR.tie_levels(shape) == 50
    x, _, _ = VR.case("ties", shape)
    assert VR.tie_share(x, 2) == 1.0
    assert 0.7 <= VR.tie_share(x, 1) <= 0.9


def test_neg_family_is_negative():
    for shape in VR.SHAPES:
        assert float(VR.case("neg", shape)[0].max()) <= -1.0


@pytest.mark.parametrize("shape", VR.SHAPES)
def test_planted_positions(shape):
    """Each column's argmax is its planted border row; each row's (but the
    border rows themselves) its planted border column; all border positions
    that exist are hit."""
    x, rows, cols = VR.case("planted", shape)
    V, R, C = shape
    carg, own, rarg = VR.planted_expect(shape)
    for v in range(V):
        assert torch.equal(cols["arg"][v], carg)
        assert torch.equal(rows["arg"][v][own], rarg[own])
    assert set(cols["arg"].unique().tolist()) == set(VR.border_positions(R)[:C])
    if own.sum() >= len(VR.border_positions(C)):
        assert set(rows["arg"][:, own].unique().tolist()) == set(VR.border_positions(C))
    assert VR.tie_share(x, 1) == 0.0 and VR.tie_share(x, 2) == 0.0


def test_consumer_volumes_have_unique_maxima():
    """The weak-loss and match-extraction comparisons go against autograd of
    max and torch.max, whose tie rule is not pinned down: no line may tie."""
    for x in (VR.weak_volume("tie_free"), VR.weak_volume("neg")):
        V, _, i, j, k, l = x.shape
        m = x.view(V, i * j, k * l)
        assert VR.tie_share(m, 1) == 0.0 and VR.tie_share(m, 2) == 0.0
    assert float(VR.weak_volume("neg").max()) <= -1.0
    x = VR.inloc_volume()
    assert x.unique().numel() == x.numel()
