"""The volume statistics kernels (csrc/volume.hip: stats_rows, stats_cols and
the one-pass stats2d) and their consumers against references that do not come
from the kernels: the fp64 statistics of tests/volume_stats_ref.py (whole
lines, explicit first-argmax), autograd of the fp64 weak-loss oracle, and the
torch.softmax / torch.max branch of the match extraction on a CPU copy.

Bounds: max bit-equal to the reference cast to fp32; first argmax equal;
sum exp(x - max) within 1e-5 relative (the bound of the project's other fp32
exp-sum kernels; a plain fp32 torch.exp(x - max).sum() is at 1.4e-7 .. 2.3e-7
on these inputs, so the kernels' evaluation order and __expf get ~50 x that);
the plain sum within 1e-5 * sum |x| (plain fp32: 2e-7).

Observed on an MI355X (the largest over all shapes, both paths and the
sub-tile settings; each test prints its own figures):

    family    se rel. error    sum error / sum |x|
    ties      3.7e-7           2.5e-7
    neg       2.8e-7           2.8e-7
    peaky     2.7e-7           1.1e-7
    flat      2.3e-7           2.2e-7
    planted   4.0e-7           2.9e-7
"""
import pytest
import torch

from ncnet_amd.ops import _ext
from ncnet_amd.ops import reference as ref
from tests import volume_stats_ref as VR

pytestmark = pytest.mark.gpu
DEV = "cuda"
SE_RTOL = 1e-5
SUM_RTOL = 1e-5


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _outputs(V, R, C):
    """Prefilled so that an element no kernel wrote shows: NaN floats, -7 indices."""
    f = dict(dtype=torch.float32, device=DEV)
    nan = float("nan")
    return {"rmx": torch.full((V, R), nan, **f), "rse": torch.full((V, R), nan, **f),
            "cmx": torch.full((V, C), nan, **f), "cse": torch.full((V, C), nan, **f),
            "rarg": torch.full((V, R), -7, dtype=torch.int32, device=DEV),
            "carg": torch.full((V, C), -7, dtype=torch.int32, device=DEV)}


def _run(path: str, x, sum_kind: int):
    o = _outputs(*x.shape)
    E = _ext.ext()
    if path == "stats2d":
        assert E.stats2d(x, o["rmx"], o["rarg"], o["rse"], o["cmx"], o["carg"], o["cse"], sum_kind)
    else:
        E.stats_rows(x, o["rmx"], o["rarg"], o["rse"] if sum_kind else None, sum_kind)
        E.stats_cols(x, o["cmx"], o["carg"], o["cse"] if sum_kind else None, sum_kind)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


def _check(tag: str, got, rows, cols, sum_kind: int):
    """One path's six outputs against the fp64 reference -> (se error, sum error)."""
    worst = [0.0, 0.0]
    for d, st in (("r", rows), ("c", cols)):
        mx, arg, s = got[d + "mx"], got[d + "arg"], got[d + "se"]
        assert torch.equal(mx, st["max"].float()), (tag, d, "max")
        assert torch.equal(arg.long(), st["arg"]), (tag, d, "argmax",
                                                    int((arg.long() != st["arg"]).sum()), "lines differ")
        if sum_kind == 0:
            assert torch.isnan(s).all(), (tag, d, "sum written without a sum kind")
        elif sum_kind == 1:
            err = float(((s.double() - st["se"]).abs() / st["se"]).max())
            print(f"{tag} {d} se relerr {err:.3e}")
            worst[0] = max(worst[0], err)
            assert torch.isfinite(s).all() and err <= SE_RTOL, (tag, d, "se", err)
        else:
            err = float(((s.double() - st["sum"]).abs() / st["abs_sum"]).max())
            print(f"{tag} {d} sum err / abs_sum {err:.3e}")
            worst[1] = max(worst[1], err)
            assert torch.isfinite(s).all() and err <= SUM_RTOL, (tag, d, "sum", err)
    return worst


OBSERVED: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for fam, (a, b) in sorted(OBSERVED.items()):
        print(f"\nobserved max [{fam}]: se relerr {a:.3e}, sum err / abs_sum {b:.3e}")


def _note(family, worst):
    o = OBSERVED.setdefault(family, [0.0, 0.0])
    o[0], o[1] = max(o[0], worst[0]), max(o[1], worst[1])


@pytest.mark.parametrize("sum_kind", [0, 1, 2])
@pytest.mark.parametrize("family", VR.FAMILIES)
@pytest.mark.parametrize("shape", VR.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stats_kernels_vs_fp64(shape, family, sum_kind):
    """stats_rows + stats_cols and stats2d, each against the fp64 reference."""
    xc, rows, cols = VR.case(family, shape)
    x = xc.to(DEV)
    for path in ("rows_cols", "stats2d"):
        _note(family, _check(f"{family} {shape} {path}", _run(path, x, sum_kind), rows, cols, sum_kind))
    assert torch.equal(x.cpu(), xc)                       # the input is read only


@pytest.mark.parametrize("sum_kind", [0, 1, 2])
@pytest.mark.parametrize("family", VR.FAMILIES)
@pytest.mark.parametrize("rt", [1, 4])
@pytest.mark.parametrize("shape", VR.SUBTILE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stats2d_subtiles_vs_fp64(shape, rt, family, sum_kind, tune):
    """stats2d_tile<*, *, RT> at 1 and 4 sub-tiles of 64 rows per block (the
    default, 2, is in test_stats_kernels_vs_fp64): R = 1030 leaves the last
    block with 6 rows of its first sub-tile."""
    tune("s2d_rt", rt)
    xc, rows, cols = VR.case(family, shape)
    _note(family, _check(f"{family} {shape} stats2d rt={rt}", _run("stats2d", xc.to(DEV), sum_kind), rows, cols,
                         sum_kind))


def test_planted_maxima_sit_on_the_borders():
    """The 'planted' argmax of the kernels is the planted position itself (not
    only equal to the reference's): first / last index and both sides of the
    64 and 256 borders."""
    shape = (2, 77, 263)
    xc, _, _ = VR.case("planted", shape)
    carg, own, rarg = VR.planted_expect(shape)
    for path in ("rows_cols", "stats2d"):
        got = _run(path, xc.to(DEV), 0)
        for v in range(shape[0]):
            assert torch.equal(got["carg"][v].long(), carg), path
            assert torch.equal(got["rarg"][v].long()[own], rarg[own]), path


# ---------------------------------------------------------------------------
# consumers
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("norm", [0, 1, 2])
@pytest.mark.parametrize("family", ["neg", "flat"])
def test_score_sum_vs_fp64(family, norm):
    """The weak-loss score value (the production statistics + score_sum) with
    the expected value from the fp64 reference statistics."""
    from ncnet_amd.ops import loss as L
    xc, rows, cols = VR.case(family, VR.SCORE_SHAPE)
    g = torch.Generator().manual_seed(17 + norm)
    wr, wc = torch.randn(VR.SCORE_SHAPE[0], generator=g), torch.randn(VR.SCORE_SHAPE[0], generator=g)
    rmax, _, rse, cmax, _, cse = L._row_col_stats(xc.to(DEV), norm)
    val = torch.full((), float("nan"), device=DEV)
    _ext.ext().score_sum(rmax, rse, cmax, cse, wr.to(DEV), wc.to(DEV), val, norm, ref.L1_EPS)

    def sc(st):
        return 1.0 / st["se"] if norm == 1 else st["max"] / (st["sum"] + ref.L1_EPS) if norm == 2 else st["max"]
    want = float((wr.double().view(-1, 1) * sc(rows)).sum() + (wc.double().view(-1, 1) * sc(cols)).sum())
    print(f"score_sum {family} norm {norm}: got {float(val):.9e} want {want:.9e}")
    assert abs(float(val) - want) <= 1e-5 * max(1.0, abs(want))


@pytest.mark.parametrize("kind,norm", [("tie_free", "softmax"), ("tie_free", "l1"), ("tie_free", None),
                                       ("neg", "softmax"), ("neg", None)])
def test_weak_loss_vs_fp64_autograd(kind, norm):
    """weak_loss_from_corr, value and gradient, on a volume of more than one
    tile both ways (R = 72, C = 273, scalar loads) against autograd of the fp64
    oracle; bounds of test_weak_loss_scores."""
    from ncnet_amd.ops.loss import weak_loss_from_corr
    xc = VR.weak_volume(kind)
    x = xc.to(DEV).requires_grad_(True)
    loss = weak_loss_from_corr(x, 2, norm)
    loss.backward()
    xr = xc.double().requires_grad_(True)
    lr = ref.match_score(xr[2:], norm) - ref.match_score(xr[:2], norm)
    lr.backward()
    gerr = relerr(x.grad, xr.grad)
    loss, lr = float(loss.detach()), float(lr.detach())
    print(f"weak loss {kind} {norm}: value {loss:.9e} vs {lr:.9e}, gradient relerr {gerr:.3e}")
    assert abs(loss - lr) < 1e-5 * max(1.0, abs(lr))
    assert gerr < 1e-4


def _assert_matches_equal(got, want, tag):
    """corr_to_matches(return_indices=True) tuples: coordinates to 1e-6
    (linspace rounding), scores to 1e-5 relative, indices equal."""
    for name, a, b in zip(("xA", "yA", "xB", "yB"), got[:4], want[:4]):
        assert float((a.cpu() - b).abs().max()) <= 1e-6, (tag, name)
    s, sr = got[4].cpu().double(), want[4].double()
    assert float(((s - sr).abs() / sr.abs()).max()) <= 1e-5, (tag, "score")
    for name, a, b in zip(("iA", "jA", "iB", "jB"), got[5:], want[5:]):
        assert torch.equal(a.cpu().long(), b.long()), (tag, name)


@pytest.mark.parametrize("do_softmax", [True, False])
@pytest.mark.parametrize("invert", [False, True])
def test_corr_to_matches_vs_cpu(invert, do_softmax):
    """Match extraction on the GPU -- through point_tnf._best (stats_cols /
    stats_rows) and through best_both (stats2d) -- against the same function
    on a CPU copy, which takes the torch.softmax / torch.max branch."""
    from ncnet_amd.eval.point_tnf import best_both, corr_to_matches
    xc = VR.inloc_volume()
    x = xc.to(DEV)
    kw = dict(do_softmax=do_softmax, invert_matching_direction=invert, return_indices=True)
    want = corr_to_matches(xc, **kw)
    _assert_matches_equal(corr_to_matches(x, best=None, **kw), want, "_best")
    both = best_both(x, do_softmax)
    assert both is not None
    _assert_matches_equal(corr_to_matches(x, best=both[1 if invert else 0], **kw), want, "best_both")


@pytest.mark.parametrize("do_softmax", [True, False])
@pytest.mark.parametrize("k", [1, 2])
def test_pair_matches_vs_cpu(k, do_softmax):
    """inloc.pair_matches on the GPU (stats2d + match_candidates) against the
    op-by-op path on a CPU copy (torch.softmax / torch.max): the same matches in
    the same order.  k = 2 decodes packed relocalization offsets."""
    import ncnet_amd.eval.inloc as inl
    xc = VR.inloc_volume()
    code = None
    if k == 2:
        g = torch.Generator().manual_seed(13)
        f4 = torch.randint(0, k, (4,) + tuple(xc.shape), generator=g)
        code = ((f4[0] << 6) | (f4[1] << 4) | (f4[2] << 2) | f4[3]).to(torch.uint8)
    want = inl.pair_matches(xc, code, k, do_softmax=do_softmax)
    assert inl._fused_candidates(xc.to(DEV), None if code is None else code.to(DEV), k, do_softmax) is not None
    got = inl.pair_matches(xc.to(DEV), None if code is None else code.to(DEV), k, do_softmax=do_softmax).cpu()
    assert got.shape == want.shape and got.shape[0] > 0
    assert float((got[:, :4] - want[:, :4]).abs().max()) <= 1e-6
    assert float(((got[:, 4] - want[:, 4]).abs() / want[:, 4].abs()).max()) <= 1e-5


# ---------------------------------------------------------------------------
# a contiguous view that is not 16-byte aligned
# ---------------------------------------------------------------------------

def _misaligned(t: torch.Tensor) -> torch.Tensor:
    """A contiguous copy of ``t`` that starts 4 bytes into its buffer."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def test_misaligned_views_equal_aligned_copies():
    """A contiguous view that starts 4 bytes into its buffer gives the results
    of an aligned copy: max, argmax and the MutualMatching output bit for bit,
    the sums within their bounds.  This pins the equality of the results, not
    the choice of the load path: the launchers take the 16-byte-load kernels
    of stats2d and mm_bwd only for 16-byte aligned pointers (aligned16,
    csrc/common.h), but gfx950 also serves a misaligned 16-byte global load
    and both kernels do their arithmetic in the same order, so the test
    cannot tell which of them ran."""
    from ncnet_amd.ops.mutual import mutual_matching
    shape = (2, 70, 260)
    xc, rows, cols = VR.case("ties", shape)
    xa = xc.to(DEV)
    xm = _misaligned(xa)
    for sum_kind in (0, 1, 2):
        a, m = _run("stats2d", xa, sum_kind), _run("stats2d", xm, sum_kind)
        _check(f"aligned {sum_kind}", a, rows, cols, sum_kind)
        _check(f"misaligned {sum_kind}", m, rows, cols, sum_kind)
        for k in ("rmx", "rarg", "cmx", "carg"):
            assert torch.equal(a[k], m[k]), (sum_kind, k)
    # MutualMatching forward and backward: c and g both misaligned
    c4 = VR.distinct((2, 1, 7, 10, 13, 20), 14, 0.0, 1.0).to(DEV)
    g4 = torch.randn(c4.shape, generator=torch.Generator().manual_seed(15)).to(DEV)
    res = []
    for mis in (False, True):
        c = (_misaligned(c4) if mis else c4.clone()).requires_grad_(True)
        g = _misaligned(g4) if mis else g4.clone()
        y = mutual_matching(c)
        y.backward(g)
        res.append((y.detach().clone(), c.grad.clone()))
    assert torch.equal(res[0][0], res[1][0])
    assert relerr(res[1][1], res[0][1]) <= 1e-5
    cr = c4.double().cpu().requires_grad_(True)
    ref.mutual_matching(cr).backward(g4.double().cpu())
    assert relerr(res[0][0], ref.mutual_matching(cr.detach())) < 1e-5
    for y, gc in res:
        assert relerr(gc, cr.grad) < 1e-4
