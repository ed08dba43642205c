"""Relocalized training on the GPU: the fused correlation pool with pair maps,
the HIP backward of the pooled correlation (csrc/corrpool_bwd.hip) at op,
autograd and Trainer level (run on an MI355X)."""
import pytest
import torch

from ncnet_amd.ops import _ext
from ncnet_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

GRIDS = [(6, 8, 10, 14), (18, 16, 10, 14)]      # N = 140 crosses v1's 128-column tile, M = 288 v2's 256-row tile
AMAP, BMAP = [0, 1, 1], [0, 1, 0]               # image 2 of A is in no volume
WEAK = ([0, 1, 1, 0], [0, 1, 0, 1])             # each image in two volumes, the weak-loss pattern


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def _operands(kind, grid, K, na=3, nb=2, seed=5):
    """(fa, fb, scale): operands of the pool and the factor of its fp64 oracle."""
    from ncnet_amd.ops.correlation import FP8, FP8_FEAT_SCALE
    hA, wA, hB, wB = grid
    g = torch.Generator().manual_seed(seed)
    fa = torch.randn(na, hA * wA, K, generator=g).to(DEV)
    fb = torch.randn(nb, hB * wB, K, generator=g).to(DEV)
    if kind == "fp8":
        return (fa * 0.125 * FP8_FEAT_SCALE).to(FP8), (fb * 0.125 * FP8_FEAT_SCALE).to(FP8), 1.0 / FP8_FEAT_SCALE ** 2
    return fa.to(torch.bfloat16).float(), fb.to(torch.bfloat16).float(), 1.0


def _top2_gap_ok(corr, k=2):
    """Per pooled cell: whether the fp64 top-two gap inside the window exceeds 1e-4 * max(1, |max|)."""
    b, _, i, j, kk, l = corr.shape
    x = corr.reshape(b, i // k, k, j // k, k, kk // k, k, l // k, k).permute(0, 1, 3, 5, 7, 2, 4, 6, 8)
    top = x.reshape(b, i // k, j // k, kk // k, l // k, k ** 4).topk(2, dim=-1).values
    return (top[..., 0] - top[..., 1]) > 1e-4 * top[..., 0].abs().clamp(min=1.0)


@pytest.mark.parametrize("v2", [0, 1])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("kind,K", [("bf16", 64), ("fp8", 64), ("fp8", 128)])
def test_fused_pool_with_pair_maps(tune, kind, K, grid, v2):
    from ncnet_amd.ops.correlation import _fp8_rows, block_order_index
    tune("corr_v2", v2)
    hA, wA, hB, wB = grid
    fa, fb, scale = _operands(kind, grid, K)
    am = torch.tensor(AMAP, dtype=torch.int32, device=DEV)
    bm = torch.tensor(BMAP, dtype=torch.int32, device=DEV)
    pa, pb = block_order_index(hA, wA, 2, DEV), block_order_index(hB, wB, 2, DEV)
    if kind == "fp8":
        a, b = _fp8_rows(fa, pa), _fp8_rows(fb, pb)
    else:
        a, b = fa.to(torch.bfloat16)[:, pa].contiguous(), fb.to(torch.bfloat16)[:, pb].contiguous()
    shape = (3, hA // 2, wA // 2, hB // 2, wB // 2)
    val = torch.full(shape, float("nan"), device=DEV)
    code = torch.full(shape, 0xFF, dtype=torch.uint8, device=DEV)
    C = _ext.ext()
    C.corr_gemm_pool2(a, b, val, code, hA, wA, hB, wB, scale, am, bm)
    assert not torch.isnan(val).any()
    assert int((code & 0xAA).max()) == 0                       # every code written: offsets 0 / 1 only
    # fp64 oracle on the same operand values
    corr = (torch.bmm(fa.double()[am.long()], fb.double()[bm.long()].transpose(1, 2)) * scale).view(3, 1, hA, wA, hB, wB)
    want, woff = ref.maxpool4d(corr, 2)
    err = rel_l2(val.unsqueeze(1), want)
    bound = 1e-4 if kind == "fp8" else 1e-5
    print(f"mapped pool {kind} K={K} {grid} v{v2 + 1}: rel. L2 {err:.3e} (bound {bound:g})")
    assert err < bound
    ok = _top2_gap_ok(corr)
    left_out = 1.0 - float(ok.float().mean())
    print(f"  cells left out of the offset comparison: {100 * left_out:.3f} % (bound 1 %)")
    assert left_out <= 0.01
    c = code.long()
    for got, w in zip(((c >> 6) & 3, (c >> 4) & 3, (c >> 2) & 3, c & 3), woff):
        assert torch.equal(got[ok], w.reshape(shape)[ok])
    # volume v with maps == the unmapped call on the gathered operands, bit for bit
    val2 = torch.full(shape, float("nan"), device=DEV)
    code2 = torch.full(shape, 0xFF, dtype=torch.uint8, device=DEV)
    if kind == "fp8":
        ag, bg = a.view(torch.uint8)[am.long()].contiguous().view(a.dtype), b.view(torch.uint8)[bm.long()].contiguous().view(b.dtype)
    else:
        ag, bg = a[am.long()].contiguous(), b[bm.long()].contiguous()
    C.corr_gemm_pool2(ag, bg, val2, code2, hA, wA, hB, wB, scale)
    assert torch.equal(val, val2) and torch.equal(code, code2)


def test_fused_pool_map_checks():
    C = _ext.ext()
    a = torch.zeros(3, 48, 64, dtype=torch.bfloat16, device=DEV)
    b = torch.zeros(2, 140, 64, dtype=torch.bfloat16, device=DEV)
    val = torch.empty(3, 3, 4, 5, 7, device=DEV)
    code = torch.empty(3, 3, 4, 5, 7, dtype=torch.uint8, device=DEV)
    am = torch.tensor(AMAP, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        C.corr_gemm_pool2(a, b, val, code, 6, 8, 10, 14, 1.0)                     # Nb != V without a bmap
    with pytest.raises(RuntimeError):
        C.corr_gemm_pool2(a, b, val, code, 6, 8, 10, 14, 1.0, am.long(), am)      # dtype
    with pytest.raises(RuntimeError):
        C.corr_gemm_pool2(a, b, val, code, 6, 8, 10, 14, 1.0, am[:2], am)         # shape


BWD_CASES = [(GRIDS[0], 3, 2, AMAP, BMAP), (GRIDS[1], 3, 2, AMAP, BMAP), ((50, 50, 50, 50), 2, 2, *WEAK)]


def _decode1(code):
    """The offsets the backward kernel reads from a code byte: the low bit of each 2-bit field."""
    c = code.long()
    return ((c >> 6) & 1, (c >> 4) & 1, (c >> 2) & 1, c & 1)


def _natural(g_blk, h, w):
    from ncnet_amd.ops.correlation import block_order_inverse
    return g_blk[:, block_order_inverse(h, w, 2, g_blk.device)]


@pytest.mark.parametrize("grid,na,nb,amap,bmap", BWD_CASES)
def test_corr_pool2_bwd_against_fp64(grid, na, nb, amap, bmap):
    from ncnet_amd.ops.correlation import block_order_index, pool2_bwd_table, _transposed_padded
    hA, wA, hB, wB = grid
    K, V = 64, len(amap)
    fa, fb, _ = _operands("bf16", grid, K, na, nb, seed=6)
    gen = torch.Generator().manual_seed(7)
    shape = (V, hA // 2, wA // 2, hB // 2, wB // 2)
    g = torch.randn(shape, generator=gen).to(DEV)
    code = torch.randint(0, 256, shape, generator=gen, dtype=torch.int64).to(torch.uint8).to(DEV)
    # every (a, b) sub-row pair the kernel can decode occurs at every grid; all 256 bytes at 50 x 50
    assert len(torch.unique(code & 0x55)) == 16
    if grid == (50, 50, 50, 50):
        assert len(torch.unique(code)) == 256
    a = fa.to(torch.bfloat16)[:, block_order_index(hA, wA, 2, DEV)].contiguous()
    b = fb.to(torch.bfloat16)[:, block_order_index(hB, wB, 2, DEV)].contiguous()
    aoff, avol, boff, bvol, am, bm = pool2_bwd_table(amap, bmap, na, nb, DEV)
    C = _ext.ext()
    bt, at = _transposed_padded(b), _transposed_padded(a)
    assert bt.shape[2] % 32 == 0 and at.shape[2] % 32 == 0

    def run():
        ga = torch.full(a.shape, float("nan"), device=DEV)
        gb = torch.full(b.shape, float("nan"), device=DEV)
        C.corr_pool2_bwd(bt, g, code, aoff, avol, bm, ga, 0, hA, wA, hB, wB)
        C.corr_pool2_bwd(at, g, code, boff, bvol, am, gb, 1, hA, wA, hB, wB)
        return ga, gb

    ga, gb = run()
    assert not torch.isnan(ga).any() and not torch.isnan(gb).any()          # every element written
    ga2, gb2 = run()
    assert torch.equal(ga, ga2) and torch.equal(gb, gb2)                      # deterministic
    for n in range(na):
        if n not in amap:
            assert bool((ga[n] == 0).all())
    ga, gb = _natural(ga, hA, wA), _natural(gb, hB, wB)
    # the kernel rounds g to bf16 (ops/correlation.py corr_pool2_bwd): quantize_g=True
    offs = _decode1(code)
    wa, wb = ref.corr_pool2_bwd(fa.double(), fb.double(), g.double(), offs, amap, bmap, hA, wA, hB, wB,
                                quantize_g=True)
    ea, eb = rel_l2(ga, wa), rel_l2(gb, wb)
    print(f"corr_pool2_bwd {grid}: rel. L2 gA {ea:.3e} gB {eb:.3e} (bound 1e-5)")
    assert ea < 1e-5 and eb < 1e-5
    # mutation: the A and B sub-rows swapped in the oracle
    di, dj, dk, dl = offs
    ma, mb = ref.corr_pool2_bwd(fa.double(), fb.double(), g.double(), (dk, dl, di, dj), amap, bmap, hA, wA, hB, wB,
                                quantize_g=True)
    sa, sb = rel_l2(ga, ma), rel_l2(gb, mb)
    print(f"  sub-rows swapped: rel. L2 gA {sa:.3e} gB {sb:.3e} (>= 1e-3)")
    assert sa >= 1e-3 and sb >= 1e-3


def test_corr_pool2_bwd_rejects_bad_arguments():
    from ncnet_amd.ops.correlation import corr_pool2_bwd
    a = torch.zeros(1, 16, 24, dtype=torch.bfloat16, device=DEV)
    g = torch.zeros(1, 2, 2, 2, 2, device=DEV)
    code = torch.zeros(1, 2, 2, 2, 2, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        corr_pool2_bwd(a, a, g, code, [0], [0], 4, 4, 4, 4)                   # K % 16
    a = torch.zeros(1, 16, 32, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError):
        corr_pool2_bwd(a, a, g, code, [1], [0], 4, 4, 4, 4)                   # map entry out of range
    C = _ext.ext()
    out = torch.empty(1, 16, 32, device=DEV)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=DEV)          # noqa: E731
    with pytest.raises(RuntimeError):                                         # ft rows not padded to 32
        C.corr_pool2_bwd(a.transpose(1, 2).contiguous(), g, code, i32(0, 1), i32(0), i32(0), out, 0, 4, 4, 4, 4)
    ft = torch.zeros(1, 32, 32, dtype=torch.bfloat16, device=DEV)
    C.corr_pool2_bwd(ft, g, code, i32(0, 1), i32(0), i32(0), out, 0, 4, 4, 4, 4)        # the aligned call is fine
    assert bool((out == 0).all())
    odd = torch.empty(16 * 32 + 1, device=DEV)[1:].view(1, 16, 32)            # contiguous, 4 bytes off
    with pytest.raises(RuntimeError, match="aligned"):
        C.corr_pool2_bwd(ft, g, code, i32(0, 1), i32(0), i32(0), odd, 0, 4, 4, 4, 4)
    oddf = torch.zeros(32 * 32 + 1, dtype=torch.bfloat16, device=DEV)[1:].view(1, 32, 32)
    with pytest.raises(RuntimeError, match="aligned"):
        C.corr_pool2_bwd(oddf, g, code, i32(0, 1), i32(0), i32(0), out, 0, 4, 4, 4, 4)


def test_autograd_through_the_mapped_pool():
    from ncnet_amd.ops.correlation import block_order_index, corr_pool2_bwd, correlation_pool2
    grid = GRIDS[1]
    hA, wA, hB, wB = grid
    fa, fb, _ = _operands("bf16", grid, 64, seed=8)
    fa.requires_grad_(True)
    fb.requires_grad_(True)
    n0 = _ext.DISPATCH["corr_pool2_bwd"]
    pooled, code = correlation_pool2(fa, fb, hA, wA, hB, wB, packed=True, amap=AMAP, bmap=BMAP)
    assert pooled.requires_grad and not code.requires_grad and code.dtype == torch.uint8
    # the forward is the inference path's, bit for bit
    with torch.no_grad():
        p2, c2 = correlation_pool2(fa, fb, hA, wA, hB, wB, packed=True, amap=AMAP, bmap=BMAP)
    assert torch.equal(pooled, p2) and torch.equal(code, c2)
    w = torch.randn(pooled.shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    ga, gb = torch.autograd.grad((w * pooled).sum(), (fa, fb))
    assert _ext.DISPATCH["corr_pool2_bwd"] == n0 + 1
    assert ga.dtype == torch.float32 and ga.shape == fa.shape and gb.shape == fb.shape
    a = fa.detach().to(torch.bfloat16)[:, block_order_index(hA, wA, 2, DEV)].contiguous()
    b = fb.detach().to(torch.bfloat16)[:, block_order_index(hB, wB, 2, DEV)].contiguous()
    ka, kb = corr_pool2_bwd(a, b, w, code, AMAP, BMAP, hA, wA, hB, wB)
    assert torch.equal(ga, _natural(ka, hA, wA)) and torch.equal(gb, _natural(kb, hB, wB))
    wa, wb = ref.corr_pool2_bwd(fa.detach().double(), fb.detach().double(), w.double(), _decode1(code), AMAP, BMAP,
                                hA, wA, hB, wB, quantize_g=True)
    ea, eb = rel_l2(ga, wa), rel_l2(gb, wb)
    print(f"autograd {grid}: rel. L2 gA {ea:.3e} gB {eb:.3e} (bound 1e-5)")
    assert ea < 1e-5 and eb < 1e-5
    # bf16 inputs get bf16 gradients: the same numbers, rounded once
    fa16 = fa.detach().to(torch.bfloat16).requires_grad_(True)
    fb16 = fb.detach().to(torch.bfloat16).requires_grad_(True)
    p16, _ = correlation_pool2(fa16, fb16, hA, wA, hB, wB, packed=True, amap=AMAP, bmap=BMAP)
    ga16, gb16 = torch.autograd.grad((w * p16).sum(), (fa16, fb16))
    assert ga16.dtype == torch.bfloat16
    assert torch.equal(ga16, ga.to(torch.bfloat16)) and torch.equal(gb16, gb.to(torch.bfloat16))
    # fp8 / f16 operands stay inference-only
    with pytest.raises(RuntimeError, match="inference-only"):
        correlation_pool2(fa.detach().half().requires_grad_(True), fb.detach().half(), hA, wA, hB, wB)


def _model(**kw):
    from ncnet_amd.models import ImMatchNet
    torch.manual_seed(0)
    return ImMatchNet(ncons_kernel_sizes=[5, 5, 5], ncons_channels=[16, 16, 1], relocalization_k_size=2, **kw).to(DEV)


def _trainer(model, loss):
    from ncnet_amd.engine.trainer import Trainer, make_adam
    from ncnet_amd.parallel.dist import DistContext
    params = [p for p in model.parameters() if p.requires_grad]
    return Trainer(model, make_adam(params, 1e-3), DistContext(device=torch.device(DEV, 0)), loss=loss)


def _restore(params, values):
    with torch.no_grad():
        for p, v in zip(params, values):
            p.copy_(v)


def test_trainer_frozen_trunk_800px():
    import importlib
    from ncnet_amd.data.augment import PairAugment
    from ncnet_amd.data.datasets import (SyntheticCorrespondenceDataset, SyntheticImageDataset, collate_uint8_images,
                                         gpu_view_batch, synthetic_batch)
    from ncnet_amd.ops.correlation import correlation_pool2
    from ncnet_amd.ops.loss import weak_loss_from_corr
    nc_ops = importlib.import_module("ncnet_amd.ops.neigh_consensus")
    model = _model()
    model.train()
    batch = synthetic_batch(2, (800, 800), DEV, seed=3)
    nc = model.NeighConsensus
    ncp = list(nc.parameters())
    state = [p.detach().clone() for p in ncp]
    f0 = _ext.DISPATCH["torch_fallback"]

    # by hand: mapped fused pool -> process_correlation -> weak loss
    with torch.no_grad():
        f, hw = model.extract(torch.cat((batch["source_image"], batch["target_image"]), 0))
    assert tuple(hw) == (50, 50)
    pooled, _ = correlation_pool2(f[:2], f[2:], 50, 50, 50, 50, amap=WEAK[0], bmap=WEAK[1])
    assert pooled.shape == (4, 1, 25, 25, 25, 25)
    # the NC stack sees the 400 px shape: the compile-time 25 x 25 kernels
    wrefs = [m.weight_ref() for m in nc.conv_layers()]
    like400 = torch.zeros(4, 1, 25, 25, 25, 25, device=DEV)
    assert nc.padded_input_ks(pooled) == nc.padded_input_ks(like400) == 5
    pad = torch.zeros(1)
    assert (nc_ops.select_path(pooled, wrefs, nc.channels, True, False, "bf16", padded=pad)
            == nc_ops.select_path(like400, wrefs, nc.channels, True, False, "bf16", padded=pad) == "bf16_padded")
    want = weak_loss_from_corr(model.process_correlation(pooled), 2, "softmax")
    want.backward()
    want_grads = [p.grad.detach().clone() for p in ncp]
    for p in ncp:
        p.grad = None

    tr = _trainer(model, "weak")
    loss = tr.train_step(batch)
    torch.cuda.synchronize()
    assert torch.equal(loss, want.detach())
    for p, w in zip(ncp, want_grads):
        assert torch.equal(p.grad, w)
    assert _ext.DISPATCH["torch_fallback"] == f0

    # strong and warp steps on the pooled volume, then the evaluation's PCK with the offsets
    ds = SyntheticCorrespondenceDataset(2, 800, seed=1)
    sb = torch.utils.data.default_collate([ds[0], ds[1]])
    sb = {k: v.to(DEV) for k, v in sb.items()}
    ims = SyntheticImageDataset(2, (500, 620), seed=3)
    wb = gpu_view_batch(collate_uint8_images([ims[0], ims[1]]), DEV, 800, 800, PairAugment(),
                        torch.Generator().manual_seed(11), with_points=True)
    for kind, b in (("strong", sb), ("warp", wb)):
        _restore(ncp, state)                  # every step starts from the initial weights
        model.train()
        t = _trainer(model, kind)
        step = t.train_step(b)
        torch.cuda.synchronize()
        assert torch.isfinite(step)
        print(f"{kind} step at 800 px, k = 2: loss {float(step):.6f}, NC grad norms "
              f"{[float(p.grad.norm()) for p in ncp]}, skipped steps {t.opt.skipped_steps}")
        assert all(torch.isfinite(p.grad).all() for p in ncp) and any(bool((p.grad != 0).any()) for p in ncp)
        model.eval()
        seen = []
        import ncnet_amd.eval.point_tnf as pt
        real = pt.corr_to_matches
        pt.corr_to_matches = lambda c, *a, **kw: (seen.append((tuple(c.shape[2:]), kw.get("k_size"),
                                                               kw.get("delta4d") is not None)), real(c, *a, **kw))[1]
        try:
            ev = t.eval_step(b)
        finally:
            pt.corr_to_matches = real
        assert torch.isfinite(ev) and seen == [((25, 25, 25, 25), 2, True)]
        pck = t._pck[-1]
        assert pck.shape == (2,) and bool(((pck >= 0) & (pck <= 1)).all())
    assert _ext.DISPATCH["torch_fallback"] == f0


def test_trainer_trainable_trunk_320px():
    from ncnet_amd.data.datasets import synthetic_batch
    det = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        model = _model()
        trunk = list(model.FeatureExtraction.model[-1][-1].parameters())     # --fe_finetune_params 1
        for p in trunk:
            p.requires_grad = True
        model.train()
        batch = synthetic_batch(2, (320, 320), DEV, seed=4)
        trained = [p for p in model.parameters() if p.requires_grad]
        state = [p.detach().clone() for p in trained]
        f0, n0 = _ext.DISPATCH["torch_fallback"], _ext.DISPATCH["corr_pool2_bwd"]
        assert not _ext.fallback_allowed()
        runs = []
        for _ in range(2):
            _restore(trained, state)
            tr = _trainer(model, "weak")
            assert not tr.prefetch.enabled
            loss = tr.train_step(batch)
            torch.cuda.synchronize()
            assert torch.isfinite(loss)
            runs.append([p.grad.detach().clone() for p in trunk])
        assert _ext.DISPATCH["corr_pool2_bwd"] == n0 + 2 and _ext.DISPATCH["torch_fallback"] == f0
        for g in runs[0]:
            assert torch.isfinite(g).all()
        assert any(bool((g != 0).any()) for g in runs[0])
        for g1, g2 in zip(*runs):
            assert torch.equal(g1, g2)
        model.relocalization_k_size = 3
        with pytest.raises(ValueError, match="k = 2"):
            _trainer(model, "weak").train_step(batch)
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = det
