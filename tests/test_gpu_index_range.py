"""The training kernels at the index range of the headline batch.

bench.py's headline step (batch 256) sends 1024 volumes through the
NeighConsensus stack: a 16-channel hidden volume [V, 25, 25, 25, 25, 16] bf16
is 12.5e6 bytes per v, so whole volumes lie past 2^31 bytes (v >= 172), past
2^32 bytes = 2^31 elements (v >= 344) and past 2^32 elements (v >= 688).
Every kernel here is per-volume, so one launch on V = 704 volumes (the smallest
round V with whole volumes past all three thresholds) must reproduce, bit for
bit, eleven launches of the same binding on 64-volume slices -- the size the
oracle tests of test_gpu_kernels.py pin to fp64.  A wrapped offset lands in an
EARLY volume, so every chunk is compared, not only the late ones.  Volume 703
is also compared with the fp64 oracle directly, and each test ends by showing
that the comparison sees a wrap: volume 700 computed from volume 12's input
(where a wrapped 32-bit element index would read: 700 - 2^32 / 6.25e6 = 12.8)
must differ from the big launch's volume 700.

The weight gradients reduce over all volumes; integer-valued operands make
every fp32 partial sum exact, so the sum of the chunk launches equals the big
launch whatever the order of the additions.
"""
import pytest
import torch

from ncnet_amd.ops import _ext
from ncnet_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

V, CH, T, KS = 704, 64, 25, 5          # volumes, volumes per chunk, plane side, kernel size
VOL = (T, T, T, T)
MUT_V, WRAP_V = 700, 12                # see the module docstring
CHUNKS = [(c0, c0 + CH) for c0 in range(0, V, CH)]
assert V % CH == 0 and len(CHUNKS) == 11
# the thresholds the shape is chosen for (bf16 elements of 16 channels per volume)
EPV = T ** 4 * 16
assert (V - 1) * EPV > 2 ** 32 and 343 * EPV < 2 ** 31 < 344 * EPV and 171 * EPV * 2 < 2 ** 31 < 172 * EPV * 2


@pytest.fixture(autouse=True)
def _memory():
    """Peak device memory of each test (printed), and nothing left in the cache."""
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    torch.cuda.synchronize()
    print(f"peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
    torch.cuda.empty_cache()


def relerr(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def bf(x):
    return x.to(torch.bfloat16).double()


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _filled(tail, dtype, draw, nv=V):
    """[nv, *tail] filled on the device chunk by chunk; draw(shape) returns fresh
    random values, so every volume differs from every other."""
    t = torch.empty((nv,) + tuple(tail), dtype=dtype, device=DEV)
    for c0 in range(0, nv, CH):
        c1 = min(nv, c0 + CH)
        t[c0:c1] = draw((c1 - c0,) + tuple(tail))
    return t


def _uniform(g):
    return lambda shape: torch.rand(shape, device=DEV, generator=g)


def _normal(g):
    return lambda shape: torch.randn(shape, device=DEV, generator=g)


def _zero_one(g):          # {0, 1}, half of each, everywhere in the tensor
    return lambda shape: (torch.rand(shape, device=DEV, generator=g) < 0.5).float()


def _sparse_sign(g):       # {-1, 0, 1}, 1 / 64 of the entries non-zero
    def draw(shape):
        u = torch.rand(shape, device=DEV, generator=g)
        return (u < 1 / 128).float() - (u > 1 - 1 / 128).float()
    return draw


def _bad_volumes(a, b, v0=0):
    """Indices (from v0) of the volumes in which a and b differ (NaN differs from everything)."""
    return [v0 + int(i) for i in (a != b).flatten(1).any(1).nonzero().flatten()]


def _all_finite(y):
    return all(bool(torch.isfinite(y[c0:c1]).all()) for c0, c1 in CHUNKS if c0 < y.shape[0])


def _check_per_volume(run, ins, out_tail, out_dtype, oracle, tol, mut_src=WRAP_V):
    """The method of the module docstring for a per-volume kernel.

    run(ins, y): launch the binding on the volume-sliced operands ``ins`` (a list
    of tensors with the volume axis first; ins[0] is the convolution input) into y;
    oracle(ins): fp64 result [1, *out_tail] for one-volume slices, compared with
    volume V - 1 of the big launch within ``tol`` (max error / max value, the
    bound of the kernel's test in test_gpu_kernels.py);
    mut_src: the volume whose input replaces volume MUT_V's in the mutation."""
    y_big = torch.full((V,) + tuple(out_tail), float("nan"), dtype=out_dtype, device=DEV)
    run(ins, y_big)
    bad = []
    for c0, c1 in CHUNKS:
        yc = torch.full((c1 - c0,) + tuple(out_tail), float("nan"), dtype=out_dtype, device=DEV)
        run([t[c0:c1] for t in ins], yc)
        if not torch.equal(y_big[c0:c1], yc):
            bad += _bad_volumes(y_big[c0:c1], yc, c0)
    assert not bad, f"{len(bad)} volumes of the V = {V} launch differ from their 64-volume launch, first {bad[:8]}"
    assert _all_finite(y_big)
    e = relerr(y_big[V - 1:], oracle([t[V - 1:] for t in ins]))
    print(f"volume {V - 1} vs fp64 oracle: {e:.2e} (bound {tol:.0e})")
    assert e < tol, e
    # mutation: volume MUT_V from another volume's input is not the big launch's volume MUT_V
    c0, c1 = CHUNKS[MUT_V // CH]
    mins = [t[c0:c1] for t in ins]
    mins[0] = mins[0].clone()
    mins[0][MUT_V - c0] = ins[0][mut_src]
    ym = torch.full((c1 - c0,) + tuple(out_tail), float("nan"), dtype=out_dtype, device=DEV)
    run(mins, ym)
    assert not torch.equal(ym[MUT_V - c0], y_big[MUT_V]), "the comparison cannot see a wrapped volume index"
    assert _bad_volumes(ym, y_big[c0:c1], c0) == [MUT_V]


def _mask_epi(z, m):
    return z * (m.double().permute(0, 5, 1, 2, 3, 4) > 0)


def _cl(y):      # oracle [n, C, I, J, K, L] -> channels-last
    return y.permute(0, 2, 3, 4, 5, 1)


# ---------------------------------------------------------------------------
# tier 1: the kernels of the headline step, default tuning
# ---------------------------------------------------------------------------
def _conv1x16_case(epi, mut_src=WRAP_V):
    from ncnet_amd.ops.packing import pack_w1x
    C = _ext.ext()
    g = _gen(100 + epi)
    w = torch.randn(16, 1, KS, KS, KS, KS, device=DEV, generator=g) * 0.05
    b = torch.randn(16, device=DEV, generator=g) * 0.1
    wa = pack_w1x(w)
    ppl = C.pad_geom(T, T, KS)[1]
    ins = [_filled(VOL, torch.bfloat16, _uniform(g))]
    if epi == 2:
        ins.append(_filled(VOL + (16,), torch.bfloat16, _normal(g)))

    def run(s, y):
        x = s[0]
        nv = x.shape[0]
        # the 1-channel padded planes of these volumes, by pad_planes at the same volume count
        xp = torch.zeros((nv * T * T, ppl), dtype=torch.bfloat16, device=DEV)
        C.pad_planes(x.reshape(nv, T * T, T * T), xp, T, T, KS, 0)
        assert C.conv1x16(xp, wa, b if epi == 1 else None, s[1] if epi == 2 else None, y, KS, epi)

    def oracle(s):
        z = ref.conv4d(s[0].double().unsqueeze(1), ref.conv4d_weight_from_std(bf(w)), None)
        return _cl(torch.relu(z + b.double().view(1, 16, 1, 1, 1, 1)) if epi == 1 else _mask_epi(z, s[1]))

    _check_per_volume(run, ins, VOL + (16,), torch.bfloat16, oracle, 1e-2, mut_src)   # test_conv1x16_vs_oracle


def test_conv1x16_fwd_index_range():
    """conv1x16 forward (bias + ReLU): 1-channel padded planes in, the 8.8 GB
    16-channel volume out."""
    _conv1x16_case(1)


def test_conv1x16_dgrad_index_range():
    """conv1x16 in data-gradient mode: the ReLU mask M read and the output
    written are both 8.8 GB 16-channel volumes."""
    _conv1x16_case(2)


def _conv16_case(epi, mut_src=WRAP_V):
    """conv16_fwd 16 -> 16 (conv16v4 by default, conv16v3 under tune conv_v3):
    epi 1 bias + ReLU, epi 2 the ReLU-mask epilogue of the data gradient."""
    from ncnet_amd.ops.packing import pack_w16
    C = _ext.ext()
    g = _gen(200 + epi)
    w_std = torch.randn(16, 16, KS, KS, KS, KS, device=DEV, generator=g) * 0.05
    b = torch.randn(16, device=DEV, generator=g) * 0.1
    w = pack_w16(w_std)
    ins = [_filled(VOL + (16,), torch.bfloat16, _uniform(g))]
    if epi == 2:
        ins.append(_filled(VOL + (16,), torch.bfloat16, _normal(g)))

    def run(s, y):
        C.conv16_fwd(s[0], w, b if epi == 1 else None, s[1] if epi == 2 else None, y, KS, epi)

    def oracle(s):
        z = ref.conv4d(s[0].double().permute(0, 5, 1, 2, 3, 4), ref.conv4d_weight_from_std(bf(w_std)), None)
        return _cl(torch.relu(z + b.double().view(1, 16, 1, 1, 1, 1)) if epi == 1 else _mask_epi(z, s[1]))

    _check_per_volume(run, ins, VOL + (16,), torch.bfloat16, oracle, 4e-3, mut_src)   # test_conv16v4_matches_v3_bitwise


def test_conv16v4_fwd_index_range():
    _conv16_case(1)


def test_conv16v4_dgrad_index_range():
    _conv16_case(2)


def _cout1_case(kind, mut_src=WRAP_V):
    """The Cout = 1 last layer, 16-channel input (8.8 GB) and fp32 output:
    cout1_taps_fwd (kind 'taps', the headline step's) or conv16_blk_fwd ('blk')."""
    from ncnet_amd.ops.packing import blk_out_weights, cout1_taps_weights, pack_w16_planes
    C = _ext.ext()
    g = _gen(300)
    w = torch.randn(1, 16, KS, KS, KS, KS, device=DEV, generator=g) * 0.05
    b = torch.randn(1, device=DEV, generator=g) * 0.1 - 0.3
    wp = cout1_taps_weights(w).to(torch.bfloat16) if kind == "taps" else pack_w16_planes(blk_out_weights(w))
    ins = [_filled(VOL + (16,), torch.bfloat16, _uniform(g))]

    def run(s, y):
        if kind == "taps":
            assert C.cout1_taps_fwd(s[0], wp, b, y, KS, 1)
        else:
            C.conv16_blk_fwd(s[0], wp, b, y, KS, 1)

    def oracle(s):
        x = s[0].double().permute(0, 5, 1, 2, 3, 4)
        return torch.relu(ref.conv4d(x, ref.conv4d_weight_from_std(bf(w)), b.double())[:, 0])

    _check_per_volume(run, ins, VOL, torch.float32, oracle, 1e-4, mut_src)   # test_cout1_taps_fwd / test_conv16_blk_fwd


def test_cout1_taps_fwd_index_range():
    _cout1_case("taps")


def test_combine_index_range(mut_src=WRAP_V):
    """combine_fwd / combine_bwd at the 1-channel sizes of the step, Vh = 352
    pairs (no byte threshold is crossed: the item and grid arithmetic only).
    The big launch against launches on 32-pair chunks and against the
    definition y = z1 + z2^T, gz = g (z > 0) (exact in fp32 / one bf16 rounding)."""
    C = _ext.ext()
    Vh, ch, R = V // 2, CH // 2, T * T
    g = _gen(400)
    z = _filled((R, R), torch.float32, _normal(g))                  # [2 Vh, R, C]: branch A, then B as [C, R]
    gy = _filled((R, R), torch.float32, _normal(g), nv=Vh)

    def run(zz, gg):
        n = gg.shape[0]
        y = torch.full((n, R, R), float("nan"), device=DEV)
        gz = torch.full((2 * n * R * R,), float("nan"), dtype=torch.bfloat16, device=DEV)
        C.combine_fwd(zz.reshape(-1), y, R, R)
        C.combine_bwd(gg, zz, gz, R, R)
        return y, gz.view(2 * n, R, R)

    y_big, gz_big = run(z, gy)
    assert torch.isfinite(y_big).all() and torch.isfinite(gz_big).all()
    bad = []
    for c0 in range(0, Vh, ch):
        c1 = c0 + ch
        zc = torch.cat((z[c0:c1], z[Vh + c0:Vh + c1]))
        yc, gzc = run(zc, gy[c0:c1])
        gzb = torch.cat((gz_big[c0:c1], gz_big[Vh + c0:Vh + c1]))
        if not (torch.equal(y_big[c0:c1], yc) and torch.equal(gzb, gzc)):
            bad += _bad_volumes(y_big[c0:c1], yc, c0) + _bad_volumes(gzb, gzc, c0)
        # the definition, on this chunk
        assert torch.equal(yc, zc[:ch] + zc[ch:].transpose(1, 2))
        assert torch.equal(gzc[:ch], (gy[c0:c1] * (zc[:ch] > 0)).to(torch.bfloat16))
        assert torch.equal(gzc[ch:], (gy[c0:c1].transpose(1, 2) * (zc[ch:] > 0)).to(torch.bfloat16))
    assert not bad, f"pairs of the Vh = {Vh} launch differ from their chunk launch, first {bad[:8]}"
    # mutation: pair 340 from another pair's branch-B input
    mv = 340
    c0 = mv // ch * ch
    zc = torch.cat((z[c0:c0 + ch], z[Vh + c0:Vh + c0 + ch]))
    zc[ch + mv - c0] = z[Vh + mut_src]
    ym, gzm = run(zc, gy[c0:c0 + ch])
    assert not torch.equal(ym[mv - c0], y_big[mv])
    assert not torch.equal(gzm[ch + mv - c0], gz_big[Vh + mv])


def _check_wgrad(launch, x, gr, nx_max=1.0, mut_src=WRAP_V):
    """launch(x, gr) -> (part, partb) partials of one binding call over the
    volumes given.  With integer operands and (non-zero gradient voxels per
    channel) x max|x| < 2^24 every partial sum is an exactly representable
    integer, so the reduced big launch equals the sum of the chunk launches."""
    nnz = torch.zeros(16, dtype=torch.int64, device=DEV)
    gsum = torch.zeros(16, dtype=torch.int64, device=DEV)
    for c0, c1 in CHUNKS:
        gc = gr[c0:c1]
        nnz += (gc != 0).flatten(0, 4).sum(0)
        gsum += gc.flatten(0, 4).sum(0, dtype=torch.float64).long()     # integers: exact
        assert float(x[c0:c1].abs().max()) <= nx_max and float(x[c0:c1].float().mean()) > 0.4   # dense, not a few ones
    print(f"non-zero gradient voxels per channel: max {int(nnz.max())}")
    assert int(nnz.max()) * nx_max < 2 ** 24 and int(nnz.min()) > 0
    part, partb = launch(x, gr)
    big, bigb = part.sum(0), partb.sum(0)
    assert torch.isfinite(big).all() and torch.isfinite(bigb).all()
    acc, accb = torch.zeros_like(big), torch.zeros_like(bigb)
    mut = None
    for c0, c1 in CHUNKS:
        p, pb = launch(x[c0:c1], gr[c0:c1])
        acc += p.sum(0)
        accb += pb.sum(0)
        if c0 <= MUT_V < c1:
            xm = x[c0:c1].clone()
            xm[MUT_V - c0] = x[mut_src]
            pm, _ = launch(xm, gr[c0:c1])
            mut = pm.sum(0) - p.sum(0)
    assert torch.equal(bigb, accb), (bigb, accb)
    assert torch.equal(big, acc), f"{int((big != acc).sum())} of {big.numel()} weight-gradient sums differ"
    # the bias partial against an integer sum of the gradient: not only launch against launch
    assert torch.equal(bigb.long(), gsum), (bigb, gsum)
    # mutation: volume MUT_V's input replaced by another volume's moves the sum
    assert not torch.equal(big, acc + mut)


def test_wgrad16v4_index_range(mut_src=WRAP_V):
    """wgrad16 (wgrad16v4 by default, wgrad16v3 under tune wgrad_v3): both
    operands 8.8 GB, the groups of the training launch (ops/nc/layers.py)."""
    from ncnet_amd.ops.nc.layers import wgrad_v3_groups
    C = _ext.ext()
    g = _gen(500)
    x = _filled(VOL + (16,), torch.bfloat16, _zero_one(g))
    gr = _filled(VOL + (16,), torch.bfloat16, _sparse_sign(g))

    def launch(xx, gg):
        ng = wgrad_v3_groups(xx.shape, KS)
        part = torch.full((2 * ng, KS * KS, KS * KS, 16, 16), float("nan"), device=DEV)
        partb = torch.full((2 * ng, 16), float("nan"), device=DEV)
        C.wgrad16(xx, gg, part, partb, KS, 0, 3)
        return part, partb

    _check_wgrad(launch, x, gr, mut_src=mut_src)


def test_wgrad1x16_index_range(mut_src=WRAP_V):
    """wgrad1x16: the 16-channel D operand is the 8.8 GB one, X1 the 1-channel
    padded planes; one partial per CU as in the training launch."""
    C = _ext.ext()
    G = torch.cuda.get_device_properties(0).multi_processor_count
    ppl = C.pad_geom(T, T, KS)[1]
    g = _gen(600)
    x1 = _filled(VOL, torch.bfloat16, _zero_one(g))
    d = _filled(VOL + (16,), torch.bfloat16, _sparse_sign(g))

    def launch(xx, dd):
        nv = xx.shape[0]
        xp = torch.zeros((nv * T * T, ppl), dtype=torch.bfloat16, device=DEV)
        C.pad_planes(xx.reshape(nv, T * T, T * T), xp, T, T, KS, 0)
        part = torch.full((G, KS * KS, 32, 16), float("nan"), device=DEV)
        partb = torch.full((G, 16), float("nan"), device=DEV)
        assert C.wgrad1x16(dd, xp, part, partb, KS)
        return part, partb

    _check_wgrad(launch, x1, d, mut_src=mut_src)


# ---------------------------------------------------------------------------
# tier 2: the fallbacks behind the tune switches and at other planes (index
# arithmetic read and found 64-bit: plane_offset / size_t products throughout)
# ---------------------------------------------------------------------------
def test_conv16v3_fwd_index_range(tune):
    tune("conv_v3", 1)
    _conv16_case(1)


def test_conv16v3_dgrad_index_range(tune):
    tune("conv_v3", 1)
    _conv16_case(2)


def test_wgrad16v3_index_range(tune):
    tune("wgrad_v3", 1)
    test_wgrad16v4_index_range()


def test_conv16_blk_fwd_index_range():
    _cout1_case("blk")


# ---------------------------------------------------------------------------
# the frozen trunk at the headline step's 512 images
# ---------------------------------------------------------------------------
# largest per-image rel_l2 between a 64-image and a 16-image plan on the same
# images, measured on an MI355X (the test prints it again), per conv mode
TRUNK_SPREAD = {"native": 1.207e-2, "auto": 1.124e-2}
TRUNK_HEADROOM = 4


def _per_image_rel_l2(a, b):
    a, b = a.float().flatten(1), b.float().flatten(1)
    return (a - b).norm(dim=1) / b.norm(dim=1).clamp_min(1e-30)


def _trunk_plan(mode):
    from ncnet_amd.models import backbones as bb
    torch.manual_seed(0)
    t = bb.resnet_trunk("resnet101", "layer3").eval()
    for m in t.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.uniform_(-0.1, 0.1)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
    plan = bb.FrozenResNetPlan(bb.fold_frozen_bn(t.to(DEV)), torch.bfloat16)
    plan.use_graphs = False
    plan.conv_mode = mode
    return plan


@pytest.mark.parametrize("mode", ["native", "auto"])
def test_trunk_512_images_match_64_image_chunks(mode):
    """FrozenResNetPlan on 512 random 400 px images (the stem and layer-1
    activations, [512,200,200,64] and [512,100,100,256] bf16, are 2.6e9 bytes
    each) against the same images in 8 chunks of 64, per image.  'native':
    every conv on the NHWC kernels of csrc/conv2d.hip; 'auto' (the default, what
    bench.py runs): each 1x1 conv on them or on hipBLASLt with the fused
    epilogue of csrc/gemm_lt.hip, whichever it times faster at that shape.

    The plan picks conv2d tile variants (and 'auto' its GEMM) by the row count,
    so the bound is not bit equality: the largest per-image rel_l2 between a
    64-image and a 16-image plan on the same images (both below every threshold)
    measured TRUNK_SPREAD = 1.207e-2 ('native') / 1.124e-2 ('auto': its timed
    choices vary, 1.10e-2 .. 1.19e-2 over five processes; this is one of the
    lower ones) on an MI355X, and the bound is 4 x that, 4.83e-2 / 4.50e-2: headroom for
    tile-variant differences.  512 images against their 64-image chunks
    measured 1.207e-2 / 1.092e-2.  A wrapped index changes an image by order 1:
    image 500 computed from image 80's pixels (the mutation at the end)
    measured 0.81 -- with the per-image contrast and offset below; on plain
    unit-noise images this random-weight trunk's features differ by 4.5e-2
    only from image to image, which the bound could not tell from rounding."""
    plan = _trunk_plan(mode)
    bound = TRUNK_HEADROOM * TRUNK_SPREAD[mode]
    g = _gen(700)
    # every image with its own contrast (0.5 .. 2) and colour offset: the features
    # of two plain-noise images differ by 4.5e-2 only, inside the bound
    amp = 2 ** (2 * torch.rand(512, 1, 1, 1, device=DEV, generator=g) - 1)
    off = torch.randn(512, 3, 1, 1, device=DEV, generator=g)
    x = torch.randn(512, 3, 400, 400, device=DEV, generator=g) * amp + off
    with torch.no_grad():
        big = plan(x)
        assert torch.isfinite(big).all()
        worst = 0.0
        for c0 in range(0, 512, 64):
            e = _per_image_rel_l2(plan(x[c0:c0 + 64]), big[c0:c0 + 64])
            worst = max(worst, float(e.max()))
        # the spread the bound comes from, measured again on the first 64 images
        y64 = plan(x[:64])
        spread = max(float(_per_image_rel_l2(plan(x[c0:c0 + 16]), y64[c0:c0 + 16]).max()) for c0 in range(0, 64, 16))
        # mutation: image 500 from the pixels of image 80 (where a byte offset into the
        # layer-1 activation wrapped at 2^31 would read: 500 - 2^31 / 5.12e6 = 80.6)
        xm = x[448:].clone()
        xm[500 - 448] = x[80]
        mut = float(_per_image_rel_l2(plan(xm), big[448:])[500 - 448])
    print(f"trunk {mode}: 512 vs 64-image chunks {worst:.3e}; 64 vs 16-image plans {spread:.3e}; "
          f"bound {bound:.3e}; mutated image {mut:.3e}")
    assert worst < bound, worst
    assert mut > bound, mut
