"""One recipe per kernel, shared by the kernel's oracle test (tests/test_gpu_kernels.py,
tests/test_gpu_x3.py, at the test's shapes) and by the LDS poison table
(tests/lds_poison_cases.py, at the smallest shapes that still exercise the kernel).

A recipe is ``name(params...) -> (outputs, check)``:

- it draws its inputs (seed and draw order fixed inside),
- calls the extension through ``ncnet_amd.ops._ext.ext()``, looked up at call time, so that
  ``lds_poison_cases.poisoned`` can swap its proxy in,
- launches the kernel into outputs it owns, prefilled with NaN (floats) or -7 (integers),
- returns ``outputs``, a dict of the tensors the kernel wrote, and
- ``check()``, which runs the fp64 oracle and asserts finiteness and the bound(s).  Nothing
  synchronises or asserts on the outputs before ``check()`` is called.  Where an oracle test
  asserts more than the recipe (a mutation, a second reference), ``check()`` returns the
  operands and the reference it needs as a dict.

Nothing here touches the GPU at import time, and there are no test functions.

A new kernel gets one recipe here, one parametrized oracle test at the kernel's shapes and one
``_add`` line in tests/lds_poison_cases.py.
"""
import importlib

import torch

DEV = "cuda"
NAN = float("nan")


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------
def _ext_mod():
    from ncnet_amd.ops import _ext
    return _ext.ext()


def _ref():
    from ncnet_amd.ops import reference
    return reference


def bf(x):
    return x.to(torch.bfloat16).double()


def relerr(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def rel_l2(a, b):
    """||a - b|| / ||b||: robust to the few ReLU-mask flips that bf16 activations
    cause in a multi-layer composite (a flip moves one element by its full value)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _nan(shape, dtype=torch.float32):
    return torch.full(tuple(shape), NAN, device=DEV).to(dtype)


def _m7(shape, dtype=torch.int32):
    return torch.full(tuple(shape), -7, dtype=dtype, device=DEV)


def _finite(t):
    assert torch.isfinite(t.float()).all(), "an output element is NaN / Inf (never written, or stale LDS reached it)"


def _split(t):
    hi = t.to(torch.bfloat16)
    return hi, (t - hi.float()).to(torch.bfloat16)


def _pairs(t_nhwc):
    """fp32 [N, H, W, C] -> bf16 [N, H, W, 2C] = [hi | lo]."""
    return torch.cat(_split(t_nhwc), -1).contiguous()


def _unpair(p):
    c = p.shape[-1] // 2
    return p[..., :c].double() + p[..., c:].double()


def _f8q(t, s):
    """OCP e4m3 rounding at the power-of-two scale s (values returned unscaled, fp64)."""
    return (t.double() * s).float().clamp(-448, 448).to(torch.float8_e4m3fn).double() / s


def _pad_1ch(x5, ks, trans=False):
    """x5 [V, I, J, K, L] (any float dtype) -> padded bf16 planes via pad_planes: [V * I * J, PPL], or with
    trans the [V * K * L, PPL] planes of the A <-> B swapped volume."""
    V, I, J, K, L = x5.shape
    C = _ext_mod()
    kk, ll = (I, J) if trans else (K, L)
    _, ppl = C.pad_geom(kk, ll, ks)
    y = torch.zeros((V * (K * L if trans else I * J), ppl), dtype=torch.bfloat16, device=DEV)
    C.pad_planes(x5.reshape(V, I * J, K * L).contiguous(), y, kk, ll, ks, 1 if trans else 0)
    return y


def _cl(t):
    """[V, I, J, K, L, 16] channels-last -> the oracle's [V, 16, I, J, K, L]."""
    return t.permute(0, 5, 1, 2, 3, 4)


def _bias_relu_or_mask(z, epi, b, m):
    """The epilogues of the 16-channel forward kernels on the fp64 pre-activation z [V, 16, I, J, K, L]:
    1 bias + ReLU, 2 the ReLU mask of the previous activation m (the data gradient), else none."""
    if epi == 1:
        return torch.relu(z + b.double().view(1, 16, 1, 1, 1, 1))
    if epi == 2:
        return z * (_cl(m.double()) > 0)
    return z


def _plane_conv_sum(x, w, ks):
    """Group-plane mode in fp64: x [grp, V, I, J, K, L, 16], w [grp, 16, 16, ks, ks] (values as the kernel
    sees them) -> the sum over the groups of the plane convs, [V, 16, I, J, K, L]."""
    grp, V, I, J, K, L = x.shape[:6]
    xx = x.double().permute(0, 1, 2, 3, 6, 4, 5).reshape(grp, V * I * J, 16, K, L)
    yr = sum(torch.nn.functional.conv2d(xx[g], w[g].double(), padding=ks // 2) for g in range(grp))
    return yr.reshape(V, I, J, 16, K, L).permute(0, 3, 1, 2, 4, 5)


# ---------------------------------------------------------------------------
# Conv4d forward kernels
# ---------------------------------------------------------------------------
def _cout1_operands(shape, cin, ks, relu):
    """x [V, cin, ...], w, b of a Cout = 1 layer and x as 16 zero-padded bf16 channels, channels last."""
    V, I, J, K, L = shape
    x = torch.rand(V, cin, I, J, K, L, device=DEV)
    w = torch.randn(1, cin, ks, ks, ks, ks, device=DEV) * 0.05
    b = torch.randn(1, device=DEV) * 0.1 - (0.3 if relu else 0.0)
    xcl = torch.zeros(V, I, J, K, L, 16, device=DEV, dtype=torch.bfloat16)
    xcl[..., :cin] = x.permute(0, 2, 3, 4, 5, 1).to(torch.bfloat16)
    return x, w, b, xcl


def _cout1_oracle(x, w, b, relu):
    ref = _ref()
    yr = ref.conv4d(bf(x), ref.conv4d_weight_from_std(bf(w)), b.double())[:, 0]
    return torch.relu(yr) if relu else yr


def cout1_taps_fwd(shape, cin, relu):
    """Seed 3; x, w, b.  fp64 Conv4d oracle on the same bf16 operands, relerr < 1e-4.  check() returns the
    operands and the oracle."""
    from ncnet_amd.ops.packing import cout1_taps_weights
    torch.manual_seed(3)
    ks = 5
    x, w, b, xcl = _cout1_operands(shape, cin, ks, relu)
    wt = cout1_taps_weights(w).to(torch.bfloat16)
    y = _nan(shape)
    assert _ext_mod().cout1_taps_fwd(xcl, wt, b, y, ks, relu)

    def check():
        yr = _cout1_oracle(x, w, b, relu)
        _finite(y)
        assert relerr(y, yr) < 1e-4, relerr(y, yr)
        return {"xcl": xcl, "w": w, "wt": wt, "b": b, "yr": yr}
    return {"y": y}, check


def conv16_fwd(ks, epi, shape, seed=1):
    """Seed ``seed``; x, m, w, b.  conv16v4 / v3 (by the conv_v3 switch and the plane): fp64 oracle on the
    same bf16 operands, relerr < 4e-3 (the only difference is the final bf16 rounding of the stored
    output, 2^-9)."""
    from ncnet_amd.ops.packing import pack_w16
    ref = _ref()
    torch.manual_seed(seed)
    V, I, J, K, L = shape
    x = torch.rand(V, I, J, K, L, 16, device=DEV).to(torch.bfloat16)
    m = torch.randn(V, I, J, K, L, 16, device=DEV).to(torch.bfloat16)
    w_std = torch.randn(16, 16, ks, ks, ks, ks, device=DEV) * 0.05
    b = torch.randn(16, device=DEV) * 0.1
    y = _nan(x.shape, torch.bfloat16)
    _ext_mod().conv16_fwd(x, pack_w16(w_std), b if epi == 1 else None, m if epi == 2 else None, y, ks, epi)

    def check():
        z = ref.conv4d(_cl(x.double()), ref.conv4d_weight_from_std(bf(w_std)), None)
        _finite(y)
        e = relerr(_cl(y), _bias_relu_or_mask(z, epi, b, m))
        assert e < 4e-3, e
    return {"y": y}, check


def conv16_fwd_group_planes(ks, epi, shape, grp=2):
    """Seed 4; x, w, then m (epi 2) or b (epi 1).  conv16v2 in group-plane mode (grp input groups), or with
    grp 0 on all (di, dj) planes; epilogue 0 (none), 1, 2 or 4 (planar fp32).  fp64 math on the same bf16
    operands, relerr < 1e-2 (bf16 output), < 1e-4 (planar fp32)."""
    from ncnet_amd.ops.packing import pack_w16, pack_w16_planes
    ref = _ref()
    torch.manual_seed(4)
    V, I, J, K, L = shape
    if grp:
        x = torch.rand(grp, V, I, J, K, L, 16, device=DEV).to(torch.bfloat16)
        w = (torch.randn(grp, 16, 16, ks, ks, device=DEV) * 0.05).to(torch.bfloat16).float()
        wp = pack_w16_planes(w)
    else:
        x = torch.rand(V, 16, I, J, K, L, device=DEV).permute(0, 2, 3, 4, 5, 1).contiguous().to(torch.bfloat16)
        w = torch.randn(16, 16, ks, ks, ks, ks, device=DEV) * 0.05
        wp = pack_w16(w)
    m = torch.randn(V, I, J, K, L, 16, device=DEV).to(torch.bfloat16) if epi == 2 else None
    b = torch.randn(16, device=DEV) * 0.1 if epi == 1 else None
    y = _nan((16, V, I, J, K, L)) if epi == 4 else _nan((V, I, J, K, L, 16), torch.bfloat16)
    _ext_mod().conv16_fwd(x, wp.to(torch.bfloat16), b, m, y, ks, epi)

    def check():
        if grp:
            yr = _plane_conv_sum(x, w, ks)
        else:
            yr = ref.conv4d(_cl(x.double()), ref.conv4d_weight_from_std(bf(w)), None)
        _finite(y)
        if epi == 4:
            assert relerr(y.permute(1, 0, 2, 3, 4, 5), yr) < 1e-4
        else:
            assert relerr(_cl(y), _bias_relu_or_mask(yr, epi, b, m)) < 1e-2
    return {"y": y}, check


def conv16_blk_fwd(ks, shape, cin, relu):
    """Seed 1; x, w, b.  fp64 Conv4d oracle on the same bf16 operands, relerr < 1e-4."""
    from ncnet_amd.ops.packing import blk_out_weights, pack_w16_planes
    torch.manual_seed(1)
    x, w, b, xcl = _cout1_operands(shape, cin, ks, relu)
    y = _nan(shape)
    _ext_mod().conv16_blk_fwd(xcl, pack_w16_planes(blk_out_weights(w)), b, y, ks, relu)

    def check():
        _finite(y)
        assert relerr(y, _cout1_oracle(x, w, b, relu)) < 1e-4
    return {"y": y}, check


def conv16f8_fwd(ks, shape, grp):
    """Seed 21; x, w, b, then (group-plane mode) wp, x2.  fp64 math on the same e4m3 values.  grp 0: bias +
    ReLU -> fp8 output, within rel. L2 0.04 (e4m3 rounding, 3 mantissa bits); grp > 0: the planar fp32
    output of group-plane mode, relerr < 1e-4."""
    from ncnet_amd.ops.packing import pack_w16, pack_w16_planes
    ref = _ref()
    F8 = torch.float8_e4m3fn
    torch.manual_seed(21)
    V, I, J, K, L = shape
    wsc = 64.0
    x = (torch.rand(V, I, J, K, L, 16, device=DEV) * 2).to(F8)
    w = (torch.randn(16, 16, ks, ks, ks, ks, device=DEV) * 0.05).to(torch.bfloat16).float()
    b = torch.randn(16, device=DEV) * 0.1
    if not grp:
        wq = (pack_w16(w).float() * wsc).to(F8)
        y = _nan((V, I, J, K, L, 16), F8)
        _ext_mod().conv16f8_fwd(x, wq, b, y, ks, 1, 1.0 / wsc)

        def check():
            wr = (w * wsc).to(F8).double() / wsc          # the exact fp8 weight values used
            yr = ref.conv4d(_cl(x.double()), ref.conv4d_weight_from_std(wr), b.double())
            _finite(y)
            assert rel_l2(y.float(), torch.relu(yr).permute(0, 2, 3, 4, 5, 1)) < 0.04
        return {"y": y.view(torch.uint8)}, check
    wp = (torch.randn(grp, 16, 16, ks, ks, device=DEV) * 0.05).to(torch.bfloat16).float()
    wpq = (pack_w16_planes(wp).float() * wsc).to(F8)
    x2 = (torch.rand(grp, V, I, J, K, L, 16, device=DEV) * 2).to(F8)
    z = _nan((16, V, I, J, K, L))
    _ext_mod().conv16f8_fwd(x2, wpq, None, z, ks, 4, 1.0 / wsc)

    def check():
        zr = _plane_conv_sum(x2, (wp * wsc).to(F8).double() / wsc, ks)
        _finite(z)
        assert relerr(z.permute(1, 0, 2, 3, 4, 5), zr) < 1e-4
    return {"z": z}, check


def conv16_fwd_x3(grp, plane, epi, ks, vij):
    """Seed 3; x, w, then bias (epi 1) or m (epi 2).  One conv16_fwd_x3 launch (group-plane or full (di, dj)
    sum): hi + lo against the fp64 emulator, rel. L2 < 2e-5."""
    from ncnet_amd.ops.packing import pack_w16, pack_w16_planes
    torch.manual_seed(3)
    V, I, J = vij
    shp = (V, I, J, plane, plane)
    x = torch.randn(((grp,) if grp else ()) + shp + (16,), device=DEV)
    xh, xl = _split(x)
    if grp:
        w, pack = torch.randn(grp, 16, 16, ks, ks, device=DEV) * 0.05, pack_w16_planes
    else:
        w, pack = torch.randn(16, 16, ks, ks, ks, ks, device=DEV) * 0.05, pack_w16
    whi = w.to(torch.bfloat16).float()
    wp2 = torch.stack((pack(whi), pack(w - whi))).contiguous()
    bias = torch.rand(16, device=DEV) * 0.1 if epi == 1 else None
    m = torch.randn(shp + (16,), device=DEV).to(torch.bfloat16) if epi == 2 else None
    yh, yl = _nan(shp + (16,), torch.bfloat16), _nan(shp + (16,), torch.bfloat16)
    _ext_mod().conv16_fwd_x3(xh, xl, wp2, bias, m, yh, yl, ks, epi)

    def check():
        from tests import emu_ext
        eh = torch.empty(shp + (16,), dtype=torch.float64)
        el = torch.empty_like(eh)
        emu_ext.conv16_fwd_x3(xh.cpu(), xl.cpu(), wp2.cpu(), None if bias is None else bias.cpu(),
                              None if m is None else m.cpu(), eh, el, ks, epi)
        _finite(yh), _finite(yl)
        err = rel_l2(yh.double().cpu() + yl.double().cpu(), eh + el)
        assert err < 2e-5, err
    return {"yh": yh, "yl": yl}, check


# ---------------------------------------------------------------------------
# weight gradients of the 16 -> 16 layer
# ---------------------------------------------------------------------------
def wgrad16(variant, ks, shape):
    """Seed 11; x, g.  The wgrad16 kernels (variant 3: the sliding ring v3 / v4, 2: v2 per plane offset) in
    full mode: autograd of the fp64 oracle, relerr < 1e-3; and the plane-only mode against the (P, P)
    slice of the same gradient."""
    nc = importlib.import_module("ncnet_amd.ops.nc.layers")
    ref = _ref()
    torch.manual_seed(11)
    V, I, J, K, L = shape
    x = torch.rand(V, I, J, K, L, 16, device=DEV).to(torch.bfloat16)
    g = torch.randn(V, I, J, K, L, 16, device=DEV).to(torch.bfloat16)
    if variant == 3:
        assert nc.wgrad_v3_ok(shape, ks)
        ng = nc.wgrad_v3_groups(shape, ks)
    else:
        ng = nc.wgrad_groups(ks, nc._nitems(shape))
    part = _nan((2 * ng, ks * ks, ks * ks, 16, 16))
    partb = _nan((2 * ng, 16))
    _ext_mod().wgrad16(x, g, part, partb, ks, 0, variant)

    def check():
        wr = torch.zeros(ks, 16, 16, ks, ks, ks, device=DEV, dtype=torch.float64, requires_grad=True)
        yr = ref.conv4d(_cl(x.double()), wr, None)
        (yr * _cl(g.double())).sum().backward()
        dstd = ref.conv4d_weight_to_std(wr.grad)           # [co, ci, di, dj, dk, dl]
        _finite(part), _finite(partb)
        assert relerr(nc._reduce_wgrad16(part.sum(0), ks, 16, 16), dstd) < 1e-3
        assert relerr(partb.sum(0), g.double().sum(dim=(0, 1, 2, 3, 4))) < 1e-3
        # plane-only: the (P, P) offset.  A further launch, made here and so outside the poison sweep
        # (check() runs after poisoned() has put the real extension back; the sweep compares ``outputs``).
        sp, sbp = nc.wgrad16_partials(_ext_mod(), x, g, ks, True)
        P = ks // 2
        assert relerr(sp[0].permute(2, 1, 0).reshape(16, 16, ks, ks), dstd[:, :, P, P]) < 1e-3
        assert relerr(sbp, partb.sum(0)) < 1e-5
    return {"part": part, "partb": partb}, check


def wgrad16p(ks, shape, nx, ng):
    """Seed 2; x, g.  Double-buffered plane-only weight gradient against the fp64 plane-conv definition
    dW[tap][ci][co] = sum X[vox + tap] G[vox], relerr < 1e-4."""
    import torch.nn.functional as F
    torch.manual_seed(2)
    V, I, J, K, L = shape
    x = (torch.rand((nx,) + shape + (16,), device=DEV) - 0.3).to(torch.bfloat16)
    g = torch.randn((ng,) + shape + (16,), device=DEV).to(torch.bfloat16)
    part = _nan((64, nx * ng, ks * ks, 16, 16))
    partb = _nan((64, nx * ng, 16))
    _ext_mod().wgrad16p(x, g, part, partb, ks)

    def check():
        _finite(part), _finite(partb)
        s, sb = part.sum(0), partb.sum(0)
        P = ks // 2
        for a in range(nx):
            for n in range(ng):
                xx = x[a].double().reshape(V * I * J, K, L, 16).permute(0, 3, 1, 2)
                gg = g[n].double().reshape(V * I * J, K, L, 16).permute(0, 3, 1, 2)
                xp = F.pad(xx, (P, P, P, P))
                want = torch.stack([torch.einsum("nckl,nokl->co", xp[:, :, dk:dk + K, dl:dl + L], gg)
                                    for dk in range(ks) for dl in range(ks)])   # [tap, ci, co]
                assert relerr(s[a * ng + n], want) < 1e-4
                assert relerr(sb[a * ng + n], gg.sum(dim=(0, 2, 3))) < 1e-4
    return {"part": part, "partb": partb}, check


# ---------------------------------------------------------------------------
# the 1-channel layers on padded planes
# ---------------------------------------------------------------------------
def conv1x16(ks, shape, epi):
    """Seed 3; x, w, b, m.  1 -> 16 Conv4d on zero-padded 1-channel planes: fp64 oracle, relerr < 1e-2."""
    from ncnet_amd.ops.packing import pack_w1x
    ref = _ref()
    torch.manual_seed(3)
    V, I, J, K, L = shape
    x = torch.rand(V, I, J, K, L, device=DEV).to(torch.bfloat16)
    w = torch.randn(16, 1, ks, ks, ks, ks, device=DEV) * 0.05
    b = torch.randn(16, device=DEV) * 0.1
    m = torch.randn(V, I, J, K, L, 16, device=DEV).to(torch.bfloat16)
    y = _nan((V, I, J, K, L, 16), torch.bfloat16)
    assert _ext_mod().conv1x16(_pad_1ch(x, ks), pack_w1x(w), b if epi == 1 else None, m if epi == 2 else None, y, ks,
                               epi)

    def check():
        z = ref.conv4d(x.double().unsqueeze(1), ref.conv4d_weight_from_std(bf(w)), None)   # [V, 16, I, J, K, L]
        _finite(y)
        assert relerr(_cl(y), _bias_relu_or_mask(z, epi, b, m)) < 1e-2
    return {"y": y}, check


def conv1x16_x3(ks, shape):
    """Seed 7; x, w, b.  conv1x16's bf16x3 mode (epi 1 | 4) as ops/nc/x3.py launches it: hi + lo against
    the fp64 Conv4d of the unsplit fp32 operands.  Bound: rel. L2 < 2e-4, what test_gpu_x3.py::
    test_x3_fused_matches_fp64 holds the stack built on this launch to."""
    from ncnet_amd.ops.packing import pack_w1x
    ref = _ref()
    torch.manual_seed(7)
    V, I, J, K, L = shape
    x = torch.rand(shape, device=DEV)
    w = torch.randn(16, 1, ks, ks, ks, ks, device=DEV) * (0.5 / ks ** 2)
    b = torch.rand(16, device=DEV) * 0.1
    xh, xl = _split(x)
    xs = torch.stack((_pad_1ch(xh, ks), _pad_1ch(xl, ks))).contiguous()
    whi = w.to(torch.bfloat16).float()
    wa = torch.stack((pack_w1x(whi), pack_w1x(w - whi))).to(torch.bfloat16).contiguous()
    a = _nan((2, V, I, J, K, L, 16), torch.bfloat16)
    assert _ext_mod().conv1x16(xs, wa, b, None, a, ks, 1 | 4)

    def check():
        xq = (xh.double() + xl.double()).unsqueeze(1)
        wq = whi.double() + (w - whi).to(torch.bfloat16).double()
        want = torch.relu(ref.conv4d(xq, ref.conv4d_weight_from_std(wq), b.double()))
        _finite(a)
        err = rel_l2(_cl(a[0].double() + a[1].double()), want)
        assert err < 2e-4, err
    return {"a": a}, check


def wgrad1x16(ks, shape, G, bias):
    """Seed 21; x1, d.  Weight gradient with a 1-channel operand straight from padded planes: autograd of
    the fp64 oracle for both uses, relerr < 1e-4 each: the first layer (D = output gradient, X1 = input:
    R = dW) and the Cout = 1 last layer (D = input, X1 = output gradient: dW = R with all four kernel
    axes flipped)."""
    ref = _ref()
    torch.manual_seed(21)
    V, I, J, K, L = shape
    x1 = torch.rand(V, I, J, K, L, device=DEV).to(torch.bfloat16)
    d = torch.randn(V, I, J, K, L, 16, device=DEV).to(torch.bfloat16)
    nt = ks * ks
    part = _nan((G, nt, 32, 16))
    partb = _nan((G, 16)) if bias else None
    assert _ext_mod().wgrad1x16(d, _pad_1ch(x1, ks), part, partb, ks)

    def check():
        _finite(part)
        R = part.sum(0)[:, :nt, :]                                   # [tap, combo, c]
        # first layer: y[co] = conv(x1; W[co, 0]), dL/dy = d  ->  dW[co, 0, di, dj, dk, dl]
        wr = torch.zeros(ks, 16, 1, ks, ks, ks, device=DEV, dtype=torch.float64, requires_grad=True)
        yr = ref.conv4d(x1.double().unsqueeze(1), wr, None)
        (yr * _cl(d.double())).sum().backward()
        want = ref.conv4d_weight_to_std(wr.grad)[:, 0].reshape(16, nt, nt)      # [co, combo, tap]
        assert relerr(R.permute(2, 1, 0), want) < 1e-4
        # last layer: y = conv(d; W[0, ci]), dL/dy = x1  ->  dW[0, ci, t] = R[2P - t][ci]
        w3 = torch.zeros(ks, 1, 16, ks, ks, ks, device=DEV, dtype=torch.float64, requires_grad=True)
        y3 = ref.conv4d(_cl(d.double()), w3, None)
        (y3 * x1.double().unsqueeze(1)).sum().backward()
        want3 = ref.conv4d_weight_to_std(w3.grad)[0]                               # [ci, di, dj, dk, dl]
        got3 = R.permute(2, 1, 0).reshape(16, ks, ks, ks, ks).flip(1, 2, 3, 4)
        assert relerr(got3, want3) < 1e-4
        if bias:
            _finite(partb)
            assert relerr(partb.sum(0), d.double().sum(dim=(0, 1, 2, 3, 4))) < 1e-4
    outs = {"part": part}
    if bias:
        outs["partb"] = partb
    return outs, check


def pad_planes_transposed():
    """Seed 4; x.  pad_planes trans = 1 (the kernel stages a tile in LDS) writes the planes of the A <-> B
    swapped volume: equal to the plain padding of the swapped volume."""
    torch.manual_seed(4)
    x = torch.randn(2, 9, 11, 9, 11, device=DEV)
    a = _pad_1ch(x, 5, trans=True)

    def check():
        assert torch.equal(a, _pad_1ch(x.permute(0, 3, 4, 1, 2).contiguous(), 5))
    return {"planes": a}, check


# ---------------------------------------------------------------------------
# fused InLoc NC stack
# ---------------------------------------------------------------------------
def _nc_k3_params():
    """w1, w2 (std layout), b1, b2 of the 1 -> 16 -> 1, k = 3 stack and the weights in the reference layout."""
    ref = _ref()
    w1 = torch.randn(16, 1, 3, 3, 3, 3, device=DEV) * 0.2
    w2 = torch.randn(1, 16, 3, 3, 3, 3, device=DEV) * 0.1
    b1, b2 = torch.rand(16, device=DEV) * 0.1 - 0.03, torch.rand(1, device=DEV) * 0.1
    return w1, w2, b1, b2, [ref.conv4d_weight_from_std(w1), ref.conv4d_weight_from_std(w2)]


def nc_fused_k3(shape, cfg, seed):
    """Seed ``seed``; w1, w2, b1, b2, x0.  The fused InLoc NeighConsensus kernel against the fp64 oracle with
    bf16 rounding of x0, the weights and the hidden activation, relerr < 2e-3.  cfg = (R, IR, TK, TL), or
    None for the production choice (fused_tiles)."""
    from ncnet_amd.engine import quantized_oracle as qo
    nc = importlib.import_module("ncnet_amd.ops.nc.fused")
    torch.manual_seed(seed)
    w1, w2, b1, b2, ws = _nc_k3_params()
    x0 = torch.rand(shape, device=DEV).to(torch.bfloat16)
    wts = nc._fused_weights(ws, [b1, b2])
    y = _nan(shape)
    tk, tl, R, IR = nc.fused_tiles(*shape) if cfg is None else (cfg[2], cfg[3], cfg[0], cfg[1])
    _ext_mod().nc_fused_k3(x0, *wts, y, R, IR, tk, tl)

    def check():
        yr = qo.nc_stack(x0.double().unsqueeze(1), [w1.double(), w2.double()], [b1.double(), b2.double()])
        _finite(y)
        assert relerr(y, yr.squeeze(1)) < 2e-3
    return {"y": y}, check


def nc_fused_k3_f8(shape, cfg):
    """Seed 41; w1, w2, b1, b2, x0 (MutualMatching-like: [0, 1], most entries small).  The e4m3 fused NC
    kernel against fp64 math with the same e4m3 roundings (x0 * sx, weights * sw, hidden * sh): relerr
    < 2e-2 and rel. L2 < 2e-3 (a hidden value on the other side of an e4m3 rounding boundary in fp32 vs
    fp64 moves by one e4m3 ulp, 6 %: a few such flips, not O(1) errors).  check() returns the unquantised
    operands."""
    nc = importlib.import_module("ncnet_amd.ops.nc.fused")
    ref = _ref()
    torch.manual_seed(41)
    w1, w2, b1, b2, ws = _nc_k3_params()
    x0 = (torch.rand(shape, device=DEV) ** 3).to(torch.bfloat16)
    tens, (sx, inv1, sh, inv2) = nc._fused_weights_f8_build(ws, [b1, b2])
    y = _nan(shape)
    tk, tl, R, IR = nc.fused_tiles(*shape) if cfg is None else (cfg[2], cfg[3], cfg[0], cfg[1])
    _ext_mod().nc_fused_k3_f8(x0, *tens, y, R, IR, tk, tl, sx, inv1, sh, inv2)

    def check():
        sw1, sw2 = 1.0 / (inv1 * sx), 1.0 / (inv2 * sh)
        xq = _f8q(x0, sx).unsqueeze(1)
        h = torch.relu(ref.conv4d(xq, ref.conv4d_weight_from_std(_f8q(w1, sw1))) + b1.double().view(1, -1, 1, 1, 1, 1))
        h = _f8q(h, sh)
        yr = torch.relu(ref.conv4d(h, ref.conv4d_weight_from_std(_f8q(w2, sw2))) + b2.double().view(1, -1, 1, 1, 1, 1))
        _finite(y)
        assert relerr(y, yr.squeeze(1)) < 2e-2 and rel_l2(y, yr.squeeze(1)) < 2e-3
        return {"x0": x0, "ws": ws, "bs": [b1, b2]}
    return {"y": y}, check


# ---------------------------------------------------------------------------
# correlation GEMMs (poison table only: the f16 tests draw other operands and batch maps)
# ---------------------------------------------------------------------------
def corr_gemm(kind, M, N, K, out16):
    """Seed 1; a, b.  fp64 GEMM of the same operand values.  fp32 C: rel. L2 < 1e-5 (test_gpu_f16.py::
    test_corr_gemm_f16; exact products, fp32 sums), fp8 operands relerr < 1e-4 (test_gpu_kernels.py::
    test_fp8_l2norm_and_correlation); 16-bit C: 1e-3 (f16) / 4e-3 (bf16), test_gpu_f16.py::
    test_corr_gemm_16bit_out.  fp8 operands need K % 16 == 0."""
    torch.manual_seed(1)
    dt = {"f16": torch.float16, "bf16": torch.bfloat16, "fp8": torch.float8_e4m3fn}[kind]
    a = (torch.randn(2, M, K, device=DEV) * 0.25).to(dt)
    b = (torch.randn(2, N, K, device=DEV) * 0.25).to(dt)
    scale = 0.5 if kind == "fp8" else 1.0
    amap = torch.tensor([1, 0], device=DEV, dtype=torch.int32)
    bmap = torch.tensor([0, 0], device=DEV, dtype=torch.int32)
    cdt = torch.float32 if not out16 else torch.float16 if kind == "f16" else torch.bfloat16
    c = _nan((2, M, N), cdt)
    _ext_mod().corr_gemm(a, b, c, amap, bmap, scale)

    def check():
        want = scale * torch.bmm(a.float().double()[amap.long()], b.float().double()[bmap.long()].transpose(1, 2))
        _finite(c)
        if out16:
            assert rel_l2(c, want) < (1e-3 if kind == "f16" else 4e-3)
        elif kind == "fp8":
            assert relerr(c, want) < 1e-4
        else:
            assert rel_l2(c, want) < 1e-5
    return {"c": c}, check


def corr_gemm_pool2(kind, K):
    """Seed 2; fa, fb.  The fused 2x2x2x2 max-pool against pooling the full volume of an fp64 GEMM: rel. L2
    < 1e-5 for f16 / bf16 (test_gpu_f16.py::test_corr_pool2_f16_matches_unfused), fp8 relerr < 1e-4
    (test_gpu_kernels.py::test_fp8_l2norm_and_correlation)."""
    from ncnet_amd.ops.correlation import FP8, FP8_FEAT_SCALE, correlation_pool2
    ref = _ref()
    torch.manual_seed(2)
    hA, wA, hB, wB = 12, 16, 10, 14
    fa = torch.nn.functional.normalize(torch.randn(1, hA * wA, K, device=DEV), dim=2)
    fb = torch.nn.functional.normalize(torch.randn(1, hB * wB, K, device=DEV), dim=2)
    if kind == "fp8":
        fa, fb = (fa * FP8_FEAT_SCALE).to(FP8), (fb * FP8_FEAT_SCALE).to(FP8)
    else:
        dt = torch.float16 if kind == "f16" else torch.bfloat16
        fa, fb = fa.to(dt), fb.to(dt)
    val, code = correlation_pool2(fa, fb, hA, wA, hB, wB, packed=True)

    def check():
        s = 1.0 / FP8_FEAT_SCALE ** 2 if kind == "fp8" else 1.0
        full = (torch.bmm(fa.double(), fb.double().transpose(1, 2)) * s).float().view(1, 1, hA, wA, hB, wB)
        want, _ = ref.maxpool4d(full, 2)
        _finite(val)
        if kind == "fp8":
            assert relerr(val, want) < 1e-4
        else:
            assert rel_l2(val, want) < 1e-5
    return {"val": val, "code": code}, check


# ---------------------------------------------------------------------------
# feature-trunk convolutions
# ---------------------------------------------------------------------------
def conv2d_nhwc(cin, cout, k, stride, pad, res, relu, shape, dt, seed):
    """Seed ``seed``; x, w, b, r.  NHWC implicit-GEMM conv (+ bias, + residual, ReLU; the kernel by the
    conv2d_variant switch and the size) against F.conv2d in fp64 on the 16-bit inputs, relerr < 1e-2."""
    torch.manual_seed(seed)
    cl = torch.channels_last
    x = torch.randn(shape[0], cin, shape[1], shape[2], device=DEV).to(dt).contiguous(memory_format=cl)
    w = (torch.randn(cout, cin, k, k, device=DEV) * 0.05).to(dt).contiguous(memory_format=cl)
    b = torch.randn(cout, device=DEV)
    ho, wo = (shape[1] + 2 * pad - k) // stride + 1, (shape[2] + 2 * pad - k) // stride + 1
    r = torch.randn((shape[0], cout, ho, wo), device=DEV).to(dt).contiguous(memory_format=cl) if res else None
    y = torch.full((shape[0], cout, ho, wo), NAN, dtype=dt, device=DEV).contiguous(memory_format=cl)
    _ext_mod().conv2d_nhwc(x, w, b, r, y, stride, pad, 1 if relu else 0)

    def check():
        yr = torch.nn.functional.conv2d(x.double(), w.double(), b.double(), stride, pad)
        if res:
            yr = yr + r.double()
        if relu:
            yr = torch.relu(yr)
        _finite(y)
        assert relerr(y, yr) < 1e-2, relerr(y, yr)
    return {"y": y}, check


def conv2d_nhwc_x3(cin, cout, k, stride, pad, res, relu, shape):
    """Seed 5; x, w, b, r.  conv2d_nhwc_v3 X3 mode ([hi | lo] bf16 pairs in and out): the fp64 conv of the
    pairs, rel. L2 < 3e-5."""
    torch.manual_seed(5)
    n, h, w = shape
    x = torch.randn(n, h, w, cin, device=DEV)
    wt = torch.randn(cout, cin, k, k, device=DEV) * (1.0 / (cin * k * k) ** 0.5)
    b = torch.randn(cout, device=DEV) * 0.1
    wcl = wt.permute(0, 2, 3, 1)
    whi = wcl.to(torch.bfloat16)
    w3 = torch.cat((whi, whi, (wcl - whi.float()).to(torch.bfloat16)), -1).contiguous()
    xp = _pairs(x)
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    r = _pairs(torch.randn((n, ho, wo, cout), device=DEV)) if res else None
    y = _nan((n, ho, wo, 2 * cout), torch.bfloat16)
    _ext_mod().conv2d_nhwc_x3(xp, w3, b, r, y, stride, pad, 1 if relu else 0)

    def check():
        want = torch.nn.functional.conv2d(_unpair(xp).permute(0, 3, 1, 2), wt.double(), b.double(), stride, pad)
        want = want.permute(0, 2, 3, 1)
        if res:
            want = want + _unpair(r)
        if relu:
            want = torch.relu(want)
        _finite(y)
        err = rel_l2(_unpair(y), want)
        assert err < 3e-5, err
    return {"y": y}, check


# ---------------------------------------------------------------------------
# MutualMatching (poison table only: test_gpu_kernels.py::_mutual_matching_vs_fp64 goes through the
# autograd function on torch.rand volumes, these launch the kernels on volumes without ties)
# ---------------------------------------------------------------------------
def _mm_inputs(shape6, seed):
    from tests import volume_stats_ref as VR
    c = VR.distinct(shape6, seed, 0.0, 1.0).to(DEV)
    V, _, I, J, K, L = shape6
    c3 = c.reshape(V, I * J, K * L).contiguous()
    return c, c3, c3.amax(2).contiguous(), c3.amax(1).contiguous()


def mm_apply(shape6, mode):
    """MutualMatching forward.  fp32 output: the fp64 reference, relerr < 1e-5 (the bound of
    test_gpu_kernels.py::_mutual_matching_vs_fp64); f16 straight / transposed outputs: rel. L2 < 1e-3
    (test_gpu_f16.py::test_mm_nc_input_f16); PAD mode: equal to the pad_planes passes
    (test_gpu_fusion.py::test_mm_apply_padded_planes_equal_pad_passes)."""
    from ncnet_amd.ops.mutual import EPS
    ref = _ref()
    C = _ext_mod()
    c, c3, rmax, cmax = _mm_inputs(shape6, 14)
    V, R, Cc = c3.shape
    I, J = shape6[2], shape6[3]
    out = _nan(c3.shape)
    outs = {"out": out}
    if mode == "plain":
        C.mm_apply(c3, rmax, cmax, out, None, None, EPS)
    elif mode == "f16t":
        outs["x"], outs["xt"] = _nan((V, R, Cc), torch.float16), _nan((V, Cc, R), torch.float16)
        C.mm_apply(c3, rmax, cmax, out, outs["x"], outs["xt"], EPS)
    else:
        _, ppl = C.pad_geom(I, J, 5)
        planes = _nan((2 * V * R, ppl), torch.bfloat16)
        C.mm_apply(c3, rmax, cmax, out, planes[:V * R], planes[V * R:], EPS, [5, I, J])
        outs["planes"] = planes

    def check():
        m = ref.mutual_matching(c.double()).reshape(V, R, Cc)
        _finite(out)
        assert relerr(out, m) < 1e-5
        if mode == "f16t":
            assert rel_l2(outs["x"], m) < 1e-3 and rel_l2(outs["xt"], m.transpose(1, 2)) < 1e-3
        if mode == "pad":                      # square volumes: (K, L) = (I, J)
            o5 = out.reshape(V, I, J, I, J)
            assert torch.equal(outs["planes"], torch.cat((_pad_1ch(o5, 5), _pad_1ch(o5, 5, trans=True))))
    return outs, check


def mm_bwd(shape6, one_pass):
    """MutualMatching backward, one pass (mm_bwd_sums2d) or the separate row / column kernels: fp64
    autograd, relerr < 1e-4 (the bound of test_gpu_kernels.py::_mutual_matching_vs_fp64)."""
    from ncnet_amd.ops.mutual import EPS
    ref = _ref()
    c, c3, rmax, cmax = _mm_inputs(shape6, 14)
    rarg, carg = c3.argmax(2).int().contiguous(), c3.argmax(1).int().contiguous()
    g = torch.randn(c.shape, generator=torch.Generator().manual_seed(15)).to(DEV)
    gc = _nan(c3.shape)
    _ext_mod().mm_bwd(c3, g.reshape(c3.shape).contiguous(), rmax, rarg, cmax, carg, gc, EPS, one_pass)

    def check():
        cr = c.double().requires_grad_(True)
        ref.mutual_matching(cr).backward(g.double())
        _finite(gc)
        assert relerr(gc.reshape(c.shape), cr.grad) < 1e-4
    return {"gc": gc}, check
