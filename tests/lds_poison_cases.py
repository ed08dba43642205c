"""Case table of the LDS poison tier (tests/test_gpu_lds_poison.py) and of its
completeness check (tests/test_lds_poison_cases_cpu.py).

LDS is not cleared between dispatches, so a kernel that reads an LDS word it
did not write in the same launch sees what an earlier kernel left there.  Each
case launches one kernel (through its binding) on the inputs of the kernel's
existing test, with ``lds_poison`` run immediately before every launch: the
outputs must be bit-identical under every pattern of PATTERNS, and the outputs
of the NaN pattern must pass the oracle and the bound of the existing test
(named in each case's comment).

A case is ``fn() -> (outputs, check)``: ``outputs`` a dict of the tensors the
kernel wrote (prefilled with NaN, or -7 for integers, where the caller owns
them), ``check()`` the oracle assertions on them.  ``fn`` calls the extension
through ``ncnet_amd.ops._ext.ext()``; the test swaps a poisoning proxy in (see
``poisoned``).  Nothing here touches the GPU at import time.

This module holds the harness, the table and the exemptions.  The recipes of
the Conv4d, weight-gradient, padded-plane, fused NC, trunk-conv, correlation
GEMM and MutualMatching kernels live in tests/kernel_cases.py, where the
kernels' oracle tests call the same functions at their own shapes; the cases
defined below take their inputs and oracle from a module their test shares
(tests/volume_stats_ref.py, tests/strong_loss_cases.py, tests/pv_scene.py,
tests/test_gpu_pnp.py).  A new kernel gets one recipe in tests/kernel_cases.py,
one parametrized oracle test at the kernel's shapes, and one ``_add`` line here
at the smallest shapes that still exercise the kernel.

Before a kernel joins the table its source was read for integers that come out
of LDS and become an index or an address: such a word must have been written
earlier in the same launch, else a poisoned value would be a wild address.
Findings: the voxel-offset tables of wgrad16v2 / wgrad16p (``voff``), the
kploss_bwd table / chains / hit lists and the p3p_ransac wave totals are all
written before their first read in every launch (p3p's inlier list lives in
global memory); no other kernel keeps an index in LDS.
"""
import contextlib
import dataclasses
import functools

import torch

from tests.kernel_cases import (DEV, _ext_mod, _finite, _m7, _nan, _ref, relerr,
                                conv1x16, conv1x16_x3, conv2d_nhwc, conv2d_nhwc_x3, conv16_blk_fwd, conv16_fwd,
                                conv16_fwd_group_planes, conv16_fwd_x3, conv16f8_fwd, corr_gemm, corr_gemm_pool2,
                                cout1_taps_fwd, mm_apply, mm_bwd, nc_fused_k3, nc_fused_k3_f8, pad_planes_transposed,
                                wgrad1x16, wgrad16, wgrad16p)

# zeros; NaN as fp32, as a bf16 pair, as an fp16 pair and as fp64 (byte 0x7F: the
# e4m3 NaN; a huge positive int32); fp32 -inf, the bf16 pair (-inf, 0) -- the
# identity value of the statistics kernels
PATTERNS = (("zeros", 0x00000000), ("nan", 0x7FC07FC0), ("neginf", 0xFF800000))
ROUNDS = 4          # lds_poison workgroups per CU (the harness check runs with the same)
LDS_ALL = 163840

# bindings that launch nothing
_NO_LAUNCH = {"pad_geom", "set_tuning", "lds_poison", "lds_probe"}


class _Poisoning:
    """The extension module with lds_poison(pattern) before every kernel launch."""

    def __init__(self, real, pattern):
        self._real, self._pattern = real, pattern

    def __getattr__(self, name):
        f = getattr(self._real, name)
        if name in _NO_LAUNCH or not callable(f):
            return f

        def call(*a, **kw):
            self._real.lds_poison(self._pattern, ROUNDS)
            return f(*a, **kw)
        return call


@contextlib.contextmanager
def poisoned(pattern: int):
    """Inside: every binding reached through ``_ext.ext()`` runs right after an
    LDS fill with ``pattern`` on the same stream."""
    from ncnet_amd.ops import _ext
    real = _ext.ext()
    _ext._C = _Poisoning(real, pattern)
    try:
        yield
    finally:
        _ext._C = real


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    launchers: tuple          # ncnet_* launchers (csrc/launchers.h) the case launches under poison
    fn: object
    tuning: tuple = ()        # ((config.RUNTIME field, value), ...) set through the ``tune`` fixture


CASES: list = []


def _add(cid, launchers, fn, *args, tuning=(), **kw):
    CASES.append(Case(cid, tuple("ncnet_" + n for n in launchers), functools.partial(fn, *args, **kw), tuple(tuning)))


# launchers of LDS-using source files that have no case, each with its reason
EXEMPT = {
    "ncnet_set_tuning": "host only: launches nothing",
    "ncnet_pad_geom": "host only: launches nothing",
    "ncnet_pv_pmax": "host only: launches nothing",
    "ncnet_lds_poison": "the poison itself; the harness check of test_gpu_lds_poison.py runs it",
    "ncnet_lds_probe": "the canary: reads uninitialised LDS on purpose; run by the harness check",
    "ncnet_debug_selftest": "its kernel (csrc/epilogue.hip) declares no LDS",
    "ncnet_bias_act": "its kernel (csrc/epilogue.hip) declares no LDS",
    "ncnet_maxpool_bias_act": "its kernel (csrc/epilogue.hip) declares no LDS",
    "ncnet_stem_im2col_x3": "its kernel (csrc/epilogue.hip) declares no LDS",
    "ncnet_maxpool_x3": "its kernel (csrc/epilogue.hip) declares no LDS",
    "ncnet_x3_to_f32": "its kernel (csrc/epilogue.hip) declares no LDS",
    "ncnet_gather_bf16": "its kernel (csrc/epilogue.hip) declares no LDS",
    "ncnet_l2norm_rows": "its kernel (csrc/corr.hip) declares no LDS (wave shuffles only)",
    "ncnet_l2norm_rows_bwd": "its kernel (csrc/corr.hip) declares no LDS (wave shuffles only)",
    "ncnet_pv_desc_err": "its kernel (csrc/pv.hip) declares no LDS",
    "ncnet_p3p_solve": "its kernel (csrc/pnp.hip) declares no LDS",
    "ncnet_stats_rows": "its kernel (csrc/volume.hip) declares no LDS (one wave per row)",
    "ncnet_match_candidates": "its kernel (csrc/volume.hip) declares no LDS",
    "ncnet_softmax_max_bwd": "its kernel (csrc/volume.hip) declares no LDS",
    "ncnet_maxpool4d": "its kernel (csrc/volume.hip) declares no LDS",
}


# ---------------------------------------------------------------------------
# Conv4d forward kernels
# ---------------------------------------------------------------------------
for _shape, _cin in (((1, 1, 1, 25, 25), 16), ((1, 2, 4, 25, 25), 16), ((2, 4, 3, 25, 25), 10)):
    for _relu in (0, 1):
        _add(f"cout1_taps_fwd-{'x'.join(map(str, _shape))}-relu{_relu}", ["cout1_taps_fwd"], cout1_taps_fwd, _shape, _cin,
             _relu)


for _ks in (5, 3):
    for _epi in (1, 2):
        # 25 x 25 planes: conv16v4 (conv_v3 0) and the general conv16v3 (conv_v3 1); 11 x 13: conv16v3
        _add(f"conv16_fwd-v4-k{_ks}-epi{_epi}-1x3x4x25x25", ["conv16_fwd"], conv16_fwd, _ks, _epi, (1, 3, 4, 25, 25),
             tuning=(("conv_v3", 0),))
        _add(f"conv16_fwd-v3-k{_ks}-epi{_epi}-1x3x4x25x25", ["conv16_fwd"], conv16_fwd, _ks, _epi, (1, 3, 4, 25, 25),
             tuning=(("conv_v3", 1),))
        _add(f"conv16_fwd-v3-k{_ks}-epi{_epi}-1x3x2x11x13", ["conv16_fwd"], conv16_fwd, _ks, _epi, (1, 3, 2, 11, 13))
        for _shape in ((1, 3, 4, 25, 25), (1, 3, 2, 11, 13)):
            _add(f"conv16_fwd-v2-groups-k{_ks}-epi{_epi}-{'x'.join(map(str, _shape))}", ["conv16_fwd"],
                 conv16_fwd_group_planes, _ks, _epi, _shape)
_add("conv16_fwd-v2-groups-k5-epi4-1x3x2x11x13", ["conv16_fwd"], conv16_fwd_group_planes, 5, 4, (1, 3, 2, 11, 13))


_add("conv16_blk_fwd-k5-1x5x6x9x7-relu1", ["conv16_blk_fwd"], conv16_blk_fwd, 5, (1, 5, 6, 9, 7), 16, 1)
_add("conv16_blk_fwd-k3-1x5x6x9x7-relu0", ["conv16_blk_fwd"], conv16_blk_fwd, 3, (1, 5, 6, 9, 7), 10, 0)


for _ks in (5, 3):
    _add(f"conv16f8_fwd-k{_ks}-1x3x2x11x13-epi1", ["conv16f8_fwd"], conv16f8_fwd, _ks, (1, 3, 2, 11, 13), 0)
    _add(f"conv16f8_fwd-k{_ks}-1x3x2x11x13-groups-epi4", ["conv16f8_fwd"], conv16f8_fwd, _ks, (1, 3, 2, 11, 13), 2)


_add("conv16_fwd_x3-v4-k5-25-epi1", ["conv16_fwd"], conv16_fwd_x3, 0, 25, 1, 5, (1, 2, 6))
_add("conv16_fwd_x3-v2-k5-9-epi2", ["conv16_fwd"], conv16_fwd_x3, 0, 9, 2, 5, (1, 2, 6))
_add("conv16_fwd_x3-v2-groups-k5-9-epi1", ["conv16_fwd"], conv16_fwd_x3, 2, 9, 1, 5, (1, 2, 6))


# ---------------------------------------------------------------------------
# weight gradients of the 16 -> 16 layer
# ---------------------------------------------------------------------------
for _shape in ((1, 3, 4, 25, 25), (1, 5, 7, 7, 9)):
    _s = "x".join(map(str, _shape))
    for _ks in (5, 3):
        _add(f"wgrad16-v2-k{_ks}-{_s}", ["wgrad16"], wgrad16, 2, _ks, _shape)
        _add(f"wgrad16-v3-k{_ks}-{_s}", ["wgrad16v3"], wgrad16, 3, _ks, _shape, tuning=(("wgrad_v3", 1),))
    # wgrad16v4: the compile-time 25 x 25 plane (wgrad_v3 0, the default)
_add("wgrad16-v4-k5-1x3x4x25x25", ["wgrad16v3"], wgrad16, 3, 5, (1, 3, 4, 25, 25), tuning=(("wgrad_v3", 0),))
_add("wgrad16-v4-k3-1x3x4x25x25", ["wgrad16v3"], wgrad16, 3, 3, (1, 3, 4, 25, 25), tuning=(("wgrad_v3", 0),))


_add("wgrad16p-k5-1x3x4x25x25-ngg2", ["wgrad16p"], wgrad16p, 5, (1, 3, 4, 25, 25), 1, 2)
_add("wgrad16p-k5-1x3x4x25x25-nsets2", ["wgrad16p"], wgrad16p, 5, (1, 3, 4, 25, 25), 2, 1)
_add("wgrad16p-k3-1x5x7x7x9-ngg2", ["wgrad16p"], wgrad16p, 3, (1, 5, 7, 7, 9), 1, 2)


# ---------------------------------------------------------------------------
# the 1-channel layers on padded planes
# ---------------------------------------------------------------------------
for _ks, _shape in ((5, (1, 2, 6, 25, 25)), (5, (1, 3, 4, 20, 20)), (3, (1, 4, 5, 25, 25))):
    _s = "x".join(map(str, _shape))
    for _epi in (1, 2):
        _add(f"conv1x16-k{_ks}-{_s}-epi{_epi}", ["conv1x16", "pad_planes"], conv1x16, _ks, _shape, _epi)
    for _bias in (True, False):
        _add(f"wgrad1x16-k{_ks}-{_s}-{'bias' if _bias else 'nobias'}", ["wgrad1x16", "pad_planes"], wgrad1x16, _ks,
             _shape, 7, _bias)
_add("conv1x16_x3-k5-1x2x6x25x25", ["conv1x16", "pad_planes"], conv1x16_x3, 5, (1, 2, 6, 25, 25))


_add("pad_planes-transposed", ["pad_planes"], pad_planes_transposed)


# ---------------------------------------------------------------------------
# fused InLoc NC stack
# ---------------------------------------------------------------------------
for _cfg in (None, (3, 4, 6, 7), (5, 2, 9, 11)):
    _c = "auto" if _cfg is None else "x".join(map(str, _cfg))
    _add(f"nc_fused_k3-2x9x13x11x14-{_c}", ["nc_fused_k3"], nc_fused_k3, (2, 9, 13, 11, 14), _cfg, 21)
    _add(f"nc_fused_k3_f8-2x9x13x11x14-{_c}", ["nc_fused_k3_f8"], nc_fused_k3_f8, (2, 9, 13, 11, 14), _cfg)
# the > 80 KB configuration: one 16-wave workgroup per CU (R = 24, 15 x 20 tiles)
_add("nc_fused_k3-one-wide-workgroup", ["nc_fused_k3"], nc_fused_k3, (1, 6, 26, 17, 22), (24, 4, 15, 20), 23)


# ---------------------------------------------------------------------------
# correlation GEMMs
# ---------------------------------------------------------------------------
for _v2 in (0, 1):
    _t = (("corr_v2", _v2),)
    for _kind in ("bf16", "f16", "fp8"):
        # 77 x 131 x 40: ragged single tiles (K 48 for fp8, K % 16 == 0; the v2 rings take K % 32 == 0,
        # fp8 K % 128 == 0, and fall back to v1 otherwise: K 64 / 128 there); 300 x 290: several tiles both ways
        _K = ((128 if _kind == "fp8" else 64) if _v2 else (48 if _kind == "fp8" else 40))
        _add(f"corr_gemm-v{_v2 + 1}-{_kind}-77x131x{_K}", ["corr_gemm"], corr_gemm, _kind, 77, 131, _K, False, tuning=_t)
        _add(f"corr_gemm-v{_v2 + 1}-{_kind}-300x290", ["corr_gemm"], corr_gemm, _kind, 300, 290,
             1024 if _kind == "fp8" else 256, False, tuning=_t)
    _add(f"corr_gemm-v{_v2 + 1}-bf16-out16-77x131", ["corr_gemm"], corr_gemm, "bf16", 77, 131, 64 if _v2 else 40, True,
         tuning=_t)
    _add(f"corr_gemm-v{_v2 + 1}-bf16-out16-300x290", ["corr_gemm"], corr_gemm, "bf16", 300, 290, 256, True, tuning=_t)
    for _kind, _K in (("bf16", 128), ("f16", 128), ("fp8", 256)):
        _add(f"corr_gemm_pool2-v{_v2 + 1}-{_kind}", ["corr_gemm_pool2"], corr_gemm_pool2, _kind, _K, tuning=_t)


# ---------------------------------------------------------------------------
# feature-trunk convolutions
# ---------------------------------------------------------------------------
_BF, _HF = torch.bfloat16, torch.float16
_add("conv2d_nhwc-v1-64x64-3x3", ["conv2d_nhwc"], conv2d_nhwc, 64, 64, 3, 1, 1, False, True, (2, 19, 23), _BF, 17)
_add("conv2d_nhwc-v1-128x256-1x1-residual", ["conv2d_nhwc"], conv2d_nhwc, 128, 256, 1, 1, 0, True, True, (2, 19, 23), _BF,
     17)
_add("conv2d_nhwc-v2-64x64-3x3-residual", ["conv2d_nhwc"], conv2d_nhwc, 64, 64, 3, 1, 1, True, True, (2, 19, 23), _BF, 17,
     tuning=(("conv2d_variant", 2),))
_add("conv2d_nhwc-v2-256x256tile-64x256-1x1", ["conv2d_nhwc"], conv2d_nhwc, 64, 256, 1, 1, 0, False, True, (2, 20, 20), _BF,
     23, tuning=(("conv2d_variant", 4),))
_add("conv2d_nhwc-v3-128x64-3x3-f16", ["conv2d_nhwc"], conv2d_nhwc, 128, 64, 3, 1, 1, False, True, (1, 20, 20), _HF, 18,
     tuning=(("conv2d_variant", 3),))
_add("conv2d_nhwc-v3-128x128-3x3-residual", ["conv2d_nhwc"], conv2d_nhwc, 128, 128, 3, 1, 1, True, True, (3, 23, 19), _BF,
     18, tuning=(("conv2d_variant", 3),))
_add("conv2d_nhwc_x3-64x64-3x3", ["conv2d_nhwc_x3"], conv2d_nhwc_x3, 64, 64, 3, 1, 1, False, True, (2, 37, 29))
_add("conv2d_nhwc_x3-256x1024-1x1-residual", ["conv2d_nhwc_x3"], conv2d_nhwc_x3, 256, 1024, 1, 1, 0, True, True,
     (2, 25, 25))


def reduce_cols():
    """test_gpu_fusion.py::test_reduce_cols_matches_torch_layouts (the kernel merges its four row slices
    through LDS): the fp64 sums in the checkpoint layout, allclose(rtol 1e-5, atol 1e-4)."""
    import importlib
    ref = _ref()
    nc = importlib.import_module("ncnet_amd.ops.nc.layers")
    torch.manual_seed(1)
    ks = 5
    p16 = torch.randn(20, ks * ks, ks * ks, 16, 16, device=DEV)
    pb = torch.randn(20, 16, device=DEV)
    p1x = torch.randn(13, ks * ks, 32, 16, device=DEV)
    f16 = lambda t: ref.conv4d_weight_from_std(nc._reduce_wgrad16(t, ks, 16, 16))  # noqa: E731
    f_last = lambda t: t[:, :25, :16].reshape((ks,) * 4 + (16,)).flip(0, 1, 2, 3).permute(2, 4, 3, 0, 1).unsqueeze(1)  # noqa: E731
    got = nc.reduce_partials([(p16, ("g16", ks), f16), (pb, None, None), (p1x, ("gl", ks), f_last)])

    def check():
        want = [f16(p16.double().sum(0)), pb.double().sum(0), f_last(p1x.double().sum(0))]
        for g, w in zip(got, want):
            assert g.shape == w.shape
            assert torch.allclose(g.double(), w, rtol=1e-5, atol=1e-4), (g.double() - w).abs().max()
    return {f"seg{i}": g for i, g in enumerate(got)}, check


_add("reduce_cols-three-segments", ["reduce_cols"], reduce_cols)


# ---------------------------------------------------------------------------
# correlation-volume kernels
# ---------------------------------------------------------------------------
def _stats_outputs(V, R, C):
    return {"rmx": _nan((V, R)), "rse": _nan((V, R)), "cmx": _nan((V, C)), "cse": _nan((V, C)),
            "rarg": _m7((V, R)), "carg": _m7((V, C))}


def _stats_check(o, which, rows, cols, sum_kind):
    """tests/test_gpu_volume_stats.py::_check: max bit-equal, first argmax equal, se within 1e-5 relative,
    the plain sum within 1e-5 * sum |x|."""
    for d, st in (("r", rows), ("c", cols)):
        if d not in which:
            continue
        mx, arg, s = o[d + "mx"].cpu(), o[d + "arg"].cpu(), o[d + "se"].cpu()
        assert torch.equal(mx, st["max"].float()), (d, "max")
        assert torch.equal(arg.long(), st["arg"]), (d, "argmax")
        if sum_kind == 1:
            err = float(((s.double() - st["se"]).abs() / st["se"]).max())
            assert torch.isfinite(s).all() and err <= 1e-5, (d, "se", err)
        elif sum_kind == 2:
            err = float(((s.double() - st["sum"]).abs() / st["abs_sum"]).max())
            assert torch.isfinite(s).all() and err <= 1e-5, (d, "sum", err)


def stats2d(family, shape, sum_kind):
    from tests import volume_stats_ref as VR
    xc, rows, cols = VR.case(family, shape)
    x = xc.to(DEV)
    o = _stats_outputs(*shape)
    assert _ext_mod().stats2d(x, o["rmx"], o["rarg"], o["rse"], o["cmx"], o["carg"], o["cse"], sum_kind)
    return o, lambda: _stats_check(o, "rc", rows, cols, sum_kind)


def stats_cols(family, shape, sum_kind):
    from tests import volume_stats_ref as VR
    xc, rows, cols = VR.case(family, shape)
    x = xc.to(DEV)
    o = _stats_outputs(*shape)
    _ext_mod().stats_cols(x, o["cmx"], o["carg"], o["cse"], sum_kind)
    o = {k: v for k, v in o.items() if k[0] == "c"}
    return o, lambda: _stats_check(o, "c", rows, cols, sum_kind)


for _shape in ((2, 70, 260), (2, 77, 263)):
    _s = "x".join(map(str, _shape))
    for _fam, _sk in (("ties", 1), ("neg", 2)):
        _add(f"stats2d-{_s}-{_fam}-sum{_sk}", ["stats2d"], stats2d, _fam, _shape, _sk)
        _add(f"stats_cols-{_s}-{_fam}-sum{_sk}", ["stats_cols"], stats_cols, _fam, _shape, _sk)
# 1, 2 (the default) and 4 sub-tiles of 64 rows per block need R >= 1024; C = 7: scalar loads, 8: 16-byte loads
for _rt in (1, 2, 4):
    for _shape in ((1, 1030, 7), (1, 1030, 8)):
        _add(f"stats2d-{'x'.join(map(str, _shape))}-rt{_rt}", ["stats2d"], stats2d, "ties", _shape, 1,
             tuning=(("s2d_rt", _rt),))
# chunked stats_cols (few wide columns: partials + merge)
_add("stats_cols-1x70x7500-chunked", ["stats_cols"], stats_cols, "peaky", (1, 70, 7500), 1)

for _shape6 in ((2, 1, 7, 10, 13, 20), (2, 1, 7, 11, 1, 263)):        # [V, R, C] = (2, 70, 260) and (2, 77, 263)
    _s = f"2x{_shape6[2] * _shape6[3]}x{_shape6[4] * _shape6[5]}"
    _add(f"mm_apply-{_s}-plain", ["mm_apply"], mm_apply, _shape6, "plain")
    _add(f"mm_apply-{_s}-f16-transposed", ["mm_apply"], mm_apply, _shape6, "f16t")
    _add(f"mm_bwd-{_s}-one-pass", ["mm_bwd"], mm_bwd, _shape6, True)
    _add(f"mm_bwd-{_s}-two-pass", ["mm_bwd"], mm_bwd, _shape6, False)
_add("mm_apply-3x49x49-pad", ["mm_apply", "pad_planes"], mm_apply, (3, 1, 7, 7, 7, 7), "pad")   # PAD mode: square volumes


def combine(V, R, C):
    """test_gpu_nc_stages.py::test_combine_nonsquare: y = z1 + z2^T (allclose), gz = bf16(g * (z > 0)) exactly."""
    torch.manual_seed(13)
    z = torch.randn(2 * V * R * C, device=DEV)
    g = torch.randn(V, R, C, device=DEV)
    y = _nan((V, R, C))
    gz = _nan((2 * V * R * C,), torch.bfloat16)
    E = _ext_mod()
    E.combine_fwd(z, y, R, C)
    E.combine_bwd(g, z, gz, R, C)

    def check():
        z1, z2 = z[:V * R * C].view(V, R, C), z[V * R * C:].view(V, C, R)
        assert torch.allclose(y, z1 + z2.transpose(1, 2))
        assert torch.equal(gz[:V * R * C].view(V, R, C), (g * (z1 > 0)).to(torch.bfloat16))
        assert torch.equal(gz[V * R * C:].view(V, C, R), (g.transpose(1, 2) * (z2 > 0)).to(torch.bfloat16))
    return {"y": y, "gz": gz}, check


def transpose(V, R, C, dtype):
    """The tiled transpose (tests/emu_ext.py: y = x^T per volume), exact."""
    torch.manual_seed(19)
    x = torch.randn(V, R, C, device=DEV).to(dtype)
    y = _nan((V, C, R), dtype)
    _ext_mod().transpose(x, y)

    def check():
        assert torch.equal(y, x.transpose(1, 2).contiguous())
    return {"y": y}, check


def score_sum(family, shape, norm):
    """test_gpu_volume_stats.py::test_score_sum_vs_fp64: the value from the fp64 reference statistics,
    within 1e-5 max(1, |value|)."""
    from ncnet_amd.ops import loss as Lm
    from tests import volume_stats_ref as VR
    ref = _ref()
    xc, rows, cols = VR.case(family, shape)
    g = torch.Generator().manual_seed(17 + norm)
    wr, wc = torch.randn(shape[0], generator=g), torch.randn(shape[0], generator=g)
    rmax, _, rse, cmax, _, cse = Lm._row_col_stats(xc.to(DEV), norm)
    val = _nan(())
    _ext_mod().score_sum(rmax, rse, cmax, cse, wr.to(DEV), wc.to(DEV), val, norm, ref.L1_EPS)

    def check():
        def sc(st):
            return 1.0 / st["se"] if norm == 1 else st["max"] / (st["sum"] + ref.L1_EPS) if norm == 2 else st["max"]
        want = float((wr.double().view(-1, 1) * sc(rows)).sum() + (wc.double().view(-1, 1) * sc(cols)).sum())
        assert abs(float(val) - want) <= 1e-5 * max(1.0, abs(want)), (float(val), want)
    return {"val": val.reshape(1)}, check


for _V, _R, _C in ((2, 70, 260), (2, 77, 263)):
    _s = f"{_V}x{_R}x{_C}"
    _add(f"combine-{_s}", ["combine_fwd", "combine_bwd"], combine, _V, _R, _C)
    _add(f"transpose-{_s}-fp32", ["transpose"], transpose, _V, _R, _C, torch.float32)
    _add(f"transpose-{_s}-bf16", ["transpose"], transpose, _V, _R, _C, torch.bfloat16)
    for _norm in (0, 1, 2):
        _add(f"score_sum-{_s}-norm{_norm}", ["score_sum"], score_sum, "neg", (_V, _R, _C), _norm)


# ---------------------------------------------------------------------------
# keypoint-supervised loss
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _kp_oracle(name):
    from tests.strong_loss_cases import make_case
    ref = _ref()
    x, kp = make_case(name)
    xd = x.double().requires_grad_(True)
    loss = ref.keypoint_ce(xd, *kp)
    loss.backward()
    return float(loss.detach()), xd.grad.detach()


def kploss(name):
    """test_gpu_strong_loss.py::test_loss_and_gradient_match_fp64_oracle / test_backward_writes_every_element:
    loss within 1e-5 max(1, |loss|), gradient relerr < 1e-4, zero exactly where the oracle is zero."""
    from tests.strong_loss_cases import CASES as KP, make_case
    (B, N, hA, wA, hB, wB) = KP[name][0]
    x, kp = make_case(name, DEV)
    x3 = x.reshape(B, hA * wA, hB * wB).contiguous()
    o = {"cells": _m7((B, N, 8)), "wts": _nan((B, N, 8)), "valid": _m7((B, N)), "lse": _nan((B, N, 2)),
         "term": _nan((B, N, 2)), "out": _nan((2,)), "gx": _nan(x3.shape)}
    C = _ext_mod()
    C.kploss_fwd(x3, *kp, hA, wA, hB, wB, o["cells"], o["wts"], o["valid"], o["lse"], o["term"], o["out"])
    C.kploss_bwd(x3, o["cells"], o["wts"], o["valid"], o["lse"], o["out"][1:], o["gx"])

    def check():
        lr, gr = _kp_oracle(name)
        for k in ("wts", "lse", "term", "out", "gx"):
            _finite(o[k])
        assert int(o["cells"].min()) >= 0 and int(o["valid"].min()) >= 0
        assert abs(float(o["out"][0]) - lr) < 1e-5 * max(1.0, abs(lr))
        assert torch.equal(o["gx"].cpu().reshape(gr.shape) == 0, gr == 0)
        assert relerr(o["gx"].reshape(gr.shape), gr) < 1e-4
    return o, check


for _name in ("small", "edge"):
    _add(f"kploss-{_name}", ["kploss_fwd", "kploss_bwd"], kploss, _name)


# ---------------------------------------------------------------------------
# localization back end
# ---------------------------------------------------------------------------
def p3p_ransac(n, outliers, seed, max_iters):
    """test_gpu_pnp.py::test_consensus_40_percent_outliers / test_consensus_many_outliers: the consensus
    criteria of _check_consensus (pose error < 1e-2, > 95 % of the inliers, mask = the numpy inlier test)."""
    import numpy as np
    from tests import test_gpu_pnp as T
    P, rays, Xw, out = T._problem(np.random.default_rng(seed), n, outliers)
    from ncnet_amd.eval.localization_gpu import key_to_int64
    off = torch.tensor([0, n], dtype=torch.int32, device=DEV)
    k = torch.tensor([key_to_int64(seed)], dtype=torch.int64, device=DEV)
    rounds = _m7((1,))
    Pg, ninl, mask = _ext_mod().p3p_ransac_batch(torch.tensor(rays.T, dtype=torch.float64, device=DEV).contiguous(),
                                                 torch.tensor(Xw.T, dtype=torch.float64, device=DEV).contiguous(), off, k,
                                                 float(T.THR), max_iters, 0.999, 20, rounds)

    def check():
        T._check_consensus(P, rays, Xw, out, Pg.cpu().numpy()[0], mask.cpu().numpy().astype(bool), int(ninl[0]))
    return {"P": Pg, "ninl": ninl, "mask": mask, "rounds": rounds}, check


_add("p3p_ransac_batch-200-points", ["p3p_ransac_batch"], p3p_ransac, 200, 0.4, 2, 2000)
_add("p3p_ransac_batch-2000-points", ["p3p_ransac_batch"], p3p_ransac, 2000, 0.7, 21, 10000)   # > 1024: tiled staging


@functools.lru_cache(maxsize=None)
def _pv_cloud():
    import numpy as np
    from tests import pv_scene as S
    _, rgb, xyz = S.scene()
    extra = np.array([[np.nan, 0.0, 4.0], [np.inf, np.inf, np.inf], [0.0, 0.0, -4.0], [0.0, 0.0, 1e-10],
                      [1e30, -1e30, 4.0]])
    rgb, xyz = np.concatenate([rgb, np.full((5, 3), -7.0, np.float32)]), np.concatenate([xyz, extra])
    names = ("true", "bad", "near")
    return rgb, xyz, names, {n: S.render_cpu(rgb, xyz, S.POSES[n]) for n in names}


def pv_render():
    """test_gpu_pv.py::test_render_equals_torch: the 60 x 80 scene at 3 poses, equal to the CPU z-buffer."""
    import numpy as np
    from tests import pv_scene as S
    rgb, xyz, names, want = _pv_cloud()
    xyz_d = torch.as_tensor(np.ascontiguousarray(xyz), dtype=torch.float64, device=DEV)
    rgb_d = torch.as_tensor(np.ascontiguousarray(rgb), dtype=torch.float32, device=DEV)
    kp = torch.stack([S.kp_matrix(S.POSES[n]) for n in names]).contiguous().to(DEV)
    synth, flag, winner = _ext_mod().pv_render(xyz_d, rgb_d, kp, S.H, S.W)

    def check():
        s, f, w = synth.cpu().numpy(), flag.cpu().numpy(), winner.cpu().numpy()
        assert int((w >= S.N_POINTS).sum()) == 0 and not (s == -7.0).any()
        assert np.array_equal(w >= 0, f)
        for c, n in enumerate(names):
            assert np.array_equal(f[c], want[n][1]), n
            assert np.array_equal(s[c], want[n][0], equal_nan=True), n
    return {"synth": synth, "flag": flag, "winner": winner}, check


_add("pv_render-60x80-3-poses", ["pv_render"], pv_render)
