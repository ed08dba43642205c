"""fp32-accurate NeighConsensus on the bf16 MFMA kernels ("bf16x3"): every
Conv4d is three bf16 convs,
conv(h, w) ~ conv(h_hi, w_hi) + conv(h_hi, w_lo) + conv(h_lo, w_hi), where
x_hi = bf16(x) and x_lo = bf16(x - x_hi), summed in fp32.  This is the
reference's fp32 NeighConsensus (lib/conv4d.py:23-24, lib/model.py:110-113)
to ~16 mantissa bits, at 3x the bf16 cost; used by ImMatchNet(corr_dtype='fp32').

``neigh_consensus_x3`` (inference) and ``NeighConsensusX3Fn`` (training) run
three launches per conv with fp32 activations between layers;
``NeighConsensusX3FusedFn`` runs each conv as one launch on hi / lo pairs;
``NeighConsensusMixedFn`` is its forward with the bf16 backward of ``train``."""
from __future__ import annotations

import contextlib

import torch

from .. import _ext
from .. import reference as ref
from ..packing import (blk_out_weights, ij_groups, ij_in_weights, ij_out_weights, pack_w16, pack_w1x, pack_w16_planes,
                       plane_dgrad_weights, transpose_for_dgrad)
from .layers import _pad_bias, _std, combine_1ch, conv_layer, ijpack, interleave, layer_wgrad, planar_to_blocks
from .train import _join_side, _OnSide, _pad_1ch, _stack_bwd, _stack_packs, _streams, _wgrad1x, fast1x_ok, unswap_gx


def _split(t: torch.Tensor, lo_dtype=torch.bfloat16):
    """fp32 t -> (hi, lo): hi = bf16(t), lo = t - hi in ``lo_dtype``."""
    hi = t.to(torch.bfloat16)
    return hi, (t - hi.float()).to(lo_dtype)


def _wsplit(w: torch.Tensor):
    """Weights: both parts stay fp32 tensors (hi holds bf16 values, lo is
    rounded when it is packed)."""
    hi, lo = _split(w, torch.float32)
    return hi.float(), lo


def _to_repr(t: torch.Tensor, c: int) -> torch.Tensor:
    """Activation/gradient (1-channel [V,...] or planar [C, V, ...]) -> the
    layer representation of the bf16 kernels (1-channel bf16 / bf16 blocks)."""
    return t.to(torch.bfloat16).contiguous() if c == 1 else planar_to_blocks(t)


def _split_repr(t: torch.Tensor, c: int):
    hi, lo = _split(t)
    return _to_repr(hi, c), _to_repr(lo, c)


def _sum3(f, a, b):
    """f(a_hi, b_hi) + f(a_hi, b_lo) + f(a_lo, b_hi), called and summed in this
    order; ``a`` and ``b`` are (hi, lo) pairs."""
    return f(a[0], b[0]) + f(a[0], b[1]) + f(a[1], b[0])


def _conv_x3(h_hi, h_lo, w: torch.Tensor, cin: int, cout: int) -> torch.Tensor:
    return _sum3(lambda h, wp: conv_layer(h, wp, cin, cout, relu=False, f32=True), (h_hi, h_lo), _wsplit(w))


def _layer_x3(h: torch.Tensor, w: torch.Tensor, b: torch.Tensor, cin: int, cout: int):
    """One fp32-accurate Conv4d + ReLU on an fp32 input -> (the input's hi and lo
    parts in the layer representation, the fp32 activation)."""
    hh, hl = _split_repr(h, cin)
    z = _conv_x3(hh, hl, w, cin, cout)
    z = z + (b.float().view(-1, *([1] * (z.dim() - 1))) if cout > 1 else b.float().view(1))
    return hh, hl, torch.relu(z)


def _stack_fwd_x3(x0: torch.Tensor, ws, bs, channels) -> torch.Tensor:
    """x0 fp32 [V,I,J,K,L] -> last layer ReLU output fp32 ([V,...] or planar [C, V, ...])."""
    h, cin = x0, 1
    for w_ref, b, cout in zip(ws, bs, channels):
        h, cin = _layer_x3(h, _std(w_ref), b, cin, cout)[2], cout
    return h


def neigh_consensus_x3(x: torch.Tensor, weights, biases, channels, symmetric: bool = True) -> torch.Tensor:
    """fp32-accurate inference NeighConsensus on the bf16 MFMA kernels (no autograd)."""
    V, _, I, J, K, L = x.shape
    cl = channels[-1]
    xf = x.reshape(V, I, J, K, L).float().contiguous()

    def as_out(z, shape):
        return z.reshape((V, 1) + shape) if cl == 1 else z.transpose(0, 1).reshape((V, cl) + shape)

    y = as_out(_stack_fwd_x3(xf, weights, biases, channels), (I, J, K, L))
    if symmetric:
        xt = xf.permute(0, 3, 4, 1, 2).contiguous()
        y2 = as_out(_stack_fwd_x3(xt, weights, biases, channels), (K, L, I, J))
        y = y + y2.permute(0, 1, 4, 5, 2, 3)
    return y.contiguous()


def _wgrad_x3(C, kind, h_hi, h_lo, g_hi, g_lo, ks, cin, cout) -> torch.Tensor:
    """dW = X.G summed as Xhi.Ghi + Xhi.Glo + Xlo.Ghi on the bf16 wgrad kernels."""
    def xin(h):
        return ijpack(C, h, ks, 1) if cin == 1 else h

    def gsp(g):
        return ijpack(C, g, ks, -1) if cout == 1 and kind == "1out" else None

    return _sum3(lambda x, g: layer_wgrad(C, kind, x, g, gsp(g), ks, cin, cout)[0], (xin(h_hi), xin(h_lo)), (g_hi, g_lo))


class NeighConsensusX3Fn(torch.autograd.Function):
    """fp32-accurate TRAINING NeighConsensus: every forward conv, data gradient
    and weight gradient is a bf16x3 split on the bf16 MFMA kernels (3x the bf16
    cost), activations and gradients stay fp32 between layers.  The reference
    trains in fp32 (lib/conv4d.py, train.py); this mode reproduces it where the
    weak loss's positive/negative signal is below bf16 resolution (random-init
    trunks, scripts/train_quality.py)."""

    @staticmethod
    def forward(ctx, x, symmetric, kinds, channels, *params):
        ws = [_std(w) for w in params[0::2]]
        bs = params[1::2]
        V, _, I, J, K, L = x.shape
        x0 = x.reshape(V, I, J, K, L).float()
        if symmetric:
            x0 = torch.cat((x0, x0.permute(0, 3, 4, 1, 2)), 0) if (I, J) == (K, L) else None
        if x0 is None:
            raise NotImplementedError("fp32 NC training: symmetric mode needs square volumes")
        h, cin, saved = x0.contiguous(), 1, []
        for w, b, cout in zip(ws, bs, channels):
            hh, hl, h = _layer_x3(h, w, b, cin, cout)
            saved += [hh, hl, h]
            cin = cout
        ctx.kinds, ctx.channels, ctx.symmetric, ctx.dims = kinds, channels, symmetric, (V, I, J, K, L)
        ctx.save_for_backward(*params, *saved)
        cl = channels[-1]
        y = h.reshape((-1, 1) + tuple(h.shape[1:])) if cl == 1 else h.transpose(0, 1)
        if symmetric:
            y1, y2 = y[:V], y[V:]
            y = y1 + y2.permute(0, 1, 4, 5, 2, 3)
        return y.contiguous()

    @staticmethod
    def backward(ctx, gy):
        C = _ext.ext()
        nl = len(ctx.kinds)
        params = ctx.saved_tensors[:2 * nl]
        saved = ctx.saved_tensors[2 * nl:]
        ws = [_std(w) for w in params[0::2]]
        V, I, J, K, L = ctx.dims
        cl = ctx.channels[-1]
        g = gy.float()
        if ctx.symmetric:
            g = torch.cat((g, g.permute(0, 1, 4, 5, 2, 3)), 0)
        g = g[:, 0] if cl == 1 else g.transpose(0, 1)        # d/d(last activation), fp32
        dws, dbs = [None] * nl, [None] * nl
        gx = None
        for li in range(nl - 1, -1, -1):
            hh, hl, a = saved[3 * li:3 * li + 3]
            cout = ctx.channels[li]
            cin = 1 if li == 0 else ctx.channels[li - 1]
            ks = ws[li].shape[-1]
            gp = g * (a > 0)                                   # d/d(pre-activation)
            dbs[li] = gp.sum().reshape(1) if cout == 1 else gp.reshape(cout, -1).sum(1)
            gh, gl = _split_repr(gp, cout)
            dws[li] = ref.conv4d_weight_from_std(_wgrad_x3(C, ctx.kinds[li], hh, hl, gh, gl, ks, cin, cout))
            if li > 0 or ctx.needs_input_grad[0]:
                g = _conv_x3(gh, gl, transpose_for_dgrad(ws[li]), cout, cin)
        if ctx.needs_input_grad[0]:
            g = g.reshape(2 * V if ctx.symmetric else V, I, J, K, L) if ctx.symmetric else g.reshape(V, I, J, K, L)
            if ctx.symmetric:
                g = g[:V] + g[V:].permute(0, 3, 4, 1, 2)
            gx = g.reshape(V, 1, I, J, K, L)
        return (gx, None, None, None, *interleave(dws, dbs))


# ---------------------------------------------------------------------------
# fp32-accurate training on the fused bf16x3 kernels (csrc/conv4d_fwd.hip
# EPI_X3).  Every activation and gradient between layers is kept as a hi / lo
# bf16 pair (x = hi + lo to ~16 mantissa bits); each Conv4d is ONE launch that
# runs the three phases (X_hi, W_hi), (X_hi, W_lo), (X_lo, W_hi) into its fp32
# accumulators and writes the split result from its epilogue (bias + ReLU, or
# the previous layer's ReLU mask for data gradients).  Weight gradients are the
# three (X, G) products on the bf16 wgrad kernels, summed.  Covers the
# 1 -> (16 ->)* 1 stacks with KS 3 / 5 (every NC-Net config); others use
# NeighConsensusX3Fn's per-conv path.

# bf16x3 precision ablation (scripts/train_quality.py --x3-drop): stages of the
# fp32-accurate training path that run in plain bf16 instead (their lo parts
# zeroed: bf16 x bf16 products accumulated in fp32, exactly the bf16 path's
# arithmetic), to find which stages the weak-loss signal needs:
#   corr     the correlation operands (the L2-normalised trunk features)
#   nc_in    the NeighConsensus input (the MutualMatching output)
#   nc_w     the NeighConsensus weights
#   nc_act   the hidden NeighConsensus activations
#   nc_grad  the backward's activation gradients
#   nc_w_bwd the NeighConsensus weights in the backward only (data gradients)
X3_STAGES = ("corr", "nc_in", "nc_w", "nc_act", "nc_grad", "nc_w_bwd")
# rebound by x3_ablation: read it in this module only (others ask x3_dropped)
_X3_DROP: frozenset = frozenset()


@contextlib.contextmanager
def x3_ablation(stages):
    """Run the bf16x3 training path with ``stages`` (subset of X3_STAGES) in bf16."""
    global _X3_DROP
    bad = set(stages) - set(X3_STAGES)
    if bad:
        raise ValueError(f"unknown x3 stages {sorted(bad)}; known: {X3_STAGES}")
    old, _X3_DROP = _X3_DROP, frozenset(stages)
    try:
        yield
    finally:
        _X3_DROP = old


def x3_dropped(stage: str) -> bool:
    return stage in _X3_DROP


def _x3_weights(ws, backward: bool = False):
    drop = "nc_w" in _X3_DROP or (backward and "nc_w_bwd" in _X3_DROP)
    return [w.to(torch.bfloat16).float() for w in ws] if drop else ws


def _pack2(fn, w: torch.Tensor) -> torch.Tensor:
    """[2, ...] packed weights: the hi set, then the lo set (the kernels' layout)."""
    hi, lo = _wsplit(w)
    return torch.stack((fn(hi), fn(lo))).contiguous()


def x3_fused_ok(kinds, channels, kernel_sizes, x: torch.Tensor, symmetric: bool) -> bool:
    I, J, K, L = x.shape[2:6]
    return (kinds is not None and len(kinds) >= 2 and kinds[0] == "1in" and kinds[-1] == "1out"
            and all(k == "16" for k in kinds[1:-1]) and max(channels) <= 16
            and all(k in (3, 5) for k in kernel_sizes) and symmetric and (I, J) == (K, L))


def _x3_fast1x_layer(C, ctx, li, kind, w, xin, g, dws, dbs, main, side, shp, ks, cin, cout):
    """Backward of a 1-channel layer of the fused bf16x3 stack on the padded-plane
    kernels: the weight gradient as the three wgrad1x16 products (X_hi G_hi +
    X_hi G_lo + X_lo G_hi), the last layer's data gradient as conv1x16's
    bf16x3 mode with the ReLU mask of its input.  ``g`` [2, 2V, ...(, 16)]: the
    hi / lo gradient w.r.t. the layer's pre-activation.  Returns the next
    (lower) layer's pre-activation gradient, or None after the first layer."""
    V, I, J, K, L = ctx.dims
    if kind == "1out":
        n = g.shape[1]
        gp = torch.zeros((2, n * I * J) + (C.pad_geom(K, L, ks)[1],), dtype=torch.bfloat16, device=g.device)
        for h in range(2):
            _pad_1ch(g[h].reshape(n, I * J, K * L), K, L, ks, 0, out=gp[h])
        with _OnSide(main, side, (xin, g, gp)):
            # (each product already in the checkpoint layout: the layout is linear)
            dws[li] = sum(_wgrad1x(C, xin[a], gp[b], ks, False, cin, False)[0] for a, b in ((0, 0), (0, 1), (1, 0)))
            dbs[li] = (g[0].sum(dtype=torch.float32) + g[1].sum(dtype=torch.float32)).reshape(1)
        gn = torch.empty((2,) + tuple(shp) + (16,), dtype=torch.bfloat16, device=g.device)
        C.conv1x16(gp, _pack2(pack_w1x, transpose_for_dgrad(w)), None, xin[0], gn, ks, 2 | 4)
        return gn
    # first layer: xin = padded planes of the NC input [2, N, PPL]; g [2, 2V, ..., 16]
    parts = [_wgrad1x(C, g[a], xin[b], ks, b == 0, cout, True) for a, b in ((0, 0), (1, 0), (0, 1))]
    dws[li] = parts[0][0] + parts[1][0] + parts[2][0]
    dbs[li] = parts[0][1] + parts[1][1]
    return None


class NeighConsensusX3FusedFn(torch.autograd.Function):
    """fp32-accurate TRAINING NeighConsensus (symmetric, square volumes) on the
    fused bf16x3 kernels; same math as NeighConsensusX3Fn."""

    @staticmethod
    def forward(ctx, x, kinds, channels, *params):
        C = _ext.ext()
        ws = [_std(w) for w in params[0::2]]
        bs = params[1::2]
        V, _, I, J, K, L = x.shape
        R, Cc = I * J, K * L
        ks0 = ws[0].shape[-1]
        dev = x.device
        fast = fast1x_ok(kinds, channels, [w.shape[-1] for w in ws], x, True)
        if fast:
            # padded 1-channel planes of hi and lo, both branches (the swapped
            # one written by pad_planes trans=1): the conv1x16 / wgrad1x16 path
            hi, lo = _split(x.reshape(V, R, Cc).float())
            _, ppl = C.pad_geom(K, L, ks0)
            xs = torch.zeros((2, 2 * V * R, ppl), dtype=torch.bfloat16, device=dev)
            for t, part in ((hi, xs[0]), (lo, xs[1])):
                _pad_1ch(t, K, L, ks0, 0, out=part[:V * R])
                _pad_1ch(t, I, J, ks0, 1, out=part[V * R:])
            shp = (2 * V, I, J, K, L)
        else:
            x0 = x.reshape(V, I, J, K, L).float()
            x0 = torch.cat((x0, x0.permute(0, 3, 4, 1, 2)), 0)      # both symmetric branches
            shp = tuple(x0.shape)
            hi, lo = _split(x0)
            del x0
            xs = torch.empty((2, ij_groups(ks0)) + shp + (16,), dtype=torch.bfloat16, device=dev)
            C.ijpack(hi, xs[0], ks0, 1)
            C.ijpack(lo, xs[1], ks0, 1)
        del hi, lo
        if "nc_in" in _X3_DROP:
            xs[1].zero_()
        ws = _x3_weights(ws)
        saved = [xs]
        h = None
        for li, kind in enumerate(kinds):
            w, b = ws[li], bs[li]
            ks = w.shape[-1]
            if kind == "1out":
                y = torch.empty(shp, dtype=torch.float32, device=dev)
                C.conv16_blk_fwd_x3(h[0], h[1], _pack2(lambda t: pack_w16_planes(blk_out_weights(t)), w),
                                    b.float().reshape(1).contiguous(), y, ks, 1)
                h = y
                break
            a = torch.empty((2,) + shp + (16,), dtype=torch.bfloat16, device=dev)
            if kind == "1in" and fast:
                C.conv1x16(xs, _pack2(pack_w1x, w), _pad_bias(b, 16), None, a, ks, 1 | 4)
            elif kind == "1in":
                C.conv16_fwd_x3(xs[0], xs[1], _pack2(lambda t: pack_w16_planes(ij_in_weights(t)), w),
                                _pad_bias(b, 16), None, a[0], a[1], ks, 1)
            else:
                C.conv16_fwd_x3(h[0], h[1], _pack2(pack_w16, w), _pad_bias(b, 16), None, a[0], a[1], ks, 1)
            if "nc_act" in _X3_DROP:
                a[1].zero_()
            saved.append(a)
            h = a
        z = h                                                      # [2V, I, J, K, L] fp32 (ReLU'd)
        ctx.kinds, ctx.channels, ctx.dims, ctx.fast1x = kinds, channels, (V, I, J, K, L), fast
        ctx.save_for_backward(z, *params, *saved)
        return combine_1ch(z, ctx.dims)

    @staticmethod
    def backward(ctx, gy):
        C = _ext.ext()
        kinds, channels = ctx.kinds, ctx.channels
        nl = len(kinds)
        z, *rest = ctx.saved_tensors
        params, saved = rest[:2 * nl], rest[2 * nl:]
        ws = _x3_weights([_std(w) for w in params[0::2]], backward=True)
        V, I, J, K, L = ctx.dims
        R, Cc = I * J, K * L
        shp = tuple(z.shape)
        dev = z.device
        g = torch.empty((2,) + shp, dtype=torch.bfloat16, device=dev)   # d/d(last pre-activation), hi / lo
        C.combine_bwd(gy.reshape(V, R, Cc).float().contiguous(), z, g[0], R, Cc, g[1])
        xs = saved[0]
        acts = saved[1:]                                              # per hidden layer: [2, 2V, ..., 16]
        dws, dbs = [None] * nl, [None] * nl
        gx = None
        main, side = _streams(z)
        for li in range(nl - 1, -1, -1):
            if "nc_grad" in _X3_DROP:
                g[1].zero_()
            kind, w = kinds[li], ws[li]
            ks = w.shape[-1]
            cout = channels[li]
            cin = 1 if li == 0 else channels[li - 1]
            xin = xs if li == 0 else acts[li - 1]                     # [2, (G,) 2V, ..., 16]
            gs = None
            gn = None
            if ctx.fast1x and kind in ("1in", "1out"):
                gn = _x3_fast1x_layer(C, ctx, li, kind, w, xin, g, dws, dbs, main, side, shp, ks, cin, cout)
            else:
                if kind == "1out":
                    gs = torch.empty((2, ij_groups(ks)) + shp + (16,), dtype=torch.bfloat16, device=dev)
                    C.ijpack(g[0], gs[0], ks, -1)
                    C.ijpack(g[1], gs[1], ks, -1)
                # the three (X, G) products; the bias gradient is sum(G_hi) + sum(G_lo)
                if kind == "1out":
                    combos = [(xin[0:1], g[0], gs[0]), (xin[0:1], g[1], gs[1]), (xin[1:2], g[0], gs[0])]
                elif kind == "1in":
                    combos = [(xin[0], g[0:1], None), (xin[0], g[1:2], None), (xin[1], g[0:1], None)]
                else:
                    combos = [(xin[0:1], g[0:1], None), (xin[0:1], g[1:2], None), (xin[1:2], g[0:1], None)]
                on_side = li > 0
                with _OnSide(main if on_side else None, side if on_side else None,
                             tuple(t for t in (xin, g, gs) if t is not None)):
                    res = [layer_wgrad(C, kind, xi, gi, gsi, ks, cin, cout) for xi, gi, gsi in combos]
                    dws[li] = ref.conv4d_weight_from_std(res[0][0] + res[1][0] + res[2][0])
                    dbs[li] = res[0][1] + res[1][1]
            if li == 0:
                if ctx.needs_input_grad[0]:
                    gx = _sum3(lambda gg, wp: conv_layer(gg, wp, cout, 1, relu=False), (g[0:1], g[1:2]),
                               _wsplit(transpose_for_dgrad(w)))
                break
            if gn is None:
                gn = torch.empty((2,) + shp + (16,), dtype=torch.bfloat16, device=dev)
                if kind == "1out":
                    wp2 = _pack2(lambda t: pack_w16_planes(plane_dgrad_weights(ij_out_weights(t))), w)
                    C.conv16_fwd_x3(gs[0], gs[1], wp2, None, xin[0], gn[0], gn[1], ks, 2)
                else:
                    C.conv16_fwd_x3(g[0], g[1], _pack2(pack_w16, transpose_for_dgrad(w)), None, xin[0], gn[0], gn[1],
                                    ks, 2)
            g = gn
        _join_side(main, side, dws + dbs)
        if gx is not None:
            gx = gx[:V] + gx[V:].permute(0, 3, 4, 1, 2)
            gx = gx.reshape(V, 1, I, J, K, L)
        return (gx, None, None, *interleave(dws, dbs))


class NeighConsensusMixedFn(torch.autograd.Function):
    """nc_precision='mixed' training NeighConsensus: the bf16x3 forward of
    NeighConsensusX3FusedFn (fp32-accurate input, weights and hidden
    activations) with a bf16 backward -- bf16 gradients, bf16 weights in the
    data gradients, each weight gradient the (X_hi, G) + (X_lo, G) products --
    on the bf16 training kernels (the padded-plane 1-channel path).  It keeps
    the fp32-accurate forward for ~2/3 of the fp32 mode's NeighConsensus work.
    Over 24 seeds (scripts/precision_ablation.py, profiles/r5/ablation) bf16,
    this mix and fp32 took off at the same rate within noise (the earlier
    4-seed 0.533 vs 0.535 PCK comparison is withdrawn): there is no evidence
    that it learns where bf16 does not."""

    @staticmethod
    def forward(ctx, x, kinds, channels, *params):
        y = NeighConsensusX3FusedFn.forward(ctx, x, kinds, channels, *params)
        ctx.nparams = len(params)
        return y

    @staticmethod
    def backward(ctx, gy):
        if not ctx.fast1x:
            return NeighConsensusX3FusedFn.backward(ctx, gy)
        C = _ext.ext()
        kinds, channels = ctx.kinds, ctx.channels
        nl = len(kinds)
        z, *rest = ctx.saved_tensors
        params, saved = rest[:2 * nl], rest[2 * nl:]
        ws = list(params[0::2])
        V, I, J, K, L = ctx.dims
        R, Cc = I * J, K * L
        gz = torch.empty(z.numel(), dtype=torch.bfloat16, device=z.device)
        C.combine_bwd(gy.reshape(V, R, Cc).float().contiguous(), z, gz, R, Cc)
        xs, acts = saved[0], saved[1:]
        hi = [xs[0]] + [a[0:1] for a in acts]
        lo = [xs[1]] + [a[1:2] for a in acts]
        need_dx0 = ctx.needs_input_grad[0]
        dws, dbs, g0 = _stack_bwd(gz.reshape(tuple(z.shape)), hi, ws, kinds, channels, need_dx0, True,
                                  _stack_packs(ws, kinds), saved_lo=lo)
        gx = unswap_gx(g0, ctx.dims) if need_dx0 else None
        return (gx, None, None, *interleave(dws, dbs))
