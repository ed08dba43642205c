"""The bf16 training stack: ``NeighConsensusFn`` (any odd kernel sizes and
channel counts, layer by layer on ``layers.conv_layer``) and
``NeighConsensusPaddedFn`` (the same with the NC input's padded planes supplied
by MutualMatching), the padded-plane 1-channel layers they use on the training
shapes, and the side-stream schedule of the weight gradients."""
from __future__ import annotations

import functools

import torch

from ... import config as _config
from .. import _ext
from .. import reference as ref
from ..packing import (_blk_packed, _cout1_packed, _w16_dgrad, _w1x_dgrad, gather_pack, ij_out_weights, pack_w16, pack_w1x,
                       pack_w16_planes, packed_weights, plane_dgrad_weights, transpose_for_dgrad)
from .layers import (_pad_bias, _std, combine_1ch, conv_layer, ijpack, interleave, layer_wgrad, nblocks, planar_to_blocks,
                     reduce_partials, swap_flat, wgrad16_ckpt)

# ---------------------------------------------------------------------------
# Padded-plane 1-channel layers (csrc/conv1x.hip) for the NC-Net training stack
# [1 -> 16 (k=5), 16 -> 16 ..., 16 -> 1 (k=5)] at a 25 x 25 (k, l) plane: the
# 1-channel operands (the NC input, the last layer's output gradient) are kept
# as zero-padded planes (0.07 GB) instead of the 16x ij-packed copies (1.6 GB
# each): the first layer's forward and the last layer's data gradient run on
# conv1x16, both weight gradients on wgrad1x16.

# False sends the fast shapes through the general ij-packed layers instead.
# Read here on every call: set it on THIS module (tests/test_gpu_kernels.py
# test_neigh_consensus_fast1x_matches_ij_path does); no environment knob.
FAST1X = True
# (kernel size, K, L) with conv1x16 / wgrad1x16 instantiations (csrc/conv1x.hip):
# --image_size 400 and 320 at k = 5, and the IVD recipe's k = 3 at 400 px
FAST1X_SHAPES = frozenset({(5, 25, 25), (5, 20, 20), (5, 30, 30), (3, 25, 25)})


def fast1x_ok(kinds, channels, kernel_sizes, x: torch.Tensor, symmetric: bool) -> bool:
    if not (FAST1X and x.is_cuda and len(kinds) >= 2 and kinds[0] == "1in" and kinds[-1] == "1out"):
        return False
    if any(k != "16" for k in kinds[1:-1]) or any(c != 16 for c in channels[:-1]):
        return False
    _, _, I, J, K, L = x.shape
    if symmetric and (I, J) != (K, L):
        return False
    return (kernel_sizes[0], K, L) in FAST1X_SHAPES and (kernel_sizes[-1], K, L) in FAST1X_SHAPES


@functools.lru_cache(maxsize=None)
def _num_cus(index: int) -> int:
    return torch.cuda.get_device_properties(index).multi_processor_count


def _pad_1ch(x3: torch.Tensor, I2: int, J2: int, ks: int, trans: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """x3 [V, R, C] (fp32 / bf16) -> zero-padded bf16 planes [N, PPL] (csrc/conv1x.hip
    pad_planes; trans 1: the planes of the A<->B-swapped volume)."""
    C = _ext.ext()
    _, ppl = C.pad_geom(I2, J2, ks)
    n = x3.shape[0] * (x3.shape[2] if trans else x3.shape[1])
    if out is None:
        out = torch.zeros((n, ppl), dtype=torch.bfloat16, device=x3.device)
    C.pad_planes(x3.contiguous(), out, I2, J2, ks, trans)
    return out


def _wgrad1x(C, d16: torch.Tensor, xp: torch.Tensor, ks: int, bias: bool, ch: int, first: bool):
    """wgrad1x16 partials reduced straight into the checkpoint layout by one
    reduce_cols launch: R[tap (dk, dl)][combo (di, dj)][c] (the kernel's
    partial layout, combos padded to 32) becomes
      first layer (Cin = 1):  dW[co = c, 0, di, dj, dk, dl] = R  -> [k, ch, 1, k, k, k];
      Cout = 1 last layer:    dW[0, ci = c, t] = R[2P - t] (all four axes
                              flipped)                          -> [k, 1, ch, k, k, k];
    and the bias sum [16] (or None) in the same launch."""
    G = _num_cus(d16.device.index)
    part = torch.empty((G, ks * ks, 32, 16), dtype=torch.float32, device=d16.device)
    partb = torch.empty((G, 16), dtype=torch.float32, device=d16.device) if bias else None

    def layout(t):
        r = t[:, : ks * ks, :ch].reshape((ks,) * 4 + (ch,))          # [dk, dl, di, dj, c]
        if first:
            return r.permute(2, 4, 3, 0, 1).unsqueeze(2)
        return r.flip(0, 1, 2, 3).permute(2, 4, 3, 0, 1).unsqueeze(1)

    C.wgrad1x16(d16, xp, part, partb, ks)
    segs = [(part, ("w1x", ks, ch, first), layout)]
    if bias:
        segs.append((partb, None, None))
    outs = reduce_partials(segs)
    return outs[0], (outs[1][:ch] if bias else None)


def _stack_fwd(x0: torch.Tensor, ws, bs, kinds, save: list, xp=None, shp=None, packs=None):
    """x0: [V,I,J,K,L] bf16 -> last layer's ReLU output, fp32: [V,I,J,K,L] if it
    has one channel, else planar [C, V,I,J,K,L].  Appends, per layer, what its
    backward reads: the ij-packed input (1-channel inputs) or the bf16 input blocks.
    ``packs``: {("f", layer): packed forward operand} from ``_stack_packs``."""
    C = _ext.ext()
    h = x0
    nl = len(kinds)
    cin = 1
    for li, (w_ref, b) in enumerate(zip(ws, bs)):
        w = _std(w_ref)
        ks, cout = w.shape[-1], w.shape[0]
        last = li == nl - 1
        xs = None
        if li == 0 and xp is not None:      # padded-plane first layer (fast1x_ok)
            y = torch.empty(tuple(shp) + (16,), dtype=torch.bfloat16, device=xp.device)
            C.conv1x16(xp, packs[("f", 0)] if packs else gather_pack(pack_w1x, w), _pad_bias(b, 16), None, y, ks, 1)
            save.append(xp)
            h, cin = y.unsqueeze(0), cout
            continue
        if cin == 1:
            xs = ijpack(C, h.contiguous(), ks, 1)
            save.append((xs, h) if li > 0 else xs)   # mid-stack 1-channel inputs also serve as ReLU masks
        else:
            save.append(h)
        y = conv_layer(h, w, cin, cout, bias=b, relu=True, f32=last and cout > 1, xs=xs,
                       wp=packs.get(("f", li)) if packs else None, wt=packs.get(("t", li)) if packs else None)
        if cout == 1 and not last:
            y = y.to(torch.bfloat16)
        h = y
        cin = cout
    return h


# Weight gradients of the layers after the first on a second HIP stream
# (config.RUNTIME.bwd_overlap, NCNET_BWD_OVERLAP=0 disables): they depend only on the layer input and the
# incoming gradient, so wgrad(l) runs while the data-gradient chain continues
# on the main stream (dgrad(l) -> dgrad(l-1) -> ...).  The first layer's
# weight gradient stays on the main stream, which is idle by then.
_SIDE_STREAMS: dict = {}


def _streams(t: torch.Tensor):
    """(main, side) streams of a backward on ``t``'s device; (None, None) when
    the weight gradients stay on the current stream."""
    if not (_config.RUNTIME.bwd_overlap and t.is_cuda):
        return None, None
    st = _SIDE_STREAMS.get(t.device.index)
    if st is None:
        st = _SIDE_STREAMS[t.device.index] = torch.cuda.Stream(device=t.device)
    return torch.cuda.current_stream(t.device), st


# side-stream inputs kept alive until the backward joins the side stream back
# (_join_side).  Not record_stream: a block marked in use by the side stream
# is reusable only once the allocator sees the side stream's event complete --
# with the host a step ahead of the GPU that is never in time, so every step
# hipMalloc'ed fresh blocks for its 16-channel volumes (reserved memory grew
# to the whole 288 GB at a per-GPU batch of 256 and the allocator's
# release-and-retry stalled whole steps for seconds).  Freed on the host after
# main.wait_stream(side), the blocks return to main's pool, where every later
# use is ordered after the side stream's reads.
_SIDE_KEEP: dict = {}


def _join_side(main, side, outs):
    """End of a backward: main waits for the side stream, the held inputs are
    released, and ``outs`` (produced on the side stream, consumed and freed on
    main) are marked in use by main."""
    if side is None:
        return
    main.wait_stream(side)
    _SIDE_KEEP.pop(id(side), None)
    for t in outs:
        t.record_stream(main)


class _OnSide:
    """Run a block on the side stream after everything queued on ``main``;
    inputs stay referenced until _join_side, outputs are marked in use by ``main``."""

    def __init__(self, main, side, inputs):
        self.main, self.side, self.inputs = main, side, inputs
        self.ctx = None

    def __enter__(self):
        if self.side is None:
            return self
        self.side.wait_stream(self.main)
        _SIDE_KEEP.setdefault(id(self.side), []).extend(self.inputs)
        self.ctx = torch.cuda.stream(self.side)
        self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)
        return False


def _stack_bwd(g_last: torch.Tensor, saved, ws, kinds, channels, need_dx0: bool, fast1x: bool = False,
               packs=None, saved_lo=None):
    """g_last: grad w.r.t. the last conv's PRE-activation, bf16: [V,I,J,K,L] for
    a 1-channel output, else blocks [NB, V,I,J,K,L,16].
    Returns (dW list in checkpoint layout, db list, grad of x0 fp32 or None).
    ``saved_lo`` (nc_precision='mixed', fast1x only): per layer the lo part of
    a bf16x3-split forward input; each weight gradient then adds the
    (X_lo, G) product to the (X_hi, G) one (G bf16)."""
    C = _ext.ext()
    nl = len(kinds)
    dws, dbs = [None] * nl, [None] * nl
    ref_layout = [False] * nl          # True: dW already in the checkpoint layout
    g = g_last
    gx0 = None
    main, side = _streams(g_last)
    for li in range(nl - 1, -1, -1):
        kind = kinds[li]
        w = _std(ws[li])
        ks = w.shape[-1]
        cout = channels[li]
        cin = 1 if li == 0 else channels[li - 1]
        sv = saved[li]
        if cin == 1:
            xin, hin = (sv if li > 0 else (sv, None))
        else:
            xin = hin = sv
        gs = None
        if fast1x and kind in ("1in", "1out"):
            if kind == "1out":                       # padded planes of the 1-channel output gradient
                gp = _pad_1ch(g.reshape(g.shape[0], g.shape[1] * g.shape[2], g.shape[3] * g.shape[4]),
                              g.shape[3], g.shape[4], ks, 0)
                xlo = saved_lo[li] if saved_lo is not None else None
                with _OnSide(main if li > 0 else None, side if li > 0 else None,
                             (xin, g, gp) + ((xlo,) if xlo is not None else ())):
                    dw, _ = _wgrad1x(C, xin[0], gp, ks, False, cin, False)
                    if xlo is not None:
                        dw = dw + _wgrad1x(C, xlo[0], gp, ks, False, cin, False)[0]
                    db = g.sum(dtype=torch.float32).reshape(1)
                if li > 0 or need_dx0:
                    gn = torch.empty((1,) + tuple(hin.shape[1:]), dtype=torch.bfloat16, device=g.device)
                    C.conv1x16(gp, packs[("b", li)] if packs else gather_pack(_w1x_dgrad, w), None, hin[0], gn[0],
                               ks, 2)
                    g = gn
            else:                                    # first layer: xin = padded NC-input planes
                dw, db = _wgrad1x(C, g[0], xin, ks, True, cout, True)
                if saved_lo is not None:
                    dw = dw + _wgrad1x(C, g[0], saved_lo[li], ks, False, cout, True)[0]
                if need_dx0:
                    gx0 = conv_layer(g, transpose_for_dgrad(w), cout, 1, relu=False)
            dws[li] = dw
            dbs[li] = db
            ref_layout[li] = True
            continue
        if cout == 1 and kind == "1out":
            gs = ijpack(C, g, ks, -1)                # adjoint of ijsum: shared by wgrad and dgrad
        on_side = li > 0
        xlo = saved_lo[li] if saved_lo is not None else None
        with _OnSide(main if on_side else None, side if on_side else None,
                     tuple(t for t in (xin, g, gs, xlo) if t is not None)):
            if kind == "16" and cin == 16 and cout == 16:
                # one reduce_cols launch: partials -> checkpoint layout + bias
                dw, db = wgrad16_ckpt(C, xin[0], g[0], ks)
                if xlo is not None:
                    dw = dw + wgrad16_ckpt(C, xlo[0], g[0], ks)[0]
                ref_layout[li] = True
            else:
                dw, db = layer_wgrad(C, kind, xin, g, gs, ks, cin, cout)
        if li > 0 or need_dx0:
            if kind == "1out":                       # reuses ijpack(g, -1) of the weight gradient
                # each input block's gradient is written straight into its slot
                # (no stacking copy of the [NB, V,I,J,K,L,16] result)
                gn = torch.empty((nblocks(cin),) + tuple(hin.shape[1:]), dtype=torch.bfloat16, device=g.device)
                for a in range(nblocks(cin)):
                    wp = pack_w16_planes(plane_dgrad_weights(ij_out_weights(w[:, 16 * a:16 * a + 16])))
                    C.conv16_fwd(gs, wp, None, hin[a], gn[a], ks, 2)
                g = gn
            elif cin == 1:                           # gradient w.r.t. a 1-channel input (fp32)
                gx = conv_layer(g, transpose_for_dgrad(w), cout, 1, relu=False)
                if li == 0:
                    gx0 = gx
                else:                                # mid-stack: the previous layer's ReLU mask
                    g = (gx * (hin > 0)).to(torch.bfloat16)
            else:                                    # "16": masked by the previous layer's ReLU output
                g = conv_layer(g, transpose_for_dgrad(w), cout, cin, relu=False, mask=hin,
                               wp=packs.get(("b", li)) if packs else None)
        dws[li] = dw
        dbs[li] = db
    _join_side(main, side, dws + dbs)
    return [d if ref_layout[i] else ref.conv4d_weight_from_std(d) for i, d in enumerate(dws)], dbs, gx0


def _stack_packs(ws, kinds):
    """Every packed operand of the padded-plane training stack (fast1x_ok) --
    conv1x16 weights of layer 0, conv16 weights of the 16 -> 16 layers and their
    data-gradient (transposed, flipped) weights, the output-plane-block weights
    of the Cout=1 layer and its conv1x16 data-gradient weights -- from ONE gather
    launch (packing.packed_weights) -> {("f" | "b", layer): bf16 tensor}."""
    specs, keys = [], []
    nl = len(kinds)
    for li, kind in enumerate(kinds):
        if li == 0:
            specs.append((0, pack_w1x)); keys.append(("f", 0))
        elif li == nl - 1:
            specs += [(li, _blk_packed), (li, _cout1_packed), (li, _w1x_dgrad)]
            keys += [("f", li), ("t", li), ("b", li)]
        else:
            specs += [(li, pack_w16), (li, _w16_dgrad)]; keys += [("f", li), ("b", li)]
    return dict(zip(keys, packed_weights(list(ws), specs)))


def _combine_multi(z1: torch.Tensor, z2: torch.Tensor, dims) -> torch.Tensor:
    """Symmetric combine of multi-channel outputs: z1 planar [C, V, I, J, K, L],
    z2 planar [C, V, K, L, I, J] -> y [V, C, I, J, K, L] fp32."""
    return (z1 + z2.permute(0, 1, 4, 5, 2, 3)).transpose(0, 1).contiguous()


def unswap_gx(g0: torch.Tensor, dims, gbt: torch.Tensor | None = None) -> torch.Tensor:
    """Input gradient of the symmetric op, ``ga + swap(gbt)`` as [V, 1, I, J, K, L]:
    ``g0`` holds both branches' 1-channel input gradients (one batched run: A
    [V,I,J,K,L], then B [V,K,L,I,J]), or branch A's with ``gbt`` branch B's."""
    V, I, J, K, L = dims
    R, Cc = I * J, K * L
    ga = g0.reshape(-1)
    if gbt is None:
        ga, gbt = ga[:V * R * Cc], ga[V * R * Cc:]
    gb = swap_flat(gbt.reshape(V, Cc, R), (K, L, I, J))
    return (ga.reshape(V, R, Cc) + gb).reshape(V, 1, I, J, K, L)


class NeighConsensusFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, symmetric, kinds, channels, *params):
        return NeighConsensusFn._fwd(ctx, x, symmetric, kinds, channels, params)

    @staticmethod
    def _fwd(ctx, x, symmetric, kinds, channels, params, xp_in=None):
        """``xp_in``: the padded bf16 planes of both symmetric branches, already
        written by MutualMatching (mutual.mutual_matching_padded); only used
        on the padded-plane path (fast1x_ok, symmetric, square)."""
        ws, bs = params[0::2], params[1::2]
        V, _, I, J, K, L = x.shape
        R, Cc = I * J, K * L
        cl = channels[-1]
        saved_layers = []
        square = (I, J) == (K, L)
        fast = fast1x_ok(kinds, channels, [w.shape[0] for w in ws], x, symmetric)
        packs = _stack_packs(ws, kinds) if fast else None
        if fast:
            # the 1-channel input as padded planes, both branches in one batch
            # (pad_planes trans=1 writes the swapped branch's planes directly)
            x3 = x.reshape(V, R, Cc)
            k0 = ws[0].shape[0]
            if symmetric:
                _, ppl = _ext.ext().pad_geom(K, L, k0)
                if xp_in is not None and tuple(xp_in.shape) == (2 * V * R, ppl) and xp_in.dtype == torch.bfloat16:
                    xp = xp_in
                else:
                    xp = torch.zeros((2 * V * R, ppl), dtype=torch.bfloat16, device=x.device)
                    _pad_1ch(x3, K, L, k0, 0, out=xp[:V * R])
                    _pad_1ch(x3, I, J, k0, 1, out=xp[V * R:])
                z = _stack_fwd(None, ws, bs, kinds, saved_layers, xp=xp, shp=(2 * V, I, J, K, L), packs=packs)
            else:
                z = _stack_fwd(None, ws, bs, kinds, saved_layers, xp=_pad_1ch(x3, K, L, k0, 0), shp=(V, I, J, K, L),
                               packs=packs)
            branches = [saved_layers]
        elif symmetric:
            xb = x.reshape(V, I, J, K, L).to(torch.bfloat16).contiguous()
            xt = swap_flat(xb.reshape(V, R, Cc), (I, J, K, L)).reshape(V, K, L, I, J)
            if square:
                z = _stack_fwd(torch.cat((xb, xt), 0), ws, bs, kinds, saved_layers)
                branches = [saved_layers]
            else:
                s1, s2 = [], []
                z1 = _stack_fwd(xb, ws, bs, kinds, s1)
                z2 = _stack_fwd(xt, ws, bs, kinds, s2)
                branches = [s1, s2]
        else:
            z = _stack_fwd(x.reshape(V, I, J, K, L).to(torch.bfloat16).contiguous(), ws, bs, kinds, saved_layers)
            branches = [saved_layers]
        if symmetric:
            if square:
                z1, z2 = (z[:V], z[V:]) if cl == 1 else (z[:, :V], z[:, V:])
            if cl == 1:
                if not square:
                    z = torch.cat((z1.reshape(-1), z2.reshape(-1)))
                y = combine_1ch(z, (V, I, J, K, L))
            else:
                if not square:
                    z = torch.cat((z1.reshape(cl, -1), z2.reshape(cl, -1)), 1)
                y = _combine_multi(z1, z2, (V, I, J, K, L))
        else:
            y = z.reshape(V, 1, I, J, K, L) if cl == 1 else z.transpose(0, 1).contiguous()
        ctx.fast1x = fast
        ctx.packs = packs
        ctx.symmetric = symmetric
        ctx.kinds = kinds
        ctx.channels = channels
        ctx.dims = (V, I, J, K, L)
        ctx.nbranch = len(branches)
        flat = []
        ctx.layout = []
        for br in branches:
            lay = []
            for t in br:
                if isinstance(t, tuple):
                    flat.extend(t)
                    lay.append(2)
                else:
                    flat.append(t)
                    lay.append(1)
            ctx.layout.append(lay)
        ctx.save_for_backward(z, *params, *flat)
        return y

    @staticmethod
    def backward(ctx, gy):
        gx, grads = NeighConsensusFn._bwd(ctx, gy)
        return (gx, None, None, None, *grads)

    @staticmethod
    def _bwd(ctx, gy):
        z, *rest = ctx.saved_tensors
        nparam = 2 * len(ctx.kinds)
        params, flat = rest[:nparam], list(rest[nparam:])
        ws = params[0::2]
        V, I, J, K, L = ctx.dims
        R, Cc = I * J, K * L
        cl = ctx.channels[-1]
        need_dx0 = ctx.needs_input_grad[0]
        branches = []
        pos = 0
        for lay in ctx.layout:
            br = []
            for n in lay:
                br.append(flat[pos] if n == 1 else tuple(flat[pos:pos + n]))
                pos += n
            branches.append(br)
        if cl == 1:
            gy3 = gy.reshape(V, R, Cc).float().contiguous()
            if ctx.symmetric:
                gz = torch.empty(z.numel(), dtype=torch.bfloat16, device=gy.device)
                _ext.ext().combine_bwd(gy3, z, gz, R, Cc)
            else:
                gz = (gy3.reshape(-1) * (z.reshape(-1) > 0)).to(torch.bfloat16)
            n1 = V * R * Cc
            if ctx.nbranch == 1:
                nv = 2 * V if ctx.symmetric else V
                gl = [gz.reshape(nv, I, J, K, L)]
            else:
                gl = [gz[:n1].reshape(V, I, J, K, L), gz[n1:].reshape(V, K, L, I, J)]
        else:
            g1 = gy.float().transpose(0, 1)                        # planar [C, V, I, J, K, L]
            if ctx.symmetric:
                g2 = g1.permute(0, 1, 4, 5, 2, 3)                  # [C, V, K, L, I, J]
                zz = z.reshape(cl, -1)
                n1 = V * R * Cc
                gz1 = g1.reshape(cl, -1) * (zz[:, :n1] > 0)
                gz2 = g2.reshape(cl, -1) * (zz[:, n1:] > 0)
                if ctx.nbranch == 1:
                    gl = [planar_to_blocks(torch.cat((gz1, gz2), 1).reshape(cl, 2 * V, I, J, K, L))]
                else:
                    gl = [planar_to_blocks(gz1.reshape(cl, V, I, J, K, L)),
                          planar_to_blocks(gz2.reshape(cl, V, K, L, I, J))]
            else:
                gl = [planar_to_blocks(g1 * (z > 0))]
        res = [_stack_bwd(g, br, ws, ctx.kinds, ctx.channels, need_dx0, ctx.fast1x, ctx.packs)
               for g, br in zip(gl, branches)]
        if len(res) == 1:            # one batched branch: no accumulation copies
            dws, dbs = res[0][0], res[0][1]
        else:
            dws = [sum(r[0][i] for r in res) for i in range(len(ws))]
            dbs = [sum(r[1][i] for r in res) for i in range(len(ws))]
        gx = None
        if need_dx0:
            if ctx.symmetric:
                gx = unswap_gx(res[0][2], ctx.dims, res[1][2] if len(res) > 1 else None)
            else:
                gx = res[0][2].reshape(V, 1, I, J, K, L)
        return gx, interleave(dws, dbs)


class NeighConsensusPaddedFn(torch.autograd.Function):
    """NeighConsensusFn with the padded NC-input planes supplied by the
    MutualMatching that produced ``x`` (mm_apply's padded mode): the two
    pad passes and the zero fill of the training step's forward disappear."""

    @staticmethod
    def forward(ctx, x, xp, symmetric, kinds, channels, *params):
        return NeighConsensusFn._fwd(ctx, x, symmetric, kinds, channels, params, xp_in=xp)

    @staticmethod
    def backward(ctx, gy):
        gx, grads = NeighConsensusFn._bwd(ctx, gy)
        return (gx, None, None, None, None, *grads)
