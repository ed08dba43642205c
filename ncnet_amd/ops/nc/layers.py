"""One "same" Conv4d layer on the HIP kernels and its launch geometry: the
channel-block / ij-encoded forward (``conv_layer``), the weight gradient
(``layer_wgrad``) with the wgrad launch helpers, and the small operand helpers
every NeighConsensus path shares (ij packing, the A<->B swap, the symmetric
combine).  ``ops/conv4d.py`` and every module of this package build on it; it
imports none of them."""
from __future__ import annotations

import torch

from ... import config as _config
from .. import _ext
from .. import reference as ref
from ..packing import (_blk_packed, _cout1_packed, gather_pack, ij_groups, ij_in_grad, ij_in_weights, ij_out_grad,
                       ij_out_weights, pack_w16, pack_w16_planes)

HIP_KS = (1, 3, 5, 7)


def nblocks(c: int) -> int:
    return (c + 15) // 16


def layer_kinds(channels, kernel_sizes):
    """Per layer ``"1in"`` (Cin=1 -> Cout>1), ``"16"`` (Cin>1 -> Cout>1),
    ``"1out"`` (Cin>1 -> Cout=1) or ``"11"`` (1 -> 1); None if some kernel
    size has no HIP kernel (only odd sizes 1..7 do)."""
    kinds, cin = [], 1
    for c, k in zip(channels, kernel_sizes):
        if k not in HIP_KS or c < 1:
            return None
        kinds.append("11" if cin == 1 and c == 1 else "1in" if cin == 1 else "1out" if c == 1 else "16")
        cin = c
    return kinds


def interleave(first, second) -> list:
    """[a0, b0, a1, b1, ...]: the (weight, bias) parameter list of the autograd
    Functions, and the (dw, db) tail of what their backward returns."""
    return [t for pair in zip(first, second) for t in pair]


_V4_PLANES = {5: (15, 20, 25, 30), 3: (15, 20, 25, 30)}     # wgrad16v4 instantiations (K == L)


def wgrad_v3_ok(shape, ks: int) -> bool:
    """wgrad16v3 (sliding G ring): KS 3/5, full-width X rows L + ks - 1 <= 32;
    or a compile-time wgrad16v4 plane (30 x 30 stages its 34-voxel rows with
    two DMA instructions)."""
    if ks not in (3, 5):
        return False
    K, L = shape[3], shape[4]
    return L + ks - 1 <= 32 or (K == L and K in _V4_PLANES[ks])


def wgrad_v3_ntl(K: int, L: int, ks: int) -> int:
    """(k, l) tiles per plane of wgrad16v3 / v4 (mirrors ncnet_wgrad16v3): ~320
    voxels per tile; on the k = 5 general kernel, more tiles until the 64-voxel
    chunk count per half-tile is 1, 2 or 5 (the instantiations that do not spill).
    The general kernel runs where no v4 plane exists or when the wgrad_v3 A/B
    switch asks for it and the rows fit (L + ks - 1 <= 32)."""
    kl = K * L
    ntl = -(-kl // 320)
    v4 = K == L and K in _V4_PLANES[ks] and not (_config.RUNTIME.wgrad_v3 and L + ks - 1 <= 32)
    if ks == 5 and not v4:
        while (-(-(-(-kl // ntl)) // 64)) not in (1, 2, 5):
            ntl += 1
    return ntl


# workgroups of the 16 -> 16 weight gradient (grid = groups * ks; partials 2 *
# groups x 160 K floats, summed afterwards); other targets measured within noise
_WGRAD_WG_TARGET = 512


def wgrad_v3_groups(shape, ks: int) -> int:
    """Column groups per dj for wgrad16v3: ~2 workgroups per CU, never more
    than the columns (v, j, tile).  Tile rule mirrors ncnet_wgrad16v3."""
    V, I, J, K, L = shape[:5]
    ntl = wgrad_v3_ntl(K, L, ks)
    ncols = V * J * ntl
    target = max(1, _WGRAD_WG_TARGET // ks)
    return max(1, min(target, ncols))


def wgrad_groups(ks: int, nitems: int) -> int:
    """K-split groups of wgrad16v2 in full mode (~3000 workgroups over the
    KS*KS plane offsets; 120 groups at KS=5 beat 20 by 1.4x on MI355X)."""
    target = max(1, 3072 // (ks * ks))
    return max(1, min(target, nitems))


def wgrad_plane_groups(nitems: int) -> int:
    """Groups of the plane-only wgrad (grid = groups): ~3 workgroups per CU."""
    return max(1, min(768, nitems))


def _nitems(shape) -> int:
    V, I, J, K, L = shape[:5]
    return V * I * J * ((K + 24) // 25) * ((L + 24) // 25)


def _wgrad16_launch(C, x16: torch.Tensor, g16: torch.Tensor, ks: int, plane_only: bool):
    """Unreduced partials (part [2 ng, dd, tap, ci, co], partb [2 ng, 16]) of a 16 -> 16 block."""
    shape = x16.shape[:5]
    if plane_only:
        variant, ng = 2, wgrad_plane_groups(_nitems(shape))
    elif wgrad_v3_ok(shape, ks):
        variant, ng = 3, wgrad_v3_groups(shape, ks)
    else:
        variant, ng = 2, wgrad_groups(ks, _nitems(shape))
    ndd = 1 if plane_only else ks * ks
    part = torch.empty((2 * ng, ndd, ks * ks, 16, 16), dtype=torch.float32, device=x16.device)
    partb = torch.empty((2 * ng, 16), dtype=torch.float32, device=x16.device)
    C.wgrad16(x16, g16, part, partb, ks, 2 if plane_only else 0, variant)
    return part, partb


def wgrad16_partials(C, x16: torch.Tensor, g16: torch.Tensor, ks: int, plane_only: bool):
    """Weight-gradient partials of a 16 -> 16 block and their reduction.

    ``plane_only`` False: all (di, dj) plane offsets (wgrad16v3 when it fits,
    else wgrad16v2); True: the (P, P) plane only (ij-encoded 1-channel layers,
    wgrad16v2).  Returns (s, sb): s [dd, tap, ci, co], sb [16] = sum of g16
    over all voxels (bias gradient, the kernels' ones-MFMA)."""
    part, partb = _wgrad16_launch(C, x16, g16, ks, plane_only)
    return part.sum(0), partb.sum(0)


def wgrad16_ckpt(C, x16: torch.Tensor, g16: torch.Tensor, ks: int):
    """The 16 -> 16 layer's weight gradient straight in the checkpoint layout
    [k, 16, 16, k, k, k] and its bias gradient [16]: the partials of every
    workgroup reduced and permuted by ONE reduce_cols launch (was two torch
    reductions, the std permute and the checkpoint permute)."""
    part, partb = _wgrad16_launch(C, x16, g16, ks, False)
    dw, db = reduce_partials([
        (part, ("w16", ks), lambda t: ref.conv4d_weight_from_std(_reduce_wgrad16(t, ks, 16, 16))),
        (partb, None, None)])
    return dw, db


# reduce_partials plans: (key, device) -> (int32 map [N], output shape)
_RED_PLANS: dict = {}


def _col_map(key, part_shape, fn, device):
    """Scatter map of a layout function: position in fn's output of every
    source column (-1: dropped by a slice), from fn applied to the column ids."""
    k = (key, tuple(part_shape), str(device))
    ent = _RED_PLANS.get(k)
    if ent is None:
        n = 1
        for d in part_shape:
            n *= d
        out = fn(torch.arange(n, dtype=torch.int64).reshape(part_shape))
        m = torch.full((n,), -1, dtype=torch.int64)
        m[out.reshape(-1)] = torch.arange(out.numel(), dtype=torch.int64)
        ent = (m.to(torch.int32).to(device), tuple(out.shape))
        _RED_PLANS[k] = ent
    return ent


def reduce_partials(segs):
    """segs: [(part [R, ...] fp32, key, fn)] -> [fn(part.sum(0))] (fn None: the
    plain sum).  ``fn`` is a layout-only function (permute / reshape / flip /
    slice) and ``key`` names it for the plan cache.  On the GPU every segment
    is reduced, laid out and written in ONE reduce_cols launch (fixed summation
    order: the same bits on every run); on the CPU the same by torch ops."""
    outs, srcs, dsts, idxs = [], [], [], []
    for part, key, fn in segs:
        R = part.shape[0]
        src = part.reshape(R, -1)
        if fn is None:
            idx, shape = None, tuple(part.shape[1:])
        else:
            idx, shape = _col_map(key, part.shape[1:], fn, part.device)
        out = torch.empty(shape, dtype=torch.float32, device=part.device)
        outs.append(out); srcs.append(src); dsts.append(out); idxs.append(idx)
    if srcs[0].is_cuda and _ext.use_hip(srcs[0]) and hasattr(_ext.ext(), "reduce_cols"):
        for i in range(0, len(srcs), 4):
            _ext.ext().reduce_cols(srcs[i:i + 4], dsts[i:i + 4], idxs[i:i + 4])
    else:
        for src, out, idx in zip(srcs, dsts, idxs):
            s = src.sum(0)
            if idx is None:
                out.view(-1).copy_(s)
            else:
                keep = idx >= 0
                out.view(-1)[idx[keep].long()] = s[keep]
    return outs


def wgrad_p_ok(shape) -> bool:
    """Plane-only weight gradient of the Cout=1 layer on wgrad16p (double-buffered
    items, both ij groups of ijpack(g, -1) against one staged X plane: 0.81 ms vs
    2 x 0.44 ms at the training shape) when the (k, l) plane is one tile; larger
    planes take the per-group wgrad16v2 calls.  The Cin=1 layer stays on
    wgrad16v2: with one G operand every X fragment feeds a single MFMA, the
    kernel is LDS-bound and v2's 2-3 workgroups per CU hide more (1.18 vs 0.89 ms)."""
    return shape[3] <= 25 and shape[4] <= 25


def wgrad16p_partials(C, x7: torch.Tensor, g7: torch.Tensor, ks: int):
    """x7 [nx, V,I,J,K,L,16], g7 [ng, ...] bf16 with nx == 1 or ng == 1:
    plane-only partials of every (x, g) pair -> (s [nx*ng, tap, ci, co], sb [nx*ng, 16])."""
    nx, ng = x7.shape[0], g7.shape[0]
    if nx * ng > 2:                       # the kernel pairs at most two operands
        if nx > 1:
            outs = [wgrad16p_partials(C, x7[i:i + 2], g7, ks) for i in range(0, nx, 2)]
        else:
            outs = [wgrad16p_partials(C, x7, g7[i:i + 2], ks) for i in range(0, ng, 2)]
        return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
    groups = max(1, min(1024 // (nx * ng), _nitems(x7.shape[1:6])))
    part = torch.empty((2 * groups, nx * ng, ks * ks, 16, 16), dtype=torch.float32, device=x7.device)
    partb = torch.empty((2 * groups, nx * ng, 16), dtype=torch.float32, device=x7.device)
    C.wgrad16p(x7, g7, part, partb, ks)
    return part.sum(0), partb.sum(0)


def _reduce_wgrad16(s: torch.Tensor, ks: int, cout: int, cin: int) -> torch.Tensor:
    # s [dd, tap, ci, co] -> std [co, ci, di, dj, dk, dl]
    return s.permute(3, 2, 0, 1).reshape(16, 16, ks, ks, ks, ks)[:cout, :cin]


def _std(w_ref: torch.Tensor) -> torch.Tensor:
    return ref.conv4d_weight_to_std(w_ref).float()


def _pad_bias(b: torch.Tensor, n: int) -> torch.Tensor:
    b = b.float()
    if b.numel() == n:
        return b.contiguous()
    out = b.new_zeros(n)
    out[: b.numel()] = b
    return out


def _blk(t: torch.Tensor, a: int, n: int) -> slice:
    return slice(16 * a, min(n, 16 * a + 16))


def planar_to_blocks(z: torch.Tensor) -> torch.Tensor:
    """fp32 planar [C, V, I, J, K, L] -> bf16 channels-last blocks [NB, V, I, J, K, L, 16]."""
    c = z.shape[0]
    nb = nblocks(c)
    if c < 16 * nb:
        z = torch.cat((z, z.new_zeros((16 * nb - c,) + tuple(z.shape[1:]))))
    return z.view((nb, 16) + tuple(z.shape[1:])).permute(0, 2, 3, 4, 5, 6, 1).to(torch.bfloat16).contiguous()


def blocks_to_ncl(h: torch.Tensor, c: int) -> torch.Tensor:
    """bf16 blocks [NB, V, I, J, K, L, 16] -> [V, C, I, J, K, L] (a view-based permute)."""
    nb = h.shape[0]
    x = h.permute(1, 0, 6, 2, 3, 4, 5).reshape((h.shape[1], nb * 16) + tuple(h.shape[2:6]))
    return x[:, :c]


def ijpack(C, t: torch.Tensor, ks: int, sign: int, dtype=torch.bfloat16) -> torch.Tensor:
    """The ij encoding of a 1-channel operand (csrc/jshift.hip): t [V,I,J,K,L] ->
    [G, V,I,J,K,L, 16] in ``dtype``, the (di, dj) plane offsets in the channel
    axis.  sign +1: a layer input; -1: a 1-channel output gradient (the adjoint
    of ijsum)."""
    out = torch.empty((ij_groups(ks),) + tuple(t.shape) + (16,), dtype=dtype, device=t.device)
    C.ijpack(t, out, ks, sign)
    return out


def _ij_in_planes(w_std: torch.Tensor) -> torch.Tensor:
    """[co<=16, 1, k^4] -> group-plane weights [G, nq, 64, 8]."""
    return pack_w16_planes(ij_in_weights(w_std))


def _ij_out_planes(w_std: torch.Tensor, nbi: int) -> torch.Tensor:
    """[1, ci, k^4] -> [G, nbi, nq, 64, 8]: combo group g, input block a."""
    per = [pack_w16_planes(ij_out_weights(w_std[:, 16 * a:16 * a + 16])) for a in range(nbi)]
    return torch.stack(per, 1).contiguous()


def cout1_taps_ok(shp, ks: int) -> bool:
    """Does the tap-row Cout=1 kernel (csrc/cout1.hip) cover this layer?
    (k, l) planes of 25 x 25 (the 400 px training volume), kernel size 5."""
    return _config.RUNTIME.cout1_taps and ks == 5 and tuple(shp[3:5]) == (25, 25)


def conv_layer(h: torch.Tensor, w_std: torch.Tensor, cin: int, cout: int, bias=None, relu: bool = True,
               mask=None, f32: bool = False, xs=None, wp=None, wt=None) -> torch.Tensor:
    """One "same" Conv4d on the HIP kernels, any channel counts.

    h: the 1-channel input [V,I,J,K,L] (bf16/fp32) when cin == 1, else bf16
    blocks [NBi, V,I,J,K,L,16]; ``xs``: ijpack(h, +1) if already built.
    Output (pre-activation + bias, then ReLU if ``relu``; or * (mask > 0)):
      f32=False: bf16 blocks [NBo, ...,16] (cout > 1) / fp32 [V,I,J,K,L] (cout == 1)
      f32=True : fp32 planar [cout, V,I,J,K,L] (cout > 1) / fp32 [V,I,J,K,L].
    ``mask`` (bf16 blocks like the output, cout > 1, f32=False only) replaces
    bias/ReLU by the data-gradient epilogue y = acc * (mask > 0).  ``wp``: the
    layer's packed operand from ``packed_weights`` (single-block 16 -> 16 and
    output-plane-block Cout=1 layers), else packed here; ``wt``: the tap-row
    Cout=1 operand (cout1_taps_weights) where cout1_taps_ok."""
    C = _ext.ext()
    ks = w_std.shape[-1]
    shp = tuple(h.shape[:5]) if cin == 1 else tuple(h.shape[1:6])
    dev = h.device
    nbo, nbi = nblocks(cout), nblocks(cin)
    if cin == 1:
        if xs is None:
            xs = ijpack(C, h.contiguous(), ks, 1)
        if cout == 1:                      # 1 -> 1: one output channel of the group-plane conv
            z = torch.empty((1,) + shp, dtype=torch.float32, device=dev)
            C.conv16_fwd(xs, _ij_in_planes(w_std), None, None, z, ks, 4)
            y = z[0]
            if bias is not None:
                y = y + bias.float().view(1)
            return torch.relu(y) if relu else y
        outs = []
        for b in range(nbo):
            wb = _ij_in_planes(w_std[_blk(w_std, b, cout)])
            outs.append(_epilogue_call(C, xs, wb, bias, b, cout, relu, mask, f32, shp, ks))
        return _gather(outs, f32, cout)
    if cout == 1 and nbi == 1 and cout1_taps_ok(shp, ks) and mask is None:
        # tap rows: the 25 in-plane taps on the MFMA rows, 76 % useful work
        # (csrc/cout1.hip), the in-plane shift applied once per output plane
        y = torch.empty(shp, dtype=torch.float32, device=dev)
        if C.cout1_taps_fwd(h[0], wt if wt is not None else gather_pack(_cout1_packed, w_std),
                            None if bias is None else bias.float().reshape(1).contiguous(), y, ks, 1 if relu else 0):
            return y
    if cout == 1 and nbi == 1:
        # output-plane blocks: the 16 MFMA rows are 4x4 output planes, no
        # combo-planar partials (2.5 GB at the training shape) and no ijsum
        y = torch.empty(shp, dtype=torch.float32, device=dev)
        C.conv16_blk_fwd(h[0], wp if wp is not None else gather_pack(_blk_packed, w_std),
                         None if bias is None else bias.float().reshape(1).contiguous(), y, ks, 1 if relu else 0)
        return y
    if cout == 1:                          # several input blocks: ij encoding, combo-planar partials shift-summed by ijsum
        G, nq = ij_groups(ks), ks * ks
        wz = _ij_out_planes(w_std, nbi)
        z = torch.empty((nq,) + shp, dtype=torch.float32, device=dev)
        for gi in range(G):
            C.conv16_fwd(h, wz[gi], None, None, z[16 * gi:min(nq, 16 * gi + 16)], ks, 4)
        y = torch.empty(shp, dtype=torch.float32, device=dev)
        C.ijsum(z, None if bias is None else _pad_bias(bias, 1), y, ks, 1 if relu else 0, 1)
        return y
    if nbi == 1:
        outs = [_epilogue_call(C, h[0], wp if (wp is not None and nbo == 1) else
                               gather_pack(pack_w16, w_std[_blk(w_std, b, cout), :16]), bias, b, cout, relu,
                               mask, f32, shp, ks) for b in range(nbo)]
        return _gather(outs, f32, cout)
    # several input blocks: fp32 partials per (out, in) block pair, summed before the activation
    outs = []
    for b in range(nbo):
        sl = _blk(w_std, b, cout)
        nco = sl.stop - sl.start
        acc = None
        for a in range(nbi):
            z = torch.empty((nco,) + shp, dtype=torch.float32, device=dev)
            C.conv16_fwd(h[a], pack_w16(w_std[sl, 16 * a:16 * a + 16]), None, None, z, ks, 4)
            acc = z if acc is None else acc.add_(z)
        if bias is not None and mask is None:
            acc += bias[sl].float().view(-1, 1, 1, 1, 1, 1)
        if mask is not None:
            acc = acc * (blocks_to_ncl(mask[b:b + 1], nco).transpose(0, 1) > 0)
        elif relu:
            acc = torch.relu_(acc)
        outs.append(acc)
    z = torch.cat(outs) if len(outs) > 1 else outs[0]
    return z if f32 else planar_to_blocks(z)


def _epilogue_call(C, x, wp, bias, b, cout, relu, mask, f32, shp, ks):
    sl = slice(16 * b, min(cout, 16 * b + 16))
    nco = sl.stop - sl.start
    if f32:
        z = torch.empty((nco,) + shp, dtype=torch.float32, device=x.device)
        C.conv16_fwd(x, wp, None, None, z, ks, 4)
        if bias is not None:
            z += bias[sl].float().view(-1, 1, 1, 1, 1, 1)
        return torch.relu_(z) if relu else z
    y = torch.empty(shp + (16,), dtype=torch.bfloat16, device=x.device)
    if mask is not None:
        C.conv16_fwd(x, wp, None, mask[b], y, ks, 2)
    elif relu:
        bb = torch.zeros(16, device=x.device) if bias is None else _pad_bias(bias[sl], 16)
        C.conv16_fwd(x, wp, bb, None, y, ks, 1)
    else:
        if bias is not None:
            raise RuntimeError("internal: bf16 output without ReLU takes no bias")
        C.conv16_fwd(x, wp, None, None, y, ks, 0)
    return y


def _gather(outs, f32: bool, cout: int):
    if f32:
        return torch.cat(outs) if len(outs) > 1 else outs[0]
    return torch.stack(outs) if len(outs) > 1 else outs[0].unsqueeze(0)


def layer_wgrad(C, kind, xin, g, gs, ks, cin, cout):
    """dW [cout, cin, k^4] (std) and db [cout] of one layer.  xin: ij-packed
    input (cin == 1) or input blocks; g: gradient w.r.t. the pre-activation
    (blocks, or 1-channel); gs = ijpack(g, -1) for 1-channel outputs."""
    G = ij_groups(ks)
    dev = g.device
    if kind == "1in":
        dw = torch.empty((cout, 1) + (ks,) * 4, device=dev)
        db = torch.empty(cout, device=dev)
        for b in range(nblocks(cout)):
            sl = slice(16 * b, min(cout, 16 * b + 16))
            parts = [wgrad16_partials(C, xin[gi], g[b], ks, True) for gi in range(G)]
            dw[sl] = ij_in_grad(torch.stack([p[0][0] for p in parts]), sl.stop - sl.start)
            db[sl] = parts[0][1][:sl.stop - sl.start]
        return dw, db
    if kind == "16":
        dw = torch.empty((cout, cin) + (ks,) * 4, device=dev)
        db = torch.empty(cout, device=dev)
        for b in range(nblocks(cout)):
            so = slice(16 * b, min(cout, 16 * b + 16))
            for a in range(nblocks(cin)):
                si = slice(16 * a, min(cin, 16 * a + 16))
                sw, sb = wgrad16_partials(C, xin[a], g[b], ks, False)
                dw[so, si] = _reduce_wgrad16(sw, ks, so.stop - so.start, si.stop - si.start)
                if a == 0:
                    db[so] = sb[:so.stop - so.start]
        return dw, db
    qc = (ks // 2) * ks + ks // 2        # combo (P, P): its channel of ijpack(g, -1) is g itself
    if kind == "1out":
        dw = torch.empty((1, cin) + (ks,) * 4, device=dev)
        db = None
        for a in range(nblocks(cin)):
            si = slice(16 * a, min(cin, 16 * a + 16))
            if wgrad_p_ok(gs.shape[1:6]):
                s, sb = wgrad16p_partials(C, xin[a:a + 1], gs, ks)
                dw[:, si] = ij_out_grad(s, si.stop - si.start)
                if a == 0:
                    db = sb[qc // 16][qc % 16].reshape(1)
                continue
            parts = [wgrad16_partials(C, xin[a], gs[gi], ks, True) for gi in range(G)]
            dw[:, si] = ij_out_grad(torch.stack([p[0][0] for p in parts]), si.stop - si.start)
            if a == 0:
                db = parts[qc // 16][1][qc % 16].reshape(1)
        return dw, db
    # "11": the 1-channel gradient as channel 0 of a 16-channel operand
    g16 = torch.zeros(tuple(g.shape) + (16,), dtype=torch.bfloat16, device=dev)
    g16[..., 0] = g
    parts = [wgrad16_partials(C, xin[gi], g16, ks, True) for gi in range(G)]
    return ij_in_grad(torch.stack([p[0][0] for p in parts]), 1), parts[0][1][:1].clone()


def swap_flat(x: torch.Tensor, shape_ab):
    """[V, I*J, K*L] -> [V, K*L, I*J] via the HIP tiled transpose."""
    C = _ext.ext()
    V = x.shape[0]
    i, j, k, l = shape_ab
    out = torch.empty((V, k * l, i * j), dtype=x.dtype, device=x.device)
    C.transpose(x.reshape(V, i * j, k * l), out)
    return out


def combine_1ch(z: torch.Tensor, dims) -> torch.Tensor:
    """y = z1 + z2^T [V, 1, I, J, K, L] fp32 from the 1-channel results of both
    symmetric branches (z: branch A [V,I,J,K,L], then branch B [V,K,L,I,J], flat)."""
    V, I, J, K, L = dims
    y = torch.empty((V, I, J, K, L), dtype=torch.float32, device=z.device)
    _ext.ext().combine_fwd(z.reshape(-1), y, I * J, K * L)
    return y.reshape(V, 1, I, J, K, L)


def swap_pair(x: torch.Tensor) -> torch.Tensor:
    """x [V, 1, I, J, K, L] with (I, J) == (K, L) -> bf16 [2V, I, J, K, L]: x, then
    its A<->B swap.  The cast and the transpose write straight into the halves
    of one buffer (no concatenation pass)."""
    V, _, I, J, K, L = x.shape
    x2 = torch.empty((2 * V, I, J, K, L), dtype=torch.bfloat16, device=x.device)
    x2[:V].copy_(x.reshape(V, I, J, K, L))
    _ext.ext().transpose(x2[:V].reshape(V, I * J, K * L), x2[V:].reshape(V, K * L, I * J))
    return x2


def symmetric_1ch(x: torch.Tensor, run) -> torch.Tensor:
    """run(x) + swap(run(swap(x))) for an inference stack ``run``: bf16
    [N, I, J, K, L] -> fp32 [N, I, J, K, L].  Square volumes go through ``run``
    once as one batch of 2V volumes, others once per branch."""
    V, _, I, J, K, L = x.shape
    if (I, J) == (K, L):
        z = run(swap_pair(x))
    else:
        xb = x.reshape(V, I, J, K, L).to(torch.bfloat16).contiguous()
        xt = swap_flat(xb.reshape(V, I * J, K * L), (I, J, K, L)).reshape(V, K, L, I, J)
        z = torch.cat((run(xb).reshape(-1), run(xt).reshape(-1)))
    return combine_1ch(z, (V, I, J, K, L))
