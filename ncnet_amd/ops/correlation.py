"""FeatureL2Norm + 4D FeatureCorrelation on the HIP kernels.

* ``l2norm_pack``: L2-normalise channels (lib/model.py:14-17) and emit the
  correlation GEMM operand ``[N, H*W, C]`` bf16 in one pass.  A channels-last
  backbone output is already ``[N, H, W, C]`` in memory, so no transpose copy.
* ``correlation``: batched MFMA GEMM ``A[amap[v]] . B[bmap[v]]^T`` with fp32
  output (lib/model.py:106-115).  ``amap``/``bmap`` express the weak loss's
  rolled negative pairs (train.py:137) without copying features.
* ``correlation_pool2``: the InLoc relocalization path; GEMM with a fused
  2x2x2x2 max-pool epilogue (lib/model.py:177-191) -- only the pooled volume
  and packed argmax offsets are written.  It takes the same pair maps, and
  bf16 features that require grad get the HIP backward ``corr_pool2_bwd``
  (``CorrelationPool2Fn``; relocalized training with a trainable trunk).
* ``pair_volumes``: the one place that chooses among them (and
  ``correlation_x3`` / ``maxpool4d``) for a set of pairs; the model's inference
  and training entries both call it.  Pair maps travel as host int sequences
  (``weak_loss_maps`` builds the weak loss's); ``_device_map`` caches their
  device copies.
* IEEE-half inference (``corr_dtype='fp16'``, half_precision models as the
  reference's eval_inloc.py): ``l2norm_pack_f16`` operands on the f16 MFMA.
* fp32-accurate inference ("bf16x3", ``corr_dtype='fp32'``): the L2-norm
  kernel also writes the bf16 rounding residual and the correlation is three
  bf16 GEMMs (hi.hi + hi.lo + lo.hi), matching the reference's fp32 bmm
  (lib/model.py:110-113) to ~16 mantissa bits.
* fp8 inference path (BASELINE config 5): ``l2norm_pack_fp8`` writes OCP
  e4m3 operands scaled by ``FP8_FEAT_SCALE`` (unit rows have entries ~1/sqrt(C),
  the scale keeps them out of the e4m3 subnormals) and both correlation entry
  points accept them, running the MX-scaled K=128 fp8 MFMA (2x the bf16 rate)
  and undoing the scale in the epilogue.  No autograd (inference only).
"""
from __future__ import annotations

import torch

from . import _ext
from . import reference as ref


class L2NormPackFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat):
        n, c, h, w = feat.shape
        x = feat.permute(0, 2, 3, 1)
        if not x.is_contiguous():
            x = x.contiguous()
        if x.dtype not in (torch.bfloat16, torch.float32):
            x = x.float()
        x2 = x.reshape(n * h * w, c)
        y = torch.empty((n * h * w, c), dtype=torch.bfloat16, device=feat.device)
        inv = torch.empty((n * h * w,), dtype=torch.float32, device=feat.device)
        _ext.ext().l2norm_rows(x2, y, inv, 0.0, None)
        ctx.save_for_backward(x2, inv)
        ctx.shape = (n, c, h, w)
        ctx.in_dtype = feat.dtype
        return y.reshape(n, h * w, c)

    @staticmethod
    def backward(ctx, gy):
        x2, inv = ctx.saved_tensors
        n, c, h, w = ctx.shape
        gx = torch.empty(x2.shape, dtype=torch.float32, device=gy.device)
        _ext.ext().l2norm_rows_bwd(x2.float().contiguous(), gy.reshape(x2.shape).float().contiguous(), inv, gx)
        return gx.reshape(n, h, w, c).permute(0, 3, 1, 2).to(ctx.in_dtype)


def l2norm_pack(feat: torch.Tensor) -> torch.Tensor:
    """[N, C, H, W] -> L2-normalised [N, H*W, C] (bf16 on GPU)."""
    if _ext.use_hip(feat):
        return L2NormPackFn.apply(feat)
    n, c, h, w = feat.shape
    return ref.feature_l2norm(feat.float()).reshape(n, c, h * w).transpose(1, 2)


FP8_FEAT_SCALE = 16.0
FP8 = torch.float8_e4m3fn


def l2norm_pack_fp8(feat: torch.Tensor) -> torch.Tensor:
    """[N, C, H, W] -> FP8_FEAT_SCALE * L2-normalised [N, H*W, C] in OCP fp8
    e4m3 (GPU, inference).  CPU: the same values through torch's fp8 cast."""
    n, c, h, w = feat.shape
    if not _ext.use_hip(feat):
        y = ref.feature_l2norm(feat.float()).reshape(n, c, h * w).transpose(1, 2) * FP8_FEAT_SCALE
        return y.contiguous().to(FP8)
    x = feat.permute(0, 2, 3, 1)
    if not x.is_contiguous():
        x = x.contiguous()
    if x.dtype not in (torch.bfloat16, torch.float32):
        x = x.float()
    y = torch.empty((n * h * w, c), dtype=FP8, device=feat.device)
    _ext.ext().l2norm_rows(x.reshape(n * h * w, c), y, None, FP8_FEAT_SCALE, None)
    return y.reshape(n, h * w, c)


def l2norm_pack_f16(feat: torch.Tensor) -> torch.Tensor:
    """[N, C, H, W] -> L2-normalised [N, H*W, C] in IEEE half (the reference's
    half_precision features, lib/model.py:263-265; inference).  The GEMMs then
    run on the f16 MFMA: 3 more mantissa bits than bf16 at the same rate."""
    n, c, h, w = feat.shape
    if not _ext.use_hip(feat):
        return ref.feature_l2norm(feat.float()).reshape(n, c, h * w).transpose(1, 2).to(torch.float16)
    x = feat.permute(0, 2, 3, 1)
    if not x.is_contiguous():
        x = x.contiguous()
    if x.dtype not in (torch.bfloat16, torch.float32):
        x = x.float()
    y = torch.empty((n * h * w, c), dtype=torch.float16, device=feat.device)
    _ext.ext().l2norm_rows(x.reshape(n * h * w, c), y, None, 0.0, None)
    return y.reshape(n, h * w, c)


def l2norm_pack_split(feat: torch.Tensor):
    """[N, C, H, W] -> (hi, lo) bf16 [N, H*W, C] with hi + lo = the L2-normalised
    rows to ~16 mantissa bits (fp32-accurate "bf16x3" inference mode)."""
    n, c, h, w = feat.shape
    x = feat.permute(0, 2, 3, 1)
    if not x.is_contiguous():
        x = x.contiguous()
    if x.dtype not in (torch.bfloat16, torch.float32):
        x = x.float()
    if not _ext.use_hip(feat):
        y = ref.feature_l2norm(feat.float()).permute(0, 2, 3, 1).reshape(n, h * w, c)
        hi = y.to(torch.bfloat16)
        return hi, (y - hi.float()).to(torch.bfloat16)
    hi = torch.empty((n * h * w, c), dtype=torch.bfloat16, device=feat.device)
    lo = torch.empty_like(hi)
    _ext.ext().l2norm_rows(x.reshape(n * h * w, c), hi, None, 0.0, lo)
    return hi.reshape(n, h * w, c), lo.reshape(n, h * w, c)


def correlation_x3(fa, fb, amap: torch.Tensor | None = None, bmap: torch.Tensor | None = None) -> torch.Tensor:
    """fp32-accurate correlation of split operands (``l2norm_pack_split``):
    A.B^T ~ Ahi.Bhi^T + Ahi.Blo^T + Alo.Bhi^T on three bf16 MFMA GEMMs with
    fp32 accumulation (the dropped Alo.Blo^T term is ~2^-16 relative).
    Inference only.  fa = (hi, lo) [Na, M, C], fb = (hi, lo) [Nb, N, C]."""
    (ah, al), (bh, bl) = fa, fb
    if amap is None:
        amap = torch.arange(ah.shape[0], device=ah.device, dtype=torch.int32)
    if bmap is None:
        bmap = torch.arange(bh.shape[0], device=bh.device, dtype=torch.int32)
    if not _ext.use_hip(ah):
        a = ah.float() + al.float()
        b = bh.float() + bl.float()
        return torch.bmm(a[amap.long()], b[bmap.long()].transpose(1, 2))
    C = _ext.ext()
    am, bm = amap.to(torch.int32), bmap.to(torch.int32)
    out = torch.empty((am.numel(), ah.shape[1], bh.shape[1]), dtype=torch.float32, device=ah.device)
    part = torch.empty_like(out)
    C.corr_gemm(ah.contiguous(), bh.contiguous(), out, am, bm, 1.0)
    C.corr_gemm(ah.contiguous(), bl.contiguous(), part, am, bm, 1.0)
    out += part
    C.corr_gemm(al.contiguous(), bh.contiguous(), part, am, bm, 1.0)
    out += part
    return out


def _fp8_rows(t: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """Row gather of an fp8 tensor (through a uint8 view: fp8 indexing kernels
    are not guaranteed on every backend)."""
    return t.view(torch.uint8)[:, idx].contiguous().view(FP8)


def pack_rows(feat: torch.Tensor) -> torch.Tensor:
    """[N, C, H, W] -> [N, H*W, C] (no normalisation)."""
    n, c, h, w = feat.shape
    return feat.permute(0, 2, 3, 1).reshape(n, h * w, c)


class CorrelationFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fa, fb, amap, bmap):
        V = amap.numel()
        out = torch.empty((V, fa.shape[1], fb.shape[1]), dtype=torch.float32, device=fa.device)
        dt = torch.float16 if fa.dtype == torch.float16 else torch.bfloat16   # f16 MFMA for half operands
        a = fa.to(dt).contiguous()
        b = fb.to(dt).contiguous()
        _ext.ext().corr_gemm(a, b, out, amap, bmap, 1.0)
        ctx.save_for_backward(a, b, amap, bmap)
        ctx.dtypes = (fa.dtype, fb.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b, amap, bmap = ctx.saved_tensors
        am, bm = amap.long(), bmap.long()
        ga = gb = None
        g = g.float()
        if ctx.needs_input_grad[0]:
            ga = torch.zeros(a.shape, dtype=torch.float32, device=g.device)
            ga.index_add_(0, am, torch.bmm(g, b.float()[bm]))
            ga = ga.to(ctx.dtypes[0])
        if ctx.needs_input_grad[1]:
            gb = torch.zeros(b.shape, dtype=torch.float32, device=g.device)
            gb.index_add_(0, bm, torch.bmm(g.transpose(1, 2), a.float()[am]))
            gb = gb.to(ctx.dtypes[1])
        return ga, gb, None, None


def correlation(fa: torch.Tensor, fb: torch.Tensor, amap: torch.Tensor | None = None,
                bmap: torch.Tensor | None = None) -> torch.Tensor:
    """fa [Na, M, C], fb [Nb, N, C] -> [V, M, N] fp32 with V = len(amap)."""
    if amap is None:
        amap = torch.arange(fa.shape[0], device=fa.device, dtype=torch.int32)
    if bmap is None:
        bmap = torch.arange(fb.shape[0], device=fb.device, dtype=torch.int32)
    if fa.dtype == FP8:
        scale = 1.0 / (FP8_FEAT_SCALE * FP8_FEAT_SCALE)
        if not _ext.use_hip(fa):
            return torch.bmm(fa.float()[amap.long()], fb.float()[bmap.long()].transpose(1, 2)) * scale
        out = torch.empty((amap.numel(), fa.shape[1], fb.shape[1]), dtype=torch.float32, device=fa.device)
        _ext.ext().corr_gemm(fa.contiguous(), fb.contiguous(), out, amap.to(torch.int32), bmap.to(torch.int32), scale)
        return out
    if _ext.use_hip(fa):
        return CorrelationFn.apply(fa, fb, amap.to(torch.int32), bmap.to(torch.int32))
    return torch.bmm(fa.float()[amap.long()], fb.float()[bmap.long()].transpose(1, 2))


_BLOCK_ORDER: dict = {}


def block_order_index(h: int, w: int, k: int, device) -> torch.Tensor:
    """Permutation putting each k x k spatial block's rows next to each other
    (row = (k*k)*blk + (k*dy + dx), blk row-major over the pooled grid).
    Cached per (h, w, k, device): a pure function of the shape, built once
    instead of ~10 small launches per InLoc pair (treat it as read-only)."""
    key = (h, w, k, str(device))
    perm = _BLOCK_ORDER.get(key)
    if perm is None:
        if torch.cuda.is_available() and torch.device(device).type == "cuda" and torch.cuda.is_current_stream_capturing():
            return _block_order_index(h, w, k, device)      # not cached from inside a graph capture
        with torch.inference_mode(False):                   # a normal tensor: usable with autograd later
            perm = _BLOCK_ORDER[key] = _block_order_index(h, w, k, device)
    return perm


def _block_order_index(h: int, w: int, k: int, device) -> torch.Tensor:
    ii = torch.arange(h, device=device).view(h, 1)
    jj = torch.arange(w, device=device).view(1, w)
    blk = (ii // k) * (w // k) + (jj // k)
    sub = (ii % k) * k + (jj % k)
    key = (blk * k * k + sub).reshape(-1)
    perm = torch.empty_like(key)
    perm[key] = torch.arange(h * w, device=device)
    return perm  # new row r takes old row perm[r]


_BLOCK_ORDER_INV: dict = {}


def block_order_inverse(h: int, w: int, k: int, device) -> torch.Tensor:
    """Inverse of ``block_order_index``: natural row r sits at block-order row
    ``inv[r]`` (cached like the permutation; read-only)."""
    key = (h, w, k, str(device))
    inv = _BLOCK_ORDER_INV.get(key)
    if inv is None:
        with torch.inference_mode(False):
            inv = _BLOCK_ORDER_INV[key] = torch.argsort(_block_order_index(h, w, k, device))
    return inv


def _host_map(m, n: int):
    """A pair map as a tuple of ints (``None``: identity over n images).  A GPU
    tensor is read back (one host sync): callers on the training path pass
    lists / CPU tensors."""
    if m is None:
        return tuple(range(n))
    if torch.is_tensor(m):
        return tuple(int(x) for x in m.reshape(-1).tolist())
    return tuple(int(x) for x in m)


_DEV_MAPS: dict = {}       # keyed by the map tuple: a trainer has one or two batch sizes, so a few entries


def _device_map(m, device) -> torch.Tensor:
    """int32 device tensor of a pair map given as a sequence or tensor (sequences cached)."""
    if torch.is_tensor(m):
        return m.to(device=device, dtype=torch.int32)
    key = (tuple(m), str(device))
    t = _DEV_MAPS.get(key)
    if t is None:
        with torch.inference_mode(False):
            t = _DEV_MAPS[key] = torch.tensor(key[0], dtype=torch.int32, device=device)
    return t


_BWD_TABLES: dict = {}     # likewise: one small table per distinct (maps, image counts, device)


def pool2_bwd_table(amap, bmap, na: int, nb: int, device):
    """Per-image volume lists of the pooled correlation's backward, built and
    validated on the host: ``(aoff [na+1], avol [V], boff [nb+1], bvol [V],
    amap [V], bmap [V])`` int32 on ``device``.  Image n of side A owns the
    volumes ``avol[aoff[n]:aoff[n+1]]`` in ascending order (likewise B); every
    map entry is in range and every volume appears exactly once per side.
    Cached per (maps, na, nb, device)."""
    am, bm = tuple(amap), tuple(bmap)
    key = (am, bm, na, nb, str(device))
    tab = _BWD_TABLES.get(key)
    if tab is not None:
        return tab
    if len(am) != len(bm):
        raise ValueError(f"amap has {len(am)} volumes, bmap {len(bm)}")
    out = []
    for name, mp, n in (("amap", am, na), ("bmap", bm, nb)):
        bad = [x for x in mp if not 0 <= x < n]
        if bad:
            raise ValueError(f"{name} entries {bad} are outside [0, {n})")
        lists = [[v for v, x in enumerate(mp) if x == img] for img in range(n)]
        off = [0]
        for ls in lists:
            off.append(off[-1] + len(ls))
        vol = [v for ls in lists for v in ls]
        if sorted(vol) != list(range(len(mp))):
            raise ValueError(f"{name}: every volume must appear exactly once in the image lists")
        out += [off, vol]
    with torch.inference_mode(False):
        tab = tuple(torch.tensor(x, dtype=torch.int32, device=device) for x in (*out, am, bm))
    _BWD_TABLES[key] = tab
    return tab


def _transposed_padded(x: torch.Tensor) -> torch.Tensor:
    """[n, R, K] -> [n, K, ldr] with ldr = R rounded up to 32, zero past R (the
    feature operand of corr_pool2_bwd: a lane's 8 reduced rows in 16 bytes)."""
    n, r, k = x.shape
    ldr = (r + 31) // 32 * 32
    if ldr == r:
        return x.transpose(1, 2).contiguous()
    t = torch.zeros((n, k, ldr), dtype=x.dtype, device=x.device)
    t[:, :, :r] = x.transpose(1, 2)
    return t


def corr_pool2_bwd(a: torch.Tensor, b: torch.Tensor, g: torch.Tensor, code: torch.Tensor, amap, bmap,
                   hA: int, wA: int, hB: int, wB: int, need=(True, True)):
    """Feature gradients of the fused pooled correlation on the HIP kernel
    (csrc/corrpool_bwd.hip).  ``a`` [Na, hA*wA, K] / ``b`` [Nb, hB*wB, K] bf16
    in 2x2-block row order, ``g`` fp32 and ``code`` uint8 [V, hA/2, wA/2, hB/2,
    wB/2] (codes as ``corr_gemm_pool2`` writes them), ``amap`` / ``bmap`` host
    sequences.  Returns (gA, gB) fp32 in block row order (``None`` where
    ``need`` is false).  ``g`` enters the MFMA rounded to bf16 (round to nearest
    even), as every gradient operand of the bf16 training path; products are
    exact and accumulate in fp32 in a fixed order: two runs are bit-identical."""
    if a.shape[2] % 16:
        raise ValueError(f"corr_pool2_bwd needs a channel count that is a multiple of 16 (got {a.shape[2]})")
    dev = a.device
    aoff, avol, boff, bvol, am, bm = pool2_bwd_table(_host_map(amap, a.shape[0]), _host_map(bmap, b.shape[0]),
                                                     a.shape[0], b.shape[0], dev)
    V = am.numel()
    g = g.reshape(V, hA // 2, wA // 2, hB // 2, wB // 2).float().contiguous()
    code = code.reshape(g.shape).contiguous()
    C = _ext.ext()
    ga = gb = None
    if need[0]:
        ga = torch.empty(a.shape, dtype=torch.float32, device=dev)
        C.corr_pool2_bwd(_transposed_padded(b), g, code, aoff, avol, bm, ga, 0, hA, wA, hB, wB)
    if need[1]:
        gb = torch.empty(b.shape, dtype=torch.float32, device=dev)
        C.corr_pool2_bwd(_transposed_padded(a), g, code, boff, bvol, am, gb, 1, hA, wA, hB, wB)
    _ext.count("corr_pool2_bwd")
    return ga, gb


class CorrelationPool2Fn(torch.autograd.Function):
    """Fused correlation + 2x2x2x2 max-pool with a HIP backward into bf16
    features (natural row order in and out; the block-order gather is inside)."""

    @staticmethod
    def forward(ctx, fa, fb, amap, bmap, dims, host_maps):
        hA, wA, hB, wB = dims
        pa = block_order_index(hA, wA, 2, fa.device)
        pb = block_order_index(hB, wB, 2, fb.device)
        a = fa.to(torch.bfloat16)[:, pa].contiguous()
        b = fb.to(torch.bfloat16)[:, pb].contiguous()
        shape = (amap.numel(), hA // 2, wA // 2, hB // 2, wB // 2)
        val = torch.empty(shape, dtype=torch.float32, device=fa.device)
        code = torch.empty(shape, dtype=torch.uint8, device=fa.device)
        _ext.ext().corr_gemm_pool2(a, b, val, code, hA, wA, hB, wB, 1.0, amap, bmap)
        ctx.save_for_backward(a, b, code)
        ctx.dims, ctx.host_maps = dims, host_maps
        ctx.dtypes = (fa.dtype, fb.dtype)
        code = code.unsqueeze(1)
        ctx.mark_non_differentiable(code)
        return val.unsqueeze(1), code

    @staticmethod
    @torch.autograd.function.once_differentiable      # the HIP result has no graph: a double backward raises
    def backward(ctx, g, _gcode):
        a, b, code = ctx.saved_tensors
        hA, wA, hB, wB = ctx.dims
        need = (ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        ga, gb = corr_pool2_bwd(a, b, g, code, *ctx.host_maps, hA, wA, hB, wB, need=need)
        if ga is not None:
            ga = ga[:, block_order_inverse(hA, wA, 2, ga.device)].to(ctx.dtypes[0])
        if gb is not None:
            gb = gb[:, block_order_inverse(hB, wB, 2, gb.device)].to(ctx.dtypes[1])
        return ga, gb, None, None, None, None


def correlation_pool2(fa: torch.Tensor, fb: torch.Tensor, hA: int, wA: int, hB: int, wB: int,
                      packed: bool = False, amap=None, bmap=None):
    """Fused correlation + maxpool4d(k=2). fa [Na, hA*wA, C], fb [Nb, hB*wB, C]
    (natural row order); volume v is the pair (fa[amap[v]], fb[bmap[v]]), the
    maps (int sequences or int tensors) defaulting to the identity.  Returns
    (pooled [V,1,hA/2,wA/2,hB/2,wB/2] fp32, (di, dj, dk, dl) uint8 offsets of
    the same shape) -- or, ``packed``, the single uint8 volume of 2-bit codes
    (``decode_offsets``).

    bf16 (or fp32, cast to bf16) features that require grad go through
    ``CorrelationPool2Fn``: the backward is the HIP kernel of
    csrc/corrpool_bwd.hip, whose MFMA operand holds the incoming gradient
    rounded to bf16 (see ``corr_pool2_bwd``).  Pass the maps as sequences or CPU
    tensors there: a GPU map tensor is read back once to build the per-image
    volume lists.  fp8 / IEEE-half operands are inference-only."""
    mapped = amap is not None or bmap is not None
    fp8 = fa.dtype == FP8
    scale = 1.0 / (FP8_FEAT_SCALE * FP8_FEAT_SCALE) if fp8 else 1.0
    if not _ext.use_hip(fa):
        a, b = fa.float(), fb.float()
        if mapped:
            a = a[torch.as_tensor(_host_map(amap, fa.shape[0]), dtype=torch.long, device=fa.device)]
            b = b[torch.as_tensor(_host_map(bmap, fb.shape[0]), dtype=torch.long, device=fb.device)]
        corr = torch.bmm(a, b.transpose(1, 2)).view(a.shape[0], 1, hA, wA, hB, wB) * scale
        return ref.maxpool4d(corr, 2)
    if torch.is_grad_enabled() and (fa.requires_grad or fb.requires_grad):
        if fp8 or fa.dtype == torch.float16 or fb.dtype == torch.float16:
            raise RuntimeError("correlation_pool2: fp8 / fp16 operands are inference-only (no backward); "
                               "use bf16 features for training")
        ha_map, hb_map = _host_map(amap, fa.shape[0]), _host_map(bmap, fb.shape[0])
        val, code = CorrelationPool2Fn.apply(fa, fb, _device_map(amap if amap is not None else ha_map, fa.device),
                                             _device_map(bmap if bmap is not None else hb_map, fa.device),
                                             (hA, wA, hB, wB), (ha_map, hb_map))
        return (val, code) if packed else (val, decode_offsets(code))
    am = bm = None
    if mapped:
        am = _device_map(amap if amap is not None else range(fa.shape[0]), fa.device)
        bm = _device_map(bmap if bmap is not None else range(fb.shape[0]), fa.device)
    V = am.numel() if mapped else fa.shape[0]
    pa = block_order_index(hA, wA, 2, fa.device)
    pb = block_order_index(hB, wB, 2, fb.device)
    if fp8:
        a, b = _fp8_rows(fa, pa), _fp8_rows(fb, pb)
    else:
        dt = torch.float16 if fa.dtype == torch.float16 else torch.bfloat16
        a = fa.to(dt)[:, pa].contiguous()
        b = fb.to(dt)[:, pb].contiguous()
    shape = (V, hA // 2, wA // 2, hB // 2, wB // 2)
    val = torch.empty(shape, dtype=torch.float32, device=fa.device)
    code = torch.empty(shape, dtype=torch.uint8, device=fa.device)
    if mapped:
        _ext.ext().corr_gemm_pool2(a, b, val, code, hA, wA, hB, wB, scale, am, bm)
    else:
        _ext.ext().corr_gemm_pool2(a, b, val, code, hA, wA, hB, wB, scale)
    if packed:
        return val.unsqueeze(1), code.unsqueeze(1)
    return val.unsqueeze(1), decode_offsets(code.unsqueeze(1))


def decode_offsets(code: torch.Tensor):
    """Packed 2-bit offsets -> (di, dj, dk, dl) as uint8 volumes (8x less traffic
    than int64 at InLoc size; they index / add like integers)."""
    return ((code >> 6) & 3, (code >> 4) & 3, (code >> 2) & 3, code & 3)


def maxpool4d(corr4d: torch.Tensor, k_size: int):
    """Batch-correct 4D max-pool with integer offsets (lib/model.py:177-191)."""
    if _ext.use_hip(corr4d) and 1 <= k_size <= 4:
        b, ch, i, j, k, l = corr4d.shape
        x = corr4d.reshape(b, i, j, k, l)
        if x.dtype not in (torch.float32, torch.bfloat16):
            x = x.float()
        x = x.contiguous()
        shape = (b, i // k_size, j // k_size, k // k_size, l // k_size)
        val = torch.empty(shape, dtype=torch.float32, device=x.device)
        code = torch.empty(shape, dtype=torch.uint8, device=x.device)
        _ext.ext().maxpool4d(x, val, code, k_size)
        return val.unsqueeze(1), decode_offsets(code.unsqueeze(1))
    return ref.maxpool4d(corr4d, k_size)


def weak_loss_maps(b: int):
    """The weak loss's pair maps as host int tuples: the positive pairs
    (a_i, b_i), then the negatives (a_{i+1}, b_i) -- sources rolled by -1
    (train.py:137)."""
    ar = tuple(range(b))
    return ar + ar[1:] + ar[:1], ar + ar


def fuses_pool(fa, hwa, hwb, k: int) -> bool:
    """Whether ``pair_volumes`` takes the fused pool (``correlation_pool2``):
    k = 2, all four grid dimensions even, operands not split."""
    return k == 2 and not isinstance(fa, tuple) and not any(d % 2 for d in (*hwa, *hwb))


def pair_volumes(fa, fb, hwa, hwb, amap=None, bmap=None, k: int = 0, packed_offsets: bool = False):
    """THE route from packed features to correlation volumes: volume v is the
    pair (fa[amap[v]], fb[bmap[v]]) -- maps as host int sequences (device copies
    from the ``_device_map`` cache), ``None``: the identity.  Returns (corr4d
    [V,1,hA',wA',hB',wB'], the pool's offsets or ``None``).  ``fuses_pool``:
    ``correlation_pool2`` (``packed_offsets`` is its ``packed``); split (hi, lo)
    operands: ``correlation_x3``, else ``correlation`` -- either followed by
    ``maxpool4d`` when k > 1 (no backward through that pool).  fp8 / IEEE-half
    operands stay inference-only inside ``correlation`` / ``correlation_pool2``."""
    (ha, wa), (hb, wb) = hwa, hwb
    if fuses_pool(fa, hwa, hwb, k):
        return correlation_pool2(fa, fb, ha, wa, hb, wb, packed=packed_offsets, amap=amap, bmap=bmap)
    split = isinstance(fa, tuple)
    dev = (fa[0] if split else fa).device
    am = _device_map(amap, dev) if amap is not None else None
    bm = _device_map(bmap, dev) if bmap is not None else None
    corr = correlation_x3(fa, fb, am, bm) if split else correlation(fa, fb, am, bm)
    corr4d = corr.view(corr.shape[0], 1, ha, wa, hb, wb)
    return maxpool4d(corr4d, k) if k > 1 else (corr4d, None)
