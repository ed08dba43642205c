"""Pure-PyTorch oracles for every NC-Net tensor primitive.

These run on any device (the CPU path of the framework and the numerics
reference for every HIP kernel test).  They re-specify the reference's
behaviour explicitly, including the places where the reference silently
depends on torch-0.3 semantics:

* ``feature_l2norm``      -- lib/model.py:14-17 (eps 1e-6 *inside* the sqrt)
* ``correlation_4d``      -- lib/model.py:106-115 ('4D' FeatureCorrelation)
* ``correlation_3d``      -- lib/model.py:97-105 ('3D' legacy mode)
* ``mutual_matching``     -- lib/model.py:155-175
* ``maxpool4d``           -- lib/model.py:177-191, but batch-correct and with
                             integer offsets (the reference folds the batch into
                             the max and returns float offsets on modern torch)
* ``conv4d``              -- lib/conv4d.py:11-51 semantics ("same" zero padding,
                             stride 1, bias added once), computed as k batched
                             conv3d calls instead of an h*k Python loop
* ``conv4d_sliced``       -- the reference *algorithm* (h*k conv3d launches,
                             lib/conv4d.py:39-48), kept only as the measured
                             baseline for bench.py
* ``softmax_max_scores``  -- the weak-loss scores of train.py:121-134
* ``keypoint_ce``         -- the keypoint-supervised loss (an extension; no
                             counterpart in the reference)
* ``warp_norm_u8``        -- the augmenting input kernel's definition (an
                             extension; no counterpart in the reference)

Weight layout: Conv4d weights are stored the way the reference checkpoints
store them, pre-permuted to ``[k, out, in, k, k, k]`` (lib/conv4d.py:75-77).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

L2NORM_EPS = 1e-6
MUTUAL_EPS = 1e-5
L1_EPS = 1e-4


def feature_l2norm(feature: torch.Tensor, dim: int = 1) -> torch.Tensor:
    """f / sqrt(sum_c f^2 + 1e-6)  (lib/model.py:14-17)."""
    norm = torch.sqrt(torch.sum(feature * feature, dim=dim, keepdim=True) + L2NORM_EPS)
    return feature / norm


def correlation_4d(feature_a: torch.Tensor, feature_b: torch.Tensor) -> torch.Tensor:
    """[b,c,hA,wA] x [b,c,hB,wB] -> [b,1,hA,wA,hB,wB] (lib/model.py:106-115)."""
    b, c, ha, wa = feature_a.shape
    _, _, hb, wb = feature_b.shape
    fa = feature_a.reshape(b, c, ha * wa).transpose(1, 2)
    fb = feature_b.reshape(b, c, hb * wb)
    return torch.bmm(fa, fb).view(b, 1, ha, wa, hb, wb)


def correlation_3d(feature_a: torch.Tensor, feature_b: torch.Tensor) -> torch.Tensor:
    """Legacy CNNGeometric layout [b, h*w, h, w] indexed
    [batch, idx_A = row_A + h*col_A, row_B, col_B] (lib/model.py:97-105)."""
    b, c, h, w = feature_a.shape
    fa = feature_a.transpose(2, 3).reshape(b, c, h * w)
    fb = feature_b.reshape(b, c, h * w).transpose(1, 2)
    mul = torch.bmm(fb, fa)  # [b, hB*wB, idx_A]
    return mul.view(b, h, w, h * w).permute(0, 3, 1, 2)


def mutual_matching(corr4d: torch.Tensor) -> torch.Tensor:
    """Soft mutual nearest-neighbour filter (lib/model.py:155-175).

    out = c * ((c / (max_A c + eps)) * (c / (max_B c + eps))); the product of
    the two ratios is taken first, exactly as the reference parenthesises it,
    which keeps the output exactly symmetric under the A<->B swap.
    """
    b, ch, i, j, k, l = corr4d.shape
    c_b = corr4d.reshape(b, i * j, k, l)        # max over A positions per B cell
    c_a = corr4d.reshape(b, i, j, k * l)        # max over B positions per A cell
    max_b = c_b.max(dim=1, keepdim=True)[0]
    max_a = c_a.max(dim=3, keepdim=True)[0]
    ratio_b = (c_b / (max_b + MUTUAL_EPS)).reshape(b, 1, i, j, k, l)
    ratio_a = (c_a / (max_a + MUTUAL_EPS)).reshape(b, 1, i, j, k, l)
    return corr4d * (ratio_a * ratio_b)


def maxpool4d(corr4d: torch.Tensor, k_size: int):
    """4D max pooling with stride = kernel = k, batch-correct, integer offsets.

    Returns ``(pooled [b,1,I/k,J/k,K/k,L/k], (di, dj, dk, dl))`` where each
    offset tensor has the pooled shape and holds the in-window argmax position
    (lib/model.py:177-191).  Ties resolve to the first index in (i,j,k,l)
    lexicographic order, the order in which the reference enumerates slices.
    """
    b, ch, i, j, k, l = corr4d.shape
    assert ch == 1
    s = k_size
    x = corr4d.reshape(b, i // s, s, j // s, s, k // s, s, l // s, s)
    x = x.permute(0, 1, 3, 5, 7, 2, 4, 6, 8).reshape(b, i // s, j // s, k // s, l // s, s ** 4)
    vals, idx = x.max(dim=-1)
    d_l = idx % s
    d_k = (idx // s) % s
    d_j = (idx // (s * s)) % s
    d_i = idx // (s * s * s)
    vals = vals.unsqueeze(1)
    return vals, tuple(t.unsqueeze(1) for t in (d_i, d_j, d_k, d_l))


def corr_pool2_bwd(fa: torch.Tensor, fb: torch.Tensor, g: torch.Tensor, offsets, amap, bmap, hA: int, wA: int,
                   hB: int, wB: int, quantize_g: bool = False):
    """Feature gradients of ``maxpool4d(bmm(fa[amap], fb[bmap]^T), 2)`` in scatter
    form: ``g`` [V,(1,)hA/2,wA/2,hB/2,wB/2] goes to the full-resolution volume at
    the argmax ``offsets`` (di, dj, dk, dl), then two ``bmm`` and ``index_add_``
    over the maps.  fa [Na, hA*wA, C], fb [Nb, hB*wB, C] in natural row order;
    works in their dtype and returns (gA, gB) of their shapes.  ``quantize_g``:
    round ``g`` to bf16 first (what the HIP kernel's MFMA operand holds)."""
    V = g.shape[0]
    pa, pb, qa, qb = hA // 2, wA // 2, hB // 2, wB // 2
    dev, dt = fa.device, fa.dtype
    g = g.reshape(V, pa, pb, qa, qb)
    if quantize_g:
        g = g.to(torch.bfloat16)
    g = g.to(dt)
    di, dj, dk, dl = (torch.as_tensor(d, device=dev).reshape(V, pa, pb, qa, qb).long() for d in offsets)
    ar = lambda n, pos: torch.arange(n, device=dev).view([n if a == pos else 1 for a in range(5)])   # noqa: E731
    row_a = (2 * ar(pa, 1) + di) * wA + 2 * ar(pb, 2) + dj
    row_b = (2 * ar(qa, 3) + dk) * wB + 2 * ar(qb, 4) + dl
    M, N = hA * wA, hB * wB
    full = torch.zeros(V, M * N, dtype=dt, device=dev)
    full.scatter_(1, (row_a * N + row_b).reshape(V, -1), g.reshape(V, -1))
    full = full.view(V, M, N)
    am = torch.as_tensor(amap, device=dev).long()
    bm = torch.as_tensor(bmap, device=dev).long()
    ga = torch.zeros_like(fa).index_add_(0, am, torch.bmm(full, fb[bm]))
    gb = torch.zeros_like(fb).index_add_(0, bm, torch.bmm(full.transpose(1, 2), fa[am]))
    return ga, gb


def conv4d_weight_to_std(weight_ref: torch.Tensor) -> torch.Tensor:
    """[k, out, in, k, k, k] (checkpoint layout) -> [out, in, k, k, k, k]."""
    return weight_ref.permute(1, 2, 0, 3, 4, 5)


def conv4d_weight_from_std(weight_std: torch.Tensor) -> torch.Tensor:
    """[out, in, k, k, k, k] -> [k, out, in, k, k, k] (checkpoint layout)."""
    return weight_std.permute(2, 0, 1, 3, 4, 5).contiguous()


def conv4d(x: torch.Tensor, weight_ref: torch.Tensor, bias: torch.Tensor | None = None) -> torch.Tensor:
    """"Same"-padded stride-1 4D cross-correlation.

    x: [N, Cin, I, J, K, L]; weight_ref: [k, Cout, Cin, k, k, k]; bias: [Cout].
    Computed as k conv3d calls, each over the whole (N*I) batch of 3D slices,
    summing the first-axis taps by shifting a once-padded view (the reference
    instead loops in Python over every output slice: lib/conv4d.py:39-48).
    """
    n, cin, i, j, k, l = x.shape
    ks = weight_ref.shape[0]
    cout = weight_ref.shape[1]
    p = ks // 2
    xp = F.pad(x, (0, 0, 0, 0, 0, 0, p, p))  # pad the I axis only
    out = None
    for di in range(ks):
        xs = xp[:, :, di:di + i].permute(0, 2, 1, 3, 4, 5).reshape(n * i, cin, j, k, l)
        o = F.conv3d(xs, weight_ref[di], bias=None, padding=p)
        out = o if out is None else out + o
    out = out.reshape(n, i, cout, j, k, l).permute(0, 2, 1, 3, 4, 5)
    if bias is not None:
        out = out + bias.view(1, cout, 1, 1, 1, 1)
    return out.contiguous()


def conv4d_sliced(x: torch.Tensor, weight_ref: torch.Tensor, bias: torch.Tensor | None = None) -> torch.Tensor:
    """The reference *algorithm* (lib/conv4d.py:39-48): one conv3d per output
    slice and per first-axis tap, i.e. I*k launches.  Used only as the
    measured "reference-algorithm" baseline in bench.py."""
    n, cin, i, j, k, l = x.shape
    ks = weight_ref.shape[0]
    p = ks // 2
    data = x.permute(2, 0, 1, 3, 4, 5).contiguous()          # [I, N, Cin, J, K, L]
    zeros = data.new_zeros((p,) + tuple(data.shape[1:]))
    padded = torch.cat((zeros, data, zeros), 0)
    slices = []
    for ii in range(i):
        acc = F.conv3d(padded[ii + p], weight_ref[p], bias=bias, padding=p)
        for t in range(1, p + 1):
            acc = acc + F.conv3d(padded[ii + p - t], weight_ref[p - t], padding=p)
            acc = acc + F.conv3d(padded[ii + p + t], weight_ref[p + t], padding=p)
        slices.append(acc)
    return torch.stack(slices, 0).permute(1, 2, 0, 3, 4, 5).contiguous()


def swap_ab(x: torch.Tensor) -> torch.Tensor:
    """[N, C, I, J, K, L] -> [N, C, K, L, I, J] (A<->B swap, lib/model.py:147)."""
    return x.permute(0, 1, 4, 5, 2, 3)


def neigh_consensus(x: torch.Tensor, weights, biases, symmetric: bool = True, conv=conv4d) -> torch.Tensor:
    """Stack of Conv4d+ReLU, optionally symmetric (lib/model.py:143-153)."""
    def stack(v):
        for w, b in zip(weights, biases):
            v = F.relu(conv(v, w, b))
        return v
    if symmetric:
        return stack(x) + swap_ab(stack(swap_ab(x)))
    return stack(x)


def softmax_max_scores(corr4d: torch.Tensor, normalization: str | None = "softmax"):
    """Per-cell matching scores of train.py:121-134.

    Returns (scores_A, scores_B): scores_B[b, kB] = max over A positions of the
    normalised column, scores_A[b, kA] = max over B positions of the row.
    """
    b = corr4d.shape[0]
    i, j, k, l = corr4d.shape[2:]
    mat = corr4d.reshape(b, i * j, k * l)

    def norm(v, dim):
        if normalization is None:
            return v
        if normalization == "softmax":
            return torch.softmax(v, dim=dim)
        if normalization == "l1":
            return v / (v.sum(dim=dim, keepdim=True) + L1_EPS)
        raise ValueError(normalization)

    scores_b = norm(mat, 1).max(dim=1)[0]  # per B cell, over A
    scores_a = norm(mat, 2).max(dim=2)[0]  # per A cell, over B
    return scores_a, scores_b


def _keypoint_axis(p: torch.Tensor, size: torch.Tensor, n: int):
    """Cells i0, i1 and fraction f of the 1-based pixel coordinates ``p`` [B, N]
    on an n-cell axis of images ``size`` [B] pixels long -- the mapping the PCK
    evaluation uses (eval/point_tnf.py normalize_axis)."""
    from ..eval.point_tnf import normalize_axis
    u = ((normalize_axis(p, size.unsqueeze(1)) + 1) / 2 * (n - 1)).clamp(0, n - 1)
    i0 = u.floor().clamp(max=max(n - 2, 0)).long()
    i1 = (i0 + 1).clamp(max=n - 1)
    return i0, i1, u - i0.to(u.dtype)


def keypoint_weight_maps(points: torch.Tensor, im_size: torch.Tensor, h: int, w: int, dtype=None) -> torch.Tensor:
    """[B, 2, N] (x, y) keypoints -> dense bilinear weight maps [B, N, h*w]: four
    cells per keypoint with weights (1-fi)(1-fj), (1-fi)fj, fi(1-fj), fi*fj
    (i: the y / row axis, j: the x / column axis); cells that coincide add up."""
    dtype = dtype or points.dtype
    p, sz = points.to(dtype), im_size.to(dtype)
    i0, i1, fi = _keypoint_axis(p[:, 1], sz[:, 0], h)
    j0, j1, fj = _keypoint_axis(p[:, 0], sz[:, 1], w)
    out = torch.zeros(p.shape[0], p.shape[2], h * w, dtype=dtype, device=p.device)
    for ci, wi in ((i0, 1 - fi), (i1, fi)):
        for cj, wj in ((j0, 1 - fj), (j1, fj)):
            out.scatter_add_(2, (ci * w + cj).unsqueeze(2), (wi * wj).unsqueeze(2))
    return out


def keypoint_valid(source_points: torch.Tensor, target_points: torch.Tensor) -> torch.Tensor:
    """[B, N] bool: all four coordinates of the pair differ from the -1 padding."""
    return ((source_points != -1).all(1)) & ((target_points != -1).all(1))


def _keypoint_maps(corr4d, source_points, target_points, source_im_size, target_im_size):
    b, _, ha, wa, hb, wb = corr4d.shape
    dt, dev = corr4d.dtype, corr4d.device
    sp, tp = source_points.to(dev), target_points.to(dev)
    valid = keypoint_valid(sp, tp).to(dt).unsqueeze(2)
    U = keypoint_weight_maps(sp, source_im_size.to(dev), ha, wa, dt) * valid      # [B, N, R]
    V = keypoint_weight_maps(tp, target_im_size.to(dev), hb, wb, dt) * valid      # [B, N, C]
    return corr4d.reshape(b, ha * wa, hb * wb), U, V, valid


def keypoint_ce(corr4d: torch.Tensor, source_points: torch.Tensor, target_points: torch.Tensor,
                source_im_size: torch.Tensor, target_im_size: torch.Tensor) -> torch.Tensor:
    """Keypoint-supervised cross-entropy on a [B,1,hA,wA,hB,wB] volume (an
    extension beyond the reference; the contract of csrc/kploss.hip).

    Points are [B, 2, N] (x, y) in 1-based pixels of the original images, -1
    padded; sizes [B, 3] (h, w, channels) -- the fields eval/pck.py consumes.
    With U_n / V_n the bilinear weight maps of keypoint n on the A / B grid and
    x = corr4d.view(B, R, C):
        s_n = U_n . x (a blend of four rows),      L_ab = -sum_m V_n(m) log_softmax(s_n)[m]
        t_n = x . V_n (a blend of four columns),   L_ba = -sum_r U_n(r) log_softmax(t_n)[r]
        loss = sum over valid keypoints of (L_ab + L_ba) / (2 max(1, Nvalid))
    A batch without a valid keypoint gives 0 (and a zero gradient)."""
    x, U, V, valid = _keypoint_maps(corr4d, source_points, target_points, source_im_size, target_im_size)
    s = torch.einsum("bnr,brc->bnc", U, x)
    t = torch.einsum("bnc,brc->bnr", V, x)
    l_ab = -(V * torch.log_softmax(s, dim=2)).sum(2)
    l_ba = -(U * torch.log_softmax(t, dim=2)).sum(2)
    return (l_ab + l_ba).sum() / (2 * valid.sum().clamp(min=1))


def keypoint_ce_grad(corr4d: torch.Tensor, source_points: torch.Tensor, target_points: torch.Tensor,
                     source_im_size: torch.Tensor, target_im_size: torch.Tensor) -> torch.Tensor:
    """Closed-form d keypoint_ce / d corr4d (what the HIP backward evaluates):
    1 / (2 Nvalid) sum_n [U_n(r) (softmax(s_n)[m] - V_n(m)) + (softmax(t_n)[r] - U_n(r)) V_n(m)]."""
    x, U, V, valid = _keypoint_maps(corr4d, source_points, target_points, source_im_size, target_im_size)
    ps = torch.softmax(torch.einsum("bnr,brc->bnc", U, x), dim=2) * valid
    pt = torch.softmax(torch.einsum("bnc,brc->bnr", V, x), dim=2) * valid
    g = torch.einsum("bnr,bnc->brc", U, ps - V) + torch.einsum("bnr,bnc->brc", pt - U, V)
    return (g / (2 * valid.sum().clamp(min=1))).reshape(corr4d.shape)


def _unit_axis(q: torch.Tensor, n: int):
    """Cells i0, i1 and fraction f of unit coordinates ``q`` on an n-cell axis:
    ``_keypoint_axis`` on unit coordinates (normalised = 2 unit - 1)."""
    u = (q * (n - 1)).clamp(0, n - 1)
    i0 = u.floor().clamp(max=max(n - 2, 0)).long()
    i1 = (i0 + 1).clamp(max=n - 1)
    return i0, i1, u - i0.to(u.dtype)


def _dense_side(m: torch.Tensor, h: int, w: int, gh: int, gw: int):
    """One side of ``dense_targets``: ``m`` [B, 12] fp64, this side's grid
    h x w, the other grid gh x gw -> cells [B, h*w, 4], weights, valid."""
    i, j = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    ux = (j / (w - 1) if w > 1 else torch.zeros_like(j)).reshape(1, -1)
    uy = (i / (h - 1) if h > 1 else torch.zeros_like(i)).reshape(1, -1)
    c = lambda k: m[:, k].unsqueeze(1)  # noqa: E731
    qx, qy = c(0) * ux + c(1) * uy + c(2), c(3) * ux + c(4) * uy + c(5)
    sx, sy = c(6) * ux + c(7) * uy + c(8), c(9) * ux + c(10) * uy + c(11)
    valid = (qx >= 0) & (qx <= 1) & (qy >= 0) & (qy <= 1) & (sx >= 0) & (sx <= 1) & (sy >= 0) & (sy <= 1)
    # an invalid cell has no target (zero cells and weights); this also keeps a non-finite map out of the clamp
    i0, i1, fi = _unit_axis(torch.where(valid, qy, torch.zeros_like(qy)), gh)
    j0, j1, fj = _unit_axis(torch.where(valid, qx, torch.zeros_like(qx)), gw)
    cells = torch.stack((i0 * gw + j0, i0 * gw + j1, i1 * gw + j0, i1 * gw + j1), 2)
    wts = torch.stack(((1 - fi) * (1 - fj), (1 - fi) * fj, fi * (1 - fj), fi * fj), 2)
    keep = valid.unsqueeze(2)
    return cells * keep, wts * keep, valid


def dense_targets(warp_maps: torch.Tensor, hA: int, wA: int, hB: int, wB: int):
    """The target table of ``dense_ce`` in fp64 (the oracle of csrc/densece.hip
    ``densece_table`` and the CPU path).

    ``warp_maps`` [B, 2, 12]: row [b, 0] describes the A cells, [b, 1] the B
    cells; a row holds two affine maps (m00, m01, c0, m10, m11, c1) on unit
    coordinates (ux, uy) of its view (pixel / (extent - 1)): entries 0..5 into
    the other view's unit frame, 6..11 into the source image's.  Cell (i, j) of
    an h x w grid sits at (j / (w - 1), i / (h - 1)) (0 on an axis of length
    1).  A cell is valid when both images of it lie in [0, 1]^2; its target
    position q takes, per axis of n cells, u = clamp(q (n - 1), 0, n - 1),
    i0 = min(floor(u), max(n - 2, 0)), i1 = min(i0 + 1, n - 1), f = u - i0
    (``_keypoint_axis``), and the four cells / bilinear weights of
    ``keypoint_weight_maps``.  Returns ``(cells_a [B, R, 4] (of the B grid),
    wts_a [B, R, 4], valid_a [B, R], cells_b [B, C, 4] (of the A grid), wts_b,
    valid_b)``; invalid cells carry zero cells and weights."""
    m = warp_maps.detach().to(device="cpu", dtype=torch.float64)
    if m.dim() != 3 or m.shape[1:] != (2, 12):
        raise ValueError(f"warp_maps must be [B, 2, 12], got {tuple(warp_maps.shape)}")
    return _dense_side(m[:, 0], hA, wA, hB, wB) + _dense_side(m[:, 1], hB, wB, hA, wA)


def _dense_maps(corr4d, warp_maps):
    """x [B, R, C] and the dense weight maps V [B, R, C] (rows of valid A
    cells), U [B, R, C] (columns of valid B cells), N_A, N_B."""
    if corr4d.dim() != 6 or corr4d.shape[1] != 1:
        raise ValueError(f"dense_ce: expected a [B,1,hA,wA,hB,wB] volume, got {tuple(corr4d.shape)}")
    b, _, ha, wa, hb, wb = corr4d.shape
    dt, dev = corr4d.dtype, corr4d.device
    ca, va, oka, cb, vb, okb = dense_targets(warp_maps, ha, wa, hb, wb)
    R, C = ha * wa, hb * wb
    V = torch.zeros(b, R, C, dtype=torch.float64).scatter_add_(2, ca, va)             # coinciding cells add up
    U = torch.zeros(b, C, R, dtype=torch.float64).scatter_add_(2, cb, vb).transpose(1, 2)
    n_a, n_b = int(oka.sum()), int(okb.sum())
    return (corr4d.reshape(b, R, C), V.to(device=dev, dtype=dt), U.to(device=dev, dtype=dt),
            oka.to(dev), okb.to(dev), max(1, n_a), max(1, n_b))


def dense_ce(corr4d: torch.Tensor, warp_maps: torch.Tensor) -> torch.Tensor:
    """Dense correspondence cross-entropy of a [B,1,hA,wA,hB,wB] volume whose
    two views are affine warps of one image (an extension beyond the reference;
    the contract of csrc/densece.hip).  With ``dense_targets``' V_r the weights
    of valid A cell r on the B grid, U_m those of valid B cell m on the A grid
    and x = corr4d.view(B, R, C):

        L_A = -sum_{valid r} sum_m V_r(m) log_softmax(x[r, :])[m]
        L_B = -sum_{valid m} sum_r U_m(r) log_softmax(x[:, m])[r]
        loss = (L_A / max(1, N_A) + L_B / max(1, N_B)) / 2

    N_A, N_B: the valid cells over the batch.  A batch without a valid cell
    gives 0 (and a zero gradient)."""
    x, V, U, _, _, n_a, n_b = _dense_maps(corr4d, warp_maps)
    l_a = -(V * torch.log_softmax(x, dim=2)).sum()
    l_b = -(U * torch.log_softmax(x, dim=1)).sum()
    return (l_a / n_a + l_b / n_b) / 2


def dense_ce_grad(corr4d: torch.Tensor, warp_maps: torch.Tensor) -> torch.Tensor:
    """Closed-form d dense_ce / d corr4d (what the HIP backward evaluates):
    validA_r (softmax(x[r, :])[m] - V_r(m)) / (2 N_A) + validB_m (softmax(x[:, m])[r] - U_m(r)) / (2 N_B)."""
    x, V, U, oka, okb, n_a, n_b = _dense_maps(corr4d, warp_maps)
    ga = (torch.softmax(x, dim=2) - V) * oka.unsqueeze(2).to(x.dtype)
    gb = (torch.softmax(x, dim=1) - U) * okb.unsqueeze(1).to(x.dtype)
    return (ga / (2 * n_a) + gb / (2 * n_b)).reshape(corr4d.shape)


def match_score(corr4d: torch.Tensor, normalization: str | None = "softmax") -> torch.Tensor:
    """mean(scores_A + scores_B) / 2 (train.py:134); needs square maps like the
    reference (train.py:124) only when the two score vectors differ in length,
    in which case each direction is averaged separately."""
    sa, sb = softmax_max_scores(corr4d, normalization)
    if sa.shape == sb.shape:
        return torch.mean(sa + sb) / 2
    return (sa.mean() + sb.mean()) / 2


def warp_norm_u8(pixels: torch.Tensor, meta: torch.Tensor, params: torch.Tensor, oh: int, ow: int, mean, std,
                 dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """The definition of the augmenting input kernel (csrc/dataprep.hip
    ``warp_norm_u8``), written out: ``pixels`` the packed HWC uint8 bytes,
    ``meta`` [N, 3] = (byte offset, H, W), ``params`` [N, 8] = (a0..a5, gain,
    bias) -> [N, 3, oh, ow] in ``dtype``.  Output pixel (ox, oy) samples

        sx = clamp(a0 ox + a1 oy + a2, 0, W - 1)      sy = clamp(a3 ox + a4 oy + a5, 0, H - 1)

    (a NaN coordinate clamps to 0, as fmaxf / fminf do) bilinearly from its
    four neighbours x0 = min(floor(sx), W - 1), x1 = min(x0 + 1, W - 1) (same
    in y), then ``gain * ((v / 255 - mean[c]) / std[c]) + bias``.  fp64 (the
    default) is the oracle of the kernel tests; ``gpu_pair_batch`` runs it in
    fp32 for CPU tensors."""
    pixels, meta = pixels.cpu(), meta.cpu()
    q = params.detach().cpu().to(dtype)
    m = torch.tensor(mean, dtype=dtype).view(3, 1, 1)
    s = torch.tensor(std, dtype=dtype).view(3, 1, 1)
    oy, ox = torch.meshgrid(torch.arange(oh, dtype=dtype), torch.arange(ow, dtype=dtype), indexing="ij")
    out = torch.empty((meta.shape[0], 3, oh, ow), dtype=dtype)
    for i, (off, h, w) in enumerate(meta.tolist()):
        im = pixels[off:off + h * w * 3].view(h, w, 3).to(dtype)
        a = q[i]
        sx = torch.nan_to_num(a[0] * ox + a[1] * oy + a[2], nan=0.0).clamp(0, w - 1)
        sy = torch.nan_to_num(a[3] * ox + a[4] * oy + a[5], nan=0.0).clamp(0, h - 1)
        x0 = sx.floor().long().clamp(max=w - 1)
        y0 = sy.floor().long().clamp(max=h - 1)
        x1, y1 = (x0 + 1).clamp(max=w - 1), (y0 + 1).clamp(max=h - 1)
        fx, fy = (sx - x0).unsqueeze(2), (sy - y0).unsqueeze(2)
        v = ((1 - fy) * (1 - fx) * im[y0, x0] + (1 - fy) * fx * im[y0, x1]
             + fy * (1 - fx) * im[y1, x0] + fy * fx * im[y1, x1]).permute(2, 0, 1)
        out[i] = a[6] * ((v / 255 - m) / s) + a[7]
    return out
