"""fp64 reference and seeded inputs for the volume statistics kernels
(csrc/volume.hip stats_rows / stats_cols / stats2d), shared by
tests/test_volume_stats_ref_cpu.py and tests/test_gpu_volume_stats.py.

The reference uses nothing of the kernels' structure (no online softmax, no
partial merges): max, an explicit first-argmax, exp-sum and sums over whole
lines in fp64 on the CPU.
"""
import functools

import torch

FAMILIES = ("ties", "neg", "peaky", "flat", "planted")

# (V, R, C) of the kernel tests.  Tiles of stats2d are 64 rows x 256 columns;
# stats_cols splits the rows into chunks when V * ceil(C / 64) < 1024 blocks.
SHAPES = (
    (1, 3, 5),        # every tile partial; merges with fewer than 4 partials
    (3, 64, 256),     # exactly one tile; nchunk == 1 in stats_cols
    (2, 77, 263),     # scalar loads (C % 4 != 0); second column tile 7 wide, second row tile partial
    (2, 130, 260),    # 16-byte loads with C % 256 = 4: one live lane in the last column tile
    (1, 70, 7500),    # 30 column tiles (the row merge loops more than once per lane); chunked stats_cols
    (1, 2100, 68),    # R >= 1024: two 64-row sub-tiles per block by default; 17 row partials per column
    (1, 1030, 7),     # R >= 1024, scalar loads, last block partial
    (1, 1030, 8),     # the same with 16-byte loads
)
# run again with the sub-tile count (tuning field s2d_rt) forced to 1 and to 4
SUBTILE_SHAPES = ((1, 1030, 7), (1, 1030, 8))

# the consumers' volumes
SCORE_SHAPE = (3, 77, 263)
WEAK_SHAPE = (4, 1, 9, 8, 13, 21)        # R = 72, C = 273: more than one tile both ways, C % 4 != 0
INLOC_SHAPE = (1, 1, 9, 12, 7, 11)
# value the constant lines of 'ties' hold: below every drawn value (>= -3), so
# the other lines keep the ties they drew
TIES_CONST = -3.5


def ref_stats(x: torch.Tensor, dim: int) -> dict:
    """Statistics of ``x`` along ``dim`` in fp64 on the CPU -> dict of
    max, arg (first index of the max, int64), se = sum exp(x - max),
    sum and abs_sum = sum |x| (the scale of the plain sum's rounding)."""
    x = x.detach().to("cpu", torch.float64)
    n = x.shape[dim]
    mx = x.amax(dim)
    view = [1] * x.dim()
    view[dim] = n
    idx = torch.arange(n).view(view)
    # the tie rule, spelled out: the smallest index that holds the max
    arg = torch.where(x == mx.unsqueeze(dim), idx, torch.full_like(idx, n)).amin(dim)
    return {"max": mx, "arg": arg, "se": torch.exp(x - mx.unsqueeze(dim)).sum(dim), "sum": x.sum(dim),
            "abs_sum": x.abs().sum(dim)}


def tie_share(x: torch.Tensor, dim: int) -> float:
    """Share of the lines along ``dim`` whose max is held by more than one element."""
    x = x.detach().to("cpu", torch.float64)
    return float(((x == x.amax(dim, keepdim=True)).sum(dim) > 1).double().mean())


def tie_levels(shape) -> int:
    """Number of distinct values 'ties' draws from: 50 (randint(0, 50) / 7 - 3,
    the draw of test_stats2d_matches_row_and_col_kernels) where the shorter
    line has >= 100 elements; half the shorter line's length below that (at
    least 2), since a line of n draws from L levels has a unique max with
    probability about (n / L) * sum_j (j / L)^(n - 1): 0.31 at L = n / 2, but
    0.8 for the 7-element rows of (1, 1030, 7) at L = 50 -- the family would
    hardly test the tie rule there."""
    return min(50, max(2, min(shape[1], shape[2]) // 2))


def border_positions(n: int):
    """First and last index, both sides of the 64-wide (wave / row tile) and
    256-wide (column tile) borders, where they exist."""
    return sorted({p for p in (0, 63, 64, 255, 256, n - 1) if 0 <= p < n})


def _seed(family: str, shape) -> int:
    return sum(map(ord, family)) * 1000003 + shape[0] * 10007 + shape[1] * 101 + shape[2]


def make_volume(family: str, shape) -> torch.Tensor:
    """[V, R, C] fp32 on the CPU, seeded by (family, shape)."""
    V, R, C = shape
    g = torch.Generator().manual_seed(_seed(family, shape))
    if family == "ties":
        x = torch.randint(0, tie_levels(shape), shape, generator=g).float() / 7.0 - 3.0
        # whole lines of one constant (first argmax 0); the same constant both
        # ways so the lines stay constant where they cross.  Only where the
        # lines across them are long enough to keep their own ties.
        if R >= 8:
            x[:, [1, R - 1], :] = TIES_CONST
        if C >= 8:
            x[:, :, [2, C - 1]] = TIES_CONST
        return x
    if family == "neg":
        return -1.0 - 40.0 * torch.rand(shape, generator=g)
    if family == "peaky":
        return 30.0 * torch.randn(shape, generator=g)
    if family == "flat":
        return 5.0 + 1e-3 * torch.rand(shape, generator=g)
    if family == "planted":
        x = torch.rand(shape, generator=g)
        pc, pr = border_positions(C), border_positions(R)
        r, c = torch.arange(R), torch.arange(C)
        # row r: 2 + r / R at column pc[r % len]; then column c: 4 + c / C at row
        # pr[c % len].  Every column's max is its planted value; so is every
        # row's but the <= 6 rows of pr, whose max is one of the column values.
        x[:, r, torch.tensor(pc)[r % len(pc)]] = 2.0 + r.float() / R
        x[:, torch.tensor(pr)[c % len(pr)], c] = 4.0 + c.float() / C
        return x
    raise ValueError(family)


def planted_expect(shape):
    """-> (column argmax [C], rows whose argmax is the row's own planted column
    (bool [R]), that column [R]) of the 'planted' volume."""
    V, R, C = shape
    pc, pr = border_positions(C), border_positions(R)
    r, c = torch.arange(R), torch.arange(C)
    own = torch.ones(R, dtype=torch.bool)
    own[torch.tensor(pr)] = False
    return torch.tensor(pr)[c % len(pr)], own, torch.tensor(pc)[r % len(pc)]


@functools.lru_cache(maxsize=None)
def case(family: str, shape):
    """(volume [V, R, C] fp32 CPU, row statistics (dim 2), column statistics
    (dim 1)), computed once per (family, shape); callers must not modify it."""
    x = make_volume(family, tuple(shape))
    return x, ref_stats(x, 2), ref_stats(x, 1)


def distinct(shape, seed: int, lo: float = 0.0, hi: float = 1.0) -> torch.Tensor:
    """fp32 values in (lo, hi), all different (a shuffled grid): no ties at
    all, for comparisons with code whose tie rule is not pinned down (autograd
    of max, torch.max)."""
    n = 1
    for s in shape:
        n *= s
    g = torch.Generator().manual_seed(seed)
    u = (torch.randperm(n, generator=g).double() + 0.5) / n
    x = (lo + (hi - lo) * u).float()
    assert x.unique().numel() == n
    return x.view(shape)


def weak_volume(kind: str) -> torch.Tensor:
    """The weak-loss test volume [4, 1, 9, 8, 13, 21]: 'tie_free' (distinct values
    in (0, 3)) or 'neg' (the all-negative family; its line maxima are unique,
    which tests/test_volume_stats_ref_cpu.py asserts)."""
    V, _, i, j, k, l = WEAK_SHAPE
    if kind == "tie_free":
        return distinct(WEAK_SHAPE, 11, 0.0, 3.0)
    if kind == "neg":
        return make_volume("neg", (V, i * j, k * l)).view(WEAK_SHAPE)
    raise ValueError(kind)


def inloc_volume() -> torch.Tensor:
    """The match-extraction test volume [1, 1, 9, 12, 7, 11]: distinct values in
    (0, 5), so softmax scores are well away from both 1 / n and 1."""
    return distinct(INLOC_SHAPE, 12, 0.0, 5.0)
