"""Inputs shared by tests/test_dense_warp_cpu.py and tests/test_gpu_dense_warp.py."""
import math

import torch

# name -> (B, hA, wA, hB, wB)
CASES = {
    "small": (2, 3, 4, 5, 3),        # lines shorter than a wave, non-square grids
    "odd": (3, 6, 7, 5, 9),          # hand-built maps, see make_case
    "train": (2, 25, 25, 25, 25),    # the training plane: R = C = 625 is odd, rows straddle 16-byte lanes
    "wide": (1, 2, 2, 40, 50),       # C = 2000, R = 4
}
# source image sizes (H, W) and the output frame of the draw_params maps of the random cases
_SOURCES = {"small": [(300, 400), (420, 360)], "train": [(333, 500), (600, 450)], "wide": [(375, 500)]}
_OUT = (400, 400)

IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def _compose(f, g):
    """(m00, m01, c0, m10, m11, c1) of f o g."""
    F, G = torch.tensor(f, dtype=torch.float64), torch.tensor(g, dtype=torch.float64)
    Fm, Gm = F[[0, 1, 3, 4]].view(2, 2), G[[0, 1, 3, 4]].view(2, 2)
    M, c = Fm @ Gm, Fm @ G[[2, 5]] + F[[2, 5]]
    return [float(M[0, 0]), float(M[0, 1]), float(c[0]), float(M[1, 0]), float(M[1, 1]), float(c[1])]


def _invert(f):
    F = torch.tensor(f, dtype=torch.float64)
    Mi = torch.linalg.inv(F[[0, 1, 3, 4]].view(2, 2))
    c = -Mi @ F[[2, 5]]
    return [float(Mi[0, 0]), float(Mi[0, 1]), float(c[0]), float(Mi[1, 0]), float(Mi[1, 1]), float(c[1])]


def out_of_frame_maps(B: int) -> torch.Tensor:
    """[B, 2, 12]: every cell of either view lands 5 frames to the side of the
    other view; y and the source positions stay strictly inside their frames."""
    inner = [0.9, 0.0, 0.05, 0.0, 0.9, 0.05]
    row_a = [1.0, 0.0, 5.0, 0.0, 0.9, 0.05] + inner
    row_b = [1.0, 0.0, -5.0, 0.0, 0.9, 0.05] + inner
    return torch.tensor([row_a, row_b], dtype=torch.float64).expand(B, 2, 12).contiguous()


def odd_maps() -> torch.Tensor:
    """The 'odd' case.  Image 0: the identity (every cell valid; cell centres
    exactly on the frame border; the last cell of an axis at i0 = n - 2,
    f = 1; on the equal-length axes of a square pair the weights are one-hot).
    Image 1: every cell out of the other frame.  Image 2: a flipped, rotated,
    scaled map, with view A showing the source magnified and shifted so that
    part of both views looks past the source's border."""
    ident = [IDENTITY + IDENTITY, IDENTITY + IDENTITY]
    th, z = math.radians(20.0), 0.9
    c, s = z * math.cos(th), z * math.sin(th)
    M = [[-c, -s], [-s, c]]                                       # R(theta) z diag(-1, 1)
    a2b = [M[0][0], M[0][1], 0.5 - 0.5 * (M[0][0] + M[0][1]) + 0.05, M[1][0], M[1][1],
           0.5 - 0.5 * (M[1][0] + M[1][1]) - 0.03]
    b2a = _invert(a2b)
    a2s = [1.1, 0.0, 0.07, 0.0, 1.1, -0.12]
    b2s = _compose(a2s, b2a)
    return torch.cat((torch.tensor([ident], dtype=torch.float64), out_of_frame_maps(1),
                      torch.tensor([[a2b + a2s, b2a + b2s]], dtype=torch.float64)), 0)


def shift_maps(B: int, n: int = 8) -> torch.Tensor:
    """[B, 2, 12]: view B is view A shifted by one cell of an n-cell axis along
    x (A cell (i, j) shows what B cell (i, j + 1) shows); the source maps are
    the identity, so only the other frame decides validity."""
    d = 1.0 / (n - 1)
    row_a = [1.0, 0.0, d, 0.0, 1.0, 0.0] + IDENTITY
    row_b = [1.0, 0.0, -d, 0.0, 1.0, 0.0] + IDENTITY
    return torch.tensor([row_a, row_b], dtype=torch.float64).expand(B, 2, 12).contiguous()


def make_case(name: str, device="cpu"):
    """-> (x [B,1,hA,wA,hB,wB] fp32 = 2 randn, warp_maps [B,2,12] fp64).  The maps
    of 'small', 'train' and 'wide' are data.augment.view_maps of draw_params
    rows (default PairAugment) on a fixed seed; 'odd' is ``odd_maps``."""
    from ncnet_amd.data.augment import PairAugment, draw_params, view_maps
    B, hA, wA, hB, wB = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randn(B, 1, hA, wA, hB, wB, generator=g) * 2
    if name == "odd":
        maps = odd_maps()
    else:
        meta = torch.tensor([[0, h, w] for h, w in _SOURCES[name]] * 2, dtype=torch.int64)
        params = draw_params(meta, _OUT[0], _OUT[1], PairAugment(), g)
        maps = view_maps(params, meta, _OUT[0], _OUT[1])
    assert maps.shape == (B, 2, 12)
    return x.to(device), maps.to(device)


def dense_weight_maps(cells: torch.Tensor, wts: torch.Tensor, n_other: int) -> torch.Tensor:
    """cells / wts [B, n, 4] -> [B, n, n_other] dense maps; coinciding cells add up."""
    out = torch.zeros(cells.shape[0], cells.shape[1], n_other, dtype=torch.float64)
    return out.scatter_add_(2, cells.long().cpu(), wts.double().cpu())


def learning_setup(device, seed: int = 1):
    """tests/strong_loss_cases.learning_setup (8x8x8x8 volumes whose target is
    the source rolled by one cell along x) with the maps 'B = A shifted by one
    cell' in place of its keypoints."""
    from tests.strong_loss_cases import learning_setup as strong_setup
    model, corr, _ = strong_setup(device, seed=seed)
    return model, corr, {"warp_maps": shift_maps(corr.shape[0], 8).to(device)}


def run_learning(model, corr, batch, steps: int = 40, lr: float = 5e-3):
    """Adam on the NC parameters for ``steps`` steps on the fixed batch ->
    (loss of the first step, loss of the last step)."""
    from ncnet_amd.ops.loss import warp_loss_from_corr
    model.train()
    opt = torch.optim.Adam(model.NeighConsensus.parameters(), lr=lr)
    losses = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = warp_loss_from_corr(model.process_correlation(corr), batch)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    return float(losses[0]), float(losses[-1])
