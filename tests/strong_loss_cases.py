"""Inputs shared by tests/test_strong_loss_cpu.py and tests/test_gpu_strong_loss.py."""
import torch

# name -> (B, N, hA, wA, hB, wB), source image (h, w), target image (h, w)
CASES = {
    "small": ((2, 5, 3, 4, 5, 3), (48, 64), (80, 48)),       # lines shorter than a wave, non-square
    "edge": ((3, 20, 6, 7, 5, 9), (96, 112), (80, 144)),
    "train": ((2, 20, 25, 25, 25, 25), (400, 400), (400, 400)),   # the training plane: C = 625 is odd
    "wide": ((1, 3, 2, 2, 40, 50), (100, 100), (200, 250)),  # C = 2000 >> the workgroup, R = 4
}


def make_case(name: str, device="cpu"):
    """-> (x [B,1,hA,wA,hB,wB] fp32, (source_points, target_points [B,2,N],
    source_im_size, target_im_size [B,3])).  'edge' holds, in image 0: points at
    (1, 1) and (w, h), two points outside the image, two keypoints in one
    cell and three -1 padded slots; image 1 has no keypoints; image 2 has five
    padded slots and one pair with a single -1 coordinate (invalid)."""
    (B, N, hA, wA, hB, wB), (sh, sw), (th, tw) = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randn(B, 1, hA, wA, hB, wB, generator=g) * 2
    u = lambda: torch.rand(B, N, generator=g)  # noqa: E731
    sp = torch.stack((1 + u() * (sw - 1), 1 + u() * (sh - 1)), 1)
    tp = torch.stack((1 + u() * (tw - 1), 1 + u() * (th - 1)), 1)
    if name == "edge":
        sp[0, :, 0] = torch.tensor([1.0, 1.0])
        tp[0, :, 0] = torch.tensor([float(tw), float(th)])
        sp[0, :, 1] = torch.tensor([float(sw), float(sh)])
        tp[0, :, 1] = torch.tensor([1.0, 1.0])
        sp[0, :, 2] = torch.tensor([-5.5, 10.0])
        tp[0, :, 2] = torch.tensor([20.0, th + 12.0])
        sp[0, :, 3] = torch.tensor([sw + 7.0, sh + 3.0])
        tp[0, :, 3] = torch.tensor([-3.0, -2.0])
        sp[0, :, 4] = torch.tensor([30.0, 20.5])
        sp[0, :, 5] = torch.tensor([31.0, 21.5])
        tp[0, :, 5] = tp[0, :, 4] + 1.0
        sp[0, :, -3:] = -1.0
        tp[0, :, -3:] = -1.0
        sp[1], tp[1] = -1.0, -1.0
        sp[2, :, -5:] = -1.0
        tp[2, :, -5:] = -1.0
        sp[2, 0, 7] = -1.0                       # one coordinate of four: the pair is invalid
    if name == "train":
        sp[1, :, -4:] = -1.0
        tp[1, :, -4:] = -1.0
    ssz = torch.tensor([float(sh), float(sw), 3.0]).expand(B, 3).contiguous()
    tsz = torch.tensor([float(th), float(tw), 3.0]).expand(B, 3).contiguous()
    return x.to(device), tuple(t.to(device) for t in (sp, tp, ssz, tsz))


def learning_setup(device, seed: int = 0, B: int = 4):
    """The learning check's fixed batch: 8x8x8x8 correlation volumes of
    32-channel unit features whose target is the source rolled by one cell
    along x plus 0.3 noise; 10 valid keypoints per image with tp = sp + 8 px (one
    cell) on 64 px images; NC (3,3)/(16,1)."""
    from ncnet_amd.models import ImMatchNet
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    fa = torch.nn.functional.normalize(torch.randn(B, 32, 8, 8, generator=g), dim=1)
    fb = torch.nn.functional.normalize(torch.roll(fa, 1, 3) + 0.3 * torch.randn(B, 32, 8, 8, generator=g), dim=1)
    corr = torch.bmm(fa.flatten(2).transpose(1, 2), fb.flatten(2)).view(B, 1, 8, 8, 8, 8)
    sp = 1 + torch.rand(B, 2, 10, generator=g) * 54
    tp = sp.clone()
    tp[:, 0] += 8.0
    sz = torch.tensor([64.0, 64.0, 3.0]).expand(B, 3).contiguous()
    batch = {"source_points": sp, "target_points": tp, "source_im_size": sz, "target_im_size": sz.clone()}
    model = ImMatchNet(use_cuda=torch.device(device).type == "cuda", ncons_kernel_sizes=[3, 3],
                       ncons_channels=[16, 1]).to(device)
    return model, corr.to(device), {k: v.to(device) for k, v in batch.items()}


def run_learning(model, corr, batch, steps: int = 40, lr: float = 5e-3):
    """Adam on the NC parameters for ``steps`` steps on the fixed batch ->
    (loss of the first step, loss of the last step)."""
    from ncnet_amd.ops.loss import strong_loss_from_corr
    model.train()
    opt = torch.optim.Adam(model.NeighConsensus.parameters(), lr=lr)
    losses = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = strong_loss_from_corr(model.process_correlation(corr), batch)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    return float(losses[0]), float(losses[-1])
