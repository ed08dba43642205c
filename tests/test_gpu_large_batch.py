"""Per-GPU batches past the 32-bit index ranges, end to end through the fused
training path (forward and backward).

At 400 px a batch of B pairs sends V = 4 B volumes through the NeighConsensus
stack (B positive plus B rolled negative pairs, times the two symmetric
branches).  The 1-channel input goes in as zero-padded bf16 planes
(csrc/conv1x.hip), and every 16-channel hidden volume [V, 25, 25, 25, 25, 16]
bf16 holds 6.25e6 elements = 12.5e6 bytes per volume, which crosses
  * 2^31 bytes            at V >= 172,
  * 2^32 bytes = 2^31 elements at V >= 344,
  * 2^32 elements         at V >= 688.
Batch 48 (BASELINE config 2: 192 volumes, 2.4 GB per hidden volume) crosses the
first; the headline batch of bench.py, 256 (1024 volumes, 12.8 GB per hidden
volume, about 58 GB in all), crosses all three.  Every kernel index must be
64-bit: the big batch must reproduce, pair for pair, independent batch-16 runs
on the same features (positives only: the rolled negatives wrap at the batch
boundary), and its parameter gradients their accumulated gradients.  The
kernels one by one at this index range: tests/test_gpu_index_range.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _big_batch_matches_chunks(B, b):
    from ncnet_amd.models import ImMatchNet
    torch.manual_seed(0)
    m = ImMatchNet(ncons_kernel_sizes=[5, 5, 5], ncons_channels=[16, 16, 1]).to(DEV)
    for p in m.NeighConsensus.parameters():
        if p.dim() == 1:
            p.data.uniform_(0.0, 0.05)
    m.train()
    g = torch.Generator(device=DEV).manual_seed(3)
    src = torch.randn(B, 3, 400, 400, device=DEV, generator=g)
    tgt = torch.randn(B, 3, 400, 400, device=DEV, generator=g)
    with torch.no_grad():
        f, hw = m.extract(torch.cat((src, tgt)))
    del src, tgt
    fs, ft = f[:B], f[B:]
    params = list(m.NeighConsensus.parameters())

    def run(fa, fb):
        n = fa.shape[0]
        vols = m.weak_loss_volumes_from_features(torch.cat((fa, fb)), hw, n)
        gsel = torch.zeros_like(vols)
        gsel[:n] = torch.linspace(-1, 1, vols[:n].numel(), device=DEV).view_as(vols[:n])
        grads = torch.autograd.grad((vols * gsel).sum(), params)
        return vols[:n].detach(), grads

    big_v, big_g = run(fs, ft)
    assert torch.isfinite(big_v).all()
    acc = None
    gs_all = torch.linspace(-1, 1, big_v.numel(), device=DEV).view_as(big_v)
    for c in range(B // b):
        sl = slice(c * b, (c + 1) * b)
        vols = m.weak_loss_volumes_from_features(torch.cat((fs[sl], ft[sl])), hw, b)
        # the chunk's positives equal the big batch's (per-volume ops only)
        d = float((vols[:b].detach() - big_v[sl]).abs().max())
        assert d == 0.0, (c, d)
        # gradients: the chunk weighted by its slice of the big run's upstream gradient
        gsel = torch.zeros_like(vols)
        gsel[:b] = gs_all[sl]
        gr = torch.autograd.grad((vols * gsel).sum(), params)
        acc = list(gr) if acc is None else [a + x for a, x in zip(acc, gr)]
    for a, x in zip(acc, big_g):
        rel = float((a - x).norm() / x.norm().clamp_min(1e-30))
        assert rel < 2e-3, rel
    print(f"batch {B}: peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")


def test_batch48_matches_batch16_chunks():
    _big_batch_matches_chunks(48, 16)


def test_headline_batch_matches_batch16_chunks():
    """bench.py's headline batch: 1024 volumes, past all three thresholds."""
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    _big_batch_matches_chunks(256, 16)
    torch.cuda.empty_cache()
