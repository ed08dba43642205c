"""Batched dense pose verification API on the CPU
(ncnet_amd/eval/pose_verification_gpu.py): ``device='cpu'`` runs ``pv_score``
per candidate, ``inloc_localize.py --pv_device gpu`` on a machine without a GPU
takes that path, re-ranks as ``--pv_device cpu`` does and keeps its cache apart
from the torch path's; the kernels of csrc/pv.hip compile without scratch."""
import glob
import os
import shutil

import numpy as np
import pytest
import torch

from ncnet_amd import kernel_resources as kr
from ncnet_amd.eval import pose_verification as pv
from ncnet_amd.eval import pose_verification_gpu as pvg
from tests import pv_scene as S


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def test_scene_is_the_documented_one():
    """The figures the scene was designed to: scores, coverage, guards."""
    _, _, xyz = S.scene()
    for name, score, covered in (("true", 25.1, 4800), ("bad", 1.06, 3610), ("near", 3.87, 4612)):
        s, _, flag, errmap = S.reference(name)
        assert abs(s - score) < 0.01 * score and int(flag.sum()) == covered
        assert errmap.shape == (8, 13) and 93 <= int((~np.isnan(errmap)).sum()) <= 104
        dist, gap = S.check_guards(xyz, S.POSES[name])
        assert dist > S.GUARD and gap > S.GUARD


def test_batch_cpu_equals_pv_score_per_candidate():
    q, rgb, xyz = S.scene()
    q2 = q[:, ::-1].copy()                                   # a second query image of the same size
    queries = [q, q2, q, q, q]
    poses = [S.POSES["true"], S.POSES["near"], None, np.full((3, 4), np.nan), S.POSES["bad"]]   # two share q
    scores, maps = pvg.pv_scores_batch(queries, rgb, xyz, poses, S.FOCAL, device="cpu", ds=S.DS, return_maps=True)
    assert pvg.pv_scores_batch(queries, rgb, xyz, poses, S.FOCAL, device="cpu", ds=S.DS) == scores
    assert len(scores) == len(maps) == 5 and scores[2] == scores[3] == 0.0 and scores[0] > scores[4] > 0
    for qi, P, s, m in zip(queries, poses, scores, maps):
        want = pv.pv_score(qi, rgb, xyz, P, S.FOCAL, device="cpu", ds=S.DS)
        assert s == want[0] and isinstance(s, float)
        assert all(_same(a, b) for a, b in zip(m, want[1:]))
    # an empty scan
    scores, maps = pvg.pv_scores_batch([q, q], rgb[:0], xyz[:0], [S.POSES["true"], None], S.FOCAL, device="cpu", ds=S.DS,
                                       return_maps=True)
    want = pv.pv_score(q, rgb[:0], xyz[:0], S.POSES["true"], S.FOCAL, device="cpu", ds=S.DS)
    assert scores == [0.0, 0.0] and want[0] == 0.0
    assert all(_same(a, b) for a, b in zip(maps[0], want[1:])) and maps[1] == (None, None, None)
    assert pvg.pv_scores_batch([], rgb, xyz, [], S.FOCAL, device="cpu") == []
    with pytest.raises(ValueError):
        pvg.pv_scores_batch([q], rgb, xyz, [], S.FOCAL, device="cpu")


def test_batched_image_stages_equal_the_per_image_ones():
    """The [B, h, w] forms of the image stages against pose_verification.py's,
    on the CPU: in-painting and the normalisation exactly (same operations per
    element up to the order of two sums), the pooled maps through dense_sift."""
    sides = [S.sides_cpu(S.POSES[n]) for n in ("bad", "near")]
    _, rgb, xyz = S.scene()
    gs = []
    for n in ("bad", "near"):
        synth, flag = S.render_cpu(rgb, xyz, S.POSES[n])
        g = pv.rgb2gray(torch.as_tensor(synth)) / 255.0
        gs.append(torch.where(torch.as_tensor(flag), g, torch.full_like(g, float("nan"))))
    flags = torch.stack([s[2] for s in sides])
    filled = pvg.inpaint_nans_batch(torch.stack(gs))
    for j in range(2):
        assert torch.allclose(filled[j], pv.inpaint_nans(gs[j]), rtol=0, atol=1e-5)
    norm = pvg.image_normalization_batch(filled, flags)
    for j in range(2):
        assert torch.allclose(norm[j], sides[j][1], rtol=0, atol=1e-4)
    one = torch.zeros(1, 60, 80, dtype=torch.bool)
    one[0, 3, 4] = True                                     # fewer than 2 valid pixels: zeros
    assert float(pvg.image_normalization_batch(filled[:1], one).abs().max()) == 0.0
    # pooled maps -> descriptors as dense_sift finishes them
    o = pvg.pooled_orientation_maps(norm)
    ys, xs = torch.arange(15, 60 - 15, 4), torch.arange(15, 80 - 15, 4)
    offs = torch.tensor([-12, -4, 4, 12])
    by, bx = ys[:, None] + offs[None], xs[:, None] + offs[None]
    for j in range(2):
        d = o[j][:, by[:, None, :, None], bx[None, :, None, :]].permute(1, 2, 3, 4, 0).reshape(-1, 128)
        d = d / d.norm(dim=1, keepdim=True).clamp_min(1e-12)
        d = d.clamp(max=0.2)
        d = d / d.norm(dim=1, keepdim=True).clamp_min(1e-12)
        _, want = pv.dense_sift(norm[j])
        assert torch.allclose(d.T, want, rtol=0, atol=1e-4)


def test_cli_pv_device_gpu_falls_back_and_caches_apart(tmp_path, monkeypatch):
    import inloc_localize as il
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)     # a machine without a GPU
    cache = str(tmp_path / "cache")
    base = ["--synthetic", "2", "--workers", "1", "--ransac_iters", "300", "--pv", "--cache_dir", cache]
    est_cpu, rate_cpu = il.main(base + ["--pv_device", "cpu", "--name", "cpu", "--out", "cpu.npz"])
    pv_files = sorted(glob.glob(os.path.join(cache, "pv", "**", "*.npz"), recursive=True))
    assert len(pv_files) == 6
    pv_bytes = [open(f, "rb").read() for f in pv_files]

    batches = []
    real = pvg.pv_scores_batch
    monkeypatch.setattr(pvg, "pv_scores_batch",
                        lambda qs, *a, **k: batches.append(len(qs)) or real(qs, *a, **k))
    est_gpu, rate_gpu = il.main(base + ["--pv_device", "gpu", "--name", "gpu", "--out", "gpu.npz"])
    assert sum(batches) == 6 and len(batches) == 2          # one call per scan
    assert sorted(glob.glob(os.path.join(cache, "pv", "**", "*.npz"), recursive=True)) == pv_files
    assert [open(f, "rb").read() for f in pv_files] == pv_bytes
    assert len(glob.glob(os.path.join(cache, "pv_gpu", "**", "*.npz"), recursive=True)) == 6
    # a second gpu run reuses its own cache: no scoring call
    est_gpu2, _ = il.main(base + ["--pv_device", "gpu", "--name", "gpu2", "--out", "gpu2.npz"])
    assert sum(batches) == 6

    assert open("error_cpu_PV.txt").read() == open("error_gpu_PV.txt").read() == open("error_gpu2_PV.txt").read()
    for est in (est_gpu, est_gpu2):
        assert {k: v[0] for k, v in est.items()} == {k: v[0] for k, v in est_cpu.items()}
    assert np.array_equal(rate_cpu, rate_gpu) and (rate_gpu[1:] == 1.0).all()       # rate[0]: the 0 m threshold
    # pano 0 carries the wrong pose on purpose: verification must have moved every query off it
    assert all(not v[0].endswith("_0_0") for v in est_cpu.values())


@pytest.mark.skipif(shutil.which(kr.HIPCC) is None and not os.path.exists(kr.HIPCC), reason="hipcc not available")
def test_pv_kernels_do_not_spill():
    recs = kr.analyse(kr.CSRC / "pv.hip")
    names = [kr.short(r.get("name", r["mangled"])) for r in recs]
    assert len(recs) >= 4, names                            # depth, resolve, gather, descriptor distance
    bad = [(n, r.get("scratch"), r.get("vgpr_spill")) for n, r in zip(names, recs)
           if r.get("scratch", 0) or r.get("vgpr_spill", 0)]
    assert not bad, f"scratch / VGPR spills in csrc/pv.hip: {bad}"
