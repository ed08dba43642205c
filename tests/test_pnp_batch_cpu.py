"""Batched P3P LO-RANSAC API on the CPU (ncnet_amd/eval/localization_gpu.py):
``device='cpu'`` runs the numpy ``p3p_ransac`` per problem with
``default_rng(key)``, and ``inloc_localize.py --pnp_device gpu`` on a machine
without a GPU takes that path, writes the poses of ``--pnp_device cpu`` and
keeps its cache apart from the numpy path's."""
import glob
import os

import numpy as np
import pytest
import torch

from ncnet_amd.eval.localization import p3p_ransac
from ncnet_amd.eval.localization_gpu import key_to_int64, p3p_ransac_batch


def _rand_pose(rng):                                   # the generators of tests/test_localization.py
    A = rng.normal(size=(3, 3))
    Q, _ = np.linalg.qr(A)
    if np.linalg.det(Q) < 0:
        Q[:, 0] *= -1
    t = rng.normal(size=3)
    return np.hstack([Q, t[:, None]])


def _scene(rng, n, P):
    Xc = np.stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.uniform(3, 8, n)])
    R, t = P[:, :3], P[:, 3:4]
    return Xc, R.T @ (Xc - t)


def _problem(rng, n, outliers):
    P = _rand_pose(rng)
    Xc, Xw = _scene(rng, n, P)
    rays = Xc / np.linalg.norm(Xc, axis=0)
    rays += rng.normal(scale=1e-4, size=rays.shape)
    out = rng.random(n) < outliers
    rays[:, out] = rng.normal(size=(3, int(out.sum())))
    rays[2, out] = np.abs(rays[2, out])
    return rays, Xw


def test_batch_cpu_equals_p3p_ransac_per_problem():
    rng = np.random.default_rng(7)
    sizes = [50, 0, 200, 2, 3]
    problems = [_problem(rng, n, 0.4 if n == 200 else 0.0) for n in sizes]
    keys = [11, 12, 13, 14, [5, 0, 2]]
    thr = np.radians(0.2)
    got = p3p_ransac_batch(problems, thr, max_iters=500, keys=keys, device="cpu")
    assert len(got) == len(sizes)
    for (rays, X), k, n, (P, inl) in zip(problems, keys, sizes, got):
        Pw, iw = p3p_ransac(rays, X, thr, max_iters=500, rng=np.random.default_rng(k))
        assert inl.shape == (n,) and inl.dtype == bool
        assert np.array_equal(inl, iw)
        if n < 3:
            assert P is None and Pw is None and not inl.any()
        else:
            assert P is not None and np.array_equal(P, Pw)
    assert got[2][1].sum() > 100                       # the 40 % outlier problem found its consensus


def test_keys_and_argument_checks():
    assert key_to_int64(5) == 5 and key_to_int64(-1) == -1
    k = key_to_int64([0, 3, 1])
    assert -(1 << 63) <= k < (1 << 63) and k == key_to_int64([0, 3, 1]) and k != key_to_int64([0, 1, 3])
    with pytest.raises(ValueError):
        p3p_ransac_batch([(np.zeros((3, 4)), np.zeros((3, 4)))], 0.01, keys=[1, 2], device="cpu")
    with pytest.raises(ValueError):
        p3p_ransac_batch([(np.zeros((3, 4)), np.zeros((3, 5)))], 0.01, device="cpu")
    assert p3p_ransac_batch([], 0.01, device="cpu") == []


def test_cli_pnp_device_gpu_falls_back_and_caches_apart(tmp_path, monkeypatch):
    import inloc_localize as il
    from ncnet_amd.eval import localization_gpu
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)     # a machine without a GPU
    cache = str(tmp_path / "cache")
    base = ["--synthetic", "2", "--workers", "1", "--ransac_iters", "300"]
    il.main(base + ["--pnp_device", "cpu", "--out", "cpu.npz", "--cache_dir", cache])
    cpu_files = sorted(glob.glob(os.path.join(cache, "pnp", "**", "*.npz"), recursive=True))
    assert len(cpu_files) == 6

    # a second cpu run reuses the cache: the solver is not called again
    calls = []
    real = il.p3p_ransac
    monkeypatch.setattr(il, "p3p_ransac", lambda *a, **k: calls.append(1) or real(*a, **k))
    il.main(base + ["--pnp_device", "cpu", "--out", "cpu2.npz", "--cache_dir", cache])
    assert not calls

    # the gpu run does not: all 6 pairs go to the batched solver, which falls back to numpy here
    batches = []
    real_batch = localization_gpu.p3p_ransac_batch
    monkeypatch.setattr(localization_gpu, "p3p_ransac_batch",
                        lambda problems, *a, **k: batches.append(len(problems)) or real_batch(problems, *a, **k))
    il.main(base + ["--pnp_device", "gpu", "--out", "gpu.npz", "--cache_dir", cache])
    assert sum(batches) == 6
    assert sorted(glob.glob(os.path.join(cache, "pnp", "**", "*.npz"), recursive=True)) == cpu_files
    assert len(glob.glob(os.path.join(cache, "pnp_gpu", "**", "*.npz"), recursive=True)) == 6
    # ... and a second gpu run reuses its own
    il.main(base + ["--pnp_device", "gpu", "--out", "gpu2.npz", "--cache_dir", cache])
    assert sum(batches) == 6

    a = np.load("cpu.npz")
    for name in ("cpu2.npz", "gpu.npz", "gpu2.npz"):
        b = np.load(name)
        assert list(a["queries"]) == list(b["queries"])
        assert np.array_equal(a["poses"], b["poses"], equal_nan=True)
        assert np.array_equal(a["inliers"], b["inliers"])
    assert np.isfinite(a["poses"]).all() and (a["inliers"] > 100).all()
