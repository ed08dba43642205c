"""Batched P3P LO-RANSAC on the MI355X (csrc/pnp.hip, eval/localization_gpu.py)
against the numpy back end (eval/localization.py): the minimal solver, the
consensus it finds, batch / key semantics, a mutation that shows every point is
scored, the inloc_localize.py --pnp_device gpu command line and the binding's
argument checks."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ncnet_amd.eval.localization import angular_errors, p3p, pose_distance
from ncnet_amd.eval.localization_gpu import key_to_int64, p3p_ransac_batch, p3p_solve

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = np.radians(0.2)
BAND = 1e-9                                            # rad around the threshold where fp64 rounding may decide
WG = 256                                               # hypotheses per sampling round (csrc/pnp.hip)


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
    """The scenario of test_p3p_ransac_with_outliers: (P, rays, Xw, outlier flags)."""
    P = _rand_pose(rng)
    Xc, Xw = _scene(rng, n, P)
    rays = Xc / np.linalg.norm(Xc, axis=0)
    rays += rng.normal(scale=1e-4, size=rays.shape)
    out = rng.random(n) < outliers
    rays[:, out] = rng.normal(size=(3, int(out.sum())))
    rays[2, out] = np.abs(rays[2, out])
    return P, rays, Xw, out


def _noise(rng, n):
    rays = rng.normal(size=(3, n))
    rays[2] = np.abs(rays[2])
    return rays, rng.uniform(-5, 5, (3, n))


def _raw(problems, keys, max_iters, thr=THR, confidence=0.999, lo_iters=20):
    """The binding itself: (P [B, 3, 4], n_inliers [B], mask [N], rounds [B]) as numpy."""
    from ncnet_amd.ops import _ext
    sizes = [r.shape[1] for r, _ in problems]
    rays = np.concatenate([r.T for r, _ in problems]) if problems else np.zeros((0, 3))
    X = np.concatenate([x.T for _, x in problems]) if problems else np.zeros((0, 3))
    dev = "cuda"
    off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=dev)
    k = torch.tensor([key_to_int64(v) for v in keys], dtype=torch.int64, device=dev)
    rounds = torch.zeros(len(problems), dtype=torch.int32, device=dev)
    P, n, m = _ext.ext().p3p_ransac_batch(torch.tensor(rays, dtype=torch.float64, device=dev).contiguous(),
                                          torch.tensor(X, dtype=torch.float64, device=dev).contiguous(), off, k,
                                          float(thr), max_iters, confidence, lo_iters, rounds)
    return P.cpu().numpy(), n.cpu().numpy(), m.cpu().numpy().astype(bool), rounds.cpu().numpy()


def _check_consensus(P_true, rays, Xw, out, Pe, inl, n_inl=None, pose=True):
    """The pass criteria of test_p3p_ransac_with_outliers + the mask is the numpy
    inlier test of the returned pose.  pose=False leaves the pose-error bound out."""
    assert Pe is not None
    dpos, dori = pose_distance(P_true, Pe)
    print(f"n={rays.shape[1]} outliers={out.mean():.2f}: dpos={dpos:.3e} dori={dori:.3e} "
          f"inliers found={inl[~out].mean():.4f} outliers accepted={inl[out].mean():.4f} n_inl={inl.sum()}")
    assert not pose or (dpos < 1e-2 and dori < 1e-2)
    assert inl[~out].mean() > 0.95 and inl[out].mean() < 0.05
    err = angular_errors(Pe, rays, Xw)
    assert not (np.abs(err - THR) < BAND).any(), "a seeded point lies in the rounding band: change the seed"
    assert np.array_equal(inl, err < THR)
    if n_inl is not None:
        assert n_inl == inl.sum()


@pytest.fixture(scope="module")
def scenario():
    """200 points, 40 % outliers, 1e-4 ray noise (test_p3p_ransac_with_outliers)."""
    return _problem(np.random.default_rng(2), 200, 0.4)


# ---------------------------------------------------------------------------
def _angle(a, b):
    return np.arctan2(np.linalg.norm(np.cross(a, b, axis=0), axis=0), (a * b).sum(0))


def test_p3p_solve_matches_numpy_and_ground_truth():
    rng = np.random.default_rng(11)
    M = 2000
    poses, rays, X = [], np.zeros((M, 3, 3)), np.zeros((M, 3, 3))
    for m in range(M):
        P = _rand_pose(rng)
        Xc, Xw = _scene(rng, 3, P)
        poses.append(P)
        rays[m], X[m] = Xc.T, Xw.T                     # row k = k-th point; camera-frame points as rays
    G, nsol = p3p_solve(rays, X)
    assert G.shape == (M, 4, 3, 4) and nsol.shape == (M,)
    kept, worst, worst_orth, worst_rep = 0, 0.0, 0.0, 0.0
    for m in range(M):
        k = int(nsol[m])
        assert 0 <= k <= 4
        assert np.isfinite(G[m, :k]).all() and np.isnan(G[m, k:]).all()
        f = rays[m].T / np.linalg.norm(rays[m].T, axis=0)
        for S in G[m, :k]:
            R = S[:, :3]
            worst_orth = max(worst_orth, np.abs(R @ R.T - np.eye(3)).max(), abs(np.linalg.det(R) - 1.0))
            Y = R @ X[m].T + S[:, 3:4]
            assert (Y[2] > 0).all()
            worst_rep = max(worst_rep, _angle(f, Y).max())
        sols = p3p(rays[m].T, X[m].T)
        if min((np.abs(S - poses[m]).max() for S in sols), default=np.inf) < 1e-6:
            kept += 1
            worst = max(worst, min((np.abs(S - poses[m]).max() for S in G[m, :k]), default=np.inf))
            assert k == len(sols), (m, k, len(sols))
    print(f"kept {kept} of {M}; worst pose error {worst:.3e}; R R^T / det {worst_orth:.3e}; reprojection {worst_rep:.3e} rad")
    assert kept >= 0.99 * M
    assert worst < 1e-6
    assert worst_orth < 1e-9 and worst_rep < 1e-9


def test_p3p_solve_degenerate_input_has_no_solution():
    rays = np.tile(np.array([[0.1, 0.0, 1.0], [0.0, 0.2, 1.0], [-0.1, 0.1, 1.0]]), (3, 1, 1))
    X = np.array([[[0, 0, 5.0], [0, 0, 5.0], [1, 2, 6.0]],            # two identical world points
                  [[0, 0, 5.0], [1, 2, 6.0], [2, 4, 7.0]],            # three collinear points
                  [[0, 0, 5.0], [1, 0, 5.0], [0, 1, 5.0]]])           # a proper triangle for contrast
    G, nsol = p3p_solve(rays, X)
    assert nsol.dtype == np.int32
    assert nsol[0] == 0 and nsol[1] == 0 and 0 <= nsol[2] <= 4
    assert np.isnan(G[:2]).all()


# ---------------------------------------------------------------------------
def test_consensus_40_percent_outliers(scenario):
    P, rays, Xw, out = scenario
    Pg, n, m, _ = _raw([(rays, Xw)], [0], 2000)
    _check_consensus(P, rays, Xw, out, Pg[0], m, n[0])
    (Pe, inl), = p3p_ransac_batch([(rays, Xw)], THR, max_iters=2000, keys=[0])
    assert np.array_equal(Pe, Pg[0]) and np.array_equal(inl, m)


@pytest.mark.parametrize("outliers,seed", [(0.7, 21), (0.9, 22)])
def test_consensus_many_outliers(outliers, seed):
    P, rays, Xw, out = _problem(np.random.default_rng(seed), 2000, outliers)
    Pg, n, m, _ = _raw([(rays, Xw)], [seed], 10000)
    _check_consensus(P, rays, Xw, out, Pg[0], m, n[0])


# ---------------------------------------------------------------------------
def test_batch_semantics_one_launch():
    rng = np.random.default_rng(5)
    sizes = [0, 2, 3, 4, 64, 257, 1000, 5000]           # 5000 > one LDS staging (1024 points)
    ratios = {3: 0.0, 4: 0.0, 64: 0.2, 257: 0.5, 5000: 0.6}
    truth, problems = {}, []
    for n in sizes:
        if n == 1000:
            problems.append(_noise(rng, n))             # pure noise: no consensus, runs every round
        else:
            P, rays, Xw, out = _problem(rng, n, ratios.get(n, 0.0))
            truth[n] = (P, out)
            problems.append((rays, Xw))
    keys = [100 + i for i in range(len(sizes))]
    max_iters = 1500
    P1, n1, m1, r1 = _raw(problems, keys, max_iters)
    P2, n2, m2, r2 = _raw(problems, keys, max_iters)
    for a, b in ((P1, P2), (n1, n2), (m1, m2), (r1, r2)):
        assert a.tobytes() == b.tobytes(), "two runs of one batch differ"
    off = np.concatenate([[0], np.cumsum(sizes)])
    for b, n in enumerate(sizes):
        Pa, na, ma, ra = _raw([problems[b]], [keys[b]], max_iters)
        assert Pa[0].tobytes() == P1[b].tobytes() and na[0] == n1[b] and ra[0] == r1[b], f"n={n}: alone != in the batch"
        assert np.array_equal(ma, m1[off[b]:off[b + 1]])
        mask = m1[off[b]:off[b + 1]]
        if n < 3:
            assert np.isnan(P1[b]).all() and n1[b] == 0 and r1[b] == 0
            continue
        assert np.isfinite(P1[b]).all() and n1[b] == mask.sum() >= 3
        err = angular_errors(P1[b], *problems[b])
        assert not (np.abs(err - THR) < BAND).any()
        assert np.array_equal(mask, err < THR)           # self-consistent, the noise problem included
        if n >= 64 and n != 1000:
            # consensus only: the threshold (3.5e-3 rad) is 35 x the ray noise, so every pose within
            # ~thr x depth (centimetres) of the truth holds the whole consensus set and the count
            # cannot tell them apart; the pose bounds are the subject of the consensus tests above
            Pt, out = truth[n]
            _check_consensus(Pt, problems[b][0], problems[b][1], out, P1[b], mask, n1[b], pose=False)
    # no consensus: exactly the bounded number of rounds; consensus: the adaptive stop ends earlier
    i_noise = sizes.index(1000)
    assert r1[i_noise] == -(-max_iters // WG)
    assert n1[i_noise] < 20
    assert r1[sizes.index(64)] < -(-max_iters // WG)
    # the python layer returns the same, with None for the problems without a pose
    res = p3p_ransac_batch(problems, THR, max_iters=max_iters, keys=keys)
    for b, (Pe, inl) in enumerate(res):
        assert inl.shape == (sizes[b],) and np.array_equal(inl, m1[off[b]:off[b + 1]])
        assert (Pe is None and sizes[b] < 3) or Pe.tobytes() == P1[b].tobytes()


def test_zero_iterations_and_hard_cap(scenario):
    _, rays, Xw, _ = scenario
    P, n, m, r = _raw([(rays, Xw)], [0], 0)
    assert np.isnan(P).all() and n[0] == 0 and not m.any() and r[0] == 0
    rays_n, X_n = _noise(np.random.default_rng(9), 300)
    for iters in (1, WG, WG + 1):
        P, n, m, r = _raw([(rays_n, X_n)], [1], iters)
        assert r[0] == -(-iters // WG)


def test_key_changes_the_stream_not_the_quality(scenario):
    P, rays, Xw, out = scenario
    res = p3p_ransac_batch([(rays, Xw), (rays, Xw)], THR, max_iters=2000, keys=[1, 2])
    for Pe, inl in res:
        _check_consensus(P, rays, Xw, out, Pe, inl)


def test_mutated_inlier_leaves_the_mask(scenario):
    P, rays, Xw, out = scenario
    (_, inl0), = p3p_ransac_batch([(rays, Xw)], THR, max_iters=2000, keys=[0])
    i = int(np.flatnonzero(inl0 & ~out)[-1])            # a true inlier, late in the point list
    X2 = Xw.copy()
    X2[0, i] += 1.0                                     # 1 m
    (Pe, inl), = p3p_ransac_batch([(rays, X2)], THR, max_iters=2000, keys=[0])
    assert inl0[i] and not inl[i]
    out2 = out.copy()
    out2[i] = True
    _check_consensus(P, rays, X2, out2, Pe, inl)


# ---------------------------------------------------------------------------
def test_cli_pnp_device_gpu(tmp_path):
    import inloc_localize as il
    scene = str(tmp_path / "scene")
    refs, qsize, focal = il.make_synthetic(scene, 3, 3, np.random.default_rng(0))   # what --synthetic 3 --seed 0 builds
    common = ["--matches_dir", os.path.join(scene, "matches"), "--shortlist", os.path.join(scene, "shortlist.mat"),
              "--cutout_dir", os.path.join(scene, "cutouts"), "--query_size", str(qsize[0]), str(qsize[1]),
              "--focal", str(focal), "--pnp_topN", "3", "--workers", "1"]
    old = os.getcwd()
    os.chdir(tmp_path)
    try:
        il.main(common + ["--pnp_device", "cpu", "--out", "cpu.npz"])
    finally:
        os.chdir(old)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "inloc_localize.py"), "--synthetic", "3", "--pnp_device", "gpu",
                        "--workers", "2", "--out", "gpu.npz"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "NCNET_CHECK" not in r.stdout + r.stderr
    c, g = np.load(tmp_path / "cpu.npz"), np.load(tmp_path / "gpu.npz")
    assert list(c["queries"]) == list(g["queries"]) and g["poses"].shape == c["poses"].shape == (3, 3, 3, 4)
    from scipy.io import loadmat
    cfg = {"cutout_dir": os.path.join(scene, "cutouts"), "trans_dir": "", "seed": 0, "thr": 0.75, "focal": focal,
           "n_subsample": None}
    panos = [f"DUC1/{q:03d}/DUC_cutout_{q:03d}_{30 * p}_0" for q in range(3) for p in range(3)]
    localized = 0
    for q in range(3):
        mats = loadmat(os.path.join(scene, "matches", f"{q + 1}.mat"))["matches"]
        for jj in range(3):
            Pc, Pg = c["poses"][q, jj], g["poses"][q, jj]
            rays, X, _ = il._pnp_tentatives(q, jj, panos[3 * q + jj], mats[0, jj], tuple(qsize), cfg)
            band = sum(int((np.abs(angular_errors(Pp, rays, X) - THR) < BAND).sum()) for Pp in (Pc, Pg))
            print(f"q{q} pano {jj}: inliers cpu {c['inliers'][q, jj]} gpu {g['inliers'][q, jj]} band {band}")
            assert abs(int(g["inliers"][q, jj]) - int(c["inliers"][q, jj])) <= band
            assert g["inliers"][q, jj] == (angular_errors(Pg, rays, X) < THR).sum()
            if jj > 0:                                   # pano 0 is built around a wrong pose on purpose
                dp, do = pose_distance(refs[q]["P"], Pc)
                if dp < 1e-2 and do < 1e-2:
                    localized += 1
                    dp, do = pose_distance(refs[q]["P"], Pg)
                    assert dp < 1e-2 and do < 1e-2
    assert localized == 6


# ---------------------------------------------------------------------------
def test_binding_rejects_malformed_arguments(scenario):
    from ncnet_amd.ops import _ext
    ext = _ext.ext()
    _, rays, Xw, _ = scenario
    n = rays.shape[1]
    r = torch.tensor(rays.T.copy(), dtype=torch.float64, device="cuda")
    x = torch.tensor(Xw.T.copy(), dtype=torch.float64, device="cuda")
    off = torch.tensor([0, 50, n], dtype=torch.int32, device="cuda")
    keys = torch.tensor([1, 2], dtype=torch.int64, device="cuda")

    def call(r=r, x=x, off=off, keys=keys, thr=float(THR), iters=100):
        return ext.p3p_ransac_batch(r, x, off, keys, thr, iters, 0.999, 20)

    P, cnt, mask = call()
    assert P.shape == (2, 3, 4) and P.dtype == torch.float64 and cnt.dtype == torch.int32
    assert mask.shape == (n,) and mask.dtype == torch.uint8
    bad = [dict(r=r.float()), dict(x=x.float()), dict(off=off.long()), dict(keys=keys.int()),     # dtypes
           dict(r=r.cpu()), dict(off=off.cpu()), dict(keys=keys.cpu()),                            # CPU tensors
           dict(r=r.t().contiguous().t()),                                                         # not contiguous
           dict(r=r[:-1].contiguous()), dict(keys=keys[:1].contiguous()),                          # shapes
           dict(off=torch.tensor([0, 120, 100], dtype=torch.int32, device="cuda")),                # not monotone
           dict(off=torch.tensor([0, 50, n - 1], dtype=torch.int32, device="cuda")),               # offsets[B] != N
           dict(off=torch.tensor([0, 50, n + 1], dtype=torch.int32, device="cuda")),
           dict(off=torch.tensor([1, 50, n], dtype=torch.int32, device="cuda")),
           dict(iters=-1), dict(thr=0.0), dict(thr=2.0)]
    for kw in bad:
        with pytest.raises(RuntimeError):
            call(**kw)
    with pytest.raises(RuntimeError):
        ext.p3p_solve(r[:198].view(66, 3, 3).float(), x[:198].view(66, 3, 3))
    with pytest.raises(RuntimeError):
        ext.p3p_solve(r[:198].view(66, 3, 3).cpu(), x[:198].view(66, 3, 3).cpu())
