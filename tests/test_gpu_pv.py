"""Batched dense pose verification on the GPU (csrc/pv.hip,
ncnet_amd/eval/pose_verification_gpu.py) against the torch path on the CPU
(ncnet_amd/eval/pose_verification.py), on the 60 x 80 scene of
tests/pv_scene.py: the z-buffer render exactly, the fused descriptor distance
and the scores within the measured spread of the torch path itself."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ncnet_amd.eval import pose_verification as pv
from ncnet_amd.eval import pose_verification_gpu as pvg
from tests import pv_scene as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# How far the torch path is from itself on these three poses, pv_score(device='cuda')
# against pv_score(device='cpu'), measured on the MI355X: profiles/pv/README.md.
# The batched path is allowed 4 times each (it changes the order of three
# reductions per descriptor and of the masked mean / standard deviation), with
# the rounding of one 128-term fp32 sum of values <= 1 as the floor.
REF_ERRMAP_ABS = 3.874302e-07   # largest |errmap(cuda) - errmap(cpu)| over the keypoints both evaluate
REF_SCORE_REL = 2.957775e-01    # largest |score(cuda) - score(cpu)| / score(cpu)
FLOOR = 128 * 2.0 ** -24
ERR_TOL = max(4 * REF_ERRMAP_ABS, FLOOR)
SCORE_TOL = max(4 * REF_SCORE_REL, FLOOR)
# REF_SCORE_REL is large because the torch path on the device loses keypoints
# (profiles/pv/README.md), which makes SCORE_TOL vacuous.  The score is
# 1 / median(err), and a median moves by no more than the largest change of its
# inputs, so errmaps within ERR_TOL bound the relative score difference by
# ERR_TOL / median = ERR_TOL * score; the tests hold the scores to twice that
# (the factor covers the second-order term and the rounding of the median).
SCORE_TOL_PER_SCORE = 2 * ERR_TOL

NAMES = ("true", "bad", "near")


@pytest.fixture(scope="module")
def ext():
    from ncnet_amd.ops import _ext
    return _ext.ext()


@pytest.fixture(scope="module")
def cloud():
    """The scene plus 5 points that must never win a pixel -> (rgb, xyz) arrays, N = 60005."""
    _, rgb, xyz = S.scene()
    extra = np.array([[np.nan, 0.0, 4.0], [np.inf, np.inf, np.inf], [0.0, 0.0, -4.0], [0.0, 0.0, 1e-10],
                      [1e30, -1e30, 4.0]])
    return (np.concatenate([rgb, np.full((5, 3), -7.0, np.float32)]), np.concatenate([xyz, extra]))


def _dev(rgb, xyz):
    return (torch.as_tensor(np.ascontiguousarray(xyz), dtype=torch.float64, device="cuda"),
            torch.as_tensor(np.ascontiguousarray(rgb), dtype=torch.float32, device="cuda"))


def _kp(poses):
    return torch.stack([S.kp_matrix(P) for P in poses]).contiguous().cuda()


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


# ---------------------------------------------------------------------------
def test_render_equals_torch(ext, cloud):
    rgb, xyz = cloud
    for name in NAMES:                                       # the guards: conditions, not measurements
        dist, gap = S.check_guards(xyz, S.POSES[name])
        assert dist > S.GUARD and gap > S.GUARD, (name, dist, gap)
    want = {n: S.render_cpu(rgb, xyz, S.POSES[n]) for n in NAMES}
    xyz_d, rgb_d = _dev(rgb, xyz)
    assert xyz_d.shape[0] == 60005
    pmax = ext.PV_PMAX
    for names in (NAMES[:1], NAMES, tuple(NAMES[i % 3] for i in range(pmax + 1))):
        synth, flag, winner = ext.pv_render(xyz_d, rgb_d, _kp([S.POSES[n] for n in names]), S.H, S.W)
        assert synth.shape == (len(names), S.H, S.W, 3) and synth.dtype == torch.float32
        assert flag.shape == (len(names), S.H, S.W) and flag.dtype == torch.bool
        synth, flag, winner = synth.cpu().numpy(), flag.cpu().numpy(), winner.cpu().numpy()
        assert int((winner >= S.N_POINTS).sum()) == 0 and not (synth == -7.0).any()     # none of the 5 extra points
        assert np.array_equal(winner >= 0, flag)
        for c, n in enumerate(names):
            assert np.array_equal(flag[c], want[n][1]), (len(names), c, n)
            assert np.array_equal(synth[c], want[n][0], equal_nan=True), (len(names), c, n)
    # N = 1 and N = 0
    one = np.array([[0.01, 0.01, 4.0]])
    synth, flag, winner = ext.pv_render(*_dev(np.full((1, 3), 9.0, np.float32), one), _kp([S.POSES["true"]]), S.H, S.W)
    ws, wf = S.render_cpu(np.full((1, 3), 9.0, np.float32), one, S.POSES["true"])
    assert int(flag.sum()) == 1 and np.array_equal(flag[0].cpu().numpy(), wf)
    assert np.array_equal(synth[0].cpu().numpy(), ws, equal_nan=True)
    synth, flag, winner = ext.pv_render(*_dev(np.zeros((0, 3), np.float32), np.zeros((0, 3))),
                                        _kp([S.POSES["true"], S.POSES["bad"]]), S.H, S.W)
    assert not bool(flag.any()) and bool(torch.isnan(synth).all()) and bool((winner == -1).all())


def test_render_tie_rule_and_reproducibility(ext, cloud):
    rgb, xyz = cloud
    xyz_d, rgb_d = _dev(rgb, xyz)
    kp3 = _kp([S.POSES[n] for n in NAMES])
    base = ext.pv_render(xyz_d, rgb_d, kp3, S.H, S.W)
    # duplicate 100 points that own a pixel at the true pose, with new colours, at the end
    owners = np.unique(base[2][0].cpu().numpy())
    owners = owners[owners >= 0][:: max(1, (owners.size - 1) // 100)][:100]
    assert owners.size == 100
    colours = np.repeat(-(1.0 + np.arange(100, dtype=np.float32))[:, None], 3, 1)
    xyz2_d, rgb2_d = _dev(np.concatenate([rgb, colours]), np.concatenate([xyz, xyz[owners]]))
    synth, flag, winner = ext.pv_render(xyz2_d, rgb2_d, kp3, S.H, S.W)
    w0, s0, b0 = winner[0].cpu().numpy(), synth[0].cpu().numpy(), base[2][0].cpu().numpy()
    for k, o in enumerate(owners):
        pix = b0 == o
        assert pix.sum() == 1 and (w0[pix] == xyz.shape[0] + k).all() and (s0[pix] == -(1.0 + k)).all()
    assert torch.equal(flag, base[1])                        # the duplicates cover nothing new
    # two runs: bitwise equal
    again = ext.pv_render(xyz2_d, rgb2_d, kp3, S.H, S.W)
    for a, b in zip((synth, flag, winner), again):
        assert torch.equal(_bits(a), _bits(b))
    # a pose alone = the same pose inside a batch
    alone = ext.pv_render(xyz2_d, rgb2_d, kp3[2:3].contiguous(), S.H, S.W)
    for a, b in zip((synth, flag, winner), alone):
        assert torch.equal(_bits(a[2]), _bits(b[0]))


def test_desc_err_equals_torch(ext):
    sides = [S.sides_cpu(S.POSES[n]) for n in NAMES]
    want = torch.stack([S.err_cpu(*s) for s in sides])       # [3, 104]
    iq = torch.stack([s[0] for s in sides]).cuda()
    isyn = torch.stack([s[1] for s in sides]).cuda()
    flag = torch.stack([s[2] for s in sides]).cuda()
    oq, osy = pvg.pooled_orientation_maps(iq), pvg.pooled_orientation_maps(isyn)
    err = ext.pv_desc_err(oq, osy, flag)
    assert err.shape == (3, 8 * 13) and err.dtype == torch.float32
    got = err.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert int((~torch.isnan(got)).sum()) >= 3 * 93
    diff = float((got - want).abs().nan_to_num(0.0).max())
    print(f"desc_err: max |err - torch| = {diff:.3e} (limit {ERR_TOL:.3e})")
    assert diff <= ERR_TOL
    # a constant image: no gradient, zero descriptors, err = 0
    const = pvg.pooled_orientation_maps(torch.full((1, S.H, S.W), 0.5, device="cuda"))
    e0 = ext.pv_desc_err(const, const.clone(), torch.ones(1, S.H, S.W, dtype=torch.bool, device="cuda"))
    assert float(e0.abs().max()) == 0.0
    # the same candidate alone and inside a batch
    alone = ext.pv_desc_err(oq[1:2].contiguous(), osy[1:2].contiguous(), flag[1:2].contiguous())
    assert torch.equal(_bits(alone[0]), _bits(err[1]))


@pytest.fixture(scope="module")
def end_to_end():
    q, rgb, xyz = S.scene()
    poses = [S.POSES[n] for n in NAMES] + [None, S.POSE_AWAY]
    return pvg.pv_scores_batch([q] * 5, rgb, xyz, poses, S.FOCAL, device="gpu", ds=S.DS, return_maps=True)


def test_end_to_end_equals_pv_score(end_to_end):
    from ncnet_amd.ops import _ext
    scores, maps = end_to_end
    assert _ext.DISPATCH["pv_render"] >= 1 and _ext.DISPATCH["pv_desc_err"] >= 1
    assert scores[3] == 0.0 and maps[3] == (None, None, None)
    q, rgb, xyz = S.scene()
    away = pv.pv_score(q, rgb, xyz, S.POSE_AWAY, S.FOCAL, device="cpu", ds=S.DS)
    assert scores[4] == 0.0 == away[0] and maps[4][2] is None and not maps[4][1].any()
    assert np.array_equal(maps[4][0], away[1], equal_nan=True)
    for i, n in enumerate(NAMES):
        s, synth, flag, errmap = S.reference(n)
        gs, (gsynth, gflag, gerr) = scores[i], maps[i]
        assert np.array_equal(gflag, flag) and np.array_equal(gsynth, synth, equal_nan=True)
        assert gerr.shape == errmap.shape and np.array_equal(np.isnan(gerr), np.isnan(errmap))
        d_err = float(np.nanmax(np.abs(gerr - errmap)))
        d_score = abs(gs - s) / s
        print(f"{n}: score {gs:.6f} torch {s:.6f} rel {d_score:.3e} (limit {SCORE_TOL:.3e}); "
              f"errmap max abs {d_err:.3e} (limit {ERR_TOL:.3e})")
        assert d_err <= ERR_TOL and d_score <= min(SCORE_TOL, SCORE_TOL_PER_SCORE * s)
    assert scores[0] > scores[2] > scores[1] > 0 and scores[0] > 2 * scores[1]


def test_mutated_pose_changes_its_score_only(end_to_end):
    scores, _ = end_to_end
    q, rgb, xyz = S.scene()
    poses = [S.POSES["true"], S.POSES["bad"], S.near_moved(1.0), None, S.POSE_AWAY]
    moved = pvg.pv_scores_batch([q] * 5, rgb, xyz, poses, S.FOCAL, device="gpu", ds=S.DS)
    assert moved[2] != scores[2] and moved[2] > 0
    assert [moved[i] for i in (0, 1, 3, 4)] == [scores[i] for i in (0, 1, 3, 4)]


def test_cli_pv_device_gpu(tmp_path):
    import inloc_localize as il
    old = os.getcwd()
    os.chdir(tmp_path)
    try:
        est_cpu, rate_cpu = il.main(["--synthetic", "2", "--pv", "--pv_device", "cpu", "--workers", "1",
                                     "--ransac_iters", "300", "--out", "cpu.npz"])
        want = open("error_NCNet_PV.txt").read()
        os.remove("error_NCNet_PV.txt")
    finally:
        os.chdir(old)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "inloc_localize.py"), "--synthetic", "2", "--pv",
                        "--pv_device", "gpu", "--workers", "2", "--ransac_iters", "300", "--out", "gpu.npz"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "NCNET_CHECK" not in r.stdout + r.stderr
    assert open(tmp_path / "error_NCNet_PV.txt").read() == want
    top1 = {ln.split(":")[0]: ln.split("PV top-1 ")[1].split()[0] for ln in r.stdout.splitlines() if "PV top-1" in ln}
    assert top1 == {k: v[0] for k, v in est_cpu.items()} and len(top1) == 2
    curve = r.stdout.split("InLoc + NCNet")[1]
    rates = [float(ln.split(":")[1].strip().rstrip("%")) for ln in curve.splitlines() if "deg:" in ln]
    assert len(rates) == len(rate_cpu) and all(v == 100.0 for v in rates[1:])      # rates[0]: the 0 m threshold
    assert (rate_cpu[1:] == 1.0).all()


def test_binding_rejects_malformed_arguments(ext, cloud):
    rgb, xyz = cloud
    xyz_d, rgb_d = _dev(rgb, xyz)
    kp = _kp([S.POSES["true"]])
    bad = [(xyz_d.float(), rgb_d, kp, S.H, S.W), (xyz_d, rgb_d.double(), kp, S.H, S.W),           # dtypes
           (xyz_d, rgb_d, kp.float(), S.H, S.W),
           (xyz_d.cpu(), rgb_d, kp, S.H, S.W), (xyz_d, rgb_d, kp.cpu(), S.H, S.W),                # CPU tensors
           (xyz_d.t().contiguous().t(), rgb_d, kp, S.H, S.W),                                     # not contiguous
           (xyz_d[:, :2].contiguous(), rgb_d, kp, S.H, S.W),                                      # an [N, 2] cloud
           (xyz_d, rgb_d[:-1].contiguous(), kp, S.H, S.W), (xyz_d, rgb_d, kp[0], S.H, S.W),       # shapes
           (xyz_d, rgb_d, kp, 0, S.W), (xyz_d, rgb_d, kp, S.H, 0), (xyz_d, rgb_d, kp, 1 << 16, 1 << 16)]
    for args in bad:
        with pytest.raises(RuntimeError):
            ext.pv_render(*args)
    o = torch.zeros(2, 8, S.H, S.W, device="cuda")
    f = torch.ones(2, S.H, S.W, dtype=torch.bool, device="cuda")
    assert ext.pv_desc_err(o, o, f).shape == (2, 104)
    assert ext.pv_desc_err(o[..., :30, :].contiguous(), o[..., :30, :].contiguous(), f[:, :30].contiguous()).shape == (2, 0)
    bad = [(o.double(), o, f), (o, o, f.to(torch.uint8)), (o.cpu(), o, f), (o, o, f.cpu()),
           (o.transpose(2, 3), o.transpose(2, 3), f.transpose(1, 2)),
           (o[:, :4].contiguous(), o[:, :4].contiguous(), f), (o, o[:1].contiguous(), f), (o, o, f[:1].contiguous())]
    for args in bad:
        with pytest.raises(RuntimeError):
            ext.pv_desc_err(*args)
