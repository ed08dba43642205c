"""The shared scene of the batched pose-verification tests (test_pv_batch_cpu.py,
test_gpu_pv.py): a random (not gridded) coloured cloud on a wavy surface, a
query rendered from it at the identity pose, three poses, the CPU torch
reference of every pose, and the two guards under which the z-buffer render
must be exactly reproducible whatever the fp64 summation order.

A regular grid must not be used: at the true pose its points fall exactly on
pixel boundaries, where the last bit of a projection decides the pixel."""
import functools
import math

import numpy as np
import torch

from ncnet_amd.eval import pose_verification as pv

N_POINTS = 60000
FOCAL = 300.0
DS = 0.25
H, W = 60, 80                       # the target size: 240 x 320 query at ds 0.25
GUARD = 1e-9


def _yaw(deg):
    a = math.radians(deg)
    return np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])


def _pitch(deg):
    a = math.radians(deg)
    return np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])


def pose(R, t):
    return np.hstack([np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)])


POSES = {
    "true": pose(np.eye(3), (0, 0, 0)),
    "bad": pose(_yaw(8.0), (0.4, 0.0, 0.0)),
    "near": pose(_pitch(2.0), (0.05, 0.02, 0.0)),
}
POSE_AWAY = pose(_yaw(180.0), (0, 0, 0))


def near_moved(deg=1.0):
    """``near`` pitched by a further ``deg`` degrees."""
    return pose(_pitch(2.0 + deg), (0.05, 0.02, 0.0))


@functools.lru_cache(maxsize=None)
def scene():
    """-> (query image [240, 320, 3] float32, rgb [N, 3] float32, xyz [N, 3] float64)."""
    rng = np.random.default_rng(0)
    K = np.array([[FOCAL, 0, 160.0], [0, FOCAL, 120.0], [0, 0, 1]])
    u, v = rng.uniform(0, 320, N_POINTS), rng.uniform(0, 240, N_POINTS)
    z = 4.0 + 0.5 * np.sin(u / 40.0) + 0.3 * np.cos(v / 25.0) + rng.uniform(0, 0.05, N_POINTS)
    X = np.ascontiguousarray((np.linalg.solve(K, np.stack([u, v, np.ones(N_POINTS)])) * z).T)
    tex = (np.sin(3 * X[:, 0]) + np.cos(4 * X[:, 1]) + 2) / 4 * 255
    rgb = np.ascontiguousarray(np.repeat(tex[:, None], 3, 1).astype(np.float32))
    img, _ = pv.points_to_perspective(torch.tensor(rgb), torch.tensor(X), torch.tensor(K @ POSES["true"]), 240, 320)
    q = pv.inpaint_nans(pv.rgb2gray(img)).numpy().astype(np.float32)
    return np.repeat(q[..., None], 3, 2), rgb, X


def kp_matrix(P, h=H, w=W, focal=FOCAL, ds=DS):
    """K @ P at the target size, built as pv_score builds it."""
    fl = focal * ds
    K = torch.tensor([[fl, 0, w / 2.0], [0, fl, h / 2.0], [0, 0, 1]], dtype=torch.float64)
    return K @ torch.as_tensor(np.asarray(P, np.float64))


def render_cpu(rgb, xyz, P):
    """points_to_perspective on the CPU -> (synth [H, W, 3] float32 array, flag [H, W] bool array)."""
    synth, sxyz = pv.points_to_perspective(torch.as_tensor(np.asarray(rgb, np.float32)),
                                           torch.as_tensor(np.asarray(xyz, np.float64)), kp_matrix(P), H, W)
    return synth.numpy(), (~torch.isnan(sxyz).any(-1)).numpy()


def check_guards(xyz, P):
    """The conditions under which the render is decided beyond rounding: every
    point in front of the camera is more than GUARD px from a pixel boundary,
    and the two nearest depths of every pixel differ by more than GUARD
    (relative).  Returns the two minima (boundary distance, relative depth gap)."""
    KP = kp_matrix(P).numpy()
    xyz = np.asarray(xyz, np.float64)
    xyz = xyz[np.isfinite(xyz).all(1)]
    p = np.concatenate([xyz, np.ones((xyz.shape[0], 1))], 1) @ KP.T
    front = p[:, 2] > 1e-9
    p = p[front]
    uv = p[:, :2] / p[:, 2:3]
    near_img = (uv[:, 0] > -1) & (uv[:, 0] < W + 1) & (uv[:, 1] > -1) & (uv[:, 1] < H + 1)
    dist = np.abs(uv[near_img] - np.round(uv[near_img])).min()
    fl = np.floor(uv)
    inside = (fl[:, 0] >= 0) & (fl[:, 0] < W) & (fl[:, 1] >= 0) & (fl[:, 1] < H)
    pix = (fl[inside, 1] * W + fl[inside, 0]).astype(np.int64)
    z = p[inside, 2]
    order = np.lexsort((z, pix))
    pix, z = pix[order], z[order]
    same = pix[1:] == pix[:-1]
    first = np.concatenate([[True], ~same])              # the nearest point of each pixel
    second = np.concatenate([[False], first[:-1]]) & ~first
    gap = ((z[second] - z[np.nonzero(second)[0] - 1]) / z[second]).min() if second.any() else np.inf
    return float(dist), float(gap)


@functools.lru_cache(maxsize=None)
def reference(name):
    """pv_score on the CPU for POSES[name] -> (score, synth, flag, errmap), computed once."""
    q, rgb, xyz = scene()
    return pv.pv_score(q, rgb, xyz, POSES[name], FOCAL, device="cpu", ds=DS)


def sides_cpu(P):
    """The two normalised images pv_score feeds to dense_sift for pose P, on the
    CPU -> (iq, isyn, flag) torch tensors [H, W]."""
    import torch.nn.functional as F
    q, rgb, xyz = scene()
    qt = torch.as_tensor(q)
    qs = F.interpolate(qt.permute(2, 0, 1)[None], size=(H, W), mode="bilinear", align_corners=False,
                       antialias=True)[0].permute(1, 2, 0)
    synth, sxyz = pv.points_to_perspective(torch.as_tensor(rgb), torch.as_tensor(xyz), kp_matrix(P), H, W)
    flag = ~torch.isnan(sxyz).any(-1)
    iq = pv.image_normalization(pv.rgb2gray(qs) / (255.0 if float(qs.max()) > 1.5 else 1.0), flag)
    gs = pv.rgb2gray(synth) / (255.0 if float(torch.nan_to_num(synth).max()) > 1.5 else 1.0)
    gs = torch.where(flag, gs, torch.full_like(gs, float("nan")))
    isyn = pv.image_normalization(pv.inpaint_nans(gs), flag)
    return iq, isyn, flag


def err_cpu(iq, isyn, flag):
    """dense_sift + root_sift + distance on the CPU -> err [n] float32 tensor, NaN off the mask."""
    fq, dq = pv.dense_sift(iq)
    fs, dsy = pv.dense_sift(isyn)
    iseval = flag[fs[1].long(), fs[0].long()]
    err = torch.sqrt(((pv.root_sift(dq) - pv.root_sift(dsy)) ** 2).sum(0))
    return torch.where(iseval, err, torch.full_like(err, float("nan")))
