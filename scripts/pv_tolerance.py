#!/usr/bin/env python
"""Measure the tolerances of tests/test_gpu_pv.py on the GPU (the figures of
profiles/pv/README.md).

REF lines: the torch path against itself on the scene of tests/pv_scene.py,
``pv_score(device='cuda')`` against ``pv_score(device='cpu')``: the largest
absolute errmap difference over the keypoints both evaluate, and the largest
relative score difference.  The batched path is allowed 4 times each, with
128 * 2^-24 as the floor.  NEW lines: the batched path against
``pv_score(device='cpu')``, for information; no limit is derived from them.

    python scripts/pv_tolerance.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ncnet_amd.eval import pose_verification as pv  # noqa: E402
from ncnet_amd.eval import pose_verification_gpu as pvg  # noqa: E402
from tests import pv_scene as S  # noqa: E402

NAMES = ("true", "bad", "near")


def _compare(tag, name, got, ref):
    s, synth, flag, em = got
    cs, csynth, cflag, cem = ref
    render_same = np.array_equal(flag, cflag) and np.array_equal(synth, csynth, equal_nan=True)
    d_err = float(np.nanmax(np.abs(em - cem)))
    d_score = abs(s - cs) / cs
    print(f"{tag} {name}: score {s!r} cpu {cs!r} rel {d_score:.6e} errmap_abs {d_err:.6e} "
          f"render_same {render_same} keypoints {int((~np.isnan(em)).sum())} cpu {int((~np.isnan(cem)).sum())}",
          flush=True)
    return d_err, d_score


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    q, rgb, xyz = S.scene()
    print("torch", torch.__version__, flush=True)
    worst = np.zeros(2)
    for n in NAMES:
        got = pv.pv_score(q, rgb, xyz, S.POSES[n], S.FOCAL, device="cuda", ds=S.DS)
        worst = np.maximum(worst, _compare("REF", n, got, S.reference(n)))
    floor = 128 * 2.0 ** -24
    print(f"REF_ERRMAP_ABS {worst[0]:.6e} REF_SCORE_REL {worst[1]:.6e}")
    print(f"limits: errmap {max(4 * worst[0], floor):.6e} score {max(4 * worst[1], floor):.6e} (floor {floor:.6e})")
    scores, maps = pvg.pv_scores_batch([q] * 3, rgb, xyz, [S.POSES[n] for n in NAMES], S.FOCAL, device="gpu", ds=S.DS,
                                       return_maps=True)
    for n, s, m in zip(NAMES, scores, maps):
        _compare("NEW", n, (s,) + tuple(m), S.reference(n))
    # where the torch path loses keypoints on the device: negative pooled values -> NaN under RootSIFT's sqrt
    iq, _, _ = S.sides_cpu(S.POSES["true"])
    for dev in ("cpu", "cuda"):
        _, d = pv.dense_sift(iq.to(dev))
        print(f"dense_sift on {dev}: min {float(d.min()):.3e}, negative entries {int((d < 0).sum())}, "
              f"NaN after root_sift {int(torch.isnan(pv.root_sift(d)).sum())}")


if __name__ == "__main__":
    main()
