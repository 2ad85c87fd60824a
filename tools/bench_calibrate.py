#!/usr/bin/env python3
"""Timing of fixed-camera calibration (lib/core/calibrate.CameraCalibrator over hrp_pnp_solve_pooled, csrc/pnp_pooled.hip): device-event
time of ``solve()`` at 10, 150, 1000 and 2340 frames of 7 key-points (70 .. 16380 points), and next to it ``pnp_solve_robust`` over
the same frames as a batch of 7-point problems - the nearest thing there was, F poses instead of one, not an equivalent.  Sequences as
tests/golden/gen_golden_pnp_pooled.py draws them, with the points in a box: +-1 px noise, 30 % of the frames on a distractor, 10 % of the
remaining points displaced.  Run on the GPU box: ``python tools/bench_calibrate.py``.  Nothing is gated on these numbers; DESIGN 7.12
records them."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hrpe_amd  # noqa: E402,F401
from hrpe_amd.lib.core.calibrate import CameraCalibrator  # noqa: E402
from hrpe_amd.lib.utils import BPnP as M  # noqa: E402
from test_pnp_host import rodrigues_np  # noqa: E402

DEV = torch.device("cuda:0")
KP = 7


def timeit(fn, warmup=5, reps=30):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def sequence(F, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    K = np.array([[615.0, 0, 320], [0, 615.0, 240], [0, 0, 1]])
    X = rng.uniform([-0.45, -0.45, 0.0], [0.45, 0.45, 0.9], (F, KP, 3))
    P = np.array([0.4, -0.3, 0.2, 0.05, -0.1, 2.0])
    p = (X @ rodrigues_np(P[None, :3])[0].T + P[3:]) @ K.T
    x = p[..., :2] / p[..., 2:3] + rng.uniform(-1, 1, (F, KP, 2))
    mask = np.ones((F, KP), bool)
    for f in rng.choice(F, int(round(0.3 * F)), replace=False):
        ang, d = rng.uniform(0, 2 * np.pi), rng.uniform(40, 120)
        x[f] += d * np.array([np.cos(ang), np.sin(ang)])
        mask[f] = False
    free = np.flatnonzero(mask.ravel())
    for i in rng.choice(free, int(0.1 * len(free)), replace=False):
        ang, d = rng.uniform(0, 2 * np.pi), rng.uniform(15, 60)
        x.reshape(-1, 2)[i] += d * np.array([np.cos(ang), np.sin(ang)])
        mask.ravel()[i] = False
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=DEV)  # noqa: E731
    return t(x), t(X), t(K), P, mask


class Robot:
    nkp = KP


def main():
    print("us per call, device events, 5 warm-up + 30 timed calls")
    for F in (10, 150, 1000, 2340):
        x, X, K, P_true, mask = sequence(F, 300 + F)
        cal = CameraCalibrator(Robot(), K, capacity_frames=F, min_inliers=4, device=DEV)
        cal.add(x, None, points_3d=X)
        res = cal.solve()
        st = res.status.cpu().numpy()
        err = np.abs(res.cTr.cpu().numpy() - P_true).max()
        same = bool((res.inliers.cpu().numpy() == mask).all())
        sig = " ".join(f"{v:.1e}" for v in res.cov.diagonal().sqrt().cpu().numpy()[3:])
        t_solve = timeit(cal.solve)
        t_rob = timeit(lambda: M.pnp_solve_robust(x, X, K))
        print(f"F = {F:4d} ({F * KP:5d} points): solve {t_solve:9.1f}   pnp_solve_robust over {F} frames {t_rob:9.1f}  |  {int(st[3])} hypotheses, "
              f"{int(st[2])} inliers (planted mask recovered: {same}), {int(st[1])} LM trials, flags {int(st[0])}, "
              f"|pose - generating| {err:.1e}, sigma_t {sig} m")


if __name__ == "__main__":
    main()
