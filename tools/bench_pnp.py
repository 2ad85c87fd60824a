#!/usr/bin/env python3
"""Timing of the back-propagatable PnP (csrc/pnp.hip): forward (EPnP + LM), backward, both, at B = 64 with panda's n = 7 FK
key-points, and one B = 64 prepare_batch(synthetic=False).  Device events around `reps` calls after warm-up.  Run on the GPU box:
``python tools/bench_pnp.py``.  ``--robust``: hrp_pnp_solve against hrp_pnp_solve_robust at B = 64 for n = 7, 17, 24 (seeded points in
a 0.6 m cube at 1-2 m, sigma = 0.5 px, a quarter of the points displaced by 30-100 px), with the robust call's phases told apart by
their own runs: the hypotheses alone (a threshold nothing meets, so the fallback's EPnP + LM is subtracted) and the refits."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hrpe_amd  # noqa: E402,F401
from hrpe_amd.lib.core.function import prepare_batch  # noqa: E402
from hrpe_amd.lib.utils import BPnP as M  # noqa: E402
from hrpe_amd.lib.utils.urdf_robot import URDFRobot  # noqa: E402
from test_gpu_pnp import _real_batch  # noqa: E402

DEV = torch.device("cuda:0")


def timeit(fn, warmup=10, reps=50):
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


def main():
    B = 64
    robot = URDFRobot("panda")
    batch = _real_batch(robot, B)
    x = torch.as_tensor(batch["keypoints_2d_original"]).to(DEV)
    rng = np.random.Generator(np.random.PCG64(1))
    x = x + torch.tensor(rng.normal(0, 1.0, x.shape), dtype=torch.float32, device=DEV)
    q = torch.stack([torch.tensor(v) for v in batch["jointpose"].values()], 1).float().to(DEV)
    X = robot.get_keypoints_only_fk(q).contiguous()
    K = torch.as_tensor(batch["K_original"])[0].to(DEV)
    P, status, rms = M.pnp_solve(x, X, K)
    go = torch.randn(B, 6, device=DEV)
    it = status[:, 1].float()
    print(f"B={B} n={x.shape[1]}: converged {int(status[:, 0].sum())}/{B}, LM iterations mean {it.mean():.1f} max {int(it.max())}, "
          f"rms {rms.mean():.3f} px")
    t_f = timeit(lambda: M.pnp_solve(x, X, K))
    t_b = timeit(lambda: M.pnp_backward(x, X, K, P, go))
    t_bf = timeit(lambda: M.pnp_backward(x, X, K, P, go, fast=True))
    xr, Xr, Kr = x.clone().requires_grad_(), X.clone().requires_grad_(), K.clone().requires_grad_()

    def both():
        M.BPnP_m3d.apply(xr, Xr, Kr).backward(go)

    t_fb = timeit(both)
    t_pb = timeit(lambda: prepare_batch(batch, robot, DEV, reference_keypoint_id=3, synthetic=False), warmup=3, reps=20)
    t_ps = timeit(lambda: prepare_batch(batch, robot, DEV, reference_keypoint_id=3, synthetic=True), warmup=3, reps=20)
    print(f"forward (EPnP + LM)        {t_f:8.1f} us")
    print(f"backward                   {t_b:8.1f} us")
    print(f"backward, fast             {t_bf:8.1f} us")
    print(f"BPnP_m3d forward+backward  {t_fb:8.1f} us")
    print(f"prepare_batch real / synth {t_pb:8.1f} / {t_ps:.1f} us")


def robust_cloud(n, B, seed):
    from test_pnp_host import rodrigues_np
    rng = np.random.Generator(np.random.PCG64(seed))
    X = rng.uniform(-0.3, 0.3, (B, n, 3))
    ax = rng.normal(size=(B, 3))
    R = rodrigues_np(ax / np.sqrt((ax ** 2).sum(1, keepdims=True)) * rng.uniform(0.1, 3.0, (B, 1)))
    d = rng.uniform(1.0, 2.0, B)
    t = np.stack([rng.uniform(-0.15, 0.15, B) * d, rng.uniform(-0.1, 0.1, B) * d, d], 1)
    K = np.array([[615.0, 0, 320], [0, 615.0, 240], [0, 0, 1]])
    p = np.einsum("bnj,ij->bni", np.einsum("bij,bnj->bni", R, X) + t[:, None], K)
    x = p[..., :2] / p[..., 2:3] + rng.normal(0, 0.5, (B, n, 2))
    k = max(1, n // 4)
    for i in range(B):
        out = rng.choice(n, size=k, replace=False)
        ang, r = rng.uniform(0, 2 * np.pi, k), rng.uniform(30, 100, k)
        x[i, out] += np.stack([r * np.cos(ang), r * np.sin(ang)], 1)
    f = lambda a: torch.tensor(a, dtype=torch.float32, device=DEV)  # noqa: E731
    return f(x), f(X), f(K), k


def robust_main():
    B = 64
    print(f"B = {B}; us per call, device events, 20 warm-up + 200 timed calls")
    for n in (7, 17, 24):
        x, X, K, k = robust_cloud(n, B, 40 + n)
        P, inl, status, rms = M.pnp_solve_robust(x, X, K)
        st = status.cpu().numpy()
        t_plain = timeit(lambda: M.pnp_solve(x, X, K), warmup=20, reps=200)
        t_rob = timeit(lambda: M.pnp_solve_robust(x, X, K), warmup=20, reps=200)
        t_all = timeit(lambda: M.pnp_solve_robust(x, X, K, refine_all=True), warmup=20, reps=200)
        # nothing lies within 1e-9 px of a pose from three other points: every hypothesis is solved and scored, then the fallback runs
        t_none = timeit(lambda: M.pnp_solve_robust(x, X, K, reproj_error=1e-9), warmup=20, reps=200)
        print(f"n = {n:2d} ({k} outliers): pnp_solve {t_plain:7.1f}  robust {t_rob:7.1f} (x{t_rob / t_plain:.2f})  refine_all {t_all:7.1f}  "
              f"hypotheses alone {t_none - t_plain:7.1f}  |  {int(st[0, 3])} hypotheses, inliers mean {st[:, 2].mean():.1f}, "
              f"LM trials mean {st[:, 1].mean():.1f}, no consensus {int((st[:, 0] & 1).sum())}/{B}")


if __name__ == "__main__":
    if "--robust" in sys.argv[1:]:
        robust_main()
    else:
        main()
