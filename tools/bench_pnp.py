#!/usr/bin/env python3
"""Timing of the back-propagatable PnP (csrc/pnp.hip): forward (EPnP + LM), backward, both, at B = 64 with panda's n = 7 FK
key-points, and one B = 64 prepare_batch(synthetic=False).  Device events around `reps` calls after warm-up.  Run on the GPU box:
``python tools/bench_pnp.py``."""
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


if __name__ == "__main__":
    main()
