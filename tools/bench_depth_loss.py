#!/usr/bin/env python3
"""Timing of the DepthNet step's loss (csrc/depth_loss.hip) at B = 64 in its three modes: one ``depthnet_loss`` call with an
evaluator (one hrp_depth_loss launch: loss, per-image errors, the batch's loss row) beside the reference-style sequence it replaces -
the same arithmetic as tensor expressions on the device plus the three ``.cpu()`` copies of the per-image errors
(train_depthnet.py:236-241).  Neither side computes a gradient (the validation pass).  Device events around `reps` calls after
warm-up, five rounds alternating the two; the median round is printed with the spread.  A call's time is the larger of the host's
enqueue time and the device's; 100 calls replayed from one captured graph give the device's share per launch.  The reference-style side ends each call in a
device-to-host copy, so its time includes that wait - which is what the fused path removes.  Run on the GPU box:
``python tools/bench_depth_loss.py``."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hrpe_amd  # noqa: E402,F401
from hrpe_amd.lib.core import depthnet as dn  # noqa: E402

DEV = torch.device("cuda:0")
MODES = {"plain l1": dict(depth_loss_func="l1"), "xy l1 + mse": dict(depth_loss_func="l1", xy_loss_func="mse"),
         "multi_kp [1, 3, 5] l1": dict(depth_loss_func="l1", kps_need_depth=[1, 3, 5])}


def timeit(fn, warmup=20, reps=200):
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
    B, J = 64, 8
    g = torch.Generator().manual_seed(1)
    kp3d = torch.rand(B, J, 3, generator=g) + 0.5
    gt = {k: v.to(DEV) for k, v in dict(root_trans=kp3d[:, 3].contiguous(), kp3d=kp3d, mask=torch.ones(B)).items()}
    for name, o in MODES.items():
        if "xy_loss_func" in o:
            pred = torch.cat([kp3d[:, 3, 0:2], kp3d[:, 3, 2:3] * 1000.0], 1)
        elif "kps_need_depth" in o:
            pred = kp3d[:, [1, 3, 5], 2] * 1000.0
        else:
            pred = kp3d[:, 3, 2:3] * 1000.0
        pred = (pred + 0.03 * torch.randn(pred.shape, generator=g)).contiguous().to(DEV)
        ev = dn.DepthEvaluator(B, device=DEV, batch_capacity=1)

        def fused():
            ev.count = ev.batches = 0                      # the same rows every call
            return dn.depthnet_loss(pred, gt, evaluator=ev, **o)

        def reference_style():
            loss = dn.depthnet_loss_expr(pred, gt, **o)
            return loss, [e.cpu() for e in dn.depthnet_errors_expr(pred, gt, o.get("xy_loss_func"), o.get("kps_need_depth"))]

        want, _ = reference_style()
        assert abs(fused().item() - want.item()) <= 2e-5 * abs(want.item()), (name, fused().item(), want.item())
        rounds = [(timeit(fused), timeit(reference_style)) for _ in range(5)]
        f, r = [sorted(c) for c in zip(*rounds)]
        # the launch without the host's share: 100 calls captured in one graph, replayed
        graph, n = torch.cuda.CUDAGraph(), 100
        with torch.cuda.graph(graph):
            for _ in range(n):
                fused()
        k = sorted(timeit(graph.replay, warmup=3, reps=20) / n for _ in range(5))
        print(f"{name:24s} B={B}: depthnet_loss call {statistics.median(f):7.1f} us ({f[0]:.1f} .. {f[-1]:.1f}), in a replayed graph "
              f"{statistics.median(k):5.2f} us per launch ({k[0]:.2f} .. {k[-1]:.2f});   tensor expressions + 3 .cpu() "
              f"{statistics.median(r):7.1f} us ({r[0]:.1f} .. {r[-1]:.1f})")


if __name__ == "__main__":
    main()
