#!/usr/bin/env python3
"""The metrics part of one validation batch, the old way and the new way, in the same run (panda, B = 64 and 128).

old: what a validate written on the tensor-expression path does per batch, following the reference's loop (function.py:137-179,
     351-376): compute_metrics_batch twice (FK branch - with its FK launch - and integral branch), a tensor-expression geodesic
     distance, then the reference's per-batch host copies: every returned metric, the eleven loss values and the rotation distance
     ``.cpu()``.
new: the FK launch + Evaluator.add (one hrp_eval_batch launch and one copy of the eleven loss values), no host synchronisation.

Device events around `reps` calls after warm-up; launches counted with torch.profiler over one call of each.
Run on the GPU box: ``python tools/bench_validate.py``."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hrpe_amd  # noqa: E402,F401
from hrpe_amd.lib.core.function import TERM_NAMES, Evaluator  # noqa: E402
from hrpe_amd.lib.dataset.const import JOINT_BOUNDS  # noqa: E402
from hrpe_amd.lib.utils.geometries import rot6d_to_rotmat  # noqa: E402
from hrpe_amd.lib.utils.metrics import compute_metrics_batch  # noqa: E402
from hrpe_amd.lib.utils.transforms import point_projection_from_3d_tensor  # noqa: E402
from hrpe_amd.lib.utils.urdf_robot import URDFRobot  # noqa: E402

DEV = torch.device("cuda:0")
ROOT_KP = 3


def timeit(fn, warmup=10, reps=50):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps, (time.perf_counter() - t0) * 1e6 / reps


def count_launches(fn):
    """Device kernels + memory copies of one call (torch.profiler); None when the profiler is not usable."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        kernels = copies = 0
        for e in prof.events():
            if str(getattr(e, "device_type", "")).endswith("CUDA"):
                if "memcpy" in e.name.lower():
                    copies += 1
                else:
                    kernels += 1
        return kernels, copies
    except Exception as exc:      # noqa: BLE001
        print(f"  (launch count unavailable: {type(exc).__name__}: {exc})")
        return None


def make(robot, B):
    g = torch.Generator().manual_seed(B)
    b = torch.tensor(JOINT_BOUNDS["panda"])
    q = (b[:, 0] + (b[:, 1] - b[:, 0]) * torch.rand(B, 8, generator=g)).to(DEV)
    rot = torch.randn(B, 6, generator=g).to(DEV)
    t = torch.cat([torch.rand(B, 2, generator=g) * 0.4 - 0.2, 1.0 + torch.rand(B, 1, generator=g)], 1).to(DEV)
    K = torch.tensor([[615.0, 0, 320], [0, 615.0, 240], [0, 0, 1]]).repeat(B, 1, 1).to(DEV)
    gt3d = robot.get_keypoints(q, rot, t)
    gt2d = point_projection_from_3d_tensor(K, gt3d)
    n = lambda *s: torch.randn(*s, generator=g).to(DEV)      # noqa: E731
    return dict(q=q, K=K, gt3d=gt3d, gt2d=gt2d, pq=q + 0.02 * n(B, 8), prot=rot + 0.02 * n(B, 6), pt=t + 0.01 * n(B, 3),
                pint=gt3d + 0.01 * n(B, 7, 3), gt_rot=rot, out=torch.rand(11, generator=g).to(DEV))


def main():
    robot = URDFRobot("panda")
    for B in (64, 128):
        c = make(robot, B)
        loss_dict = {n: c["out"][i] for i, n in enumerate(TERM_NAMES)}
        loss = c["out"][10]
        common = dict(robot=robot, gt_keypoints3d=c["gt3d"], gt_keypoints2d=c["gt2d"], K_original=c["K"], gt_joint=c["q"], pred_depth=None,
                      pred_xy=None, reference_keypoint_id=ROOT_KP)

        def old(host_copies=True):
            r = compute_metrics_batch(pred_joint=c["pq"], pred_rot=c["prot"], pred_trans=c["pt"], pred_xyz_integral=None, **common)
            ri = compute_metrics_batch(pred_joint=None, pred_rot=None, pred_trans=None, pred_xyz_integral=c["pint"], **common)
            m = torch.bmm(rot6d_to_rotmat(c["prot"]), rot6d_to_rotmat(c["gt_rot"]).transpose(1, 2))
            rd = torch.acos(torch.clamp((m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2] - 1) / 2, -1.0, 1.0)).mean()
            if host_copies:
                return [v.cpu() for v in r] + [v.cpu() for v in ri] + [rd.cpu(), loss.cpu()] + [v.cpu() for v in loss_dict.values()]
            return r, ri, rd

        ev = Evaluator(robot, B, reference_keypoint_id=ROOT_KP, device=DEV, batch_capacity=1)

        def new():
            ev.count = ev.batches = 0                       # the same slots every time: the accumulator does not grow
            fk = robot.get_keypoints_root(c["pq"], c["prot"], c["pt"], root=ROOT_KP)
            return ev.add(dict(kp3d_fk=fk, kp3d_int=c["pint"], joint=c["pq"], rot=c["prot"]),
                          dict(kp3d=c["gt3d"], kp2d_original=c["gt2d"], K_original=c["K"], joint=c["q"], rot=c["gt_rot"]), loss, loss_dict)

        t_old, w_old = timeit(old)
        t_old_dev, w_old_dev = timeit(lambda: old(False))
        t_new, w_new = timeit(new)
        print(f"B={B}: old {t_old:8.1f} us (host wall {w_old:.1f}); old without the host copies {t_old_dev:8.1f} us (wall {w_old_dev:.1f}); "
              f"new {t_new:8.1f} us (wall {w_new:.1f})", flush=True)
        n_old, n_new = count_launches(old), count_launches(new)
        if n_old and n_new:
            print(f"B={B}: launches old {n_old[0]} kernels + {n_old[1]} copies; new {n_new[0]} kernels + {n_new[1]} copies", flush=True)


if __name__ == "__main__":
    main()
