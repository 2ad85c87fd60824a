#!/usr/bin/env python3
"""Timing of the kinematic refit (lib/utils/kinfit.py, csrc/kin.hip) on the Panda at B = 1, 16, 64, 1024.

Per B, device events around 30 calls after 5 warm-up calls, per call:
  fixed_camera  ``kin_solve`` with the pose shared and fixed, the six observable joints free (npar 6), start 0.15 rad off
  holistic      pose and joints free with prior_q = 1, root = 3 (npar 12), start 0.15 rad / 0.05 rad / 0.03 m off
  pnp_solve     ``pnp_solve(ini_pose=...)`` on the same key-points with the joints known: the nearest thing that existed (npar 6)
with the smallest and largest LM trial count of the batch.  With ``--filter`` also, on the fixed-camera inputs:
  filter_start   ``KinematicFilter.step`` with keep = 0 in every call: the stream starts at the same q0 as kin_solve, with the prior
                 diag(p0_var) (0.15 rad)^2 on the joints - kin_solve's problem plus the filter's covariance algebra and xyz_next
  filter_update  a step from a saved one-frame-old state on key-points moved as by 0.3 rad/s (gate 40, nothing gated); the state is put
                 back before every call by two device copies, which are inside the timed region  The samples of a batch are seeded random configurations inside the joint
bounds seen from about 1.5 m with +-1 px noise, so the trial counts are those of a realistic mix.  Nothing is gated on speed.
Run on the GPU box: ``python tools/bench_kinfit.py [--filter]``; prints one JSON line per B.

``--smooth`` times the smoother instead (``KinematicFilter.smooth`` / ``kin_smooth``, csrc/kin_smooth.hip) and prints one JSON line
per (case, B): the Panda with a fixed camera (n = 6) and holistic (n = 12) filtered over 256 frames of a sinusoidal motion with a
ring of 256 slots, and a synthetic history with n = 20 on the Baxter's chain; B = 1, 16; per L = 8, 32, 256 and cov on / off the
microseconds per call and per frame (device events, 5 + 30 calls), next to the filter step's microseconds per frame without and with
the recording launch (events around the 256 steps of the same run; their difference is ``hrp_kin_history_push``).

``--views V[,V...]`` times the multi-view refit instead (``kin_solve_views``, csrc/kin_views.hip) and prints one JSON line per (V, B):
the same draws of the Panda seen with +-1 px noise from the first V cameras of tests/kinviews_oracle.py (1.5 - 2 m away, looking at
(0, 0, 0.4)), the six observable joints free, start 0.15 rad off; microseconds per call, the smallest and largest LM trial count of the
batch and the microseconds per trial of the slowest sample, next to ``kin_solve`` in fixed_camera mode on view 0 alone in the same run."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hrpe_amd  # noqa: E402,F401
import kinfit_oracle as ko  # noqa: E402
from hrpe_amd.lib.dataset.const import JOINT_BOUNDS  # noqa: E402
from hrpe_amd.lib.utils import kinfit  # noqa: E402
from hrpe_amd.lib.utils.BPnP import pnp_solve  # noqa: E402
from hrpe_amd.lib.utils.urdf_robot import URDFRobot  # noqa: E402

DEV = torch.device("cuda:0")
K = np.float32([[600, 0, 320], [0, 600, 240], [0, 0, 1]])
POSE = np.array([1.2, -1.0, 0.8, 0.05, -0.1, 1.5])


def timed_us(fn, warmup=5, reps=30):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps, out


def batch(robot, B, root):
    """B samples: (pts2d, q_true, q0, base-frame key-points), float32 on the host; 64 distinct draws, repeated."""
    rng = np.random.default_rng(B)
    tab = ko.tables(robot.chain)
    lim = np.array(JOINT_BOUNDS["panda"])
    obs = kinfit.observable_joints(robot)
    rows = []
    for _ in range(min(B, 64)):
        q = np.float32(lim[:, 0] + (0.2 + 0.6 * rng.random(8)) * (lim[:, 1] - lim[:, 0])).astype(np.float64)
        X = ko.keypoints(tab, q, ko.rodrigues(POSE[:3]), POSE[3:], root)
        x = ko.project(K, X) + rng.uniform(-1, 1, (7, 2))
        q0 = np.clip(q + 0.15 * rng.standard_normal(8) * obs, lim[:, 0], lim[:, 1])
        rows.append((x, q, q0, ko.keypoints(tab, q, np.eye(3), np.zeros(3), 0)))
    rows = [rows[i % len(rows)] for i in range(B)]
    return [torch.from_numpy(np.stack([r[i] for r in rows]).astype(np.float32)).to(DEV) for i in range(4)]


def filter_rows(robot, B, x, q, q0, Kd):
    """The two filter timings on kin_solve's fixed-camera inputs."""
    tab = ko.tables(robot.chain)
    obs = kinfit.observable_joints(robot)
    flt = kinfit.KinematicFilter(robot, "fixed_camera", 1 / 30, 10.0, np.r_[np.full(6, 0.15 ** 2), np.full(6, 1.0)], streams=B, cTr=POSE,
                                 gate_chi2=40.0)
    zero = torch.zeros(B, dtype=torch.int32, device=DEV)
    us, res = timed_us(lambda: flt.step(x, Kd, q0, keep=zero))
    st = res.status.cpu().numpy()
    row = dict(filter_start_us=round(us, 1), filter_start_trials=[int(st[:, 1].min()), int(st[:, 1].max())],
               filter_start_converged=int((st[:, 0] & 32).sum() // 32))
    mean, cov = flt.mean.clone(), flt.cov.clone()
    qn = q.cpu().numpy().astype(np.float64)
    rng = np.random.default_rng(B + 1)
    xn = np.stack([ko.project(K, ko.keypoints(tab, qn[b] + 0.01 * obs, ko.rodrigues(POSE[:3]), POSE[3:], 0)) + rng.uniform(-1, 1, (7, 2))
                   for b in range(min(B, 64))])
    xn = torch.from_numpy(np.float32(xn[[b % len(xn) for b in range(B)]])).to(DEV)

    def update():
        flt.mean.copy_(mean)
        flt.cov.copy_(cov)
        return flt.step(xn, Kd, q0)
    us, res = timed_us(update)
    st = res.status.cpu().numpy()
    row.update(filter_update_us=round(us, 1), filter_update_trials=[int(st[:, 1].min()), int(st[:, 1].max())],
               filter_update_gated=int(st[:, 3].sum()), filter_update_converged=int((st[:, 0] & 32).sum() // 32))
    return row


def motion(robot, T, holistic, seed):
    """T frames of a sinusoidal motion seen by the fixed camera POSE: (pts2d [T, 7, 2], q_in [T, 8], rot [T, 3], trans [T, 3]) float32."""
    rng = np.random.default_rng(seed)
    tab = ko.tables(robot.chain)
    lim = np.array(JOINT_BOUNDS["panda"])
    obs = kinfit.observable_joints(robot)
    centre, freq, phase = lim.mean(1), rng.uniform(0.3, 0.6, 8), rng.uniform(0, 2 * np.pi, 8)
    Rc, tc = ko.rodrigues(POSE[:3]), POSE[3:]
    rows = []
    for t in range(T):
        q = centre + 0.25 * np.sin(2 * np.pi * freq * t / 30 + phase) * obs
        x = ko.project(K, ko.keypoints(tab, q, Rc, tc, 0)) + rng.standard_normal((7, 2))
        Troot = ko.frames(tab, q)[tab["kp_frame"][3]] if holistic else np.eye(4)
        pose = np.r_[ko.rotvec(Rc @ Troot[:3, :3]), Rc @ Troot[:3, 3] + tc]
        rows.append((x, q + 0.05 * rng.standard_normal(8) * obs, pose[:3], pose[3:]))
    return [torch.from_numpy(np.float32(np.stack([r[i] for r in rows]))).to(DEV) for i in range(4)]


def smooth_rows():
    import kinsmooth_oracle as ks
    T = 256
    Kd = torch.from_numpy(K).to(DEV)
    panda = URDFRobot("panda")
    for case in ("panda_fixed_camera", "panda_holistic", "synthetic_n20"):
        for B in (1, 16):
            row = dict(case=case, B=B)
            if case == "synthetic_n20":
                robot, free = URDFRobot("baxter"), np.arange(15) < 14
                hist, q_acc = ks.synthetic(20, T, 0)
                up = lambda a: torch.from_numpy(np.ascontiguousarray(a)[:, None].repeat(B, 1)).to(DEV)      # noqa: E731
                h = kinfit.KinHistory(up(hist["mean"]), up(hist["cov"]), up(hist["valid"]), up(hist["flags"]), torch.from_numpy(hist["dt"]).to(DEV),
                                      torch.zeros(T, B, 15, device=DEV))
                row["n"] = 20
                call = lambda L, c: kinfit.kin_smooth(robot, h, q_acc, free, free_pose=True, limits=False, first=T - L, length=L, cov=c)      # noqa: E731
            else:
                hol = case == "panda_holistic"
                x, q, rot, trans = motion(panda, T, hol, B)
                rep = lambda v: v[:, None].repeat(1, B, *([1] * (v.dim() - 1))).contiguous()      # noqa: E731
                x, q, rot, trans = rep(x), rep(q), rep(rot), rep(trans)
                per_frame = {}
                for slots in (0, T):
                    if hol:
                        flt = kinfit.KinematicFilter(panda, "holistic", 1 / 30, np.r_[np.full(6, 10.0), np.full(3, 10.0), np.full(3, 2.0)],
                                                     np.r_[np.full(6, 0.01), np.full(3, 0.01), np.full(3, 0.0025), np.full(6, 1.0), np.full(3, 1.0),
                                                           np.full(3, 0.25)], streams=B, gate_chi2=40.0, w_q=50.0)
                        one = lambda t: flt.step(x[t], Kd, q[t], rot[t], trans[t])      # noqa: E731
                    else:
                        flt = kinfit.KinematicFilter(panda, "fixed_camera", 1 / 30, 10.0, np.r_[np.full(6, 0.01), np.full(6, 1.0)], streams=B, cTr=POSE,
                                                     gate_chi2=40.0)
                        one = lambda t: flt.step(x[t], Kd, q[t])      # noqa: E731
                    flt.history = slots
                    for t in range(5):
                        one(t)
                    flt.reset()
                    flt.clear_history()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    a.record()
                    for t in range(T):
                        res = one(t)
                    b.record()
                    torch.cuda.synchronize()
                    per_frame[slots] = a.elapsed_time(b) * 1e3 / T
                st = res.status.cpu().numpy()
                row.update(n=flt.n, filter_step_us_per_frame=round(per_frame[0], 1), recording_step_us_per_frame=round(per_frame[T], 1),
                           push_us_per_frame=round(per_frame[T] - per_frame[0], 1), last_frame_flags=sorted(set(st[:, 0].tolist())))
                call = lambda L, c: flt.smooth(lag=L, cov=c)      # noqa: E731
            for L in (8, 32, T):
                for c in (True, False):
                    us, res = timed_us(lambda: call(L, c))
                    st = res.status.cpu().numpy()
                    row[f"L{L}_{'cov' if c else 'mean'}_us"] = round(us, 1)
                    row[f"L{L}_{'cov' if c else 'mean'}_us_per_frame"] = round(us / L, 2)
                    row[f"L{L}_smoothed"] = int((st[:, 0, 0] & 1).sum())
            print(json.dumps(row), flush=True)


def views_rows(views):
    import kinviews_oracle as kv
    robot = URDFRobot("panda")
    tab = ko.tables(robot.chain)
    poses = np.stack([kv.look_at(c) for c in kv.CAMERAS])
    Kd = torch.from_numpy(K).to(DEV)
    for V in views:
        for B in (1, 16, 64, 1024):
            _, q, q0, _ = batch(robot, B, 0)
            rng = np.random.default_rng(1000 + B)
            x = np.stack([[ko.project(K, ko.keypoints(tab, qb, ko.rodrigues(c[:3]), c[3:], 0)) + rng.uniform(-1, 1, (7, 2)) for c in poses[:V]]
                          for qb in q.cpu().numpy().astype(np.float64)[:64]])
            x = torch.from_numpy(np.float32(x[[b % len(x) for b in range(B)]])).to(DEV)
            multi = kinfit.MultiViewRefit(robot, poses[:V])
            us, res = timed_us(lambda: multi.solve(x, Kd.expand(V, 3, 3), q0))
            st = res.status.cpu().numpy()
            row = dict(V=V, B=B, views_us=round(us, 1), views_trials=[int(st[:, 1].min()), int(st[:, 1].max())],
                       views_converged=int((st[:, 0] & 1).sum()), views_us_per_trial=round(us / max(int(st[:, 1].max()), 1), 2))
            single = kinfit.KinematicRefit(robot, "fixed_camera", cTr=poses[0])
            x0 = x[:, 0].contiguous()
            us, res = timed_us(lambda: single.solve(x0, Kd, q0))
            st = res.status.cpu().numpy()
            row.update(fixed_camera_view0_us=round(us, 1), fixed_camera_view0_trials=[int(st[:, 1].min()), int(st[:, 1].max())],
                       fixed_camera_view0_us_per_trial=round(us / max(int(st[:, 1].max()), 1), 2))
            print(json.dumps(row), flush=True)


def main():
    if "--smooth" in sys.argv[1:]:
        return smooth_rows()
    if "--views" in sys.argv[1:]:
        i = sys.argv.index("--views")
        views = [int(v) for v in sys.argv[i + 1].split(",")] if i + 1 < len(sys.argv) else [1, 2, 4]
        return views_rows(views)
    with_filter = "--filter" in sys.argv[1:]
    robot = URDFRobot("panda")
    Kd = torch.from_numpy(K).to(DEV)
    rng = np.random.default_rng(0)
    for B in (1, 16, 64, 1024):
        row = dict(B=B)
        x, q, q0, Xb = batch(robot, B, 0)
        fixed = kinfit.KinematicRefit(robot, "fixed_camera", cTr=POSE)
        us, res = timed_us(lambda: fixed.solve(x, Kd, q0))
        st = res.status.cpu().numpy()
        row.update(fixed_camera_us=round(us, 1), fixed_camera_trials=[int(st[:, 1].min()), int(st[:, 1].max())],
                   fixed_camera_converged=int((st[:, 0] & 1).sum()))
        x3, _, q03, _ = batch(robot, B, 3)
        start = np.float32(POSE + np.r_[0.05 * rng.standard_normal(3), 0.03 * rng.standard_normal(3)])
        rot = torch.from_numpy(np.float32(ko.rodrigues(start[:3].astype(np.float64))[:2].ravel())).to(DEV).repeat(B, 1)
        trans = torch.from_numpy(start[3:]).to(DEV).repeat(B, 1)
        hol = kinfit.KinematicRefit(robot, "holistic", prior_q=1.0)
        us, res = timed_us(lambda: hol.solve(x3, Kd, q03, rot, trans))
        st = res.status.cpu().numpy()
        row.update(holistic_us=round(us, 1), holistic_trials=[int(st[:, 1].min()), int(st[:, 1].max())],
                   holistic_converged=int((st[:, 0] & 1).sum()))
        ini = torch.from_numpy(start).to(DEV).repeat(B, 1)
        us, (P6, pst, rms) = timed_us(lambda: pnp_solve(x, Xb, Kd, ini_pose=ini))
        pst = pst.cpu().numpy()
        row.update(pnp_solve_us=round(us, 1), pnp_solve_trials=[int(pst[:, 1].min()), int(pst[:, 1].max())])
        if with_filter:
            row.update(filter_rows(robot, B, x, q, q0, Kd))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
