#!/usr/bin/env python3
"""Timing of the streaming tracker (lib/core/tracker.py, csrc/track.hip) on 640 x 480 frames and 256 x 256 views at B = 1, 4, 16.

(a) ``prepare`` + ``update`` alone (a fixed prediction in between): device events over `reps` graph replays, and over as many
    eager calls, the median of three windows each, after a warm-up.
(b) ``PoseTracker.step`` with the HRNet-W32 pair in bf16: wall latency per frame (a synchronise after every step, what a camera loop
    that consumes the pose sees) and frames per second with the synchronise only at the end of the window.
(c) the same loop written with the public pieces that existed before the tracker: read ``xyz_fk`` back, the loader's geometry in
    numpy per stream (get_bbox, _resize_geometry, _view), descriptor_table, upload, pixel_launches, compute_k_values, the model.
(d) acquisition at B = 1, 4: ``PoseTracker.acquire`` (CtRNet's ``seg_mask_inference.detect`` in bf16 on the full frame + the seed
    launch), the key-point read-out launch pair alone on the detector's 30 x 40 x 2048 feature, and ``step`` with
    ``acquire_every=30``.  Nothing is gated on speed.
(e) ``--verify``: verification at B = 1, 4 next to the figures of (d): ``acquire`` (not forced; every stream has an estimate, so the
    seed launch skips them all) without verification, with the skeleton criteria, and with a box mesh of 432 faces as renderer
    (mesh pose + rasteriser + the IoU); the ``hrp_track_verify`` launch alone by device events on the detector's 240 x 320 map and
    on a 480 x 640 one, without and with a silhouette.  The thresholds are 0, so every measurement is taken and no stream is
    dropped from one repetition to the next.
Also: whether the model's forward synchronises (torch's sync debug mode around one call).  Prints one JSON line per B and row.
(f) ``--refit``: ``step`` at B = 1, 4, 16 without and with a holistic kinematic refit, and the refit's LM trial counts.
Run on the GPU box: ``python tools/bench_track.py`` (``--acquire``: the rows of (d) only; ``--verify``: the rows of (d) and (e) only;
``--refit``: the rows of (f) only)."""
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hrpe_amd  # noqa: E402,F401
from hrpe_amd.lib.core.common import compute_k_values  # noqa: E402
from hrpe_amd.lib.core.tracker import PoseTracker  # noqa: E402
from hrpe_amd.lib.dataset import dream as D  # noqa: E402
from hrpe_amd.lib.dataset.const import INITIAL_JOINT_ANGLE  # noqa: E402
from hrpe_amd.lib.models.full_net import RootNetwithRegInt  # noqa: E402
from hrpe_amd.lib.utils.urdf_robot import URDFRobot  # noqa: E402
import dream_scene  # noqa: E402
import track_oracle as O  # noqa: E402

DEV = torch.device("cuda:0")
H, W, HW = 480, 640, (256, 256)
K = np.array([[615.0, 0, 320], [0, 615, 240], [0, 0, 1]])


def model_bf16():
    class A(dict):
        __getattr__ = dict.__getitem__
    args = A(backbone_name="hrnet32", rootnet_backbone_name="hrnet32", other_image_size=256.0, use_rpmg=False, n_iter=4,
             p_dropout=0.0, reg_joint_map=False, joint_conv_dim=[], rotation_dim=6, direct_reg_rot=False,
             rot_iterative_matmul=False, fix_root=True, bbox_3d_shape=[1300, 1300, 1300], reference_keypoint_id=3, add_fc=False,
             multi_kp=False, kps_need_depth=None, pretrained_rootnet=None)
    init = {"robot_type": "panda", "pose_params": INITIAL_JOINT_ANGLE, "cam_params": np.eye(4), "init_pose_from_mean": True}
    torch.manual_seed(0)
    return RootNetwithRegInt(init, args).to(DEV).set_compute_dtype(torch.bfloat16).eval()


def seeds(B):
    rng = np.random.default_rng(0)
    return np.stack([np.array([320.0, 240.0]) + rng.uniform(-1, 1, (7, 2)) * np.array([120.0, 140.0]) for _ in range(B)])


def xyz_for(kp2d):
    z = 1.25 + 0.05 * np.arange(7)
    return torch.from_numpy(np.stack([(kp2d[..., 0] - 320) / 615 * z, (kp2d[..., 1] - 240) / 615 * z, np.broadcast_to(z, kp2d.shape[:-1])],
                                     -1).astype(np.float32)).to(DEV)


def window_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def median_us(fn, warmup=50, reps=300, windows=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return statistics.median(window_us(fn, reps) for _ in range(windows))


def bench_launches(B, frames):
    """(a): prepare + update alone, eager and as graph replays."""
    trk = PoseTracker(None, URDFRobot("panda"), K, (H, W), streams=B, device=DEV)
    kp = seeds(B)
    xyz = xyz_for(kp)
    trk.reset(kp)

    def body():
        trk.prepare(frames)
        trk.update(xyz)
    eager = median_us(body)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    return eager, median_us(g.replay)


def wall(step, frames_seq, warmup=10, n=60):
    """Per-frame wall latency (synchronise after every step) and throughput (synchronise at the end), in ms."""
    for i in range(warmup):
        step(frames_seq[i % len(frames_seq)])
    torch.cuda.synchronize()
    lat = []
    for i in range(n):
        t0 = time.perf_counter()
        step(frames_seq[i % len(frames_seq)])
        torch.cuda.synchronize()
        lat.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    for i in range(n):
        step(frames_seq[i % len(frames_seq)])
    torch.cuda.synchronize()
    return statistics.median(lat) * 1e3, (time.perf_counter() - t0) / n * 1e3


class HostLoop:
    """(c): the loop with the public pieces that existed before the tracker."""

    def __init__(self, model, B):
        self.model, self.B, self.kp, self.have = model, B, seeds(B), np.ones(B, bool)
        self.out = torch.empty(B, 3, *HW, dtype=torch.uint8, device=DEV)
        self.lsum = torch.empty(B, D.nv.DREAM_BANDS, dtype=torch.int64, device=DEV)
        self.scratch = torch.empty(B * H * W * 3, dtype=torch.uint8, device=DEV)
        self.noise = torch.empty(0, dtype=torch.uint8, device=DEV)

    def step(self, frames):
        recs = [O.tracker_record(self.kp[b], bool(self.have[b]), K, W, H, HW, HW) for b in range(self.B)]
        tab, _, _ = D.descriptor_table(O.aug_rows(recs, W, H), [b""] * self.B)
        table = torch.from_numpy(tab.view(np.uint8).copy()).to(DEV, non_blocking=True)
        D.pixel_launches(frames, table, self.noise, self.scratch, self.lsum, self.out)
        K_root = torch.stack([r["root"]["K"] for r in recs]).to(DEV, non_blocking=True)
        boxes = torch.stack([r["root"]["bbox_gt2d_extended"] for r in recs]).to(DEV, non_blocking=True)
        k = compute_k_values(K_root[:, 0, 0], K_root[:, 1, 1], boxes)
        with torch.no_grad():
            pred = self.model(self.out, self.out, k, K_root)
        x = pred[-1].float().cpu().numpy().astype(np.float64)                  # the read-back: a synchronisation every frame
        with np.errstate(all="ignore"):
            kp = np.stack([615.0 * x[..., 0] / x[..., 2] + 320.0, 615.0 * x[..., 1] / x[..., 2] + 240.0], -1)
        inside = (kp[..., 0] >= 0) & (kp[..., 0] < W) & (kp[..., 1] >= 0) & (kp[..., 1] < H)
        self.kp, self.have = kp, np.isfinite(kp).all((1, 2)) & (x[..., 2] > 0).all(1) & (inside.sum(1) >= 1)    # as hrp_track_update
        return pred


def forward_syncs(model, p):
    """The warnings torch's sync debug mode raises during one forward (an empty list: the forward does not synchronise)."""
    mode = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with torch.no_grad():
                model(p["reg_images"], p["root_images"], p["k_values"], p["other_K"])
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    return sorted({str(w.message).split("(")[0].strip() for w in seen if "ynchron" in str(w.message) and "prototype" not in str(w.message)})


def readout_alone_us(B, dtype=torch.bfloat16):
    """hrp_kp_readout_fwd (both launches) on a [B, 30, 40, 2048] feature, device events over eager calls."""
    from hrpe_amd import _native as nv
    cin, k, hin, win = 2048, 7, 30, 40
    x = torch.randn(B, hin, win, cin, device=DEV).to(dtype)
    w = torch.randn(cin, k, 4, 4, device=DEV) * 2.0 ** -5
    bias = torch.zeros(k, device=DEV)
    dt = nv.HRP_BF16 if dtype == torch.bfloat16 else nv.HRP_F32
    packed = torch.zeros(16 * cin * 32, dtype=dtype, device=DEV)
    nv.call("hrp_kp_readout_pack", w.data_ptr(), cin, k, packed.data_ptr(), dt, None)
    wsb = int(nv.lib().hrp_kp_readout_ws(B, hin))
    ws, kp, ms = torch.zeros(wsb // 4, device=DEV), torch.zeros(B, k, 2, device=DEV), torch.zeros(B, k, 2, device=DEV)
    return median_us(lambda: nv.call("hrp_kp_readout_fwd", x.data_ptr(), dt, B, hin, win, cin, cin, packed.data_ptr(), bias.data_ptr(), k,
                                     -1.0, -1.0, 160.0, 120.0, kp.data_ptr(), ms.data_ptr(), ws.data_ptr(), wsb, None), warmup=10, reps=50)


def bench_acquire(model, robot, B, seq):
    """(d): detector + seed, and step with a detection every 30 frames."""
    from hrpe_amd.lib.models.ctrnet.mask_inference import seg_mask_inference
    torch.manual_seed(1)
    det = seg_mask_inference((615.0, 615.0, 320.0, 240.0), "azure", image_hw=(H, W), allow_random_init=True).to(DEV)
    det.set_compute_dtype(torch.bfloat16)
    trk = PoseTracker(model, robot, K, (H, W), streams=B, device=DEV, detector=det.detect, detector_scale=det.args.scale,
                      acquire_every=30)
    trk.reset(seeds(B))
    alat, athr = wall(lambda f: trk.acquire(f, force=True), seq, warmup=6, n=30)
    lat, thr = wall(trk.step, seq, warmup=10, n=60)
    return dict(B=B, row="acquire", acquire_latency_ms=round(alat, 3), acquire_pipelined_ms=round(athr, 3),
                kp_readout_bf16_us=round(readout_alone_us(B), 1), kp_readout_fp32_us=round(readout_alone_us(B, torch.float32), 1),
                step_acquire_every_30_latency_ms=round(lat, 3), step_acquire_every_30_pipelined_ms=round(thr, 3),
                seed_status=trk.seed_status.cpu().tolist())


def bench_verify(model, robot, B, seq):
    """(e): acquire with verification, and the verify launch alone."""
    from hrpe_amd.lib.models.ctrnet.mask_inference import seg_mask_inference
    from bench_sim2real import grid_box_mesh
    torch.manual_seed(1)
    det = seg_mask_inference((615.0, 615.0, 320.0, 240.0), "azure", image_hw=(H, W), allow_random_init=True).to(DEV)
    det.set_compute_dtype(torch.bfloat16)
    scale = det.args.scale
    mesh = tuple(t.to(DEV) for t in grid_box_mesh(2))
    renderer = robot.set_robot_renderer(torch.tensor(K), (H, W), scale=scale, device=DEV, mesh=mesh)
    common = dict(streams=B, device=DEV, detector=det.detect, detector_scale=scale)
    rows = dict(B=B, row="verify", mesh_faces=int(mesh[2].shape[0]))
    trackers = {}
    for name, kw in (("plain", {}), ("skeleton", dict(min_support=0.0, min_coverage=0.0)),
                     ("silhouette", dict(min_support=0.0, min_coverage=0.0, min_iou=0.0, renderer=renderer))):
        trk = trackers[name] = PoseTracker(model, robot, K, (H, W), **common, **kw)
        trk.reset(seeds(B))
        if name == "silhouette":         # a pose in front of the camera stands in for the last prediction
            trk._last = (torch.zeros(B, robot.dof, device=DEV), torch.tensor([1.0, 0, 0, 0, 1, 0], device=DEV).repeat(B, 1),
                         torch.tensor([0.0, 0.0, 1.5], device=DEV).repeat(B, 1))
        lat, thr = wall(trk.acquire, seq, warmup=6, n=30)
        rows[f"acquire_{name}_latency_ms"], rows[f"acquire_{name}_pipelined_ms"] = round(lat, 3), round(thr, 3)
        rows[f"{name}_status"] = trk.verify_status.cpu().tolist()
    trk = trackers["silhouette"]
    for hm, wm in ((H // 2, W // 2), (H, W)):
        yy, xx = torch.meshgrid(torch.arange(hm, device=DEV), torch.arange(wm, device=DEV), indexing="ij")
        blob = ((((xx - wm / 2) / (wm / 4)) ** 2 + ((yy - hm / 2) / (hm / 4)) ** 2) <= 1).float()
        mask = (blob * 0.9).repeat(B, 1, 1).contiguous()
        alpha = torch.roll(mask, (hm // 8, wm // 8), (1, 2)).contiguous()
        trk._verify["scale"] = (wm / W, hm / H)
        rows[f"verify_{hm}x{wm}_us"] = round(median_us(lambda: trk.verify(mask), warmup=20, reps=200), 1)
        rows[f"verify_{hm}x{wm}_silhouette_us"] = round(median_us(lambda: trk.verify(mask, alpha), warmup=20, reps=200), 1)
        rows[f"verify_{hm}x{wm}_counts"] = trk.verify_counts.cpu().tolist()
    return rows


def bench_refit(model, robot):
    """(f): ``step`` without and with a holistic kinematic refit (kinfit.KinematicRefit, prior_q = 1; two more launches per frame)."""
    from hrpe_amd.lib.utils.kinfit import KinematicRefit
    for B in (1, 4, 16):
        seq = [torch.from_numpy(np.stack([dream_scene.texture(H, W, 10 * t + b) for b in range(B)])).to(DEV) for t in range(4)]
        row = dict(B=B)
        for name, refit in (("step", None), ("step_refit", KinematicRefit(robot, "holistic", prior_q=1.0))):
            trk = PoseTracker(model, robot, K, (H, W), streams=B, device=DEV, refit=refit)
            trk.reset(seeds(B))
            lat, thr = wall(trk.step, seq)
            row[name + "_latency_ms"], row[name + "_pipelined_ms"] = round(lat, 3), round(thr, 3)
            if refit is not None:
                st = trk.refit_result.status.cpu().numpy()
                row["refit_flags"], row["refit_trials"] = sorted(set(int(v) for v in st[:, 0])), [int(st[:, 1].min()), int(st[:, 1].max())]
        print(json.dumps(row), flush=True)


def main():
    model = model_bf16()
    robot = URDFRobot("panda")
    if "--refit" in sys.argv[1:]:
        return bench_refit(model, robot)
    for B in (1, 4):
        seq = [torch.from_numpy(np.stack([dream_scene.texture(H, W, 10 * t + b) for b in range(B)])).to(DEV) for t in range(4)]
        print(json.dumps(bench_acquire(model, robot, B, seq)), flush=True)
        if "--verify" in sys.argv[1:]:
            print(json.dumps(bench_verify(model, robot, B, seq)), flush=True)
    if "--acquire" in sys.argv[1:] or "--verify" in sys.argv[1:]:
        return
    for B in (1, 4, 16):
        seq = [torch.from_numpy(np.stack([dream_scene.texture(H, W, 10 * t + b) for b in range(B)])).to(DEV) for t in range(4)]
        eager, replay = bench_launches(B, seq[0])
        trk = PoseTracker(model, robot, K, (H, W), streams=B, device=DEV)
        trk.reset(seeds(B))
        lat, thr = wall(trk.step, seq)
        syncs = forward_syncs(model, trk.prepare(seq[0]))
        lost = int((trk.status != 0).sum())
        host = HostLoop(model, B)
        hlat, hthr = wall(host.step, seq)
        print(json.dumps(dict(B=B, prepare_update_eager_us=round(eager, 1), prepare_update_graph_us=round(replay, 1),
                              step_latency_ms=round(lat, 3), step_fps=round(B / lat * 1e3, 1), step_pipelined_ms=round(thr, 3),
                              step_pipelined_fps=round(B / thr * 1e3, 1), host_loop_latency_ms=round(hlat, 3),
                              host_loop_fps=round(B / hlat * 1e3, 1), host_loop_pipelined_ms=round(hthr, 3),
                              launches_per_frame_outside_model=3, streams_without_estimate_at_end=lost, forward_syncs=syncs)),
              flush=True)


if __name__ == "__main__":
    main()
