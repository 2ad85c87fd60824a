#!/usr/bin/env python3
"""Benchmark of the HoRoPose image->pose hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W

N > 1 without a torch.distributed environment: this process (which never touches the GPU) starts N ranks of itself
through torch.distributed.run and relays rank 0's line; under torch.distributed.run it is one of the ranks.

Workloads (--workload):
  full   (default, the headline) one training step of the reference's full network (RootNetwithRegInt with HRNet-W32
         as the regression AND the root/depth backbone, configs[2] of BASELINE.json) on one synthetic batch of 64
         256x256 images per GPU: forward, loss of lib/core/function.py:191-322, backward, gradient all-reduce (N > 1),
         clip_grad_norm_(5.0) and the Adam update (scripts/train_full.py:53-67).
  hrnet  the metric's literal workload: ONE HRNet-W32 (RootNet("hrnet32") = DepthNet, scripts/train_depthnet.py:231-250)
         forward + L1 loss + backward + clip + Adam, B = 64.
  --forward-only   BASELINE.json configs[1]: eval-mode forward of the chosen workload (BatchNorm folded).
The convolution trunk runs in bf16 on MFMA, heads in fp32.  The whole step is captured once in a HIP graph and replayed.

Prints ONE JSON line (rank 0): images/sec over all GPUs and the milliseconds of one timed step (`ms_per_step`).  A plain run
does only that: set up, warm up, time --steps steps, write the outputs of the last step (--dump-outputs DIR), print the line.

--full adds everything else, each part a run of its own after the timed steps: the roofline entry of the dominant kernel
family and the per-family kernel times (durations measured with HIP events on the launch stream in an instrumented pass of
the same step), the step time without the optimizer, the end-to-end key-point error in pixels against the reference's
fixture, the secondary workloads and precisions (hrnet_step, forward_only, fp32_step, ... in child processes) and a CPU
baseline of the same step timed with the oracle on the host cores.

--dump-outputs DIR writes what the timed path computed in its last step as DIR/<name>.npy (float32, or float64 where the
tensor is): the forward outputs, the loss and, for a training step, the parameters after the update and their gradients.
An array of more than DUMP_SAMPLE elements is a fixed, seeded sample of DUMP_SAMPLE of them (the parameters and gradients:
the same positions of the flat concatenation in model.parameters() order).  The inputs are seeded: the same arguments give
the same inputs in every run.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import hrpe_amd  # noqa: E402,F401
from hrpe_amd import _native as nv  # noqa: E402
from hrpe_amd.lib.core.function import compute_k_values, depth_l1_loss, full_loss  # noqa: E402
from hrpe_amd.lib.dataset.const import INITIAL_JOINT_ANGLE, JOINT_BOUNDS  # noqa: E402
from hrpe_amd.lib.utils.geometries import rotmat_to_rot6d  # noqa: E402
from hrpe_amd.optim import FusedClipAdam  # noqa: E402
from hrpe_amd.parallel import GradAllReducer, broadcast_module, init_distributed  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0   # dense MFMA bf16, MI355X_MICROARCH.md
PEAK_F32_TFLOPS = 157.3
PEAK_HBM_GBS = 8000.0       # HBM3E peak (MI355X_MICROARCH.md; ~6300 achievable)
PEAK_HBM_GBS = 8000.0
# algorithmic forward FLOP per image (2*MAC over conv/linear), SURVEY.md 6: HRNet-W32 hm+feat 23.416 G,
# DepthNet trunk 23.299 G, heads 0.05 G; fwd+bwd = 3x
FWD_GFLOP_PER_IMAGE = {"full": 23.416 + 23.299 + 0.05, "depthnet": 23.299}


class Args(dict):
    __getattr__ = dict.__getitem__


REG_BACKBONE = os.environ.get("HRP_BENCH_REG_BACKBONE", "hrnet32")   # "resnet50" = the shipped full.yaml pairing


def model_args(p_dropout):
    return Args(backbone_name=REG_BACKBONE, rootnet_backbone_name="hrnet32", other_image_size=256.0, use_rpmg=False,
                n_iter=4, p_dropout=p_dropout, reg_joint_map=False, joint_conv_dim=[], rotation_dim=6,
                direct_reg_rot=False, rot_iterative_matmul=False, fix_root=True, bbox_3d_shape=[1300, 1300, 1300],
                reference_keypoint_id=3, add_fc=False, multi_kp=False, kps_need_depth=None, pretrained_rootnet=None)


def random_rotations(g, n):
    q = g.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)
    return R.reshape(n, 3, 3).astype(np.float32)


def synthetic_batch(B, seed):
    """Panda-DR-shaped synthetic batch: images U[0,1), crop intrinsics, boxes, poses."""
    g = np.random.Generator(np.random.PCG64(seed))
    d = {}
    d["x_reg"] = g.random((B, 3, 256, 256), dtype=np.float32)
    d["x_root"] = g.random((B, 3, 256, 256), dtype=np.float32)
    s = g.uniform(0.8, 2.5, B).astype(np.float32)
    K = np.zeros((B, 3, 3), np.float32)
    K[:, 0, 0] = K[:, 1, 1] = 320.0 * s
    K[:, 0, 2] = K[:, 1, 2] = 128.0
    K[:, 2, 2] = 1.0
    side = g.uniform(80.0, 240.0, B).astype(np.float32)
    d["K"] = K
    d["bbox"] = np.stack([128 - side / 2, 128 - side / 2, 128 + side / 2, 128 + side / 2], 1).astype(np.float32)
    b = np.array(JOINT_BOUNDS["panda"])
    d["q"] = (b[:, 0] + (b[:, 1] - b[:, 0]) * g.random((B, 8))).astype(np.float32)
    d["R"] = random_rotations(g, B)
    d["t"] = np.stack([g.uniform(-.3, .3, B), g.uniform(-.3, .3, B), g.uniform(.6, 2.0, B)], 1).astype(np.float32)
    return d


def build_model(p_dropout):
    from hrpe_amd.lib.models.full_net import RootNetwithRegInt
    init = {"robot_type": "panda", "pose_params": INITIAL_JOINT_ANGLE, "cam_params": np.eye(4),
            "init_pose_from_mean": True}
    torch.manual_seed(808)  # reference seed, scripts/train_full.py:18
    m = RootNetwithRegInt(init, model_args(p_dropout))
    # random init of this architecture, scaled so that activations stay O(1) (the reference's own
    # N(0, sqrt(2/n)) conv init on top of BN would do as well; values do not change the work done)
    return m


def host_cores():
    """Cores this process may actually use: the affinity mask, capped by the cgroup CPU quota (the GPU boxes expose
    256 hardware threads behind a 16-CPU quota - 64 threads there run the oracle 5x slower than 16)."""
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    for path, parse in (("/sys/fs/cgroup/cpu.max", lambda t: t.split()),
                        ("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", lambda t: (t.strip(), None))):
        try:
            with open(path) as fh:
                quota, period = parse(fh.read())
            if period is None:
                with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as fh:
                    period = fh.read().strip()
            if quota != "max" and int(quota) > 0:
                cores = min(cores, max(1, int(quota) // int(period)))
            break
        except (OSError, ValueError):
            continue
    return max(1, min(cores, 64))


def cpu_baseline(B, threads, workload="full", forward_only=False):
    """The same step (forward, loss, backward; or the eval forward) on the host with the CPU oracle (fp32)."""
    from oracle import fk as ofk, heads as oheads
    torch.set_num_threads(threads)
    d = {k: torch.tensor(v) for k, v in synthetic_batch(B, 1).items()}
    K = d["K"]
    kv = torch.sqrt(K[:, 0, 0] * K[:, 1, 1] * 1e6 / (d["bbox"][:, 2] - d["bbox"][:, 0]) ** 2)
    if workload == "hrnet":
        m = build_depthnet()
    else:
        m = build_model(0.0)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    if not forward_only:
        for k, v in sd.items():
            if v.dtype.is_floating_point and "running" not in k and not k.startswith("init_"):
                v.requires_grad_(True)
    if workload == "hrnet":
        gt_depth = d["t"][:, 2:3]

        def step():
            for v in sd.values():
                v.grad = None
            if forward_only:
                with torch.no_grad():
                    oheads.rootnet_forward(sd, d["x_root"], kv, training=False)
                return
            pred = oheads.rootnet_forward(sd, d["x_root"], kv, training=True) / 1000.0
            torch.nn.functional.l1_loss(pred, gt_depth).backward()
        what = "DepthNet (one HRNet-W32)"
    else:
        robot = ofk.Robot(os.path.join(ROOT, "holistic-robot-pose-estimation_amd", "assets", "panda_kinematics.urdf"))
        rot6 = ofk.rotmat_to_rot6d(d["R"])
        with torch.no_grad():
            kp3d = robot.get_keypoints(d["q"], rot6, d["t"])
            kp2d = ofk.project(K, kp3d)
            gt = dict(pose=d["q"], root_rot=robot.get_rotation_at_specific_root(d["q"], rot6, d["t"], root=3),
                      root_trans=kp3d[:, 3], root_uv=kp2d[:, 3], kp3d=kp3d, kp2d=kp2d, mask=torch.ones(B, 7))

        def step():
            for v in sd.values():
                v.grad = None
            if forward_only:
                with torch.no_grad():
                    oheads.full_forward(sd, robot, d["x_reg"], d["x_root"], kv, K, training=False, reg_backbone=REG_BACKBONE)
                return
            pred = oheads.full_forward(sd, robot, d["x_reg"], d["x_root"], kv, K, training=True, reg_backbone=REG_BACKBONE)
            loss, _ = oheads.full_loss(pred, gt, K)
            loss.backward()
        what = "full-network"

    step()                      # warm-up: oneDNN primitive creation, allocator
    t0, n = time.time(), 0
    while n < 3 or (time.time() - t0 < 12.0 and n < 200):   # a bounded sample: >= 3 steps, about 12-15 s of CPU work
        step()
        n += 1
    dt = time.time() - t0
    return {"value": B * n / dt, "unit": "images/sec", "cores": threads, "kind": "port",
            "sample": f"oracle (torch fp32 CPU restatement) {what} {'eval forward' if forward_only else 'forward+loss+backward'}, "
                      f"B={B}, 1 warm-up + {n} timed steps, {dt:.1f} s"}


def build_depthnet():
    from hrpe_amd.lib.models.depth_net import get_rootnet
    torch.manual_seed(808)
    return get_rootnet("hrnet32")


def launch_descs(name, args):
    """-> (family entry point, descriptors) of one launch: a single C-ABI call or one batched launch of n problems.
    A launch counts towards the family of the REFERENCE operation it carries out: the backward forms of the Bottleneck tail
    (hrp_conv_desc.tail_mode 3 / 4, csrc/conv_pw.h) enter through hrp_conv2d_fwd but ARE the BatchNorm backward's reduce / apply
    passes (they replace hrp_ew_bwd_reduce / _apply launches one for one) - they are listed with those families and keep their
    time out of the convolution family's roofline, which prices convolutions by SURVEY 8(d) bytes; the forward forms (mode 1:
    the product's statistics, mode 2 / 5: the product with its BatchNorm, shortcut and ReLU) are the convolution."""
    if name == "hrp_batch_launch":
        b = args[0]
        return nv.FAMILY_FN[b.fam], [it.desc for it in b.items]
    if name == "hrp_block_launch":      # fused inference blocks (hrp_block_desc)
        return name, [it.desc for it in args[0].items]
    try:
        d = args[0]._obj
    except (AttributeError, IndexError):
        return name, []
    if name == "hrp_conv2d_fwd" and getattr(d, "tail_mode", 0) in (3, 4):
        return ("hrp_ew_bwd_reduce" if d.tail_mode == 3 else "hrp_ew_bwd_apply"), [d]
    return name, [d]


def conv_flops(name, args):
    """Algorithmic FLOP of one launch from its descriptor(s) (real channel counts)."""
    fam, descs = launch_descs(name, args)
    if fam == "hrp_conv2d_fwd":
        # (the Bottleneck-tail launches - hrp_conv_desc.tail_mode - multiply again what the reference multiplies once: only the launch
        # that writes the layer's output, mode 2, counts as the layer's algorithmic FLOP)
        return sum(2.0 * d.N * d.Ho * d.Wo * d.Cout * d.Cin * d.ntaps * (2 if getattr(d, "tail_mode", 0) == 5 else 1)
                   for d in descs if getattr(d, "tail_mode", 0) in (0, 2, 5))
    if fam == "hrp_conv2d_bwd_weight":
        return sum(2.0 * d.N * d.Ho * d.Wo * d.Cout * d.dw_cin * d.ntaps for d in descs)
    if fam == "hrp_block_launch":       # both convolutions of the block
        return sum(2 * 2.0 * q.conv1.N * q.conv1.Ho * q.conv1.Wo * q.conv1.Cout * q.conv1.Cin * q.conv1.ntaps for q in descs)
    return 0.0


def conv_bytes(name, args, extended=False):
    """Algorithmic HBM bytes of one launch by SURVEY 8(d): the layer's input read once, its output written once, its weights
    once.  extended=True adds what THIS design moves on top inside the same launch - residuals, the operands of the fused
    BatchNorm prologues / epilogues, side outputs - reported as `bytes_incl_fused_operands`, never used for `frac`."""
    fam, descs = launch_descs(name, args)
    if fam == "hrp_block_launch":       # what the fused block must move: x read once, out written once, both weights
        return float(sum(2 * d.conv1.N * d.conv1.H * d.conv1.W * d.conv1.Cin * 2 + 2 * 9 * d.conv1.Cin * d.conv1.Cout * 2 for d in descs))
    if fam not in ("hrp_conv2d_fwd", "hrp_conv2d_bwd_weight"):
        return 0.0       # (incl. the tail's backward forms, listed with the element-wise backward families: launch_descs)
    tot = 0.0
    for d in descs:
        esz = 2 if d.dtype == nv.HRP_BF16 else 4
        if fam == "hrp_conv2d_fwd":
            b = (d.N * d.H * d.W * d.Cin + d.N * d.Ho * d.Wo * d.Cout + d.ntaps * d.Cin * d.Cout) * esz
            tm = getattr(d, "tail_mode", 0)
            if tm == 1:
                # the statistics pass of a Bottleneck tail multiplies what mode 2 / 5 multiplies again: part of the SAME convolution of
                # SURVEY 8(d) - zero strict bytes of its own (its TIME stays in the family); extended: what it moves
                tot += d.N * d.H * d.W * d.Cin * esz if extended else 0.0
                continue
            if tm == 5:       # two layers in one launch (conv3 and the projection): both inputs, both weights, one output
                b += (d.N * d.H * d.W * d.Cin + d.ntaps * d.Cin * d.Cout) * esz
            if extended:
                if d.res:
                    b += d.N * d.Ho * d.Wo * d.Cout * esz
                if d.bnb_x:      # BatchNorm-backward reduce in the epilogue: reads the BatchNorm input once (+ 1/16 mask)
                    b += d.N * d.Ho * d.Wo * d.Cout * esz
                # fused BatchNorm prologues of the row-strip kernels: the second operand (BatchNorm input) read once, every side
                # output written once (an accumulated one also read)
                tin = d.N * d.H * d.W * d.Cin * esz
                if d.pro_mode == 2:
                    b += tin
                b += tin * (bool(d.pro_side) + bool(d.pro_side2) * (2 if d.pro_side2_acc else 1))
            tot += b
        else:
            tot += (d.N * d.H * d.W * d.Cin + d.N * d.Ho * d.Wo * d.Cout) * esz + d.Cout * d.dw_cin * d.ntaps * 4
    return float(tot)


def self_launch(a, argv):
    """`python bench.py --gpus N` outside torch.distributed.run: start N ranks as children of a process that has made no
    GPU call (never exec from a process that initialised HIP), relay their output and exit code."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + argv
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    r = subprocess.run(cmd, env=env)
    raise SystemExit(r.returncode)


def keypoint_px_error(dev, dtypes):
    """End-to-end key-point error in pixels on the reference's eval fixture (tests/golden/golden_full_eval.npz, written by
    the reference itself, B = 2): the network's FK key-points and the reference's, both projected with K
    (lib/utils/transforms.py:17-21).  -> {dtype name: max |uv - uv_ref| in px}"""
    gdir = os.path.join(ROOT, "tests", "golden")
    path = os.path.join(gdir, "golden_full_eval.npz")
    if not os.path.exists(path) or REG_BACKBONE != "hrnet32":      # (the fixture is the all-HRNet-W32 network's)
        return None
    sys.path.insert(0, gdir)
    from synth import synth_inputs, synth_state_dict
    from hrpe_amd.lib.models.full_net import RootNetwithRegInt
    from hrpe_amd.lib.utils.transforms import point_projection_from_3d_tensor
    g = np.load(path)
    init = {"robot_type": "panda", "pose_params": INITIAL_JOINT_ANGLE, "cam_params": np.eye(4), "init_pose_from_mean": True}
    m = RootNetwithRegInt(init, model_args(0.0))
    m.load_state_dict(synth_state_dict(m.state_dict()))
    m = m.to(dev).eval()
    x_reg, x_root, kv, K = [t.to(dev) for t in synth_inputs(2)]
    ref_uv = point_projection_from_3d_tensor(K, torch.tensor(g["xyz_fk"]).to(dev))
    # the reference's arithmetic in float64 on the same inputs (golden_full_eval_fp64.npz, gen_golden.py full_eval_fp64): what the
    # reference's own fp32 run loses is the yardstick for the fp32 path here
    p64 = os.path.join(gdir, "golden_full_eval_fp64.npz")
    g64 = np.load(p64) if os.path.exists(p64) else None
    uv64 = point_projection_from_3d_tensor(K.double(), torch.tensor(g64["xyz_fk"]).to(dev)) if g64 is not None else None
    out = {}
    for name, dt in dtypes:
        m.set_compute_dtype(dt)
        with torch.no_grad():
            o = m(x_reg, x_root, kv, K)
        uv = point_projection_from_3d_tensor(K, o[7])
        out[name] = round(float((uv - ref_uv).abs().max()), 6)
        if uv64 is not None:
            e = (uv.double() - uv64).abs().amax(-1)            # [B, key-points]
            out[name + "_vs_fp64"] = round(float(e.max()), 6)
            if name == "bf16":   # key-point 0 of the fixture sits 0.13 m in front of the camera: 1 / z amplifies everything there
                out["bf16_by_keypoint"] = [round(float(v), 3) for v in e.amax(0)]
    if g64 is not None:
        out["reference_fp32_vs_fp64"] = round(float(g64["ref_fp32_px_err"].max()), 6)
    return out


DUMP_SAMPLE = 1 << 20      # elements per dumped array at most (a seeded sample beyond): 4-8 MB each, far below 64 MB in all
OUTPUT_NAMES = ("pose", "rot", "trans", "root_uv", "depth", "uvd", "xyz_int", "xyz_fk")     # RootNetwithRegInt.forward


def _host(t):
    return t.detach().to(torch.float64 if t.dtype == torch.float64 else torch.float32).cpu().numpy()


def _sample(tensors, seed):
    """The flat concatenation of `tensors` or, beyond DUMP_SAMPLE elements, the same seeded DUMP_SAMPLE positions of it, in
    order.  tensors: [(tensor, numel)]; a None tensor stands for numel zeros (a parameter without a gradient)."""
    total = sum(n for _, n in tensors)
    idx = np.arange(total) if total <= DUMP_SAMPLE else \
        np.sort(np.random.Generator(np.random.PCG64(seed)).choice(total, DUMP_SAMPLE, replace=False))
    parts, off = [], 0
    for t, n in tensors:
        lo, hi = np.searchsorted(idx, [off, off + n])
        if hi > lo:
            parts.append(np.zeros(hi - lo, np.float32) if t is None else
                         _host(t.detach().reshape(-1)[torch.from_numpy(idx[lo:hi] - off).to(t.device)]))
        off += n
    return np.concatenate(parts) if parts else np.zeros(0, np.float32)


def dump_outputs(path, holder, params):
    """--dump-outputs: what the last timed step computed, as the step's caller receives it - the forward outputs, the loss and,
    for a training step (params not None), the parameters after the update and this step's gradients."""
    os.makedirs(path, exist_ok=True)
    outs = holder["outputs"]
    names = OUTPUT_NAMES if len(outs) == len(OUTPUT_NAMES) else ("depth",)      # the full network / DepthNet
    arrays = {n: _host(t) if t.numel() <= DUMP_SAMPLE else _sample([(t, t.numel())], 1) for n, t in zip(names, outs)}
    arrays["loss"] = _host(holder["loss"])
    if params is not None:
        arrays["params"] = _sample([(p, p.numel()) for p in params], 2)
        arrays["grads"] = _sample([(p.grad, p.numel()) for p in params], 2)
    for n, v in arrays.items():
        np.save(os.path.join(path, n + ".npy"), v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64, help="images per GPU")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32", "fp32x3"],
                    help="fp32x3: fp32 tensors, convolution products as three bf16 MFMAs on split operands (HRP_F32X3)")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--torch-optim", action="store_true", help="clip_grad_norm_ + torch.optim.Adam(fused) instead of FusedClipAdam")
    ap.add_argument("--forward-only", action="store_true",
                    help="BASELINE.json configs[1]: eval-mode forward of the full network (folded BN), images/s to stderr-free JSON")
    ap.add_argument("--cpu-batch", type=int, default=4)
    ap.add_argument("--cpu-threads", type=int, default=0, help="host threads of the CPU baseline (0 = all cores, at most 64)")
    ap.add_argument("--p-dropout", type=float, default=0.5, help="lib/core/config.py:70 default")
    ap.add_argument("--cpu-baseline-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--workload", default="full", choices=["full", "hrnet"],
                    help="full: the full network (headline, BASELINE.json configs[2]); hrnet: one HRNet-W32 (DepthNet), the metric's literal workload")
    ap.add_argument("--no-extra", action="store_true",
                    help="--full: skip the secondary measurements in child processes (hrnet_step, forward_only, fp32_step, ...)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)   # a secondary measurement of a --full invocation
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also: instrumented per-kernel pass + roofline, step without the optimizer, key-point "
                         "pixel error, the secondary workloads / precisions (unless --no-extra) and the CPU baseline (unless --no-cpu-baseline)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (see the module docstring)")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        raise SystemExit("bench.py: --steps must be >= 1 and --warmup >= 0")
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ and not a.cpu_baseline_only:
        self_launch(a, sys.argv[1:])

    if a.cpu_baseline_only:
        cores = host_cores()
        print(json.dumps(cpu_baseline(a.cpu_batch, a.cpu_threads or cores, a.workload, a.forward_only)))
        return

    rank, world, local = init_distributed()
    if world != a.gpus:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but the launcher started {world} rank(s): the line would be mislabelled")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: no HIP device visible (there is no CPU path)")
    if os.environ.get("HRP_BENCH_DEVICE"):   # functional test of the N > 1 structure with all ranks on one GPU (gloo)
        local = int(os.environ["HRP_BENCH_DEVICE"])
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    if not nv.lib().hrp_device_ok():
        raise SystemExit("libhrp_hip.so is built for gfx950 only")
    B = a.batch
    dtype = torch.bfloat16 if a.dtype == "bf16" else (torch.float32 if a.dtype == "fp32" else "fp32x3")

    hrnet = a.workload == "hrnet"
    fwd_only = a.forward_only
    model = (build_depthnet() if hrnet else build_model(0.0 if fwd_only else a.p_dropout)).to(dev).set_compute_dtype(dtype)
    model.train(not fwd_only)
    if not fwd_only:
        broadcast_module(model)
    params = [p for p in model.parameters() if p.requires_grad]
    # Adam(lr 1e-4) as scripts/train_full.py:42; fused multi-tensor kernels (the default foreach path spends
    # ~3 500 tiny launches per step on the per-parameter step counters)
    opt = None
    if not fwd_only:
        if a.torch_optim:
            opt = torch.optim.Adam(params, lr=1e-4, fused=True, capturable=not a.no_graph)
        else:   # clip_grad_norm_(5) + Adam as two table-driven launches (hrpe_amd/optim.py)
            opt = FusedClipAdam(params, lr=1e-4, max_norm=1.0 if hrnet else 5.0)   # depthnet.yaml clips at 1, full.yaml at 5
    reducer = GradAllReducer(bucket_mb=64)
    info = {}

    d = {k: torch.tensor(v).to(dev) for k, v in synthetic_batch(B, 808 + rank).items()}
    K = d["K"]
    kv = compute_k_values(K[:, 0, 0], K[:, 1, 1], d["bbox"])
    loss_holder = {}

    def keep(out):
        """The forward's outputs as the caller of the step receives them (detached views; a captured graph rewrites them on every
        replay): what --dump-outputs writes after the timed steps."""
        loss_holder["outputs"] = tuple(t.detach() for t in (out if isinstance(out, tuple) else (out,)))
        return out

    h2d = os.environ.get("HRP_BENCH_H2D")
    if h2d in ("u8", "u8res"):     # the dataset's bytes: the model's input kernel divides by 255
        for k in ("x_reg", "x_root"):
            d[k] = (d[k] * 255).to(torch.uint8)
    if hrnet:
        gt_depth = d["t"][:, 2:3].contiguous()

        def forward():
            return keep(model(d["x_root"], kv))

        def fwd_bwd():
            loss = depth_l1_loss(forward(), gt_depth)   # scripts/train_depthnet.py:231-250 (one launch, analytic gradient)
            loss.backward()
            loss_holder["loss"] = loss.detach()
    else:
        rot6 = rotmat_to_rot6d(d["R"])
        with torch.no_grad():
            kp3d, kp2d = model.robot.get_keypoints_and_projection(d["q"], rot6, d["t"], K, root=0)
            gt = dict(pose=d["q"], root_rot=model.robot.get_rotation_at_specific_root(d["q"], rot6, d["t"], root=3),
                      root_trans=kp3d[:, 3].clone(), root_uv=kp2d[:, 3].clone(), kp3d=kp3d, kp2d=kp2d,
                      mask=torch.ones(B, 7, device=dev))

        def forward():
            return keep(model(d["x_reg"], d["x_root"], kv, K))

        def fwd_bwd():
            loss, _ = full_loss(forward(), gt, K)
            loss.backward()
            loss_holder["loss"] = loss.detach()
    if fwd_only:
        def fwd_bwd():    # noqa: F811  (the "step" of a forward-only run)
            with torch.no_grad():
                loss_holder["loss"] = forward()[0].float().mean()

    def update():
        if fwd_only:
            return
        if a.torch_optim:
            torch.nn.utils.clip_grad_norm_(params, 1.0 if hrnet else 5.0)   # configs/panda/full.yaml:39, depthnet.yaml
        opt.step()

    def step_eager():
        fwd_bwd()
        if not fwd_only:
            reducer(model.flat_grads())
        update()

    # first step eagerly: builds the plan, allocates gradients / optimizer state
    step_eager()
    torch.cuda.synchronize(dev)

    use_graph = not a.no_graph
    if use_graph:
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            step_eager()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        from hrpe_amd.parallel import force_world1
        # (HRP_BENCH_TWO_GRAPHS exercises the N > 1 graph structure on one GPU; HRP_DIST_WORLD1=1 also creates the RCCL group of one
        # rank and issues every collective of the k-cut step)
        if fwd_only or (world == 1 and not os.environ.get("HRP_BENCH_TWO_GRAPHS") and not force_world1()):
            g1 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g1):
                fwd_bwd()
                update()

            def step():
                g1.replay()
        else:
            # process-group threads (the RCCL watchdog polls events) keep running while this thread captures: only this
            # thread's calls are held to the capture rules
            gmode = dict(capture_error_mode="thread_local")

            def capture_plain():
                g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
                with torch.cuda.graph(g1, **gmode):
                    fwd_bwd()
                with torch.cuda.graph(g2, **gmode):
                    update()

                def step():
                    g1.replay()
                    reducer(model.flat_grads())
                    g2.replay()
                return step

            def capture_overlapped():
                """Backward in k + 1 graphs around the plan's cuts (PlannedModule.enable_split_backward(fracs=...)): the gradients
                that are final after a segment - first the heads, then stage 4, then stage 3 - are all-reduced while the next
                segment runs; only the stems' and stage 2's gradients (a few per cent of the bytes) travel behind the backward."""
                if os.environ.get("HRP_NO_AR_OVERLAP"):
                    info["ar_overlap"] = {"enabled": False, "reason": "HRP_NO_AR_OVERLAP is set"}
                    return None
                fracs = tuple(float(v) for v in os.environ.get("HRP_AR_SPLITS", "0.25,0.5,0.8,0.9").split(","))
                sp = model.enable_split_backward(fracs=fracs)
                if sp is None:
                    info["ar_overlap"] = {"enabled": False, "reason": "the plan has no top-level cut positions for these fractions"}
                    return None
                plan, groups = sp
                arena = plan.grad_arena
                # small ranges are not worth a collective of their own: they travel with the rest
                groups = [[(o, n) for o, n in grp if n >= (1 << 18)] for grp in groups]
                covered = [r for grp in groups for r in grp]
                rest = GradAllReducer.complement(covered, arena.numel())
                nseg = len(plan.bwd_cuts) + 1
                g_first, g_upd = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
                g_seg = [torch.cuda.CUDAGraph() for _ in range(nseg - 1)]
                with torch.cuda.graph(g_first, **gmode):
                    fwd_bwd()                       # (split active: the backward stops at the first cut)
                for j, gj in enumerate(g_seg):
                    with torch.cuda.graph(gj, **gmode):
                        plan.run_backward(("seg", j + 1))
                with torch.cuda.graph(g_upd, **gmode):
                    update()
                # self-check on this machine (PlannedModule.check_split_backward: every later segment must leave the ranges
                # already handed to RCCL untouched, bit for bit), here on the captured graphs' first part
                g_first.replay()
                model.check_split_backward(groups)
                if sum(n for _, n in covered) + sum(n for _, n in rest) != arena.numel():
                    raise RuntimeError("split backward self-check failed: ranges do not cover the arena")
                info["ar_overlap"] = {"enabled": True, "cuts": list(plan.bwd_cuts), "bwd_ops": len(plan.bwd_ops()),
                                      "final_fraction_after_each_cut": [round(sum(n for grp in groups[:j + 1] for _, n in grp) / arena.numel(), 3)
                                                                         for j in range(len(groups))],
                                      "tail_fraction": round(sum(n for _, n in rest) / arena.numel(), 3),
                                      "payload": reducer.payload}

                def step():
                    g_first.replay()
                    w = reducer.start(arena, groups[0])
                    for j, gj in enumerate(g_seg):
                        gj.replay()
                        if j + 1 < len(groups):
                            w += reducer.start(arena, groups[j + 1])
                    w += reducer.start(arena, rest)
                    reducer.finish(w, [arena])
                    g_upd.replay()
                return step

            step = None
            try:
                step = capture_overlapped()
            except Exception as e:   # anything unexpected: the plain two-graph step - said in the line, not only on stderr
                print(f"warning: overlapped all-reduce disabled ({e!r})", file=sys.stderr)
                info["ar_overlap"] = {"enabled": False, "reason": repr(e)[:300]}
                step = None
            if world > 1:   # every rank must issue the same sequence of collectives: one failure -> all fall back
                flag = torch.tensor([1.0 if step is not None else 0.0], device=dev)
                torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MIN)
                if flag.item() < 0.5 and step is not None:
                    step = None
                    info["ar_overlap"] = {"enabled": False, "reason": "another rank could not set up the split backward"}
            if step is None:
                model.disable_split_backward()
                step = capture_plain()
    else:
        step = step_eager

    # Opt-in (never the headline `value`): HRP_BENCH_H2D=u8|f32 feeds every step's two image batches from pinned host
    # memory - the dataset's bytes (the model's input kernel divides by 255) or the reference's fp32
    # images - through a staging buffer filled on a copy stream while the previous step computes.
    if h2d:
        assert h2d in ("u8", "f32", "u8res") and use_graph
        inner = step
        host = {k: d[k].cpu().pin_memory() for k in ("x_reg", "x_root")}
        staging = {k: torch.empty_like(d[k]) for k in host}
        copy_stream = torch.cuda.Stream(dev)
        ready, consumed = torch.cuda.Event(), torch.cuda.Event()
        consumed.record()

        def fill():
            with torch.cuda.stream(copy_stream):
                copy_stream.wait_event(consumed)
                for k in host:
                    staging[k].copy_(host[k], non_blocking=True)
                ready.record()

        fill()

        def step():
            if h2d == "u8res":      # development aid: uint8 images resident in HBM
                return inner()
            cur = torch.cuda.current_stream(dev)
            cur.wait_event(ready)
            for k in host:
                d[k].copy_(staging[k])
            consumed.record(cur)
            fill()
            inner()

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize(dev)

    for _ in range(a.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([dt], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.MAX)
        dt = tt.item()
    final_loss = float(loss_holder["loss"].item())
    if a.dump_outputs and rank == 0:     # before anything else runs the step again
        dump_outputs(a.dump_outputs, loss_holder, None if fwd_only else params)

    # the same step without clip + Adam (SURVEY 8d C3 "Adam excluded and included: report both"), one GPU only
    ms_no_opt = None
    if a.full and world == 1 and use_graph and not fwd_only and not h2d and not os.environ.get("HRP_BENCH_TWO_GRAPHS") and not force_world1():
        gno = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gno):
            fwd_bwd()
        for _ in range(2):
            gno.replay()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            gno.replay()
        torch.cuda.synchronize(dev)
        ms_no_opt = (time.perf_counter() - t0) / a.steps * 1e3

    if rank != 0:
        return
    ms_per_step = dt / a.steps * 1e3
    value = B * world * a.steps / dt

    from hrpe_amd import plan as plan_mod
    # (fp32x3: three bf16 MFMAs per product - its roof is a third of the bf16 matrix peak)
    peak = PEAK_BF16_TFLOPS if a.dtype == "bf16" else (PEAK_F32_TFLOPS if a.dtype == "fp32" else PEAK_BF16_TFLOPS / 3.0)
    gf_img = FWD_GFLOP_PER_IMAGE["depthnet" if hrnet else "full"] * (1 if fwd_only else 3)
    step_tflops = gf_img * 1e9 * B * world / (ms_per_step * 1e-3) / 1e12 / world     # per GPU
    passes = 1 if hrnet else 2
    net = ("one HRNet-W32 (RootNet('hrnet32') = DepthNet, the metric's literal workload)" if hrnet else
           f"full network ({'HRNet-W32' if REG_BACKBONE.startswith('hrnet') else REG_BACKBONE + ' + deconv head'} reg backbone + "
           "HRNet-W32 DepthNet + heads + FK loss)")
    what = (f"{net} eval forward (BatchNorm folded), BASELINE.json configs[1]" if fwd_only else
            f"{net} fwd+loss+bwd+clip+Adam" + ("" if hrnet else ", BASELINE.json configs[2]"))
    clip = 1 if hrnet else 5
    # which collective library carried the gradients: "rccl_ranks" is only printed when it was RCCL ("nccl" on ROCm) - a gloo
    # run (two ranks on one GPU, a development configuration) must not read as an RCCL measurement
    import torch.distributed as _dist
    backend = _dist.get_backend() if (_dist.is_available() and _dist.is_initialized()) else "single-process"
    out = {
        "metric": "images/sec/GPU fwd+bwd HRNet-W32 256x256 bs=64; 1/2/4/8-GPU scaling",
        "value": round(value, 2), "value_per_gpu": round(value / world, 2), "unit": "images/sec", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": a.dtype, "data": "synthetic",
        "config": {"workload": what,
                   "global_batch": B * world, "per_gpu_batch": B, "image": "3x256x256",
                   "hrnet_w32_passes_per_image": passes, "parallelism": f"dp{world}", "backend": backend,
                   **({"rccl_ranks": world} if backend in ("nccl", "single-process") else {}), "hip_graph": use_graph,
                   "plan_mode": plan_mod.PLAN_MODE, "p_dropout": 0.0 if (hrnet or fwd_only) else a.p_dropout,
                   "inputs": {None: "resident in HBM", "u8": "uint8 images from pinned host memory every step (PCIe-inclusive)",
                              "f32": "fp32 images from pinned host memory every step (PCIe-inclusive)",
                              "u8res": "uint8 images resident in HBM"}[h2d],
                   "optimizer": None if fwd_only else (f"clip_grad_norm_({clip})+torch.optim.Adam(fused)" if a.torch_optim else
                                                      f"hrpe_amd.optim.FusedClipAdam (clip {clip} + Adam, lr 1e-4)")},
        "hrnet_w32_passes_per_sec": round(passes * value, 2),
        "step_model_tflops": round(step_tflops, 2),
        "step_frac_of_mfma_peak": round(step_tflops / peak, 4),
        "loss": final_loss,
        **info,
    }
    if not a.full:      # a plain run: the headline line and nothing else
        print(json.dumps(out))
        return

    # ---- instrumented pass: HIP events around every C-ABI launch on the launch stream --------------
    records, records_shape = [], []

    def shape_key(name, args):
        fam, descs = launch_descs(name, args)
        if not descs:
            return ""
        def one(dd):
            if fam == "hrp_conv2d_fwd":
                return f"{dd.Cin}->{dd.Cout} taps{dd.ntaps} s{dd.in_stride}/{dd.out_stride} @{dd.Ho}x{dd.Wo}"
            if fam == "hrp_conv2d_bwd_weight":
                return f"{dd.Cin}->{dd.Cout} taps{dd.ntaps} s{dd.in_stride} @{dd.Ho}x{dd.Wo}"
            if fam == "hrp_ew_fwd":
                return f"C{dd.C} @{dd.H}x{dd.W} nin{dd.nin}"
            if fam.startswith("hrp_ew_bwd"):
                return f"C{dd.C} @{dd.H}x{dd.W} up{dd.inp.up} mode{dd.inp.mode}"
            return ""
        if len(descs) == 1:
            return one(descs[0])
        return f"batch{len(descs)}[" + " | ".join(sorted({one(dd) for dd in descs}))[:100] + "]"

    def hook(name, args, launch):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        fl = conv_flops(name, args)
        fam = launch_descs(name, args)[0]      # batched launches count towards their family
        records.append((fam, fl, e0, e1, conv_bytes(name, args), conv_bytes(name, args, extended=True)))
        if os.environ.get("HRP_BENCH_SHAPES"):
            records_shape.append((fam, fl, e0, e1, shape_key(name, args)))

    # lanes (concurrent graph branches) are folded onto one stream here: a kernel's duration is its own
    if not fwd_only:
        model.disable_split_backward()      # (N > 1: the timed step ran the backward in two graphs)
    plan_mod.SERIAL_LANES = True
    nv.set_profile_hook(hook)
    # park the stream behind a spin kernel while the host enqueues the step: the event intervals then are the
    # device-side durations (the Python launch loop alone would pace small kernels at ~10 us each)
    torch.cuda._sleep(int(os.environ.get("HRP_BENCH_SLEEP_CYCLES", "400000000")))
    fwd_bwd()
    nv.set_profile_hook(None)
    plan_mod.SERIAL_LANES = bool(os.environ.get("HRP_SERIAL_LANES"))
    torch.cuda.synchronize(dev)
    if os.environ.get("HRP_BENCH_SHAPES"):   # development aid: time per (kernel, shape) class to stderr
        shp = {}
        for name, fl, e0, e1, key in records_shape:
            v = shp.setdefault((name, key), [0, 0.0, 0.0])
            v[0] += 1
            v[1] += e0.elapsed_time(e1)
            v[2] += fl
        for (name, key), v in sorted(shp.items(), key=lambda kv: -kv[1][1])[:int(os.environ.get("HRP_BENCH_SHAPES", "40")) if os.environ.get("HRP_BENCH_SHAPES", "1") != "1" else 40]:
            tf = f"{v[2] / (v[1] * 1e-3) / 1e12:7.1f} TF/s" if v[2] else ""
            print(f"{name:24s} {key:44s} n={v[0]:4d} {v[1]:8.3f} ms  avg {v[1] / v[0] * 1e3:7.1f} us {tf}", file=sys.stderr)
    fam = {}
    for name, fl, e0, e1, by, byx in records:
        f = fam.setdefault(name, [0, 0.0, 0.0, 0.0, 0.0])
        f[0] += 1
        f[1] += e0.elapsed_time(e1)
        f[2] += fl
        f[3] += by
        f[4] += byx
    kernels = {n: {"launches": v[0], "ms": round(v[1], 3), "tflops": round(v[2] / (v[1] * 1e-3) / 1e12, 1) if v[2] else None}
               for n, v in sorted(fam.items(), key=lambda kv: -kv[1][1])}
    dom = max(fam.items(), key=lambda kv: kv[1][1])
    ach_tf = dom[1][2] / (dom[1][1] * 1e-3) / 1e12 if dom[1][2] else 0.0
    ach_gb = dom[1][3] / (dom[1][1] * 1e-3) / 1e9 if dom[1][3] else 0.0
    # which roof binds the family: its arithmetic intensity against the ridge point peak_flops / peak_bytes
    intensity = dom[1][2] / dom[1][3] if dom[1][3] else float("inf")
    hbm_bound = intensity < peak * 1e12 / (PEAK_HBM_GBS * 1e9)
    # measured HBM bytes per launch of the dominant family: the rocprofv3 PMC passes (FETCH_SIZE doubled, WRITE_SIZE; separate
    # passes over tools/one_step.py, the same network and batch) summarised in profiles/r02_traffic.json; a family = its
    # single-problem and its batched kernels together
    traffic, traffic_source = None, None
    tpath = next((pp for pp in (os.path.join(ROOT, "profiles", f"r{r:02d}_traffic.json") for r in (6, 5, 4, 3, 2)) if os.path.exists(pp)), None)
    fam_kernels = {"hrp_conv2d_fwd": ("conv_tile_kernel", "conv_batch_kernel", "conv_row_kernel", "conv_deep_kernel", "conv_img_kernel", "conv_pw_kernel",
                                      "conv_pw_tail_kernel", "conv_pw_tail2_kernel"),
                   "hrp_block_launch": ("block_kernel",),
                   "hrp_conv2d_bwd_weight": ("conv_wgrad_kernel", "wgrad_batch_kernel", "wgrad_octo_batch_kernel", "wgrad_octo_x3_batch_kernel",
                                             "wgrad_reduce_kernel", "wgrad_reduce_batch_kernel", "wgrad_fold_batch_kernel"),
                   "hrp_ew_fwd": ("ew_fwd_kernel", "ew_fwd_batch_kernel"),
                   "hrp_ew_bwd_reduce": ("ew_bwd_reduce_kernel",), "hrp_ew_bwd_apply": ("ew_bwd_apply_kernel",)}.get(dom[0])
    if tpath and fam_kernels and B == 64 and a.dtype == "bf16" and not hrnet and not fwd_only:
        with open(tpath) as fh:
            tj = json.load(fh)
        have = nv.lib().hrp_source_hash().decode()
        if tj.get("source_hash") != have:
            # the counter passes were collected on other sources than the library measured here: no figure rather than a stale one
            traffic_source = (f"dropped: profiles/{os.path.basename(tpath)} was collected on library sources {tj.get('source_hash')}, "
                              f"this run measures {have} (re-run tools/collect_profiles.sh)")
        else:
            by = sum(tj["families"].get(k, {}).get("hbm_bytes_per_step", 0.0) for k in fam_kernels)
            if by > 0:
                traffic = by / dom[1][0]      # per launch of the family as bench.py counts launches
                traffic_source = ("profiles/" + os.path.basename(tpath) + ": rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over "
                                  "tools/one_step.py (same network, batch and library sources), not collected in this run")
    # ... and the family's time inside the step as rocprofv3 saw it (kernel trace of this command, committed next to the counter passes
    # by tools/collect_profiles.sh): the cross-check of the one-by-one figure below
    profiled = None
    if traffic is not None:
        spath = tpath.replace("_traffic.json", "_bench_kernel_stats.csv")
        if os.path.exists(spath):
            import csv
            import re
            pat = re.compile(r"hrp::(" + "|".join(fam_kernels) + r")[<(]")
            steps_seen = fam_ns = fam_calls = 0
            with open(spath) as fh:
                for row in csv.DictReader(fh):
                    if "softargmax_bwd_kernel" in row["Name"]:
                        steps_seen += int(row["Calls"])
                    # (the tails' backward forms are BatchNorm-backward launches, as launch_descs attributes them; the fp32 / fp32x3
                    # instantiations in the trace belong to the run's pixel-error passes, not to the bf16 step)
                    if (pat.search(row["Name"]) and not re.search(r"conv_pw_tail_kernel<\d+, [34]>", row["Name"])
                            and "<float" not in row["Name"] and "f32x3_t" not in row["Name"]):
                        fam_ns += int(row["TotalDurationNs"])
                        fam_calls += int(row["Calls"])
            if steps_seen and fam_calls:
                pms = fam_ns / steps_seen * 1e-6
                profiled = {"family_ms_per_step": round(pms, 3), "kernel_launches_per_step": round(fam_calls / steps_seen, 1),
                            "achieved": round(dom[1][3] / (pms * 1e-3) / 1e9, 2), "frac": round(dom[1][3] / (pms * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
                            "source": "profiles/" + os.path.basename(spath) + ": rocprofv3 --kernel-trace --stats of bench.py (graph replays, "
                                      "both trunk lanes running) on the same library sources; per step = per soft-argmax backward launch"}
    roofline = {"kernel": dom[0], "bound": "hbm" if hbm_bound else "mfma",
                "achieved": round(ach_gb if hbm_bound else ach_tf, 2), "peak": PEAK_HBM_GBS if hbm_bound else peak,
                "unit": "GB/s" if hbm_bound else "TFLOP/s",
                "frac": round((ach_gb / PEAK_HBM_GBS) if hbm_bound else (ach_tf / peak), 4),
                "traffic": traffic, "traffic_source": traffic_source, "launches": dom[1][0],
                "avg_launch_us": round(dom[1][1] / dom[1][0] * 1e3, 2),
                "algorithmic_bytes_per_launch": round(dom[1][3] / dom[1][0]),
                "bytes_incl_fused_operands_per_launch": round(dom[1][4] / dom[1][0]),
                "achieved_incl_fused_operands": round(dom[1][4] / (dom[1][1] * 1e-3) / 1e9, 2), "flop_per_byte": round(intensity, 1),
                "mfma_tflops": round(ach_tf, 2), "mfma_frac": round(ach_tf / peak, 4)}
    if profiled:
        roofline["profiled"] = profiled
    out["ms_per_step_without_optimizer"] = round(ms_no_opt, 3) if ms_no_opt is not None else None
    out["roofline"] = roofline
    out["kernels"] = kernels
    if a.child:     # a secondary measurement: the parent embeds this line
        out["roofline"].pop("traffic", None)
        out["roofline"].pop("traffic_source", None)
        print(json.dumps(out))
        return
    try:   # end-to-end key-point error against the reference's own eval fixture (fp32 parity path and the benchmarked bf16)
        out["max_px_err"] = keypoint_px_error(dev, [("fp32", torch.float32), ("fp32x3", "fp32x3"), ("bf16", torch.bfloat16)])
    except Exception as e:   # the parity tests are the gate; a missing fixture must not take the number down
        out["max_px_err"] = {"error": repr(e)[:200]}
    # does the benchmarked precision keep every key-point of the fixture within 0.5 px of the reference run in float64?  (bf16:
    # key-point 0, 0.13 m in front of the camera, does not - DESIGN 4; the precision that does is timed as `fp32_step` below)
    mp = out["max_px_err"] or {}
    if "bf16_by_keypoint" in mp:
        met = {"bf16": bool(max(mp["bf16_by_keypoint"]) < 0.5), "fp32": bool(mp.get("fp32_vs_fp64", 1.0) < 0.5),
               "fp32x3": bool(mp.get("fp32x3_vs_fp64", 1.0) < 0.5)}
        out["px_bar_met"] = {"bar_px": 0.5, **met, "benchmarked_dtype": a.dtype, "benchmarked_dtype_meets_bar": met.get(a.dtype)}
    # A --full run also times the metric's literal workload (ONE HRNet-W32 = DepthNet, forward + L1 + backward +
    # clip + Adam) and BASELINE.json configs[1] (the full network's eval forward, BatchNorm folded), 10 steps each, in fresh
    # processes (one training plan per process: a second plan next to the first runs ~16 % slower), while this
    # process idles on the GPU.  Each carries its own roofline entry; `value` above stays the headline.
    profiled = any(k.startswith(("ROCP_", "ROCPROF")) for k in os.environ) or "rocprofiler" in os.environ.get("LD_PRELOAD", "")
    if world == 1 and not a.no_extra and not profiled and not hrnet and not fwd_only and not h2d and B == 64 and a.dtype == "bf16":
        import subprocess
        # "fp32_step": the SAME step with fp32 trunks - the precision that meets the north star's pixel tolerance on every
        # key-point (max_px_err.fp32); its fraction is of the fp32 matrix peak (157 TFLOP/s), 5 steps
        for key, extra in (("hrnet_step", ["--workload", "hrnet"]), ("forward_only", ["--forward-only"]),
                           ("fp32_step", ["--dtype", "fp32", "--steps", "5", "--warmup", "2"]),
                           ("fp32x3_step", ["--dtype", "fp32x3", "--steps", "5", "--warmup", "2"]),
                           # the pixel bar is a property of the OUTPUTS: configs[1] in the cheapest mode that meets it
                           ("forward_only_fp32x3", ["--forward-only", "--dtype", "fp32x3"])):
            r = None
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--full", "--child", "--no-cpu-baseline", "--steps", "10",
                                    "--warmup", "3"] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240)
                c = json.loads(r.stdout.strip().splitlines()[-1])
                out[key] = {k: c[k] for k in ("value", "unit", "ms_per_step", "steps", "warmup", "step_model_tflops",
                                              "step_frac_of_mfma_peak", "roofline") if k in c}
                out[key]["workload"] = c["config"]["workload"]
                if key == "fp32_step":
                    out[key]["dtype"] = "fp32"
                    out[key]["step_frac_of_f32_mfma_peak"] = out[key].pop("step_frac_of_mfma_peak", None)
                if key in ("fp32x3_step", "forward_only_fp32x3"):      # fp32 tensors, 3 x bf16 products: the cheapest measured mode under the pixel bar
                    out[key]["dtype"] = "fp32x3"
                    out[key]["step_frac_of_a_third_of_bf16_mfma_peak"] = out[key].pop("step_frac_of_mfma_peak", None)
            except Exception as e:
                out[key] = {"value": None, "error": repr(e)[:200], "stderr_tail": (r.stderr[-400:] if r is not None and r.stderr else None)}
    if not a.no_cpu_baseline:
        # separate process (own thread pool, hard time limit): the baseline must never take the GPU number
        # down with it
        import subprocess
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-only", "--cpu-batch",
                                str(a.cpu_batch), "--workload", a.workload] + (["--forward-only"] if fwd_only else []),
                               stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=240)
            out["cpu_baseline"] = json.loads(r.stdout.strip().splitlines()[-1])
        except Exception as e:
            out["cpu_baseline"] = {"value": None, "unit": "images/sec", "error": repr(e)[:200]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
