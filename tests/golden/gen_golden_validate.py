"""Generate tests/golden/golden_validate.npz and golden_validate_quat.npz: the reference's own ``validate`` (lib/core/function.py:330-417)
run on CPU over a three-batch loader with a stand-in model.

Run by hand where the reference tree exists:  ``python tests/golden/gen_golden_validate.py``

What runs is the reference's code: ``validate`` -> ``farward_loss(train=False)`` -> its real ``lib.utils.metrics`` (``compute_metrics_batch`` in
both call forms, ``summary_add_pck``) and ``compute_geodesic_distance_from_two_matrices``.  Shells, as in gen_golden.py: cv2 / kornia /
BPnP (not on the synthetic path), seaborn / matplotlib (curve drawing only), ``lib.utils.utils.cast`` (the reference's ``obj.to(device)``),
a mean meter standing in for torchnet's AverageValueMeter (sum of the added values / their number, in fp64), tqdm as a pass-through
when it is absent, and a ``writer`` that records ``(tag, value)``.

The model is a stub ``nn.Module`` whose forward returns seeded predictions near the ground truth, one error regime per batch
(sigma 0.002 / 0.02 / 0.2, as gen_golden.gen_metrics) so that the AUC curves are not flat; real synthetic-weight HRNets put every
error above 0.1 m and make ADD-AUC identically 0.

The loader is a list of three batches of 4, 4 and 3 samples (the unequal last batch pins the unweighted meter means and the
accumulator offsets).  640 x 480 original frames with DREAM-like intrinsics; the poses are drawn until every key-point of every
image is in frame, then batch 0 image 1 is redrawn until one to three key-points leave the frame and batch 1 image 2 is moved 3 m
sideways so that all of them do (its image_dis2d_avg is the reference's 0 / 0 = NaN).  Every key-point stays in frame in at least one
image of each batch, so the per-key-point meters are finite; the generator asserts that every recorded scalar is finite and that the
NaN sits exactly there.  ``valid_mask_crop`` has three zeros.

Keys: ``sizes`` [3]; per batch i ``b{i}:<field>`` for q, R, t, K (crop intrinsics), K_original, bbox, kp3d, kp2d, kp2d_original,
mask; ``b{i}:pred:<name>`` (the stub's 8 outputs); ``b{i}:loss``, ``b{i}:term:<name>``, ``b{i}:metric:<name>`` (what farward_loss returned);
``scalar:<tag>`` (everything validate logged); ``summary_rel:<key>`` (summary_add_pck of error3d_relative with image_dis2d_avg,
scripts/test.py:226-235); ``mean_depth_error``, ``relative_depth_error`` (:240-242); ``auc`` (validate's return value); ``rotation_dim``.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

rh.setup()
import torch  # noqa: E402

from lib.dataset.const import JOINT_BOUNDS, JOINT_NAMES  # noqa: E402
from lib.utils.geometries import rotmat_to_quat, rotmat_to_rot6d  # noqa: E402
from lib.utils.transforms import point_projection_from_3d_tensor  # noqa: E402
from lib.utils.urdf_robot import URDFRobot  # noqa: E402

NAMES8 = ["pose", "rot", "trans", "root_uv", "depth", "uvd", "xyz_int", "xyz_fk"]
ROOT = 3


class MeanMeter:
    """torchnet.meter.AverageValueMeter as validate uses it: add(value), .mean = sum / n."""

    def __init__(self):
        self.sum, self.n = 0.0, 0

    def add(self, value, n=1):
        self.sum += float(value)
        self.n += n

    @property
    def mean(self):
        return self.sum / self.n if self.n else float("nan")


class Recorder:
    def __init__(self):
        self.scalars = {}

    def add_scalar(self, tag, value, epoch):
        assert tag not in self.scalars, tag
        self.scalars[tag] = float(value)


def import_reference_function():
    for name in ("seaborn", "matplotlib", "matplotlib.pyplot"):
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                sys.modules[name] = types.ModuleType(name)
    bp = types.ModuleType("lib.utils.BPnP")
    bp.BPnP_m3d = None
    sys.modules["lib.utils.BPnP"] = bp
    ut = types.ModuleType("lib.utils.utils")
    ut.cast = lambda obj, device, dtype=None: obj.to(device)
    sys.modules["lib.utils.utils"] = ut
    tn, tm = types.ModuleType("torchnet"), types.ModuleType("torchnet.meter")
    tm.AverageValueMeter = MeanMeter
    tn.meter = tm
    sys.modules["torchnet"], sys.modules["torchnet.meter"] = tn, tm
    try:
        import tqdm  # noqa: F401
    except ImportError:
        tq = types.ModuleType("tqdm")
        tq.tqdm = lambda it, **kw: it
        sys.modules["tqdm"] = tq
    from lib.core import function
    return function


def random_rotation(g):
    q = g.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float32)


K_ORIGINAL = np.array([[615.0, 0, 320], [0, 615.0, 240], [0, 0, 1]], np.float32)


def in_frame(uv):
    return (uv[:, 0] <= 640.0) & (uv[:, 0] >= 0) & (uv[:, 1] <= 480.0) & (uv[:, 1] >= 0)


def draw_sample(g, robot, want):
    """One (q, R, t) whose number of out-of-frame key-points satisfies want(n_out)."""
    b = np.array(JOINT_BOUNDS["panda"], dtype=np.float64)
    while True:
        q = (b[:, 0] + (b[:, 1] - b[:, 0]) * g.random(8)).astype(np.float32)
        R = random_rotation(g)
        t = np.array([g.uniform(-.5, .5), g.uniform(-.4, .4), g.uniform(.8, 2.0)], np.float32)
        with torch.no_grad():
            kp3d = robot.get_keypoints(torch.tensor(q)[None], rotmat_to_rot6d(torch.tensor(R)[None]), torch.tensor(t)[None])
            uv = point_projection_from_3d_tensor(torch.tensor(K_ORIGINAL)[None], kp3d)[0].numpy()
        if kp3d[0, :, 2].min() > 0.3 and want(int((~in_frame(uv)).sum())):
            return q, R, t


def make_batch(g, robot, B, index):
    rows = []
    for n in range(B):
        if index == 0 and n == 1:
            rows.append(draw_sample(g, robot, lambda k: 1 <= k <= 3))       # some key-points outside the frame
        else:
            rows.append(draw_sample(g, robot, lambda k: k == 0))
    q, R, t = [np.stack(c) for c in zip(*rows)]
    if index == 1:
        t[2, 0] += 3.0                                                       # every key-point of this image outside the frame
    TCO = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    TCO[:, :3, :3], TCO[:, :3, 3] = R, t
    s = g.uniform(0.8, 2.5, B).astype(np.float32)
    K = np.zeros((B, 3, 3), np.float32)
    K[:, 0, 0] = K[:, 1, 1] = 320 * s
    K[:, 0, 2] = K[:, 1, 2] = 128
    K[:, 2, 2] = 1
    side = g.uniform(80, 240, B).astype(np.float32)
    bbox = np.stack([128 - side / 2, 128 - side / 2 * 0.8, 128 + side / 2, 128 + side / 2 * 0.8], 1).astype(np.float32)
    K_original = np.tile(K_ORIGINAL, (B, 1, 1))
    with torch.no_grad():
        kp3d = robot.get_keypoints(torch.tensor(q), rotmat_to_rot6d(torch.tensor(R)), torch.tensor(t))
        kp2d = point_projection_from_3d_tensor(torch.tensor(K), kp3d)
        kp2d_original = point_projection_from_3d_tensor(torch.tensor(K_original), kp3d)
    mask = np.ones((B, 7), np.float32)
    mask[0, 5] = 0.0
    if index == 2:
        mask[1, 3] = mask[2, 0] = 0.0                                        # the root key-point of one image, and one more
    jointpose = {n: [float(q[i, j]) for i in range(B)] for j, n in enumerate(JOINT_NAMES["panda"])}
    img = torch.zeros(B, 3, 8, 8)                                            # the stub model does not look at the images
    batch = {
        "root": {"images": img, "K": torch.tensor(K), "bbox_strict_bounded": torch.tensor(bbox), "bbox_gt2d_extended": torch.tensor(bbox)},
        "other": {"images": img.clone(), "K": torch.tensor(K), "keypoints_2d": kp2d, "valid_mask_crop": torch.tensor(mask),
                  "keypoints_3d": kp3d},
        "TCO": torch.tensor(TCO), "K_original": torch.tensor(K_original), "jointpose": jointpose,
        "keypoints_2d_original": kp2d_original, "valid_mask": torch.tensor(mask),
    }
    small = dict(q=q, R=R, t=t, K=K, K_original=K_original, bbox=bbox, kp3d=kp3d.numpy(), kp2d=kp2d.numpy(),
                 kp2d_original=kp2d_original.numpy(), mask=mask)
    return batch, small


class Stub(torch.nn.Module):
    """forward returns the prescribed 8-tuple of the batch it is called for (in loader order)."""

    def __init__(self, per_batch):
        super().__init__()
        self.per_batch, self.calls = per_batch, 0
        self.w = torch.nn.Parameter(torch.zeros(1))

    def forward(self, reg_images, root_images, k_values, K=None):
        out = self.per_batch[self.calls % len(self.per_batch)]
        self.calls += 1
        return tuple(t.clone() for t in out)


def generate(rotation_dim, path):
    function = import_reference_function()
    robot = URDFRobot("panda")
    g = np.random.Generator(np.random.PCG64(4242))
    tg = torch.Generator().manual_seed(4243)
    r = lambda *sh: torch.randn(*sh, generator=tg)          # noqa: E731
    sizes = [4, 4, 3]
    args = rh._AttrDict(rh.default_args(rotation_dim=rotation_dim))
    args.update(urdf_robot_name="panda", use_origin_bbox=False, use_extended_bbox=True,
                train_ds_names="dream/synthetic/panda_synth_train_dr", use_joint_valid_mask=False,
                known_joint=False, joint_individual_weights=None, image_size=256.0, fix_mask=False,
                pose_loss_func="mse", rot_loss_func="mse", trans_loss_func="l2norm",
                depth_loss_func="l1", uv_loss_func="l2norm", kp2d_loss_func="l2norm",
                kp3d_loss_func="l2norm", kp2d_int_loss_func="l2norm", kp3d_int_loss_func="l2norm",
                align_3d_loss_func="l2norm", pose_loss_weight=1.0, rot_loss_weight=1.0,
                trans_loss_weight=1.0, depth_loss_weight=10.0, uv_loss_weight=1.0,
                kp2d_loss_weight=10.0, kp3d_loss_weight=10.0, kp2d_int_loss_weight=10.0,
                kp3d_int_loss_weight=10.0, align_3d_loss_weight=0.0)
    out = {"sizes": np.array(sizes), "rotation_dim": np.int32(rotation_dim)}
    loader, preds = [], []
    for i, B in enumerate(sizes):
        batch, small = make_batch(g, robot, B, i)
        loader.append(batch)
        out.update({f"b{i}:{k}": v for k, v in small.items()})
        q, R, t = torch.tensor(small["q"]), torch.tensor(small["R"]), torch.tensor(small["t"])
        kp3d, kp2d = torch.tensor(small["kp3d"]), torch.tensor(small["kp2d"])
        gt_rot = rotmat_to_quat(R) if rotation_dim == 4 else rotmat_to_rot6d(R)
        with torch.no_grad():
            root_rot = robot.get_rotation_at_specific_root(q, gt_rot, t, root=ROOT)
        sc = [0.002, 0.02, 0.2][i]
        p = [q + sc * r(B, 8), root_rot + sc * r(B, rotation_dim), kp3d[:, ROOT] + 0.5 * sc * r(B, 3),
             kp2d[:, ROOT] + 50.0 * sc * r(B, 2), kp3d[:, ROOT, 2:3] + 0.5 * sc * r(B, 1), r(B, 7, 3),
             kp3d + 0.3 * sc * r(B, 7, 3), kp3d + 0.3 * sc * r(B, 7, 3)]
        preds.append(p)
        out.update({f"b{i}:pred:{n}": v.numpy() for n, v in zip(NAMES8, p)})

    # record what farward_loss returns per batch, and the ninth output (error3d_relative) it drops, without touching its code
    per_batch, extra = [], {"rel": [], "dis2d": [], "depth": [], "relz": []}
    plain_fl, plain_cm = function.farward_loss, function.compute_metrics_batch

    def recording_cm(*a, **k):
        res = plain_cm(*a, **k)
        if k.get("pred_joint") is not None:
            extra["rel"].extend(list(res[8]))
            extra["dis2d"].extend(list(res[1]))
            extra["depth"].extend(list(res[6]))
            extra["relz"].extend(list(res[7]))
        return res

    def recording_fl(*a, **k):
        res = plain_fl(*a, **k)
        per_batch.append(res)
        return res
    function.compute_metrics_batch, function.farward_loss = recording_cm, recording_fl
    model, writer = Stub(preds), Recorder()
    with np.errstate(invalid="ignore", divide="ignore"):
        auc = function.validate(args, 7, "dr", loader, model, robot, writer, "cpu", [0])
        summary_rel = plain_summary(function)({"dis3d": extra["rel"], "dis2d": extra["dis2d"]})
    function.compute_metrics_batch, function.farward_loss = plain_cm, plain_fl
    assert len(per_batch) == 3 and model.training
    for i, (loss, terms, metrics) in enumerate(per_batch):
        out[f"b{i}:loss"] = np.array(loss.item())
        for k, v in terms.items():
            out[f"b{i}:term:{k}"] = np.array(v.item())
        for k, v in metrics.items():
            out[f"b{i}:metric:{k}"] = np.asarray(v.detach().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float64)
    for tag, v in writer.scalars.items():
        out["scalar:" + tag] = np.float64(v)
    for k, v in summary_rel.items():
        out["summary_rel:" + k] = np.float64(v)
    out["mean_depth_error"] = np.float64(np.mean(extra["depth"]))
    out["relative_depth_error"] = np.float64(np.mean(extra["relz"]))
    out["auc"] = np.float64(auc)
    # the properties the fixture is built for
    bad = [t for t, v in writer.scalars.items() if not np.isfinite(v)]
    assert not bad, bad
    for i in range(3):
        nan2d = np.isnan(out[f"b{i}:metric:image_dis2d_avg"])
        assert nan2d.tolist() == ([False, False, True, False] if i == 1 else [False] * sizes[i]), (i, nan2d)
        assert np.array_equal(nan2d, np.isnan(out[f"b{i}:metric:image_dis2d_avg_int"]))
        assert all(np.isfinite(out[f"b{i}:metric:{k}"]).all() for k in per_batch[i][2] if "dis2d_avg" not in k or "batch" in k)
    n_out = (~in_frame(out["b0:kp2d_original"][1])).sum()
    assert 1 <= n_out <= 3 and not in_frame(out["b1:kp2d_original"][2]).any()
    assert 0.0 < auc < 1.0 and out["scalar:Val/AUC_ADD_dr"] == auc
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes): rotation_dim {rotation_dim}, {len(writer.scalars)} scalars, ADD-AUC {auc:.6f}, "
          f"PCK-AUC {writer.scalars['Val/AUC_PCK_dr']:.6f}, rot_diff {writer.scalars['Val/rot_diff_dr']:.4f}, "
          f"relative ADD-AUC {summary_rel['ADD/AUC']:.6f}")


def plain_summary(function):
    return function.summary_add_pck


if __name__ == "__main__":
    torch.set_num_threads(8)
    generate(6, os.path.join(HERE, "golden_validate.npz"))
    generate(4, os.path.join(HERE, "golden_validate_quat.npz"))
