"""Generate tests/golden/golden_depthnet_step.npz: the reference's own DepthNet trainer (scripts/train_depthnet.py) run on CPU for one
epoch - three training steps, then its validation of the ``dr`` and ``photo`` sets - once per loss configuration.

Run by hand where the reference tree exists:  ``python tests/golden/gen_golden_depthnet_step.py``

The step (``farward_loss``, train_depthnet.py:152-273) and the validation (``validate``, :276-303) are functions nested inside the epoch
loop of ``train_depthnet(args)`` and cannot be imported, so what runs is ``train_depthnet(args)`` itself, with stand-ins for what
surrounds the step:
  * ``DreamDataset`` / ``DataLoader`` / ``MultiEpochDataLoader`` / ``PartialSampler``: list loaders (a data set is its list of batches);
  * ``create_logger``: a temporary folder (``torch.save`` writes the checkpoint there; its ``loss`` entry is ``validate("dr")``'s return
    value) and a writer that records ``(tag, value)``;
  * ``get_rootnet``: a stub module whose forward returns seeded predictions near the ground truth plus a learnable offset (zero at
    the first step, moved by Adam afterwards), records the ``k_values`` it is called with, and keeps each training output with
    ``retain_grad()`` so that d loss / d pred is there after the run;
  * torchnet's AverageValueMeter: a mean meter (sum of the added values / their number, in fp64, as gen_golden_validate.py) that also
    keeps every value added - the per-batch losses; ``defaultdict``: one that is remembered - ``validate``'s per-image error lists;
  * ``cast``, ``set_random_seed``, ``get_scheduler``, tqdm: pass-throughs.
The robot is kuka: only ``dr`` and ``photo`` are validated for it (:336-339), so no real-camera loader is needed.  Both sets are the
same list here (the generator asserts that their scalars agree); the per-batch validation keys are those of the ``dr`` pass.

Loaders: train and validation lists of three batches of 4, 4 and 3 samples (the unequal last batch pins the unweighted meter mean
and the accumulator offsets).  Poses are drawn until the root key-point (3) and the base lie between 0.5 and 2 m.  ``valid_mask_crop``
has a zero in the root column in two batches of each list.  One intrinsic matrix carries a negative fx (pins the ``abs`` of :212).  The
batches have no ``"other"`` view: the reference's step never reads it.  In the xy runs, training batch 0 sample 1 predicts x exactly
(pins sign(0) = 0 of the l1 gradient; the masked rows pin it as well).

Runs (``RUNS``): l1 plain (the shipped choice), mse plain (root 0, strict bbox), xy branch with l1 (original bbox and intrinsics), xy
branch with mse, multi_kp [1, 3, 5] root 3 with l1, the same with mse.

Keys: ``sizes`` [3]; ``runs`` is implied by the key names.  Inputs per batch, ``{train|val}{i}:<field>`` for K, K_original, bbox_strict,
bbox_extended, bbox_original, kp3d, mask (valid_mask_crop [B, 8]), TCO.  Per run and batch ``<run>:{train|val}{i}:<field>``: k_values, pred,
loss, and dpred (training) or error_depth / error_x / error_y (validation).  Per run: ``<run>:scalar:<tag>`` for everything the trainer
logged, ``<run>:validate_return`` (the checkpoint's ``loss``), ``<run>:opt:<name>`` for the options that differ between runs.
Numeric arrays only."""
import collections
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

rh.setup()
import torch  # noqa: E402

from lib.dataset.const import JOINT_BOUNDS, JOINT_NAMES  # noqa: E402
from lib.utils.geometries import rotmat_to_rot6d  # noqa: E402

SIZES = [4, 4, 3]
NKP = 8
RUNS = {
    "l1": dict(depth_loss_func="l1"),
    "mse": dict(depth_loss_func="mse", reference_keypoint_id=0, use_extended_bbox=False),
    "xy_l1": dict(depth_loss_func="l1", use_rootnet_xy_branch=True, xy_loss_func="l1", use_extended_bbox=False, use_origin_bbox=True),
    "xy_mse": dict(depth_loss_func="l1", use_rootnet_xy_branch=True, xy_loss_func="mse"),
    "mkp_l1": dict(depth_loss_func="l1", multi_kp=True, kps_need_depth=[1, 3, 5]),
    "mkp_mse": dict(depth_loss_func="mse", multi_kp=True, kps_need_depth=[1, 3, 5]),
}
OPT_KEYS = ("reference_keypoint_id", "use_extended_bbox", "use_origin_bbox")


class MeanMeter:
    """torchnet.meter.AverageValueMeter as the trainer uses it: add(value), .mean = sum / n, reset(); keeps what was added."""
    created = []

    def __init__(self):
        self.sum, self.n, self.history = 0.0, 0, []
        MeanMeter.created.append(self)

    def add(self, value, n=1):
        self.history.append(np.asarray(value).copy())
        self.sum += float(value)
        self.n += n

    def reset(self):
        self.sum, self.n = 0.0, 0

    @property
    def mean(self):
        return self.sum / self.n if self.n else float("nan")


class RememberedDict(collections.defaultdict):
    created = []

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        RememberedDict.created.append(self)


class Recorder:
    def __init__(self):
        self.scalars = {}

    def add_scalar(self, tag, value, step):
        self.scalars.setdefault(tag, []).append(float(value))

    def flush(self):
        pass


class ListDataset:
    def __init__(self, batches):
        self.batches = batches


class Stub(torch.nn.Module):
    """forward returns base[call] + offset: the prescribed prediction of the batch it is called for (in loader order)."""

    def __init__(self, bases):
        super().__init__()
        self.bases, self.calls, self.outputs, self.k_values = bases, 0, [], []
        self.offset = torch.nn.Parameter(torch.zeros(1))

    def forward(self, images, k_values):
        assert images.dtype == torch.float32 and float(images.max()) <= 1.0
        out = self.bases[self.calls] + self.offset
        self.calls += 1
        if torch.is_grad_enabled():
            out.retain_grad()
        self.outputs.append(out)
        self.k_values.append(k_values.detach().clone())
        return out


def import_trainer():
    """scripts/train_depthnet.py as a module, with shells for the modules it imports that carry none of the step's arithmetic."""
    def shell(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m
    shell("lib.dataset.dream", DreamDataset=None)
    shell("lib.dataset.multiepoch_dataloader", MultiEpochDataLoader=None)
    shell("lib.dataset.samplers", PartialSampler=None)
    shell("lib.utils.utils", cast=lambda obj, device, dtype=None: obj.to(device), set_random_seed=lambda s: torch.manual_seed(s),
          create_logger=None, get_scheduler=lambda *a, **k: None)
    tm = shell("torchnet.meter", AverageValueMeter=MeanMeter)
    shell("torchnet", meter=tm)
    try:
        import tqdm  # noqa: F401
    except ImportError:
        shell("tqdm", tqdm=lambda it, **kw: it)
    path = os.path.join(rh.REFERENCE_ROOT, "scripts", "train_depthnet.py")
    spec = importlib.util.spec_from_file_location("ref_train_depthnet", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def random_rotation(g):
    q = g.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float32)


def draw_sample(g, robot):
    b = np.array(JOINT_BOUNDS["kuka"], dtype=np.float64)
    while True:
        q = (b[:, 0] + (b[:, 1] - b[:, 0]) * g.random(7)).astype(np.float32)
        R = random_rotation(g)
        t = np.array([g.uniform(-.5, .5), g.uniform(-.4, .4), g.uniform(.6, 1.9)], np.float32)
        with torch.no_grad():
            kp3d = robot.get_keypoints(torch.tensor(q)[None], rotmat_to_rot6d(torch.tensor(R)[None]), torch.tensor(t)[None])[0]
        if kp3d[:, 2].min() > 0.3 and 0.5 < float(kp3d[3, 2]) < 2.0:
            return q, R, t, kp3d.numpy()


def make_batch(g, robot, B, index, negative_fx):
    q, R, t, kp3d = [np.stack(c) for c in zip(*[draw_sample(g, robot) for _ in range(B)])]
    TCO = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    TCO[:, :3, :3], TCO[:, :3, 3] = R, t
    s = g.uniform(0.8, 2.5, B).astype(np.float32)
    K = np.zeros((B, 3, 3), np.float32)
    K[:, 0, 0], K[:, 1, 1] = 320 * s, 330 * s
    K[:, 0, 2] = K[:, 1, 2] = 128
    K[:, 2, 2] = 1
    if negative_fx:
        K[1, 0, 0] = -K[1, 0, 0]
    K_original = np.tile(np.array([[615.0, 0, 320], [0, 617.0, 240], [0, 0, 1]], np.float32), (B, 1, 1))

    def boxes(lo, hi):
        side = g.uniform(lo, hi, B).astype(np.float32)
        return np.stack([128 - side / 2, 128 - side / 2 * 0.8, 128 + side / 2, 128 + side / 2 * 0.8], 1).astype(np.float32)
    bbox_strict, bbox_extended, bbox_original = boxes(80, 200), boxes(100, 240), boxes(150, 400)
    mask = np.ones((B, NKP), np.float32)
    mask[0, 5] = 0.0
    if index in (0, 2):
        mask[index, 3] = 0.0                                     # the root key-point of one image in two batches
        mask[index, 0] = 0.0                                     # and the base (the root of the run with reference_keypoint_id 0)
    jointpose = {n: [float(q[i, j]) for i in range(B)] for j, n in enumerate(JOINT_NAMES["kuka"])}
    images = torch.tensor(g.integers(0, 256, (B, 3, 8, 8)), dtype=torch.uint8)      # the stub model does not look at the images
    batch = {
        "root": {"images": images, "K": torch.tensor(K), "bbox_strict_bounded": torch.tensor(bbox_strict),
                 "bbox_gt2d_extended": torch.tensor(bbox_extended), "keypoints_3d": torch.tensor(kp3d),
                 "valid_mask_crop": torch.tensor(mask)},
        "TCO": torch.tensor(TCO), "K_original": torch.tensor(K_original), "bbox_strict_bounded_original": torch.tensor(bbox_original),
        "jointpose": jointpose, "valid_mask": torch.tensor(mask),
    }
    small = dict(K=K, K_original=K_original, bbox_strict=bbox_strict, bbox_extended=bbox_extended, bbox_original=bbox_original,
                 kp3d=kp3d, mask=mask, TCO=TCO)
    return batch, small


def make_bases(opts, smalls, tg, exact_x):
    """The stub's prescribed outputs for a list of batches: depth in mm, sigma 30 mm; x, y in metres, sigma 0.03 m."""
    ref = opts.get("reference_keypoint_id", 3)
    bases = []
    for i, s in enumerate(smalls):
        kp3d, t = torch.tensor(s["kp3d"]), torch.tensor(s["TCO"][:, :3, 3])
        root_trans = t if ref == 0 else kp3d[:, ref]
        B = kp3d.shape[0]
        if opts.get("multi_kp"):
            base = kp3d[:, opts["kps_need_depth"], 2] * 1000.0 + 30.0 * torch.randn(B, 3, generator=tg)
        elif opts.get("use_rootnet_xy_branch"):
            base = torch.cat([root_trans[:, 0:2] + 0.03 * torch.randn(B, 2, generator=tg),
                              root_trans[:, 2:3] * 1000.0 + 30.0 * torch.randn(B, 1, generator=tg)], 1)
            if exact_x and i == 0:
                base[1, 0] = root_trans[1, 0]
        else:
            base = root_trans[:, 2:3] * 1000.0 + 30.0 * torch.randn(B, 1, generator=tg)
        bases.append(base.float())
    return bases


def run(td, name, opts, robot_name, train, val, out, seed):
    """One ``train_depthnet(args)`` of the reference; everything it computed goes to ``out`` under ``<name>:``."""
    tg = torch.Generator().manual_seed(seed)
    bases = make_bases(opts, [s for _, s in train], tg, True) + 2 * make_bases(opts, [s for _, s in val], tg, False)
    model, writer = Stub(bases), Recorder()
    folder = tempfile.mkdtemp(prefix="hrp_depthnet_")
    sets = {"train": [b for b, _ in train], "test_dr": [b for b, _ in val], "test_photo": [b for b, _ in val]}
    td.DreamDataset = lambda ds_name, **kw: ListDataset(next(v for k, v in sets.items() if k in ds_name))
    td.DataLoader = lambda ds, **kw: ds.batches
    td.MultiEpochDataLoader = lambda loader: loader
    td.PartialSampler = lambda ds, epoch_size=None: None
    td.create_logger = lambda args: (folder, folder, folder, writer)
    td.get_rootnet = lambda *a, **k: model
    td.defaultdict = RememberedDict
    td.tqdm = lambda it, **kw: it
    MeanMeter.created, RememberedDict.created = [], []
    args = rh._AttrDict(urdf_robot_name=robot_name, device_id=[0], no_cuda=True, train_ds_names="dream/synthetic/kuka_synth_train_dr",
                        jitter=False, other_aug=False, occlusion=False, rootnet_flip=False, occlu_p=0.0, padding=False,
                        extend_ratio=[0.2, 0.13], epoch_size=11, resample=False, batch_size=4, n_dataloader_workers=0,
                        backbone_name="stub", use_rootnet_xy_branch=False, add_fc=False, use_offset=False, lr=1e-4, weight_decay=0.0,
                        resume_run=False, n_epochs=0, use_schedule=False, clip_gradient=None, use_origin_bbox=False,
                        use_extended_bbox=True, reference_keypoint_id=3, multi_kp=False, kps_need_depth=None,
                        bbox_3d_shape=[1300, 1300, 1300], depth_loss_func="l1", xy_loss_func="mse")
    args.update(opts)
    td.train_depthnet(args)
    torch.autograd.set_detect_anomaly(False)
    n = len(SIZES)
    assert model.calls == 3 * n and model.training
    train_meter, dr_meter, photo_meter = MeanMeter.created[0], MeanMeter.created[1], MeanMeter.created[3]
    dr_lists, photo_lists = RememberedDict.created
    assert len(train_meter.history) == len(dr_meter.history) == len(photo_meter.history) == n
    off = 0
    for i, B in enumerate(SIZES):
        for part, call, meter in (("train", i, train_meter), ("val", n + i, dr_meter)):
            key = f"{name}:{part}{i}:"
            o = model.outputs[call]
            out[key + "k_values"] = model.k_values[call].numpy()
            out[key + "pred"] = o.detach().numpy().copy()
            out[key + "loss"] = np.asarray(meter.history[i], dtype=np.float32)
            if part == "train":
                out[key + "dpred"] = o.grad.numpy().copy()
            else:
                for field, lst in (("error_depth", "deptherror"), ("error_x", "xerror"), ("error_y", "yerror")):
                    out[key + field] = np.asarray(dr_lists[lst][off:off + B], dtype=np.float32).reshape(B)
        off += B
    for tag, values in writer.scalars.items():
        if tag.startswith("LR/"):
            continue
        assert len(values) == 1, (tag, values)
        out[f"{name}:scalar:{tag}"] = np.float64(values[0])
    for tag in ("rootz_loss", "mean_depth_error", "mean_x_error", "mean_y_error"):      # same list, same model: same scalars
        assert writer.scalars[f"Val/{tag}_dr"] == writer.scalars[f"Val/{tag}_photo"], tag
    ckpt = torch.load(os.path.join(folder, "curr_best_root_depth_model.pk"), weights_only=False)
    out[f"{name}:validate_return"] = np.float64(ckpt["loss"])
    assert out[f"{name}:validate_return"] == out[f"{name}:scalar:Val/mean_depth_error_dr"]
    for k in OPT_KEYS:
        out[f"{name}:opt:{k}"] = np.int32(args[k])
    # the properties the fixture is built for
    assert all(np.isfinite(v).all() for k, v in out.items() if k.startswith(name + ":"))
    if opts.get("use_rootnet_xy_branch"):
        ref = args.reference_keypoint_id
        assert out[f"{name}:train0:pred"][1, 0] == train[0][1]["kp3d"][1, ref, 0] and train[0][1]["mask"][1, ref] == 1.0
        assert out[f"{name}:train0:dpred"][1, 0] == 0.0
        assert out[f"{name}:val1:error_x"].min() > 0
    else:
        assert all(not out[f"{name}:val{i}:error_x"].any() and not out[f"{name}:val{i}:error_y"].any() for i in range(n))
    print(f"{name}: Train/loss {out[name + ':scalar:Train/loss']:.6f}, rootz_loss {out[name + ':scalar:Val/rootz_loss_dr']:.6f}, "
          f"mean depth error {ckpt['loss']:.6f}")


def generate(path):
    td = import_trainer()
    from lib.utils.urdf_robot import URDFRobot
    robot = URDFRobot("kuka")
    assert len(robot.link_names) == NKP
    g = np.random.Generator(np.random.PCG64(5151))
    out = {"sizes": np.array(SIZES)}
    lists = {}
    for part in ("train", "val"):
        lists[part] = [make_batch(g, robot, B, i, negative_fx=(part, i) in (("train", 1), ("val", 2))) for i, B in enumerate(SIZES)]
        for i, (_, small) in enumerate(lists[part]):
            out.update({f"{part}{i}:{k}": v for k, v in small.items()})
            assert 0.5 < small["kp3d"][:, 3, 2].min() and small["kp3d"][:, 3, 2].max() < 2.0
            assert 0.5 < small["TCO"][:, 2, 3].min() and small["TCO"][:, 2, 3].max() < 2.0
        zeros = [int((small["mask"][:, 3] == 0).sum()) for _, small in lists[part]]
        assert zeros == [1, 0, 1], zeros
    for r, (name, opts) in enumerate(RUNS.items()):
        run(td, name, opts, "kuka", lists["train"], lists["val"], out, 6000 + r)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1 << 20, size
    assert all(v.dtype.kind in "fi" for v in np.load(path).values())
    print(f"wrote {path} ({size} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    torch.set_num_threads(8)
    generate(os.path.join(HERE, "golden_depthnet_step.npz"))
