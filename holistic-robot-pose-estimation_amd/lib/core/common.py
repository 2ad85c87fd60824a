"""What the three trainers (lib/core/function.py, depthnet.py, sim2real.py) decide in one place: the option lookup, the upload of
a batch's pieces, ``k_values``, the growth of an epoch accumulator, the AverageValueMeter mean, the walk over a validation loader,
the step prologue the two pose trainers share and the second half of their validation scalars.  Plain functions; what differs
between the trainers stays in their modules."""
import types

import numpy as np
import torch

from hrpe_amd.lib.dataset.const import INITIAL_JOINT_ANGLE, JOINT_NAMES, JOINT_TO_KP

ADD_THRESHOLDS = [1, 5, 10, 20, 40, 60, 80, 100]                      # function.py:342-343
PCK_THRESHOLDS = [2.5, 5.0, 7.5, 10.0, 12.5, 15.0, 17.5, 20.0]


def opt(args, name, default=None):
    try:
        return getattr(args, name)
    except (AttributeError, KeyError):
        return default


def to_device(t, device, dtype=torch.float32):
    return torch.as_tensor(t).to(device=device, dtype=dtype, non_blocking=True)


def images_to_device(t, device):
    """uint8 images stay uint8 on the way to the device (4x less PCIe traffic; the model's input kernel does the ``.float() / 255.``
    while it writes the trunk's NHWC layout); float images (the reference's loaders hand over float tensors holding 0..255) are
    scaled here as the reference does."""
    t = torch.as_tensor(t)
    if t.dtype == torch.uint8:
        return t.to(device, non_blocking=True)
    return to_device(t, device) / 255.


def select_bbox_and_K(input_batch, root_view, K_root, device, use_origin_bbox, use_extended_bbox):
    """(bboxes, K) that ``k_values`` is computed from (function.py:43-48, 89-94; train_depthnet.py:165-170, 203-208): the extended
    box or the strict box of the root crop with the crop's intrinsics ``K_root``, or the strict box of the original image with its."""
    if use_extended_bbox:
        return to_device(root_view["bbox_gt2d_extended"], device), K_root
    if use_origin_bbox:
        return to_device(input_batch["bbox_strict_bounded_original"], device), to_device(input_batch["K_original"], device)
    return to_device(root_view["bbox_strict_bounded"], device), K_root


def compute_k_values(fx, fy, bboxes, real_bbox=(1000.0, 1000.0), absolute=False):
    """k = sqrt(fx*fy*1000*1000 / max(|x2-x1|, |y2-y1|)^2) in the reference's order of operations (function.py:88-98);
    ``absolute``: |fx| * |fy|, as the DepthNet trainer takes it (train_depthnet.py:202-212)."""
    area = torch.max(torch.abs(bboxes[:, 2] - bboxes[:, 0]), torch.abs(bboxes[:, 3] - bboxes[:, 1])) ** 2
    if absolute:
        fx, fy = torch.abs(fx), torch.abs(fy)
    return torch.sqrt(fx * fy * real_bbox[0] * real_bbox[1] / area).to(torch.float32)


def grown(t, axis, used, need):
    """``t`` when it holds ``need`` entries along ``axis``; otherwise a zero-filled tensor with max(need, twice as many) entries
    there and the first ``used`` copied.  The host knows ``used``, so growing an accumulator needs no synchronisation."""
    if need <= t.shape[axis]:
        return t
    shape = list(t.shape)
    shape[axis] = max(need, 2 * t.shape[axis])
    new = torch.zeros(shape, dtype=t.dtype, device=t.device)
    new.narrow(axis, 0, used).copy_(t.narrow(axis, 0, used))
    return new


def meter_mean(rows):
    """AverageValueMeter over axis 0: the sum of the added values, fp64, in the order they were added, over their number."""
    rows = np.asarray(rows, dtype=np.float64)
    acc = np.zeros(rows.shape[1:], np.float64)
    for r in rows:
        acc = acc + r
    return acc / rows.shape[0]


def loader_capacity(loader, default=1024):
    """The number of images an epoch over ``loader`` will add, where its dataset can tell; the accumulators grow past it."""
    dataset = getattr(loader, "dataset", None)
    try:
        return (len(dataset) if dataset is not None else 0) or default
    except TypeError:
        return default


def validation_batches(loader, device):
    """The batches of ``loader``; one over this project's DreamDataset (host items with ``frame`` / ``aug``) goes through
    ``DreamDataset.to_device`` first, a batch already in the reference schema is passed on as it is."""
    for sample in loader:
        if "frame" in sample and "aug" in sample:
            sample = loader.dataset.to_device(sample, device=device)
        yield sample


def pose_step_inputs(args, input_batch, model, robot, device, rotation_dim, evaluate=False):
    """The step of the two pose trainers from the batch to the weighted joint angles (function.py:25-186; train_sim2real.py:151-311):
    ``prepare_batch``, the joint valid mask, the model call, ``known_joint`` and ``joint_individual_weights``.  ``evaluate``: the two
    dictionaries ``Evaluator.add`` takes are built as well (one FK launch).  The caller has checked the options and set the modes;
    the length of ``pred`` is the caller's to check."""
    from hrpe_amd.lib.core.function import prepare_batch
    root = int(args.reference_keypoint_id)
    p = prepare_batch(input_batch, robot, device, reference_keypoint_id=root, use_origin_bbox=bool(opt(args, "use_origin_bbox", False)),
                      use_extended_bbox=bool(opt(args, "use_extended_bbox", True)),
                      synthetic="synth" in args.train_ds_names, rotation_dim=rotation_dim)                # :66
    gt = dict(p["gt"])
    gt_pose_before_mask = gt["pose"]                                                                     # :107
    if opt(args, "use_joint_valid_mask", False):                                                         # :104-114
        valid_mask = torch.as_tensor(input_batch["valid_mask"]).to(device=device, dtype=torch.float32)
        joint_valid_mask = valid_mask[:, JOINT_TO_KP[robot.robot_type]]
        assert joint_valid_mask.shape == gt["pose"].shape, (joint_valid_mask.shape, gt["pose"].shape)
        mean_joints = torch.tensor([INITIAL_JOINT_ANGLE["mean"][robot.robot_type][k] for k in JOINT_NAMES[robot.robot_type]],
                                   dtype=torch.float32, device=device).unsqueeze(0)
        gt["pose"] = gt["pose"] * joint_valid_mask + mean_joints * (1 - joint_valid_mask)
    pred = tuple(model(p["reg_images"], p["root_images"], p["k_values"], K=p["other_K"]))                # :115-120
    pred_pose, pred_rot, pred_trans = pred[0], pred[1], pred[2]
    if opt(args, "known_joint", False):                                                                  # :124-125
        pred_pose = gt["pose"].clone()
    ev_pred = ev_gt = None
    if evaluate:                                                                                         # :137-179
        with torch.no_grad():
            kp3d_fk = robot.get_keypoints_root(pred_pose.detach().float(), pred_rot.detach().float(), pred_trans.detach().float(),
                                               root=root)                                                # metrics.py:27-34
        ev_pred = dict(kp3d_fk=kp3d_fk, kp3d_int=pred[-2], joint=pred_pose, rot=pred_rot)
        # the reference's quirk, kept: rotation_diff compares pred_rot - the rotation at the ROOT key-point - with the BASE
        # rotation gt_rot, not with gt_root_rot (function.py:169-172; train_sim2real.py:298); the metrics use the unmasked joint
        # angles (:145; :272)
        ev_gt = dict(kp3d=gt["kp3d"], kp2d_original=torch.as_tensor(input_batch["keypoints_2d_original"]),
                     K_original=torch.as_tensor(input_batch["K_original"]), joint=gt_pose_before_mask, rot=gt["rot"])
    jw = opt(args, "joint_individual_weights")
    if jw is not None:                                                                                   # :182-186
        assert len(jw) == robot.dof
        w = torch.tensor(list(jw), dtype=torch.float32, device=device).reshape(1, -1)
        pred_pose, gt["pose"] = pred_pose * w, gt["pose"] * w
    return types.SimpleNamespace(p=p, gt=gt, gt_pose_before_mask=gt_pose_before_mask, pred=pred, pred_pose=pred_pose, ev_pred=ev_pred,
                                 ev_gt=ev_gt, root=root)


def log_pose_validation(add, s, nkp, dof, integral_details, integral_epoch=None):
    """The scalars the two pose trainers' validation loops share, from ``Val/mean_joint_error`` on (function.py:380-415;
    train_sim2real.py:609-623), through ``add(tag, value[, epoch])``.  ``s``: the evaluator's summary.  ``integral_details``: the
    thresholds and per-key-point distances of the integral branch are logged too (function.py does, train_sim2real.py does not).
    ``integral_epoch``: the epoch the two integral AUCs are logged at, where it is not ``add``'s own."""
    m, s_int = s["meters"], s["integral"]
    at = () if integral_epoch is None else (integral_epoch,)
    add("Val/mean_joint_error", s["mean_joint_error"])
    add("Val/AUC_ADD", s["ADD/AUC"])
    add("Val/AUC_PCK", s["PCK/AUC"])
    add("Val/AUC_ADD_integral_xyz_metrics", s_int["ADD/AUC"], *at)
    add("Val/AUC_PCK_integral_xyz_metrics", s_int["PCK/AUC"], *at)
    for th in ADD_THRESHOLDS:
        add(f"Val/ADD_{th}_mm", s[f"ADD_{th}_mm"])
    for th in PCK_THRESHOLDS:
        add(f"Val/PCK_{th}_pixel", s[f"PCK_{th}_pixel"])
    if integral_details:
        for th in ADD_THRESHOLDS:
            add(f"Val/ADD_{th}_mm_integral_xyz_metrics", s_int[f"ADD_{th}_mm"])
        for th in PCK_THRESHOLDS:
            add(f"Val/PCK_{th}_pixel_integral_xyz_metrics", s_int[f"PCK_{th}_pixel"])
    names = (("dis3d", ""), ("dis2d", ""))
    if integral_details:
        names += (("dis3d_int", "_integral_xyz_metrics"), ("dis2d_int", "_integral_xyz_metrics"))
    for name, suffix in names:
        kind = "3D" if name.startswith("dis3d") else "2D"
        for k in range(nkp):
            add(f"Val/distance{kind}_keypoint_{k + 1}{suffix}", m[name][k])
    for k in range(dof):
        add(f"Val/l1error_joint_{k + 1}", m["l1_joint"][k])
