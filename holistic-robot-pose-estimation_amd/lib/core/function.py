"""Caller-side step function pieces the benchmark / tests need (reference lib/core/function.py).

The model call itself is ``model(reg_images, root_images, k_values, K=other_K)`` exactly as in
function.py:119-120.  What lives here is the caller contract around it, restated for device tensors:
``k_values`` (function.py:88-98) without the per-sample Python loop and the loss assembly of
function.py:191-322 for the ``configs/panda/full.yaml`` choice of loss functions.  These are O(B*7*3)
element tensor expressions (torch ops, not part of the accelerated path); the two key-point
projections go through the projection kernel.

``farward_loss`` (the reference's spelling) and ``validate`` are the reference's step and validation functions
(function.py:19-327, 330-417) on top of those pieces; the metrics of a validation batch are one launch (hrp_eval_batch)
into the device-side accumulators of an ``Evaluator``, read once per epoch."""
import functools
import math

import torch

from hrpe_amd.lib.core.common import ADD_THRESHOLDS, PCK_THRESHOLDS  # noqa: F401  (module constants of this trainer as well)
from hrpe_amd.lib.core.common import (compute_k_values, grown, images_to_device, loader_capacity, log_pose_validation, meter_mean, opt,
                                      pose_step_inputs, select_bbox_and_K, to_device, validation_batches)
from hrpe_amd.lib.dataset.const import JOINT_NAMES
from hrpe_amd.lib.utils.geometries import rotmat_to_quat, rotmat_to_rot6d
from hrpe_amd.lib.utils.transforms import point_projection_from_3d_tensor

FULL_YAML_WEIGHTS = dict(pose=1.0, rot=1.0, trans=1.0, depth=10.0, uv=1.0, kp2d=10.0, kp3d=10.0,
                         kp2d_int=10.0, kp3d_int=10.0, align_3d=0.0)   # configs/panda/full.yaml:57-66


def prepare_batch(input_batch, robot, device, reference_keypoint_id=3, use_origin_bbox=False, use_extended_bbox=True,
                  synthetic=True, rotation_dim=6):
    """The batch unpacking of function.py:25-98 for a DreamDataset batch (lib/dataset/dream.py:393-413), without the
    per-sample Python loops (gt pose/rot/trans at :50-64, k_values at :98) and without the fp32 image round trip:
    uint8 images stay uint8 on the way to the device (4x less PCIe traffic) and the model's input kernel does the
    ``.float() / 255.`` of :26,29 while it writes the trunk's NHWC layout (hrp_u8_nchw_to_nhwc); float images (the
    reference's loaders hand over float tensors holding 0..255) are scaled here as the reference does.

    Returns dict(reg_images, root_images, root_K, other_K, k_values, gt = dict(pose, rot, trans, root_rot,
    root_trans, root_depth, root_uv, kp3d, kp2d, mask)); ``gt`` feeds ``full_loss``.  `synthetic=False` (real
    datasets, function.py:66-74): the ground-truth rotation is the PnP solution (lib/utils/BPnP.py BPnP_m3d, one launch for
    the batch) of the annotated ``keypoints_2d_original`` against the FK key-points of the ground-truth joint angles under
    ``K_original[0]``; ``root_rot`` follows from it, ``trans`` stays TCO's."""

    dev = functools.partial(to_device, device=device)
    root, other = input_batch["root"], input_batch["other"]
    out = dict(root_images=images_to_device(root["images"], device), reg_images=images_to_device(other["images"], device),
               root_K=dev(root["K"]), other_K=dev(other["K"]))
    TCO = dev(input_batch["TCO"])
    jp = input_batch["jointpose"]
    pose = torch.stack([dev(jp[k]) for k in JOINT_NAMES[robot.robot_type]], dim=1)        # :51
    to_rot = rotmat_to_quat if rotation_dim == 4 else rotmat_to_rot6d                        # :60-65
    rot, trans = to_rot(TCO[:, :3, :3]), TCO[:, :3, 3].contiguous()                          # :53-54
    if not synthetic:                                                                      # :66-74
        from hrpe_amd.lib.utils.BPnP import BPnP_m3d
        from hrpe_amd.lib.utils.geometries import angle_axis_to_rotation_matrix
        world_3d_pts = robot.get_keypoints_only_fk(pose)
        P_6d = BPnP_m3d.apply(dev(input_batch["keypoints_2d_original"]), world_3d_pts, dev(input_batch["K_original"])[0])
        rot = to_rot(angle_axis_to_rotation_matrix(P_6d[:, 0:3])[:, :3, :3]).float()
    kp3d, kp2d = dev(other["keypoints_3d"]), dev(other["keypoints_2d"])
    if reference_keypoint_id == 0:                                                         # :76-78
        root_trans, root_rot = trans, rot
    else:                                                                                  # :80-82
        assert reference_keypoint_id < len(robot.link_names), reference_keypoint_id
        root_trans = kp3d[:, reference_keypoint_id, :]
        root_rot = robot.get_rotation_at_specific_root(pose, rot, trans, root=reference_keypoint_id)
    bboxes, Kk = select_bbox_and_K(input_batch, root, out["root_K"], device, use_origin_bbox, use_extended_bbox)   # :43-48, 89-94
    out["k_values"] = compute_k_values(Kk[:, 0, 0], Kk[:, 1, 1], bboxes)
    out["gt"] = dict(pose=pose, rot=rot, trans=trans, root_rot=root_rot, root_trans=root_trans,
                     root_depth=root_trans[:, 2:3], root_uv=kp2d[:, reference_keypoint_id, 0:2],
                     kp3d=kp3d, kp2d=kp2d, mask=dev(other["valid_mask_crop"]))
    return out


TERM_NAMES = ("loss_joint", "loss_rot", "loss_uv", "loss_depth", "loss_trans", "loss_error3d", "loss_error2d",
              "loss_error2d_int", "loss_error3d_int", "loss_error3d_align")          # order of function.py:313-319
_WEIGHT_KEYS = ("pose", "rot", "uv", "depth", "trans", "kp2d", "kp3d", "kp2d_int", "kp3d_int", "align_3d")


class _FusedPoseLoss(torch.autograd.Function):
    """hrp_pose_loss: the ten terms, their weighted sum and its gradient with respect to the predictions in one launch
    (the reference builds them from ~60 tensor expressions and two per-sample projection loops)."""

    @staticmethod
    def forward(ctx, K, root, image_size, wvec, gtt, pose, rot, trans, root_uv, depth, xyz_int, xyz_fk):
        import ctypes as C
        from hrpe_amd import _native as nv
        preds = [t.contiguous().float() for t in (pose, rot, trans, root_uv, depth, xyz_int, xyz_fk)]
        need = any(t.requires_grad for t in (pose, rot, trans, root_uv, depth, xyz_int, xyz_fk))
        # the seven gradients are views of ONE buffer: the backward scales it by the incoming gradient in one launch
        flat = torch.empty(sum(t.numel() for t in preds), dtype=torch.float32, device=pose.device) if need else None
        grads, off = [], 0
        for t in preds:
            grads.append(flat[off:off + t.numel()].view(t.shape) if need else None)
            off += t.numel()
        out = torch.empty(11, dtype=torch.float32, device=pose.device)
        d = nv.PoseLossDesc()
        for name, t in zip(("pose", "rot", "trans", "root_uv", "depth", "xyz_int", "xyz_fk"), preds):
            setattr(d, name, t.data_ptr())
        for name, t in zip(("gt_pose", "gt_root_rot", "gt_root_trans", "gt_root_uv", "gt_kp3d", "gt_kp2d", "mask"), gtt):
            setattr(d, name, t.data_ptr())
        d.K = K.data_ptr()
        if need:
            for name, t in zip(("d_pose", "d_rot", "d_trans", "d_root_uv", "d_depth", "d_xyz_int", "d_xyz_fk"), grads):
                setattr(d, name, t.data_ptr())
        d.out = out.data_ptr()
        for i, w in enumerate(wvec):
            d.weights[i] = w
        d.B, d.P, d.J, d.root, d.image_size = pose.shape[0], pose.shape[1], xyz_fk.shape[1], root, image_size
        d.rot_dim = rot.shape[1]
        nv.call("hrp_pose_loss", C.byref(d), torch.cuda.current_stream(pose.device).cuda_stream)
        ctx.flat, ctx.shapes = flat, [t.shape for t in preds]
        ctx.mark_non_differentiable(out)
        return out[10], out

    @staticmethod
    def backward(ctx, g_loss, _g_terms):
        if ctx.flat is None:
            return (None,) * 12
        fs, gs, off = ctx.flat * g_loss, [], 0
        for shape in ctx.shapes:
            gs.append(fs[off:off + shape.numel()].view(shape))
            off += shape.numel()
        return (None, None, None, None, None) + tuple(gs)


class _L1Loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, scale):
        from hrpe_amd import _native as nv
        p, g = pred.contiguous().float(), gt.contiguous().float()
        out = torch.empty((), dtype=torch.float32, device=pred.device)
        grad = torch.empty_like(p) if pred.requires_grad else None
        nv.call("hrp_l1_loss", p.data_ptr(), g.data_ptr(), float(scale), p.numel(), out.data_ptr(),
                grad.data_ptr() if grad is not None else None, torch.cuda.current_stream(pred.device).cuda_stream)
        ctx.grad = grad
        return out

    @staticmethod
    def backward(ctx, g_loss):
        return (ctx.grad * g_loss).view_as(ctx.grad) if ctx.grad is not None else None, None, None


SIM2REAL_YAML_WEIGHTS = dict(mask=0.0, iou=1.0, scale=0.0, align=1.0)       # configs/panda/self_supervised/*.yaml:109-112
_MASK_LOSS = {"mse_mean": 0, "bce": 1, "mse_sum": 2}


class _Sim2RealLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rendered, seg, kp3d, kp3d_int, mask_loss, w):
        import ctypes as C
        from hrpe_amd import _native as nv
        r, s_ = rendered.contiguous().float(), seg.contiguous().float()
        a, b = kp3d.contiguous().float(), kp3d_int.contiguous().float()
        B = r.shape[0]
        d = nv.Sim2RealLossDesc()
        terms = torch.empty(5, dtype=torch.float32, device=r.device)
        ws = torch.empty(8 * B, dtype=torch.float32, device=r.device)
        grads = [torch.empty_like(t) if req else None for t, req in ((r, rendered.requires_grad), (a, kp3d.requires_grad), (b, kp3d_int.requires_grad))]
        d.rendered, d.seg, d.kp3d, d.kp3d_int = r.data_ptr(), s_.data_ptr(), a.data_ptr(), b.data_ptr()
        d.B, d.HW, d.K, d.mask_loss = B, r.numel() // B, a.shape[1], mask_loss
        d.w_mask, d.w_iou, d.w_scale, d.w_align = w
        d.terms, d.workspace = terms.data_ptr(), ws.data_ptr()
        d.d_rendered, d.d_kp3d, d.d_kp3d_int = [None if g is None else g.data_ptr() for g in grads]
        nv.call("hrp_sim2real_loss", C.byref(d), torch.cuda.current_stream(r.device).cuda_stream)
        ctx.grads = [None if g is None else g.view(t.shape) for g, t in zip(grads, (rendered, kp3d, kp3d_int))]
        ctx.mark_non_differentiable(terms)
        return terms[0], terms

    @staticmethod
    def backward(ctx, g_loss, _g_terms):
        gr, ga, gb = [None if g is None else g * g_loss for g in ctx.grads]
        return gr, None, ga, gb, None, None


def sim2real_mask_loss(rendered_masks, seg_masks, pred_keypoints3d, pred_keypoints3d_int, mask_loss_func="mse_mean",
                       weights=SIM2REAL_YAML_WEIGHTS):
    """The render-and-compare losses of the self-supervised trainer (reference scripts/train_sim2real.py:435-468, BASELINE config
    5): mask (mse_mean | bce | mse_sum), IoU, scale and 3-D alignment, weighted.  rendered_masks [B, H, W] are the soft
    silhouettes of the posed robot mesh, seg_masks [B, H, W] (or [B, 1, H, W]) the segmentation network's output (detached there).
    -> (loss, dict(loss_mask, loss_iou, loss_scale, loss_error3d_align)).  Device tensors: hrp_sim2real_loss (one call, analytic
    gradient); host tensors: the same arithmetic as tensor expressions."""
    seg = seg_masks.reshape(rendered_masks.shape).detach()
    if rendered_masks.is_cuda:
        w = (float(weights["mask"]), float(weights["iou"]), float(weights["scale"]), float(weights["align"]))
        loss, t = _Sim2RealLoss.apply(rendered_masks, seg, pred_keypoints3d, pred_keypoints3d_int, _MASK_LOSS[mask_loss_func], w)
        return loss, dict(loss_mask=t[1], loss_iou=t[2], loss_scale=t[3], loss_error3d_align=t[4])
    r = rendered_masks
    if mask_loss_func == "mse_mean":
        l_mask = torch.nn.functional.mse_loss(r, seg)
    elif mask_loss_func == "bce":
        l_mask = torch.nn.functional.binary_cross_entropy(r, seg)
    else:
        l_mask = 0.001 * torch.nn.functional.mse_loss(r, seg, reduction="sum")
    inter = torch.sum(seg * r, dim=(1, 2))
    seg_area, render_area = torch.sum(seg, dim=(1, 2)), torch.sum(r, dim=(1, 2))
    l_iou = 1 - torch.mean(inter / (seg_area + render_area - inter))
    ratio = (seg_area - inter) / (render_area - inter)
    flt = (ratio.detach() > 5.0) | (ratio.detach() < 0.2)
    l_scale = torch.sum(torch.abs(torch.log(ratio)) * flt) / (torch.sum(flt) + 1e-9)
    l_align = torch.mean(torch.norm(pred_keypoints3d - pred_keypoints3d_int, dim=2))
    loss = weights["mask"] * l_mask + weights["iou"] * l_iou + weights["scale"] * l_scale + weights["align"] * l_align
    return loss, dict(loss_mask=l_mask, loss_iou=l_iou, loss_scale=l_scale, loss_error3d_align=l_align)


def depth_l1_loss(pred_depth_mm, gt_depth_m):
    """nn.L1Loss()(model(images, k_values) / 1000, gt_root_depth) of the DepthNet trainer (reference
    scripts/train_depthnet.py:231-250) as one launch with its analytic gradient (device tensors; host tensors: torch)."""
    if not pred_depth_mm.is_cuda:
        return torch.nn.functional.l1_loss(pred_depth_mm / 1000.0, gt_depth_m)
    assert pred_depth_mm.shape == gt_depth_m.shape
    return _L1Loss.apply(pred_depth_mm, gt_depth_m, 1e-3)


def full_loss(pred, gt, K, root=3, image_size=256.0, weights=FULL_YAML_WEIGHTS, kps_need_depth=None):
    """pred: the model's 8-tuple.  gt: dict(pose, root_rot, root_trans, root_uv, kp3d, kp2d, mask).
    Returns (loss, dict of the ten terms named as in function.py:313-319).  Device tensors: one fused launch
    (hrp_pose_loss, analytic gradient); host tensors: the tensor-expression form below (tests of the harness).
    multi_kp (a 9-tuple with pred_depths after pred_depth, function.py:115-117): pass kps_need_depth; the L1 term
    over the listed key-points' depths is added with weight 1 (function.py:300-311) and is not in the dict, as there."""
    if len(pred) == 9:
        assert kps_need_depth is not None, "a multi_kp prediction needs kps_need_depth"
        depths = pred[5]
        loss, terms = full_loss(pred[:5] + pred[6:], gt, K, root, image_size, weights)
        gt_depths = gt["kp3d"][:, list(kps_need_depth), 2]
        assert gt_depths.shape == depths.shape, (gt_depths.shape, depths.shape)
        return loss + torch.nn.functional.l1_loss(depths, gt_depths), terms
    if pred[0].is_cuda:
        pose, rot, trans, root_uv, depth, uvd, xyz_int, xyz_fk = pred
        f32 = lambda t: t.contiguous().float()   # noqa: E731
        gtt = [f32(gt[k]) for k in ("pose", "root_rot", "root_trans", "root_uv", "kp3d", "kp2d", "mask")]
        wvec = [float(weights[k]) for k in _WEIGHT_KEYS]
        loss, out = _FusedPoseLoss.apply(f32(K).reshape(-1, 9), int(root), float(image_size), wvec, gtt, pose, rot, trans,
                                         root_uv, depth, xyz_int, xyz_fk)
        return loss, {n: out[i] for i, n in enumerate(TERM_NAMES)}
    return full_loss_expr(pred, gt, K, root, image_size, weights)


def full_loss_expr(pred, gt, K, root=3, image_size=256.0, weights=FULL_YAML_WEIGHTS):
    """The same loss as tensor expressions (autograd) - the line-by-line restatement of function.py:191-322 the fused
    kernel is tested against."""
    pose, rot, trans, root_uv, depth, uvd, xyz_int, xyz_fk = pred
    uv_int = point_projection_from_3d_tensor(K, xyz_int)        # function.py:121
    uv_fk = point_projection_from_3d_tensor(K, xyz_fk)          # function.py:122
    m = gt["mask"]
    t = {}
    t["loss_joint"] = torch.nn.functional.mse_loss(pose, gt["pose"])
    t["loss_rot"] = torch.nn.functional.mse_loss(rot, gt["root_rot"])
    t["loss_depth"] = torch.nn.functional.l1_loss(depth, gt["root_trans"][:, 2:3])
    e = torch.norm((root_uv - gt["root_uv"]) / image_size, dim=1) * m[:, root]
    t["loss_uv"] = e.sum() / (m[:, root] != 0).sum()
    e = torch.norm(trans - gt["root_trans"], dim=1)
    coeff = torch.where(e.mean() > 0.5, torch.exp(-20.0 * e).detach(), torch.ones_like(e))  # function.py:245-251
    t["loss_trans"] = (e * coeff).mean()
    t["loss_error3d"] = torch.norm(xyz_fk - gt["kp3d"], dim=2).mean()
    gt2d = gt["kp2d"] / image_size
    nvalid = (m != 0).sum()
    t["loss_error2d"] = (torch.norm(uv_fk / image_size - gt2d, dim=2) * m).sum() / nvalid
    t["loss_error3d_int"] = torch.norm(xyz_int - gt["kp3d"], dim=2).mean()
    t["loss_error2d_int"] = (torch.norm(uv_int / image_size - gt2d, dim=2) * m).sum() / nvalid
    t["loss_error3d_align"] = torch.norm(xyz_fk - xyz_int, dim=2).mean()
    w = weights
    loss = (w["pose"] * t["loss_joint"] + w["rot"] * t["loss_rot"] + w["uv"] * t["loss_uv"]
            + w["depth"] * t["loss_depth"] + w["trans"] * t["loss_trans"] + w["kp2d"] * t["loss_error2d"]
            + w["kp3d"] * t["loss_error3d"] + w["kp2d_int"] * t["loss_error2d_int"]
            + w["kp3d_int"] * t["loss_error3d_int"] + w["align_3d"] * t["loss_error3d_align"])
    return loss, t


# the choice of loss functions hrp_pose_loss implements: identical in every configs/*/full.yaml
SHIPPED_LOSS_FUNCS = dict(pose_loss_func="mse", rot_loss_func="mse", trans_loss_func="l2norm", depth_loss_func="l1",
                          uv_loss_func="l2norm", kp2d_loss_func="l2norm", kp3d_loss_func="l2norm", kp2d_int_loss_func="l2norm",
                          kp3d_int_loss_func="l2norm", align_3d_loss_func="l2norm")
LOSS_SLOTS = TERM_NAMES + ("loss",)       # the eleven values an Evaluator keeps per batch
METRIC_KEYS = ("image_dis3d_avg", "image_dis2d_avg", "batch_dis3d_avg", "batch_dis2d_avg", "batch_l1jointerror_avg",
               "image_l1jointerror_avg", "root_depth_error", "image_dis3d_avg_int", "image_dis2d_avg_int", "batch_dis3d_avg_int",
               "batch_dis2d_avg_int", "root_depth_error_int", "rotation_diff")          # function.py:173-179


def check_loss_options(args):
    """NotImplementedError, naming the option, for what the fused loss does not cover (function.py:195-298)."""
    for name, shipped in SHIPPED_LOSS_FUNCS.items():
        got = opt(args, name, shipped)
        if got != shipped:
            raise NotImplementedError(f"{name}={got!r}: the fused loss implements {name}={shipped!r} (every configs/*/full.yaml)")
    if opt(args, "fix_mask", False):
        raise NotImplementedError("fix_mask=True: the fused loss has no masked kp3d_int / align_3d terms (function.py:276-278, 294-296)")


class Evaluator:
    """The accumulators of one validation epoch, on the device (reference function.py:337-376: thirteen AverageValueMeters,
    five lists and a host copy of everything per batch).

    ``add`` is one hrp_eval_batch launch and one copy of the eleven loss values; nothing synchronises with the host until
    ``summary``.  Per-image values live in ``per_image`` [11, capacity] (rows: nv.EvalDesc.PER_IMAGE), per-batch values in
    ``dis`` [4, batch_capacity, nkp] (dis3d, dis2d, dis3d_int, dis2d_int), ``l1_joint`` [batch_capacity, dof], ``rot_diff``
    [batch_capacity] and ``losses`` [batch_capacity, 11] (LOSS_SLOTS).  ``count`` images and ``batches`` batches are filled;
    the host knows both, so growing (reallocate + copy) needs no synchronisation either."""

    def __init__(self, robot, capacity, reference_keypoint_id=3, device=None, batch_capacity=64):
        from hrpe_amd import _native as nv
        self.robot, self.root = robot, int(reference_keypoint_id)
        self.device = torch.device(device if device is not None else "cuda")
        self.nkp, self.dof = len(robot.link_names), robot.dof
        self.capacity, self.batch_capacity = max(int(capacity), 1), max(int(batch_capacity), 1)
        self.count = self.batches = 0
        self.last = None                                    # (offset, B, batch index) of the last add
        self._names = nv.EvalDesc.PER_IMAGE
        f = dict(dtype=torch.float32, device=self.device)
        self.per_image = torch.zeros(len(self._names), self.capacity, **f)
        self.dis = torch.zeros(4, self.batch_capacity, self.nkp, **f)
        self.l1_joint = torch.zeros(self.batch_capacity, self.dof, **f)
        self.rot_diff = torch.zeros(self.batch_capacity, **f)
        self.losses = torch.zeros(self.batch_capacity, len(LOSS_SLOTS), **f)

    def _grow(self, images, batches):
        if images <= self.capacity and batches <= self.batch_capacity:
            return
        self.per_image = grown(self.per_image, 1, self.count, images)
        for name, axis in (("dis", 1), ("l1_joint", 0), ("rot_diff", 0), ("losses", 0)):
            setattr(self, name, grown(getattr(self, name), axis, self.batches, batches))
        self.capacity, self.batch_capacity = self.per_image.shape[1], self.losses.shape[0]

    def add(self, pred, gt, loss=None, loss_dict=None):
        """pred: dict(kp3d_fk [B,nkp,3], kp3d_int [B,nkp,3], joint [B,dof] or None, rot [B,rot_dim]);
        gt: dict(kp3d, kp2d_original [B,nkp,2], K_original [B,3,3], joint [B,dof], rot [B,rot_dim] - the base rotation).
        loss / loss_dict: what full_loss returned (optional).  Returns ``metric_dict()`` of this batch."""
        import ctypes as C
        from hrpe_amd import _native as nv
        f32 = lambda t: t.detach().to(self.device, torch.float32, non_blocking=True).contiguous()   # noqa: E731
        ins = dict(pred_kp3d_fk=f32(pred["kp3d_fk"]), pred_kp3d_int=f32(pred["kp3d_int"]), gt_kp3d=f32(gt["kp3d"]),
                   gt_kp2d=f32(gt["kp2d_original"]), K=f32(gt["K_original"]), gt_joint=f32(gt["joint"]),
                   pred_rot=f32(pred["rot"]), gt_rot=f32(gt["rot"]))
        if pred.get("joint") is not None:
            ins["pred_joint"] = f32(pred["joint"])
        B = ins["pred_kp3d_fk"].shape[0]
        shapes = dict(pred_kp3d_fk=(B, self.nkp, 3), pred_kp3d_int=(B, self.nkp, 3), gt_kp3d=(B, self.nkp, 3), gt_kp2d=(B, self.nkp, 2),
                      K=(B, 3, 3), gt_joint=(B, self.dof), pred_joint=(B, self.dof), pred_rot=(B, ins["pred_rot"].shape[-1]),
                      gt_rot=tuple(ins["pred_rot"].shape))
        for k, t in ins.items():
            if k in shapes and tuple(t.shape) != shapes[k]:
                raise nv.HrpError(f"Evaluator.add: {k} is {tuple(t.shape)}, expected {shapes[k]}")
        self._grow(self.count + B, self.batches + 1)
        d = nv.EvalDesc()
        for k, t in ins.items():
            setattr(d, k, t.data_ptr())
        for i, k in enumerate(self._names):
            setattr(d, k, self.per_image[i].data_ptr())
        for i, k in enumerate(("dis3d", "dis2d", "dis3d_int", "dis2d_int")):
            setattr(d, k, self.dis[i].data_ptr())
        d.l1_jointerror, d.rotation_diff = self.l1_joint.data_ptr(), self.rot_diff.data_ptr()
        d.B, d.nkp, d.dof, d.rot_dim, d.root = B, self.nkp, self.dof, ins["pred_rot"].shape[1], self.root
        d.drop_last_joint = int(self.robot.robot_type == "panda")                 # metrics.py:84-85
        d.offset, d.capacity, d.batch_index, d.batch_capacity = self.count, self.capacity, self.batches, self.batch_capacity
        nv.call("hrp_eval_batch", C.byref(d), torch.cuda.current_stream(self.device).cuda_stream)
        if loss_dict is not None:
            torch.stack([loss_dict[n].detach().float().reshape(()) for n in TERM_NAMES] + [loss.detach().float().reshape(())],
                        out=self.losses[self.batches])
        self.last = (self.count, B, self.batches)
        self.count, self.batches = self.count + B, self.batches + 1
        return self.metric_dict()

    def metric_dict(self):
        """The thirteen entries of function.py:173-179 for the last batch: views of the accumulators (device tensors)."""
        o, B, i = self.last
        im = {n: self.per_image[k, o:o + B] for k, n in enumerate(self._names)}
        return {"image_dis3d_avg": im["error3d"], "image_dis2d_avg": im["error2d"], "batch_dis3d_avg": self.dis[0, i],
                "batch_dis2d_avg": self.dis[1, i], "batch_l1jointerror_avg": self.l1_joint[i],
                "image_l1jointerror_avg": im["mean_jointerror"], "root_depth_error": im["error_depth"],
                "image_dis3d_avg_int": im["error3d_int"], "image_dis2d_avg_int": im["error2d_int"],
                "batch_dis3d_avg_int": self.dis[2, i], "batch_dis2d_avg_int": self.dis[3, i],
                "root_depth_error_int": im["error_depth_int"], "rotation_diff": self.rot_diff[i]}

    def summary(self):
        """The one synchronisation of the epoch: the accumulators come to the host in one piece each.  Returns the reference's
        ``summary_add_pck`` of the FK branch at the top level (``['ADD/AUC']`` ...), of the integral branch under ``'integral'`` and
        of the root-relative errors under ``'relative'`` (scripts/test.py:226-235), and
          'meters'  the AverageValueMeter means of function.py:337-376 - unweighted means over batches, fp64, in batch order - of
                    the eleven LOSS_SLOTS, 'rotation_diff', and the vectors 'dis3d', 'dis2d', 'dis3d_int', 'dis2d_int', 'l1_joint';
          'mean_joint_error' in degrees (function.py:380), 'mean_depth_error', 'relative_depth_error' (scripts/test.py:240-242),
          'Relative_ADD/AUC' (:254)."""
        from hrpe_amd.lib.utils.metrics import summary_add_pck
        n, nb = self.count, self.batches
        assert n > 0 and nb > 0, "Evaluator.summary: nothing was added"
        im = dict(zip(self._names, self.per_image[:, :n].cpu()))
        out = summary_add_pck({"dis3d": im["error3d"], "dis2d": im["error2d"]})
        out["integral"] = summary_add_pck({"dis3d": im["error3d_int"], "dis2d": im["error2d_int"]})
        out["relative"] = summary_add_pck({"dis3d": im["error3d_relative"], "dis2d": im["error2d"]})
        losses = meter_mean(self.losses[:nb].cpu())
        dis = self.dis[:, :nb].cpu()
        meters = {k: float(losses[i]) for i, k in enumerate(LOSS_SLOTS)}
        meters["rotation_diff"] = float(meter_mean(self.rot_diff[:nb].cpu().reshape(nb, 1))[0])
        for i, k in enumerate(("dis3d", "dis2d", "dis3d_int", "dis2d_int")):
            meters[k] = meter_mean(dis[i])
        meters["l1_joint"] = meter_mean(self.l1_joint[:nb].cpu())
        out["meters"] = meters
        out["mean_joint_error"] = float(im["mean_jointerror"].double().mean()) / math.pi * 180.0
        out["mean_depth_error"] = float(im["error_depth"].double().mean())
        out["relative_depth_error"] = float(im["batch_error_relative"].double().mean())
        out["Relative_ADD/AUC"] = out["relative"]["ADD/AUC"]
        return out


def farward_loss(args, input_batch, model, robot, device, device_id, train=True, evaluator=None):
    """The reference's step function (function.py:19-327; its spelling): ``(loss, loss_dict)`` when training, plus
    ``metric_dict`` (device tensors) when not.  Batch unpacking is ``prepare_batch``, the loss ``full_loss`` (one launch), the
    metrics one hrp_eval_batch launch into ``evaluator`` (validate passes the epoch's; without one the metrics of this batch
    alone are computed).  ``device_id`` is the reference's DataParallel list: the model is called as it is (bring it to
    ``device`` and wrap it for several GPUs - hrpe_amd.parallel - before)."""
    check_loss_options(args)
    model.train() if train else model.eval()
    multi_kp = bool(opt(args, "multi_kp", False))
    st = pose_step_inputs(args, input_batch, model, robot, device, int(opt(args, "rotation_dim", 6)), evaluate=not train)
    p, gt, pred, pred_pose, root = st.p, st.gt, st.pred, st.pred_pose, st.root
    assert len(pred) == (9 if multi_kp else 8), len(pred)
    if not train and evaluator is None:
        evaluator = Evaluator(robot, pred_pose.shape[0], reference_keypoint_id=root, device=device, batch_capacity=1)
    if opt(args, "known_joint", False):                                                                  # :188-189
        pred_pose = gt["pose"].clone()
    weights = {k: float(opt(args, k + "_loss_weight", FULL_YAML_WEIGHTS[k])) for k in _WEIGHT_KEYS}
    loss, loss_dict = full_loss((pred_pose,) + pred[1:], gt, p["other_K"], root=root, image_size=float(opt(args, "image_size", 256.0)),
                                weights=weights, kps_need_depth=opt(args, "kps_need_depth") if multi_kp else None)
    if train:
        return loss, loss_dict
    metric_dict = evaluator.add(st.ev_pred, st.ev_gt, loss, loss_dict)
    return loss, loss_dict, metric_dict


def validate(args, epoch, dsname, loader, model, robot, writer, device, device_id):
    """The reference's validation loop (function.py:330-417): one farward_loss(train=False) per batch into one Evaluator, one
    summary - the only host synchronisation - at the end, every scalar the reference logs under its tag.  Returns ADD-AUC.
    ``writer`` may be None.  A loader over this project's DreamDataset (host items with ``frame`` / ``aug``) goes through
    ``DreamDataset.to_device`` first; a batch already in the reference schema goes straight to ``prepare_batch``."""
    assert (dsname != "photo" or args.urdf_robot_name != "baxter")          # ds == photo -> not baxter
    assert (dsname in ["dr", "photo"] or args.urdf_robot_name == "panda")   # ds != dr/photo -> panda
    ds = "_" + dsname
    model.eval()
    ev = Evaluator(robot, loader_capacity(loader), reference_keypoint_id=args.reference_keypoint_id, device=device)
    with torch.no_grad():
        for sample in validation_batches(loader, device):
            farward_loss(args=args, input_batch=sample, model=model, robot=robot, device=device, device_id=device_id, train=False,
                         evaluator=ev)
    s = ev.summary()
    if writer is not None:
        m = s["meters"]
        add = lambda tag, v: writer.add_scalar(tag + ds, float(v), epoch)   # noqa: E731
        add("Val/loss", m["loss"])
        add("Val/pose_loss", m["loss_joint"])
        add("Val/rot_loss", m["loss_rot"])
        add("Val/rot_diff", m["rotation_diff"])
        add("Val/trans_loss", m["loss_trans"])
        add("Val/uv_loss", m["loss_uv"])
        add("Val/depth_loss", m["loss_depth"])
        add("Val/error2d_loss", m["loss_error2d"])
        add("Val/error3d_loss", m["loss_error3d"])
        # as the reference: the two *_int_loss tags log the NON-integral meters (function.py:390-391)
        add("Val/error2d_int_loss", m["loss_error2d"])
        add("Val/error3d_int_loss", m["loss_error3d"])
        add("Val/error3d_align_loss", m["loss_error3d_align"])
        log_pose_validation(add, s, ev.nkp, ev.dof, integral_details=True)
    model.train()
    return s["ADD/AUC"]
