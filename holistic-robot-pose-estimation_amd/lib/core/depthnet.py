"""The step and validation functions of the DepthNet trainer (reference scripts/train_depthnet.py).

The reference has no module for them: its step is a function nested inside the epoch loop (train_depthnet.py:152-273) and its
validation another (:276-303).  What lives here is their caller contract, restated for device tensors:
``prepare_depthnet_batch`` (:161-213) without the per-sample Python loops, ``depthnet_loss`` (:220-268) as ONE launch
(hrp_depth_loss: loss, its gradient with respect to the model output, the per-image errors), ``DepthEvaluator`` - the
accumulators of one validation epoch on the device, read once - and ``farward_loss`` (the reference's spelling) / ``validate`` on
top of those pieces.  The model call itself is ``model(images, k_values)`` exactly as at :222-231.

It differs from ``lib/core/function.py`` where the reference's two trainers differ: the ground truth comes from the ROOT view
(``input_batch["root"]["keypoints_3d"]`` / ``["valid_mask_crop"]``, :172-174) and ``k_values`` takes ``abs(fx) * abs(fy)`` (:212)."""
import functools
import types

import numpy as np
import torch

from hrpe_amd.lib.core.common import (compute_k_values, grown, images_to_device, loader_capacity, meter_mean, opt, select_bbox_and_K,
                                      to_device, validation_batches)
from hrpe_amd.lib.dataset.const import LINK_NAMES

DEPTH_LOSS_FUNCS = ("l1", "mse")        # train_depthnet.py:249-254, 263-268
XY_LOSS_FUNCS = ("l1", "mse")           # :256-261
VAL_TAGS = ("Val/rootz_loss", "Val/mean_depth_error", "Val/mean_x_error", "Val/mean_y_error")       # :298-301


def compute_depthnet_k_values(fx, fy, bboxes, real_bbox=(1000.0, 1000.0)):
    """k = sqrt(|fx| * |fy| * 1000 * 1000 / max(|x2-x1|, |y2-y1|)^2) in the reference's order of operations (:202-212)."""
    return compute_k_values(fx, fy, bboxes, real_bbox, absolute=True)


def prepare_depthnet_batch(input_batch, robot, device, reference_keypoint_id=3, use_origin_bbox=False, use_extended_bbox=True,
                           multi_kp=False, kps_need_depth=None):
    """The batch unpacking of train_depthnet.py:161-213 for a DreamDataset batch, without the per-sample Python loops (gt
    translation at :178-187, k_values at :212) and without the fp32 image round trip: uint8 images stay uint8 on the way to the
    device and the model's input kernel does the ``.float() / 255.`` of :161; float images are scaled here as the reference does.

    Returns dict(images, K, k_values, gt = dict(root_trans [B,3], root_depth [B,1], kp3d [B,J,3], mask [B])); ``gt`` feeds
    ``depthnet_loss``.  Everything in ``gt`` is the ROOT view's (:172-174); ``mask`` is ``valid_mask_crop[:, reference_keypoint_id]``
    (:247).  With ``multi_kp``, ``gt["kp_depths"]`` = ``kp3d[:, kps_need_depth, 2]`` (:196-197) is there as well (a view for the host
    path; the kernel gathers it itself)."""

    dev = functools.partial(to_device, device=device)
    root = input_batch["root"]
    images = images_to_device(root["images"], device)                                                         # :161
    K = dev(root["K"])                                                                                        # :163
    bboxes, Kk = select_bbox_and_K(input_batch, root, K, device, use_origin_bbox, use_extended_bbox)          # :165-170, 203-208
    kp3d = dev(root["keypoints_3d"])                                                                          # :172
    valid_mask_crop = dev(root["valid_mask_crop"])                                                            # :174
    ref = int(reference_keypoint_id)
    if ref == 0:                                                                                              # :188-189
        root_trans = dev(input_batch["TCO"])[:, :3, 3].contiguous()
    else:                                                                                                     # :190-192
        assert ref < len(robot.link_names), ref
        root_trans = kp3d[:, ref, :].contiguous()
    assert root_trans.shape == (images.shape[0], 3), root_trans.shape                                         # :193
    gt = dict(root_trans=root_trans, root_depth=root_trans[:, 2:3], kp3d=kp3d, mask=valid_mask_crop[:, ref].contiguous())
    if multi_kp:                                                                                              # :196-197
        gt["kp_depths"] = kp3d[:, list(kps_need_depth), 2]
    return dict(images=images, K=K, k_values=compute_depthnet_k_values(Kk[:, 0, 0], Kk[:, 1, 1], bboxes), gt=gt)


def check_depthnet_options(depth_loss_func, xy_loss_func, kps_need_depth=None):
    """NotImplementedError for a loss function the reference does not know (:253-254, 260-261, 267-268)."""
    if depth_loss_func not in DEPTH_LOSS_FUNCS:
        raise NotImplementedError(f"depth_loss_func={depth_loss_func!r}: the DepthNet trainer knows {DEPTH_LOSS_FUNCS}")
    if xy_loss_func is not None and xy_loss_func not in XY_LOSS_FUNCS:
        raise NotImplementedError(f"xy_loss_func={xy_loss_func!r}: the DepthNet trainer knows {XY_LOSS_FUNCS}")
    if xy_loss_func is not None and kps_need_depth is not None:
        raise NotImplementedError("the xy branch and multi_kp exclude each other (the reference's xy forward has no pred_depths, :221-229)")


def _root_col(xy_loss_func, kps_need_depth, reference_keypoint_id):
    if xy_loss_func is not None:
        return 2                                                                  # :223
    if kps_need_depth is not None:
        return list(kps_need_depth).index(int(reference_keypoint_id))             # :228
    return 0


def depthnet_errors_expr(pred, gt, xy_loss_func=None, kps_need_depth=None, reference_keypoint_id=3):
    """(error_depth, error_x, error_y), each [B] (train_depthnet.py:223-241) as tensor expressions."""
    B = pred.shape[0]
    col = _root_col(xy_loss_func, kps_need_depth, reference_keypoint_id)
    pred_root_depth = pred[:, col] / 1000.0
    error_depth = torch.abs(pred_root_depth.reshape(B) - gt["root_trans"][:, 2].reshape(B)).detach()
    if xy_loss_func is None:
        return error_depth, torch.zeros_like(error_depth), torch.zeros_like(error_depth)
    return (error_depth, torch.abs(pred[:, 0] - gt["root_trans"][:, 0]).detach(),
            torch.abs(pred[:, 1] - gt["root_trans"][:, 1]).detach())


def depthnet_loss_expr(pred, gt, depth_loss_func="l1", xy_loss_func=None, kps_need_depth=None, reference_keypoint_id=3):
    """The loss of train_depthnet.py:220-268 as tensor expressions (autograd) - the line-by-line restatement the kernel is tested
    against."""
    check_depthnet_options(depth_loss_func, xy_loss_func, kps_need_depth)
    L = {"l1": torch.nn.functional.l1_loss, "mse": torch.nn.functional.mse_loss}
    B = pred.shape[0]
    gt_root_trans = gt["root_trans"]
    gt_root_depth = gt_root_trans[:, 2].unsqueeze(-1)                             # :194
    if kps_need_depth is not None:                                                # :225-229, 263-266
        pred_depths = pred / 1000.0
        gt_kp_depths = gt["kp3d"][:, list(kps_need_depth), 2]
        assert pred_depths.shape == gt_kp_depths.shape, (pred_depths.shape, gt_kp_depths.shape)
        return L[depth_loss_func](pred_depths, gt_kp_depths)
    if xy_loss_func is None:                                                      # :231-232, 249-252
        assert pred.shape == (B, 1), pred.shape
        return L[depth_loss_func](pred / 1000.0, gt_root_depth)
    coord = pred                                                                  # :222-223
    assert coord.shape == (B, 3), coord.shape
    pred_root_depth = coord[:, 2] / 1000.0
    # the reference hands nn.L1Loss / nn.MSELoss a [B] prediction and a [B, 1] target (:223, :250): torch broadcasts the pair to
    # [B, B] - element (i, j) is (prediction j, target i) - and takes the mean over all B * B.  Written out, without the warning:
    loss = L[depth_loss_func](pred_root_depth.reshape(1, B).expand(B, B), gt_root_depth.expand(B, B))
    mask = gt["mask"].reshape(B, 1)                                               # :247
    return loss + L[xy_loss_func](coord[:, 0:2] * mask, gt_root_trans[:, 0:2] * mask)       # :255-259


class DepthEvaluator:
    """The accumulators of one DepthNet validation epoch, on the device (reference train_depthnet.py:285-301: one
    AverageValueMeter, three lists and three host copies per batch).

    ``errors`` [3, capacity] holds |depth error|, |x error|, |y error| per image, ``losses`` [batch_capacity] the loss per batch;
    ``count`` images and ``batches`` batches are filled.  The host knows both counters, so growing (reallocate + copy) needs no
    synchronisation.  hrp_depth_loss writes a batch at ``reserve(B)``; ``commit(B)`` advances the counters."""

    ROWS = ("error_depth", "error_x", "error_y")

    def __init__(self, capacity, device=None, batch_capacity=64):
        self.device = torch.device(device if device is not None else "cuda")
        self.capacity, self.batch_capacity = max(int(capacity), 1), max(int(batch_capacity), 1)
        self.count = self.batches = 0
        self.last = None                                    # (offset, B, batch index) of the last batch
        self.errors = torch.zeros(3, self.capacity, dtype=torch.float32, device=self.device)
        self.losses = torch.zeros(self.batch_capacity, dtype=torch.float32, device=self.device)

    def reserve(self, B):
        """Make room for one more batch of B images -> (offset, batch index)."""
        if self.count + B > self.capacity or self.batches + 1 > self.batch_capacity:
            self.errors = grown(self.errors, 1, self.count, self.count + B)
            self.losses = grown(self.losses, 0, self.batches, self.batches + 1)
            self.capacity, self.batch_capacity = self.errors.shape[1], self.losses.shape[0]
        return self.count, self.batches

    def commit(self, B):
        self.last = (self.count, B, self.batches)
        self.count, self.batches = self.count + B, self.batches + 1

    def add_host(self, loss, error_depth, error_x, error_y):
        """One batch from tensor expressions (the host path of ``depthnet_loss``)."""
        B = error_depth.shape[0]
        o, i = self.reserve(B)
        for r, e in enumerate((error_depth, error_x, error_y)):
            self.errors[r, o:o + B].copy_(e.detach().reshape(B))
        self.losses[i].copy_(loss.detach().reshape(()))
        self.commit(B)

    def last_errors(self):
        """(error_depth, error_x, error_y) of the last batch: views of the rows (device tensors)."""
        o, B, _ = self.last
        return tuple(self.errors[r, o:o + B] for r in range(3))

    def summary(self):
        """The one synchronisation of the epoch: both accumulators come to the host in one piece each.  ``rootz_loss`` is the
        AverageValueMeter mean (:285, 291, 298) - the unweighted mean over batches, fp64, in batch order; the three error means are
        ``np.mean`` over the per-image fp32 values as at :296-297."""
        n, nb = self.count, self.batches
        assert n > 0 and nb > 0, "DepthEvaluator.summary: nothing was added"
        errors, losses = self.errors[:, :n].cpu().numpy(), self.losses[:nb].cpu().numpy()
        return dict(rootz_loss=float(meter_mean(losses)), mean_depth_error=float(np.mean(errors[0])), mean_x_error=float(np.mean(errors[1])),
                    mean_y_error=float(np.mean(errors[2])))


class _DepthLoss(torch.autograd.Function):
    """hrp_depth_loss: the loss, its gradient with respect to the model output and (with an evaluator) the per-image errors of the
    batch in one launch."""

    @staticmethod
    def forward(ctx, pred, gt, depth_loss_func, xy_loss_func, kps_need_depth, root_col, evaluator):
        import ctypes as C
        from hrpe_amd import _native as nv
        p = pred.detach().contiguous().float()
        dev = p.device
        f32 = lambda t: t.detach().to(dev, torch.float32).contiguous()   # noqa: E731
        root_trans = f32(gt["root_trans"])
        B, W = p.shape
        assert root_trans.shape == (B, 3), root_trans.shape
        d = nv.DepthLossDesc()
        keep = [p, root_trans]
        d.pred, d.gt_root_trans = p.data_ptr(), root_trans.data_ptr()
        if kps_need_depth is not None:
            kp3d = f32(gt["kp3d"])
            assert kp3d.dim() == 3 and kp3d.shape[0] == B and kp3d.shape[2] == 3, kp3d.shape
            keep.append(kp3d)
            d.gt_kp3d, d.J, d.nk = kp3d.data_ptr(), kp3d.shape[1], len(kps_need_depth)
            if d.nk > nv.DEPTH_LOSS_MAX_KP:
                raise nv.HrpError(f"depthnet_loss: {d.nk} key-points need a depth, hrp_depth_loss takes {nv.DEPTH_LOSS_MAX_KP}")
            for i, k in enumerate(kps_need_depth):
                d.kp_index[i] = int(k)
        if xy_loss_func is not None:
            mask = f32(gt["mask"]).reshape(-1)
            assert mask.shape == (B,), mask.shape
            keep.append(mask)
            d.mask = mask.data_ptr()
        loss = torch.empty((), dtype=torch.float32, device=dev)
        grad = torch.empty_like(p) if pred.requires_grad else None
        d.loss, d.d_pred, d.want_grad = loss.data_ptr(), (grad.data_ptr() if grad is not None else None), int(grad is not None)
        d.B, d.W, d.root_col = B, W, root_col
        d.depth_loss, d.xy_loss = nv.DEPTH_LOSS_KINDS[depth_loss_func], nv.XY_LOSS_KINDS[xy_loss_func]
        if evaluator is not None:
            assert evaluator.errors.device == dev, (evaluator.errors.device, dev)
            d.offset, d.batch_index = evaluator.reserve(B)
            d.capacity, d.batch_capacity = evaluator.capacity, evaluator.batch_capacity
            d.errors, d.losses = evaluator.errors.data_ptr(), evaluator.losses.data_ptr()
        nv.call("hrp_depth_loss", C.byref(d), torch.cuda.current_stream(dev).cuda_stream)
        if evaluator is not None:
            evaluator.commit(B)
        ctx.grad = grad
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        return (ctx.grad * g_loss if ctx.grad is not None else None,) + (None,) * 6


def depthnet_loss(pred, gt, depth_loss_func="l1", xy_loss_func=None, kps_need_depth=None, reference_keypoint_id=3, evaluator=None):
    """The DepthNet trainer's loss (train_depthnet.py:220-268).  pred [B, W]: the model output in mm - W = 1 (plain), 3 with the xy
    branch ``(x, y, depth)`` (``xy_loss_func`` 'l1' | 'mse'), len(kps_need_depth) with multi_kp.  gt: dict(root_trans [B,3],
    kp3d [B,J,3] (multi_kp), mask [B] (xy branch)) as ``prepare_depthnet_batch`` returns it.  ``evaluator`` (a DepthEvaluator): the
    batch's loss and per-image errors are added to it (``evaluator.last_errors()``).  Returns the loss.
    Device tensors: one hrp_depth_loss launch with its analytic gradient; host tensors: the same arithmetic as tensor expressions.
    A loss function the reference does not know raises NotImplementedError, as there."""
    check_depthnet_options(depth_loss_func, xy_loss_func, kps_need_depth)
    B = pred.shape[0]
    want_w = len(kps_need_depth) if kps_need_depth is not None else (3 if xy_loss_func is not None else 1)
    assert pred.shape == (B, want_w), (tuple(pred.shape), want_w)
    root_col = _root_col(xy_loss_func, kps_need_depth, reference_keypoint_id)
    if pred.is_cuda:
        kps = None if kps_need_depth is None else tuple(int(k) for k in kps_need_depth)
        return _DepthLoss.apply(pred, gt, depth_loss_func, xy_loss_func, kps, root_col, evaluator)
    loss = depthnet_loss_expr(pred, gt, depth_loss_func, xy_loss_func, kps_need_depth, reference_keypoint_id)
    if evaluator is not None:
        evaluator.add_host(loss, *depthnet_errors_expr(pred, gt, xy_loss_func, kps_need_depth, reference_keypoint_id))
    return loss


def farward_loss(args, input_batch, device, model, train=True, evaluator=None):
    """The reference's nested step function (train_depthnet.py:152-273; its spelling and its parameters): the loss when training,
    ``(loss, error_depth, error_x, error_y)`` - device tensors, each [B] - when not.  Batch unpacking is
    ``prepare_depthnet_batch``, everything after the model call one hrp_depth_loss launch.  With an ``evaluator`` (validate passes
    the epoch's) the three errors are views of its rows; without one the errors of this batch alone are computed.  The model is
    called as it is (bring it to ``device`` - and wrap it for several GPUs, hrpe_amd.parallel - before)."""
    xy = bool(opt(args, "use_rootnet_xy_branch", False))
    multi_kp = bool(opt(args, "multi_kp", False))
    depth_loss_func = opt(args, "depth_loss_func", "l1")
    xy_loss_func = opt(args, "xy_loss_func", "mse") if xy else None
    if xy and xy_loss_func is None:
        raise NotImplementedError("xy_loss_func=None with use_rootnet_xy_branch")
    kps = list(args.kps_need_depth) if multi_kp else None
    check_depthnet_options(depth_loss_func, xy_loss_func, kps)
    model.train() if train else model.eval()                                                                 # :153-156
    ref = int(args.reference_keypoint_id)
    name = opt(args, "urdf_robot_name", "panda")
    robot = types.SimpleNamespace(robot_type=name, link_names=LINK_NAMES[name])
    p = prepare_depthnet_batch(input_batch, robot, device, reference_keypoint_id=ref,
                               use_origin_bbox=bool(opt(args, "use_origin_bbox", False)),
                               use_extended_bbox=bool(opt(args, "use_extended_bbox", True)), multi_kp=multi_kp, kps_need_depth=kps)
    pred = model(p["images"], p["k_values"])                                                                 # :221-231
    if train:
        return depthnet_loss(pred, p["gt"], depth_loss_func, xy_loss_func, kps, ref)
    if evaluator is None:
        evaluator = DepthEvaluator(pred.shape[0], device=pred.device, batch_capacity=1)
    loss = depthnet_loss(pred, p["gt"], depth_loss_func, xy_loss_func, kps, ref, evaluator=evaluator)
    return (loss,) + evaluator.last_errors()


def validate(args, epoch, dsname, loader, model, writer, device):
    """The reference's nested validation loop (train_depthnet.py:276-303; ``loader`` is the data loader its ``ds`` selects): one
    farward_loss(train=False) per batch into one DepthEvaluator, one summary - the only host synchronisation - at the end, the
    reference's four scalars under their tags with the ``"_" + dsname`` suffix.  Returns mean_depth_error, the number that picks
    the checkpoint (:336, 374-376).  ``writer`` may be None.  A loader over this project's DreamDataset (host items with ``frame`` /
    ``aug``) goes through ``DreamDataset.to_device`` first."""
    ds = "_" + dsname                                                                                        # :283
    model.eval()
    ev = DepthEvaluator(loader_capacity(loader), device=device)
    with torch.no_grad():
        for sample in validation_batches(loader, device):
            farward_loss(args=args, input_batch=sample, device=device, model=model, train=False, evaluator=ev)
    s = ev.summary()
    if writer is not None:
        writer.add_scalar("Val/rootz_loss" + ds, s["rootz_loss"], epoch)                                     # :298-301
        writer.add_scalar("Val/mean_depth_error" + ds, s["mean_depth_error"], epoch)
        writer.add_scalar("Val/mean_x_error" + ds, s["mean_x_error"], epoch)
        writer.add_scalar("Val/mean_y_error" + ds, s["mean_y_error"], epoch)
    model.train()                                                                                            # :302
    return s["mean_depth_error"]
