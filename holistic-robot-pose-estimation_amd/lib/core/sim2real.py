"""The step and validation functions of the self-supervised render-and-compare trainer (reference scripts/train_sim2real.py,
BASELINE config 5).

The reference has no module for them: its step is a function nested inside the epoch loop (train_sim2real.py:137-534), its
validation another (:536-625), and the training loop feeds twelve AverageValueMeters with twelve host copies per step (:649-660).
What lives here is their caller contract, restated for device tensors on top of the pieces this library already has -
``prepare_batch`` (lib/core/function.py), ``URDFRobot.get_rendered_masks``, ``sim2real_mask_loss``, ``Evaluator``:

``sim2real_monitor``   the seven supervised terms the script computes every step for its logs (:313-400), next to the mask terms, as
                       ONE launch (hrp_sim2real_monitor) that also advances meters living on the device;
``TrainMeters``        those meters: one read, every tenth step in the reference's loop (:662-686), is the only synchronisation;
``farward_loss``       the step (the reference's spelling): ``(loss, loss_dict)`` when training, plus ``metric_dict`` when not;
``Sim2RealEvaluator``  the accumulators of one validation epoch on the device (``function.Evaluator`` plus the image ids and the
                       twelve values per batch), read once;
``validate``           the validation loop with every scalar of :597-623 under its tag, or the "worst cases" list (:582-592).

The supervised terms differ from ``function.full_loss``'s where the two scripts differ: ``loss_uv`` here is the plain mean of the
root key-point error (:350-353), not the masked quotient of function.py:231-235, and there are no integral-branch terms.

PARITY UNPINNED: the reference's step is a closure inside the script and needs pytorch3d, cv2 and CUDA, so no fixture comes from it;
the terms are held to a float64 restatement of :313-400 (tests/test_sim2real_step_host.py, tests/test_gpu_sim2real_step.py).
Out of scope: the cv2 / matplotlib visualisation (:417-433, 471-529) and the 5-tuple model branch (:245-251)."""
import weakref

import numpy as np
import torch

from hrpe_amd import _native as nv
from hrpe_amd.lib.core import function as F
from hrpe_amd.lib.core.common import grown, loader_capacity, log_pose_validation, meter_mean, opt, pose_step_inputs, validation_batches

ROW = nv.SIM2REAL_ROW                   # the twelve values of one step, in hrp_sim2real_monitor's order
LOSS_KEYS = ("loss_joint", "loss_rot", "loss_uv", "loss_depth", "loss_trans", "loss_error2d", "loss_error3d", "loss_mask", "loss_scale",
             "loss_iou", "loss_error3d_align")                         # loss_dict of train_sim2real.py:395-400
# the loss functions hrp_sim2real_monitor implements: identical in every configs/*/self_supervised/*.yaml (:45-51)
SHIPPED_LOSS_FUNCS = dict(pose_loss_func="mse", rot_loss_func="mse", trans_loss_func="l2norm", depth_loss_func="l1",
                          uv_loss_func="l2norm", kp2d_loss_func="l2norm", kp3d_loss_func="l2norm")
MASK_LOSS_FUNCS = ("mse_mean", "bce", "mse_sum")                       # :435-442
MODEL_OPTIONS = ("use_rootnet_with_reg_int_shared_backbone", "use_rootnet_with_reg_with_int_separate_backbone")       # :239
_WEIGHT_OPTIONS = dict(mask="mask_loss_weight", iou="iou_loss_weight", scale="scale_loss_weight", align="align_3d_loss_weight")  # :468


def check_sim2real_options(args):
    """NotImplementedError, naming the option, for what the step does not cover: a loss function outside the shipped ones
    (train_sim2real.py:317-388, 435-442) and the 5-tuple model branch (:244-251)."""
    for name, shipped in SHIPPED_LOSS_FUNCS.items():
        got = opt(args, name, shipped)
        if got != shipped:
            raise NotImplementedError(f"{name}={got!r}: the monitor kernel implements {name}={shipped!r} "
                                      "(every configs/*/self_supervised/*.yaml)")
    got = opt(args, "mask_loss_func", "mse_mean")
    if got not in MASK_LOSS_FUNCS:
        raise NotImplementedError(f"mask_loss_func={got!r}: the mask loss implements {MASK_LOSS_FUNCS}")
    flags = [opt(args, n) for n in MODEL_OPTIONS]
    if any(f is not None for f in flags) and not any(flags):
        raise NotImplementedError(f"{MODEL_OPTIONS[0]}=False and {MODEL_OPTIONS[1]}=False: the 5-tuple model branch "
                                  "(train_sim2real.py:244-251) is not built; the step takes an 8-tuple model")


def monitor_expr(pred, gt, K, image_size=256.0, mask_terms=None):
    """The twelve values of ``ROW`` as tensor expressions - train_sim2real.py:313-400 line by line, in the dtype of the inputs.
    The projection of transforms.py:17-21 is written out (the library's projection is a device kernel)."""
    pose, rot, trans, root_uv, depth, xyz_fk = pred[0], pred[1], pred[2], pred[3], pred[4], pred[7]
    K = K.reshape(-1, 3, 3).to(xyz_fk.dtype)
    S = float(image_size)
    t = {}
    t["loss_joint"] = torch.nn.functional.mse_loss(pose, gt["pose"])                                   # :321-322
    t["loss_rot"] = torch.nn.functional.mse_loss(rot, gt["root_rot"])                                  # :330-331
    t["loss_depth"] = torch.nn.functional.l1_loss(depth, gt["root_trans"][:, 2:3])                     # :337-338
    t["loss_uv"] = torch.mean(torch.norm((root_uv - gt["root_uv"]) / S, dim=1))                        # :350-353
    e = torch.norm(trans - gt["root_trans"], dim=1)                                                    # :364-370
    t["loss_trans"] = torch.where(e.mean() > 0.5, (e * torch.exp(-20.0 * e)).mean(), e.mean())
    t["loss_error3d"] = torch.mean(torch.norm(xyz_fk - gt["kp3d"], dim=2))                             # :374-377
    h = torch.einsum("bij,bkj->bki", K, xyz_fk)                                                        # :243; transforms.py:17-21
    uv = h[..., :2] / h[..., 2:3]
    m = gt["mask"]
    t["loss_error2d"] = torch.sum(torch.norm(uv / S - gt["kp2d"] / S, dim=2) * m) / torch.sum(m != 0)  # :381-386
    zero = torch.zeros((), dtype=xyz_fk.dtype, device=xyz_fk.device)
    mt = None if mask_terms is None else mask_terms.to(xyz_fk.dtype)
    t["loss"] = zero if mt is None else mt[0]                                                          # :402, 468
    for k, i in (("loss_mask", 1), ("loss_scale", 3), ("loss_iou", 2), ("loss_error3d_align", 4)):     # :399, 463-466
        t[k] = zero if mt is None else mt[i]
    return torch.stack([t[k].detach() for k in ROW])


class TrainMeters:
    """The twelve AverageValueMeters of the training loop (train_sim2real.py:638-640) as one device buffer: ``double sum[12]``
    followed by ``int64 count``.  hrp_sim2real_monitor adds a step's row to it (``sim2real_monitor(..., meters=this)``); nothing
    reaches the host until ``read_and_reset`` - the reference's twelve host copies per step (:649-660) are gone."""

    def __init__(self, device=None):
        self.device = torch.device(device if device is not None else "cuda")
        self.buffer = torch.zeros(13, dtype=torch.float64, device=self.device)

    @property
    def sum(self):
        return self.buffer[:12]

    @property
    def count(self):
        return self.buffer[12:].view(torch.int64)

    def add_host(self, row):
        """One step from tensor expressions (the host path of ``sim2real_monitor``)."""
        self.sum.add_(row.detach().to(self.device, torch.float64))
        self.count.add_(1)

    def read(self):
        """(dict of the twelve means under the names of ``ROW``, the number of steps they cover): ONE copy to the host.  No step:
        the means are NaN, as AverageValueMeter's."""
        host = self.buffer.cpu()
        n = int(host[12:].view(torch.int64)[0])
        s = host[:12].numpy()
        return {k: (float(s[i]) / n if n else float("nan")) for i, k in enumerate(ROW)}, n

    def reset(self):
        self.buffer.zero_()                                  # a memset on the stream: no synchronisation

    def read_and_reset(self):
        """The twelve means since the last reset (:663-674), then the reset of :675-686.  The read is the only synchronisation
        of the training loop's bookkeeping; the reference's loop wants it every tenth step (:662)."""
        means, _ = self.read()
        self.reset()
        return means


def sim2real_monitor(pred, gt, K, image_size=256.0, mask_terms=None, meters=None, rows=None, row_index=0):
    """The twelve values the self-supervised trainer logs for one step (train_sim2real.py:313-400, 463-468), detached as there.
    pred: the model's 8-tuple (pose, rot, trans, root_uv, depth, uvd, xyz_int, xyz_fk).  gt: dict(pose, root_rot, root_trans, root_uv,
    kp3d, kp2d, mask) as ``prepare_batch`` returns it.  K [B, 3, 3]: the "other" crop's intrinsics.  mask_terms: the five values
    ``sim2real_mask_loss`` computed (loss, mask, iou, scale, align) as one tensor, or None in validation, where the reference logs
    zeros and a zero loss (:399-402).  meters (a TrainMeters): the row is added to it.  rows [capacity, 12] float32: the row is also
    written at ``row_index`` (validation keeps one row per batch).
    -> (row [12] in the order of ``ROW``, dict of views under the reference's names).
    Device tensors: one hrp_sim2real_monitor launch; host tensors: the same arithmetic as tensor expressions."""
    pose, rot, trans, root_uv, depth, xyz_fk = pred[0], pred[1], pred[2], pred[3], pred[4], pred[7]
    B = pose.shape[0]
    if not pose.is_cuda:
        row = monitor_expr(pred, gt, K, image_size, mask_terms).float()
        if rows is not None:
            if not 0 <= row_index < rows.shape[0]:
                raise nv.HrpError(f"sim2real_monitor: row {row_index} of a capacity of {rows.shape[0]}")
            rows[row_index].copy_(row)
        if meters is not None:
            meters.add_host(row)
        return row, {k: row[i] for i, k in enumerate(ROW)}
    import ctypes as C
    dev = pose.device
    f32 = lambda t: t.detach().to(dev, torch.float32).contiguous()   # noqa: E731
    P, J = pose.shape[1], xyz_fk.shape[1]
    ins = dict(pose=f32(pose), rot=f32(rot), trans=f32(trans), root_uv=f32(root_uv), depth=f32(depth), xyz_fk=f32(xyz_fk),
               gt_pose=f32(gt["pose"]), gt_root_rot=f32(gt["root_rot"]), gt_root_trans=f32(gt["root_trans"]),
               gt_root_uv=f32(gt["root_uv"]), gt_kp3d=f32(gt["kp3d"]), gt_kp2d=f32(gt["kp2d"]), mask=f32(gt["mask"]), K=f32(K))
    shapes = dict(pose=(B, P), rot=(B, 6), trans=(B, 3), root_uv=(B, 2), depth=(B, 1), xyz_fk=(B, J, 3), gt_pose=(B, P),
                  gt_root_rot=(B, 6), gt_root_trans=(B, 3), gt_root_uv=(B, 2), gt_kp3d=(B, J, 3), gt_kp2d=(B, J, 2), mask=(B, J))
    for k, want in shapes.items():
        if tuple(ins[k].shape) != want:
            raise nv.HrpError(f"sim2real_monitor: {k} is {tuple(ins[k].shape)}, expected {want}")
    if ins["K"].numel() != 9 * B:
        raise nv.HrpError(f"sim2real_monitor: K is {tuple(ins['K'].shape)}, expected {(B, 3, 3)}")
    d = nv.Sim2RealMonitorDesc()
    for k, t in ins.items():
        setattr(d, k, t.data_ptr())
    if mask_terms is not None:
        mt = f32(mask_terms)
        if mt.shape != (5,):
            raise nv.HrpError(f"sim2real_monitor: mask_terms is {tuple(mt.shape)}, expected (5,)")
        ins["mask_terms"] = mt
        d.mask_terms = mt.data_ptr()
    row = torch.empty(12, dtype=torch.float32, device=dev)
    d.row = row.data_ptr()
    if meters is not None:
        if meters.buffer.device != dev:
            raise nv.HrpError(f"sim2real_monitor: the meters live on {meters.buffer.device}, the step on {dev}")
        d.meters = meters.buffer.data_ptr()
    if rows is not None:
        if rows.device != dev or rows.dtype != torch.float32 or rows.dim() != 2 or rows.shape[1] != 12 or not rows.is_contiguous():
            raise nv.HrpError(f"sim2real_monitor: rows must be a dense float32 [capacity, 12] tensor on {dev}")
        d.rows, d.row_index, d.capacity = rows.data_ptr(), int(row_index), rows.shape[0]
    d.B, d.P, d.J, d.image_size = B, P, J, float(image_size)
    nv.call("hrp_sim2real_monitor", C.byref(d), torch.cuda.current_stream(dev).cuda_stream)
    return row, {k: row[i] for i, k in enumerate(ROW)}


def worst_cases(dis3d, idx):
    """The "worst cases" list of train_sim2real.py:582-588: the pairs (dis3d, idx) sorted ascending as Python tuples, reversed, and
    positions 0, 5, ..., 95 taken -> (view_ids_list, errors_list).  DEVIATION: with fewer than 96 images the reference raises
    IndexError; here the list is cut to the positions that exist."""
    dis3d, idx = np.asarray(dis3d).reshape(-1), np.asarray(idx).reshape(-1)
    assert len(idx) == len(dis3d), (len(idx), len(dis3d))                                # :582
    result_ordered = sorted((dis3d[i].item(), idx[i].item()) for i in range(len(idx)))   # :583-584
    errors_down = [item[0] for item in result_ordered][::-1]
    view_ids_down = [item[1] for item in result_ordered][::-1]
    pos = [int(i) for i in np.arange(0, 100, 5) if i < len(idx)]                         # :587-588
    return [view_ids_down[i] for i in pos], [errors_down[i] for i in pos]


class Sim2RealEvaluator:
    """The accumulators of one validation epoch of the self-supervised trainer, on the device (reference train_sim2real.py:544-580:
    twelve AverageValueMeters, six lists and a host copy of everything per batch).  It composes ``function.Evaluator`` (the metrics
    of a batch are its one hrp_eval_batch launch) and adds ``image_ids`` [capacity] int64, filled per batch by a copy, and ``rows``
    [batch_capacity, 12], which hrp_sim2real_monitor fills at row ``reserve(B)``.  The host knows both counters, so growing needs
    no synchronisation."""

    def __init__(self, robot, capacity, reference_keypoint_id=3, device=None, batch_capacity=64):
        self.ev = F.Evaluator(robot, capacity, reference_keypoint_id=reference_keypoint_id, device=device, batch_capacity=batch_capacity)
        self.device, self.nkp, self.dof = self.ev.device, self.ev.nkp, self.ev.dof
        self.image_ids = torch.zeros(self.ev.capacity, dtype=torch.int64, device=self.device)
        self.rows = torch.zeros(self.ev.batch_capacity, 12, dtype=torch.float32, device=self.device)

    count = property(lambda self: self.ev.count)
    batches = property(lambda self: self.ev.batches)

    def reserve(self, B):
        """Make room for one more batch of B images -> the row of ``rows`` that batch owns."""
        n, nb = self.ev.count, self.ev.batches
        self.image_ids = grown(self.image_ids, 0, n, n + B)
        self.rows = grown(self.rows, 0, nb, nb + 1)
        return nb

    def add(self, pred, gt, image_id):
        """``function.Evaluator.add`` (pred / gt as there) plus the image ids of the batch.  Call it after the monitor launch that
        wrote ``rows[reserve(B)]``.  Returns the reference's metric_dict (:299-304) of this batch: device tensors, ``idx`` included."""
        B = pred["kp3d_fk"].shape[0]
        self.reserve(B)
        o = self.ev.count
        md = dict(self.ev.add(pred, gt))
        ids = torch.as_tensor(image_id).reshape(-1).to(torch.int64)
        assert ids.shape[0] == B, (ids.shape, B)
        self.image_ids[o:o + B].copy_(ids, non_blocking=True)
        md["idx"] = self.image_ids[o:o + B]
        return md

    def _host(self):
        n, nb = self.ev.count, self.ev.batches
        assert n > 0 and nb > 0, "Sim2RealEvaluator: nothing was added"
        return self.image_ids[:n].cpu().numpy(), self.rows[:nb].cpu().double().numpy()

    def worst_cases(self):
        """``worst_cases`` of this epoch's (image_dis3d_avg, image id) pairs, on the host after one copy of the two arrays."""
        ids, _ = self._host()
        return worst_cases(self.ev.per_image[0, :self.ev.count].cpu().numpy(), ids)

    def summary(self):
        """The one synchronisation of the epoch: the accumulators come to the host in one piece each.  Returns ``summary_add_pck``
        of the FK branch at the top level and of the integral branch under ``'integral'`` (:594-595), ``'mean_joint_error'`` in
        degrees (:596), and
          'meters'       the AverageValueMeter means (unweighted means over batches, fp64, in batch order) of the twelve ``ROW``
                         values (:558-569), 'rotation_diff', and the per-key-point / per-joint vectors 'dis3d', 'dis2d',
                         'dis3d_int', 'dis2d_int', 'l1_joint' (:576-580);
          'image_ids'    the image ids in the order they were added;
          'worst_cases'  ``worst_cases()``: (view_ids_list, errors_list)."""
        ids, rows = self._host()
        s = self.ev.summary()
        out = {k: v for k, v in s.items() if k not in ("meters", "relative", "mean_depth_error", "relative_depth_error", "Relative_ADD/AUC")}
        means = meter_mean(rows)
        meters = {k: float(means[i]) for i, k in enumerate(ROW)}
        for k in ("rotation_diff", "dis3d", "dis2d", "dis3d_int", "dis2d_int", "l1_joint"):
            meters[k] = s["meters"][k]
        out["meters"] = meters
        out["image_ids"] = ids
        out["worst_cases"] = worst_cases(self.ev.per_image[0, :self.ev.count].cpu().numpy(), ids)
        return out


def renderer_for(robot, K_original, device, mesh=None, scale=0.5, original_image_size=(480, 640), sigma=None):
    """The renderer of train_sim2real.py:406-408 for the camera ``K_original`` [3, 3], cached on ``robot`` per (the nine values of
    K_original, device).  DEVIATION: the reference rebuilds its two renderers, and reloads every .obj, on every step; here the
    first call for a camera builds the renderer (``robot.set_robot_renderer``; ``mesh``, ``scale``, ``original_image_size`` and
    ``sigma`` are its and the renderer's arguments) and every later call for that camera returns the same object, whatever else it
    passes.  A K_original that lives on the device is read back for the key (one synchronisation); loaders hand it over on the host."""
    Kh = torch.as_tensor(K_original).detach()
    key = (tuple(float(v) for v in Kh.reshape(-1).cpu().tolist()), str(torch.device(device)))
    cache = robot.__dict__.setdefault("_sim2real_renderers", {})
    if key not in cache:
        r = robot.set_robot_renderer(Kh.cpu(), original_image_size=original_image_size, scale=scale, device=device, mesh=mesh)
        if sigma is not None:
            r.sigma, r.blur_radius = float(sigma), float(np.log(1.0 / 1e-4 - 1.0) * sigma)
        cache[key] = r
    return cache[key]


_MODE_LISTS = weakref.WeakKeyDictionary()      # model -> (runtime.MODE_EPOCH, its BatchNorm modules, its other modules)


def set_step_modes(model, train):
    """``model.train()`` / ``model.eval()``, then every BatchNorm1d / BatchNorm2d in ``eval()`` (train_sim2real.py:139-146), on every
    call.  When every module already has the mode that leaves it with - every step after the first - nothing is called: a train() call
    on a PlannedModule invalidates the plan cache's BatchNorm signature (runtime.MODE_EPOCH), and two walks over every module
    of the full network plus that rebuild cost several ms of host time per step.  The module lists are cached per
    MODE_EPOCH, as runtime.py caches its own: a module added to the tree is seen after the next train() / eval() call."""
    from hrpe_amd.runtime import MODE_EPOCH
    bn = (torch.nn.BatchNorm2d, torch.nn.BatchNorm1d)
    c = _MODE_LISTS.get(model)
    if c is None or c[0] != MODE_EPOCH[0]:
        bns, others = [], []
        for m in model.modules():
            (bns if isinstance(m, bn) else others).append(m)
        c = (MODE_EPOCH[0], bns, others)
        _MODE_LISTS[model] = c
    train = bool(train)
    if all(m.training == train for m in c[2]) and not any(m.training for m in c[1]):
        return
    model.train(train)                                                                                   # :139-142
    for m in c[1]:                                                                                       # :144-146
        m.eval()
    _MODE_LISTS[model] = (MODE_EPOCH[0], c[1], c[2])


def _mask_terms(loss, terms):
    """(loss, mask, iou, scale, align) of ``sim2real_mask_loss`` as one tensor.  On the device the four terms are views of the five
    floats hrp_sim2real_loss wrote: that buffer itself, no launch."""
    base = getattr(terms["loss_mask"], "_base", None)
    if base is not None and tuple(base.shape) == (5,):
        return base
    return torch.stack([t.detach().reshape(()) for t in (loss, terms["loss_mask"], terms["loss_iou"], terms["loss_scale"],
                                                         terms["loss_error3d_align"])])


def farward_loss(args, input_batch, device, model, robot, seg_net, train=True, evaluator=None, meters=None):
    """The reference's nested step function (train_sim2real.py:137-534; its spelling; ``robot`` and ``seg_net`` are closure
    variables there): ``(loss, loss_dict)`` when training, plus ``metric_dict`` (device tensors) when not.

    Batch unpacking is ``prepare_batch``; every BatchNorm1d / BatchNorm2d is put in eval() on every call (:144-146).  Training:
    ``seg_net(images_original_255).detach()``, the rendered masks of the predicted pose at the root key-point (one launch chain for
    the batch), ``sim2real_mask_loss`` with the four ``*_loss_weight`` options - the returned ``loss`` is exactly its loss - and one
    hrp_sim2real_monitor launch for ``loss_dict`` (eleven detached device scalars, the names of :395-400) and for ``meters`` (a
    TrainMeters).  Validation: one monitor launch (zero mask terms and a zero loss, :399-402) and one hrp_eval_batch launch into
    ``evaluator`` (a Sim2RealEvaluator; validate passes the epoch's; without one the metrics of this batch alone are computed).
    The renderer comes from ``renderer_for`` (cached per camera; the reference rebuilds it per step).  Only 8-tuple models are
    accepted; the 5-tuple branch and a loss function outside the shipped ones raise NotImplementedError naming the option.  The model
    is called as it is (bring it to ``device`` - and wrap it for several GPUs, hrpe_amd.parallel - before)."""
    check_sim2real_options(args)
    set_step_modes(model, train)                                                                         # :139-146
    st = pose_step_inputs(args, input_batch, model, robot, device, rotation_dim=6, evaluate=not train)   # :151-311
    p, gt, pred, pred_pose, root = st.p, st.gt, st.pred, st.pred_pose, st.root
    if len(pred) != 8:
        raise NotImplementedError(f"the model returned {len(pred)} values: the 5-tuple model branch (train_sim2real.py:244-251, "
                                  f"{MODEL_OPTIONS[0]}=False and {MODEL_OPTIONS[1]}=False) is not built; the step takes an 8-tuple model")
    mon_pred = (pred_pose,) + pred[1:]
    image_size = float(opt(args, "image_size", 256.0))
    if not train:                                                                                        # :265-304
        B = pred_pose.shape[0]
        if evaluator is None:
            evaluator = Sim2RealEvaluator(robot, B, reference_keypoint_id=root, device=device, batch_capacity=1)
        row_index = evaluator.reserve(B)                  # (may reallocate evaluator.rows)
        row, terms = sim2real_monitor(mon_pred, gt, p["other_K"], image_size, mask_terms=None, rows=evaluator.rows, row_index=row_index)
        metric_dict = evaluator.add(st.ev_pred, st.ev_gt, input_batch["image_id"])
        return row[0], {k: terms[k] for k in LOSS_KEYS}, metric_dict                                     # :402, 534
    if opt(args, "known_joint", False):                                                                  # :404-405
        pred_pose = gt["pose"].clone()
    images_original = torch.as_tensor(input_batch["images_original"]).to(device, non_blocking=True)
    images_original_255 = images_original.float()        # :158-159 (x / 255 * 255 of a 0..255 value)
    K0 = torch.as_tensor(input_batch["K_original"])[0]
    renderer = renderer_for(robot, K0, device)                                                           # :406-408
    seg_masks = seg_net(images_original_255).detach()                                                    # :412
    rendered_masks = robot.get_rendered_masks(pred_pose, pred[1], pred[2], renderer, root=root)          # :414-416, 434
    weights = {k: float(opt(args, name, F.SIM2REAL_YAML_WEIGHTS[k])) for k, name in _WEIGHT_OPTIONS.items()}
    loss, mterms = F.sim2real_mask_loss(rendered_masks, seg_masks, pred[7], pred[6], opt(args, "mask_loss_func", "mse_mean"),
                                        weights)                                                         # :435-468
    _, terms = sim2real_monitor(mon_pred, gt, p["other_K"], image_size, mask_terms=_mask_terms(loss, mterms), meters=meters)
    return loss, {k: terms[k] for k in LOSS_KEYS}                                                        # :532


ADD_THRESHOLDS = F.ADD_THRESHOLDS                                     # :549-550
PCK_THRESHOLDS = F.PCK_THRESHOLDS


def validate(args, epoch_log, dsname, loader, model, robot, seg_net, writer, device, get_lowest=False, view_ids=None, errors=None,
             epoch=None):
    """The reference's nested validation loop (train_sim2real.py:536-625; ``loader`` is the data loader its ``ds`` selects,
    ``model``, ``robot``, ``seg_net``, ``writer``, ``device`` are closure variables there): one farward_loss(train=False) per batch
    into one Sim2RealEvaluator - nothing reaches the host inside the loop - and one summary at the end.  ``get_lowest=True`` (the
    dataset must be one of ``args.train_ds_names``, :537-539): returns ``(view_ids_list, errors_list)``, the worst cases the epoch loop
    feeds back in (:627-634); with fewer than 96 images the list is cut to the positions that exist.  Otherwise every scalar of
    :597-623 is logged under its tag - the two ``*_integral_xyz_metrics`` tags at ``epoch`` (the epoch loop's variable there; default
    ``epoch_log``), the rest at ``epoch_log`` - and ``(ADD/AUC, mean loss)`` is returned.  ``writer`` may be None.  ``view_ids`` and
    ``errors`` only steer the reference's visualisation, which is out of scope: accepted and unused.  A loader over this project's
    DreamDataset (host items with ``frame`` / ``aug``) goes through ``DreamDataset.to_device`` first.  The model is left in
    train() in both cases (the reference returns the worst cases before its model.train(), and the loop that follows sets it)."""
    if get_lowest:
        assert dsname in args.train_ds_names, dsname                                                     # :537-539
    ds = "_" + dsname
    model.eval()
    ev = Sim2RealEvaluator(robot, loader_capacity(loader), reference_keypoint_id=args.reference_keypoint_id, device=device)
    with torch.no_grad():
        for sample in validation_batches(loader, device):
            farward_loss(args=args, input_batch=sample, device=device, model=model, robot=robot, seg_net=seg_net, train=False,
                         evaluator=ev)
    model.train()                                                                                        # :624
    if get_lowest:                                                                                       # :591-592
        return ev.worst_cases()
    s = ev.summary()
    if writer is not None:
        m = s["meters"]
        at = epoch_log if epoch is None else epoch
        add = lambda tag, v, e=epoch_log: writer.add_scalar(tag + ds, float(v), e)   # noqa: E731
        add("Val/loss", m["loss"])                                                                       # :597-608
        add("Val/mask_loss", m["loss_mask"])
        add("Val/scale_loss", m["loss_scale"])
        add("Val/align_loss", m["loss_error3d_align"])
        add("Val/iou_loss", m["loss_iou"])
        add("Val/pose_loss", m["loss_joint"])
        add("Val/rot_loss", m["loss_rot"])
        add("Val/trans_loss", m["loss_trans"])
        add("Val/uv_loss", m["loss_uv"])
        add("Val/depth_loss", m["loss_depth"])
        add("Val/error2d_loss", m["loss_error2d"])
        add("Val/error3d_loss", m["loss_error3d"])
        log_pose_validation(add, s, ev.nkp, ev.dof, integral_details=False, integral_epoch=at)           # :609-623
    return s["ADD/AUC"], s["meters"]["loss"]
