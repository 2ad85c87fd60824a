"""Streaming pose tracker: the deployment counterpart of the three trainers.  A camera frame and the intrinsics go in, a pose comes
out, and the crop of the NEXT frame is taken from this frame's estimate - all on the device (csrc/track.hip).

The reference's loader crops around ANNOTATED key-points (lib/dataset/dream.py:171-216, 287-394; roboutils.py:59-156, 224-257;
lib/utils/geometries.py:360-395) and its step derives ``k_values`` from the annotated boxes (lib/core/function.py:43-48, 88-98).
``PoseTracker`` runs the same arithmetic on the key-points the model predicted for the previous frame:

* ``prepare``  one launch (``hrp_track_prepare``): crop box, canvas, both views' K and boxes, ``k_values`` from the state, and the
  crop + bilinear resize of both views straight from the frame;
* the model    ``model(reg_images, root_images, k_values, other_K)``, ``RootNetwithRegInt.forward``'s signature, ``xyz_fk`` last;
* ``update``   one launch (``hrp_track_update``): ``xyz_fk`` projected with ``K_original`` becomes the state.

Nothing crosses PCIe except the frame, nothing here synchronises or reads a device value, every buffer is owned by the tracker and
reused, so ``prepare`` and ``update`` can be captured in a graph.  A stream without a usable estimate (none yet, a box the loader
would refuse, a prediction behind the camera or outside the frame) takes the whole frame and says so in ``status``; it recovers
as soon as a prediction is usable again, or - the networks were trained on tight crops - at the next ACQUISITION: ``acquire`` runs a
full-frame detector (CtRNet's ``seg_mask_inference.detect``) and one launch (``hrp_track_seed``) makes its key-points the estimate of
the streams that have none; ``step`` schedules it every ``acquire_every`` frames.  With ``min_support`` / ``min_coverage`` /
``min_iou`` one more launch in between (``hrp_track_verify``) drops the estimate of a stream that the detector's mask contradicts.  ``process_truncation`` is not part of the tracker: it crops inside the frame.  There is
no CPU path: CPU tensors raise HrpError."""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from hrpe_amd import _native as nv

TrackResult = namedtuple("TrackResult", "pose rot trans kp3d kp2d_original depth status k_values")


class PoseTracker:
    STATE_DTYPE = torch.float64

    def __init__(self, model, robot, K_original, frame_hw, streams=1, rootnet_resize_hw=(256, 256), other_resize_hw=(256, 256),
                 extend_ratio=(0.2, 0.13), use_origin_bbox=False, use_extended_bbox=True, reference_keypoint_id=3, min_inside=1,
                 device=None, detector=None, detector_scale=0.5, acquire_every=0, min_support=None, min_coverage=None, min_iou=None,
                 bones=None, verify_samples=16, verify_min_fg=16, verify_min_samples=4, verify_min_prob=0.5, renderer=None, filter=None,
                 crop_from_prediction=False, refit=None):
        """model: a callable with RootNetwithRegInt.forward's signature returning its tuple (xyz_fk last); a module is put in
        eval().  robot: its ``nkp`` (or ``link_names``) gives the number of key-points.  K_original: [3, 3] or [streams, 3, 3].
        frame_hw: (H, W) of every frame.  The bbox options select the box and K of ``k_values`` as prepare_batch does
        (use_extended_bbox first, then use_origin_bbox, else the strict box).  reference_keypoint_id is the model's root key-point,
        kept for the caller.  min_inside: how many predicted key-points must lie in the frame for the estimate to be used.
        detector: a callable uint8 [B, 3, H, W] -> (key-points [B, nkp, 2] fp32 in ITS pixels, foreground probability [B, 1, h, w] /
        [B, h, w] or None, ms [B, nkp, 2] or None), e.g. ``seg_mask_inference.detect``; detector_scale: detector pixels per frame
        pixel (a number or (x, y); seg_mask_inference's ``scale``); acquire_every: ``step`` runs ``acquire`` on every
        acquire_every-th frame (0: never).
        min_support / min_coverage / min_iou: thresholds in [0, 1] of the verification that ``acquire`` runs between the detector
        and ``seed`` (``verify``, include/hrp.h hrp_track_verify); verification is on when any of them is given.  bones: key-point
        index pairs the support samples lie along (default: the serial chain (i, i + 1) for panda and kuka, none otherwise);
        verify_samples per bone; verify_min_fg foreground pixels below which the detector is taken to see no robot;
        verify_min_samples support samples inside the map below which support is not applied; verify_min_prob the foreground
        probability.  renderer: a RobotMeshRenderer at the detector's resolution (``robot.set_robot_renderer(K_original, frame_hw,
        scale=detector_scale)``), needed by min_iou and only by it: the silhouette of the last prediction is rendered on
        acquisition frames.
        refit: a ``kinfit.KinematicRefit``, a ``kinfit.MultiViewRefit`` or None.  With a MultiViewRefit the ``streams`` are its
        ``views``: V fixed, calibrated cameras on ONE arm.  ``step`` projects each stream's ``kp3d_int`` with that stream's
        K_original, solves the joints once over all streams (``hrp_kin_solve_views``) from the mean of the model's ``pose`` over the
        streams, and gives every stream the same joints, its own calibrated ``(rot, trans)`` in the model's rotation representation
        and its own camera's key-points, so each stream's next crop comes from the joint estimate as its camera sees it; the
        KinViewsResult is left in ``refit_result``; a filter together with it raises (there is no multi-view filter).
        With a KinematicRefit, ``step`` projects the integral head's key-points (``kp3d_int``, the
        model's output before ``xyz_fk``) to 2-D targets, refits the model's ``(pose, rot, trans)`` to them (one more launch pair:
        ``hrp_project_fwd``, ``hrp_kin_solve``) and tracks the refit's key-points; the KinResult is left in ``refit_result``.  In
        "holistic" mode the targets and the solve use the crop's ``other_K``; in "fixed_camera" mode ``K_original`` (cropping changes
        K, not the camera frame).  None: exactly the launches of a tracker without the argument.
        filter: a ``kinfit.KinematicFilter`` with ``streams`` streams, or None; not together with refit.  With one, ``step`` projects
        ``kp3d_int`` as the refit does, steps the filter with the model's ``(pose, rot, trans)`` as its inputs (``pose`` is also the
        joints' measurement when the filter has w_q) and with a copy of ``have`` taken right after ``prepare`` as ``keep`` - a stream
        that just lost or re-acquired its estimate starts its filter again - and tracks the filter's key-points; the
        KinFilterResult is left in ``filter_result``.  crop_from_prediction (with a filter only): the next crop comes from the
        filter's prediction of the next frame's key-points (``kp3d_next``, one more ``hrp_track_update``), not from this frame's,
        which removes the one-frame lag of the crop; ``kp2d_predicted`` holds their projection.  filter=None: exactly the launches of
        a tracker without the argument."""
        if refit is not None and not (hasattr(refit, "solve") and hasattr(refit, "mode")):
            raise nv.HrpError("PoseTracker: refit must be a kinfit.KinematicRefit, a kinfit.MultiViewRefit or None")
        if filter is not None and not (hasattr(filter, "step") and hasattr(filter, "mode") and hasattr(filter, "valid")):
            raise nv.HrpError("PoseTracker: filter must be a kinfit.KinematicFilter or None")
        if filter is not None and refit is not None:
            raise nv.HrpError("PoseTracker: filter and refit are mutually exclusive (the filter's update is the refit with a state prior)")
        if crop_from_prediction and filter is None:
            raise nv.HrpError("PoseTracker: crop_from_prediction needs a filter (it is the filter that predicts)")
        if refit is not None and refit.mode == "multi_view" and int(refit.views) != int(streams):
            raise nv.HrpError(f"PoseTracker: the refit has {refit.views} views, the tracker {int(streams)} streams (one stream per camera)")
        if filter is not None and int(filter.B) != int(streams):
            raise nv.HrpError(f"PoseTracker: the filter has {filter.B} streams, the tracker {int(streams)}")
        self.refit, self.refit_result = refit, None
        self.filter, self.filter_result, self.crop_from_prediction = filter, None, bool(crop_from_prediction)
        ds = tuple(detector_scale) if isinstance(detector_scale, (tuple, list)) else (detector_scale, detector_scale)
        if len(ds) != 2 or not all(np.isfinite(float(v)) and float(v) > 0 for v in ds):
            raise nv.HrpError(f"PoseTracker: detector_scale {detector_scale!r}, want one or two positive numbers")
        if int(acquire_every) < 0 or (int(acquire_every) > 0 and detector is None):
            raise nv.HrpError(f"PoseTracker: acquire_every {acquire_every!r} (>= 0, and > 0 only with a detector)")
        self.detector, self.acquire_every, self._frame = detector, int(acquire_every), 0
        thresholds = dict(min_support=min_support, min_coverage=min_coverage, min_iou=min_iou)
        for name, v in thresholds.items():
            if v is not None and not 0.0 <= float(v) <= 1.0:           # (false for NaN)
                raise nv.HrpError(f"PoseTracker: {name} {v!r}, want a number in [0, 1] or None")
        self.verifying = any(v is not None for v in thresholds.values())
        if self.verifying and detector is None:
            raise nv.HrpError("PoseTracker: min_support / min_coverage / min_iou need a detector")
        if (min_iou is None) != (renderer is None):
            raise nv.HrpError("PoseTracker: min_iou and renderer go together (the silhouette is rendered for the IoU only)")
        if renderer is not None and np.asarray(K_original).size != 9:
            raise nv.HrpError("PoseTracker: renderer with a per-stream K_original (the renderer has one camera)")
        self.renderer, self._last = renderer, None
        if self.verifying or bones is not None:
            nkp = int(getattr(robot, "nkp", None) or len(robot.link_names))
            if bones is None:
                bones = [(i, i + 1) for i in range(nkp - 1)] if getattr(robot, "robot_type", None) in ("panda", "kuka") else []
            bones = [tuple(int(i) for i in b) for b in bones]
            if len(bones) > nv.TRACK_MAX_BONES or any(len(b) != 2 or not all(0 <= i < nkp for i in b) for b in bones):
                raise nv.HrpError(f"PoseTracker: bones {bones!r}, want at most {nv.TRACK_MAX_BONES} pairs of key-point indices below {nkp}")
            if not 1 <= int(verify_samples) <= nv.TRACK_MAX_SAMPLES:
                raise nv.HrpError(f"PoseTracker: verify_samples {verify_samples!r}, want 1 .. {nv.TRACK_MAX_SAMPLES}")
        self._verify = dict(thresholds, bones=bones or [], samples=int(verify_samples), min_fg=int(verify_min_fg),
                            min_samples=int(verify_min_samples), min_prob=float(verify_min_prob), scale=(float(ds[0]), float(ds[1])))
        self._inv_scale = (C.c_double * 2)(1.0 / float(ds[0]), 1.0 / float(ds[1]))       # frame pixels per detector pixel
        device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if device.type != "cuda":
            raise nv.HrpError(f"PoseTracker: {device} is not a GPU (there is no CPU path)")
        nv.lib()
        self.device, self.model, self.robot = device, model, robot
        if isinstance(model, torch.nn.Module):
            model.eval()
        self.nkp = int(getattr(robot, "nkp", None) or len(robot.link_names))
        self.B, (self.H, self.W) = int(streams), (int(frame_hw[0]), int(frame_hw[1]))
        self.root_hw = (int(min(rootnet_resize_hw)), int(max(rootnet_resize_hw)))
        self.other_hw = (int(min(other_resize_hw)), int(max(other_resize_hw)))
        self.bbox_mode = nv.TRACK_BBOX_EXTENDED if use_extended_bbox else (nv.TRACK_BBOX_ORIGIN if use_origin_bbox else nv.TRACK_BBOX_STRICT)
        self.reference_keypoint_id, self.min_inside = int(reference_keypoint_id), int(min_inside)
        self._extend = (C.c_double * 2)(float(extend_ratio[0]), float(extend_ratio[1]))
        if not (1 <= self.nkp <= nv.TRACK_MAX_KP) or self.B < 1:
            raise nv.HrpError(f"PoseTracker: {self.nkp} key-points (1 .. {nv.TRACK_MAX_KP}), {self.B} streams")
        for v in (self.H, self.W) + self.root_hw + self.other_hw:
            if not (1 <= v <= nv.TRACK_MAX_SIZE):
                raise nv.HrpError(f"PoseTracker: size {v}, want 1 .. {nv.TRACK_MAX_SIZE}")
        K = torch.as_tensor(np.asarray(K_original, dtype=np.float64)).reshape(-1, 9)
        if K.shape[0] not in (1, self.B):
            raise nv.HrpError(f"PoseTracker: K_original for {K.shape[0]} streams, want 1 or {self.B}")
        B, new = self.B, lambda *s, dt: torch.zeros(*s, dtype=dt, device=device)      # noqa: E731
        self.K_original = K.expand(B, 9).to(device=device, dtype=torch.float32).contiguous()
        self.kp2d, self.have = new(B, self.nkp, 2, dt=torch.float64), new(B, dt=torch.int32)
        self.root_images = new(B, 3, *self.root_hw, dt=torch.uint8)
        self.same = self.root_hw == self.other_hw              # one size: written once and aliased, as DreamDataset.to_device does
        self.reg_images = self.root_images if self.same else new(B, 3, *self.other_hw, dt=torch.uint8)
        self.root_K, self.other_K = new(B, 3, 3, dt=torch.float32), new(B, 3, 3, dt=torch.float32)
        self.k_values, self.status = new(B, dt=torch.float32), new(B, dt=torch.int32)
        self.geom = new(B, C.sizeof(nv.TrackGeom), dt=torch.uint8)                       # hrp_track_geom records
        self._geom_status = self.geom.view(torch.int32)[:, 0]
        self.kp2d_original = new(B, self.nkp, 2, dt=torch.float32)
        self.jpeg_status = None
        self.seed_status = new(B, dt=torch.int32)
        self.verify_status, self.verify_counts = new(B, dt=torch.int32), new(B, 4, dt=torch.int32)
        self.verify_sums = new(B, 3, dt=torch.float64)
        if filter is not None:
            self._keep = new(B, dt=torch.int32)
            self.kp2d_predicted = new(B, self.nkp, 2, dt=torch.float32)

    def reset(self, kp2d=None, streams=None):
        """Seed the estimate: kp2d [B, nkp, 2] in original-image pixels (float64 is kept bit for bit), or None for no estimate.
        streams: the indices it applies to (kp2d then has one row per index); the other streams keep their state.  Dropping an
        estimate also restarts the host frame count of ``acquire_every``: the next ``step`` runs the detector."""
        idx = torch.arange(self.B) if streams is None else torch.as_tensor(list(streams), dtype=torch.int64)
        idx = idx.to(self.device)
        if kp2d is None:
            self.have.index_fill_(0, idx, 0)
            self._frame = 0                  # the next step is a scheduled detection again (acquire_every)
            return
        kp = torch.as_tensor(kp2d, dtype=torch.float64).to(self.device)
        if tuple(kp.shape) != (idx.numel(), self.nkp, 2):
            raise nv.HrpError(f"PoseTracker.reset: kp2d {tuple(kp.shape)}, want {(idx.numel(), self.nkp, 2)}")
        self.kp2d.index_copy_(0, idx, kp)
        self.have.index_fill_(0, idx, 1)
        self._last = None                    # the state is no longer the last prediction: no silhouette at the next verification

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _check_frames(self, frames):
        if not isinstance(frames, torch.Tensor) or not frames.is_cuda or frames.dtype != torch.uint8:
            raise nv.HrpError("PoseTracker: frames must be a uint8 GPU tensor (there is no CPU path)")
        if tuple(frames.shape) != (self.B, self.H, self.W, 3):
            raise nv.HrpError(f"PoseTracker: frames {tuple(frames.shape)}, want {(self.B, self.H, self.W, 3)}")

    def seed(self, det_kp, mask=None, ms=None, force=False, min_inside=None, min_prob=0.5, min_peak=0.0):
        """One launch (``hrp_track_seed``): the detector's key-points [B, nkp, 2] fp32 (its pixels) become the estimate of the streams
        that have none (force: of every stream).  A key-point counts when it is finite, lies in the frame, the mask [B, 1, h, w] /
        [B, h, w] (if given) is >= min_prob at its detector pixel and its peak probability 1 / ms[..., 1] (if given) is >= min_peak;
        a stream takes the detection when all its key-points are finite and at least min_inside (default: the tracker's) count.
        Returns ``seed_status`` [B] int32 (_native.SEED_SKIPPED / SEED_TAKEN / SEED_REFUSED), the tracker's own buffer."""
        def dev32(t, shapes, what):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise nv.HrpError(f"PoseTracker.seed: {what} must be a GPU tensor (there is no CPU path)")
            if tuple(t.shape) not in shapes:
                raise nv.HrpError(f"PoseTracker.seed: {what} {tuple(t.shape)}, want {shapes[0]}")
            return t.detach().float().contiguous()
        kp = dev32(det_kp, [(self.B, self.nkp, 2)], "key-points")
        hm = wm = 0
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or mask.dim() not in (3, 4) or mask.shape[0] != self.B:
                raise nv.HrpError(f"PoseTracker.seed: mask {tuple(mask.shape)}, want [B, 1, h, w] or [B, h, w]")
            hm, wm = int(mask.shape[-2]), int(mask.shape[-1])
            mask = dev32(mask, [(self.B, 1, hm, wm), (self.B, hm, wm)], "mask")
        if ms is not None:
            ms = dev32(ms, [(self.B, self.nkp, 2)], "ms")
        nv.call("hrp_track_seed", kp.data_ptr(), self.B, self.nkp, self._inv_scale, None if mask is None else mask.data_ptr(), hm, wm,
                float(min_prob), None if ms is None else ms.data_ptr(), float(min_peak),
                self.min_inside if min_inside is None else int(min_inside), 1 if force else 0, self.W, self.H, self.kp2d.data_ptr(),
                self.have.data_ptr(), self.seed_status.data_ptr(), self._stream())
        return self.seed_status

    def verify(self, mask, alpha=None):
        """One launch (``hrp_track_verify``): every stream's estimate against the detector's foreground probability ``mask``
        [B, 1, h, w] / [B, h, w] - the skeleton's support on the foreground (min_support), the foreground's coverage by the
        estimate's box (min_coverage) and, with ``alpha`` [B, h, w] (the soft silhouette of the last prediction), their IoU
        (min_iou).  A stream that fails an enabled criterion loses its estimate (``have`` = 0), so that a ``seed`` that follows takes
        the detection.  Returns ``verify_status`` [B] int32 (_native.VERIFY_*), the tracker's own buffer; ``verify_counts`` [B, 4] =
        (h_s, n_s, n_in, n_fg) and ``verify_sums`` [B, 3] float64 = (I, S, R) hold what was measured."""
        def dev32(t, what):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise nv.HrpError(f"PoseTracker.verify: {what} must be a GPU tensor (there is no CPU path)")
            if t.dim() not in (3, 4) or t.shape[0] != self.B or (t.dim() == 4 and t.shape[1] != 1):
                raise nv.HrpError(f"PoseTracker.verify: {what} {tuple(t.shape)}, want [B, 1, h, w] or [B, h, w]")
            return t.detach().float().contiguous()
        mask = dev32(mask, "mask")
        hm, wm = int(mask.shape[-2]), int(mask.shape[-1])
        if alpha is not None:
            alpha = dev32(alpha, "alpha")
            if tuple(alpha.shape[-2:]) != (hm, wm):
                raise nv.HrpError(f"PoseTracker.verify: alpha {tuple(alpha.shape)} and mask {tuple(mask.shape)} differ in size")
        v, d = self._verify, nv.TrackVerifyDesc()
        d.state_kp2d, d.state_have, d.mask = self.kp2d.data_ptr(), self.have.data_ptr(), mask.data_ptr()
        d.alpha = None if alpha is None else alpha.data_ptr()
        d.verify_status, d.counts, d.sums = self.verify_status.data_ptr(), self.verify_counts.data_ptr(), self.verify_sums.data_ptr()
        d.B, d.nkp, d.hm, d.wm = self.B, self.nkp, hm, wm
        d.nb, d.samples, d.min_fg, d.min_samples, d.min_prob = len(v["bones"]), v["samples"], v["min_fg"], v["min_samples"], v["min_prob"]
        for i, (a, b) in enumerate(v["bones"]):
            d.bones[i][0], d.bones[i][1] = a, b
        d.scale[0], d.scale[1] = v["scale"]
        d.extend_ratio[0], d.extend_ratio[1] = self._extend[0], self._extend[1]
        off = lambda t: -1.0 if t is None else float(t)   # noqa: E731
        d.min_support, d.min_coverage = off(v["min_support"]), off(v["min_coverage"])
        d.min_iou = off(v["min_iou"]) if alpha is not None else -1.0
        nv.call("hrp_track_verify", C.byref(d), self._stream())
        return self.verify_status

    def _silhouette(self, hm, wm):
        """The soft silhouette [B, hm, wm] of the last prediction, or None when the state is not a prediction."""
        if self.renderer is None or self._last is None:
            return None
        if tuple(self.renderer.image_size) != (hm, wm):
            raise nv.HrpError(f"PoseTracker.acquire: the renderer draws {tuple(self.renderer.image_size)}, the detector's mask is {(hm, wm)}")
        pose, rot, trans = self._last
        if rot.dim() != 2 or rot.shape[1] != 6:
            raise nv.HrpError(f"PoseTracker.acquire: rotations {tuple(rot.shape)}, the renderer takes the 6-D form")
        with torch.no_grad():
            return self.robot.get_rendered_masks(pose, rot, trans, self.renderer, root=self.reference_keypoint_id)

    def acquire(self, frames, force=False, min_inside=None, min_prob=0.5, min_peak=0.0):
        """Run the detector on the frames (uint8 [B, H, W, 3] on the device) and seed the streams without an estimate from it
        (``seed``).  With verification on (and not forced) ``verify`` runs in between, so a stream whose estimate disagrees with the
        detector's mask takes this frame's detection in the same call.  Returns ``seed_status``; never synchronises.  The
        NHWC -> NCHW view the detector takes is a torch copy."""
        if self.detector is None:
            raise nv.HrpError("PoseTracker.acquire: the tracker was built without a detector")
        self._check_frames(frames)
        with torch.no_grad():
            kp, mask, ms = self.detector(frames.permute(0, 3, 1, 2).contiguous())
        if self.verifying and not force:
            if not isinstance(mask, torch.Tensor) or mask.dim() not in (3, 4):
                raise nv.HrpError("PoseTracker.acquire: verification needs the detector's foreground mask, and it returned none")
            self.verify(mask, self._silhouette(int(mask.shape[-2]), int(mask.shape[-1])))
        return self.seed(kp, mask, ms, force=force, min_inside=min_inside, min_prob=min_prob, min_peak=min_peak)

    def prepare(self, frames):
        """frames: uint8 [B, H, W, 3] on the device.  Returns the model's inputs (tensors owned by the tracker, rewritten by the
        next call): root_images / reg_images uint8 [B, 3, h, w], root_K / other_K [B, 3, 3], k_values [B], geom [B, 112] uint8
        (hrp_track_geom records: crop box, canvas, boxes, status)."""
        self._check_frames(frames)
        frames = frames.contiguous()
        nv.call("hrp_track_prepare", frames.data_ptr(), self.kp2d.data_ptr(), self.have.data_ptr(), self.K_original.data_ptr(), self.B,
                self.H, self.W, self.nkp, self.root_images.data_ptr(), self.root_hw[0], self.root_hw[1],
                None if self.same else self.reg_images.data_ptr(), self.other_hw[0], self.other_hw[1], self._extend, self.bbox_mode,
                self.root_K.data_ptr(), self.other_K.data_ptr(), self.k_values.data_ptr(), self.geom.data_ptr(), self._stream())
        self.status.copy_(self._geom_status)
        return dict(root_images=self.root_images, reg_images=self.reg_images, root_K=self.root_K, other_K=self.other_K,
                    k_values=self.k_values, geom=self.geom)

    def update(self, pred):
        """Apply the model's output (its tuple, or xyz_fk [B, nkp, 3] itself) to the state.  Returns kp2d_original [B, nkp, 2] fp32;
        ``status`` gains HRP_TRACK_LOST_OUT where the prediction was refused."""
        xyz = pred[-1] if isinstance(pred, (tuple, list)) else pred
        if not isinstance(xyz, torch.Tensor) or not xyz.is_cuda:
            raise nv.HrpError("PoseTracker.update: xyz_fk must be a GPU tensor (there is no CPU path)")
        if tuple(xyz.shape) != (self.B, self.nkp, 3):
            raise nv.HrpError(f"PoseTracker.update: xyz_fk {tuple(xyz.shape)}, want {(self.B, self.nkp, 3)}")
        xyz = xyz.detach().float().contiguous()
        nv.call("hrp_track_update", xyz.data_ptr(), self.K_original.data_ptr(), self.B, self.nkp, self.W, self.H, self.min_inside,
                self.kp2d.data_ptr(), self.have.data_ptr(), self.kp2d_original.data_ptr(), self.status.data_ptr(), self._stream())
        return self.kp2d_original

    def _refit(self, out, other_K):
        """The model's (pose, rot, trans) refitted to its own integral key-points (out[-2], camera frame): what scripts/test.py:179
        projects, here with the K of the view the refit works in."""
        if len(out) < 4:
            raise nv.HrpError("PoseTracker: a refit needs the model's kp3d_int before xyz_fk in its output")
        from hrpe_amd.lib.utils.transforms import point_projection_from_3d_tensor
        if self.refit.mode == "multi_view":
            return self._refit_views(out, point_projection_from_3d_tensor)
        K = self.K_original.view(self.B, 3, 3) if self.refit.mode == "fixed_camera" else other_K
        kp3d_int = out[-2].detach().float()
        with torch.no_grad():
            uv = point_projection_from_3d_tensor(K, kp3d_int)
        res = self.refit.solve(uv, K, out[0].detach(), out[1].detach(), out[2].detach())
        self.refit_result = res
        return res.q, res.rot, res.trans, res.kp3d

    def _refit_views(self, out, project):
        """The streams as the views of one arm: one joint solve from every stream's integral key-points, started at the mean of the
        model's joints over the streams; every stream then carries the same joints, its own calibrated pose and its own camera's
        key-points."""
        K = self.K_original.view(self.B, 3, 3)
        with torch.no_grad():
            uv = project(K, out[-2].detach().float())
            q_guess = out[0].detach().float().mean(0, keepdim=True)
        res = self.refit.solve(uv.unsqueeze(0), K, q_guess)
        self.refit_result = res
        rot, trans = self.refit.pose_on(uv.device, int(out[1].shape[-1]))
        return res.q.expand(self.B, -1), rot, trans, res.kp3d[0]

    def _filter(self, out, other_K):
        """The filter stepped on the model's integral key-points, with the model's (pose, rot, trans) as its inputs; ``_keep`` holds
        ``have`` as ``prepare`` saw it."""
        if len(out) < 4:
            raise nv.HrpError("PoseTracker: a filter needs the model's kp3d_int before xyz_fk in its output")
        from hrpe_amd.lib.utils.transforms import point_projection_from_3d_tensor
        f = self.filter
        K = self.K_original.view(self.B, 3, 3) if f.mode == "fixed_camera" else other_K
        kp3d_int = out[-2].detach().float()
        with torch.no_grad():
            uv = point_projection_from_3d_tensor(K, kp3d_int)
        pose = out[0].detach()
        if f.mode == "fixed_camera":
            res = f.step(uv, K, pose, keep=self._keep)
        else:
            res = f.step(uv, K, pose, out[1].detach(), out[2].detach(), keep=self._keep)
        self.filter_result = res
        return res.q, res.rot, res.trans, res.kp3d

    def decode(self, files):
        """A list of JPEG files' bytes -> uint8 [B, H, W, 3] on the device through dream.decode_frames: baseline files on the GPU,
        the others by Pillow.  The decode's status tensor is left in ``jpeg_status`` (jpeg.check_status reads it, and
        synchronises)."""
        from hrpe_amd.lib.dataset import dream
        enc = [dream._Encoded(bytes(f)) for f in files]
        frames, self.jpeg_status = dream.decode_frames([e.jpeg for e in enc], np.stack([e.hdr for e in enc]), [e.host for e in enc],
                                                       self.device)
        return frames

    def step(self, frames):
        """One frame per stream: prepare, the model, update.  frames: uint8 [B, H, W, 3] on the device, or a list of JPEG bytes.
        Returns TrackResult(pose, rot, trans, kp3d, kp2d_original, depth, status, k_values), device tensors; kp2d_original,
        status and k_values are the tracker's own buffers.  With a detector and acquire_every = n > 0, every n-th frame (counted
        on the host, the first included) runs ``acquire`` first: only streams without an estimate take the detection, so a lost
        stream recovers at the next scheduled detection without a read-back; with verification on, a stream whose estimate disagrees
        with the detector's mask does too.  Without, exactly prepare - model - update."""
        if isinstance(frames, (list, tuple)):
            frames = self.decode(frames)
        if self.acquire_every > 0:
            if self._frame % self.acquire_every == 0:
                self.acquire(frames)
            self._frame += 1
        p = self.prepare(frames)
        if self.filter is not None:
            self._keep.copy_(self.have)
        with torch.no_grad():
            out = tuple(self.model(p["reg_images"], p["root_images"], p["k_values"], p["other_K"]))
        pose, rot, trans, kp3d = out[0], out[1], out[2], out[-1]
        if self.refit is not None:
            pose, rot, trans, kp3d = self._refit(out, p["other_K"])
        if self.filter is not None:
            pose, rot, trans, kp3d = self._filter(out, p["other_K"])
        kp2d = self.update(kp3d)
        if self.crop_from_prediction:          # the state the next prepare crops from: the projection of the predicted key-points
            nv.call("hrp_track_update", self.filter_result.kp3d_next.data_ptr(), self.K_original.data_ptr(), self.B, self.nkp, self.W, self.H,
                    self.min_inside, self.kp2d.data_ptr(), self.have.data_ptr(), self.kp2d_predicted.data_ptr(), self.status.data_ptr(),
                    self._stream())
        if self.renderer is not None:
            self._last = (pose, rot, trans)                      # references: what the state now is the projection of
        return TrackResult(pose=pose, rot=rot, trans=trans, kp3d=kp3d, kp2d_original=kp2d, depth=out[4] if len(out) > 4 else None, status=self.status,
                           k_values=self.k_values)
