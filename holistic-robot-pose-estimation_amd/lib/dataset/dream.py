"""DREAM-format dataset with the reference's interface (lib/dataset/dream.py) and its pixel work on the GPU.

``DreamDataset.__getitem__`` does the cheap per-sample work on the host: JPEG decode, the JSON annotations, every random
draw (in the reference's order on ``random`` and ``np.random``, so the same seeds give the same augmentations) and all
crop / K / key-point / box geometry in float64 numpy.  It returns the decoded frame (uint8, HWC), a small parameter
record and the occlusion noise bytes; the default DataLoader collate batches them.  ``DreamDataset.to_device`` then
runs the per-pixel steps of the whole batch in two HIP launches (csrc/dream.hip):

* ``hrp_dream_augment``: truncation padding, colour jitter, the occlusion fill, ImageEnhance.Sharpness, and the
  convert("L") sums that ImageEnhance.Contrast needs;
* ``hrp_dream_crop_resize``: the square canvas of resize_image, the Contrast / Brightness / Color tail and
  CropResizeToAspectAugmentation's bilinear resize, written as uint8 NCHW;

and returns the reference's batch dict on the device (images as uint8, which ``prepare_batch`` takes unchanged).
There is no CPU path for the pixel work: CPU tensors or a missing library raise HrpError.

Not implemented (the shipped configs never enable them): ``flip``, ``rotate`` and ``padding``.
"""
import json
import os
import random
from collections import OrderedDict, defaultdict
from copy import deepcopy
from pathlib import Path

import numpy as np
import torch

from hrpe_amd import _native as nv
from hrpe_amd.lib.dataset import jpeg
from hrpe_amd.lib.dataset.augmentations import occlusion_aug
from hrpe_amd.lib.dataset.const import KEYPOINT_NAMES
from hrpe_amd.lib.dataset.roboutils import bbox_transform, get_bbox, get_bbox_raw, get_extended_bbox

KUKA_SYNT_TRAIN_DR_INCORRECT_IDS = {83114, 28630}

# dream.py:229 and :248-251: probability of each draw and the interval of its factor.  Module constants so that a test (or
# a user) can force a branch; the reference constructs the four enhancements inside __getitem__ with these values.
JITTER_P = 0.4
RGB_AUGMENTATIONS = OrderedDict([("sharpness", (0.3, (0.0, 50.0))), ("contrast", (0.3, (0.7, 1.8))),
                                 ("brightness", (0.3, (0.7, 1.8))), ("color", (0.3, (0.0, 4.0)))])
_ENH_FLAGS = (nv.DREAM_SHARPNESS, nv.DREAM_CONTRAST, nv.DREAM_BRIGHTNESS, nv.DREAM_COLOR)
TRUNCATION_PAD = 120          # roboutils.py:163 max_pad, each side
_REF_W, _REF_H = 640, 480     # frame size that process_truncation and valid_mask hard-code (roboutils.py:166-181, dream.py:218)

# the per-sample parameter record returned by __getitem__ (float64; integers are exact)
AUG_FIELDS = ("jitter0", "jitter1", "jitter2", "sharpness", "contrast", "brightness", "color", "flags",
              "occ_x", "occ_y", "occ_w", "occ_h", "pad_x", "pad_y", "work_w", "work_h",
              "crop_x0", "crop_y0", "crop_x1", "crop_y1", "off_x", "off_y", "side")
_A = {k: i for i, k in enumerate(AUG_FIELDS)}


def quat_to_rotmat_np(quat):
    """The reference's quaternion -> matrix of DREAM annotations (lib/utils/geometries.py:43-62): numpy, (w, x, y, z) names
    bound to the annotation's xyzw order as there, normalised first."""
    q = quat / np.linalg.norm(quat, ord=2, axis=0, keepdims=True)
    w, x, y, z = q[0], q[1], q[2], q[3]
    w2, x2, y2, z2 = w * w, x * x, y * y, z * z
    wx, wy, wz = w * x, w * y, w * z
    xy, xz, yz = x * y, x * z, y * z
    return np.array([[w2 - x2 - y2 + z2, -2 * yz + 2 * wx, 2 * wy + 2 * xz],
                     [2 * wx + 2 * yz, -(w2 - x2 + y2 - z2), 2 * xy - 2 * wz],
                     [-2 * xz + 2 * wy, 2 * wz + 2 * xy, -(w2 + x2 - y2 - z2)]])


def get_K_crop_resize(K, boxes, orig_size, crop_resize):
    """Intrinsics after cropping `boxes` and resizing to crop_resize, in float32 torch (lib/utils/geometries.py:360-395)."""
    K, boxes = K.float(), boxes.float()
    new_K = K.clone()
    crop_resize = torch.tensor(crop_resize, dtype=torch.float)
    fw, fh = max(crop_resize), min(crop_resize)
    cw, ch = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    cj, ci = (boxes[:, 0] + boxes[:, 2]) / 2, (boxes[:, 1] + boxes[:, 3]) / 2
    cx = K[:, 0, 2] + (cw - 1) / 2 - cj
    cy = K[:, 1, 2] + (ch - 1) / 2 - ci
    dx, dy = cx - (cw - 1) / 2, cy - (ch - 1) / 2
    sx, sy = fw / cw, fh / ch
    new_K[:, 0, 0] = sx * K[:, 0, 0]
    new_K[:, 1, 1] = sy * K[:, 1, 1]
    new_K[:, 0, 2] = (fw - 1) / 2 + sx * dx
    new_K[:, 1, 2] = (fh - 1) / 2 + sy * dy
    return new_K


def build_frame_index(base_dir):
    """rgb_path / scene_id / view_id of every ``NNNNNN.rgb.jpg`` under base_dir, sorted (dream.py:29-45), as a pandas
    DataFrame."""
    import pandas as pd
    base_dir = Path(base_dir)
    infos = defaultdict(list)
    for p in sorted(base_dir.glob("*.jpg")):
        view_id = int(p.with_suffix("").with_suffix("").name)
        if view_id == 0 and "panda_synth_test_photo" in str(base_dir):
            continue
        if "kuka_synth_train_dr" in str(base_dir) and view_id in KUKA_SYNT_TRAIN_DR_INCORRECT_IDS:
            continue
        infos["rgb_path"].append(p.as_posix())
        infos["scene_id"].append(view_id)
        infos["view_id"].append(view_id)
    return pd.DataFrame(infos)


def _resize_geometry(bbox, kp2d, K):
    """resize_image's square canvas (roboutils.py:124-150) without the pixels: side, offsets; kp2d and K updated in place."""
    x0, y0, x1, y1 = (int(v) for v in bbox)
    side = int(max(x1 - x0, y1 - y0))
    off_x, off_y = int((side - (x1 - x0)) // 2), int((side - (y1 - y0)) // 2)
    for k in kp2d:
        k[1] -= y0
        k[1] += off_y
        k[0] += off_x
        k[0] -= x0
    K[0, 2] -= (x0 - off_x)
    K[1, 2] -= (y0 - off_y)
    return side, off_x, off_y


def _view(shared, resize_hw, extend_ratio):
    """_get_rootnet_data / _get_other_data (dream.py:287-394) without the pixels."""
    kp2d = deepcopy(shared["_kp2d"])
    K = deepcopy(shared["_K"])
    kp3d = shared["keypoints_3d_original"]
    side, _, _ = _resize_geometry(shared["_bbox"], kp2d, K)
    out_h, out_w = min(resize_hw), max(resize_hw)
    if (side, side) != (out_h, out_w):                     # CropResizeToAspectAugmentation (augmentations.py:170-242)
        box = torch.tensor([side / 2 - side / 2, side / 2 - side / 2, side / 2 + side / 2, side / 2 + side / 2])
        Kt = get_K_crop_resize(torch.tensor(K).unsqueeze(0), box.unsqueeze(0), orig_size=(side, side),
                               crop_resize=(out_h, out_w))
        Kn = Kt.numpy()[0]
        kp2d = []
        for p3 in kp3d:
            v = np.matmul(Kn, p3)
            kp2d.append(list((v / v[-1])[:-1]))
        K = Kn
    K_r = torch.FloatTensor(np.asarray(K))
    K_orig_inv = np.linalg.inv(shared["K_original"])
    bs = bbox_transform(shared["bbox_strict_bounded_original"], K_orig_inv, np.asarray(K), resize_hw=resize_hw)
    bs = np.array([max(0, bs[0]), max(0, bs[1]), min(resize_hw[0], bs[2]), min(resize_hw[1], bs[3])])
    g = np.concatenate([np.min(kp2d, axis=0)[0:2], np.max(kp2d, axis=0)[0:2]])
    w_, h_ = g[2] - g[0], g[3] - g[1]
    ext = get_extended_bbox(g, w_ * extend_ratio[0], h_ * extend_ratio[1], w_ * extend_ratio[0], h_ * extend_ratio[1],
                            bounded=True, image_size=resize_hw)
    kp2d_r = torch.FloatTensor(kp2d)[:, 0:2]
    k = kp2d_r.numpy()
    valid = torch.FloatTensor((k[:, 0] < resize_hw[0]) & (k[:, 0] >= 0) & (k[:, 1] < resize_hw[1]) & (k[:, 1] >= 0))
    return {"bbox_strict_bounded": torch.FloatTensor(bs), "bbox_gt2d_extended": torch.FloatTensor(ext), "K": K_r,
            "keypoints_3d": torch.FloatTensor(kp3d), "keypoints_2d": kp2d_r, "valid_mask_crop": valid}


class _Encoded:
    """A frame that is not decoded in the worker (device_decode): the file's bytes and its parsed header, or - for a file that
    jpeg.parse_header refuses - Pillow's decode as raw bytes.  ``shape`` is all that __getitem__ reads of a frame."""

    def __init__(self, data):
        from PIL import Image
        hdr = jpeg.parse_header(data)
        if hdr is None:
            import io
            host = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
            rec = np.zeros(1, dtype=jpeg.HDR_DTYPE)
            rec["height"], rec["width"] = host.shape[0], host.shape[1]
            self.jpeg, self.hdr, self.host = b"", rec.view(np.uint8).reshape(jpeg.HDR_BYTES), host.tobytes()
            self.shape = host.shape
        else:
            r = jpeg.record(hdr)
            self.jpeg, self.hdr, self.host = data, hdr, b""
            self.shape = (int(r["height"]), int(r["width"]), 3)


class DreamDataset(torch.utils.data.Dataset):
    """The reference's DreamDataset (dream.py:48-412) with the same constructor and batch schema.  __getitem__ returns, besides
    the reference's non-image entries, ``frame`` (the decoded uint8 [H, W, 3]), ``aug`` (float64 [len(AUG_FIELDS)]: the drawn
    factors and the crop geometry) and ``noise`` (bytes: the occlusion fill); ``to_device`` turns a collated batch into the
    reference's dict on the GPU.

    device_decode=True leaves the JPEG decode to the GPU (lib/dataset/jpeg.py): the worker only reads the file and parses its
    header, and the item carries ``jpeg`` (the file's bytes), ``jpeg_hdr`` (uint8 [jpeg.HDR_BYTES]) and ``jpeg_host`` in place
    of ``frame``.  A file the device path does not take (progressive, grayscale, ...) is decoded with Pillow in the worker:
    its ``jpeg`` is empty and ``jpeg_host`` holds the raw RGB bytes, which ``to_device`` uploads into the same frame buffer.
    jpeg_entropy="sync" makes ``to_device`` decode with jpeg.Batch(entropy="sync"): a file without restart markers by a whole
    workgroup instead of one lane, with the same result."""

    def __init__(self, base_dir, rootnet_resize_hw=(256, 256), other_resize_hw=(256, 256), visibility_check=True,
                 strict_crop=True, color_jitter=True, rgb_augmentation=True, occlusion_augmentation=True, flip=False,
                 rotate=False, padding=False, occlu_p=0.5, process_truncation=False, extend_ratio=[0.2, 0.13],
                 device_decode=False, jpeg_entropy="segment"):
        if flip or rotate or padding:
            raise NotImplementedError("DreamDataset: flip / rotate / padding are not implemented (no shipped config enables them)")
        if jpeg_entropy not in ("segment", "sync"):
            raise nv.HrpError(f"DreamDataset: jpeg_entropy {jpeg_entropy!r}, want 'segment' or 'sync'")
        self.device_decode, self.jpeg_entropy = device_decode, jpeg_entropy
        self.base_dir = Path(base_dir)
        self.ds_name = os.path.basename(base_dir)
        self.rootnet_resize_hw, self.other_resize_hw = rootnet_resize_hw, other_resize_hw
        self.color_jitter, self.rgb_augmentation = color_jitter, rgb_augmentation
        self.occlusion_augmentation, self.total_occlusions = occlusion_augmentation, 1
        self.rootnet_flip, self.rootnet_rotate, self.padding = flip, rotate, padding
        self.visibility_check, self.process_truncation = visibility_check, process_truncation
        self.occlu_p, self.strict_crop, self.extend_ratio = occlu_p, strict_crop, extend_ratio
        self.frame_index = build_frame_index(self.base_dir)
        self.synthetic = True
        s = str(base_dir)
        if "panda" in s:
            self.label = "panda"
            if "panda-3cam" in self.ds_name or "panda-orb" in self.ds_name:
                self.synthetic = False
        elif "baxter" in s:
            self.label = "baxter"
        elif "kuka" in s:
            self.label = "kuka"
        else:
            raise NotImplementedError(f"DreamDataset: no robot name in {base_dir}")
        self.keypoint_names = KEYPOINT_NAMES[self.label]
        self.scale = 0.01 if "synthetic" in str(self.base_dir) else 1.0
        self.all_labels = [self.label]

    def __len__(self):
        return len(self.frame_index)

    def _annotations(self, idx):
        """Decode the frame, read its JSON and the camera (dream.py:106-216)."""
        from PIL import Image
        row = self.frame_index.iloc[idx]
        rgb_path = Path(row.rgb_path)
        rgb = _Encoded(rgb_path.read_bytes()) if self.device_decode else np.asarray(Image.open(rgb_path))
        ann = json.loads(rgb_path.with_suffix("").with_suffix(".json").read_text())
        h, w = rgb.shape[0], rgb.shape[1]
        cam_path = self.base_dir / "_camera_settings.json"
        if cam_path.exists():
            cams = json.loads(cam_path.read_text())
            assert len(cams["camera_settings"]) == 1
            ci = cams["camera_settings"][0]["intrinsic_settings"]
            fx, fy, cx, cy = [ci[k] for k in ("fx", "fy", "cx", "cy")]
        else:
            fx, fy, cx, cy = 320, 320, w / 2, h / 2
        K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
        obj = ann["objects"][0]
        TWO = np.zeros((4, 4), dtype=float)
        if "quaternion_xyzw" in obj:
            TWO[:3, :3] = quat_to_rotmat_np(np.array(obj["quaternion_xyzw"]))
        else:
            TWO[:3, :3] = quat_to_rotmat_np(np.array([1.0, 0.0, 0.0, 0.0]))
        TWO[:3, 3] = np.array(obj["location"]) * self.scale
        TWO[3, 3] = 1.0
        if "quaternion_xyzw" in obj:
            TWO[:3, :3] = TWO[:3, :3] @ np.array([[0, -1, 0], [0, 0, -1], [1, 0, 0]])    # R_NORMAL_UE
        TCO = torch.FloatTensor(np.asarray(torch.eye(4, dtype=torch.float64) @ torch.as_tensor(TWO)))   # invert_T(TWC = I) @ TWO
        joints = OrderedDict((d["name"].split("/")[-1], float(d["position"])) for d in ann["sim_state"]["joints"])
        if self.label == "kuka":
            joints = {k.replace("iiwa7_", "iiwa_"): v for k, v in joints.items()}
        return row, rgb, K, obj, TCO, joints

    def __getitem__(self, idx):
        row, rgb, K, obj, TCO, joints = self._annotations(idx)
        h, w = rgb.shape[0], rgb.shape[1]
        kps = obj["keypoints"]
        uniq = np.unique(np.concatenate([np.array(k["projected_location"])[None] for k in kps], axis=0), axis=0)
        bbox_gt2d = np.concatenate([np.min(uniq, axis=0), np.max(uniq, axis=0)])
        bbox = get_bbox(bbox_gt2d, w, h, strict=self.strict_crop)
        bboxes_raw = get_bbox_raw(bbox_gt2d)
        ext_orig = get_extended_bbox(bbox_gt2d, 20, 20, 20, 20, bounded=True, image_size=(w, h))
        if "bounding_box" in obj:
            bi = obj["bounding_box"]
            bs = np.array([bi["min"][0], bi["min"][1], bi["max"][0], bi["max"][1]])
            strict_bounded = np.array([max(0, bs[0]), max(0, bs[1]), min(w, bs[2]), min(h, bs[3])])
        else:
            strict_bounded = ext_orig
        kp3d = {k["name"]: np.array(k["location"]) * self.scale for k in kps}
        kp3d = np.array([kp3d.get(k, np.nan) for k in self.keypoint_names])
        assert not np.isnan(kp3d).any()
        kp2d = {k["name"]: k["projected_location"] for k in kps}
        kp2d = np.array([np.append(kp2d.get(k, np.nan), 0) for k in self.keypoint_names])
        K_original, kp2d_original = K.copy(), kp2d.copy()
        valid = ((kp2d_original[:, 0] < 640.0) & (kp2d_original[:, 0] >= 0) &
                 (kp2d_original[:, 1] < 480.0) & (kp2d_original[:, 1] >= 0))

        aug = np.zeros(len(AUG_FIELDS))
        flags = 0
        pad_x = pad_y = 0
        work_w, work_h = w, h
        if self.process_truncation:                                     # roboutils.py:163-195 without the pixels
            x0, y0, x1, y1 = bboxes_raw
            if x0 > 0 and y0 > 0 and y1 < _REF_H and x1 < _REF_W:
                bbox = bboxes_raw
            else:
                if (h, w) != (_REF_H, _REF_W):
                    raise ValueError(f"process_truncation needs {_REF_W} x {_REF_H} frames (got {w} x {h}), as the reference")
                d = [min(TRUNCATION_PAD, int(max(0, int(v)))) for v in (-x0, -y0, x1 - _REF_W, y1 - _REF_H)]
                pad_x, pad_y = d[0], d[1]
                work_w, work_h = _REF_W + d[2] + d[0], _REF_H + d[3] + d[1]
                for k in kp2d:
                    k[1] += pad_y
                    k[0] += pad_x
                K[0, 2] += pad_x
                K[1, 2] += pad_y
                raw = np.concatenate([np.min(kp2d, axis=0)[0:2], np.max(kp2d, axis=0)[0:2]])
                bbox = get_bbox(raw, work_w, work_h)

        if self.color_jitter and random.random() < JITTER_P:          # dream.py:229-237
            factor = 2 * random.random()
            for c in range(3):
                aug[_A["jitter%d" % c]] = random.uniform(1 - factor, 1 + factor)
            flags |= nv.DREAM_JITTER
        noise = b""
        for _ in range(self.total_occlusions):                         # :239-245
            if self.occlusion_augmentation and random.random() < self.occlu_p:
                oy, oh, ox, ow = occlusion_aug(bbox, np.array([h, w]), min_area=0.0, max_area=0.3, max_try_times=5)
                noise = (np.random.rand(oh, ow, 3) * 255).astype(np.uint8).tobytes()
                aug[[_A["occ_x"], _A["occ_y"], _A["occ_w"], _A["occ_h"]]] = ox, oy, ow, oh
                flags |= nv.DREAM_OCCLUSION
        if self.rgb_augmentation:                                      # :247-255
            for (name, (p, interval)), flag in zip(RGB_AUGMENTATIONS.items(), _ENH_FLAGS):
                if random.random() <= p:
                    aug[_A[name]] = random.uniform(*interval)
                    flags |= flag

        x0, y0, x1, y1 = (int(v) for v in bbox)
        if not (0 <= x0 < x1 <= work_w and 0 <= y0 < y1 <= work_h):
            raise ValueError(f"DreamDataset: crop box {list(bbox)} outside the {work_w} x {work_h} working frame (frame {idx})")
        shared = {"K_original": K_original, "keypoints_3d_original": kp3d, "_kp2d": kp2d, "_K": K, "_bbox": bbox,
                  "bbox_strict_bounded_original": torch.FloatTensor(strict_bounded.copy())}
        side, off_x, off_y = _resize_geometry(bbox, deepcopy(kp2d), K.copy())
        aug[_A["flags"]] = flags
        for k, v in (("pad_x", pad_x), ("pad_y", pad_y), ("work_w", work_w), ("work_h", work_h), ("crop_x0", x0),
                     ("crop_y0", y0), ("crop_x1", x1), ("crop_y1", y1), ("off_x", off_x), ("off_y", off_y), ("side", side)):
            aug[_A[k]] = v
        if isinstance(rgb, _Encoded):
            frame = {"jpeg": rgb.jpeg, "jpeg_hdr": torch.from_numpy(rgb.hdr.copy()), "jpeg_host": rgb.host}
        else:
            frame = {"frame": torch.from_numpy(np.array(rgb, dtype=np.uint8))}
        return {
            "image_id": idx,
            "scene_id": row.scene_id,
            **frame,
            "aug": torch.from_numpy(aug),
            "noise": noise,
            "bbox_strict_bounded_original": shared["bbox_strict_bounded_original"],
            "bbox_gt2d_extended_original": torch.FloatTensor(ext_orig),
            "TCO": TCO,
            "K_original": K_original,
            "jointpose": joints,
            "keypoints_2d_original": kp2d_original[:, 0:2],
            "valid_mask": torch.FloatTensor(valid),
            "keypoints_3d_original": kp3d.copy(),
            "root": _view(shared, self.rootnet_resize_hw, self.extend_ratio),
            "other": _view(shared, self.other_resize_hw, self.extend_ratio),
        }

    def to_device(self, batch, device=None, stream=None, jpeg_status=None, jpeg_entropy=None, subseq_bytes=None, min_subseq=None):
        """A collated batch -> the reference's batch dict on `device` (default: the current CUDA device), with the pixel work of
        the whole batch in two launches on the current stream.  ``images_original`` is the decoded frame as uint8 [B, 3, H, W]
        (a view of the uploaded [B, H, W, 3]); ``root/images`` and ``other/images`` are uint8 [B, 3, h, w].  When the two
        views have the same size (every shipped config: 256 x 256) they are written once and both entries hold the same
        tensor.  A batch of a device_decode dataset is decoded on the GPU first; by default the decode's status is checked
        before returning (which synchronises) - pass a list as jpeg_status to receive the status tensor instead and call
        jpeg.check_status on it later.  jpeg_entropy (default: the constructor's), subseq_bytes and min_subseq go to jpeg.Batch."""
        return to_device(batch, self.rootnet_resize_hw, self.other_resize_hw, device=device, stream=stream, jpeg_status=jpeg_status,
                         jpeg_entropy=self.jpeg_entropy if jpeg_entropy is None else jpeg_entropy, subseq_bytes=subseq_bytes,
                         min_subseq=min_subseq)


def _move(v, device):
    if isinstance(v, torch.Tensor):
        return v.to(device, non_blocking=True)
    if isinstance(v, dict):
        return {k: _move(x, device) for k, x in v.items()}
    return v


def descriptor_table(aug, noise):
    """Collated ``aug`` [B, len(AUG_FIELDS)] and ``noise`` (list of bytes) -> (hrp_dream_sample records as a numpy structured
    array, packed noise bytes, scratch bytes).  Every offset and rectangle is checked here: the kernels index with them."""
    aug = np.asarray(torch.as_tensor(aug, dtype=torch.float64))
    B = aug.shape[0]
    if aug.ndim != 2 or aug.shape[1] != len(AUG_FIELDS) or len(noise) != B:
        raise nv.HrpError(f"DreamDataset batch: aug {aug.shape}, {len(noise)} noise entries")
    tab = np.zeros(B, dtype=np.dtype(nv.DreamSample))
    ints = lambda k: aug[:, _A[k]].astype(np.int64)                   # noqa: E731
    tab["jitter"] = aug[:, 0:3]
    tab["enh"] = aug[:, 3:7]
    for k in AUG_FIELDS[7:]:
        tab[k] = ints(k)
    sizes = np.array([len(n) for n in noise], dtype=np.int64)
    occ = (tab["flags"] & nv.DREAM_OCCLUSION) != 0
    if (sizes != np.where(occ, tab["occ_w"].astype(np.int64) * tab["occ_h"] * 3, 0)).any():
        raise nv.HrpError("DreamDataset batch: occlusion noise does not match its rectangle")
    if (occ & ((tab["occ_x"] < 0) | (tab["occ_y"] < 0) | (tab["occ_x"] + tab["occ_w"] > tab["work_w"]) |
               (tab["occ_y"] + tab["occ_h"] > tab["work_h"]))).any():
        raise nv.HrpError("DreamDataset batch: occlusion rectangle outside the working frame")
    if ((tab["crop_x0"] < 0) | (tab["crop_y0"] < 0) | (tab["crop_x1"] > tab["work_w"]) | (tab["crop_y1"] > tab["work_h"]) |
            (tab["crop_x1"] <= tab["crop_x0"]) | (tab["crop_y1"] <= tab["crop_y0"]) | (tab["side"] < 1) |
            (tab["off_x"] + tab["crop_x1"] - tab["crop_x0"] > tab["side"]) |
            (tab["off_y"] + tab["crop_y1"] - tab["crop_y0"] > tab["side"])).any():
        raise nv.HrpError("DreamDataset batch: crop box outside the working frame or the canvas")
    tab["noise_off"] = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    frame_bytes = tab["work_w"].astype(np.int64) * tab["work_h"] * 3
    tab["scratch_off"] = np.concatenate([[0], np.cumsum(frame_bytes)[:-1]])
    return tab, b"".join(noise), int(frame_bytes.sum())


def pixel_launches(frames, table, noise, scratch, lsum, out0, out1=None, max_hw=None, stream=None):
    """The two launches on device tensors: frames [B, H, W, 3] uint8, table (hrp_dream_sample bytes, uint8), noise (uint8, may be
    empty), scratch (uint8, at least the working frames' bytes), lsum [B, DREAM_BANDS] int64, out0 / out1 [B, 3, h, w] uint8.
    max_hw bounds every working frame (default: the frame size).  Caller-owned buffers, no host sync, a fixed launch count:
    graph-capturable."""
    for name, t, dt in (("frames", frames, torch.uint8), ("table", table, torch.uint8), ("noise", noise, torch.uint8),
                        ("scratch", scratch, torch.uint8), ("lsum", lsum, torch.int64), ("out0", out0, torch.uint8)):
        if not t.is_cuda or t.dtype != dt or not t.is_contiguous():
            raise nv.HrpError(f"dream pixel launches: {name} must be a contiguous {dt} GPU tensor (there is no CPU path)")
    B, H, W, C3 = frames.shape
    if C3 != 3 or table.numel() != B * np.dtype(nv.DreamSample).itemsize or lsum.numel() != B * nv.DREAM_BANDS:
        raise nv.HrpError("dream pixel launches: frames / table / lsum shapes do not match")
    for o in (out0, out1):
        if o is not None and (o.dim() != 4 or o.shape[0] != B or o.shape[1] != 3):
            raise nv.HrpError(f"dream pixel launches: output {tuple(o.shape)} is not [B, 3, h, w]")
    if out1 is not None and (not out1.is_cuda or out1.dtype != torch.uint8 or not out1.is_contiguous()):
        raise nv.HrpError("dream pixel launches: out1 must be a contiguous uint8 GPU tensor")
    mh, mw = max_hw or (H, W)
    s = stream if stream is not None else torch.cuda.current_stream(frames.device).cuda_stream
    nv.call("hrp_dream_augment", frames.data_ptr(), B, H, W, table.data_ptr(), noise.data_ptr() if noise.numel() else None,
            noise.numel(), mh, mw, scratch.data_ptr(), scratch.numel(), lsum.data_ptr(), s)
    h1, w1 = (out1.shape[2], out1.shape[3]) if out1 is not None else (0, 0)
    nv.call("hrp_dream_crop_resize", scratch.data_ptr(), scratch.numel(), table.data_ptr(), lsum.data_ptr(), B, mh, mw,
            out0.data_ptr(), out0.shape[2], out0.shape[3], out1.data_ptr() if out1 is not None else None, h1, w1, s)


def decode_frames(datas, hdrs, hosts, device, stream=None, entropy="segment", subseq_bytes=None, min_subseq=None):
    """The frames of a device_decode batch as one uint8 [B, H, W, 3] device tensor, and the decode's status ([B] int32 on the
    device, None when no file went to the GPU): the files with a header in one jpeg.Batch, the frames that the worker decoded
    (``hosts``, raw RGB bytes) uploaded into the same buffer.  All frames of a batch have one size, as ``frame`` requires.
    entropy, subseq_bytes, min_subseq: jpeg.Batch's."""
    kw = dict(entropy=entropy, subseq_bytes=subseq_bytes, min_subseq=min_subseq)
    recs = jpeg.record(hdrs)
    B = len(datas)
    if recs.shape != (B,) or len(hosts) != B:
        raise nv.HrpError(f"DreamDataset batch: {B} jpeg entries, {recs.shape} headers, {len(hosts)} host frames")
    H, W = int(recs["height"][0]), int(recs["width"][0])
    if H < 1 or W < 1 or (recs["height"] != H).any() or (recs["width"] != W).any():
        raise nv.HrpError("DreamDataset batch: the frames of a batch must have one size")
    on_dev = [i for i in range(B) if len(datas[i])]
    for i in range(B):
        if (len(datas[i]) == 0) == (len(hosts[i]) == 0) or len(hosts[i]) not in (0, H * W * 3):
            raise nv.HrpError(f"DreamDataset batch: sample {i} needs either its file or its {H} x {W} decoded frame")
    if len(on_dev) == B:
        b = jpeg.Batch(datas, recs, device, **kw)
        b.launch(stream)
        return b.flat.view(B, H, W, 3), b.status
    frames_d = torch.empty(B, H, W, 3, dtype=torch.uint8, device=device)
    status = None
    if on_dev:
        b = jpeg.Batch([datas[i] for i in on_dev], recs[on_dev], device, **kw)
        b.launch(stream)
        frames_d[torch.as_tensor(on_dev, device=device)] = b.flat.view(len(on_dev), H, W, 3)
        status = b.status
    host = [i for i in range(B) if len(hosts[i])]
    up = torch.from_numpy(np.frombuffer(b"".join(hosts[i] for i in host), dtype=np.uint8).copy()).to(device, non_blocking=True)
    frames_d[torch.as_tensor(host, device=device)] = up.view(len(host), H, W, 3)
    return frames_d, status


def to_device(batch, rootnet_resize_hw=(256, 256), other_resize_hw=(256, 256), device=None, stream=None, jpeg_status=None,
              jpeg_entropy="segment", subseq_bytes=None, min_subseq=None):
    """DreamDataset.to_device for a collated batch (see there)."""
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if device.type != "cuda":
        raise nv.HrpError(f"DreamDataset.to_device: {device} is not a GPU (there is no CPU path for the pixel work)")
    nv.lib()
    if "jpeg" in batch:
        return _to_device_jpeg(batch, rootnet_resize_hw, other_resize_hw, device, stream, jpeg_status,
                               dict(entropy=jpeg_entropy, subseq_bytes=subseq_bytes, min_subseq=min_subseq))
    frames = torch.as_tensor(batch["frame"])
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        raise nv.HrpError(f"DreamDataset.to_device: frames {tuple(frames.shape)} {frames.dtype}, want uint8 [B, H, W, 3]")
    B, H, W, _ = frames.shape
    tab, noise, scratch_bytes = descriptor_table(batch["aug"], batch["noise"])
    mh, mw = int(max(H, tab["work_h"].max())), int(max(W, tab["work_w"].max()))
    frames_d = frames.to(device, non_blocking=True).contiguous()
    return _pixel_work(batch, frames_d, tab, noise, scratch_bytes, (mh, mw), rootnet_resize_hw, other_resize_hw, device, stream)


def _to_device_jpeg(batch, rootnet_resize_hw, other_resize_hw, device, stream, jpeg_status, jpeg_kw):
    """to_device for a batch that carries ``jpeg`` / ``jpeg_hdr`` / ``jpeg_host`` in place of ``frame``."""
    tab, noise, scratch_bytes = descriptor_table(batch["aug"], batch["noise"])
    frames_d, status = decode_frames(batch["jpeg"], batch["jpeg_hdr"], batch["jpeg_host"], device, stream, **jpeg_kw)
    _, H, W, _ = frames_d.shape
    mh, mw = int(max(H, tab["work_h"].max())), int(max(W, tab["work_w"].max()))
    out = _pixel_work(batch, frames_d, tab, noise, scratch_bytes, (mh, mw), rootnet_resize_hw, other_resize_hw, device, stream)
    if jpeg_status is not None:
        jpeg_status.append(status)
    elif status is not None:
        jpeg.check_status(status)
    return out


def _pixel_work(batch, frames_d, tab, noise, scratch_bytes, max_hw, rootnet_resize_hw, other_resize_hw, device, stream):
    """The part of to_device after the frames are on the device: the two launches and the batch dict."""
    B = frames_d.shape[0]
    mh, mw = max_hw
    table_d = torch.from_numpy(tab.view(np.uint8).copy()).to(device, non_blocking=True)
    noise_d = torch.from_numpy(np.frombuffer(noise, dtype=np.uint8).copy()).to(device, non_blocking=True)
    scratch = torch.empty(max(scratch_bytes, 1), dtype=torch.uint8, device=device)
    lsum = torch.empty(B, nv.DREAM_BANDS, dtype=torch.int64, device=device)
    hr, wr = min(rootnet_resize_hw), max(rootnet_resize_hw)
    ho, wo = min(other_resize_hw), max(other_resize_hw)
    out_r = torch.empty(B, 3, hr, wr, dtype=torch.uint8, device=device)
    same = (hr, wr) == (ho, wo)
    out_o = out_r if same else torch.empty(B, 3, ho, wo, dtype=torch.uint8, device=device)
    pixel_launches(frames_d, table_d, noise_d, scratch, lsum, out_r, None if same else out_o, max_hw=(mh, mw), stream=stream)
    out = {k: _move(v, device) for k, v in batch.items()
           if k not in ("frame", "jpeg", "jpeg_hdr", "jpeg_host", "aug", "noise", "root", "other")}
    out["images_original"] = frames_d.permute(0, 3, 1, 2)
    out["root"] = dict(_move(batch["root"], device), images=out_r)
    out["other"] = dict(_move(batch["other"], device), images=out_o)
    return out
