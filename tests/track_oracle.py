"""The oracle of the streaming tracker's tests: the existing host path of the DREAM loader (roboutils.get_bbox / get_extended_bbox,
dream._resize_geometry, dream._view with get_K_crop_resize and bbox_transform, common.compute_k_values, and on the GPU
dream.descriptor_table + dream.pixel_launches with flags = 0) fed float64 key-points instead of annotations.  That path is pinned
byte for byte to the reference by tests/golden/golden_dream.npz (tests/test_dream_host.py, tests/test_gpu_dream.py).  Not a test
module; tests/test_track_host.py and tests/test_gpu_track.py import it."""
import os
import sys
from copy import deepcopy

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hrpe_amd  # noqa: E402,F401
from hrpe_amd import _native as nv  # noqa: E402
from hrpe_amd.lib.core.common import compute_k_values  # noqa: E402
from hrpe_amd.lib.dataset import dream as D  # noqa: E402
from hrpe_amd.lib.dataset.roboutils import get_bbox, get_extended_bbox  # noqa: E402

MODES = {"extended": nv.TRACK_BBOX_EXTENDED, "origin": nv.TRACK_BBOX_ORIGIN, "strict": nv.TRACK_BBOX_STRICT}
ATOL, RTOL = 1e-5, 1e-6           # the project's tolerance for K, boxes and k_values (tests/test_gpu_dream.py:151-152)


def k_value(mode, root_view, strict_original, K_original):
    """select_bbox_and_K + compute_k_values (function.py:43-48, 88-98) for one sample."""
    if mode == "extended":
        box, K = root_view["bbox_gt2d_extended"], root_view["K"]
    elif mode == "origin":
        box, K = strict_original, torch.as_tensor(K_original, dtype=torch.float32)
    else:
        box, K = root_view["bbox_strict_bounded"], root_view["K"]
    return float(compute_k_values(K[None, 0, 0], K[None, 1, 1], box[None])[0])


def loader_record(pts, K_original, W, H, root_hw, other_hw, extend_ratio=(0.2, 0.13)):
    """The loader's geometry (dream.py:257-346) for key-points ``pts`` [n, 2] float64 in original pixels, their 3-D points taken on
    the rays of those pixels.  Raises ValueError where DreamDataset.__getitem__ does (dream.py:318)."""
    pts = np.asarray(pts, dtype=np.float64)
    K_original = np.asarray(K_original, dtype=np.float64).reshape(3, 3)
    if not np.isfinite(pts).all():
        raise ValueError("key-points not finite")
    bbox_gt2d = np.concatenate([pts.min(0), pts.max(0)])
    bbox = get_bbox(bbox_gt2d, W, H, strict=True)
    x0, y0, x1, y1 = (int(v) for v in bbox)
    if not (0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H):
        raise ValueError(f"crop box {list(bbox)} outside the {W} x {H} frame")
    strict_original = torch.FloatTensor(get_extended_bbox(bbox_gt2d, 20, 20, 20, 20, bounded=True, image_size=(W, H)))
    fx, fy, cx, cy = K_original[0, 0], K_original[1, 1], K_original[0, 2], K_original[1, 2]
    kp3d = np.stack([(pts[:, 0] - cx) / fx, (pts[:, 1] - cy) / fy, np.ones(len(pts))], 1)
    kp2d = np.concatenate([pts, np.zeros((len(pts), 1))], 1)
    shared = {"K_original": K_original, "keypoints_3d_original": kp3d, "_kp2d": kp2d, "_K": K_original.copy(), "_bbox": bbox,
              "bbox_strict_bounded_original": strict_original}
    side, off_x, off_y = D._resize_geometry(bbox, deepcopy(kp2d), K_original.copy())
    root, other = D._view(shared, root_hw, extend_ratio), D._view(shared, other_hw, extend_ratio)
    rec = dict(crop=(x0, y0, x1, y1), side=side, off=(off_x, off_y), root=root, other=other, strict_original=strict_original)
    rec["k"] = {m: k_value(m, root, strict_original, K_original) for m in MODES}
    return rec


def tracker_record(kp2d, have, K_original, W, H, root_hw, other_hw, mode="extended", extend_ratio=(0.2, 0.13)):
    """What the tracker must take for one stream: the loader's record of the estimate, or - no estimate, a box the loader refuses, a
    k_value that is not finite and positive - the loader's record of the whole frame's corners, with the status bits."""
    status = 0
    if have:
        try:
            with np.errstate(all="ignore"):
                rec = loader_record(kp2d, K_original, W, H, root_hw, other_hw, extend_ratio)
            if np.isfinite(rec["k"][mode]) and rec["k"][mode] > 0:
                return dict(rec, status=0)
        except (ValueError, OverflowError):
            pass
        status = nv.TRACK_BAD_BOX
    corners = [[0.0, 0.0], [W, 0.0], [W, H], [0.0, H]]
    return dict(loader_record(corners, K_original, W, H, root_hw, other_hw, extend_ratio), status=status | nv.TRACK_NO_ESTIMATE)


def aug_rows(records, W, H):
    """DreamDataset's ``aug`` rows (no augmentation, no truncation padding) of the records' crops."""
    aug = np.zeros((len(records), len(D.AUG_FIELDS)))
    for a, r in zip(aug, records):
        for k, v in (("work_w", W), ("work_h", H), ("crop_x0", r["crop"][0]), ("crop_y0", r["crop"][1]), ("crop_x1", r["crop"][2]),
                     ("crop_y1", r["crop"][3]), ("off_x", r["off"][0]), ("off_y", r["off"][1]), ("side", r["side"])):
            a[D.AUG_FIELDS.index(k)] = v
    return aug


def host_images(frames, records, root_hw, other_hw):
    """dream.pixel_launches with flags = 0 over device ``frames`` [B, H, W, 3] on the records' table: (root, other) uint8 images."""
    B, H, W, _ = frames.shape
    dev = frames.device
    tab, noise, scratch_bytes = D.descriptor_table(aug_rows(records, W, H), [b""] * B)
    table = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
    out = [torch.empty(B, 3, min(hw), max(hw), dtype=torch.uint8, device=dev) for hw in (root_hw, other_hw)]
    D.pixel_launches(frames.contiguous(), table, torch.empty(0, dtype=torch.uint8, device=dev),
                     torch.empty(scratch_bytes, dtype=torch.uint8, device=dev),
                     torch.empty(B, nv.DREAM_BANDS, dtype=torch.int64, device=dev), out[0], out[1])
    return out


def geom_array(t):
    """A [B, sizeof(hrp_track_geom)] uint8 tensor (or bytes) as a numpy structured array of hrp_track_geom."""
    raw = t.cpu().numpy().tobytes() if isinstance(t, torch.Tensor) else bytes(t)
    return np.frombuffer(raw, dtype=np.dtype(nv.TrackGeom))


def check_record(g, K_root, K_other, k, rec, mode, where=""):
    """One hrp_track_geom (a row of geom_array), its K and k_value against a loader / tracker record."""
    got = (int(g["crop_x0"]), int(g["crop_y0"]), int(g["crop_x1"]), int(g["crop_y1"]))
    assert got == rec["crop"], (where, got, rec["crop"])
    assert (int(g["side"]), int(g["off_x"]), int(g["off_y"])) == (rec["side"],) + tuple(rec["off"]), where
    if "status" in rec:
        assert int(g["status"]) == rec["status"], (where, int(g["status"]), rec["status"])
    close = lambda a, b: np.allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), atol=ATOL, rtol=RTOL)   # noqa: E731
    for v, (name, Kv) in enumerate((("root", K_root), ("other", K_other))):
        assert close(np.asarray(Kv).reshape(3, 3), rec[name]["K"].numpy()), (where, name, "K", Kv, rec[name]["K"])
        assert close(g["bbox_strict_bounded"][v], rec[name]["bbox_strict_bounded"].numpy()), \
            (where, name, g["bbox_strict_bounded"][v], rec[name]["bbox_strict_bounded"])
        assert close(g["bbox_gt2d_extended"][v], rec[name]["bbox_gt2d_extended"].numpy()), \
            (where, name, g["bbox_gt2d_extended"][v], rec[name]["bbox_gt2d_extended"])
    assert close(g["bbox_strict_bounded_original"], rec["strict_original"].numpy()), where
    assert close(k, rec["k"][mode]), (where, "k_value", k, rec["k"][mode])
