"""Host-side bounding-box helpers of the DREAM loader, with the reference's names and arithmetic
(lib/dataset/roboutils.py:59-122, 196-257).  They work on a handful of numbers per sample; the pixel work they
describe runs on the GPU (csrc/dream.hip, driven by lib/dataset/dream.py)."""
import random

import numpy as np


def get_bbox(bbox, w, h, strict=True):
    """Key-point box -> crop box (roboutils.py:59-103): 30 % margin, clamped to the w x h frame; strict=False widens or
    narrows it by two random.random() draws (width first); a box under 150 x 120 grows by 75 / 60 px a side."""
    assert len(bbox) == 4
    x0, y0, x1, y1 = bbox
    x0, y0, x1, y1 = max(0, x0), max(0, y0), min(w, x1), min(h, y1)
    bw, bh = x1 - x0, y1 - y0
    x0, x1 = int(max(0, x0 - 0.3 * bw)), int(min(w, x1 + 0.3 * bw))
    y0, y1 = int(max(0, y0 - 0.3 * bh)), int(min(h, y1 + 0.3 * bh))
    bw, bh = x1 - x0, y1 - y0
    if not strict:
        rw = (random.random() - 0.2) / 2
        rh = (random.random() - 0.2) / 2
        dw = rw * bw
        x1 += dw / 2
        x0 -= dw / 2
        dh = rh * bh
        y1 += dh / 2
        y0 -= dh / 2
        x0, x1, y0, y1 = int(max(0, x0)), int(min(w, x1)), int(max(0, y0)), int(min(h, y1))
        bw, bh = x1 - x0, y1 - y0
    if bw < 150:
        x1 += 75
        x0 -= 75
    if bh < 120:
        y1 += 60
        y0 -= 60
    x0, y0, x1, y1 = max(0, x0), max(0, y0), min(w, x1), min(h, y1)
    x0, y0, x1, y1 = min(w, x0), min(h, y0), max(0, x1), max(0, y1)
    return np.array([x0, y0, x1, y1])


def get_bbox_raw(bbox):
    """get_bbox without the frame clamp and without random widening (roboutils.py:105-122)."""
    assert len(bbox) == 4
    x0, y0, x1, y1 = bbox
    bw, bh = x1 - x0, y1 - y0
    x0, x1 = int(x0 - 0.3 * bw), int(x1 + 0.3 * bw)
    y0, y1 = int(y0 - 0.3 * bh), int(y1 + 0.3 * bh)
    if x1 - x0 < 150:
        x1 += 75
        x0 -= 75
    if y1 - y0 < 120:
        y1 += 60
        y0 -= 60
    return np.array([x0, y0, x1, y1])


def bbox_transform(bbox, K_original_inv, K, resize_hw):
    """Box corners through K_original^-1 then K, clipped to the resized view (roboutils.py:224-242); x is clipped to
    resize_hw[0], y to resize_hw[1], as there."""
    x0, y0, x1, y1 = (float(v) for v in bbox)
    corners = np.array([[x0, y0, 1.0], [x1, y0, 1.0], [x1, y1, 1.0], [x0, y1, 1.0]])
    c = np.matmul(K, np.matmul(K_original_inv, corners.T)).T
    assert all(c[:, 2] == 1.0), c
    return np.array([np.clip(c[0, 0], 0, resize_hw[0]), np.clip(c[0, 1], 0, resize_hw[1]),
                     np.clip(c[1, 0], 0, resize_hw[0]), np.clip(c[2, 1], 0, resize_hw[1])])


def get_extended_bbox(bbox, dwmin, dhmin, dwmax, dhmax, bounded=True, image_size=None):
    """Grow a box by the four margins; bounded: clamp to image_size = (w, h) (roboutils.py:244-257)."""
    x0, y0, x1, y1 = bbox
    ext = np.array([x0 - dwmin, y0 - dhmin, x1 + dwmax, y1 + dhmax])
    if bounded:
        assert image_size
        x0, y0, x1, y1 = ext
        ext = np.array([max(0, x0), max(0, y0), min(image_size[0], x1), min(image_size[1], y1)])
    return ext
