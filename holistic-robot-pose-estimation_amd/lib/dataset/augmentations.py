"""Host-side draw of the DREAM occlusion augmentation (reference lib/dataset/augmentations.py:43-74).  The fill itself
(and every other per-pixel augmentation) runs on the GPU: csrc/dream.hip, driven by lib/dataset/dream.py."""
import math
import random


def occlusion_aug(bbox, img_shape, min_area=0.0, max_area=0.3, max_try_times=5):
    """Random rectangle inside bbox of area fraction [min_area, max_area) and aspect ratio [0.5, 2) that fits the image
    (img_shape = (h, w)); four random.random() draws per try, (0, 0, 0, 0) after max_try_times + 1 failed tries.
    Returns (ymin, h, xmin, w) as ints."""
    x0, y0, x1, y1 = bbox[0], bbox[1], bbox[2], bbox[3]
    img_h, img_w = img_shape
    for _ in range(max_try_times + 1):
        area = (random.random() * (max_area - min_area) + min_area) * (x1 - x0) * (y1 - y0)
        ratio = random.random() * (1 / 0.5 - 0.5) + 0.5
        h = math.sqrt(area * ratio)
        w = math.sqrt(area / ratio)
        xmin = random.random() * ((x1 - x0) - w - 1) + x0
        ymin = random.random() * ((y1 - y0) - h - 1) + y0
        if xmin >= 0 and ymin >= 0 and xmin + w < img_w and ymin + h < img_h:
            return int(ymin), int(h), int(xmin), int(w)
    return 0, 0, 0, 0
