"""Writes tests/golden/golden_jpeg.npz: JPEG files written by Pillow and Pillow's own decode of each (libjpeg-turbo defaults:
islow inverse DCT, fancy up-sampling), the reference of tests/test_jpeg_host.py and tests/test_gpu_jpeg.py.  Pillow only.

Per case ``<name>/file`` (the file's bytes) and ``<name>/rgb`` (uint8 [H, W, 3]); ``names`` lists the cases the device path
decodes, ``fallback`` those that parse_header must refuse.  Every image comes from one seeded texture: a smooth colour field
(blocks with no AC coefficients) with bands of per-pixel noise (blocks with dense AC).

    python tests/golden/gen_golden_jpeg.py
"""
import io
import os

import numpy as np
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))


def texture(h, w, seed, saturate=False):
    rng = np.random.Generator(np.random.PCG64(seed))
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([128 + 100 * np.sin(x / 19.0 + seed) * np.cos(y / 13.0), 128 + 90 * np.cos((x + 2 * y) / 23.0),
                    40 + 170 * (x + y) / (h + w)], -1)
    noisy = ((x // 11 + y // 7) % 3 == 0)[..., None]
    img = img + noisy * rng.normal(0, 40, (h, w, 3))
    if saturate:        # hard black / white / primary patches next to each other: the inverse DCT overshoots and clamps
        img[: h // 2, : w // 2] = np.where(((x // 3 + y // 5) % 2 == 0)[: h // 2, : w // 2, None], 255.0, 0.0)
        img[h // 2:, : w // 3] = [255.0, 0.0, 255.0]
    return np.clip(img, 0, 255).astype(np.uint8)


# name: (h, w, save keywords, saturate)
CASES = {
    "mcu_16x16_420": (16, 16, dict(quality=92, subsampling=2), False),
    "odd_23x37_444": (23, 37, dict(quality=92, subsampling=0), False),
    "odd_23x37_422": (23, 37, dict(quality=92, subsampling=1), False),
    "odd_23x37_420": (23, 37, dict(quality=92, subsampling=2), False),
    "wide_9x50_420": (9, 50, dict(quality=92, subsampling=2), False),
    "tall_33x17_420": (33, 17, dict(quality=92, subsampling=2), False),
    "q50_48x64_420": (48, 64, dict(quality=50, subsampling=2), False),
    "q100_sat_48x64_420": (48, 64, dict(quality=100, subsampling=2), True),
    "optimize_40x56_420": (40, 56, dict(quality=92, subsampling=2, optimize=True), False),
    "rst_blocks2_40x56_420": (40, 56, dict(quality=92, subsampling=2, restart_marker_blocks=2), False),
    "rst_rows1_40x56_420": (40, 56, dict(quality=92, subsampling=2, restart_marker_rows=1), False),
    "rows_96x128_420": (96, 128, dict(quality=92, subsampling=2), False),
}
FALLBACK = {
    "progressive_40x56": (40, 56, dict(quality=92, subsampling=2, progressive=True), "RGB"),
    "gray_40x56": (40, 56, dict(quality=92), "L"),
    "narrow_20x3_420": (20, 3, dict(quality=92, subsampling=2), "RGB"),
}


def main():
    assert features.check_feature("libjpeg_turbo"), "the fixture records libjpeg-turbo's decode"
    out = {"names": np.array(sorted(CASES)), "fallback": np.array(sorted(FALLBACK)),
           "pillow": np.array(f"{Image.__version__} jpg {features.version('jpg')}")}
    for i, (name, (h, w, kw, sat)) in enumerate(sorted(CASES.items())):
        buf = io.BytesIO()
        Image.fromarray(texture(h, w, 10 + i, sat)).save(buf, format="JPEG", **kw)
        out[name + "/file"] = np.frombuffer(buf.getvalue(), dtype=np.uint8)
        out[name + "/rgb"] = np.asarray(Image.open(io.BytesIO(buf.getvalue())))
        assert out[name + "/rgb"].shape == (h, w, 3)
    for i, (name, (h, w, kw, mode)) in enumerate(sorted(FALLBACK.items())):
        buf = io.BytesIO()
        Image.fromarray(texture(h, w, 50 + i)).convert(mode).save(buf, format="JPEG", **kw)
        out[name + "/file"] = np.frombuffer(buf.getvalue(), dtype=np.uint8)
        out[name + "/rgb"] = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
    path = os.path.join(HERE, "golden_jpeg.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
