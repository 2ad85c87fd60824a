"""A small DREAM-format scene from a seeded procedural formula (used by tests/golden/gen_golden_dream.py and the DREAM tests).

``write_scene(dirpath)`` writes ``NNNNNN.rgb.jpg`` + ``NNNNNN.json`` (the name the loaders read: ``.rgb.jpg`` with both suffixes replaced) per frame and ``_camera_settings.json``.  The images
are textured (smooth colour gradients, stripes and per-pixel noise) so that ImageEnhance.Sharpness changes them; each frame's
key-points are the projections of seven 3-D points through the scene camera, placed so that the frames cover a centred robot,
one touching the frame border, one past the frame edge (process_truncation pads it) and a small one whose crop grows to the
150 x 120 minimum.  The directory name must contain a robot label ("panda") for DreamDataset to accept it.
"""
import json
import os

import numpy as np

FX, FY, CX, CY = 615.0, 615.0, 320.0, 240.0
NAMES = ["panda_link0", "panda_link2", "panda_link3", "panda_link4", "panda_link6", "panda_link7", "panda_hand"]
JOINTS = ["panda_joint%d" % i for i in range(1, 8)] + ["panda_finger_joint1"]

# per frame: key-point pixel centre (u, v), spread (px), depth (cm, the synthetic datasets' unit), frame size
FRAMES = [
    dict(center=(330.0, 250.0), spread=(120.0, 140.0), depth=120.0, size=(640, 480)),   # centred
    dict(center=(70.0, 200.0), spread=(110.0, 150.0), depth=110.0, size=(640, 480)),    # crop clamped at the left border
    dict(center=(600.0, 420.0), spread=(130.0, 120.0), depth=100.0, size=(640, 480)),   # key-points past the right / bottom edge
    dict(center=(300.0, 230.0), spread=(25.0, 20.0), depth=300.0, size=(640, 480)),     # small: 150 x 120 minimum crop
    dict(center=(200.0, 150.0), spread=(90.0, 70.0), depth=150.0, size=(400, 300)),     # another frame size
]


def texture(h, w, seed):
    """uint8 [h, w, 3]: gradients + stripes + seeded noise."""
    rng = np.random.Generator(np.random.PCG64(seed))
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    r = 128 + 90 * np.sin(x / 23.0 + seed) * np.cos(y / 31.0)
    g = 128 + 100 * np.sin((x + y) / 17.0 + 0.5 * seed)
    b = 60 + 150 * ((np.floor(x / 8) + np.floor(y / 8)) % 2)
    img = np.stack([r, g, b], -1) + rng.normal(0, 6, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def frame_annotation(i, spec, seed):
    rng = np.random.Generator(np.random.PCG64(1000 + seed * 7 + i))
    cu, cv = spec["center"]
    su, sv = spec["spread"]
    z = spec["depth"] + rng.uniform(-10, 10, len(NAMES))
    u = cu + su * rng.uniform(-1, 1, len(NAMES))
    v = cv + sv * rng.uniform(-1, 1, len(NAMES))
    loc = np.stack([(u - CX) * z / FX, (v - CY) * z / FY, z], 1)
    kps = [{"name": n, "location": [float(a) for a in p], "projected_location": [float(a) for a in (uu, vv)]}
           for n, p, uu, vv in zip(NAMES, loc, FX * loc[:, 0] / loc[:, 2] + CX, FY * loc[:, 1] / loc[:, 2] + CY)]
    q = rng.normal(0, 1, 4)
    return {"objects": [{"class": "panda", "location": [float(a) for a in loc.mean(0)],
                         "quaternion_xyzw": [float(a) for a in q / np.linalg.norm(q)], "keypoints": kps}],
            "sim_state": {"joints": [{"name": "panda/" + j, "position": float(p)} for j, p in zip(JOINTS, rng.uniform(-1, 1, 8))]}}


def write_scene(dirpath, seed=0, frames=None):
    """Write the scene into dirpath (created); returns the list of jpg paths."""
    from PIL import Image
    os.makedirs(dirpath, exist_ok=True)
    with open(os.path.join(dirpath, "_camera_settings.json"), "w") as f:
        json.dump({"camera_settings": [{"intrinsic_settings": {"fx": FX, "fy": FY, "cx": CX, "cy": CY}}]}, f)
    paths = []
    for i, spec in enumerate(frames or FRAMES):
        w, h = spec["size"]
        p = os.path.join(dirpath, "%06d.rgb.jpg" % i)
        Image.fromarray(texture(h, w, seed * 100 + i)).save(p, quality=92)
        with open(os.path.join(dirpath, "%06d.json" % i), "w") as f:
            json.dump(frame_annotation(i, spec, seed), f)
        paths.append(p)
    return paths
