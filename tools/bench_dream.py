#!/usr/bin/env python3
"""Timing of the DREAM pixel launches (csrc/dream.hip) and of the host side of DreamDataset.__getitem__.

Device: events around `reps` calls of the two launches (hrp_dream_augment + hrp_dream_crop_resize) at B = 64 on 640 x 480 frames
with the training defaults plus every stage forced (worst case), with and without process_truncation.  Host: __getitem__ per
sample (JPEG decode, JSON, draws, geometry) on the procedural scene of tests/dream_scene.py, one thread.  Run on the GPU box:
``python tools/bench_dream.py``."""
import os
import random
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hrpe_amd  # noqa: E402,F401
from hrpe_amd import _native as nv  # noqa: E402
from hrpe_amd.lib.dataset import dream as D  # noqa: E402
import dream_scene  # noqa: E402

DEV = torch.device("cuda:0")


def timeit(fn, warmup=10, reps=50):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def launches(ds, batch):
    tab, noise, sbytes = D.descriptor_table(batch["aug"], batch["noise"])
    B = len(tab)
    frames = batch["frame"].to(DEV)
    table = torch.from_numpy(tab.view(np.uint8).copy()).to(DEV)
    noise_d = torch.from_numpy(np.frombuffer(noise, np.uint8).copy()).to(DEV)
    scratch = torch.empty(max(sbytes, 1), dtype=torch.uint8, device=DEV)
    lsum = torch.empty(B, nv.DREAM_BANDS, dtype=torch.int64, device=DEV)
    out = torch.empty(B, 3, 256, 256, dtype=torch.uint8, device=DEV)
    mh, mw = int(tab["work_h"].max()), int(tab["work_w"].max())
    return lambda: D.pixel_launches(frames, table, noise_d, scratch, lsum, out, max_hw=(mh, mw)), sbytes


def main():
    base = os.path.join(tempfile.mkdtemp(), "panda_synth_bench")
    dream_scene.write_scene(base, frames=dream_scene.FRAMES[:4])
    B = 64
    saved = dict(D.RGB_AUGMENTATIONS)
    for trunc in (False, True):
        for forced in (False, True):
            if forced:
                for k, (p, iv) in saved.items():
                    D.RGB_AUGMENTATIONS[k] = (1.0, iv)
            D.JITTER_P = 1.0 if forced else 0.4
            ds = D.DreamDataset(base, process_truncation=trunc, occlu_p=1.0 if forced else 0.5)
            random.seed(0)
            np.random.seed(0)
            batch = torch.utils.data.default_collate([ds[i % len(ds)] for i in range(B)])
            fn, sbytes = launches(ds, batch)
            t = timeit(fn)
            print(f"B={B} 640x480 truncation={int(trunc)} {'all stages forced' if forced else 'training draws   '}: "
                  f"{t:8.1f} us for both launches (working frames {sbytes / 1e6:.1f} MB)")
            D.RGB_AUGMENTATIONS.update(saved)
            D.JITTER_P = 0.4
    torch.set_num_threads(1)
    ds = D.DreamDataset(base)
    random.seed(0)
    np.random.seed(0)
    for i in range(8):
        ds[i % len(ds)]
    n = 200
    t0 = time.perf_counter()
    for i in range(n):
        ds[i % len(ds)]
    print(f"host __getitem__ (decode + JSON + draws + geometry, 1 thread): {(time.perf_counter() - t0) / n * 1e3:.2f} ms / sample")


if __name__ == "__main__":
    main()
