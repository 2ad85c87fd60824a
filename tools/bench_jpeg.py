#!/usr/bin/env python3
"""Timing of the device JPEG decode (csrc/jpeg.hip) at B = 64 frames of tests/dream_scene.texture, 640 x 480, quality 92 (4:2:0,
what DreamDataset's scenes hold).

Device events after warm-up, five rounds, median and spread (min .. max) of:
  * the entropy stage (clear + checksum + entropy launches) at 1 and at 64 segments per wave, without restart markers (one segment per
    image) and with one restart interval per MCU row (30 segments per image),
  * the pixel stage (inverse DCT + colour launches),
  * the whole hrp_jpeg_decode call,
  * the same with the many-lanes-per-segment entropy stage (jpeg.Batch(entropy="sync")): its entropy stage and the whole
    hrp_jpeg_decode_sync call at 32, 64, 128 and 256 bytes per sub-sequence with every segment a long one, the rounds the batch
    needed (the maximum over its segments), and the call at jpeg.SUBSEQ_BYTES for several values of min_subseq and for the
    default one,
  * the upload of the compressed bytes against the upload of the decoded frames (pageable host memory, as to_device has it),
and, on the host, Pillow's single-thread decode per frame.  Every decode is checked against Pillow's bytes before it is timed.
``python tools/bench_jpeg.py [--out FILE.json]``"""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hrpe_amd  # noqa: E402,F401
from hrpe_amd import _native as nv  # noqa: E402
from hrpe_amd.lib.dataset import jpeg as J  # noqa: E402
import dream_scene  # noqa: E402

DEV = torch.device("cuda:0")
B, H, W = 64, 480, 640
ROUNDS = 5


def rounds(fn, warmup, reps):
    """Median, min, max over ROUNDS of the mean time of `reps` calls, in microseconds."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / reps)
    return {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts)}


def encode(**kw):
    from PIL import Image
    out = []
    for i in range(B):
        buf = io.BytesIO()
        Image.fromarray(dream_scene.texture(H, W, i)).save(buf, format="JPEG", quality=92, **kw)
        out.append(buf.getvalue())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    from PIL import Image
    res = {"B": B, "frame": [H, W]}
    for label, kw in (("no_restart", {}), ("restart_per_mcu_row", {"restart_marker_rows": 1})):
        datas = encode(**kw)
        want = torch.from_numpy(np.stack([np.asarray(Image.open(io.BytesIO(d))) for d in datas]))
        b = J.Batch(datas, np.stack([J.parse_header(d) for d in datas]), DEV)
        b.launch()
        J.check_status(b.status)
        assert torch.equal(b.flat.view(B, H, W, 3).cpu(), want), "the device decode differs from Pillow"
        a = b.args()
        r = {"compressed_bytes": sum(len(d) for d in datas), "segments": len(b.segments)}
        for lanes in (1, 64):
            r[f"entropy_lanes{lanes}"] = rounds(lambda: nv.call("hrp_jpeg_decode_stage", 0, lanes, *a), 1, 3)
        r["pixel"] = rounds(lambda: nv.call("hrp_jpeg_decode_stage", 1, 0, *a), 3, 20)
        r["decode"] = rounds(b.launch, 1, 3)
        hdrs = np.stack([J.parse_header(d) for d in datas])

        def sync(S, m):
            bs = J.Batch(datas, hdrs, DEV, entropy="sync", subseq_bytes=S, min_subseq=m)
            bs.launch()
            J.check_status(bs.status)
            assert torch.equal(bs.flat, b.flat) and torch.equal(bs.coef, b.coef), "the sync decode differs from the segment path"
            sa = bs.sync_args()
            out = {"long": len(bs.long), "short": len(bs.short), "rounds_max": int(bs.rounds().max()) if len(bs.long) else 0,
                   "entropy": rounds(lambda: nv.call("hrp_jpeg_decode_sync_stage", 0, 0, 0, *sa), 2, 5),
                   "decode": rounds(bs.launch, 2, 5)}
            return out
        for S in (32, 64, 128, 256):
            r[f"sync_subseq{S}"] = sync(S, 1)
        for m in (4, 16, 17, 18, 32):
            r[f"sync_min_subseq{m}"] = sync(J.SUBSEQ_BYTES, m)
        r["sync_defaults"] = dict(sync(J.SUBSEQ_BYTES, J.MIN_SUBSEQ), subseq_bytes=J.SUBSEQ_BYTES, min_subseq=J.MIN_SUBSEQ)
        r["decode_again"] = rounds(b.launch, 1, 3)      # the segment path once more, behind the sync rows
        res[label] = r
        if not kw:
            comp = torch.from_numpy(np.frombuffer(b"".join(datas), dtype=np.uint8).copy())
            raw = want.clone()
            res["upload_compressed"] = dict(rounds(lambda: comp.to(DEV, non_blocking=True), 3, 20), bytes=comp.numel())
            res["upload_frames"] = dict(rounds(lambda: raw.to(DEV, non_blocking=True), 3, 20), bytes=raw.numel())
            torch.set_num_threads(1)
            t0 = time.perf_counter()
            for d in datas:
                np.asarray(Image.open(io.BytesIO(d)))
            res["pillow_decode_ms_per_frame"] = (time.perf_counter() - t0) / B * 1e3
    for k, v in res.items():
        print(k, json.dumps(v))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
