#!/usr/bin/env python3
"""Cost of gradient accumulation over micro-batches (PlannedModule.set_grad_accumulation) on the benchmark network:

1. hrp_grad_accumulate alone over a buffer of the network's gradient-arena size, first micro-batch (reads src, writes acc: 8 bytes
   per element) and later ones (reads src and acc, writes acc: 12 bytes per element): device events around `reps` launches after
   warm-up, five rounds, median and spread, bytes / time beside the rate of the repository's memory-bound pointwise kernels.
2. one micro-batch (forward + loss + backward through the module's graph cache, no optimizer) with accumulation off and on, five
   rounds alternating the two modes; the difference is what the mode costs per micro-batch.

Run on the GPU box: ``python tools/bench_grad_accum.py [--batch 16] [--dtype fp32]``."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from hrpe_amd import _native as nv  # noqa: E402
from hrpe_amd.lib.core.function import compute_k_values  # noqa: E402

DEV = torch.device("cuda:0")
POINTWISE_TBS = (5.1, 5.5)     # README round 6: what the memory-bound element-wise kernels of this library reach


def timeit(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps     # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16, help="images per micro-batch")
    ap.add_argument("--dtype", default="fp32", choices=["bf16", "fp32", "fp32x3"])
    ap.add_argument("--steps", type=int, default=4, help="micro-batches per accumulation cycle")
    a = ap.parse_args()
    m = bench.build_model(0.5).to(DEV)
    m.set_compute_dtype({"bf16": torch.bfloat16, "fp32": torch.float32, "fp32x3": "fp32x3"}[a.dtype]).train()
    d = {k: torch.tensor(v).to(DEV) for k, v in bench.synthetic_batch(a.batch, 808).items()}
    K = d["K"]
    kv = compute_k_values(K[:, 0, 0], K[:, 1, 1], d["bbox"])

    def micro_batch():
        pred = m(d["x_reg"], d["x_root"], kv, K)
        sum(p.float().mean() for p in pred).backward()

    def cycle():
        m.begin_accumulation()
        for _ in range(a.steps):
            micro_batch()

    micro_batch()
    n = m.flat_grads()[0].numel()
    s = torch.cuda.current_stream(DEV).cuda_stream
    src, acc = torch.randn(n, device=DEV), torch.randn(n, device=DEV)
    print(f"gradient arena: {n} floats ({4 * n / 1e6:.1f} MB)")
    for first, nbytes in ((1, 8 * n), (0, 12 * n)):
        for scale in (1.0, 0.25):
            t = sorted(timeit(lambda: nv.call("hrp_grad_accumulate", src.data_ptr(), acc.data_ptr(), n, first, scale, s), 10, 50)
                       for _ in range(5))
            med = statistics.median(t)
            print(f"hrp_grad_accumulate first={first} scale={scale}: {med:7.1f} us ({t[0]:.1f} .. {t[-1]:.1f}), "
                  f"{nbytes / med / 1e6:.2f} TB/s = {nbytes / med / 1e6 / POINTWISE_TBS[0]:.2f} .. {nbytes / med / 1e6 / POINTWISE_TBS[1]:.2f} "
                  f"of the pointwise kernels' {POINTWISE_TBS[0]} .. {POINTWISE_TBS[1]} TB/s")
    del src, acc
    rounds = []
    for _ in range(5):
        m.set_grad_accumulation(1)
        off = timeit(cycle, 2, 5) / a.steps
        m.set_grad_accumulation(a.steps)
        on = timeit(cycle, 2, 5) / a.steps
        rounds.append((off, on))
    off, on = [sorted(c) for c in zip(*rounds)]
    mo, mn = statistics.median(off), statistics.median(on)
    print(f"micro-batch B={a.batch} {a.dtype} (forward + loss + backward): accumulation off {mo / 1e3:8.3f} ms "
          f"({off[0] / 1e3:.3f} .. {off[-1] / 1e3:.3f}), on (steps={a.steps}) {mn / 1e3:8.3f} ms ({on[0] / 1e3:.3f} .. {on[-1] / 1e3:.3f}): "
          f"{(mn - mo):+.0f} us per micro-batch")


if __name__ == "__main__":
    main()
