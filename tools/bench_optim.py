#!/usr/bin/env python3
"""Cost of reading Adam's hyper-parameters from device memory, on tensors of the benchmark network's parameter shapes:

  old     hrp_opt_grad_sumsq + hrp_opt_adam_step         lr / betas / eps as launch arguments: FusedClipAdam as bench.py builds it
  one     hrp_opt_grad_sumsq + hrp_opt_adam_step_groups  device_hyper=True, one group, no weight decay (the same bits as `old`)
  two     hrp_opt_grad_sumsq + hrp_opt_adam_step_groups  two groups (the parameter list cut in halves), weight decay 1e-2 in the second

Each is a whole clipped step (two launches and the step counter's increment), eager, timed with device events around `--reps` steps
after warm-up; five rounds that alternate the three; median and min .. max per variant.  `old` is the yardstick: the bytes moved are
identical (16 bytes read + 16 written per element), so `one` is expected inside `old`'s own min .. max.
The setter (hrp_opt_set_group, what publish_hyper() issues per changed group) is timed too: `--reps` one-thread launches.

Run on the GPU box: ``python tools/bench_optim.py [--reps 50]``."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from hrpe_amd import _native as nv  # noqa: E402
from hrpe_amd.optim import FusedClipAdam  # noqa: E402

DEV = torch.device("cuda:0")


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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    shapes = [tuple(p.shape) for p in bench.build_model(0.5).parameters() if p.requires_grad]
    n = sum(torch.Size(s).numel() for s in shapes)
    print(f"{len(shapes)} tensors, {n} parameters ({4 * n / 1e6:.1f} MB each for p, g, m, v; 32 bytes moved per element and step)")
    g = torch.Generator(device="cpu").manual_seed(1)

    def make(**kw):
        ps = [torch.nn.Parameter(torch.randn(s, generator=g).to(DEV)) for s in shapes]
        for p in ps:
            p.grad = torch.randn_like(p) * 0.01
        half = len(ps) // 2
        groups = kw.pop("groups", False)
        opt = FusedClipAdam([{"params": ps[:half]}, {"params": ps[half:], "lr": 3e-5, "weight_decay": 1e-2}] if groups else ps,
                            lr=1e-4, max_norm=5.0, **kw)
        opt.prepare()
        return opt

    variants = {"old": make(), "one": make(device_hyper=True), "two": make(groups=True)}
    assert not variants["old"]._device_hyper and variants["one"]._device_hyper and len(variants["two"].param_groups) == 2
    times = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, opt in variants.items():
            times[k].append(timeit(opt.step, 5, a.reps))
    for k, t in times.items():
        t = sorted(t)
        med = statistics.median(t)
        print(f"{k:4s} step: median {med:8.1f} us (min {t[0]:.1f} .. max {t[-1]:.1f}), {32 * n / med / 1e6:.2f} TB/s over the whole step")
    lo, hi = min(times["old"]), max(times["old"])
    for k in ("one", "two"):
        med = statistics.median(times[k])
        print(f"{k}: median {'inside' if lo <= med <= hi else 'OUTSIDE'} old's min .. max ({lo:.1f} .. {hi:.1f} us), "
              f"{(med / statistics.median(times['old']) - 1) * 100:+.2f} % against old's median")
    opt = variants["two"]
    s = torch.cuda.current_stream(DEV).cuda_stream
    t = sorted(timeit(lambda: nv.call("hrp_opt_set_group", opt._groups.data_ptr(), 2, 1, 3e-5, 0.9, 0.999, 1e-8, 1e-2, s), 10, a.reps)
               for _ in range(a.rounds))
    print(f"hrp_opt_set_group: median {statistics.median(t):.1f} us per launch, back to back (min {t[0]:.1f} .. max {t[-1]:.1f})")


if __name__ == "__main__":
    main()
