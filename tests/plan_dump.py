#!/usr/bin/env python3
"""Canonical text form of a finalised plan (helper of tests/test_plan_finalize_host.py and of refactors of plan.py / plan_passes.py:
a change that is meant to leave the plans alone is checked by comparing these dumps before and after).

``canonical(plan)`` -> list of text lines: every entry of the forward and the backward launch list (lane; marker kind, parent and
children; launch class and family; a batched launch's BatchInfo and fold descriptors; every field of every descriptor; for a plain
closure the C-ABI calls it makes, recorded with a stand-in for nv.call - nothing is launched), the pack tables, the three BatchNorm
tables, the counters, the weight-gradient scratch sizes, the streams and the cut positions of analyze_backward_split.

Pointers are written as region+offset for the plan's own arenas (stats, bsums, grad_arena, the packed-weight arenas, the
weight-gradient scratch buffers) and as @k, k = order of first appearance, for every other address: neither the allocation order nor
the process shows, offsets inside the arenas and the scratch do.  Plain integer arguments of a recorded call carry no type: one of
2^32 or more counts as an address (no size or count of these plans comes near it).

``python tests/plan_dump.py OUTDIR`` builds a fixed set of plans on cuda:0 (no launch), writes OUTDIR/<name>.txt and prints
``sha256  name`` per plan."""
import ctypes as C
import hashlib
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import hrpe_amd  # noqa: E402,F401
from hrpe_amd import _native as nv  # noqa: E402
from hrpe_amd import plan as P  # noqa: E402

INFO_SCALARS = ("family", "n", "dtype", "variant", "grid", "lds_bytes", "grid2", "grid3", "lds_bytes3")


class _Pointers:
    """address -> 'region+offset' / '@k'"""

    def __init__(self, plan):
        self.regions, self.other = [], {}
        self.add("stats", plan.stats)
        self.add("bsums", plan.bsums)
        if plan.grad_arena is not None:
            self.add("grad_arena", plan.grad_arena)
        seen = set()
        for w in plan.weight_list:
            a = getattr(w, "arena", None)
            if a is not None and a.data_ptr() not in seen:
                seen.add(a.data_ptr())
                self.add("packed_" + str(a.dtype).replace("torch.", ""), a)
        for lane in sorted(plan.wgrad_ws):
            self.add(f"wgrad_ws[{lane}]", plan.wgrad_ws[lane])

    def add(self, name, t):
        if t.numel():
            self.regions.append((name, t.data_ptr(), t.numel() * t.element_size()))

    def __call__(self, addr):
        if not addr:
            return "null"
        for name, base, nbytes in self.regions:
            if base <= addr < base + nbytes:
                return f"{name}+{addr - base}"
        return "@%d" % self.other.setdefault(addr, len(self.other))


def _value(v, ctype, ptr):
    """One field / array element / call argument as text (the walk of plan_passes.analyze_backward_split, with the field types)."""
    if ctype is not None and issubclass(ctype, C.c_void_p):
        return ptr(v.value if isinstance(v, C.c_void_p) else v)
    if isinstance(v, C.Structure):
        return "{" + " ".join(f"{name}={_value(getattr(v, name), t, ptr)}" for name, t in v._fields_) + "}"
    if isinstance(v, C.Array):
        return "[" + " ".join(_value(x, v._type_, ptr) for x in v) + "]"
    if isinstance(v, C.c_void_p):
        return ptr(v.value)
    if hasattr(v, "_obj"):            # ctypes.byref(struct)
        return _value(v._obj, None, ptr)
    if v is None:
        return "null"
    if isinstance(v, int) and not isinstance(v, bool) and ctype is None and v >= 1 << 32:
        return ptr(v)
    return repr(v)


def _table(tdev, n, ctype, ptr):
    raw = bytes(tdev.cpu().numpy().tobytes())
    rows = (ctype * n).from_buffer_copy(raw[:C.sizeof(ctype) * n])
    return [_value(r, None, ptr) for r in rows]


def canonical(plan):
    ptr = _Pointers(plan)
    lines, calls = [], []
    real = nv.call
    nv.call = lambda name, *args: calls.append(name + "(" + ", ".join(_value(a, None, ptr) for a in args) + ")") and None
    try:
        for side, ops in (("fwd", plan.fwd_ops()), ("bwd", plan.bwd_ops())):
            for i, e in enumerate(ops):
                op, head = e.op, f"{side}[{i}] lane={e.lane}"
                if e.lane is None:
                    lines.append(f"{head} marker {getattr(op, 'kind', 'pack_join')} parent={getattr(op, 'parent', None)} "
                                 f"children={getattr(op, 'children', None)}")
                elif hasattr(op, "launches"):
                    lines.append(f"{head} {type(op).__name__} {op.fam}")
                    if isinstance(op, P.BatchLaunch):
                        info = "none" if op.info is None else " ".join(f"{k}={getattr(op.info, k)}" for k in INFO_SCALARS) + \
                            f" ws_bytes={list(op.info.ws_bytes[:op.info.n])} blk0={list(op.info.blk0[:op.info.n + 1])}" \
                            f" blk2={list(op.info.blk2[:op.info.n + 1])}"
                        lines.append(f"  singles={op.singles} info {info}")
                    for it in op.launches():
                        lines.append("  item " + _value(it.desc, None, ptr))
                    if isinstance(op, P.BatchLaunch) and op.fam == "wgrad" and op.items[0].desc.phase == 1:
                        lines += ["  fold " + _value(f, None, ptr) for f in op.fold_descs()]
                else:
                    del calls[:]
                    op(0)
                    lines.append(f"{head} closure")
                    lines += ["  call " + c for c in calls]
    finally:
        nv.call = real
    for name, tabs in (("pack", plan._pack_tables), ("pack_late", plan._pack_tables_late)):
        for tdev, fdev, n, nblk, cdt in tabs:
            lines.append(f"{name} n={n} blocks={nblk} dtype={cdt} first={fdev.cpu().tolist()}")
            lines += ["  row " + r for r in _table(tdev, n, nv.PackEntry, ptr)]
    for name in ("_run_tab", "_fold_tab", "_pgrad_tab"):
        tab = getattr(plan, name)
        lines.append(f"bn{name} n={tab[1] if tab else 0}")
        if tab:
            lines += ["  row " + r for r in _table(tab[0], tab[1], nv.BnEntry, ptr)]
    lines.append("counters " + " ".join(f"{k}={v}" for k, v in sorted(plan.counters.items())))
    lines.append("wgrad_ws " + " ".join(f"{lane}:{plan.wgrad_ws[lane].numel()}" for lane in sorted(plan.wgrad_ws)))
    lines.append(f"n_lanes={plan.n_lanes} side_streams={[s is not None for s in plan._side_streams]} "
                 f"pack_stream={plan._pack_stream is not None}")
    lines.append(f"split {plan.analyze_backward_split()}")
    lines.append(f"split_fracs {plan.analyze_backward_split(fracs=(0.25, 0.6, 0.9))}")
    return lines


# ---- the fixed set of plans ----------------------------------------------------------------------------------------------------
def build_plan(module, tensors, times=None):
    """What PlannedModule._run does up to the finished plan (nothing runs); the inputs are bound, so that the closures can be replayed."""
    need_grad = module.training
    plan = P.Plan(tensors[0].device, module._compute_dtype, module.training, need_grad)
    plan.x3 = bool(module._x3)
    if need_grad:
        plan.preallocate_param_grads(list(module.parameters()))
    pb = P.PlanBuilder(plan)
    in_names, outs, _ = module._build(pb, *tensors)
    for kind, h, _shape in outs:
        pb.output(h["handle"] if kind == "nchw" else h)
    t0 = time.perf_counter()
    pb.finish()
    if times is not None:
        times.append(time.perf_counter() - t0)
    plan.dyn.update(zip(in_names, tensors))
    return plan


def patched(**switches):
    """Context manager: plan.X = value for the duration of a build."""
    import contextlib

    @contextlib.contextmanager
    def cm():
        saved = {k: getattr(P, k) for k in switches}
        try:
            for k, v in switches.items():
                setattr(P, k, v)
            yield
        finally:
            for k, v in saved.items():
                setattr(P, k, v)
    return cm()


def plan_set(dev):
    """-> [(name, switches, function building the plan)]"""
    import argparse
    import bench
    from hrpe_amd.lib.models.ctrnet.keypoint_seg_resnet import KeyPointSegNet
    B = 2
    g = torch.Generator().manual_seed(3)

    def full(dtype, training, backbone="hrnet32"):
        def make(times=None):
            bench.REG_BACKBONE = backbone
            try:
                m = bench.build_model(0.5 if training else 0.0)
            finally:
                bench.REG_BACKBONE = "hrnet32"
            m = m.to(dev).set_compute_dtype(dtype).train(training)
            x = [torch.rand(B, 3, 256, 256, generator=g).to(dev) for _ in range(2)]
            kv, K = torch.full((B, 1), 3000.0, device=dev), torch.eye(3, device=dev).reshape(1, 9).repeat(B, 1)
            return build_plan(m, (x[0], x[1], kv, K, m.init_pose.expand(B, -1).float().contiguous(),
                                  m.init_rot.expand(B, -1).float().contiguous()), times)
        return make

    def depthnet(times=None):
        m = bench.build_depthnet().to(dev).set_compute_dtype(torch.bfloat16).train()
        return build_plan(m, (torch.rand(B, 3, 256, 256, generator=g).to(dev), torch.full((B, 1), 3000.0, device=dev)), times)

    def segnet(times=None):
        a = argparse.Namespace(use_gpu=True, n_kp=7, height=64, width=96)
        torch.manual_seed(1234)
        m = KeyPointSegNet(a).eval().to(dev).set_compute_dtype(torch.bfloat16)
        m._select_plans(True)
        return build_plan(m, (torch.rand(B, 3, 64, 96, generator=g).to(dev),), times)

    out = []
    for vname, dtype, training in (("train_bf16", torch.bfloat16, True), ("train_fp32", torch.float32, True), ("eval_bf16", torch.bfloat16, False)):
        for mode in ("hybrid", "merged", "lanes"):
            out.append((f"full_{vname}_{mode}", dict(PLAN_MODE=mode), full(dtype, training)))
        for sname, sw in (("nodefer", dict(WGRAD_DEFER=False)), ("nobatch", dict(BATCHING=False)), ("sink0", dict(WGRAD_SINK=0)),
                          ("sink3", dict(WGRAD_SINK=3))):
            out.append((f"full_{vname}_hybrid_{sname}", dict(PLAN_MODE="hybrid", **sw), full(dtype, training)))
    out.append(("full_resnet50_train_bf16", {}, full(torch.bfloat16, True, "resnet50")))
    out.append(("depthnet_train_bf16", {}, depthnet))
    out.append(("segnet_eval_bf16_keypoints", {}, segnet))
    return out


def main(outdir, dev="cuda:0", only=None):
    os.makedirs(outdir, exist_ok=True)
    dev = torch.device(dev)
    for name, switches, make in plan_set(dev):
        if only and only not in name:
            continue
        times = []
        with patched(**switches), torch.no_grad():
            plan = make(times)
            text = "\n".join(canonical(plan)) + "\n"
        with open(os.path.join(outdir, name + ".txt"), "w") as fh:
            fh.write(text)
        print(f"{hashlib.sha256(text.encode()).hexdigest()}  {name}  (finish() {times[0] * 1e3:.0f} ms)", flush=True)
        del plan


if __name__ == "__main__":
    main(*sys.argv[1:])
