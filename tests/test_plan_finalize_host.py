"""Plan.finalize on the host: small training plans are built with the real PlanBuilder on the CPU device and finalised in merged mode
(and in hybrid mode with virtual blocks only: neither creates a stream), nothing is launched.  Checked: the launch list the passes
produce, and where plan_passes.assign_wgrad_scratch puts the partial slabs of every weight-gradient problem - with deferred folds (the
default), with WGRAD_DEFER off (one buffer per stream), with BATCHING off, and for a launch marked `reserved`.

Plan A: three lanes, each its own input and two 3x3 convolutions 32 -> 32 (N = 2, 16 x 16, bf16): six parameters.
Plan B: the same with a 1x1 and a stride-2 3x3 convolution per lane."""
import ctypes as C

import pytest
import torch

import hrpe_amd  # noqa: F401
from hrpe_amd import _native as nv
from hrpe_amd import plan as P

from plan_dump import canonical

CPU = torch.device("cpu")
LAYERS = {"A": [(3, 1), (3, 1)], "B": [(1, 1), (3, 2)]}


def build(which="A", mode="merged", reserve=None, **switches):
    """-> finalised plan.  mode "hybrid": the lanes are a VIRTUAL block.  reserve: index of a weight-gradient launch of plan.bwd that is
    marked reserved = 1 before finalize().  switches: plan.X = value while the plan is built (restored afterwards)."""
    switches["PLAN_MODE"] = mode
    saved = {k: getattr(P, k) for k in switches}
    try:
        for k, v in switches.items():
            setattr(P, k, v)
        g = torch.Generator().manual_seed(1)
        layers = LAYERS[which]
        params = [torch.nn.Parameter(torch.randn(32, 32, k, k, generator=g)) for _ in range(3) for k, _ in layers]
        pl = P.Plan(CPU, torch.bfloat16, True, True)
        pl.preallocate_param_grads(params)
        pb = P.PlanBuilder(pl)
        with pb.parallel(3, virtual=mode == "hybrid") as par:
            for i in range(3):
                with par.lane(i):
                    x = pl.new(2, 16, 16, 32)
                    x.requires_grad = True
                    for j, (_, stride) in enumerate(layers):
                        x = pb.conv(x, params[len(layers) * i + j], stride=stride)
                    pb.output(x)
        if reserve is None:
            pb.finish()
        else:           # PlanBuilder.finish() with the flag set between the backward emitters and finalize()
            for lane, path, emit in reversed(pb.bwd_stack):
                if lane is None:
                    list.append(pl.bwd, P.Entry(None, (), emit))
                else:
                    pl.cur_lane, pl.lane_path = lane, path
                    emit()
            pl.cur_lane, pl.lane_path = 0, ()
            [e.op for e in pl.bwd if fam_of(e.op) == "wgrad"][reserve].desc.reserved = 1
            pl.finalize()
        return pl
    finally:
        for k, v in saved.items():
            setattr(P, k, v)


def fam_of(op):
    return getattr(op, "fam", None) if hasattr(op, "launches") else None


def shape_of(op):
    kind = "B%d" % len(op.items) if isinstance(op, P.BatchLaunch) else "L"
    return f"{kind}:{op.fam}"


def wgrad_ops(pl):
    return [e for e in pl.bwd_ops() if fam_of(e.op) == "wgrad"]


def single_need(d):
    return int(nv.lib().hrp_wgrad_workspace_bytes(C.byref(d)))


def regions_in(buf, descs, aligned=True):
    """The scratch regions of these descriptors lie inside `buf`, start at multiples of 256 bytes from its base and are pairwise
    disjoint.  -> [(offset, bytes)]"""
    base, size = buf.data_ptr(), buf.numel() * 4
    regs = []
    for d in descs:
        if not d.workspace_bytes:
            assert not d.workspace
            continue
        off = d.workspace - base
        assert 0 <= off and off + d.workspace_bytes <= size, (off, d.workspace_bytes, size)
        assert not aligned or off % 256 == 0
        regs.append((off, d.workspace_bytes))
    regs.sort()
    assert all(a + n <= b for (a, n), (b, _) in zip(regs, regs[1:])), regs
    return regs


@pytest.mark.parametrize("mode", ["merged", "hybrid"])
def test_deferred_folds_backward_list_and_scratch_regions(mode):
    pl = build("A", mode)
    assert pl.merged and pl._pack_stream is None and not any(pl._side_streams)
    assert [shape_of(e.op) for e in pl.bwd_ops()] == ["B3:conv", "B3:conv", "B6:wgrad", "B6:wgrad_fold"]
    assert {e.lane for e in pl.bwd_ops()} == {0} and sorted(pl.wgrad_ws) == [0]
    wg, fold = pl.bwd_ops()[2].op, pl.bwd_ops()[3].op
    assert not wg.singles and not fold.singles
    descs = [it.desc for it in wg.items]
    assert all(d.phase == 1 for d in descs)
    assert len(regions_in(pl.wgrad_ws[0], descs)) == 6
    for i, d in enumerate(descs):
        assert d.workspace_bytes >= single_need(d) and d.workspace_bytes >= wg.info.ws_bytes[i] > 0
    outs = [it.desc.dw + 4 * it.desc.dw_tap_off for it in fold.items]
    assert len(set(outs)) == 6 and set(outs) == {d.dw + 4 * d.dw_tap_off for d in descs}


@pytest.mark.parametrize("mode", ["merged", "hybrid"])
def test_deferred_folds_with_a_pointwise_and_a_strided_layer(mode):
    pl = build("B", mode)
    ents = wgrad_ops(pl)
    descs = [it.desc for e in ents for it in e.op.launches()]
    assert len(descs) == 6 and sorted(d.ntaps for d in descs) == [1, 1, 1, 9, 9, 9] and all(d.phase == 1 for d in descs)
    regions_in(pl.wgrad_ws[0], descs)
    for e in ents:
        for i, it in enumerate(e.op.launches()):
            assert it.desc.workspace_bytes >= single_need(it.desc)
            if isinstance(e.op, P.BatchLaunch) and not e.op.singles:
                assert it.desc.workspace_bytes >= e.op.info.ws_bytes[i]
    folds = [it.desc for e in pl.bwd_ops() if fam_of(e.op) == "wgrad_fold" for it in e.op.items]
    outs = [f.dw + 4 * f.dw_tap_off for f in folds]
    assert len(set(outs)) == len(outs) and set(outs) <= {d.dw + 4 * d.dw_tap_off for d in descs}
    # the folds come behind every weight-gradient launch of their lane
    fams = [fam_of(e.op) for e in pl.bwd_ops()]
    assert max(i for i, f in enumerate(fams) if f == "wgrad") < min(i for i, f in enumerate(fams) if f == "wgrad_fold")


@pytest.mark.parametrize("which", ["A", "B"])
def test_without_deferred_folds_one_buffer_per_stream(which):
    pl = build(which, WGRAD_DEFER=False)
    ents = wgrad_ops(pl)
    assert [shape_of(e.op) for e in ents] == ["B3:wgrad", "B3:wgrad"]
    assert all(fam_of(e.op) != "wgrad_fold" for e in pl.bwd_ops())
    assert sorted(pl.wgrad_ws) == [0]
    need = 0
    for e in ents:
        descs = [it.desc for it in e.op.items]
        assert all(d.phase == 0 for d in descs) and not e.op.singles
        regions_in(pl.wgrad_ws[e.lane], descs)
        for i, d in enumerate(descs):
            assert d.workspace_bytes == e.op.info.ws_bytes[i]
        need = max(need, sum((int(b) + 255) // 256 * 256 for b in e.op.info.ws_bytes[:3]))
    assert pl.wgrad_ws[0].numel() * 4 >= need > 0


def test_without_batching_the_same_launches_one_by_one():
    ref = build("A")
    pl = build("A", BATCHING=False)
    ops = [e.op for e in pl.bwd_ops()]
    assert all(isinstance(op, P.Launch) for op in ops if fam_of(op) != "wgrad_fold")
    key = lambda f, d: (f, d.ntaps, d.Cin, d.Cout, d.H, d.W, d.Ho, d.Wo)      # noqa: E731
    one_by_one = sorted(key(op.fam, op.desc) for op in ops if fam_of(op) in ("conv", "wgrad"))
    batched = sorted(key(e.op.fam, it.desc) for e in ref.bwd_ops() if fam_of(e.op) in ("conv", "wgrad") for it in e.op.launches())
    assert one_by_one == batched and len(one_by_one) == 12
    # each lane keeps its order: weight gradient and data gradient of the second layer, then of the first
    assert [op.fam for op in ops if fam_of(op) != "wgrad_fold"] == ["wgrad"] * 3 + ["conv"] * 3 + ["wgrad"] * 3 + ["conv"] * 3
    descs = [op.desc for op in ops if fam_of(op) == "wgrad"]
    assert len(regions_in(pl.wgrad_ws[0], descs)) == 6
    assert all(d.phase == 1 and d.workspace_bytes >= single_need(d) > 0 for d in descs)
    folds = [it.desc for op in ops if fam_of(op) == "wgrad_fold" for it in op.items]
    assert len({f.dw + 4 * f.dw_tap_off for f in folds}) == len(folds) == 6


def test_reserved_weight_gradient_stays_in_place_and_folds_itself():
    pl = build("A", reserve=0)
    ents = pl.bwd_ops()
    fams = [fam_of(e.op) for e in ents]
    (at,) = [i for i, e in enumerate(ents) if fams[i] == "wgrad" and any(it.desc.reserved for it in e.op.launches())]
    assert isinstance(ents[at].op, P.Launch)
    stay = ents[at].op.desc
    assert stay.reserved == 1 and stay.phase == 0 and stay.workspace_bytes >= single_need(stay)
    # not sunk: it still runs in front of its own layer's data gradient (the convolution that reads the same output gradient), while
    # the other five follow the last convolution
    dgrad = next(i for i, e in enumerate(ents) if fams[i] == "conv" and any(it.desc.x == stay.dy for it in e.op.launches()))
    last_conv = max(i for i, f in enumerate(fams) if f == "conv")
    assert at < dgrad
    rest = [it.desc for i, e in enumerate(ents) if fams[i] == "wgrad" and i != at for it in e.op.launches()]
    assert all(i > last_conv for i, f in enumerate(fams) if f == "wgrad" and i != at)
    assert len(rest) == 5 and all(d.phase == 1 and d.reserved == 0 for d in rest)
    regions_in(pl.wgrad_ws[0], [stay] + rest)
    folds = [it.desc for e in ents if fam_of(e.op) == "wgrad_fold" for it in e.op.items]
    outs = {f.dw + 4 * f.dw_tap_off for f in folds}
    assert len(folds) == 5 and stay.dw + 4 * stay.dw_tap_off not in outs and outs == {d.dw + 4 * d.dw_tap_off for d in rest}


@pytest.mark.parametrize("which", ["A", "B"])
def test_canonical_dump_of_two_builds_is_equal(which):
    a, b = canonical(build(which)), canonical(build(which))
    assert a == b and any(" BatchLaunch wgrad" in ln for ln in a) and any("workspace=wgrad_ws[0]+" in ln for ln in a)
    assert canonical(build(which, WGRAD_DEFER=False)) != a
