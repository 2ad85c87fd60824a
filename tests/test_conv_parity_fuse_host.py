"""Host side of the parity-fused stride-2 data gradient (csrc/conv_parity.h): the query hrp_conv_parity_fusable, the grouping of a
HRP_BATCH_CONV prepare into one fused problem per layer, the paths that must stay what they were, the cut rule of the lock-step merge
and a small training plan.  No GPU: prepare makes no HIP call, the pointers are made-up addresses."""
import ctypes as C

import pytest
import torch

import hrpe_amd  # noqa: F401
from hrpe_amd import _native as nv
from hrpe_amd import conv_geometry as G
from hrpe_amd import plan as P
from hrpe_amd import plan_passes as PP

BF16, F32 = nv.HRP_BF16, nv.HRP_F32
PARITY_VARIANT = 209


def class_descs(base, N, H, W, cdy, cdx, pad4, res=True, dtype=BF16, pitch=None):
    """The four class descriptors of the data gradient of a 3x3 stride-2 layer with the input [N, H, W, cdx] and the output gradient
    [N, ceil(H / 2), ceil(W / 2), cdy], filled by the function the plans use."""
    src = G.Operand(base, N, (H + 1) // 2, (W + 1) // 2, cdy, cdy)
    dst = G.Operand(base + 0x4000000, N, H, W, cdx, pitch or cdx)
    return [G.fill_conv(geo, src, dst, dtype, w=base + 0x8000000, res=(dst.ptr, dst.pitch) if res else None)
            for geo in G.data_grad_s2(H, W, 3, pad4)]


def fusable(d):
    return nv.lib().hrp_conv_parity_fusable(C.byref(d))


def prepare(descs):
    """-> (return code, info, the fused problems' tile configurations)."""
    n = len(descs)
    arr = (nv.ConvDesc * n)(*descs)
    info = nv.BatchInfo()
    host = (C.c_char * int(nv.lib().hrp_batch_table_bytes(nv.BATCH_CONV, n)))()
    rc = nv.lib().hrp_batch_prepare(nv.BATCH_CONV, arr, n, host, C.byref(info))
    cfgs = (C.c_int32 * nv.BATCH_MAX)()
    nq = nv.lib().hrp_batch_conv_parity_configs(host, C.byref(info), cfgs) if rc == 0 else 0
    return rc, info, list(cfgs[:max(nq, 0)])


def blocks(N, Ho, Wo, cout, cfg):
    """Workgroups of a fused problem on the Ho x Wo dy grid for a tile configuration, from the tile rule of csrc/conv_tile.h (plan_cfg):
    TW = the power of two >= Wo up to 16, TH likewise up to BM pixels, the rest of BM in images."""
    BM, BN = {1214: (256, 32), 1114: (128, 32), 2114: (128, 64)}[cfg]
    TW = 1
    while TW < Wo and TW < 16:
        TW *= 2
    TH = 1
    while TH < Ho and TH * TW < BM:
        TH *= 2
    TI = min(BM // (TW * TH), N)
    cd = lambda a, b: -(-a // b)      # noqa: E731
    return cd(Wo, TW) * cd(Ho, TH) * cd(N, TI) * cd(cout, BN)


def test_fusable_query():
    for pad4 in (False, True):
        ds = class_descs(0x100000, 2, 12, 16, 48, 32, pad4)
        assert [d.ntaps for d in ds] == ([4, 4, 4, 4] if pad4 else [1, 2, 2, 4]) and [d.w_ntaps for d in ds] == [10 if pad4 else 9] * 4
        assert [fusable(d) for d in ds] == [1, 1, 1, 1]
        assert [fusable(d) for d in class_descs(0x100000, 2, 12, 16, 48, 32, pad4, res=False)] == [1, 1, 1, 1]
    # odd H or W: the classes walk grids of different sizes
    for H, W in ((11, 16), (12, 15), (9, 7)):
        assert [fusable(d) for d in class_descs(0x100000, 2, H, W, 16, 32, True)] == [0, 0, 0, 0]
    assert [fusable(d) for d in class_descs(0x100000, 2, 12, 16, 16, 32, False, dtype=F32)] == [0, 0, 0, 0]
    assert nv.lib().hrp_conv_parity_fusable(None) == 0

    def changed(cls=3, pad4=True, **fields):
        d = class_descs(0x100000, 2, 12, 16, 48, 32, pad4)[cls]
        for k, v in fields.items():
            setattr(d, k, v)
        return d
    assert fusable(changed()) == 1
    for fields in (dict(relu=1), dict(stats=0x7000000), dict(bias=0x7000000), dict(scale=0x7000000, shift=0x7000000), dict(bnb_x=0x7000000),
                   dict(pro_mode=1), dict(res_mask=0x7000000), dict(tail_mode=1), dict(out_stride=1), dict(in_stride=2), dict(Cout=28),
                   dict(Cin=40), dict(y_pitch=36), dict(res_pitch=36), dict(y_H=14), dict(w_ntaps=16), dict(out_off_x=2)):
        assert fusable(changed(**fields)) == 0, fields
    # the real taps are the class's, in its order; a padding tap reads the zero slot
    d = changed(cls=1)
    d.dx[0], d.dx[1] = d.dx[1], d.dx[0]
    assert fusable(d) == 0
    d = changed(cls=2)
    d.wtap[1] = 4
    assert fusable(d) == 0
    d = changed(cls=0)
    assert d.ntaps == 4 and d.wtap[3] == 9
    d.wtap[3] = 8
    assert fusable(d) == 0
    d = changed(cls=0, pad4=False, ntaps=4)      # four taps on a packing without the zero slot
    assert fusable(d) == 0
    # the 1x1 stride-2 gradient is another problem
    (d,) = [G.fill_conv(geo, G.Operand(0x100000, 2, 6, 8, 16, 16), G.Operand(0x200000, 2, 12, 16, 32, 32), BF16, w=0x300000)
            for geo in G.data_grad_s2(12, 16, 1)]
    assert fusable(d) == 0


def test_prepare_fuses_complete_quadruples_in_any_order(monkeypatch):
    layers = [class_descs(0x10000000, 64, 64, 64, 64, 32, True),            # 64 -> 32, dy 32 x 32
              class_descs(0x20000000, 64, 32, 32, 128, 64, False),          # 128 -> 64, dy 16 x 16, unpadded next to padded
              class_descs(0x30000000, 3, 10, 12, 16, 128, True, res=False, pitch=136)]
    order = [5, 0, 11, 6, 2, 9, 4, 1, 8, 3, 7, 10]
    descs = [d for l in layers for d in l]
    monkeypatch.setenv("HRP_PARITY_MIN_WGS", "0")      # the largest tiles whatever the launch size
    rc, info, cfgs = prepare([descs[i] for i in order])
    assert rc == 0, nv.lib().hrp_last_error()
    assert info.variant == PARITY_VARIANT and info.n == 12 and cfgs == [2114, 1214, 2114]
    # heaviest K loop first: 128 dy channels, then 64, then 16; one block range per layer, the other table entries parked at the grid
    want = [blocks(64, 16, 16, 64, 2114), blocks(64, 32, 32, 32, 1214), blocks(3, 5, 6, 128, 2114)]
    assert want == [128, 256, 4]
    assert [info.blk0[i + 1] - info.blk0[i] for i in range(3)] == want
    assert info.grid == sum(want) and all(info.blk0[i] == info.grid for i in range(3, 13))
    assert 0 < info.lds_bytes <= 80 * 1024
    # below two workgroups per CU the launch takes the 128 x 32 tile for every problem
    monkeypatch.delenv("HRP_PARITY_MIN_WGS")
    rc, info, cfgs = prepare([descs[i] for i in order])
    want = [blocks(64, 16, 16, 64, 1114), blocks(64, 32, 32, 32, 1114), blocks(3, 5, 6, 128, 1114)]
    assert rc == 0 and info.variant == PARITY_VARIANT and cfgs == [1114] * 3 and want == [256, 512, 8]
    assert [info.blk0[i + 1] - info.blk0[i] for i in range(3)] == want and info.grid == sum(want)
    # ... and keeps the large ones where they fill the chip
    big = class_descs(0x10000000, 64, 128, 128, 64, 32, True) + class_descs(0x20000000, 64, 64, 64, 128, 64, True)
    rc, info, cfgs = prepare(big)
    assert rc == 0 and cfgs == [2114, 1214] and info.grid == blocks(64, 32, 32, 64, 2114) + blocks(64, 64, 64, 32, 1214)


def test_prepare_keeps_the_old_path_for_anything_else():
    def old_path(descs, variant):
        rc, info, cfgs = prepare(descs)
        assert rc == 0, nv.lib().hrp_last_error()
        assert info.variant == variant and cfgs == [] and info.blk0[len(descs)] == info.grid
        return info

    ref = old_path(class_descs(0x10000000, 2, 11, 16, 16, 32, True), 104)          # odd H: four padded 4-tap problems, the LIGHT kernel
    assert [ref.blk0[i + 1] - ref.blk0[i] > 0 for i in range(4)] == [True] * 4
    old_path(class_descs(0x10000000, 2, 12, 15, 16, 32, True), 104)                # odd W
    quad = class_descs(0x10000000, 2, 12, 16, 16, 32, True)
    assert prepare(quad)[1].variant == PARITY_VARIANT
    prev = nv.lib().hrp_conv_parity_fuse_enable(0)                                 # the library's switch (plan.PARITY_FUSE sets it)
    try:
        assert prev == 1
        old_path(quad, 104)
    finally:
        assert nv.lib().hrp_conv_parity_fuse_enable(prev) == 0
    assert prepare(quad)[1].variant == PARITY_VARIANT
    old_path(quad[:3], 104)                                                        # a missing class
    old_path(quad[:3] + quad[:1], 104)                                             # ... replaced by a repeated one
    other = class_descs(0x20000000, 2, 12, 16, 16, 32, True)
    old_path(quad[:3] + other[3:], 104)                                            # ... by the class of another layer
    mixed = class_descs(0x10000000, 2, 12, 16, 16, 32, True)
    mixed[2].res = 0x7000000                                                       # one class accumulates onto another tensor
    old_path(mixed, 104)
    for field in ("relu", "stats"):
        q = class_descs(0x10000000, 2, 12, 16, 16, 32, True)
        for d in q:
            setattr(d, field, 1 if field == "relu" else 0x7000000)
        old_path(q, 104)
    rc, info, cfgs = prepare(class_descs(0x10000000, 2, 12, 16, 16, 32, True, dtype=F32))      # a complete quadruple in fp32
    assert rc == 0 and (info.variant, info.dtype) == (104, F32) and cfgs == [] and all(info.blk0[i + 1] > info.blk0[i] for i in range(4))
    # unpadded classes: an incomplete quadruple under mixed tap counts is refused, as every mixed batch is
    un = class_descs(0x10000000, 2, 12, 16, 16, 32, False)
    assert prepare(un)[1].variant == PARITY_VARIANT
    rc, _, _ = prepare(un[:3])
    assert rc != 0 and b"mixed tap counts" in nv.lib().hrp_last_error()
    odd = class_descs(0x10000000, 2, 11, 16, 16, 32, False)
    rc, _, _ = prepare(odd)
    assert rc != 0 and b"mixed tap counts" in nv.lib().hrp_last_error()
    rc, _, _ = prepare(un + odd[3:])
    assert rc != 0


def test_two_layers_with_swapped_classes_are_two_complete_quadruples():
    """Completeness is per layer, not per position: classes of two layers interleaved are still two whole layers."""
    a, b = class_descs(0x10000000, 2, 12, 16, 16, 32, True), class_descs(0x20000000, 2, 12, 16, 16, 32, False)
    rc, info, cfgs = prepare(a[:3] + b[3:] + b[:3] + a[3:])
    assert rc == 0 and info.variant == PARITY_VARIANT and len(cfgs) == 2


def test_merge_key_and_cut_rule(monkeypatch):
    """Launch.merge_key gives the parity classes one key whatever their tap count; _merge_ops cuts a batch of them between layers only:
    at BATCH_MAX problems and where a layer writes what an earlier layer of the batch wrote."""
    pl = P.Plan(torch.device("cpu"), torch.bfloat16, True, True)
    layers = [class_descs(0x10000000 * (i + 1), 2, 12, 16, 16, 32, pad4=bool(i & 1)) for i in range(9)]
    ops = [P.Launch("conv", d) for l in layers for d in l]
    monkeypatch.setattr(P, "PARITY_FUSE", True)
    assert {op.merge_key() for op in ops} == {P.PARITY_KEY}
    out = P._merge_ops(pl, ops)
    assert [len(b.items) for b in out] == [32, 4] and out[0].items == ops[:32] and out[0].merge_key() == P.PARITY_KEY
    # batches that arrive from nested blocks merge by whole layers too
    out = P._merge_ops(pl, [P.BatchLaunch(pl, ops[0:4]), P.BatchLaunch(pl, ops[4:12])])
    assert [len(b.items) for b in out] == [12]
    # a layer that accumulates onto the tensor an earlier layer of the batch writes starts a new batch - with all four classes
    again = [P.Launch("conv", d) for d in class_descs(0x10000000, 2, 12, 16, 16, 32, True)]
    out = P._merge_ops(pl, ops[:8] + again + ops[8:12])
    assert [len(b.items) for b in out] == [8, 8] and out[1].items[:4] == again
    # an odd-sized layer keeps the tap-count keys; so does everything with the switch off
    odd = [P.Launch("conv", d) for d in class_descs(0x10000000, 2, 11, 16, 16, 32, False)]
    assert [op.merge_key() for op in odd] == [("conv", BF16, t) for t in (1, 2, 2, 4)]
    monkeypatch.setattr(P, "PARITY_FUSE", False)
    assert [op.merge_key() for op in ops[:8]] == [("conv", BF16, t) for t in (1, 2, 2, 4, 4, 4, 4, 4)]
    out = P._merge_ops(pl, [ops[4 * i + 3] for i in range(9)] + [ops[3]])       # the ordinary rule: one problem at a time
    assert [len(b.items) if isinstance(b, P.BatchLaunch) else 1 for b in out] == [9, 1]


def emit_backward(pl, pb, *outputs):
    """PlanBuilder.finish() without finalize(): the outputs' gradients come from outside, the backward emitters run in reverse."""
    for t in outputs:
        pb.output(t)
    for lane, path, emit in reversed(pb.bwd_stack):
        if lane is None:
            list.append(pl.bwd, P.Entry(None, (), emit))
        else:
            pl.cur_lane, pl.lane_path = lane, path
            emit()
    pl.cur_lane, pl.lane_path = 0, ()


def build_backward():
    """Two stride-2 3x3 layers side by side (the paths of a fuse layer): a small one, whose classes are padded to four taps, and one
    above 4 GFLOP of data gradient, whose classes keep 1 / 2 / 2 / 4.  -> the merged backward list."""
    g = torch.Generator().manual_seed(5)
    pl = P.Plan(torch.device("cpu"), torch.bfloat16, True, True)
    pb = P.PlanBuilder(pl)
    shapes = [(2, 16, 16, 32, 64), (2, 128, 128, 128, 256)]
    ws = [torch.nn.Parameter(torch.randn(co, ci, 3, 3, generator=g)) for _, _, _, ci, co in shapes]
    xs = []
    for N, H, W, ci, _ in shapes:
        x = pl.new(N, H, W, ci, torch.bfloat16)
        x.requires_grad = True
        xs.append(x)
    ys = []
    with pb.parallel(2, virtual=True) as par:
        for i in range(2):
            with par.lane(i):
                ys.append(pb.conv(xs[i], ws[i], stride=2))
    emit_backward(pl, pb, *ys)
    return pl, [e.op for e in PP.flatten(pl, pl.bwd)]


def test_training_plan_keeps_the_four_classes_of_each_layer_in_one_batch(monkeypatch):
    monkeypatch.setattr(P, "PLAN_MODE", "merged")
    monkeypatch.setattr(P, "PARITY_FUSE", True)
    pl, ops = build_backward()
    convs = [op for op in ops if P.is_fam(op, "conv")]
    assert len(convs) == 1 and isinstance(convs[0], P.BatchLaunch)
    items = convs[0].items
    assert [it.desc.ntaps for it in items] in ([4, 4, 4, 4, 1, 2, 2, 4], [1, 2, 2, 4, 4, 4, 4, 4])
    for q in (items[:4], items[4:]):
        assert len({(it.desc.x, it.desc.y) for it in q}) == 1 and [(it.desc.out_off_y, it.desc.out_off_x) for it in q] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    # the library fuses that batch (the packed-weight pointers, patched at finalize, stand in here)
    descs = []
    for it in items:
        d = nv.ConvDesc.from_buffer_copy(it.desc)
        d.w = 0x7000000 if d.Cout == 32 else 0x7800000
        descs.append(d)
    rc, info, cfgs = prepare(descs)
    assert rc == 0 and info.variant == PARITY_VARIANT and len(cfgs) == 2
    # the descriptors are what they are without the switch: launches by tap count then (the padded layer's four classes; the large
    # layer's 1-tap class, its two 2-tap classes and its 4-tap class, whose lane reaches it after the other lane's batch has gone)
    monkeypatch.setattr(P, "PARITY_FUSE", False)
    pl0, ops0 = build_backward()
    convs0 = [op for op in ops0 if P.is_fam(op, "conv")]
    assert sorted(len(op.launches()) for op in convs0) == [1, 1, 2, 4]
    assert all(len({it.desc.ntaps for it in op.launches()}) == 1 for op in convs0)

    def body(d):      # a descriptor without its addresses (the two plans allocate their own tensors)
        skip = {"x", "y", "w", "res"}
        return [(n, tuple(v) if hasattr(v, "__len__") else v) for n, _ in nv.ConvDesc._fields_ if n not in skip for v in [getattr(d, n)]]
    key = lambda d: (d.Cout, d.out_off_y, d.out_off_x)      # noqa: E731
    a = sorted((it.desc for it in items), key=key)
    b = sorted((it.desc for op in convs0 for it in op.launches()), key=key)
    assert [body(d) for d in a] == [body(d) for d in b]
    assert [bool(d.res) for d in a] == [bool(d.res) for d in b]
