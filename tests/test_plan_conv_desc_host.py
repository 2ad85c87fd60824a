"""The convolution and weight-gradient descriptors the plans build, proved on the host: the real PlanBuilder emits a layer into a
plan on the CPU device (no finalize(): nothing is launched and the packed-weight pointers stay null), every Launch("conv") /
Launch("wgrad") descriptor of plan.fwd / plan.bwd is read back (conv_exact_oracle.problem_of / evaluate_wgrad), evaluated literally in
float64 and compared with torch's own float64 convolution and its autograd.  The packed weights are the test's (slots_fwd / slots_bwd
with the ParamW's pad_t).

Tolerance: rtol 0, atol 1e-12 max(1, max |ref|): float64 sums of at most a few thousand O(1) terms."""
import pytest
import torch
import torch.nn.functional as F

import conv_exact_oracle as O
from conv_exact_oracle import F64

import hrpe_amd  # noqa: F401
from hrpe_amd import plan as P

CPU = torch.device("cpu")
SENTINEL = 7.0
DTYPES = [torch.bfloat16, torch.float32]
IDS = ["bf16", "fp32"]


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def rnd(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F64)


def close(got, ref):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    atol = 1e-12 * max(1.0, float(ref.abs().max()))
    err = float((got - ref).abs().max())
    assert err <= atol, f"max |got - ref| = {err} > {atol}"


def builder(dtype, training=True, need_grad=True):
    pl = P.Plan(CPU, dtype, training, need_grad)
    return pl, P.PlanBuilder(pl)


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


def launches(lst, fam):
    return [e for e in lst if isinstance(e.op, P.Launch) and e.op.fam == fam]


def descs(lst, fam):
    return [e.op.desc for e in launches(lst, fam)]


def run_convs(ds, x, slots, y0=None, bias=None):
    """The conv launches `ds` (all writing one buffer) evaluated in order.  A launch with res set accumulates onto that buffer
    (res == y).  -> (the buffer, how often each element was written)."""
    d0 = ds[0]
    buf = torch.full((x.shape[0], d0.y_H, d0.y_W, d0.y_pitch), SENTINEL, dtype=F64) if y0 is None else y0.clone()
    seen = torch.zeros(buf.shape, dtype=torch.int32)
    for d in ds:
        assert d.y == d0.y and not d.w, "one destination; the packed-weight pointer is patched at finalize"
        assert d.res in (None, d.y)
        Pr = O.problem_of(d, x, slots, res=buf[..., :d.Cout] if d.res else None, bias=bias if d.bias else None)
        r = O.evaluate(Pr, y0=buf)
        assert torch.equal(r.y[~r.written], buf[~r.written])
        buf, seen = r.y, seen + r.written.int()
    return buf, seen


def run_wgrads(gs, x, dy, shape):
    """The weight-gradient launches `gs` of one parameter (tap groups write disjoint elements).  -> (dW, times written)."""
    dw, seen = None, None
    for g in gs:
        assert g.dw == gs[0].dw
        dw, wr = O.evaluate_wgrad(g, x, dy, dw0=dw)
        seen = wr.int() if seen is None else seen + wr.int()
    assert tuple(dw.shape) == tuple(shape), (dw.shape, shape)
    return dw, seen


def layer_reference(x, w, gy, stride, dilation):
    """float64 layer and its autograd: -> (y, dx, dW), NHWC / weight layout."""
    xg, wg = nchw(x).clone().requires_grad_(), w.clone().requires_grad_()
    k = w.shape[2]
    y = F.conv2d(xg, wg, stride=stride, padding=dilation * (k // 2), dilation=dilation)
    gx, gw = torch.autograd.grad(y, (xg, wg), nchw(gy) if gy is not None else torch.ones_like(y))
    return nhwc(y.detach()), nhwc(gx), gw


CONV_CASES = [  # (k, stride, dilation, (H, W))
    (3, 1, 1, (9, 7)), (3, 1, 1, (8, 12)), (3, 2, 1, (9, 7)), (3, 2, 1, (8, 12)), (1, 1, 1, (9, 7)), (1, 2, 1, (9, 12)), (3, 1, 2, (9, 7)),
    (3, 1, 2, (8, 12))]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("k,stride,dilation,hw", CONV_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_conv_layer_descriptors(k, stride, dilation, hw, dtype):
    """PlanBuilder.conv of a training plan: the forward descriptor, the data-gradient descriptor(s) and the weight-gradient descriptor."""
    g = torch.Generator().manual_seed(11 * k + stride + dilation + hw[0])
    N, (H, W), cin, cout = 2, hw, 8, 16
    weight = torch.nn.Parameter(torch.randn(cout, cin, k, k, generator=g))
    pl, pb = builder(dtype)
    xt = pl.new(N, H, W, cin, dtype)
    xt.requires_grad = True
    yt = pb.conv(xt, weight, stride=stride, dilation=dilation)
    emit_backward(pl, pb, yt)
    (wp,) = pl.weight_list
    x, w64 = rnd(g, N, H, W, cin), weight.detach().double()
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    assert (yt.H, yt.W) == (Ho, Wo)
    gy = rnd(g, N, Ho, Wo, cout)
    y_ref, gx_ref, gw_ref = layer_reference(x, w64, gy, stride, dilation)
    # forward
    (d,) = descs(pl.fwd, "conv")
    assert (d.x, d.y) == (xt.ptr(), yt.ptr())
    y, seen = run_convs([d], x, O.slots_fwd(w64.view(cout, cin, k * k)))
    close(y, y_ref)
    assert bool((seen == 1).all())
    # data gradient
    ents = launches(pl.bwd, "conv")
    ds = [e.op.desc for e in ents]
    assert all((q.x, q.y) == (yt.gptr(), xt.gptr()) for q in ds)
    slots_t = O.slots_bwd(w64.view(cout, cin, k * k), pad_t=wp.pad_t)
    assert wp.t_ntaps == {k * k + wp.pad_t}
    y0 = None
    if stride == 1:
        assert len(ds) == 1 and not ds[0].res
    elif k == 1:
        # only the even pixels receive a gradient: the one launch accumulates onto a buffer an hrp_fill_zero op cleared in front of it,
        # the three classes without a tap emit nothing
        assert len(ds) == 1 and ds[0].res == ds[0].y and (ds[0].out_off_y, ds[0].out_off_x, ds[0].out_stride) == (0, 0, 2)
        ops = [e.op for e in pl.bwd]
        assert not isinstance(ops[ops.index(ents[0].op) - 1], P.Launch)
        y0 = torch.zeros(N, H, W, xt.pitch, dtype=F64)
    else:
        padded = dtype == torch.bfloat16       # (PARITY_PAD: bf16 layers below 4 GFLOP of data gradient)
        assert wp.pad_t == (1 if padded else 0)
        assert [q.ntaps for q in ds] == ([4, 4, 4, 4] if padded else [1, 2, 2, 4])
        assert [q.w_ntaps for q in ds] == [9 + wp.pad_t] * 4
        # the class index selects the virtual lane
        assert [e.path[-1][1] for e in ents] == [2 * q.out_off_y + q.out_off_x for q in ds] == [0, 1, 2, 3]
    gx, seen = run_convs(ds, x=gy, slots=slots_t, y0=y0)
    close(gx, gx_ref)
    if not (stride == 2 and k == 1):
        assert bool((seen == 1).all()), "the launches write every pixel of the gradient exactly once"
    else:
        assert bool((seen[:, ::2, ::2] == 1).all()) and int(seen.sum()) == N * Ho * Wo * cin
    # weight gradient
    (gd,) = descs(pl.bwd, "wgrad")
    assert (gd.x, gd.dy, gd.dw_tap_stride, gd.dw_tap_off, gd.reserved) == (xt.ptr(), yt.gptr(), 0, 0, 0)
    dw, seen = run_wgrads([gd], x, gy, (cout, cin, k * k))
    close(dw, gw_ref.reshape(cout, cin, k * k))
    assert bool((seen == 1).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("dilation,hw,nlaunch", [(12, (20, 20), 9), (36, (30, 40), 3)])
def test_far_dilated_conv_is_the_sum_of_one_tap_launches(dilation, hw, nlaunch, dtype):
    """Dilation beyond MAX_TILE_DILATION (inference plans): one-tap problems on the rectangles whose source lies inside the image, the
    centre tap first (with the bias), the others accumulating onto it; at rate 36 on 30 rows the vertical taps vanish."""
    g = torch.Generator().manual_seed(dilation)
    N, (H, W), cin, cout = 1, hw, 8, 16
    assert dilation > P.MAX_TILE_DILATION
    weight, bias = torch.nn.Parameter(torch.randn(cout, cin, 3, 3, generator=g)), torch.nn.Parameter(torch.randn(cout, generator=g))
    pl, pb = builder(dtype, training=False, need_grad=False)
    xt = pl.new(N, H, W, cin, dtype)
    yt = pb.conv(xt, weight, bias=bias, dilation=dilation)
    ds = descs(pl.fwd, "conv")
    assert len(ds) == nlaunch and all(q.ntaps == 1 and q.w_ntaps == 9 for q in ds)
    assert ds[0].wtap[0] == 4 and ds[0].bias and not ds[0].res and all(q.res == q.y and not q.bias for q in ds[1:])
    assert sorted(q.wtap[0] for q in ds) == ([3, 4, 5] if nlaunch == 3 else list(range(9)))
    x, w64, b64 = rnd(g, N, H, W, cin), weight.detach().double(), bias.detach().double()
    y, seen = run_convs(ds, x, O.slots_fwd(w64.view(cout, cin, 9)), bias=b64)
    close(nchw(y), F.conv2d(nchw(x), w64, b64, padding=dilation, dilation=dilation))
    assert bool((seen >= 1).all())         # (the centre tap's rectangle is the whole image)
    assert yt.producer is None


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_deconv4x4s2_descriptors(dtype):
    """ConvTranspose2d(4, stride 2, padding 1): four forward parity launches that cover y exactly once, the 16-tap in_stride-2 data
    gradient, the weight gradient in four groups of four taps."""
    g = torch.Generator().manual_seed(5)
    N, H, W, cin_t, cout_t = 2, 6, 5, 8, 16
    weight = torch.nn.Parameter(torch.randn(cin_t, cout_t, 4, 4, generator=g))
    pl, pb = builder(dtype)
    xt = pl.new(N, H, W, cin_t, dtype)
    xt.requires_grad = True
    yt = pb.deconv4x4s2(xt, weight)
    emit_backward(pl, pb, yt)
    x, w64, gy = rnd(g, N, H, W, cin_t), weight.detach().double(), rnd(g, N, 2 * H, 2 * W, cout_t)
    xg, wg = nchw(x).clone().requires_grad_(), w64.clone().requires_grad_()
    y_ref = F.conv_transpose2d(xg, wg, stride=2, padding=1)
    gx_ref, gw_ref = torch.autograd.grad(y_ref, (xg, wg), nchw(gy))
    wv = w64.view(cin_t, cout_t, 16)            # the weight of V = Conv2d(cout_t -> cin_t, 4, stride 2, padding 1)
    ds = descs(pl.fwd, "conv")
    assert len(ds) == 4 and all(q.ntaps == 4 and q.w_ntaps == 16 and q.out_stride == 2 and (q.x, q.y) == (xt.ptr(), yt.ptr()) for q in ds)
    assert [(q.out_off_y, q.out_off_x) for q in ds] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    y, seen = run_convs(ds, x, O.slots_bwd(wv))
    close(y, nhwc(y_ref.detach()))
    assert bool((seen == 1).all())
    (d,) = descs(pl.bwd, "conv")
    assert (d.ntaps, d.w_ntaps, d.in_stride, d.out_stride, d.x, d.y) == (16, 16, 2, 1, yt.gptr(), xt.gptr())
    gx, seen = run_convs([d], gy, O.slots_fwd(wv))
    close(gx, nhwc(gx_ref))
    assert bool((seen == 1).all())
    gs = descs(pl.bwd, "wgrad")
    assert [(q.ntaps, q.dw_tap_stride, q.dw_tap_off, q.in_stride) for q in gs] == [(4, 16, 4 * i, 2) for i in range(4)]
    assert all((q.x, q.dy) == (yt.gptr(), xt.ptr()) for q in gs)
    dw, seen = run_wgrads(gs, gy, x, (cin_t, cout_t, 16))
    close(dw, gw_ref.reshape(cin_t, cout_t, 16))
    assert bool((seen == 1).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_stem7x7_s2d_descriptors_and_index_maps(dtype):
    """The 7x7 stride-2 stem on the space-to-depth image (16 x 12 image): 16 taps over 12 channels, the weights gathered through the
    plan's own idx_w; the weight gradient in four groups with dw_tap_stride 16, brought back through idx_g, which inverts idx_w on every
    7x7 entry."""
    g = torch.Generator().manual_seed(6)
    N, cin, cout, H, W = 2, 3, 16, 16, 12
    weight = torch.nn.Parameter(torch.randn(cout, cin, 7, 7, generator=g))
    pl, pb = builder(dtype)
    xs = pl.new(N, H // 2, W // 2, 4 * cin, dtype, pitch=16)
    yt = pb.stem7x7_s2d(xs, weight)
    emit_backward(pl, pb, yt)
    maps = [t for t in pl.keep if t.dtype == torch.int32]
    idx_w = next(t for t in maps if tuple(t.shape) == (cout, 4 * cin, 16)).long()
    idx_g = next(t for t in maps if tuple(t.shape) == (cout, cin, 49)).long()
    img, w64 = rnd(g, N, cin, H, W), weight.detach().double()
    gy = rnd(g, N, H // 2, W // 2, cout)
    wg = w64.clone().requires_grad_()
    y_ref = F.conv2d(img, wg, stride=2, padding=3)
    (gw_ref,) = torch.autograd.grad(y_ref, wg, nchw(gy))
    # idx_w: the 4x4 weight over the 12 channels (what hrp_gather_f32 writes: src[idx] or, idx < 0, zero)
    w12 = torch.where(idx_w >= 0, w64.reshape(-1)[idx_w.clamp_min(0)], torch.zeros((), dtype=F64))
    assert int((idx_w >= 0).sum()) == cout * cin * 49 and len(set(idx_w[idx_w >= 0].tolist())) == cout * cin * 49
    assert torch.equal(idx_w.reshape(-1)[idx_g], torch.arange(cout * cin * 49).view(cout, cin, 49)), "idx_g inverts idx_w on every 7x7 entry"
    x = O.space_to_depth(img)
    (d,) = descs(pl.fwd, "conv")
    assert (d.ntaps, d.w_ntaps, d.in_stride, d.x, d.y) == (16, 16, 1, xs.ptr(), yt.ptr())
    y, seen = run_convs([d], x, O.slots_fwd(w12))
    close(y, nhwc(y_ref.detach()))
    assert bool((seen == 1).all())
    gs = descs(pl.bwd, "wgrad")
    assert [(q.ntaps, q.dw_tap_stride, q.dw_tap_off, q.in_stride, q.accumulate, q.reserved) for q in gs] == [(4, 16, 4 * i, 1, 0, 1) for i in range(4)]
    assert all((q.x, q.dy) == (xs.ptr(), yt.gptr()) for q in gs)
    dw12, seen = run_wgrads(gs, x, gy, (cout, 4 * cin, 16))
    assert bool((seen == 1).all())
    close(dw12.reshape(-1)[idx_g], gw_ref.reshape(cout, cin, 49))
    assert not descs(pl.bwd, "conv")        # (the image needs no gradient)


def test_fused_basic_block_data_and_weight_gradients():
    """conv -> BN -> ReLU -> conv on the row-strip kernels (train mode, bf16): the geometry of the two forward and the two data-gradient
    descriptors (g2, g1: mirrored taps on the transposed packing; their BatchNorm prologues are not evaluated here) and of the
    two weight gradients, on the raw operands."""
    g = torch.Generator().manual_seed(8)
    N, H, W, Cc = 1, 8, 64, 32
    c1, c2 = (torch.nn.Parameter(torch.randn(Cc, Cc, 3, 3, generator=g)) for _ in range(2))
    bn1 = torch.nn.BatchNorm2d(Cc).train()
    pl, pb = builder(torch.bfloat16)
    xt = pl.new(N, H, W, Cc)
    xt.requires_grad = True
    y2 = pb.conv_bn_relu_conv(xt, c1, bn1, c2)
    assert y2 is not None, "the row-strip form of this block (32 channels, 64 pixels per row, bf16, train mode)"
    emit_backward(pl, pb, y2)
    w1, w2 = c1.detach().double(), c2.detach().double()
    a, gy = rnd(g, N, H, W, Cc), rnd(g, N, H, W, Cc)
    d1, d2 = descs(pl.fwd, "conv")
    for d, w in ((d1, w1), (d2, w2)):
        y, seen = run_convs([d], a, O.slots_fwd(w.view(Cc, Cc, 9)))
        close(y, layer_reference(a, w, None, 1, 1)[0])
        assert bool((seen == 1).all())
    assert d1.x == xt.ptr() and d2.x == d1.y and d2.y == y2.ptr() and d2.pro_mode == 1
    g2, g1 = descs(pl.bwd, "conv")
    assert g2.x == y2.gptr() and g1.x == g2.y and g1.y == xt.gptr() and g1.pro_mode == 2 and not g1.res and not g2.res
    gws = descs(pl.bwd, "wgrad")
    assert len(gws) == 2 and [q.dy for q in gws] == [y2.gptr(), g1.pro_side] and gws[0].x == d2.pro_side and gws[1].x == xt.ptr()
    for d, q, w in ((g2, gws[0], w2), (g1, gws[1], w1)):
        _, gx_ref, gw_ref = layer_reference(a, w, gy, 1, 1)
        gx, seen = run_convs([d], gy, O.slots_bwd(w.view(Cc, Cc, 9)))
        close(gx, gx_ref)
        assert bool((seen == 1).all())
        dw, seen = run_wgrads([q], a, gy, (Cc, Cc, 9))
        close(dw, gw_ref.reshape(Cc, Cc, 9))
        assert bool((seen == 1).all())
