"""Exact-arithmetic tests of the forward / data-gradient convolutions through the C ABI: the row-strip kernel (csrc/conv_row.h), the
general tile program (csrc/conv_tile.h) and the pointwise kernel (csrc/conv_pw.h), single launches and one HRP_BATCH_CONV launch.

Operands are small non-zero integers (tests/conv_exact_oracle.py), so every product is exact in bf16 MFMA, fp32 and the fp32x3 split,
every partial sum in any order is an integer below 2^24, the float64 oracle is exact and every comparison is torch.equal: y, the
pitch columns / pixels outside the written set (pre-filled with the sentinel 7.0), the statistic slots, the side outputs and ReLU
bits of the fused prologues.  A missing, doubled or misplaced term changes some output by at least 1.  Before a launch each test
asserts on the ORACLE's result alone that it is made of bf16 numbers and that the per-channel sums stay below 2^24.

Which program a case reaches is asserted through hrp_conv_rowstrip_channels / hrp_conv_pointwise / hrp_conv_tile_config:

  ROW_SHAPES (C, N, H), W = 2048 / C        rowstrip_channels == C, the other two 0; forms plain+stats / eval / res == y, forward and
                                            mirrored taps.  32: (1,8) (3,24) (32,64: spw 2); 64: (1,8) (5,8) (2,32); 128 / 256 whole-image
                                            (16x16 / 8x8, N = 1, 3) and strip form (128 @ H 8, 256 @ H 16)
  FUSED_SHAPES x pro1 / pro3 / pro2 / bnb   rowstrip_channels == C (prologues 1-3, epilogue reduce with recomputed mask and with bits)
  TILE (name: tile_config)                  rowstrip_channels == 0, pointwise == 0, tile_config as listed in TILE below: 2214, 2114, 1122,
                                            1214, 1114 for 9 taps and 1 tap in bf16; 1 / 2 / 4 / 9 / 16 taps in fp32 and fp32x3; 11122 =
                                            1122 with split-K
  test_gpu_pwconv.SHAPES                    pointwise == 1, tile_config == 0; then the same problem with the threshold raised:
                                            pointwise == 0, tile_config != 0, bit-equal again
  batched                                   one row-strip, one pointwise-shaped (runs the tile program in a batch) and one tile problem

Measured on an MI355X (wall time of the test call, float64 oracle included): the slowest case is the row-strip problem C = 32, N = 32,
H = 64 (131 072 pixels) accumulating onto y, 0.18 s; the tile cases with 65 536 pixels take 0.06 s; the whole module 4.5 s."""
import ctypes as C

import pytest
import torch

import conv_exact_oracle as O
from conv_exact_oracle import F64

import hrpe_amd  # noqa: F401
from hrpe_amd import conv_geometry as G
from test_gpu_pwconv import SHAPES as PW_SHAPES, desc1, pack1, small_problems_allowed  # noqa: F401  (autouse fixture: HRP_PW_MIN_PIXELS = 1)
from test_gpu_rowconv import DEV, SLOTS, desc, mask_bits, nhwc, nvmod, pack, rup

pytestmark = pytest.mark.gpu
SENTINEL = 7.0
NO_PW = str(2 ** 31 - 1)           # HRP_PW_MIN_PIXELS beyond every problem: 1x1 layers run the tile program


def tdtype(dt):
    return torch.bfloat16 if dt == "bf16" else torch.float32


def code(nv, dt):
    return {"bf16": nv.HRP_BF16, "f32": nv.HRP_F32, "f32x3": nv.HRP_F32X3}[dt]


def packn(nv, w, dt, transposed=False, pad_t=0):
    """Problem-sense weights w [Cout, Cin, taps] (float64 integers) -> the packed buffer the problem reads: the forward packing of w,
    or (transposed) the data-gradient packing of the LAYER weight w^T [Cin, Cout, taps] with pad_t extra zero tap slots."""
    src = (w.permute(1, 0, 2) if transposed else w).contiguous().float().to(DEV)
    cout, cin, nt = src.shape
    ck = 16 if dt == "bf16" else 8
    nf = -(-cin // ck) * nt * rup(cout, 32) * ck
    nb = -(-cout // ck) * (nt + pad_t) * rup(cin, 32) * ck
    dst = torch.zeros(nf, dtype=tdtype(dt), device=DEV)
    dst_t = torch.zeros(nb, dtype=tdtype(dt), device=DEV)
    tab = (nv.PackEntry * 1)()
    tab[0].src, tab[0].dst, tab[0].dst_t = src.data_ptr(), dst.data_ptr(), dst_t.data_ptr()
    tab[0].Cout, tab[0].Cin, tab[0].ntaps, tab[0].pad_t = cout, cin, nt, pad_t
    tdev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(DEV)
    nv.call("hrp_pack_weights", tdev.data_ptr(), 1, code(nv, dt), max(nf, nb), None)
    torch.cuda.synchronize()
    return dst_t if transposed else dst


def fill_desc(nv, d, P, dt, x, w, y, x_pitch):
    """The geometry, taps and element type of problem P into descriptor d (pointers: device tensors x, w, y), by the function the
    plans fill their descriptors with."""
    N, H, W, cin = P.x.shape
    geo = G.ConvGeometry(P.Ho, P.Wo, P.in_stride, P.out_stride, P.out_off[0], P.out_off[1], P.taps, P.w.shape[0])
    return G.fill_conv(geo, G.Operand(x.data_ptr(), N, H, W, cin, x_pitch), G.Operand(y.data_ptr(), N, P.y_H, P.y_W, P.Cout, P.y_pitch),
                       code(nv, dt), d=d, w=w.data_ptr())


def route(nv, d):
    L = nv.lib()
    return (L.hrp_conv_rowstrip_channels(C.byref(d)), L.hrp_conv_pointwise(C.byref(d)), L.hrp_conv_tile_config(C.byref(d)))


def check_equal(got, want, what):
    """torch.equal, with the first differing (n, y, x, c) and the count of differing elements when it fails."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    i = tuple(bad[0].tolist())
    msg = (f"{what}: {len(bad)} of {got.numel()} elements differ; first at (n, y, x, c) = {i}: got {got[i].item()}, "
           f"oracle {want[i].item()}")
    print(msg)
    raise AssertionError(msg)


def ints(g, shape, lo, hi):
    """Non-zero integers in [lo, hi] as float64."""
    vals = [v for v in range(lo, hi + 1) if v != 0]
    return O.pick(g, shape, vals)


def upload(t, dt, pitch=None):
    """float64 [N, H, W, C] -> device tensor of the element type with `pitch` channels per pixel (the padding holds the sentinel)."""
    if pitch is None or pitch == t.shape[-1]:
        return t.to(tdtype(dt)).contiguous().to(DEV)
    buf = torch.full((*t.shape[:-1], pitch), SENTINEL, dtype=F64)
    buf[..., :t.shape[-1]] = t
    return buf.to(tdtype(dt)).contiguous().to(DEV)


def run_exact(nv, P, dt, wd, expect, g, *, res=None, stats=True, x_pitch=None, acc=None, base=None, what=""):
    """One launch of problem P against the oracle.  res: None | "y" (accumulate onto y) | "other" | "misaligned" (a residual tensor at
    an address that is no multiple of 16 bytes).  expect: what the three queries must answer.  -> the oracle's Result."""
    N, H, W, cin = P.x.shape
    x_pitch = x_pitch or cin
    xd = upload(P.x, dt, x_pitch)
    wr = O.written(P)
    y0 = torch.full(wr.shape, SENTINEL, dtype=F64)
    keep = [xd]
    P.res = None
    if res == "y":
        y0[wr] = ints(g, wr.shape, -3, 3)[wr]
        P.res = y0[..., :P.Cout]
    elif res is not None:
        P.res = ints(g, (N, P.y_H, P.y_W, P.Cout), -3, 3)
        if P.scale is not None:
            P.res = P.res * P.scale.abs()        # (a channel scaled by 2 stays even: bf16 holds the even integers up to 512)
    R = O.evaluate(P, y0, acc=acc)
    # preconditions, on the oracle alone
    if dt == "bf16":
        O.assert_representable(R.pre, what + " value before the residual")
        O.assert_representable(R.out, what + " reference")
    else:
        assert float(R.out.abs().max()) < 2 ** 24 and float(R.pre.abs().max()) < 2 ** 24
    if stats:
        O.assert_stats_exact(R.stats, P.Cout)
    yd = y0.to(tdtype(dt)).contiguous().to(DEV)
    d = fill_desc(nv, base if base is not None else nv.ConvDesc(), P, dt, xd, wd, yd, x_pitch)
    if res == "y":
        d.res = yd.data_ptr()
    elif res is not None:
        rbuf = torch.full((P.res.numel() + 16,), SENTINEL, dtype=tdtype(dt), device=DEV)
        off = 1 if res == "misaligned" else 0
        rbuf[off:off + P.res.numel()] = P.res.reshape(-1).to(tdtype(dt)).to(DEV)
        d.res, d.res_pitch = rbuf.data_ptr() + off * rbuf.element_size(), P.Cout
        assert (d.res % 16 != 0) == (res == "misaligned")
        keep.append(rbuf)
    for name in ("bias", "scale", "shift"):
        v = getattr(P, name)
        if v is not None:
            t = v.float().to(DEV)
            keep.append(t)
            setattr(d, name, t.data_ptr())
    d.relu = 1 if P.relu else 0
    st = torch.zeros(SLOTS, 2 * P.Cout, dtype=torch.float64, device=DEV)
    d.stats = st.data_ptr() if stats else None
    assert route(nv, d) == expect, (what, route(nv, d), expect)
    nv.call("hrp_conv2d_fwd", C.byref(d), None)
    torch.cuda.synchronize()
    check_equal(yd.double().cpu(), R.y, what + " y")
    if stats:
        got = st.sum(0).cpu()
        assert torch.equal(got, R.stats), (what, "statistics", (got != R.stats).nonzero().flatten().tolist()[:8])
    return R


# ---- row-strip kernel ------------------------------------------------------------------------------------------------------------

ROW_SHAPES = [(32, 1, 8), (32, 3, 24), (32, 32, 64), (64, 1, 8), (64, 5, 8), (64, 2, 32), (128, 1, 16), (128, 3, 16), (256, 1, 8),
              (256, 3, 8), (128, 2, 8), (256, 1, 16)]       # (C, N, H); W = 2048 / C
ROW_XVALS = {32: (1, -1, 2, -2, 3, -3), 64: (1, -1, 2, -2), 128: (1, -1), 256: (1, -1)}
_row_cache = {}


def row_operands(shape, transposed):
    """Operands, packed weights and tap sum of a row-strip shape, computed once for its three forms."""
    key = (shape, transposed)
    if key not in _row_cache:
        nv = nvmod()
        Cc, N, H = shape
        W = 2048 // Cc
        g = torch.Generator().manual_seed(Cc * 1000 + N * 10 + transposed)
        # 131 072 pixels per channel: +-1 operands on three live channel pairs keep the sum of y^2 below 2^24 (<= 4 * 27 per pixel)
        big = N * H * W > 20000
        x, w = O.int_operands(g, N, H, W, Cc, Cc, 9, xvals=(1, -1) if big else ROW_XVALS[Cc], live=3 if big else None)
        if transposed:
            P = O.from_geometry(x, O.slots_fwd(w), G.data_grad_s1(H, W, 3))
            wd = pack(nv, w.permute(1, 0, 2).contiguous().view(Cc, Cc, 3, 3).float())[1]
        else:
            P = O.from_geometry(x, O.slots_fwd(w), G.forward(H, W, 3))
            wd = pack(nv, w.view(Cc, Cc, 3, 3).float())[0]
        _row_cache.clear()          # (one shape at a time: the largest tap sum is 34 MB)
        _row_cache[key] = (P, wd, O.accumulate(P))
    return _row_cache[key]


def eval_epilogue(g, P, Cc):
    """scale in {1, 2, -1}, integer shift, ReLU.  A channel scaled by 2 gets an even shift (and an even residual, run_exact): its
    values stay even, and bf16 holds the even integers up to 512 - the doubled sum of a 256-channel layer reaches 440."""
    P.scale = O.pick(g, (Cc,), (1, 2, -1))
    P.shift = ints(g, (Cc,), -2, 2) * P.scale.abs()
    P.relu = True


@pytest.mark.parametrize("transposed", [False, True], ids=["fwd", "mirrored"])
@pytest.mark.parametrize("form", ["plain_stats", "eval", "accumulate"])
@pytest.mark.parametrize("shape", ROW_SHAPES, ids=lambda s: "C%d-N%d-H%d" % s)
def test_rowstrip_exact(shape, form, transposed):
    nv = nvmod()
    Cc, N, H = shape
    P0, wd, acc = row_operands(shape, transposed)
    P = O.Problem(P0.x, P0.w, P0.taps, P0.Ho, P0.Wo)
    g = torch.Generator().manual_seed(Cc + N + H + len(form))
    base = desc(nv, torch.zeros(8, device=DEV), wd, torch.zeros(8, device=DEV), N, H, 2048 // Cc, Cc, transposed=transposed)
    res, stats = None, form == "plain_stats"
    if form == "eval":
        eval_epilogue(g, P, Cc)
        res = "other"
    elif form == "accumulate":
        res = "y"
    run_exact(nv, P, "bf16", wd, (Cc, 0, 0), g, res=res, stats=stats, acc=acc, base=base, what=f"row {shape} {form}")


def test_rowstrip_exact_permuted_tap_order():
    """The nine taps listed in another order, reading tap slots that hold the kernel positions in yet another order."""
    nv = nvmod()
    Cc, N, H, W = 64, 2, 16, 32
    g = torch.Generator().manual_seed(77)
    x, w = O.int_operands(g, N, H, W, Cc, Cc, 9, xvals=ROW_XVALS[Cc])
    sigma = torch.randperm(9, generator=g).tolist()            # slot s holds kernel position sigma[s]
    order = torch.randperm(9, generator=g).tolist()
    assert sigma != list(range(9)) and order != list(range(9))
    ws = w[:, :, sigma]
    taps = [(G.TAPS3[sigma[s]][0], G.TAPS3[sigma[s]][1], s) for s in order]
    P = O.Problem(x, O.slots_fwd(ws), taps, H, W)
    ref = O.evaluate(O.from_geometry(x, O.slots_fwd(w), G.forward(H, W, 3))).y
    assert torch.equal(O.evaluate(P).y, ref)                   # the same convolution, by the oracle
    wd = pack(nv, ws.contiguous().view(Cc, Cc, 3, 3).float())[0]
    run_exact(nv, P, "bf16", wd, (Cc, 0, 0), g, what="row permuted taps")


# ---- row-strip kernel: BatchNorm prologues and the reduce epilogue with exact constants ------------------------------------------

FUSED_SHAPES = [(32, 3, 24), (64, 5, 8), (128, 3, 16), (128, 2, 8), (256, 3, 8), (256, 1, 16)]
# Live channel pairs of the fused forms.  The staged operand x' is not centred (ReLU; the constant k0), so a channel's y has the mean
# 2 sum w E[x'] next to its spread: two pairs (forward, x' <= 8) and one (backward, |x'| <= 16) keep |y| below 256 and the sum of
# y^2 over 4 608 pixels below 2^24 with room to spare.
LIVE = 2
LIVE2 = 1


def paired(t):
    """[..., C / 2] -> [..., C]: both halves of the channel pairs (c, c + C / 2) hold the same values."""
    return torch.cat([t, t], -1)


def paired_weights(g, Cc, live):
    """[C, C, 9] of +-1: the pairs (c, c + C / 2) of INPUT channels cancel exactly for equal inputs, except `live` of them."""
    h = Cc // 2
    w0 = O.pick(g, (Cc, h, 9), (1, -1))
    keep = torch.zeros(h, dtype=F64)
    keep[torch.randperm(h, generator=g)[:live]] = 1
    return torch.cat([w0, w0 * (2 * keep - 1)[None, :, None]], 1)


def unit_stats(g, Cc, count):
    """Statistic slots with sum 0 and sum of squares `count` per channel, spread over the 8 slots in integers: mean 0, invstd
    rsqrt(1 + 0) = 1 with eps = 0."""
    cut = torch.sort(torch.randint(0, count + 1, (SLOTS - 1, Cc), generator=g), 0).values
    parts = torch.diff(torch.cat([torch.zeros(1, Cc, dtype=torch.int64), cut, torch.full((1, Cc), count)]), dim=0).double()
    s1 = ints(g, (SLOTS, Cc), -5, 5)
    s1[-1] -= s1.sum(0)
    assert bool((parts.sum(0) == count).all()) and bool((s1.sum(0) == 0).all())
    return torch.cat([s1, parts], 1).contiguous().to(DEV)


def sums_slots(g, total):
    """Per-channel totals [2C] (integers) spread over the 8 slots in integers."""
    r = ints(g, (SLOTS, total.numel()), -4, 4)
    r[-1] += total - r.sum(0)
    return r.contiguous().to(DEV)


def bits_of(pos_nhwc):
    return mask_bits(pos_nhwc.permute(0, 3, 1, 2))


def fused_setup(shape, seed):
    nv = nvmod()
    Cc, N, H = shape
    W = 2048 // Cc
    g = torch.Generator().manual_seed(seed * 7919 + Cc + N)
    return nv, Cc, N, H, W, g, float(N * H * W)


def fused_launch(nv, d, Cc):
    assert route(nv, d) == (Cc, 0, 0), route(nv, d)
    nv.call("hrp_conv2d_fwd", C.byref(d), None)
    torch.cuda.synchronize()


def bf16_dev(t):
    O.assert_representable(t, "operand")
    return nhwc(t.permute(0, 3, 1, 2).float()).view(t.shape)


@pytest.mark.parametrize("mode", [1, 3])
@pytest.mark.parametrize("shape", FUSED_SHAPES, ids=lambda s: "C%d-N%d-H%d" % s)
def test_rowstrip_exact_forward_prologues(shape, mode):
    """pro_mode 1: conv(relu(gamma x + beta)); pro_mode 3: conv(relu(gamma x + beta + x2)) with the ReLU bits as an output.  gamma a
    power of two, beta an integer, mean 0 and invstd 1 from the slots: the activation is an exact integer."""
    nv, Cc, N, H, W, g, cnt = fused_setup(shape, mode)
    h = Cc // 2
    x = paired(ints(g, (N, H, W, h), -2, 2))
    gamma, beta = paired(O.pick(g, (h,), (1, 2, -1))), paired(ints(g, (h,), -2, 2))
    x2 = paired(ints(g, (N, H, W, h), -2, 2)) if mode == 3 else None
    a = x * gamma + beta + (x2 if mode == 3 else 0)
    a = a.clamp_min(0)
    w = paired_weights(g, Cc, LIVE)
    P = O.from_geometry(a, O.slots_fwd(w), G.forward(H, W, 3))
    R = O.evaluate(P, torch.full((N, H, W, Cc), SENTINEL, dtype=F64))
    O.assert_representable(R.out)
    O.assert_stats_exact(R.stats, Cc)
    xd, wd = bf16_dev(x), pack(nv, w.view(Cc, Cc, 3, 3).float())[0]
    y = torch.full((N, H, W, Cc), SENTINEL, dtype=torch.bfloat16, device=DEV)
    side = torch.full((N, H, W, Cc), SENTINEL, dtype=torch.bfloat16, device=DEV)
    mask = torch.full((N * H * W * Cc // 8,), 0xAA, dtype=torch.uint8, device=DEV)
    st_in, st = unit_stats(g, Cc, int(cnt)), torch.zeros(SLOTS, 2 * Cc, dtype=torch.float64, device=DEV)
    gd, bd = gamma.float().to(DEV), beta.float().to(DEV)
    d = desc(nv, xd, wd, y, N, H, W, Cc)
    d.stats = st.data_ptr()
    d.pro_mode, d.pro_stats, d.pro_gamma, d.pro_beta = mode, st_in.data_ptr(), gd.data_ptr(), bd.data_ptr()
    d.pro_count, d.pro_eps, d.pro_side = cnt, 0.0, side.data_ptr()
    if mode == 3:
        x2d = bf16_dev(x2)
        d.pro_x2, d.pro_mask = x2d.data_ptr(), mask.data_ptr()
    fused_launch(nv, d, Cc)
    check_equal(side.double().cpu(), a, "side output == the integer activation (else the constants are not exact on the device)")
    if mode == 3:
        assert torch.equal(mask.cpu(), bits_of(a > 0).cpu()), "ReLU bits of pro_mask"
    check_equal(y.double().cpu(), R.y, "y")
    assert torch.equal(st.sum(0).cpu(), R.stats)


@pytest.mark.parametrize("bits", [False, True], ids=["recomputed", "bits"])
@pytest.mark.parametrize("shape", FUSED_SHAPES, ids=lambda s: "C%d-N%d-H%d" % s)
def test_rowstrip_exact_backward_prologue(shape, bits):
    """pro_mode 2 on the mirrored taps: x' = gamma (g - k0 - x2 k1), g = x masked by [gamma2 x2 + beta2 > 0] (recomputed) or by a bit
    mask; k0, k1 = +-1, +-2 from pro_bsums; side output x', second side output g; accumulated onto y (res == y)."""
    nv, Cc, N, H, W, g, cnt = fused_setup(shape, 20 + bits)
    h = Cc // 2
    x, x2 = paired(ints(g, (N, H, W, h), -2, 2)), paired(ints(g, (N, H, W, h), -2, 2))
    gamma, beta = paired(O.pick(g, (h,), (1, 2))), paired(ints(g, (h,), -2, 2))
    k0, k1 = paired(O.pick(g, (h,), (1, -1, 2))), paired(O.pick(g, (h,), (1, -1, -2)))
    on = paired(torch.rand(N, H, W, h, generator=g) > 0.45) if bits else (x2 * gamma + beta > 0)
    gm = x * on
    a = gamma * (gm - k0 - x2 * k1)
    w = paired_weights(g, Cc, LIVE2)
    P = O.from_geometry(a, O.slots_fwd(w), G.data_grad_s1(H, W, 3))
    prev = ints(g, (N, H, W, Cc), -3, 3)
    P.res = prev
    R = O.evaluate(P, prev)
    O.assert_representable(R.out)
    xd, x2d = bf16_dev(x), bf16_dev(x2)
    wd = pack(nv, w.permute(1, 0, 2).contiguous().view(Cc, Cc, 3, 3).float())[1]
    y = bf16_dev(prev)
    side = torch.full((N, H, W, Cc), SENTINEL, dtype=torch.bfloat16, device=DEV)
    side2 = torch.full((N, H, W, Cc), 5.0, dtype=torch.bfloat16, device=DEV)
    st_in, bs_in = unit_stats(g, Cc, int(cnt)), sums_slots(g, torch.cat([k0, k1]) * cnt)
    gd, bd = gamma.float().to(DEV), beta.float().to(DEV)
    d = desc(nv, xd, wd, y, N, H, W, Cc, transposed=True)
    d.res = y.data_ptr()
    d.pro_mode, d.pro_x2, d.pro_stats, d.pro_bsums = 2, x2d.data_ptr(), st_in.data_ptr(), bs_in.data_ptr()
    d.pro_gamma, d.pro_beta, d.pro_count, d.pro_eps, d.pro_side = gd.data_ptr(), bd.data_ptr(), cnt, 0.0, side.data_ptr()
    if bits:
        mk = bits_of(on)
        d.pro_mask, d.pro_side2, d.pro_side2_acc = mk.data_ptr(), side2.data_ptr(), 0
    fused_launch(nv, d, Cc)
    check_equal(side.double().cpu(), a, "side output == the integer BatchNorm input gradient (else the constants are not exact on the device)")
    if bits:
        check_equal(side2.double().cpu(), gm, "second side output == the masked gradient")
    check_equal(y.double().cpu(), R.y, "y")


@pytest.mark.parametrize("bits", [False, True], ids=["recomputed", "bits"])
@pytest.mark.parametrize("shape", FUSED_SHAPES, ids=lambda s: "C%d-N%d-H%d" % s)
def test_rowstrip_exact_reduce_epilogue(shape, bits):
    """bnb_x epilogue of a data gradient: stats = sum g, sum g xhat with g = the stored y masked by [gamma b + beta > 0] (recomputed from
    the BatchNorm input b) or by a bit mask, xhat = b (mean 0, invstd 1)."""
    nv, Cc, N, H, W, g, cnt = fused_setup(shape, 30 + bits)
    x, w = O.int_operands(g, N, H, W, Cc, Cc, 9, xvals=ROW_XVALS[Cc])
    P = O.from_geometry(x, O.slots_fwd(w), G.data_grad_s1(H, W, 3))
    R = O.evaluate(P, torch.full((N, H, W, Cc), SENTINEL, dtype=F64))
    O.assert_representable(R.out)
    b = ints(g, (N, H, W, Cc), -2, 2)
    gamma, beta = O.pick(g, (Cc,), (1, 2, -1)), ints(g, (Cc,), -2, 2)
    on = (torch.rand(N, H, W, Cc, generator=g) > 0.4) if bits else (b * gamma + beta > 0)
    gm = R.out * on
    want = torch.cat([gm.sum((0, 1, 2)), (gm * b).sum((0, 1, 2))])
    assert float(torch.cat([gm.abs().sum((0, 1, 2)), (gm * b).abs().sum((0, 1, 2))]).max()) < 2 ** 24, "the test's inputs are wrong"
    xd, bd_x = bf16_dev(x), bf16_dev(b)
    wd = pack(nv, w.permute(1, 0, 2).contiguous().view(Cc, Cc, 3, 3).float())[1]
    y = torch.full((N, H, W, Cc), SENTINEL, dtype=torch.bfloat16, device=DEV)
    st_in, bs = unit_stats(g, Cc, int(cnt)), torch.zeros(SLOTS, 2 * Cc, dtype=torch.float64, device=DEV)
    gd, bd = gamma.float().to(DEV), beta.float().to(DEV)
    d = desc(nv, xd, wd, y, N, H, W, Cc, transposed=True)
    d.stats, d.bnb_x, d.bnb_x_pitch = bs.data_ptr(), bd_x.data_ptr(), Cc
    d.bnb_stats, d.bnb_gamma, d.bnb_beta, d.bnb_count, d.bnb_eps = st_in.data_ptr(), gd.data_ptr(), bd.data_ptr(), cnt, 0.0
    if bits:
        mk = bits_of(on)
        d.bnb_mask, d.bnb_mask_pitch = mk.data_ptr(), Cc // 8
    fused_launch(nv, d, Cc)
    check_equal(y.double().cpu(), R.y, "y")
    got = bs.sum(0).cpu()
    assert torch.equal(got, want), ("sum g, sum g xhat", (got != want).nonzero().flatten().tolist()[:8])


# ---- general tile program --------------------------------------------------------------------------------------------------------

def T(dt, kind, N, H, W, cin, cout, cfg, **kw):
    return dict(dt=dt, kind=kind, N=N, H=H, W=W, cin=cin, cout=cout, cfg=cfg, **kw)


# name -> case; cfg = the hrp_conv_tile_config the case must reach.  The large tiles need pixels / 256 * ceil(Cout / 64) >= 256.
TILE = {
    # every configuration, 9 taps and 1 tap, bf16
    "k3-2214": T("bf16", "k3", 16, 64, 64, 32, 64, 2214, stats=False),
    "k3-2214-wide": T("bf16", "k3", 4, 64, 64, 32, 256, 2214),
    "k3-2114": T("bf16", "k3", 8, 64, 64, 32, 64, 2114),
    "k3-1122": T("bf16", "k3", 2, 16, 16, 32, 64, 1122),
    "k3-1214": T("bf16", "k3", 16, 128, 32, 32, 32, 1214, stats=False),
    "k3-1114": T("bf16", "k3", 2, 16, 16, 32, 32, 1114),
    "k1-2214": T("bf16", "k1", 16, 64, 64, 32, 64, 2214),
    "k1-2114": T("bf16", "k1", 8, 64, 64, 32, 64, 2114),
    "k1-1122": T("bf16", "k1", 2, 16, 16, 32, 64, 1122),
    "k1-1214": T("bf16", "k1", 16, 64, 64, 32, 32, 1214),
    "k1-1114": T("bf16", "k1", 2, 16, 16, 32, 32, 1114),
    # the other tap counts and descriptor forms
    "stem-16taps-cin8": T("bf16", "stem", 2, 24, 20, 8, 64, 1122),
    "k3-in-stride2": T("bf16", "k3s2", 2, 17, 22, 32, 64, 1122),
    "k3-dilation2": T("bf16", "dil2", 2, 16, 20, 32, 64, 1122),
    "par00-1tap": T("bf16", "par", 2, 9, 12, 64, 32, 1114, cls=(0, 0)),
    "par01-2taps": T("bf16", "par", 2, 9, 12, 64, 32, 1114, cls=(0, 1)),
    "par10-2taps": T("bf16", "par", 2, 9, 12, 64, 32, 1114, cls=(1, 0)),
    "par11-4taps": T("bf16", "par", 2, 9, 12, 64, 32, 1114, cls=(1, 1)),
    "par00-padded": T("bf16", "par", 2, 9, 12, 64, 32, 1114, cls=(0, 0), padded=True),
    "par01-padded": T("bf16", "par", 2, 9, 12, 64, 32, 1114, cls=(0, 1), padded=True),
    "par10-padded": T("bf16", "par", 2, 9, 12, 64, 32, 1114, cls=(1, 0), padded=True),
    "par11-padded-odd": T("bf16", "par", 2, 9, 12, 64, 32, 1114, cls=(1, 1), padded=True, odd=True),
    "k1-stride2-even-pixels": T("bf16", "k1s2bwd", 2, 8, 10, 64, 32, 1114, res="y"),
    "aspp-one-tap-window": T("bf16", "aspp", 1, 20, 24, 32, 64, 1122, res="y", y_pitch=72),
    # ragged edges
    "ragged-13x9": T("bf16", "k3", 3, 13, 9, 32, 64, 1122),
    "image-1x1": T("bf16", "k3", 5, 1, 1, 32, 64, 1122),
    "cin40": T("bf16", "k3", 2, 10, 12, 40, 64, 1122),
    "cout17": T("bf16", "k3", 2, 10, 12, 32, 17, 1114, y_pitch=24),
    "cout448": T("bf16", "k3", 1, 12, 12, 32, 448, 1122),
    "scalar-stores": T("bf16", "k3", 2, 10, 12, 32, 40, 1122, y_pitch=48, res="misaligned", relu=True),
    "bias": T("bf16", "k3", 2, 10, 12, 32, 64, 1122, bias=True, eval=True, res="other"),
    # one shape per tap count in fp32 and fp32x3 (fp32 outputs: no representability condition)
    **{f"{dt}-{name}": T(dt, kind, *shape, **kw) for dt in ("f32", "f32x3") for name, kind, shape, kw in [
        ("k1", "k1", (2, 12, 10, 32, 64, 1122), {}), ("2taps", "par", (2, 9, 12, 64, 32, 1114), dict(cls=(0, 1))),
        ("4taps", "par", (2, 9, 12, 64, 32, 1114), dict(cls=(1, 1))), ("k3", "k3", (2, 12, 10, 32, 64, 1122), dict(res="other", relu=True)),
        ("16taps", "stem", (2, 12, 10, 12, 64, 1122), {})]},
    "f32-split-k": T("f32", "k1", 64, 1, 1, 2056, 1024, 11122, stats=False, xvals=(1, -1, 2, -2)),
}


def tile_problem(c, g):
    """-> (Problem, transposed packing?, pad_t, problem-sense weights [Cout, Cin, taps])."""
    N, H, W, cin, cout, kind = c["N"], c["H"], c["W"], c["cin"], c["cout"], c["kind"]
    nt = {"k3": 9, "k3s2": 9, "dil2": 9, "k1": 1, "stem": 16, "par": 9, "k1s2bwd": 1, "aspp": 9}[kind]
    x, w = O.int_operands(g, N, H, W, cin, cout, nt, xvals=c.get("xvals", (1, -1)), live=c.get("live"))
    yp = c.get("y_pitch", 0)
    if kind in ("k3", "dil2", "k1"):
        return O.from_geometry(x, O.slots_fwd(w), G.forward(H, W, 3 if nt == 9 else 1, 1, 2 if kind == "dil2" else 1), y_pitch=yp), False, 0, w
    if kind == "k3s2":
        geo = G.forward(H, W, 3, 2)
        assert (geo.Ho, geo.Wo, geo.in_stride) == ((H - 1) // 2 + 1, (W - 1) // 2 + 1, 2)
        return O.from_geometry(x, O.slots_fwd(w), geo, y_pitch=yp), False, 0, w
    if kind == "stem":
        return O.from_geometry(x, O.slots_fwd(w), G.stem_s2d(H, W), y_pitch=yp), False, 0, w
    if kind == "par":       # x = the output gradient of a 3x3 stride-2 layer, y = the gradient of its (2H or 2H - 1) x (2W or 2W - 1) input
        (py, px), pad = c["cls"], 1 if c.get("padded") else 0
        yH, yW = 2 * H - (1 if c.get("odd") else 0), 2 * W - (1 if c.get("odd") else 0)
        (geo,) = [q for q in G.data_grad_s2(yH, yW, 3, pad4=bool(pad)) if q.cls == 2 * py + px]
        assert (geo.Ho, geo.Wo, geo.out_stride, geo.out_off_y, geo.out_off_x) == ((yH - py + 1) // 2, (yW - px + 1) // 2, 2, py, px)
        assert (geo.Ho, geo.Wo) in ((H, W), (H - 1, W), (H, W - 1), (H - 1, W - 1)) and len(geo.taps) == (4 if pad else (1 + py) * (1 + px))
        slots = torch.cat([O.slots_fwd(w), torch.zeros(pad, cout, cin, dtype=F64)], 0)
        return O.from_geometry(x, slots, geo, y_H=yH, y_W=yW, y_pitch=yp), True, pad, w
    if kind == "k1s2bwd":
        (geo,) = G.data_grad_s2(2 * H, 2 * W - 1, 1)
        assert (geo.Ho, geo.Wo, geo.out_stride, geo.cls) == (H, W, 2, 0)
        return O.from_geometry(x, O.slots_fwd(w), geo, y_H=2 * H, y_W=2 * W - 1, y_pitch=yp), True, 0, w
    if kind == "aspp":      # tap (a, b) = (1, -1) of a rate-6 3x3 layer on the rectangle whose source pixels exist, onto the centre tap's sum
        (geo,) = [q for q in G.shifted_taps(H, W, 6) if q.taps[0][2] == 6]
        assert (geo.taps, geo.Ho, geo.Wo, geo.out_off_y, geo.out_off_x) == ([(6, 0, 6)], H - 6, W - 6, 0, 6)
        return O.from_geometry(x, O.slots_fwd(w), geo, y_H=H, y_W=W, y_pitch=yp), False, 0, w
    raise ValueError(kind)


@pytest.mark.parametrize("name", list(TILE))
def test_tile_program_exact(name, monkeypatch):
    monkeypatch.setenv("HRP_PW_MIN_PIXELS", NO_PW)
    nv = nvmod()
    c = TILE[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    P, transposed, pad_t, w = tile_problem(c, g)
    if c.get("bias"):
        P.bias = ints(g, (P.Cout,), -3, 3)
    if c.get("eval"):
        eval_epilogue(g, P, P.Cout)
    P.relu = P.relu or bool(c.get("relu"))
    wd = packn(nv, w, c["dt"], transposed, pad_t)
    x_pitch = rup(c["cin"], 8 if c["dt"] == "bf16" else 4)
    run_exact(nv, P, c["dt"], wd, (0, 0, c["cfg"]), g, res=c.get("res"), stats=c.get("stats", True), x_pitch=x_pitch, what=name)


def test_tile_cases_reach_every_configuration_and_tap_count():
    """The table above holds what the issue asks for (the launches themselves assert that each case reaches its `cfg`)."""
    for kind in ("k3", "k1"):
        assert {c["cfg"] for c in TILE.values() if c["kind"] == kind and c["dt"] == "bf16"} >= {2214, 2114, 1122, 1214, 1114}
    g = torch.Generator().manual_seed(0)
    for dt in ("bf16", "f32", "f32x3"):
        assert {len(tile_problem(c, g)[0].taps) for n, c in TILE.items() if c["dt"] == dt and c["N"] * c["H"] * c["W"] < 4096} >= {1, 2, 4, 9, 16}


# ---- pointwise kernel ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["plain_stats", "eval", "accumulate"])
@pytest.mark.parametrize("shape", PW_SHAPES, ids=lambda s: "%d-%d-N%d-%dx%d" % s)
def test_pointwise_exact(shape, form, monkeypatch):
    """The pointwise kernel and, with the threshold raised, the tile program on the same problem: both bit-equal to the oracle."""
    nv = nvmod()
    cin, cout, N, H, W = shape
    g = torch.Generator().manual_seed(cin * 3 + cout + len(form))
    x, w = O.int_operands(g, N, H, W, cin, cout, 1, xvals=(1, -1, 2, -2) if cin <= 64 else (1, -1))
    wd = pack1(nv, w.view(cout, cin, 1, 1).float())[0]
    for pw in (1, 0):
        if not pw:
            monkeypatch.setenv("HRP_PW_MIN_PIXELS", NO_PW)
        P = O.from_geometry(x, O.slots_fwd(w), G.forward(H, W, 1))
        g2 = torch.Generator().manual_seed(cin + cout)
        res = None
        if form == "eval":
            eval_epilogue(g2, P, cout)
            res = "other"
        elif form == "accumulate":
            res = "y"
        base = desc1(nv, torch.zeros(8, device=DEV), wd, torch.zeros(8, device=DEV), N, H, W, cin, cout)
        d_expect = (0, 1, 0) if pw else None
        if pw:
            run_exact(nv, P, "bf16", wd, d_expect, g2, res=res, stats=form == "plain_stats", base=base, what=f"pointwise {shape} {form}")
        else:
            cfg = tile_config_of(nv, P, wd)
            assert cfg != 0
            run_exact(nv, P, "bf16", wd, (0, 0, cfg), g2, res=res, stats=form == "plain_stats", base=base, what=f"tile program {shape} {form}")


def tile_config_of(nv, P, wd):
    N, H, W, cin = P.x.shape
    t = torch.zeros(8, device=DEV)
    d = fill_desc(nv, nv.ConvDesc(), P, "bf16", t, wd, t, cin)
    return nv.lib().hrp_conv_tile_config(C.byref(d))


# ---- one batched launch ----------------------------------------------------------------------------------------------------------

def test_batched_launch_exact():
    """A row-strip problem, a pointwise-shaped problem (which a batch runs on the tile program) and a ragged tile problem, all 3x3 or
    all 1x1 being a batch's rule: here three 9-tap problems plus, in a second launch, two 1-tap ones.  Each bit-equal to the oracle."""
    nv = nvmod()
    g = torch.Generator().manual_seed(123)
    for group in ([("row", 32, 32, 3, 24, 64), ("tile", 32, 64, 3, 13, 9), ("row", 256, 256, 3, 8, 8), ("tile", 32, 17, 2, 10, 12)],
                  [("pw", 64, 256, 2, 16, 16), ("tile1", 32, 40, 2, 12, 10)]):
        descs, checks, keep = [], [], []
        for kind, cin, cout, N, H, W in group:
            nt = 9 if kind in ("row", "tile") else 1
            x, w = O.int_operands(g, N, H, W, cin, cout, nt, xvals=(1, -1))
            P = O.from_geometry(x, O.slots_fwd(w), G.forward(H, W, 3 if nt == 9 else 1), y_pitch=rup(cout, 8))
            y0 = torch.full((N, H, W, P.y_pitch), SENTINEL, dtype=F64)
            R = O.evaluate(P, y0)
            O.assert_representable(R.out)
            O.assert_stats_exact(R.stats, cout)
            xd, yd, wd = upload(x, "bf16", rup(cin, 8)), y0.to(torch.bfloat16).to(DEV), packn(nv, w, "bf16")
            st = torch.zeros(SLOTS, 2 * cout, dtype=torch.float64, device=DEV)
            d = fill_desc(nv, nv.ConvDesc(), P, "bf16", xd, wd, yd, rup(cin, 8))
            d.stats = st.data_ptr()
            r = route(nv, d)
            assert (r[0] != 0, r[1] != 0, r[2] != 0) == {"row": (True, False, False), "pw": (False, True, False)}.get(kind, (False, False, True)), (kind, r)
            descs.append(d)
            checks.append((kind, yd, st, R))
            keep += [xd, wd]
        n = len(descs)
        arr = (nv.ConvDesc * n)(*descs)
        info = nv.BatchInfo()
        nb = int(nv.lib().hrp_batch_table_bytes(nv.BATCH_CONV, n))
        host = (C.c_char * nb)()
        nv.check(nv.lib().hrp_batch_prepare(nv.BATCH_CONV, arr, n, host, C.byref(info)), "prepare")
        table = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(DEV)
        nv.check(nv.lib().hrp_batch_launch(table.data_ptr(), C.byref(info), None), "launch")
        torch.cuda.synchronize()
        for kind, yd, st, R in checks:
            check_equal(yd.double().cpu(), R.y, f"batched {kind} y")
            assert torch.equal(st.sum(0).cpu(), R.stats), kind
