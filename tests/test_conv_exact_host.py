"""The float64 convolution oracle of the exact-arithmetic tests (tests/conv_exact_oracle.py) and the geometries the plans build from
(the package's conv_geometry module: taps, windows, parity classes, the stem's index maps) proved together against torch's own
convolutions in double on the CPU - no GPU - for every descriptor form, and the integer operand generators checked for the
preconditions the GPU tests (test_gpu_conv_exact.py) assert before a launch."""
import pytest
import torch
import torch.nn.functional as F

import conv_exact_oracle as O
from conv_exact_oracle import F64

import hrpe_amd  # noqa: F401
from hrpe_amd import conv_geometry as G


def nchw(t):
    return t.permute(0, 3, 1, 2)


def rnd(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F64)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("hw", [(9, 7), (8, 12), (1, 1)])
def test_oracle_3x3_forward(stride, hw):
    g = torch.Generator().manual_seed(1)
    H, W = hw
    x, w = rnd(g, 2, H, W, 5), rnd(g, 6, 5, 9)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    geo = G.forward(H, W, 3, stride)
    assert (geo.Ho, geo.Wo) == (Ho, Wo)
    r = O.evaluate(O.from_geometry(x, O.slots_fwd(w), geo))
    ref = F.conv2d(nchw(x), w.view(6, 5, 3, 3), stride=stride, padding=1)
    assert torch.allclose(nchw(r.y), ref, rtol=0, atol=1e-12)
    assert bool(r.written.all())


def test_oracle_1x1_stride2_and_dilation2():
    g = torch.Generator().manual_seed(2)
    x, w1, w3 = rnd(g, 2, 9, 12, 4), rnd(g, 3, 4, 1), rnd(g, 3, 4, 9)
    r = O.evaluate(O.from_geometry(x, O.slots_fwd(w1), G.forward(9, 12, 1, 2)))
    assert torch.allclose(nchw(r.y), F.conv2d(nchw(x), w1.view(3, 4, 1, 1), stride=2), rtol=0, atol=1e-12)
    r = O.evaluate(O.from_geometry(x, O.slots_fwd(w3), G.forward(9, 12, 3, 1, 2)))
    assert torch.allclose(nchw(r.y), F.conv2d(nchw(x), w3.view(3, 4, 3, 3), padding=2, dilation=2), rtol=0, atol=1e-12)


@pytest.mark.parametrize("dilation", [1, 2])
def test_oracle_stride1_data_gradient_is_the_mirrored_problem(dilation):
    g = torch.Generator().manual_seed(3)
    dy, w = rnd(g, 2, 7, 6, 4), rnd(g, 4, 5, 9)          # layer 5 -> 4
    r = O.evaluate(O.from_geometry(dy, O.slots_bwd(w), G.data_grad_s1(7, 6, 3, dilation)))
    ref = F.conv_transpose2d(nchw(dy), w.view(4, 5, 3, 3), padding=dilation, dilation=dilation)
    assert torch.allclose(nchw(r.y), ref, rtol=0, atol=1e-12)


@pytest.mark.parametrize("hw", [(8, 10), (9, 7)])
@pytest.mark.parametrize("padded", [False, True])
def test_oracle_stride2_data_gradient_by_parity_classes(hw, padded):
    """The four output-parity launches of a 3x3 stride-2 layer's data gradient (out_stride 2, 1 / 2 / 2 / 4 taps, or all padded to four
    taps with a zero tap slot) together write conv_transpose2d; each launch writes its own class only."""
    g = torch.Generator().manual_seed(4)
    H, W = hw
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy, w = rnd(g, 2, Ho, Wo, 4), rnd(g, 4, 3, 9)
    slots = O.slots_bwd(w, pad_t=1 if padded else 0)
    buf = torch.full((2, H, W, 3), 7.0, dtype=F64)
    seen = torch.zeros(2, H, W, 3, dtype=torch.int32)
    geos = G.data_grad_s2(H, W, 3, pad4=padded)
    assert [(q.cls, q.out_off_y, q.out_off_x, q.out_stride) for q in geos] == [(0, 0, 0, 2), (1, 0, 1, 2), (2, 1, 0, 2), (3, 1, 1, 2)]
    for q in geos:
        # a padding tap repeats the class's first offset and reads the zero slot 9
        real = [t for t in q.taps if t[2] < 9]
        assert real == G.class_taps(3, 1, q.out_off_y, q.out_off_x)
        assert q.taps[len(real):] == ([(real[0][0], real[0][1], 9)] * (4 - len(real)) if padded else [])
        r = O.evaluate(O.from_geometry(dy, slots, q, y_H=H, y_W=W), y0=buf)
        assert torch.equal(r.y[~r.written], buf[~r.written])
        buf, seen = r.y, seen + r.written.int()
    assert sorted(len([t for t in q.taps if t[2] < 9]) for q in geos) == [1, 2, 2, 4]
    assert bool((seen == 1).all())
    ref = F.conv_transpose2d(nchw(dy), w.view(4, 3, 3, 3), stride=2, padding=1, output_padding=(H - 1 - 2 * (Ho - 1), W - 1 - 2 * (Wo - 1)))
    assert torch.allclose(nchw(buf), ref, rtol=0, atol=1e-12)


def test_oracle_1x1_stride2_data_gradient_accumulates_on_even_pixels():
    g = torch.Generator().manual_seed(5)
    dy, w, prev = rnd(g, 2, 4, 5, 6), rnd(g, 6, 3, 1), rnd(g, 2, 8, 9, 3)
    assert [len(G.class_taps(1, 0, py, px)) for py in range(2) for px in range(2)] == [1, 0, 0, 0]
    (geo,) = G.data_grad_s2(8, 9, 1)             # the three classes without a tap are no problem
    assert geo.cls == 0
    r = O.evaluate(O.from_geometry(dy, O.slots_bwd(w), geo, y_H=8, y_W=9, res=prev), y0=prev)
    ref = prev + F.conv_transpose2d(nchw(dy), w.view(6, 3, 1, 1), stride=2, output_padding=(1, 0)).permute(0, 2, 3, 1)
    assert torch.allclose(r.y, ref, rtol=0, atol=1e-12)
    assert int(r.written.sum()) == 2 * 4 * 5 * 3


def test_oracle_space_to_depth_stem():
    g = torch.Generator().manual_seed(6)
    img, w7 = rnd(g, 2, 3, 16, 12), rnd(g, 5, 3, 7, 7)
    idx_w, idx_g = (torch.from_numpy(m).long() for m in G.stem_index_maps(5, 3))
    w12 = torch.where(idx_w >= 0, w7.reshape(-1)[idx_w.clamp_min(0)], torch.zeros((), dtype=F64))      # (hrp_gather_f32)
    r = O.evaluate(O.from_geometry(O.space_to_depth(img), O.slots_fwd(w12), G.stem_s2d(8, 6)))
    assert torch.allclose(nchw(r.y), F.conv2d(img, w7, stride=2, padding=3), rtol=0, atol=1e-12)
    assert torch.equal(idx_w.reshape(-1)[idx_g], torch.arange(5 * 3 * 49).view(5, 3, 49))      # idx_g inverts idx_w on every 7x7 entry


def test_oracle_epilogue_window_and_pitch():
    """bias, scale / shift, residual, ReLU in the descriptor's order; an out_off window accumulating onto y (the ASPP form) and
    pitch columns beyond Cout stay what they were."""
    g = torch.Generator().manual_seed(7)
    x, w = rnd(g, 1, 6, 6, 4), rnd(g, 3, 4, 9)
    b, sc, sh, res = rnd(g, 3), rnd(g, 3), rnd(g, 3), rnd(g, 1, 6, 6, 3)
    r = O.evaluate(O.from_geometry(x, O.slots_fwd(w), G.forward(6, 6, 3), bias=b, scale=sc, shift=sh, res=res, relu=True))
    conv = F.conv2d(nchw(x), w.view(3, 4, 3, 3), padding=1).permute(0, 2, 3, 1)
    assert torch.allclose(r.y, torch.relu((conv + b) * sc + sh + res), rtol=0, atol=1e-12)
    assert torch.allclose(r.stats, torch.cat([r.y.sum((0, 1, 2)), (r.y * r.y).sum((0, 1, 2))]))
    # one shifted tap of a rate-3 3x3 layer: tap (1, -1) of slot 6 on the rectangle whose source lies inside the image
    y0 = rnd(g, 1, 6, 6, 5)
    (geo,) = [q for q in G.shifted_taps(6, 6, 3) if q.taps[0][2] == 6]
    assert (geo.taps, geo.Ho, geo.Wo, geo.out_off_y, geo.out_off_x) == ([(0 + 3, 3 - 3, 6)], 3, 3, 0, 3)
    p = O.from_geometry(x, O.slots_fwd(w), geo, y_H=6, y_W=6, y_pitch=5, res=y0[..., :3])
    r = O.evaluate(p, y0=y0)
    want = y0.clone()
    want[:, 0:3, 3:6, :3] += torch.einsum("nyxc,oc->nyxo", x[:, 3:6, 0:3], w[:, :, 6])
    assert torch.allclose(r.y, want, rtol=0, atol=1e-12)
    assert int(r.written.sum()) == 27 and not bool(r.written[..., 3:].any())


ROW_SETS = [(32, (1, -1, 2, -2, 3, -3)), (64, (1, -1, 2, -2)), (128, (1, -1)), (256, (1, -1))]


@pytest.mark.parametrize("Cc,xvals", ROW_SETS)
def test_integer_operands_keep_the_row_strip_reference_representable(Cc, xvals):
    """The value sets the GPU tests draw from, on a row-strip shape: the exact result is a bf16 number everywhere and the per-channel
    sum of squares stays below 2^24."""
    g = torch.Generator().manual_seed(Cc)
    W = 2048 // Cc
    x, w = O.int_operands(g, 2, 8, W, Cc, Cc, 9, xvals=xvals)
    r = O.evaluate(O.from_geometry(x, O.slots_fwd(w), G.forward(8, W, 3)))
    assert bool((x != 0).all()) and bool((w != 0).all()) and bool((x == x.round()).all())
    O.assert_representable(r.y)
    O.assert_stats_exact(r.stats, Cc)


def test_cancelling_channel_pairs_bound_the_sum_and_still_see_a_misplaced_term():
    g = torch.Generator().manual_seed(9)
    x, w = O.int_operands(g, 2, 8, 64, 32, 32, 9, live=3)
    assert bool((x.abs() == 1).all()) and bool((w.abs() == 1).all())
    p = O.from_geometry(x, O.slots_fwd(w), G.forward(8, 64, 3))
    r = O.evaluate(p)
    assert float(r.y.abs().max()) <= 2 * 3 * 9 and float(r.y.abs().max()) > 0
    # an 8-channel slot swapped with its neighbour in ONE pixel changes the nine outputs around it
    x2 = x.clone()
    x2[0, 3, 5, 0:8], x2[0, 3, 5, 8:16] = x[0, 3, 5, 8:16], x[0, 3, 5, 0:8]
    r2 = O.evaluate(O.Problem(x2, p.w, p.taps, 8, 64))
    diff = (r2.y != r.y).any(-1)
    assert bool(diff[0, 2:5, 4:7].any()) and int(diff.sum()) <= 9
    with pytest.raises(AssertionError):
        O.assert_representable(torch.tensor([257.0], dtype=F64))


class _Ptr:
    """Stands in for a device tensor where only the address is looked at (the three queries are host-only)."""

    def __init__(self, p):
        self.p = p

    def data_ptr(self):
        return self.p


def test_tile_config_query_answers_the_case_table_without_a_gpu(monkeypatch):
    """hrp_conv_tile_config on the descriptors of test_gpu_conv_exact.TILE: the configuration each case claims to reach, 0 for a
    row-strip problem, a pointwise problem, an invalid problem and one that fits no configuration."""
    import ctypes as C

    import test_gpu_conv_exact as GT
    nv = GT.nvmod()
    L = nv.lib()
    g = torch.Generator().manual_seed(0)
    monkeypatch.setenv("HRP_PW_MIN_PIXELS", GT.NO_PW)
    seen = set()
    for name, c in GT.TILE.items():
        if c["N"] * c["H"] * c["W"] * c["cin"] > 1 << 20:       # (the big cases: shape only, no operands)
            P = O.from_geometry(torch.zeros(c["N"], c["H"], c["W"], c["cin"], dtype=F64), torch.zeros(9 if c["kind"] == "k3" else 1, c["cout"], c["cin"], dtype=F64),
                                G.forward(c["H"], c["W"], 3 if c["kind"] == "k3" else 1))
        else:
            P = GT.tile_problem(c, g)[0]
        d = GT.fill_desc(nv, nv.ConvDesc(), P, c["dt"], _Ptr(0x100000), _Ptr(0x200000), _Ptr(0x300000), GT.rup(c["cin"], 8 if c["dt"] == "bf16" else 4))
        if c.get("stats", True):
            d.stats = 0x400000
        if c.get("res") == "y":
            d.res = d.y
        elif c.get("res") == "misaligned":
            d.res, d.res_pitch = 0x500002, P.Cout
        assert GT.route(nv, d) == (0, 0, c["cfg"]), (name, GT.route(nv, d), L.hrp_last_error().decode())
        seen.add(c["cfg"] % 10000)
    assert seen == {2214, 2114, 1122, 1214, 1114}
    # a row-strip problem, a pointwise problem, an invalid problem, a problem no configuration fits
    x = torch.zeros(1, 8, 64, 32, dtype=F64)
    P = O.from_geometry(x, torch.zeros(9, 32, 32, dtype=F64), G.forward(8, 64, 3))
    d = GT.fill_desc(nv, nv.ConvDesc(), P, "bf16", _Ptr(0x100000), _Ptr(0x200000), _Ptr(0x300000), 32)
    assert GT.route(nv, d) == (32, 0, 0)
    d.x_pitch = 40                      # no longer dense rows: the tile program
    assert GT.route(nv, d) == (0, 0, 1114)
    d.x = 0x100008                      # misaligned input: hrp_conv2d_fwd refuses it
    assert GT.route(nv, d) == (0, 0, 0)
    P1 = O.from_geometry(x, torch.zeros(1, 64, 32, dtype=F64), G.forward(8, 64, 1))
    d1 = GT.fill_desc(nv, nv.ConvDesc(), P1, "bf16", _Ptr(0x100000), _Ptr(0x200000), _Ptr(0x300000), 32)
    assert GT.route(nv, d1) == (0, 0, 1122)
    monkeypatch.setenv("HRP_PW_MIN_PIXELS", "1")
    assert GT.route(nv, d1) == (0, 1, 0)
    far = O.from_geometry(torch.zeros(1, 64, 64, 32, dtype=F64), torch.zeros(9, 64, 32, dtype=F64), G.forward(64, 64, 3, 1, 40))
    df = GT.fill_desc(nv, nv.ConvDesc(), far, "bf16", _Ptr(0x100000), _Ptr(0x200000), _Ptr(0x300000), 32)
    assert GT.route(nv, df) == (0, 0, 0)     # taps 40 pixels apart: beyond every tile that fits LDS (plan.py runs such layers as one-tap problems)
    assert L.hrp_conv_tile_config(None) == 0
