"""Exact-arithmetic tests of the parity-fused data gradient of the 3x3 stride-2 layers (csrc/conv_parity.h) through the C ABI: the four
class descriptors of a layer, as the plans fill them (conv_geometry.data_grad_s2), go into one HRP_BATCH_CONV launch, which must run one
fused problem per layer.

Operands are +-1 (tests/conv_exact_oracle.py): every product and partial sum is a small integer, the float64 oracle - the four class
problems evaluated literally, one after the other - is exact, and the comparison is torch.equal on the whole buffer: dx lies between
guard rows and behind a channel pitch wider than C, both pre-filled with the sentinel 7.0.  A dx value is at most 4 taps x 48 channels
+ 3 (the residual) = 195 in magnitude, a bf16 integer; the oracle's result is checked for that before the launch.  With a residual
(res == y, as the plans accumulate) a pixel stored twice would carry it twice; the oracle counts that the four classes cover every
pixel once.

Shapes (dy N x H x W, dy channels -> dx channels): the smallest that can go wrong - N 2 and 3, 5 x 6 (a partial tile whose halo row and
column lie outside the image) and 8 x 8 (exactly one tile), 16 and 48 dy channels (one and three K chunks), 32 / 64 / 128 dx channels
(128: two or four channel blocks) - plus 20 x 18, where the halo of a tile is its neighbour's pixels.  Which tile configuration a case
runs is asserted from hrp_batch_conv_parity_configs; HRP_PARITY_MIN_WGS = 0 keeps the large tiles for these small launches.

Last, on random bf16 data the fused launch is bit-equal to the class launches (each class as a batch of its own, and as a single
launch): within a class the additions keep their order.

Measured on an MI355X: the 15 cases of the module, float64 oracles included, take 3.0 s together."""
import ctypes as C

import pytest
import torch

import conv_exact_oracle as O
from conv_exact_oracle import F64

import hrpe_amd  # noqa: F401
from hrpe_amd import conv_geometry as G
from test_gpu_conv_exact import SENTINEL, check_equal, ints, packn, upload
from test_gpu_rowconv import DEV, nvmod

pytestmark = pytest.mark.gpu
PARITY_VARIANT = 209
GUARD = 3          # guard rows (of 2 W pixels) in front of and behind dx

# name: (N, H, W, dy channels, dx channels, padded descriptors, residual, large tiles, expected configuration)
CASES = {
    "5x6-16-32-padded-res-1214": (2, 5, 6, 16, 32, True, True, True, 1214),
    "8x8-48-32-unpadded-1214": (2, 8, 8, 48, 32, False, False, True, 1214),
    "20x18-16-32-padded-res-1214": (2, 20, 18, 16, 32, True, True, True, 1214),
    "8x8-48-64-unpadded-2114": (3, 8, 8, 48, 64, False, False, True, 2114),
    "5x6-48-128-padded-res-2114": (3, 5, 6, 48, 128, True, True, True, 2114),
    "8x8-16-128-unpadded-res-1114": (2, 8, 8, 16, 128, False, True, False, 1114),
    "5x6-16-32-padded-1114": (3, 5, 6, 16, 32, True, False, False, 1114),
    "20x18-48-64-unpadded-res-1114": (3, 20, 18, 48, 64, False, True, False, 1114),
}


class Layer:
    """One layer's data gradient: operands on the device, the four class descriptors and the oracle's buffer."""

    def __init__(self, nv, g, N, H, W, cdy, cdx, padded, res):
        pad = 1 if padded else 0
        x, w = O.int_operands(g, N, H, W, cdy, cdx, 9)           # problem sense: x = dy, w [dx channels, dy channels, 9]
        slots = torch.cat([O.slots_fwd(w), torch.zeros(pad, cdx, cdy, dtype=F64)], 0)
        yH, yW, yp = 2 * H, 2 * W, cdx + 8
        geos = G.data_grad_s2(yH, yW, 3, pad4=padded)
        assert len(geos) == 4 and [len(q.taps) for q in geos] == ([4] * 4 if padded else [1, 2, 2, 4])
        y = torch.full((N, yH, yW, yp), SENTINEL, dtype=F64)
        if res:
            y[..., :cdx] = ints(g, (N, yH, yW, cdx), -3, 3)
        self.y0 = y.clone()
        seen = torch.zeros(y.shape, dtype=torch.int32)
        for geo in geos:          # the oracle: the class problems one after the other, each accumulating onto the buffer
            Pr = O.from_geometry(x, slots, geo, y_H=yH, y_W=yW, y_pitch=yp, res=y[..., :cdx].clone() if res else None)
            R = O.evaluate(Pr, y0=y)
            O.assert_representable(R.pre, "value before the residual")
            O.assert_representable(R.out, "reference")
            y, seen = R.y, seen + R.written.int()
        assert bool((seen[..., :cdx] == 1).all()) and bool((seen[..., cdx:] == 0).all()), "the classes write every pixel of dx once"
        self.want = y
        self.xd = upload(x, "bf16")
        self.wd = packn(nv, w, "bf16", transposed=True, pad_t=pad)
        self.rows = N * yH * yW
        self.buf = torch.full((self.rows + 2 * GUARD * yW, yp), SENTINEL, dtype=torch.bfloat16, device=DEV)
        self.buf[GUARD * yW:GUARD * yW + self.rows] = self.y0.reshape(-1, yp).to(torch.bfloat16).to(DEV)
        yptr = self.buf.data_ptr() + GUARD * yW * yp * 2
        src = G.Operand(self.xd.data_ptr(), N, H, W, cdy, cdy)
        dst = G.Operand(yptr, N, yH, yW, cdx, yp)
        self.descs = [G.fill_conv(geo, src, dst, nv.HRP_BF16, w=self.wd.data_ptr(), res=(yptr, yp) if res else None) for geo in geos]
        assert all(nv.lib().hrp_conv_parity_fusable(C.byref(d)) == 1 for d in self.descs)
        self.yW, self.shape = yW, (N, yH, yW, yp)

    def result(self):
        """-> (dx with its pitch columns, the guard rows)."""
        got = self.buf.double().cpu()
        lo, hi = GUARD * self.yW, GUARD * self.yW + self.rows
        return got[lo:hi].reshape(self.shape), torch.cat([got[:lo], got[hi:]])

    def check(self, what):
        got, guards = self.result()
        assert bool((guards == SENTINEL).all()), f"{what}: a guard row was written"
        check_equal(got, self.want, what)


def launch_batch(nv, descs):
    """One HRP_BATCH_CONV launch of `descs`.  -> (variant, configurations of the fused problems, block counts)."""
    n = len(descs)
    arr = (nv.ConvDesc * n)(*descs)
    info = nv.BatchInfo()
    host = (C.c_char * int(nv.lib().hrp_batch_table_bytes(nv.BATCH_CONV, n)))()
    nv.check(nv.lib().hrp_batch_prepare(nv.BATCH_CONV, arr, n, host, C.byref(info)), "prepare")
    cfgs = (C.c_int32 * nv.BATCH_MAX)()
    nq = nv.lib().hrp_batch_conv_parity_configs(host, C.byref(info), cfgs)
    table = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(DEV)
    nv.check(nv.lib().hrp_batch_launch(table.data_ptr(), C.byref(info), None), "launch")
    torch.cuda.synchronize()
    return info.variant, list(cfgs[:nq]), [info.blk0[i + 1] - info.blk0[i] for i in range(max(nq, 1))]


def tiles(monkeypatch, large):
    if large:
        monkeypatch.setenv("HRP_PARITY_MIN_WGS", "0")
    else:
        monkeypatch.delenv("HRP_PARITY_MIN_WGS", raising=False)


@pytest.mark.parametrize("name", list(CASES))
def test_parity_fused_exact(name, monkeypatch):
    nv = nvmod()
    N, H, W, cdy, cdx, padded, res, large, cfg = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    L = Layer(nv, g, N, H, W, cdy, cdx, padded, res)
    tiles(monkeypatch, large)
    order = torch.randperm(4, generator=g).tolist()
    variant, cfgs, _ = launch_batch(nv, [L.descs[i] for i in order])
    assert (variant, cfgs) == (PARITY_VARIANT, [cfg])
    L.check(name)


def test_cases_reach_every_configuration_and_variation():
    rows = list(CASES.values())
    assert {r[8] for r in rows} == {1214, 1114, 2114}
    assert {r[0] for r in rows} >= {2, 3} and {(r[1], r[2]) for r in rows} >= {(5, 6), (8, 8)}
    assert {r[3] for r in rows} >= {16, 48} and {r[4] for r in rows} >= {32, 64, 128}
    for cfg in (1214, 1114, 2114):          # padded and unpadded, with and without the residual: in every configuration
        assert {r[5] for r in rows if r[8] == cfg} == {True, False} and {r[6] for r in rows if r[8] == cfg} == {True, False}


@pytest.mark.parametrize("large", [True, False], ids=["large-tiles", "small-tiles"])
def test_three_layers_in_one_batch(large, monkeypatch):
    """Layers of different shapes, padded next to unpadded, with and without the residual, their twelve class problems in a scrambled
    order: one launch, three fused problems."""
    nv = nvmod()
    g = torch.Generator().manual_seed(31 + large)
    layers = [Layer(nv, g, 2, 5, 6, 16, 32, True, True), Layer(nv, g, 3, 8, 8, 48, 64, False, False), Layer(nv, g, 3, 5, 6, 48, 128, True, True)]
    descs = [d for L in layers for d in L.descs]
    order = torch.randperm(12, generator=g).tolist()
    tiles(monkeypatch, large)
    variant, cfgs, nblk = launch_batch(nv, [descs[i] for i in order])
    # heaviest K loop first (48 dy channels: the two later layers, in the order the scrambled list meets them), then the 16-channel layer
    assert variant == PARITY_VARIANT and cfgs == ([2114, 2114, 1214] if large else [1114] * 3)
    assert sorted(nblk[:2]) == ([2, 4] if large else [4, 8]) and nblk[2] == 1
    for i, L in enumerate(layers):
        L.check(f"layer {i}")


@pytest.mark.parametrize("padded", [True, False], ids=["padded", "unpadded"])
@pytest.mark.parametrize("shape", [(3, 20, 18, 128, 32), (2, 12, 16, 96, 64)], ids=["128-32", "96-64"])
def test_fused_equals_class_launches_on_random_data(shape, padded, monkeypatch):
    """Random bf16 operands and residual: the fused launch, the four classes as batches of their own (the ordinary batched kernel) and
    the four single launches give the same bits."""
    nv = nvmod()
    N, H, W, cdy, cdx = shape
    pad = 1 if padded else 0
    g = torch.Generator().manual_seed(cdy + pad)
    x = torch.randn(N, H, W, cdy, generator=g).to(torch.bfloat16).to(DEV)
    w = torch.randn(cdx, cdy, 9, generator=g, dtype=F64) * 0.1
    wd = packn(nv, w, "bf16", transposed=True, pad_t=pad)
    yH, yW = 2 * H, 2 * W
    r0 = torch.randn(N, yH, yW, cdx, generator=g).to(torch.bfloat16).to(DEV)
    y = r0.clone()
    src, dst = G.Operand(x.data_ptr(), N, H, W, cdy, cdy), G.Operand(y.data_ptr(), N, yH, yW, cdx, cdx)
    descs = [G.fill_conv(geo, src, dst, nv.HRP_BF16, w=wd.data_ptr(), res=(y.data_ptr(), cdx)) for geo in G.data_grad_s2(yH, yW, 3, pad4=padded)]
    outs = []
    for large in (True, False):
        tiles(monkeypatch, large)
        y.copy_(r0)
        variant, cfgs, _ = launch_batch(nv, descs)
        assert variant == PARITY_VARIANT and len(cfgs) == 1
        outs.append(y.clone())
    y.copy_(r0)
    for d in descs:
        variant, cfgs, _ = launch_batch(nv, [d])
        assert variant in (101, 102, 104, 1, 2, 4) and cfgs == []
    outs.append(y.clone())
    if padded:          # the four padded classes in one launch of the ordinary kernel: the plans' launch with the switch off
        y.copy_(r0)
        prev = nv.lib().hrp_conv_parity_fuse_enable(0)
        try:
            variant, cfgs, _ = launch_batch(nv, descs)
        finally:
            nv.lib().hrp_conv_parity_fuse_enable(prev)
        assert variant in (104, 4) and cfgs == []
        assert torch.equal(outs[0], y), "fused differs from the four padded classes in one ordinary launch"
    y.copy_(r0)
    for d in descs:
        nv.call("hrp_conv2d_fwd", C.byref(d), None)
    torch.cuda.synchronize()
    outs.append(y.clone())
    assert not torch.equal(outs[0], r0)
    for i, what in ((1, "small tiles"), (2, "class batches"), (3, "single launches")):
        assert torch.equal(outs[0], outs[i]), f"fused (large tiles) differs from {what}: {int((outs[0] != outs[i]).sum())} elements"
