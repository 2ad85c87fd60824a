"""Geometry of every convolution and weight-gradient problem the plans build, and the two functions that fill a descriptor from one.

A convolution problem (hrp_conv_desc, include/hrp.h) computes, on a logical Ho x Wo grid,
    y[n, oy * out_stride + out_off_y, ox * out_stride + out_off_x, :] = sum_i W[wtap[i]] . x[n, oy * in_stride + dy[i], ox * in_stride + dx[i], :]
with zero outside the image; a weight-gradient problem (hrp_wgrad_desc) sums dy[n, oy, ox, co] x[n, oy * in_stride + dy_t[t], ox *
in_stride + dx_t[t], ci] into dW[co][ci][t].  Everything above fill_conv is plain Python: no tensors, no plan, no device.
tests/test_plan_conv_desc_host.py proves the descriptors the real builder fills from it against torch in float64."""
from collections import namedtuple

import numpy as np

from . import _native as nv

TAPS3 = [(ky - 1, kx - 1) for ky in range(3) for kx in range(3)]
TAPS4_DECONV = [(ky - 1, kx - 1) for ky in range(4) for kx in range(4)]    # V = Conv2d(4, stride 2, padding 1): iy = 2 oy + ky - 1
TAPS4_STEM = [(ty - 2, tx - 2) for ty in range(4) for tx in range(4)]      # the 7x7 stride-2 stem on the space-to-depth image
# hrp_dtype code -> (bytes per element, elements per 16-byte vector: the channel granularity of a problem's Cin)
ELEM = {nv.HRP_BF16: (2, 8), nv.HRP_F32: (4, 4), nv.HRP_F32X3: (4, 4)}

# one side of a problem: device address and the NHWC shape / channel pitch behind it (a forward tensor or a gradient buffer)
Operand = namedtuple("Operand", "ptr N H W C pitch")
# taps: [(dy, dx, wtap)]; w_ntaps: tap slots per chunk of the packing read; cls: index of the output-parity class (0 .. 3) or None
ConvGeometry = namedtuple("ConvGeometry", "Ho Wo in_stride out_stride out_off_y out_off_x taps w_ntaps cls", defaults=(None,))
# taps: [(dy, dx)], forward sense; dw_tap_stride / dw_tap_off: the launch is a tap group of a larger kernel (0, 0: the whole kernel)
WgradGeometry = namedtuple("WgradGeometry", "in_stride taps dw_tap_stride dw_tap_off", defaults=(0, 0))


def rup(a, b):
    return (a + b - 1) // b * b


def _offsets(ksize, dilation=1):
    assert ksize in (1, 3)
    return [(a * dilation, b * dilation) for a, b in TAPS3] if ksize == 3 else [(0, 0)]


def _whole(Ho, Wo, in_stride, offsets):
    return ConvGeometry(Ho, Wo, in_stride, 1, 0, 0, [(a, b, i) for i, (a, b) in enumerate(offsets)], len(offsets))


def forward(H, W, ksize, stride=1, dilation=1):
    """Conv2d(k, stride, padding = dilation * (k // 2), dilation) on an H x W input, k in (1, 3): tap i reads slot i."""
    assert dilation == 1 or (ksize == 3 and stride == 1), "dilated convolutions: 3x3, stride 1"
    return _whole((H + 2 * (ksize // 2) - ksize) // stride + 1, (W + 2 * (ksize // 2) - ksize) // stride + 1, stride, _offsets(ksize, dilation))


def data_grad_s1(H, W, ksize, dilation=1):
    """Data gradient of a stride-1 layer: the same sum with mirrored offsets on the transposed packing."""
    return _whole(H, W, 1, [(-a, -b) for a, b in _offsets(ksize, dilation)])


def class_taps(k, pad, py, px):
    """Taps of output-parity class (py, px) of a stride-2 transposed convolution / data gradient: the forward conv reads
    iy = 2 oy + ky - pad, so pixel iy = 2 a + py receives from (ky, oy = a + (py + pad - ky) / 2)."""
    ys = [(ky, (py + pad - ky) // 2) for ky in range(k) if (py + pad - ky) % 2 == 0]
    xs = [(kx, (px + pad - kx) // 2) for kx in range(k) if (px + pad - kx) % 2 == 0]
    return [(oy, ox, ky * k + kx) for (ky, oy) in ys for (kx, ox) in xs]


def parity_classes(H, W, k, pad, pad4=False):
    """The H x W input of a stride-2 k x k layer, written from the layer's output (gradient) as up to four problems, one per parity
    class of the written pixel (out_stride 2).  A class without a tap (1x1: the odd pixels) or without a pixel is no problem.
    pad4: every class gets four taps - the padding taps repeat the class's first offset (any offset inside the halo) and read tap slot
    k * k, which the packing keeps zero (ParamW.pad_t = 1)."""
    out = []
    for ci, (py, px) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
        taps, Ho, Wo = class_taps(k, pad, py, px), (H - py + 1) // 2, (W - px + 1) // 2
        if taps and Ho > 0 and Wo > 0:
            if pad4:
                taps = taps + [(taps[0][0], taps[0][1], k * k)] * (4 - len(taps))
            out.append(ConvGeometry(Ho, Wo, 1, 2, py, px, taps, k * k + (1 if pad4 else 0), ci))
    return out


def data_grad_s2(H, W, ksize, pad4=False):
    """Data gradient of a stride-2 layer (k in (1, 3), padding k // 2) with an H x W input."""
    assert ksize in (1, 3)
    return parity_classes(H, W, ksize, ksize // 2, pad4)


def deconv4x4s2_forward(H, W):
    """ConvTranspose2d(4, stride 2, padding 1) of an H x W input = V's data gradient: 2 x 2 taps per class on V's transposed packing."""
    return parity_classes(2 * H, 2 * W, 4, 1)


def deconv4x4s2_data_grad(H, W):
    """... and its gradient with respect to that input = V's forward: 16 taps, in_stride 2."""
    return _whole(H, W, 2, TAPS4_DECONV)


def stem_s2d(H, W):
    """Conv2d(7, stride 2, padding 3) as a 4 x 4 stride-1 convolution over the H x W space-to-depth image."""
    return _whole(H, W, 1, TAPS4_STEM)


def stem_index_maps(cout, cin):
    """-> (idx_w [cout, 4 cin, 16], idx_g [cout, cin, 49]) int32.  idx_w: element of the stem's 4 x 4 weight w'[co][(dy, dx, c)][ty, tx] =
    w[co][c][2 ty + dy - 1][2 tx + dx - 1] -> flat index into w, -1 where the 8 x 8 embedding has no 7 x 7 entry; idx_g: element of w ->
    flat index into dW'."""
    idx_w = np.full((cout, 4 * cin, 16), -1, dtype=np.int32)
    idx_g = np.zeros((cout, cin, 49), dtype=np.int32)
    co, c = np.arange(cout)[:, None], np.arange(cin)[None, :]
    for dy, dx, ty, tx in np.ndindex(2, 2, 4, 4):
        ky, kx = 2 * ty + dy - 1, 2 * tx + dx - 1
        if ky >= 0 and kx >= 0:
            q = (dy * 2 + dx) * cin + c
            idx_w[co, q, ty * 4 + tx] = (co * cin + c) * 49 + ky * 7 + kx
            idx_g[co, c, ky * 7 + kx] = (co * 4 * cin + q) * 16 + ty * 4 + tx
    return idx_w, idx_g


def shifted_taps(H, W, dilation):
    """3x3 layer (stride 1, padding = dilation) as ONE-tap problems over its nine tap slots, each on the rectangle of output pixels whose
    source pixel lies inside the image - the offset folded into the window, so that no problem needs border handling.  The centre tap
    (the whole image) comes first; a tap whose rectangle is empty is no problem."""
    out = []
    for i, (a, b) in sorted(enumerate(TAPS3), key=lambda kv: (kv[1] != (0, 0), kv[0])):
        ty, tx = a * dilation, b * dilation
        y0, y1, x0, x1 = max(0, -ty), min(H, H - ty), max(0, -tx), min(W, W - tx)
        if y1 > y0 and x1 > x0:
            out.append(ConvGeometry(y1 - y0, x1 - x0, 1, 1, y0, x0, [(y0 + ty, x0 + tx, i)], 9))
    return out


def wgrad(ksize, stride=1, dilation=1):
    """Weight gradient of a k x k layer, k in (1, 3): the forward offsets."""
    return WgradGeometry(stride, _offsets(ksize, dilation))


def wgrad_groups(offsets, in_stride):
    """Weight gradient of a 16-tap kernel (TAPS4_DECONV, TAPS4_STEM) as four launches of one kernel row each."""
    return [WgradGeometry(in_stride, offsets[4 * g:4 * g + 4], len(offsets), 4 * g) for g in range(4)]


def fill_conv(geo, src, dst, dtype, d=None, w=None, res=None):
    """Geometry `geo` reading Operand `src`, writing Operand `dst` -> nv.ConvDesc (a new one, or `d`).  dtype: hrp_dtype code.
    w: address of the packed weights where it is known already.  res: (address, pitch) of the residual; None leaves the pointer
    alone and sets res_pitch to dst's."""
    d = nv.ConvDesc() if d is None else d
    assert src.N == dst.N and 0 < len(geo.taps) <= nv.MAX_TAPS and all(0 <= t < geo.w_ntaps for _, _, t in geo.taps)
    assert geo.out_off_y + (geo.Ho - 1) * geo.out_stride < dst.H and geo.out_off_x + (geo.Wo - 1) * geo.out_stride < dst.W, \
        "the problem would write outside its output"
    d.x, d.y, d.dtype = src.ptr, dst.ptr, dtype
    if w is not None:
        d.w = w
    d.N, d.H, d.W, d.Cin, d.x_pitch = src.N, src.H, src.W, rup(src.C, ELEM[dtype][1]), src.pitch
    d.Ho, d.Wo, d.Cout = geo.Ho, geo.Wo, dst.C
    d.y_H, d.y_W, d.y_pitch, d.res_pitch = dst.H, dst.W, dst.pitch, dst.pitch
    if res is not None:
        d.res, d.res_pitch = res
    d.in_stride, d.out_stride, d.out_off_y, d.out_off_x = geo.in_stride, geo.out_stride, geo.out_off_y, geo.out_off_x
    d.ntaps, d.w_ntaps, d.w_cout_pad = len(geo.taps), geo.w_ntaps, rup(dst.C, 32)
    for i, (a, b, t) in enumerate(geo.taps):
        d.dy[i], d.dx[i], d.wtap[i] = a, b, t
    return d


def fill_wgrad(geo, x, dy, dw, dw_cin, dtype, accumulate):
    """Geometry `geo` on the layer input `x` and the output gradient `dy` (Operands) -> nv.WgradDesc.  dw: address of the fp32
    gradient [Cout][dw_cin][taps]."""
    g = nv.WgradDesc()
    assert x.N == dy.N and 0 < len(geo.taps) <= nv.MAX_TAPS
    g.x, g.dy, g.dw, g.dtype = x.ptr, dy.ptr, dw, dtype
    g.N, g.H, g.W, g.Cin, g.x_pitch = x.N, x.H, x.W, rup(x.C, ELEM[dtype][1]), x.pitch
    g.Ho, g.Wo, g.Cout, g.dy_pitch = dy.H, dy.W, dy.C, dy.pitch
    g.in_stride, g.ntaps = geo.in_stride, len(geo.taps)
    for i, (a, b) in enumerate(geo.taps):
        g.dy_t[i], g.dx_t[i] = a, b
    g.dw_cin, g.dw_tap_stride, g.dw_tap_off, g.accumulate = dw_cin, geo.dw_tap_stride, geo.dw_tap_off, accumulate
    return g
