"""Float64 oracle of one convolution problem (`hrp_conv_desc`, include/hrp.h), evaluated literally from the descriptor's definition:

    y[n, oy * out_stride + out_off_y, ox * out_stride + out_off_x, :] = epilogue( sum_i W[wtap[i]] . x[n, oy * in_stride + dy[i], ox * in_stride + dx[i], :] )

with zero outside the image and the epilogue  v + bias -> v * scale + shift -> v + res -> relu(v).  Nothing here knows how a kernel
tiles, stages or orders the sum.  Also here: the descriptors the plans build (plan.py::_conv_desc / _conv_bwd / stem7x7_s2d) restated
as tap lists, and the integer operand generators of the exact-arithmetic tests.

With small non-zero integer operands every product and every partial sum of a problem is an integer below 2^24: bf16 MFMA, fp32 and
the fp32x3 split all compute it exactly in any order, the oracle is exact, and a kernel is compared with torch.equal.  A bf16 output
must be representable: `assert_representable` is the precondition on a test's INPUTS, checked on the oracle's result alone."""
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import torch

F64 = torch.float64
TAPS3 = [(ky - 1, kx - 1) for ky in range(3) for kx in range(3)]


@dataclass
class Problem:
    """An hrp_conv_desc in host terms.  x: [N, H, W, Cin] float64 (NHWC); w: [slots, Cout, Cin] float64, w[s] = the matrix in tap slot s of
    the packed weights; taps: (dy, dx, wtap) per tap."""
    x: torch.Tensor
    w: torch.Tensor
    taps: List[Tuple[int, int, int]]
    Ho: int
    Wo: int
    y_H: int = 0
    y_W: int = 0
    y_pitch: int = 0
    in_stride: int = 1
    out_stride: int = 1
    out_off: Tuple[int, int] = (0, 0)
    bias: Optional[torch.Tensor] = None          # [Cout]
    scale: Optional[torch.Tensor] = None
    shift: Optional[torch.Tensor] = None
    res: Optional[torch.Tensor] = None           # [N, y_H, y_W, Cout] float64 (res == y: the initial contents of y)
    relu: bool = False
    extra: dict = field(default_factory=dict)

    def __post_init__(self):
        self.y_H = self.y_H or self.Ho
        self.y_W = self.y_W or self.Wo
        self.y_pitch = self.y_pitch or self.w.shape[1]

    @property
    def Cout(self):
        return self.w.shape[1]


@dataclass
class Result:
    y: torch.Tensor         # [N, y_H, y_W, y_pitch] float64: the buffer after the launch, given its contents before (`y0`)
    written: torch.Tensor   # bool, same shape: the elements the launch may write
    pre: torch.Tensor       # [N, Ho, Wo, Cout]: the value before the residual is added (a kernel may round it to the element type)
    out: torch.Tensor       # [N, Ho, Wo, Cout]: the stored values on the logical output grid
    stats: torch.Tensor     # [2 * Cout]: sum and sum of squares of the stored values per channel


def _span(n_out, n_in, stride, off):
    """Output indices o in [0, n_out) whose source o * stride + off lies in [0, n_in): -> (o0, o1), empty when o1 <= o0."""
    o0 = max(0, -(off // stride))                     # ceil(-off / stride)
    o1 = min(n_out, (n_in - 1 - off) // stride + 1) if n_in - 1 - off >= 0 else 0
    return o0, o1


def accumulate(p: Problem) -> torch.Tensor:
    """[N, Ho, Wo, Cout]: the sum over the taps, before the epilogue (forms of one problem that differ in the epilogue share it)."""
    x, w = p.x.to(F64), p.w.to(F64)
    N, H, W, _ = x.shape
    s = p.in_stride
    acc = torch.zeros(N, p.Ho, p.Wo, p.Cout, dtype=F64)
    for dy, dx, slot in p.taps:
        a0, a1 = _span(p.Ho, H, s, dy)
        b0, b1 = _span(p.Wo, W, s, dx)
        if a1 <= a0 or b1 <= b0:
            continue
        xs = x[:, a0 * s + dy:(a1 - 1) * s + dy + 1:s, b0 * s + dx:(b1 - 1) * s + dx + 1:s, :]
        acc[:, a0:a1, b0:b1] += torch.einsum("nyxc,oc->nyxo", xs, w[slot])
    return acc


def window(p: Problem):
    """The rows and columns of y the logical output grid is stored at."""
    o, (fy, fx) = p.out_stride, p.out_off
    assert fy >= 0 and fx >= 0 and fy + (p.Ho - 1) * o < p.y_H and fx + (p.Wo - 1) * o < p.y_W, "the launch would write outside y"
    return slice(fy, fy + (p.Ho - 1) * o + 1, o), slice(fx, fx + (p.Wo - 1) * o + 1, o)


def written(p: Problem) -> torch.Tensor:
    """bool [N, y_H, y_W, y_pitch]: the elements of the y buffer the launch may write."""
    ys, xs = window(p)
    m = torch.zeros(p.x.shape[0], p.y_H, p.y_W, p.y_pitch, dtype=torch.bool)
    m[:, ys, xs, :p.Cout] = True
    return m


def evaluate(p: Problem, y0: Optional[torch.Tensor] = None, acc: Optional[torch.Tensor] = None) -> Result:
    v = accumulate(p) if acc is None else acc
    if p.bias is not None:
        v = v + p.bias.to(F64)
    if p.scale is not None:
        v = v * p.scale.to(F64) + p.shift.to(F64)
    pre = v
    ys, xs = window(p)
    if p.res is not None:
        v = v + p.res.to(F64)[:, ys, xs, :]
    if p.relu:
        v = v.clamp_min(0)
    y = torch.zeros(p.x.shape[0], p.y_H, p.y_W, p.y_pitch, dtype=F64) if y0 is None else y0.to(F64).clone()
    y[:, ys, xs, :p.Cout] = v
    return Result(y, written(p), pre, v, torch.cat([v.sum((0, 1, 2)), (v * v).sum((0, 1, 2))]))


# ---- the descriptors the plans build, as tap lists ------------------------------------------------------------------------------

def forward_taps(ksize, dilation=1):
    """plan.py::_conv_desc: 3x3 (padding = dilation) or 1x1, tap i reads slot i."""
    taps = TAPS3 if ksize == 3 else [(0, 0)]
    return [(a * dilation, b * dilation, i) for i, (a, b) in enumerate(taps)]


def mirrored_taps(ksize, dilation=1):
    """plan.py::_conv_bwd, stride 1: the data gradient is the same sum with mirrored offsets on the transposed packing."""
    return [(-a, -b, i) for a, b, i in forward_taps(ksize, dilation)]


def class_taps(k, pad, py, px):
    """plan.py::_class_taps: taps of output-parity class (py, px) of a stride-2 data gradient.  The forward conv reads
    iy = 2 oy + ky - pad, so pixel iy = 2 a + py receives from (ky, oy = a + (py + pad - ky) / 2)."""
    ys = [(ky, (py + pad - ky) // 2) for ky in range(k) if (py + pad - ky) % 2 == 0]
    xs = [(kx, (px + pad - kx) // 2) for kx in range(k) if (px + pad - kx) % 2 == 0]
    return [(oy, ox, ky * k + kx) for (ky, oy) in ys for (kx, ox) in xs]


def stem_taps():
    """plan.py::stem7x7_s2d: the 7x7 stride-2 stem as a 4x4 stride-1 convolution over the 2x2 space-to-depth image."""
    return [(ty - 2, tx - 2, ty * 4 + tx) for ty in range(4) for tx in range(4)]


def stem_weight_s2d(w7):
    """[Cout, C, 7, 7] -> [Cout, 4 C, 16]: w'[co][(dy, dx, c)][ty, tx] = w[co][c][2 ty + dy - 1][2 tx + dx - 1], zero where the 8x8
    embedding has no 7x7 entry."""
    cout, cin = w7.shape[:2]
    out = torch.zeros(cout, 4 * cin, 16, dtype=w7.dtype)
    for dy in range(2):
        for dx in range(2):
            for ty in range(4):
                for tx in range(4):
                    ky, kx = 2 * ty + dy - 1, 2 * tx + dx - 1
                    if ky >= 0 and kx >= 0:
                        out[:, (dy * 2 + dx) * cin:(dy * 2 + dx + 1) * cin, ty * 4 + tx] = w7[:, :, ky, kx]
    return out


def space_to_depth(x_nchw):
    """hrp_nchw_to_nhwc_s2d: dst[n, y, x, (dy * 2 + dx) * C + c] = src[n, c, 2 y + dy, 2 x + dx]."""
    N, Cc, H, W = x_nchw.shape
    v = x_nchw.view(N, Cc, H // 2, 2, W // 2, 2)          # n c y dy x dx
    return v.permute(0, 2, 4, 3, 5, 1).reshape(N, H // 2, W // 2, 4 * Cc)


def slots_fwd(w):
    """PyTorch weight [Cout, Cin, taps] -> tap slots of the forward packing [taps, Cout, Cin]."""
    return w.permute(2, 0, 1).contiguous()


def slots_bwd(w, pad_t=0):
    """... -> tap slots of the transposed packing [taps + pad_t, Cin, Cout] (the problem's Cout is the layer's Cin); pad_t zero slots."""
    s = w.permute(2, 1, 0).contiguous()
    if pad_t:
        s = torch.cat([s, torch.zeros(pad_t, *s.shape[1:], dtype=s.dtype)], 0)
    return s


# ---- integer operands -----------------------------------------------------------------------------------------------------------

def pick(g, shape, values):
    """Uniform draws from `values` (non-zero integers) as float64."""
    v = torch.tensor(values, dtype=F64)
    return v[torch.randint(0, len(values), shape, generator=g)]


def int_operands(g, N, H, W, cin, cout, ntaps, xvals=(1, -1), wvals=(1, -1), live=None):
    """x [N, H, W, cin] and w [cout, cin, ntaps] of non-zero integers.

    live = k (cin even): only k of the cin / 2 channel pairs (c, c + cin / 2) contribute to the result, the others cancel EXACTLY -
    x[.., c + cin/2] = q(c) x[.., c] and w[:, c + cin/2, :] = -+ q(c) w[:, c, :] - which keeps a wide sum over many pixels small (the
    per-channel sum of y^2 has to stay below 2^24) while every term is still a non-zero product: a term that is missing, doubled or
    taken from another pixel, tap or channel breaks the cancellation."""
    if live is None:
        return pick(g, (N, H, W, cin), xvals), pick(g, (cout, cin, ntaps), wvals)
    h = cin // 2
    assert cin % 2 == 0 and 0 <= live <= h
    x0, w0 = pick(g, (N, H, W, h), xvals), pick(g, (cout, h, ntaps), wvals)
    q = pick(g, (h,), (1, -1))
    keep = torch.zeros(h, dtype=F64)
    keep[torch.randperm(h, generator=g)[:live]] = 1
    sign = (2 * keep - 1) * q                     # live pair: the two halves add up; otherwise they cancel
    x = torch.cat([x0, x0 * q], -1)
    w = torch.cat([w0, w0 * sign[None, :, None]], 1)
    return x, w


def representable(t, dtype=torch.bfloat16):
    return bool((t.to(dtype).to(F64) == t.to(F64)).all())


def assert_representable(t, what="reference"):
    bad = t.to(torch.bfloat16).to(F64) != t.to(F64)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} values are no bf16 numbers (max |v| = {t.abs().max().item()}): the test's inputs are wrong"


def assert_stats_exact(stats, cout):
    """The fp32 partial sums of the statistics are exact integers when the per-channel sum of squares stays below 2^24."""
    assert float(stats[cout:].max()) < 2 ** 24 and float(stats[:cout].abs().max()) < 2 ** 24, \
        f"per-channel sum of y^2 = {float(stats[cout:].max())} >= 2^24: the test's inputs are wrong"
