"""Float64 oracle of one convolution problem (`hrp_conv_desc`, include/hrp.h), evaluated literally from the descriptor's definition:

    y[n, oy * out_stride + out_off_y, ox * out_stride + out_off_x, :] = epilogue( sum_i W[wtap[i]] . x[n, oy * in_stride + dy[i], ox * in_stride + dx[i], :] )

with zero outside the image and the epilogue  v + bias -> v * scale + shift -> v + res -> relu(v).  Nothing here knows how a kernel
tiles, stages or orders the sum, nor which taps and windows the plans choose: those come from the package's conv_geometry module
(from_geometry) or from a descriptor the real builder filled (problem_of).  Also here: the same literal evaluation of an hrp_wgrad_desc,
and the integer operand generators of the exact-arithmetic tests.

With small non-zero integer operands every product and every partial sum of a problem is an integer below 2^24: bf16 MFMA, fp32 and
the fp32x3 split all compute it exactly in any order, the oracle is exact, and a kernel is compared with torch.equal.  A bf16 output
must be representable: `assert_representable` is the precondition on a test's INPUTS, checked on the oracle's result alone."""
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import torch

F64 = torch.float64


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


# ---- operands and packings ----------------------------------------------------------------------------------------------------------

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


# ---- geometries and descriptors read back ---------------------------------------------------------------------------------------------------------

def from_geometry(x, w, geo, y_H=0, y_W=0, y_pitch=0, **kw):
    """A conv_geometry.ConvGeometry (window, strides, taps) on the operands x and w as a Problem."""
    assert w.shape[0] == geo.w_ntaps, "the geometry reads another packing"
    return Problem(x, w, list(geo.taps), geo.Ho, geo.Wo, y_H=y_H, y_W=y_W, y_pitch=y_pitch, in_stride=geo.in_stride,
                   out_stride=geo.out_stride, out_off=(geo.out_off_y, geo.out_off_x), **kw)


def problem_of(d, x, slots, res=None, bias=None, scale=None, shift=None):
    """A filled hrp_conv_desc (ctypes nv.ConvDesc) as a Problem on the host operands x [N, H, W, C] and slots [w_ntaps, Cout, C]:
    window, strides and taps are the descriptor's; the descriptor must describe these operands (shapes, tap slots, channel padding)."""
    N, H, W, Cc = x.shape
    assert (d.N, d.H, d.W) == (N, H, W) and Cc <= d.Cin <= d.x_pitch, "the descriptor reads another input"
    assert tuple(slots.shape) == (d.w_ntaps, d.Cout, Cc) and d.w_cout_pad == -(-d.Cout // 32) * 32, "the descriptor reads another packing"
    assert 0 < d.ntaps <= len(d.dy) and d.Cout <= d.y_pitch
    taps = [(d.dy[i], d.dx[i], d.wtap[i]) for i in range(d.ntaps)]
    assert all(0 <= t < d.w_ntaps for _, _, t in taps), "a tap reads a slot the packing does not have"
    return Problem(x, slots, taps, d.Ho, d.Wo, y_H=d.y_H, y_W=d.y_W, y_pitch=d.y_pitch, in_stride=d.in_stride, out_stride=d.out_stride,
                   out_off=(d.out_off_y, d.out_off_x), bias=bias, scale=scale, shift=shift, res=res, relu=bool(d.relu))


def evaluate_wgrad(g, x, dy, dw0=None):
    """hrp_wgrad_desc (include/hrp.h) evaluated literally in float64 on x [N, H, W, Cin] and dy [N, Ho, Wo, Cout]:

        dW[co][ci][t] (+)= sum_{n, oy, ox} dy[n, oy, ox, co] * x[n, oy * in_stride + dy_t[t], ox * in_stride + dx_t[t], ci]

    stored at (co * dw_cin + ci) * T + dw_tap_off + t with T = dw_tap_stride or, 0, ntaps.  -> (dw [Cout, dw_cin, T] after the launch
    given its contents before (dw0, zero when None), bool mask of the elements the launch writes)."""
    N, H, W, Cc = x.shape
    assert (g.N, g.H, g.W) == (N, H, W) and Cc <= g.Cin <= g.x_pitch and Cc <= g.dw_cin, "the descriptor reads another input"
    assert tuple(dy.shape) == (N, g.Ho, g.Wo, g.Cout) and g.Cout <= g.dy_pitch, "the descriptor reads another output gradient"
    T = g.dw_tap_stride or g.ntaps
    assert 0 < g.ntaps and 0 <= g.dw_tap_off and g.dw_tap_off + g.ntaps <= T
    dw = torch.zeros(g.Cout, g.dw_cin, T, dtype=F64) if dw0 is None else dw0.to(F64).clone()
    assert tuple(dw.shape) == (g.Cout, g.dw_cin, T)
    wr = torch.zeros_like(dw, dtype=torch.bool)
    x, dy, s = x.to(F64), dy.to(F64), g.in_stride
    for t in range(g.ntaps):
        a0, a1 = _span(g.Ho, H, s, g.dy_t[t])
        b0, b1 = _span(g.Wo, W, s, g.dx_t[t])
        v = torch.zeros(g.Cout, Cc, dtype=F64)
        if a1 > a0 and b1 > b0:
            xs = x[:, a0 * s + g.dy_t[t]:(a1 - 1) * s + g.dy_t[t] + 1:s, b0 * s + g.dx_t[t]:(b1 - 1) * s + g.dx_t[t] + 1:s, :]
            v = torch.einsum("nyxo,nyxc->oc", dy[:, a0:a1, b0:b1], xs)
        k = g.dw_tap_off + t
        dw[:, :Cc, k] = v + (dw[:, :Cc, k] if g.accumulate else 0)
        wr[:, :Cc, k] = True
    return dw, wr


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


# ---- operands of the exact weight-gradient tests ----------------------------------------------------------------------------------------
# Magnitudes (signs are drawn).  BF16_INTS are bf16 numbers.  WIDE_INTS are not: they need 9 or 10 significant bits, so a path that
# rounds an fp32 operand to bf16 changes them - yet each is hi + lo with hi = bf16(v), lo = bf16(v - hi) exactly, so the fp32x3 kernels'
# hi.hi + hi.lo + lo.hi is the exact product with a bf16 integer (the dropped lo.lo term is zero because the other operand's lo is).
BF16_INTS = (1, 2, 3)
WIDE_INTS = (257, 259, 1001)
WIDE_INTS_SMALL = (257, 259, 261)
EXACT_LIMIT = 2 ** 24


def split_planes(v):
    """The fp32x3 kernels' operand split, with torch on the CPU: hi = rne_bf16(v), lo = rne_bf16(v - hi)."""
    v = v.to(torch.float32)
    hi = v.to(torch.bfloat16).to(torch.float32)
    lo = (v - hi).to(torch.bfloat16).to(torch.float32)
    return hi, lo


def assert_value_class(t, wide, what):
    """wide: every value differs from its bf16 rounding AND equals hi + lo; otherwise every value is a bf16 number."""
    hi, lo = split_planes(t)
    assert bool((t != 0).all()) and bool((t == t.round()).all()), f"{what}: operands are non-zero integers"
    if wide:
        assert bool((hi.to(F64) != t.to(F64)).all()), f"{what}: some values are bf16 numbers - a rounded operand would pass"
        assert bool(((hi + lo).to(F64) == t.to(F64)).all()), f"{what}: some values are not hi + lo - the three products are not exact"
    else:
        assert bool((hi.to(F64) == t.to(F64)).all()) and bool((lo == 0).all()), f"{what}: some values are no bf16 numbers"


def wgrad_values(dt, split, pixels):
    """(x magnitudes, dy magnitudes) of a weight-gradient problem summed over `pixels` positions: the richest sets that keep
    pixels * max|x| * max|dy| + 7 below 2^24.  bf16: bf16 integers.  f32 / f32x3: the operand `split` ("x" / "dy") comes from the
    integers that are no bf16 numbers, the other from bf16 integers."""
    if dt == "bf16":
        cands = [(BF16_INTS, BF16_INTS)]
    else:
        cands = [(WIDE_INTS, BF16_INTS), (WIDE_INTS_SMALL, BF16_INTS), (WIDE_INTS_SMALL, (1,))]
    for wide, small in cands:
        if pixels * max(wide) * max(small) + 7 < EXACT_LIMIT:
            return (wide, small) if split == "x" or dt == "bf16" else (small, wide)
    raise AssertionError(f"{pixels} pixels: no value set keeps the sums below 2^24")


def signed(g, shape, mags):
    return pick(g, shape, tuple(mags) + tuple(-m for m in mags))


def wgrad_operands(g, dt, split, N, H, W, cin, Ho, Wo, cout):
    """x [N, H, W, cin], dy [N, Ho, Wo, cout] as float64 integers of the problem's value class."""
    xm, dm = wgrad_values(dt, split, N * Ho * Wo)
    return signed(g, (N, H, W, cin), xm), signed(g, (N, Ho, Wo, cout), dm)


def assert_wgrad_exact(x, dy, dw0, pixels):
    """The precondition of an exact weight gradient, on the operands alone."""
    bound = pixels * float(x.abs().max()) * float(dy.abs().max()) + float(dw0.abs().max())
    assert bound < EXACT_LIMIT, f"N Ho Wo max|x| max|dy| + max|dw0| = {bound} >= 2^24: the test's inputs are wrong"


def representable(t, dtype=torch.bfloat16):
    return bool((t.to(dtype).to(F64) == t.to(F64)).all())


def assert_representable(t, what="reference"):
    bad = t.to(torch.bfloat16).to(F64) != t.to(F64)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} values are no bf16 numbers (max |v| = {t.abs().max().item()}): the test's inputs are wrong"


def assert_stats_exact(stats, cout):
    """The fp32 partial sums of the statistics are exact integers when the per-channel sum of squares stays below 2^24."""
    assert float(stats[cout:].max()) < 2 ** 24 and float(stats[:cout].abs().max()) < 2 ** 24, \
        f"per-channel sum of y^2 = {float(stats[cout:].max())} >= 2^24: the test's inputs are wrong"
