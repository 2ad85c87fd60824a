"""Oracle of the fused element-wise op and the BatchNorm table kernels, restated from include/hrp.h (hrp_ew_desc,
hrp_ew_bwd_desc, hrp_ew_pool2, hrp_bn_entry) in plain torch, plus the device-buffer / descriptor builders the GPU tests share.

Every formula takes `dt`: torch.float64 is the oracle, torch.float32 the restatement the arithmetic tests measure their noise
floor with (same formulas, torch's own evaluation order - nothing of the kernels' loops is copied).  Layout is NHWC.

LeakyReLU: the slope is the fp32 constant 0.01f (nn.LeakyReLU() evaluates in fp32); SLOPE is that number, so the product with a
small integer is one correctly rounded fp32 multiply in the oracle as on the device.
"""
import ctypes as C

import numpy as np
import torch

IDENTITY, AFFINE, BN_TRAIN = 0, 1, 2
SLOTS = 8                                   # HRP_STAT_SLOTS
SLOPE = float(np.float32(0.01))
VEC = {torch.bfloat16: 8, torch.float32: 4}  # channels per 16-byte vector = channels per mask byte
F64 = torch.float64


class OIn:
    """One input of the op: x [N, H/up, W/up, C] (values already rounded to the element type)."""

    def __init__(self, x, up=1, mode=IDENTITY, a=None, b=None, stats=None, count=0.0, eps=1e-5):
        self.x, self.up, self.mode, self.a, self.b, self.stats, self.count, self.eps = x, up, mode, a, b, stats, count, eps


def slot_total(stats):
    """[SLOTS][n] double -> [n]: only the sum over the slots is defined."""
    return stats.to(F64).sum(0)


def consts(inp, Cn, dt=F64):
    """scale, shift, mean, invstd [C] of an input (hrp_ew_input)."""
    one, zero = torch.ones(Cn, dtype=dt), torch.zeros(Cn, dtype=dt)
    if inp.mode == IDENTITY:
        return one, zero, zero, one
    if inp.mode == AFFINE:
        a, b = inp.a.to(dt), inp.b.to(dt)
        return a, b, torch.where(a != 0, -b / torch.where(a != 0, a, one), zero), a
    s = slot_total(inp.stats).to(dt)
    cnt = torch.tensor(inp.count, dtype=dt)
    mean = s[:Cn] / cnt
    var = (s[Cn:] / cnt - mean * mean).clamp_min(0)
    inv = 1.0 / torch.sqrt(var + torch.tensor(inp.eps, dtype=dt))
    sc = inp.a.to(dt) * inv
    return sc, inp.b.to(dt) - mean * sc, mean, inv


def upsample(x, up):
    return x if up == 1 else x.repeat_interleave(up, 1).repeat_interleave(up, 2)


def pack_bits(pos, vec):
    """[..., C] bool -> [..., ceil(C / vec)] uint8, bit i of byte k = channel vec * k + i."""
    Cn = pos.shape[-1]
    nb = -(-Cn // vec)
    p = torch.zeros(pos.shape[:-1] + (nb * vec,), dtype=torch.int32)
    p[..., :Cn] = pos.to(torch.int32)
    w = (1 << torch.arange(vec, dtype=torch.int32))
    return (p.view(pos.shape[:-1] + (nb, vec)) * w).sum(-1).to(torch.uint8)


def activate(pre, relu):
    if relu == 0:
        return pre
    neg = torch.zeros_like(pre) if relu == 1 else pre * torch.tensor(SLOPE, dtype=pre.dtype)
    return torch.where(pre > 0, pre, neg)


def ew_forward(inputs, relu, vec, dt=F64):
    """-> pre-activation, output, mask bytes.  out = act(sum_j f_j(in_j[n, y // up, x // up, c]))."""
    Cn = inputs[0].x.shape[-1]
    pre = None
    for inp in inputs:
        sc, sh, _, _ = consts(inp, Cn, dt)
        t = upsample(inp.x.to(dt), inp.up) * sc + sh
        pre = t if pre is None else pre + t
    return pre, activate(pre, relu), pack_bits(pre > 0, vec)


def masked_grad(dout, pos, relu, dt=F64):
    """g at output resolution: dOut where the output was positive, slope * dOut elsewhere (0 for ReLU)."""
    d = dout.to(dt)
    if relu == 0:
        return d
    return torch.where(pos, d, torch.zeros_like(d) if relu == 1 else d * torch.tensor(SLOPE, dtype=dt))


def window_sum(g, up):
    if up == 1:
        return g
    N, H, W, Cn = g.shape
    return g.view(N, H // up, up, W // up, up, Cn).sum((2, 4))


def ew_backward(dout, pos, inp, relu, sums=None, din_old=None, din2_old=None, dt=F64, g=None):
    """Backward of one input.  pos: where the forward output was > 0 (None with relu == 0).  g may be given (the `pooled` tensor).
    sums: [2C] totals the apply pass of a BN_TRAIN input reads (default: the ones computed here).
    -> dict g [N, H/up, W/up, C], sums [2C] = (sum g, sum g * xhat), din (+ din_old), din2 = g (+ din2_old)."""
    Cn = dout.shape[-1]
    if g is None:
        g = window_sum(masked_grad(dout, pos, relu, dt), inp.up)
    g = g.to(dt)
    sc, _, mean, inv = consts(inp, Cn, dt)
    r = {"g": g}
    xhat = None
    if inp.x is not None:
        xhat = (inp.x.to(dt) - mean) * inv
        r["sums"] = torch.cat([g.sum((0, 1, 2)), (g * xhat).sum((0, 1, 2))])
    if inp.mode == IDENTITY:
        din = g
    elif inp.mode == AFFINE:
        din = sc * g
    else:
        s = (r["sums"] if sums is None else sums).to(dt)
        cnt = torch.tensor(inp.count, dtype=dt)
        din = sc * (g - s[:Cn] / cnt - xhat * (s[Cn:] / cnt))
    r["din"] = din if din_old is None else din + din_old.to(dt)
    r["din2"] = g if din2_old is None else g + din2_old.to(dt)
    return r


def pool2(src, pos=None, dt=F64):
    """2 x 2 window sums of src [N, H, W, C] (masked by pos), order ((a + b) + (c + d)) as the header fixes it."""
    s = src.to(dt)
    if pos is not None:
        s = torch.where(pos, s, torch.zeros_like(s))
    return (s[:, 0::2, 0::2] + s[:, 0::2, 1::2]) + (s[:, 1::2, 0::2] + s[:, 1::2, 1::2])


def bn_moments(stats, Cn, count, dt=F64):
    s = slot_total(stats).to(dt)
    cnt = torch.tensor(count, dtype=dt)
    mean = s[:Cn] / cnt
    return mean, (s[Cn:] / cnt - mean * mean).clamp_min(0)


def bn_running_update(stats, rmean, rvar, count, momentum, dt=F64):
    """-> running_mean, running_var after one train-mode step (unbiased variance when count > 1)."""
    Cn = rmean.numel()
    mean, var = bn_moments(stats, Cn, count, dt)
    if count > 1:
        var = var * (torch.tensor(count, dtype=dt) / torch.tensor(count - 1.0, dtype=dt))
    m = torch.tensor(momentum, dtype=dt)
    return (1 - m) * rmean.to(dt) + m * mean, (1 - m) * rvar.to(dt) + m * var


def bn_fold(gamma, beta, rmean, rvar, eps, dt=F64):
    sc = gamma.to(dt) / torch.sqrt(rvar.to(dt) + torch.tensor(eps, dtype=dt))
    return sc, beta.to(dt) - rmean.to(dt) * sc


def bn_param_grad(sums, Cn, dgamma_old=None, dbeta_old=None, dt=F64):
    """backward sums [SLOTS][2C] = (sum g, sum g * xhat) -> dgamma, dbeta."""
    s = slot_total(sums).to(dt)
    dg, db = s[Cn:], s[:Cn]
    return (dg if dgamma_old is None else dg + dgamma_old.to(dt)), (db if dbeta_old is None else db + dbeta_old.to(dt))


def batch_stats(x):
    """[2C] float64 (sum, sum of squares) of x over its pixels."""
    v = x.to(F64).reshape(-1, x.shape[-1])
    return torch.cat([v.sum(0), (v * v).sum(0)])


def spread_slots(total, gen):
    """[n] float64 -> [SLOTS][n] with uneven, partly negative shares: no single slot (and no subset) is the statistic."""
    w = torch.tensor([2.5, -1.25, 0.5, -0.75, 0.125, 1.0, -1.5, 0.0], dtype=F64)
    w = w[torch.randperm(SLOTS, generator=gen)]
    w[-1] = 1.0 - w[:-1].sum()
    return w[:, None] * total.to(F64)[None, :]


def near_zero_share(pre, floor):
    return float((pre.abs() <= floor).to(F64).mean())


# ---- device side (plain torch + ctypes; the host tests use only what is above) ----------------------------------------------
FSENT = -768.0    # exact in bf16; the integer data stays within +-512 * 8
BSENT = 0xA5


class Buf:
    """[rows][pitch] device buffer inside a larger allocation filled with a sentinel: guard rows before and after, the pitch
    padding between the rows.  offset: elements the base pointer is shifted by (misalignment cases)."""

    def __init__(self, rows, Cn, pitch, tdt, dev, offset=0, guard=3):
        self.rows, self.C, self.pitch = rows, Cn, pitch
        self.sent = BSENT if tdt == torch.uint8 else FSENT
        self.lead = -(-guard * pitch // 64) * 64 + offset
        self.t = torch.full((self.lead + (rows + guard) * pitch + 64,), self.sent, dtype=tdt, device=dev)

    @property
    def ptr(self):
        return self.t.data_ptr() + self.lead * self.t.element_size()

    def region(self, t=None):
        t = self.t if t is None else t
        return t[self.lead:self.lead + self.rows * self.pitch].view(self.rows, self.pitch)[:, :self.C]

    def put(self, v):
        self.region().copy_(v.reshape(self.rows, self.C).to(self.t.dtype))
        return self

    def get(self, shape=None):
        v = self.region().cpu()
        return v if shape is None else v.reshape(shape)

    def outside_untouched(self):
        c = self.t.clone()
        self.region(c).fill_(self.sent)
        return bool((c == self.sent).all())

    def untouched(self):
        return bool((self.t == self.sent).all())


def dev_f32(v, dev):
    return v.to(torch.float32).contiguous().to(dev)


def fill_input(e, inp, buf, keep, dev):
    """hrp_ew_input <- OIn + its device buffer (None: in.ptr == NULL)."""
    e.ptr, e.pitch = (buf.ptr, buf.pitch) if buf is not None else (None, 0)
    e.up, e.mode, e.count, e.eps = inp.up, inp.mode, float(inp.count), float(inp.eps)
    if inp.mode != IDENTITY:
        a, b = dev_f32(inp.a, dev), dev_f32(inp.b, dev)
        keep += [a, b]
        e.a, e.b = a.data_ptr(), b.data_ptr()
    if inp.mode == BN_TRAIN and inp.stats is not None:
        s = inp.stats.to(F64).contiguous().to(dev)
        keep.append(s)
        e.stats = s.data_ptr()


def copy_struct(dst, src):
    C.memmove(C.byref(dst), C.byref(src), C.sizeof(src))


def run_batch(nv, family, descs, dev):
    """hrp_batch_prepare + hrp_batch_launch of the descriptors; -> (rc of prepare, BatchInfo)."""
    n = len(descs)
    arr = (type(descs[0]) * n)()
    for i, d in enumerate(descs):
        copy_struct(arr[i], d)
    info = nv.BatchInfo()
    host = (C.c_char * max(int(nv.lib().hrp_batch_table_bytes(family, n)), 1))()
    rc = nv.lib().hrp_batch_prepare(family, arr, n, host, C.byref(info))
    if rc != 0:
        return rc, info
    table = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(dev)
    nv.check(nv.lib().hrp_batch_launch(table.data_ptr(), C.byref(info), None), "hrp_batch_launch")
    torch.cuda.synchronize()
    return 0, info


# ---- real-valued cases of the arithmetic tests (host test: floors and near-zero shares; GPU test: the kernels) ------------
EPS = 1e-5


def real_input(gen, shape, tdt, up=1, mode=BN_TRAIN, ratio=2.0, exact_ratio=False):
    """Random normal input with per-channel mean and scale, |mean| / std <= ratio (== ratio when exact_ratio), gamma in
    [0.5, 1.5]; values rounded to the element type; BN_TRAIN statistics in float64 spread over the slots."""
    N, H, W, Cn = shape
    h, w = H // up, W // up
    std = 0.5 + 1.5 * torch.rand(Cn, generator=gen, dtype=F64)
    r = torch.full((Cn,), 1.0, dtype=F64) if exact_ratio else 2 * torch.rand(Cn, generator=gen, dtype=F64) - 1
    x = (torch.randn(N, h, w, Cn, generator=gen, dtype=F64) * std + r * ratio * std).to(tdt)
    gamma = 0.5 + torch.rand(Cn, generator=gen, dtype=F64)
    beta = torch.rand(Cn, generator=gen, dtype=F64) - 0.5
    if mode == IDENTITY:
        return OIn(x, up)
    if mode == AFFINE:
        return OIn(x, up, AFFINE, gamma.float(), beta.float())
    return OIn(x, up, BN_TRAIN, gamma.float(), beta.float(), spread_slots(batch_stats(x), gen), float(N * h * w), EPS)


# name -> (element type, (N, H, W, C), [(up, mode)], ratio).  C: vector one-slab, scalar, vector two-slab, scalar two-slab.
ARITH_FWD = {
    "bf16-bn-alone": (torch.bfloat16, (2, 8, 12, 64), [(1, BN_TRAIN)], 2.0),
    "f32-bn-alone": (torch.float32, (2, 8, 12, 36), [(1, BN_TRAIN)], 2.0),
    "bf16-bn-residual": (torch.bfloat16, (2, 8, 12, 64), [(1, BN_TRAIN), (1, IDENTITY)], 2.0),
    "f32-bn-residual": (torch.float32, (2, 8, 12, 36), [(1, BN_TRAIN), (1, IDENTITY)], 2.0),
    "bf16-bn-fuse4": (torch.bfloat16, (1, 16, 16, 32), [(1, BN_TRAIN), (2, BN_TRAIN), (4, BN_TRAIN), (8, AFFINE)], 2.0),
    "f32-bn-fuse4": (torch.float32, (1, 16, 16, 32), [(1, BN_TRAIN), (2, BN_TRAIN), (4, BN_TRAIN), (8, AFFINE)], 2.0),
    "f32-bn-mean30": (torch.float32, (2, 8, 12, 36), [(1, BN_TRAIN)], 30.0),
}
# the whole chain fwd -> reduce -> apply -> param_grad on one BN_TRAIN tensor: (element type, (N, H, W, C), up)
ARITH_CHAIN = {
    "bf16-vec-1slab-up1": (torch.bfloat16, (2, 8, 12, 64), 1), "bf16-scalar-up1": (torch.bfloat16, (2, 8, 12, 36), 1),
    "bf16-vec-2slab-up1": (torch.bfloat16, (1, 6, 8, 576), 1), "bf16-scalar-2slab-up2": (torch.bfloat16, (1, 6, 8, 300), 2),
    "f32-vec-1slab-up2": (torch.float32, (2, 8, 12, 64), 2), "f32-scalar-up1": (torch.float32, (2, 8, 12, 7), 1),
    "f32-vec-2slab-up1": (torch.float32, (1, 6, 8, 520), 1), "f32-scalar-2slab-up2": (torch.float32, (1, 6, 8, 257), 2),
    "bf16-vec-1slab-up2": (torch.bfloat16, (2, 8, 12, 64), 2),
}


def seed_of(name):
    return 1000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 9973


def arith_fwd_case(name):
    tdt, shape, ins, ratio = ARITH_FWD[name]
    gen = torch.Generator().manual_seed(seed_of(name))
    return tdt, shape, [real_input(gen, shape, tdt, up, mode, ratio, exact_ratio=ratio > 2.0) for up, mode in ins]


def arith_chain_case(name):
    tdt, shape, up = ARITH_CHAIN[name]
    gen = torch.Generator().manual_seed(seed_of(name))
    inp = real_input(gen, shape, tdt, up, BN_TRAIN)
    dout = torch.randn(shape, generator=gen, dtype=F64).to(tdt)
    return tdt, shape, inp, dout


def rel_dev(a, ref):
    """max |a - ref| relative to the tensor's scale max |ref|."""
    return float((a.to(F64) - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def chain_oracle(inp, dout, tdt, dt):
    """The chain in precision dt.  The device stores `out` and `din` in the element type and hands the sums over as doubles;
    the mask comes from the fp32 pre-activation.  -> pre, out, sums [2C], din, dgamma, dbeta (all dt, unrounded)."""
    pre, out, _ = ew_forward([inp], 1, VEC[tdt], dt)
    b = ew_backward(dout, pre > 0, inp, 1, dt=dt)
    dgamma, dbeta = bn_param_grad(b["sums"][None, :].to(F64), dout.shape[-1], dt=dt)
    return pre, out, b["sums"], b["din"], dgamma, dbeta
