"""Float64 statement of CtRNet's key-point read-out (reference lib/models/ctrnet/keypoint_seg_resnet.py:29-33, 75-100, 137-143) and
the exact operands hrp_kp_readout_fwd is tested on.

``readout64``: F.conv_transpose2d(stride 2, padding 1), softmax over the positions and the weighted mean of fp32-cast
``torch.linspace(-1, 1, n)`` coordinates, all in float64; then ``(mean - (lim[0], lim[2])) * (width // 2, height // 2)``.

Exact operands (the argument of tests/conv_exact_oracle.py): features are integers in -2 .. 2, weights integers in -2 .. 2 times
2^-s, the bias a multiple of 0.25.  A logit is a sum of at most 4 Cin products, each an integer of magnitude <= 4 in units of
2^-s: every partial sum is an integer below 2^24 in those units for Cin <= 2^19, so every product and partial sum is exact in the
bf16 MFMA (fp32 accumulation) and in fp32, IN ANY ORDER, and the logits of a correct kernel equal the float64 ones bit for bit.  What
is left to a tolerance is the softmax itself.  s is chosen per Cin so that the logits have a standard deviation of about 2.5."""
import math

import numpy as np
import torch
import torch.nn.functional as F

LIM = (-0.75, 1.0, -1.25, 1.0)          # exact in fp32; not the default, so a kernel that ignores lim fails
SIZE = (640, 480)                       # (width, height): scale = (320, 240)
# (B, Cin, k, Hin, Win)
SHAPES = [(1, 32, 17, 1, 1),            # one K step, every tap at an edge, p_max 0.96 (s = 2)
          (1, 96, 1, 2, 2),             # Cin not a power of two, one channel
          (2, 64, 7, 3, 5),             # odd sides
          (1, 64, 32, 2, 3),            # maximum k
          (2, 2048, 7, 6, 8),           # the product's Cin
          (1, 32, 3, 2, 40),            # 32 < Win <= 64: the second 32-position tile of a workgroup holds valid rows
          (1, 32, 2, 1, 70),            # Win > 64: a second pass over the positions, the running softmax sums are rescaled
          (1, 64, 5, 3, 131)]           # three passes, the last one with 3 positions
# spikes at the last and at the first output position: on a narrow map (one pass), and on one wider than 64, where the maximum of
# one channel arrives in the last pass over a row's positions and that of another in the first
SPIKE_SHAPES = [(1, 64, 7, 3, 5), (1, 64, 7, 2, 70)]


def seam_shapes(strip):
    """One strip + 1 and two strips + 1 input rows: the last workgroup of a batch element holds a single row."""
    return [(1, 32, 3, strip + 1, 3), (2, 32, 5, 2 * strip + 1, 2)]


def all_cases(strip):
    """(shape, spikes) of every exact case for a strip height"""
    return [(s, False) for s in SHAPES + seam_shapes(strip)] + [(s, True) for s in SPIKE_SHAPES]


def shift_for(cin, shape=None):
    """s with std(logit) = 4 sqrt(Cin) 2^-s ~ 2.5 (x and w uniform integers in -2 .. 2: variance 2 each, 4 Cin products); the
    four-position map of the first shape takes s = 2, which puts one channel's peak probability at 0.96."""
    if shape == SHAPES[0]:
        return 2
    return max(0, round(math.log2(4.0 * math.sqrt(cin) / 2.5)))


def seed_of(shape, spikes=False):
    return 1000003 * shape[1] + 10007 * shape[2] + 101 * shape[3] + 7 * shape[4] + shape[0] + (5 if spikes else 0)


def operands(shape, spikes=False):
    """-> x [B, Cin, Hin, Win], w [Cin, k, 4, 4], b [k] (float64 tensors), s.  spikes: channel 0 gets a logit far above the rest at
    the LAST output position in scan order and channel k - 1 one at the FIRST, each built by aligning one input pixel with the signs
    of the one tap that reaches that corner (w[:, c, 2, 2] for the last position, w[:, c, 1, 1] for the first); the other pixels
    then are integers in -1 .. 1 and s = 1."""
    B, cin, k, hin, win = shape
    g = torch.Generator().manual_seed(seed_of(shape, spikes))
    s = 1 if spikes else shift_for(cin, tuple(shape))
    lo, hi = (-1, 2) if spikes else (-2, 3)
    x = torch.randint(lo, hi, (B, cin, hin, win), generator=g).double()
    w = torch.randint(-2, 3, (cin, k, 4, 4), generator=g).double()
    b = torch.randint(-8, 9, (k,), generator=g).double() * 0.25
    if spikes:
        x[:, :, hin - 1, win - 1] = 2.0 * torch.sign(w[:, 0, 2, 2])
        x[:, :, 0, 0] = 2.0 * torch.sign(w[:, k - 1, 1, 1])
    return x, w * 2.0 ** -s, b, s


def coords(n):
    return torch.linspace(-1, 1, n, dtype=torch.float32).double()


def softargmax64(heat, lim=LIM, size=SIZE):
    """heat [B, k, Ho, Wo] float64 -> dict(kp [B, k, 2] in pixels, max [B, k], pmax [B, k])"""
    B, k, ho, wo = heat.shape
    p = torch.softmax(heat.reshape(B, k, ho * wo), dim=-1).reshape(B, k, ho, wo)
    xm = (p * coords(wo)[None, None, None, :]).sum(dim=(2, 3))
    ym = (p * coords(ho)[None, None, :, None]).sum(dim=(2, 3))
    kp = torch.stack([(xm - lim[0]) * (size[0] // 2), (ym - lim[2]) * (size[1] // 2)], dim=-1)
    return dict(kp=kp, max=heat.amax(dim=(2, 3)), pmax=p.amax(dim=(2, 3)))


def readout64(x, w, b, lim=LIM, size=SIZE):
    """x [B, Cin, Hin, Win], w [Cin, k, 4, 4], b [k] -> softargmax64's dict plus heat [B, k, 2 Hin, 2 Win]"""
    heat = F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2, padding=1)
    out = softargmax64(heat, lim, size)
    out["heat"] = heat
    return out


def nhwc(x, dtype, pad=8):
    """[B, C, H, W] float64 -> the kernel's NHWC operand with a channel pitch of C + pad; returns (tensor, pitch)"""
    B, c, h, w = x.shape
    t = torch.zeros(B, h, w, c + pad, dtype=dtype)
    t[..., :c] = x.permute(0, 2, 3, 1).to(dtype)
    return t, c + pad


def key(shape, spikes=False):
    return "x".join(str(v) for v in shape) + ("_spikes" if spikes else "")
