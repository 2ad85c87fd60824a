"""The cases of the exact-arithmetic weight-gradient tests: one table for tests/test_wgrad_exact_host.py (what the table reaches, asked
from the launcher on the host) and tests/test_gpu_wgrad_exact.py (the launches, against the float64 oracle).  A case is a Prob - a
conv_geometry.WgradGeometry, element type, N, H, W, real input channels Cc (= dw_cin), Cout, the two pitches, the operand that carries the
non-bf16 integers - the paths it runs and, for a batch, its companions.  Descriptors are filled with conv_geometry.fill_wgrad.

Which program a problem runs is the launcher's answer (hrp_wgrad_config_of / hrp_batch_wgrad_configs), pinned in EXPECT_S / EXPECT_B
below; nothing here repeats the tiling arithmetic.  Steering in a batch (wgrad_batch_prepare_nt): a problem's workgroups are
round(512 work / total) (256 among the eight-wave problems), work = pixels x 32-channel block pairs, G = budget / pairs capped at
ntiles - so next to a heavy companion a small problem gets G = 1 and its one workgroup walks all its tiles.

Reached (asserted by the host test), each four-wave instantiation by a single launch AND in a batch:
  conv_wgrad_body<bf16, NT, NKS, 1>    NT 1 / 4 / 9 x NKS 1 / 2 / 4
  conv_wgrad_body<bf16, 1, NKS, 2>     NKS 1 / 2
  conv_wgrad_body<float, NT, 0, 1>     NT 1 / 4 / 9 at BM 16, 64 and 128 (also 32 under stride 2)
  conv_wgrad_body<f32x3, NT, NKS, 1>   NT 1 / 4 / 9 x NKS 1 / 2
  eight-wave bf16 (batched and batched phase 1)   <1, 4>; <4, 4> with ring 3 and with ring 2 (3 x 32 x 1 images: a 306-pixel halo tile);
                                                  <4, 2> (stride 2)
  eight-wave fp32x3                               9 taps with 4 / 2 / 1 k-steps, 1 tap with 4
  the fp32 atomics path with accumulate 0 and 1 for every (type, taps); 1, 2, >= 3 and uneven tiles per workgroup for the four-wave
  program in each type and for both eight-wave programs; xmode 0 and 2; fold G of 1, 2, 3, 6, 32, 33, 35

Not reachable, by the launcher's own limits (the host test sweeps shapes and fails when one of them becomes reachable):
  conv_wgrad_body<bf16, 1, 4, 2>       64-channel blocks are 128 bytes per pixel: the dY tile of 256 pixels is 32 DMA pieces, wgrad_tiling
                                       allows 24, so BM stops at 128 (the same limit makes 128 the largest fp32 BM)
  conv_wgrad_octo_x3_body<1, 2>        a 1-tap tile has no halo: 128 pixels are at most 32 + 32 pieces and 128 KiB of LDS, so
                                       wgrad_tiling_octo never refuses 4 k-steps and wgrad_plan_one never falls back to 2

ROW4 is a WgradGeometry written out by hand (one row of the stem's taps as a kernel of its own): the atomics path with accumulate = 0
needs a 4-tap problem that is no tap group, and conv_geometry builds 4-tap problems as tap groups only."""
import ctypes as C
from collections import namedtuple

import hrpe_amd  # noqa: F401
from hrpe_amd import _native as nv
from hrpe_amd import conv_geometry as G

DT = {"bf16": nv.HRP_BF16, "f32": nv.HRP_F32, "f32x3": nv.HRP_F32X3}
W1, W3, W3S2, W1S2, W3D2 = G.wgrad(1), G.wgrad(3), G.wgrad(3, 2), G.wgrad(1, 2), G.wgrad(3, 1, 2)
DECONV = G.wgrad_groups(G.TAPS4_DECONV, 2)      # the 4x4 stride-2 transposed layer: x is the LARGE map
STEM = G.wgrad_groups(G.TAPS4_STEM, 1)          # the 7x7 stride-2 stem on the space-to-depth image
COST_CAP = 3 * 10 ** 9
FIELDS = ("program", "arrange", "nks", "BM", "TI", "TH", "TW", "ring", "xmode", "G", "ntiles", "pairs", "use_ws")
Config = namedtuple("Config", FIELDS)


class Prob(namedtuple("Prob", "geo dt N H W Cc Cout x_pitch dy_pitch split")):
    """One weight-gradient problem.  H x W: the layer input; Cc: its real channels (= dw_cin; Cin is Cc rounded up to a 16-byte
    vector); split: the operand ("x" / "dy") drawn from the integers that are no bf16 numbers (fp32, fp32x3)."""
    __slots__ = ()
    Ho = property(lambda s: (s.H - 1) // s.geo.in_stride + 1)
    Wo = property(lambda s: (s.W - 1) // s.geo.in_stride + 1)
    Cin = property(lambda s: G.rup(s.Cc, G.ELEM[DT[s.dt]][1]))
    dw_cin = property(lambda s: s.Cc)
    ntaps = property(lambda s: len(s.geo.taps))
    T = property(lambda s: s.geo.dw_tap_stride or len(s.geo.taps))
    pixels = property(lambda s: s.N * s.Ho * s.Wo)
    cost = property(lambda s: s.pixels * s.Cin * s.Cout * s.ntaps)


def P(geo, dt, N, H, W, Cc, Cout, x_pitch=0, dy_pitch=0, split="x"):
    vec = G.ELEM[DT[dt]][1]
    return Prob(geo, dt, N, H, W, Cc, Cout, x_pitch or G.rup(Cc, vec), dy_pitch or G.rup(Cout, vec), split)


def fill(p, x_ptr, dy_ptr, dw_ptr, accumulate, phase=0):
    """The problem's descriptor, by the function the plans fill theirs with."""
    g = G.fill_wgrad(p.geo, G.Operand(x_ptr, p.N, p.H, p.W, p.Cc, p.x_pitch), G.Operand(dy_ptr, p.N, p.Ho, p.Wo, p.Cout, p.dy_pitch),
                     dw_ptr, p.dw_cin, DT[p.dt], accumulate)
    g.phase = phase
    return g


def config_of(g):
    """hrp_wgrad_config_of as a Config; an invalid problem raises nv.HrpError with the launcher's message."""
    c = nv.WgradConfig()
    nv.check(nv.lib().hrp_wgrad_config_of(C.byref(g), C.byref(c)), "hrp_wgrad_config_of")
    return Config(*[getattr(c, f) for f in FIELDS])


def prepare_batch(descs, alloc):
    """Size query, workspaces from alloc(i, bytes) -> address, prepare.  -> (descriptor array, info, host table, [Config])."""
    L = nv.lib()
    n = len(descs)
    arr = (nv.WgradDesc * n)(*descs)
    info = nv.BatchInfo()
    nv.check(L.hrp_batch_prepare(nv.BATCH_WGRAD, arr, n, None, C.byref(info)), "hrp_batch_prepare (size query)")
    for i in range(n):
        arr[i].workspace, arr[i].workspace_bytes = alloc(i, int(info.ws_bytes[i])), int(info.ws_bytes[i])
    host = (C.c_char * int(L.hrp_batch_table_bytes(nv.BATCH_WGRAD, n)))()
    nv.check(L.hrp_batch_prepare(nv.BATCH_WGRAD, arr, n, host, C.byref(info)), "hrp_batch_prepare")
    cfgs = (nv.WgradConfig * n)()
    nv.check(L.hrp_batch_wgrad_configs(host, C.byref(info), cfgs), "hrp_batch_wgrad_configs")
    return arr, info, host, [Config(*[getattr(c, f) for f in FIELDS]) for c in cfgs]


def host_single(p, ws=True, accumulate=0):
    """What a single launch of p runs, asked with made-up addresses (the query is host code)."""
    g = fill(p, 0x100000, 0x200000, 0x300000, accumulate)
    if ws:
        g.workspace, g.workspace_bytes = 0x40000000, int(nv.lib().hrp_wgrad_workspace_bytes(C.byref(g)))
    return config_of(g)


def host_batch(probs):
    descs = [fill(p, 0x100000, 0x200000, 0x300000 + 0x100000 * i, 0) for i, p in enumerate(probs)]
    return prepare_batch(descs, lambda i, b: 0x40000000 + 0x4000000 * i)[3]


def tiles_per_workgroup(c):
    """Workgroup g of G walks the tiles g, g + G, ..: the set of tile counts of a problem's workgroups."""
    return {(c.ntiles - 1 - g) // c.G + 1 for g in range(c.G)}


# ---- the table ------------------------------------------------------------------------------------------------------------------------
# paths: S-ws / S-ws1 single launch with workspace (accumulate 0 / 1), S-atom0 / S-atom1 without, S-ph1 phase 1 + fold launch,
# B batched, B-ph1 batched phase 1 + fold launch.  companions: the other problems of the batch (B paths); shared: the case's problems
# are the tap groups of ONE dw - S paths launch them in sequence, B paths in one batch - otherwise S paths launch `prob` alone.
Case = namedtuple("Case", "name prob paths companions shared", defaults=((), False))
S_ALL = ("S-ws", "S-atom0", "S-atom1", "S-ph1", "B", "B-ph1")
SB = ("S-ws", "B")
ATOMS = ("S-atom0", "S-atom1")
GROUP = ("S-ws", "S-atom1", "B")
ROW4 = G.WgradGeometry(1, G.TAPS4_STEM[4:8])        # a 4-tap kernel of its own (no tap group): the only 4-tap form that may overwrite without a workspace


def _four_wave(dt, tag, geos, ch1, chn, split):
    """The small / ragged shapes of one element type for 1, 4 and 9 taps: 1 x 8 x 8 and 2 x 8 x 8 (64- and 128-pixel tiles), the ragged
    3 x 13 x 9 with a partly empty second input block, Cout = 17 and both pitches padded, and five 1 x 1 images (fp32: the 16-pixel tile)."""
    out = []
    for nt, geo in geos:
        sp = split if nt != 4 else ("dy" if split == "x" else "x")
        (c1, o1), (c2, o2) = (ch1, chn) if nt != 9 or dt != "bf16" else ((40, 17), (32, 64))     # (bf16 3x3 32 -> 32: the eight-wave program in a batch)
        out += [Case(f"{tag}{nt}_1x8x8", P(geo, dt, 1, 8, 8, c1, o1, split=sp), S_ALL if nt == 9 else SB + ATOMS[1:] if nt == 4 else SB + ATOMS),
                Case(f"{tag}{nt}_2x8x8", P(geo, dt, 2, 8, 8, c2, o2, split=sp), SB),
                Case(f"{tag}{nt}_3x13x9", P(geo, dt, 3, 13, 9, 40, 17, x_pitch=48, dy_pitch=24, split=sp), SB + ({1: "S-ws1", 4: "S-ph1", 9: "B-ph1"}[nt],))]
        if dt == "f32" or (dt, nt) == ("bf16", 9):          # 1 x 1 images; fp32: the 16-pixel tile
            out.append(Case(f"{tag}{nt}_5x1x1", P(geo, dt, 5, 1, 1, c1, o1, split=sp), SB))
    return out


def _groups(tag, geos, dt, N, H, W, Cc, Cout, **kw):
    """A 16-tap kernel as its four tap groups: each alone, then all four into one dw."""
    ps = [P(g, dt, N, H, W, Cc, Cout, **kw) for g in geos]
    return [Case(f"{tag}_g{i}", p, GROUP) for i, p in enumerate(ps)] + [Case(f"{tag}_all", ps[0], GROUP, tuple(ps[1:]), True)]


def _heavy(geo, dt):
    return P(geo, dt, 2, 32, 32, 128, 160)       # outweighs a 99-pixel problem by more than 256 x its pixels: that one gets G = 1


TABLE = (
    _four_wave("bf16", "b", ((1, W1), (4, STEM[2]), (9, W3)), (32, 32), (32, 32), "x")
    + _four_wave("f32", "f", ((1, W1), (4, STEM[1]), (9, W3)), (32, 32), (32, 32), "x")
    + _four_wave("f32x3", "x", ((1, W1), (4, STEM[3]), (9, W3)), (32, 32), (32, 32), "dy")
    + [
        # 4-tap kernels of their own: the atomics path with accumulate = 0
        Case("b4_row", P(ROW4, "bf16", 1, 8, 8, 32, 32), ATOMS),
        Case("f4_row", P(ROW4, "f32", 1, 8, 8, 32, 32, split="dy"), ATOMS),
        Case("x4_row", P(ROW4, "f32x3", 1, 8, 8, 32, 32), ATOMS),
        # 64 x 64 blocks of the bf16 1x1 layers (NB = 2), Cout = 72: the second output block holds 8 rows
        Case("b1n2_1x8x8", P(W1, "bf16", 1, 8, 8, 64, 72), SB + ATOMS),
        Case("b1n2_2x8x8", P(W1, "bf16", 2, 8, 8, 64, 72), SB),
        Case("b1n2_3x13x9", P(W1, "bf16", 3, 13, 9, 64, 72, x_pitch=72, dy_pitch=80), ("S-ws", "S-ph1", "B", "B-ph1")),
        # stride 2 with odd H and W (17 x 22 -> 9 x 11), 1x1 stride 2, dilation 2, one- and two-row images, N no multiple of TI
        Case("b9_s2", P(W3S2, "bf16", 2, 17, 22, 32, 64), SB + ("S-atom1",)),
        Case("f9_s2", P(W3S2, "f32", 2, 17, 22, 32, 64, split="dy"), SB),
        Case("x9_s2", P(W3S2, "f32x3", 2, 17, 22, 32, 64), SB),
        Case("b1_s2", P(W1S2, "bf16", 2, 17, 22, 32, 64), SB),
        Case("f1_s2", P(W1S2, "f32", 1, 17, 22, 40, 17, x_pitch=44, dy_pitch=20), SB),
        Case("b9_d2", P(W3D2, "bf16", 2, 16, 20, 32, 64), SB),
        Case("x9_d2", P(W3D2, "f32x3", 2, 16, 20, 32, 64, split="dy"), SB),
        Case("b9_h1", P(W3, "bf16", 3, 1, 20, 32, 64), SB),
        Case("f9_h2", P(W3, "f32", 3, 2, 9, 32, 32), SB),
        Case("b9_n3ti2", P(W3, "bf16", 3, 8, 8, 40, 17), SB),
        Case("x1_n5ti2", P(W1, "f32x3", 5, 8, 8, 32, 32), SB),
        # the fold's slab loop: G = 33, 32, 6 (and the 1, 2 and 3 of the cases above)
        Case("b9_G33", P(W3, "bf16", 33, 16, 16, 32, 32), ("S-ws", "S-ph1")),
        Case("b4_G32", P(DECONV[1], "bf16", 8, 32, 32, 32, 32), SB),
        Case("f1_G35", P(W1, "f32", 35, 8, 16, 32, 32), ("S-ws",)),
        Case("b1_G8x2", P(W1, "bf16", 8, 16, 16, 32, 32), SB),                       # in a batch: XCD-aware numbering (xmode 2)
        Case("x9_uneven", P(W3, "f32x3", 5, 16, 16, 32, 64), ("B",)),                # in a batch: 10 tiles on 8 workgroups
        Case("b4_uneven", P(DECONV[1], "bf16", 3, 26, 18, 40, 17), SB),              # in a batch: 12 tiles on 8 workgroups
    ]
    # the 7x7 stem on the space-to-depth image (12 real channels in 16) and the 4x4 stride-2 transposed layer
    + _groups("stem_b", STEM, "bf16", 2, 13, 9, 12, 40)
    + _groups("stem_f", STEM, "f32", 1, 13, 9, 10, 17, dy_pitch=20)
    + _groups("deconv_x", DECONV, "f32x3", 2, 16, 12, 32, 24, split="dy")
    + [
        # tiles per workgroup of the four-wave program: next to the heavy problem the others get G = 1 (2 and 3 tiles)
        Case("b9_steer", _heavy(W3, "bf16"), ("B", "B-ph1"), (P(W3S2, "bf16", 1, 15, 22, 32, 64), P(W3S2, "bf16", 1, 17, 22, 32, 64))),
        Case("f1_steer", _heavy(W1, "f32"), ("B", "B-ph1"), (P(W1S2, "f32", 1, 15, 22, 32, 64, split="dy"), P(W1S2, "f32", 1, 17, 22, 32, 64))),
        Case("x4_steer", _heavy(STEM[1], "f32x3"), ("B", "B-ph1"),
             (P(DECONV[1], "f32x3", 1, 15, 22, 32, 64, split="dy"), P(DECONV[1], "f32x3", 1, 17, 22, 32, 64))),
        # the eight-wave programs
        Case("octo_b", P(W3, "bf16", 12, 32, 32, 128, 128), ("B", "B-ph1"),
             (P(W3S2, "bf16", 2, 16, 16, 64, 64), P(W3S2, "bf16", 3, 16, 16, 64, 64), P(W3, "bf16", 5, 8, 8, 64, 64),
              P(W3, "bf16", 3, 32, 1, 64, 64), P(W3, "bf16", 2, 32, 32, 32, 32), P(W3S2, "bf16", 1, 32, 32, 64, 128))),
        Case("octo_x9", P(W3, "f32x3", 6, 32, 32, 128, 128), ("B", "B-ph1"),
             (P(W3, "f32x3", 3, 32, 1, 64, 64, split="dy"), P(W3, "f32x3", 6, 32, 1, 64, 64), P(W3S2, "f32x3", 2, 16, 16, 64, 64, split="dy"),
              P(W3S2, "f32x3", 3, 16, 16, 64, 64), P(W3, "f32x3", 5, 8, 8, 64, 64, split="dy"))),
        Case("octo_x1", P(W1, "f32x3", 6, 32, 32, 128, 128, split="dy"), ("B", "B-ph1"),
             (P(W1, "f32x3", 2, 16, 16, 64, 64), P(W1, "f32x3", 5, 8, 8, 64, 64, split="dy"), P(W1, "f32x3", 3, 16, 16, 256, 64))),
    ]
)
TABLE = tuple(TABLE)


# What the launcher's query answered for every case when the table was written, as Config without use_ws: (program, arrange, nks, BM,
# TI, TH, TW, ring, xmode, G, ntiles, pairs).  EXPECT_S: a single launch of each of the case's problems.  EXPECT_B: the batch, per
# problem, where it differs from the single launch (XCD-aware numbering, the eight-wave programs, a steered G).
EXPECT_S = {
    "b1_1x8x8": (0, 1, 1, 64, 1, 8, 8, 0, 0, 1, 1, 1), "b1_2x8x8": (0, 1, 2, 128, 2, 8, 8, 0, 0, 1, 1, 1), "b1_3x13x9": (0, 1, 4, 256, 1, 16, 16, 0, 0, 3, 3, 2),
    "b4_1x8x8": (0, 1, 1, 64, 1, 8, 8, 0, 0, 1, 1, 1), "b4_2x8x8": (0, 1, 2, 128, 2, 8, 8, 0, 0, 1, 1, 1), "b4_3x13x9": (0, 1, 4, 256, 1, 16, 16, 0, 0, 3, 3, 2),
    "b9_1x8x8": (0, 1, 1, 64, 1, 8, 8, 0, 0, 1, 1, 2), "b9_2x8x8": (0, 1, 2, 128, 2, 8, 8, 0, 0, 1, 1, 2), "b9_3x13x9": (0, 1, 4, 256, 1, 16, 16, 0, 0, 3, 3, 2),
    "b9_5x1x1": (0, 1, 1, 64, 5, 1, 1, 0, 0, 1, 1, 2),
    "f1_1x8x8": (0, 1, 0, 64, 1, 8, 8, 0, 0, 1, 1, 1), "f1_2x8x8": (0, 1, 0, 128, 2, 8, 8, 0, 0, 1, 1, 1), "f1_3x13x9": (0, 1, 0, 128, 1, 8, 16, 0, 0, 6, 6, 2),
    "f1_5x1x1": (0, 1, 0, 16, 5, 1, 1, 0, 0, 1, 1, 1),
    "f4_1x8x8": (0, 1, 0, 64, 1, 8, 8, 0, 0, 1, 1, 1), "f4_2x8x8": (0, 1, 0, 128, 1, 8, 8, 0, 0, 2, 2, 1), "f4_3x13x9": (0, 1, 0, 128, 1, 8, 16, 0, 0, 6, 6, 2),
    "f4_5x1x1": (0, 1, 0, 16, 5, 1, 1, 0, 0, 1, 1, 1),
    "f9_1x8x8": (0, 1, 0, 64, 1, 8, 8, 0, 0, 1, 1, 1), "f9_2x8x8": (0, 1, 0, 128, 1, 8, 8, 0, 0, 2, 2, 1), "f9_3x13x9": (0, 1, 0, 128, 1, 8, 16, 0, 0, 6, 6, 2),
    "f9_5x1x1": (0, 1, 0, 16, 5, 1, 1, 0, 0, 1, 1, 1),
    "x1_1x8x8": (0, 1, 1, 64, 1, 8, 8, 0, 0, 1, 1, 1), "x1_2x8x8": (0, 1, 2, 128, 2, 8, 8, 0, 0, 1, 1, 1), "x1_3x13x9": (0, 1, 2, 128, 1, 8, 16, 0, 0, 6, 6, 2),
    "x4_1x8x8": (0, 1, 1, 64, 1, 8, 8, 0, 0, 1, 1, 1), "x4_2x8x8": (0, 1, 2, 128, 1, 8, 8, 0, 0, 2, 2, 1), "x4_3x13x9": (0, 1, 2, 128, 1, 8, 16, 0, 0, 6, 6, 2),
    "x9_1x8x8": (0, 1, 1, 64, 1, 8, 8, 0, 0, 1, 1, 1), "x9_2x8x8": (0, 1, 2, 128, 1, 8, 8, 0, 0, 2, 2, 1), "x9_3x13x9": (0, 1, 2, 128, 1, 8, 16, 0, 0, 6, 6, 2),
    "b4_row": (0, 1, 1, 64, 1, 8, 8, 0, 0, 1, 1, 1), "f4_row": (0, 1, 0, 64, 1, 8, 8, 0, 0, 1, 1, 1), "x4_row": (0, 1, 1, 64, 1, 8, 8, 0, 0, 1, 1, 1),
    "b1n2_1x8x8": (0, 2, 1, 64, 1, 8, 8, 0, 0, 1, 1, 2), "b1n2_2x8x8": (0, 2, 2, 128, 2, 8, 8, 0, 0, 1, 1, 2), "b1n2_3x13x9": (0, 2, 2, 128, 1, 8, 16, 0, 0, 6, 6, 2),
    "b9_s2": (0, 1, 1, 64, 1, 4, 16, 0, 0, 6, 6, 2), "f9_s2": (0, 1, 0, 32, 1, 2, 16, 0, 0, 10, 10, 2), "x9_s2": (0, 1, 1, 64, 1, 4, 16, 0, 0, 6, 6, 2),
    "b1_s2": (0, 1, 2, 128, 1, 8, 16, 0, 0, 4, 4, 2), "f1_s2": (0, 1, 0, 64, 1, 4, 16, 0, 0, 3, 3, 2),
    "b9_d2": (0, 1, 2, 128, 1, 8, 16, 0, 0, 8, 8, 2), "x9_d2": (0, 1, 1, 64, 1, 4, 16, 0, 0, 16, 16, 2),
    "b9_h1": (0, 1, 1, 64, 3, 1, 16, 0, 0, 2, 2, 2), "f9_h2": (0, 1, 0, 32, 1, 2, 16, 0, 0, 3, 3, 1),
    "b9_n3ti2": (0, 1, 2, 128, 2, 8, 8, 0, 0, 2, 2, 2), "x1_n5ti2": (0, 1, 2, 128, 2, 8, 8, 0, 0, 3, 3, 1),
    "b9_G33": (0, 1, 4, 256, 1, 16, 16, 0, 0, 33, 33, 1), "b4_G32": (0, 1, 1, 64, 1, 4, 16, 0, 0, 32, 32, 1), "f1_G35": (0, 1, 0, 128, 1, 8, 16, 0, 0, 35, 35, 1),
    "b1_G8x2": (0, 1, 4, 256, 1, 16, 16, 0, 0, 8, 8, 1), "b4_uneven": (0, 1, 1, 64, 1, 4, 16, 0, 0, 12, 12, 2),
    **{f"stem_b_{k}": (0, 1, 2, 128, 1, 8, 16, 0, 0, 4, 4, 2) for k in ("g0", "g1", "g2", "g3", "all")},
    **{f"stem_f_{k}": (0, 1, 0, 64, 1, 4, 16, 0, 0, 4, 4, 1) for k in ("g0", "g1", "g2", "g3", "all")},
    **{f"deconv_x_{k}": (0, 1, 1, 64, 1, 8, 8, 0, 0, 2, 2, 1) for k in ("g0", "g1", "g2", "g3", "all")},
}
EXPECT_B = {
    "f9_s2": [(0, 1, 0, 32, 1, 2, 16, 0, 2, 8, 10, 2)],
    "b9_d2": [(0, 1, 2, 128, 1, 8, 16, 0, 2, 8, 8, 2)], "x9_d2": [(0, 1, 1, 64, 1, 4, 16, 0, 2, 16, 16, 2)],
    "b4_G32": [(0, 1, 1, 64, 1, 4, 16, 0, 2, 32, 32, 1)], "b1_G8x2": [(0, 1, 4, 256, 1, 16, 16, 0, 2, 8, 8, 1)],
    "x9_uneven": [(0, 1, 2, 128, 1, 8, 16, 0, 2, 8, 10, 2)], "b4_uneven": [(0, 1, 1, 64, 1, 4, 16, 0, 2, 8, 12, 2)],
    "b9_steer": [(0, 1, 4, 256, 1, 16, 16, 0, 0, 8, 8, 20), (0, 1, 1, 64, 1, 4, 16, 0, 0, 1, 2, 2), (0, 1, 1, 64, 1, 4, 16, 0, 0, 1, 3, 2)],
    "f1_steer": [(0, 1, 0, 128, 1, 8, 16, 0, 0, 16, 16, 20), (0, 1, 0, 64, 1, 4, 16, 0, 0, 1, 2, 2), (0, 1, 0, 64, 1, 4, 16, 0, 0, 1, 3, 2)],
    "x4_steer": [(0, 1, 2, 128, 1, 8, 16, 0, 0, 16, 16, 20), (0, 1, 1, 64, 1, 4, 16, 0, 0, 1, 2, 2), (0, 1, 1, 64, 1, 4, 16, 0, 0, 1, 3, 2)],
    "octo_b": [(1, 4, 4, 128, 1, 8, 16, 3, 2, 56, 96, 4), (1, 4, 2, 64, 1, 8, 8, 3, 0, 1, 2, 1), (1, 4, 2, 64, 1, 8, 8, 3, 0, 1, 3, 1),
               (1, 4, 4, 128, 2, 8, 8, 3, 0, 2, 3, 1), (1, 4, 4, 128, 3, 32, 1, 2, 0, 1, 1, 1), (1, 1, 4, 512, 1, 32, 16, 2, 0, 3, 4, 1),
               (1, 4, 2, 64, 1, 4, 16, 3, 0, 1, 4, 2)],
    "octo_x9": [(2, 4, 4, 128, 1, 8, 16, 0, 2, 48, 48, 4), (2, 4, 2, 64, 2, 32, 1, 0, 0, 1, 2, 1), (2, 4, 2, 64, 2, 32, 1, 0, 0, 2, 3, 1),
                (2, 4, 1, 32, 1, 4, 8, 0, 0, 1, 4, 1), (2, 4, 1, 32, 1, 4, 8, 0, 0, 2, 6, 1), (2, 4, 2, 64, 1, 8, 8, 0, 0, 3, 5, 1)],
    "octo_x1": [(2, 4, 4, 128, 1, 8, 16, 0, 2, 48, 48, 4), (2, 4, 4, 128, 1, 8, 16, 0, 0, 4, 4, 1), (2, 4, 4, 128, 2, 8, 8, 0, 0, 3, 3, 1),
                (2, 4, 4, 128, 1, 8, 16, 0, 0, 6, 6, 4)],
}


def expected(case, path):
    """One Config per problem the path launches."""
    n = len(problems(case, path))
    rows = EXPECT_B[case.name] if path.startswith("B") and case.name in EXPECT_B else [EXPECT_S[case.name]] * n
    assert len(rows) == n, case.name
    return [Config(*r, use_ws=0 if path.startswith("S-atom") else 1) for r in rows]


def problems(case, path):
    """The problems a path of a case launches."""
    return (case.prob,) + tuple(case.companions) if case.shared or path.startswith("B") else (case.prob,)


def host_configs(case, path):
    """What the path's launches will run, asked on the host: one Config per problem."""
    ps = problems(case, path)
    if path.startswith("B"):
        return host_batch(ps)
    return [host_single(p, ws=not path.startswith("S-atom"), accumulate=int(path in ("S-ws1", "S-atom1"))) for p in ps]


def gpu_cases():
    return [(c, path) for c in TABLE for path in c.paths]
