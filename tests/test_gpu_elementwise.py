"""hrp_ew_fwd / hrp_ew_bwd_reduce / hrp_ew_bwd_apply / hrp_ew_pool2, the three HRP_BATCH_EW_* families (csrc/elementwise.hip)
and the BatchNorm table kernels (csrc/core.hip) against the float64 oracle of tests/ew_oracle.py (itself proved against
autograd in test_elementwise_host.py).

1. EXACT tests: integers in [-8, 8], modes IDENTITY / AFFINE(1, 0), every fp32 sum below 2^24 -> the kernels must equal the
   oracle bit for bit; every written buffer has a pitch > C, guard rows and a sentinel fill, and nothing outside [pixels][0:C]
   may change.  The case names say which branch of geom() / the launchers (elementwise.hip) they reach:
     geom(): V = VEC (8 bf16 / 4 fp32) when C % VEC == 0 and every pointer / pitch is 16-byte aligned, else 1; tpr = the power of
     two >= C / V, at most 512 / VEC (vector) or 256 (scalar); nslab = ceil(C / V / tpr); ppb = 256 / tpr pixels per block and
     step; gx = min(ceil(pixels / ppb), cap / nslab), cap = 256 (forward with nin <= 2 and no upsampling, reduce, apply at
     up == 1), 1024 (other forwards, apply at up > 1), 512 (reduce at up > 1); one grid step covers S = gx * ppb pixels and the four-pixel
     trips need more than 3 S pixels.
   LeakyReLU: slope * integer is one fp32 rounding, so outputs and up == 1 gradients stay exact; SUMS of such terms are not, so
   the LeakyReLU reduce is held to the summation bound n * 2^-24 * sum |terms| (n terms per channel) instead.
2. ARITHMETIC tests: real data, BN_TRAIN statistics spread over the 8 slots.  Bound = 8 x the fp32 noise floor (deviation of
   the fp32 restatement from float64 relative to the tensor's scale, never below one fp32 rounding 2^-24), + 2^-8 |ref| for
   bf16 outputs.  Floors measured on the CPU: 0.6e-7 .. 3.2e-7 of scale for every |mean| / std <= 2 case (pre-activation,
   sums, din, dgamma, dbeta; 1.8e-6 for the 257-channel fp32 pre-activation), 6.5e-5 for |mean| / std = 30 (E[x^2] - mean^2
   cancels).  Device deviations: printed by every arithmetic test (pytest -s); DESIGN.md 4.1 keeps the list.
3. REFUSALS: bad descriptors return non-zero, set hrp_last_error and write nothing."""
import ctypes as C

import pytest
import torch

import hrpe_amd  # noqa: F401
from hrpe_amd import _native as nv

import ew_oracle as O
from ew_oracle import AFFINE, BN_TRAIN, F64, IDENTITY, Buf

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF, F32 = torch.bfloat16, torch.float32
DT = {BF: nv.HRP_BF16, F32: nv.HRP_F32}
TN = {BF: "bf16", F32: "f32"}
ID, AF = IDENTITY, AFFINE


def rint(gen, shape):
    return torch.randint(-8, 9, shape, generator=gen).to(F64)


def rounded(v, tdt):
    """float64 -> the element type through fp32, as the device converts."""
    return v.to(torch.float32).to(tdt)


class Prob:
    """One forward problem on the device + its oracle.  ins: ((up, mode), ..); mis = (operand, 'pitch' | 'ptr'): the one
    misaligned operand ('in0'.., 'out', 'dout', 'din', 'din2').  inputs: real-valued OIn list instead of integers."""

    def __init__(self, tdt, N, H, W, Cn, ins=((1, ID),), relu=1, mask=True, mis=None, seed=0, inputs=None, consts_out=False):
        self.tdt, self.shape, self.relu, self.mis, self.vec = tdt, (N, H, W, Cn), relu, mis, O.VEC[tdt]
        self.gen = gen = torch.Generator().manual_seed(seed)
        one, zero = torch.ones(Cn), torch.zeros(Cn)
        if inputs is None:
            inputs = [O.OIn(rint(gen, (N, H // up, W // up, Cn)), up, mode, *((one, zero) if mode == AF else ())) for up, mode in ins]
        self.inputs, self.keep = inputs, []
        fwd_mis = mis is not None and (mis[0] == "out" or mis[0].startswith("in"))
        self.vector = Cn % self.vec == 0 and not fwd_mis
        self.pre, self.ref_out, self.ref_bits = O.ew_forward(inputs, relu, self.vec)
        self.inb = [self.buf(f"in{j}", inp.x.shape[0] * inp.x.shape[1] * inp.x.shape[2]).put(inp.x) for j, inp in enumerate(inputs)]
        self.out = self.buf("out", N * H * W)
        nb = -(-Cn // self.vec)
        self.maskb = Buf(N * H * W, nb, nb + 3, torch.uint8, DEV) if mask and relu and self.vector else None
        d = self.desc = nv.EwDesc()
        d.nin, d.out, d.out_pitch, d.dtype = len(inputs), self.out.ptr, self.out.pitch, DT[tdt]
        d.N, d.H, d.W, d.C, d.relu = N, H, W, Cn, relu
        if self.maskb is not None:
            d.mask, d.mask_pitch = self.maskb.ptr, self.maskb.pitch
        for j, inp in enumerate(inputs):
            O.fill_input(d.inp[j], inp, self.inb[j], self.keep, DEV)
        self.consts = None
        if consts_out:
            self.consts = torch.full((2 * Cn + 8,), O.FSENT, dtype=F32, device=DEV)
            d.consts_out = self.consts.data_ptr()
        self.dout = self.dout_ref = None

    def buf(self, name, rows, Cn=None, tdt=None):
        Cn = self.shape[3] if Cn is None else Cn
        pitch = -(-Cn // self.vec) * self.vec + 2 * self.vec
        bad = self.mis is not None and self.mis[0] == name
        return Buf(rows, Cn, pitch + (1 if bad and self.mis[1] == "pitch" else 0), tdt or self.tdt, DEV,
                   offset=1 if bad and self.mis[1] == "ptr" else 0)

    def launch(self):
        nv.call("hrp_ew_fwd", C.byref(self.desc), None)
        torch.cuda.synchronize()
        return self

    def check_exact(self, what=""):
        N, H, W, Cn = self.shape
        got = self.out.get()
        want = rounded(self.ref_out, self.tdt).reshape(-1, Cn)
        bad = (got != want).nonzero()
        assert bad.numel() == 0, f"{what}: out differs at (pixel, channel) {bad[:4].tolist()} of {bad.shape[0]}"
        assert self.out.outside_untouched(), f"{what}: out written outside [pixels][0:C]"
        if self.maskb is not None:
            assert torch.equal(self.maskb.get(), self.ref_bits.reshape(N * H * W, -1)), f"{what}: mask bits"
            assert self.maskb.outside_untouched(), f"{what}: mask written outside [pixels][0:C/VEC]"

    def make_dout(self, real=False):
        N, H, W, Cn = self.shape
        self.dout_ref = rounded(torch.randn(self.shape, generator=self.gen, dtype=F64), self.tdt).to(F64) if real else rint(self.gen, self.shape)
        self.dout = self.buf("dout", N * H * W).put(self.dout_ref)

    def pooled_level(self, k):
        """k applications of hrp_ew_pool2 to (dout, mask): the first in the plan type with the bits, the rest in fp32; each level
        is compared with the oracle."""
        N, H, W, Cn = self.shape
        src, ref, pos = self.dout, self.dout_ref, self.pre > 0
        for lvl in range(k):
            h, w = H >> lvl, W >> lvl
            dst = Buf(N * (h // 2) * (w // 2), Cn, Cn, F32, DEV)
            rc = nv.lib().hrp_ew_pool2(src.ptr, DT[self.tdt] if lvl == 0 else nv.HRP_F32, src.pitch, self.maskb.ptr if lvl == 0 else None,
                                       self.maskb.pitch if lvl == 0 else 0, N, h, w, Cn, dst.ptr, None)
            assert rc == 0, nv.lib().hrp_last_error()
            torch.cuda.synchronize()
            ref = O.pool2(ref, pos if lvl == 0 else None)
            assert torch.equal(dst.get(), ref.float().reshape(-1, Cn)) and dst.outside_untouched(), f"pool2 level {lvl + 1}"
            src, pos = dst, None
        self.keep.append(src)
        return src, ref


class Bwd:
    """Backward of input j of a forward problem.  how: 'mask' | 'out' | 'none' (relu == 0) | 'pooled'."""

    def __init__(self, P, j, how, acc=0, din2=None, null_in=False, pos=None):
        self.P, self.j, self.how = P, j, how
        N, H, W, Cn = P.shape
        inp = self.inp = P.inputs[j]
        up = inp.up
        rows = N * (H // up) * (W // up)
        ishape = (N, H // up, W // up, Cn)
        if P.dout is None:
            P.make_dout()
        self.din = P.buf("din", rows)
        self.din_old = self.din2_old = None
        if acc:
            self.din_old = rint(P.gen, ishape)
            self.din.put(self.din_old)
        self.din2 = None
        if din2 is not None:
            self.din2 = P.buf("din2", rows)
            if din2:
                self.din2_old = rint(P.gen, ishape)
                self.din2.put(self.din2_old)
        self.sums0 = torch.zeros(O.SLOTS * 2 * Cn + 16, dtype=F64)
        self.sums0[:O.SLOTS * 2 * Cn] = rint(P.gen, (O.SLOTS * 2 * Cn,))       # the reduce ADDS to what the slots hold
        self.sums = self.sums0.clone().to(DEV)
        d = self.desc = nv.EwBwdDesc()
        d.dout, d.dout_pitch, d.dtype = P.dout.ptr, P.dout.pitch, DT[P.tdt]
        d.N, d.H, d.W, d.C, d.relu, d.accumulate = N, H, W, Cn, P.relu, acc
        if P.relu:
            d.out, d.out_pitch = P.out.ptr, P.out.pitch
        if how in ("mask", "pooled"):
            d.mask, d.mask_pitch = P.maskb.ptr, P.maskb.pitch
        O.fill_input(d.inp, inp, None if null_in else P.inb[j], P.keep, DEV)
        d.din, d.din_pitch, d.sums = self.din.ptr, self.din.pitch, self.sums.data_ptr()
        if self.din2 is not None:
            d.din2, d.din2_pitch, d.accumulate2 = self.din2.ptr, self.din2.pitch, 1 if din2 else 0
        g = None
        if P.relu == 2:      # slope * dOut is an fp32 product on the device: round it before it is added to anything
            g = O.window_sum(O.masked_grad(P.dout_ref, P.pre > 0, 2).float().to(F64), up)
        if how == "pooled":
            pb, g = P.pooled_level(up.bit_length() - 1)
            d.pooled = pb.ptr
        self.ref = O.ew_backward(P.dout_ref, (P.pre > 0) if pos is None else pos, inp, P.relu, din_old=self.din_old, din2_old=self.din2_old, g=g)

    def reduce(self):
        nv.call("hrp_ew_bwd_reduce", C.byref(self.desc), None)
        torch.cuda.synchronize()
        return self

    def apply(self):
        nv.call("hrp_ew_bwd_apply", C.byref(self.desc), None)
        torch.cuda.synchronize()
        return self

    def got_sums(self):
        Cn = self.P.shape[3]
        s = self.sums.cpu()
        assert torch.equal(s[O.SLOTS * 2 * Cn:], self.sums0[O.SLOTS * 2 * Cn:]), "reduce wrote past [SLOTS][2C]"
        return (s - self.sums0)[:O.SLOTS * 2 * Cn].view(O.SLOTS, 2 * Cn).sum(0)

    def check_reduce(self, what=""):
        got, want = self.got_sums(), self.ref["sums"]
        if self.P.relu == 2:
            # sums of slope * integer terms round: n terms per channel, |error| <= n * 2^-24 * sum |terms| (recursive summation)
            N, H, W, Cn = self.P.shape
            g = O.masked_grad(self.P.dout_ref, self.P.pre > 0, 2).abs()
            x = O.upsample(self.inp.x, self.inp.up).abs()
            bound = N * H * W * 2.0 ** -24 * torch.cat([g.sum((0, 1, 2)), (g * x).sum((0, 1, 2))])
            assert bool(((got - want).abs() <= bound).all()), f"{what}: LeakyReLU sums off by {(got - want).abs().max()}"
            return
        bad = (got != want).nonzero()
        assert bad.numel() == 0, f"{what}: sums differ at {bad[:4].flatten().tolist()}: {got[bad[:4].flatten()].tolist()} != {want[bad[:4].flatten()].tolist()}"

    def check_apply(self, what=""):
        Cn = self.P.shape[3]
        for name, b in (("din", self.din), ("din2", self.din2)):
            if b is None:
                continue
            bad = (b.get() != rounded(self.ref[name], self.P.tdt).reshape(-1, Cn)).nonzero()
            assert bad.numel() == 0, f"{what}: {name} differs at (pixel, channel) {bad[:4].tolist()} of {bad.shape[0]}"
            assert b.outside_untouched(), f"{what}: {name} written outside [pixels][0:C]"


def run_chain(tdt, N, H, W, Cn, ins, relu=1, how="mask", acc=0, din2=None, mis=None, null_in=False, js=None):
    """forward, then reduce + apply of the inputs js (default: all), everything exact."""
    P = Prob(tdt, N, H, W, Cn, ins, relu, mask=how in ("mask", "pooled"), mis=mis, seed=N * 7 + H * 5 + W * 3 + Cn).launch()
    P.check_exact("forward")
    if not P.vector and how == "mask":
        how = "out"
    if mis is not None and relu:
        how = "out"          # a misaligned backward operand puts reduce / apply on the scalar path: no bit mask there
    for j in (range(len(ins)) if js is None else js):
        up = P.inputs[j].up
        h = how if (how != "pooled" or up > 1) else "mask"
        B = Bwd(P, j, h, acc, din2 if up == 1 else None, null_in and P.inputs[j].mode == ID)
        if not (null_in and P.inputs[j].mode == ID):
            B.reduce().check_reduce(f"reduce of input {j}")
        B.apply().check_apply(f"apply of input {j}")


# ---- 1a. threads per row, idle lanes, slabs, scalar instances ----------------------------------------------------------------
# (element type, C): what geom() makes of it.  N, H, W = 3, 4, 6: more pixels than one block step of the wide rows, fewer than a grid.
LANES = [
    (BF, 8, "V8 tpr1"), (BF, 16, "V8 tpr2"), (BF, 24, "V8 tpr4, 3 of 4 lanes live"), (BF, 32, "V8 tpr4"),
    (BF, 48, "V8 tpr8, 6 of 8 lanes live"), (BF, 128, "V8 tpr16"), (BF, 256, "V8 tpr32"), (BF, 448, "V8 tpr64, 56 of 64 lanes live"),
    (BF, 512, "V8 tpr64 = one full slab"), (BF, 576, "V8 tpr64, 2 slabs, 8 live columns in the second"),
    (F32, 4, "V4 tpr1"), (F32, 12, "V4 tpr4, 3 of 4 lanes live"), (F32, 64, "V4 tpr16"), (F32, 512, "V4 tpr128 = one full slab"),
    (F32, 520, "V4 tpr128, 2 slabs, 2 live columns in the second"),
    (BF, 3, "scalar (C % 8): tpr4, 3 live"), (BF, 7, "scalar: tpr8"), (BF, 36, "scalar: tpr64"), (BF, 257, "scalar: tpr256, 2 slabs, 1 live"),
    (BF, 300, "scalar: tpr256, 2 slabs"), (F32, 3, "scalar (C % 4): tpr4"), (F32, 130, "scalar: tpr256"), (F32, 257, "scalar: tpr256, 2 slabs"),
]


@pytest.mark.parametrize("tdt,Cn,what", LANES, ids=[f"{TN[t]}-C{c}" for t, c, _ in LANES])
def test_exact_lanes_and_slabs(tdt, Cn, what):
    run_chain(tdt, 3, 4, 6, Cn, ((1, AF), (1, ID)), relu=1, how="mask", acc=1, din2=0)


# one misaligned operand, everything else aligned: each operand the launchers inspect (ew_fwd_t: out, in[j]; ew_bwd_t: dout, in,
# out, din, din2), by pitch and by base pointer.  C = 32 would be a vector problem.
MIS = [(op, kind) for op in ("in0", "in1", "out", "dout", "din", "din2") for kind in ("pitch", "ptr")]


@pytest.mark.parametrize("tdt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("mis", MIS, ids=[f"{o}-{k}" for o, k in MIS])
def test_exact_one_misaligned_operand(tdt, mis):
    run_chain(tdt, 2, 5, 7, 32, ((1, AF), (1, ID)), relu=1, how="out", din2=1, mis=mis)


# ---- 1b. pixel loops at up == 1 (cap 256 blocks: forward nin <= 2, reduce, apply) ---------------------------------------------
# S = 256 * ppb pixels per grid step.  (bf16 C = 512: ppb 4, S 1024; fp32 C = 64: ppb 16, S 4096; bf16 C = 36 scalar: ppb 4, S 1024)
LOOPS = [(BF, 512, 1024), (F32, 64, 4096), (BF, 36, 1024)]
PIX = [("1-pixel", lambda S: 1), ("less-than-a-block", lambda S: 3), ("3S-no-trip-remainder-3", lambda S: 3 * S),
       ("4S-one-trip-no-tail", lambda S: 4 * S), ("6S+1-one-trip-remainder-2", lambda S: 6 * S + 1),
       ("9S+3-two-trips-remainder-1-ragged", lambda S: 9 * S + 3)]


@pytest.mark.parametrize("tdt,Cn,S", LOOPS, ids=[f"{TN[t]}-C{c}" for t, c, _ in LOOPS])
@pytest.mark.parametrize("pix", PIX, ids=[p[0] for p in PIX])
def test_exact_pixel_loops(tdt, Cn, S, pix):
    run_chain(tdt, 1, 1, pix[1](S), Cn, ((1, AF), (1, ID)), relu=1, how="mask", din2=0, js=[0])


@pytest.mark.parametrize("tdt,Cn,S", LOOPS, ids=[f"{TN[t]}-C{c}" for t, c, _ in LOOPS])
@pytest.mark.parametrize("relu,how", [(0, "none"), (1, "out")], ids=["no-relu", "saved-output"])
def test_exact_pixel_loops_other_maskings(tdt, Cn, S, relu, how):
    """reduce_pixels<RM 0 / 2, U 4> and the apply trips without bits, one input (nin 1), accumulating."""
    run_chain(tdt, 1, 1, 9 * S + 3, Cn, ((1, AF),), relu=relu, how=how, acc=1)


# ---- 1c. forward: input counts, upsampling sets, shapes, activations ---------------------------------------------------------
UPS = [((1,), "nin1 -> <V, 2> four-pixel path"), ((1, 1), "nin2"), ((1, 2), "nin2 with an upsampled input: one-pixel loop"),
       ((1, 2, 4), "nin3 -> <V, 4>"), ((1, 2, 4, 8), "nin4"), ((2, 1), "upsampled input 0")]


@pytest.mark.parametrize("tdt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("ups", [u for u, _ in UPS], ids=["up" + "".join(map(str, u)) for u, _ in UPS])
@pytest.mark.parametrize("N,H,W", [(1, 8, 24), (3, 16, 8)], ids=["1x8x24", "3x16x8"])
def test_exact_forward_inputs_and_upsampling(tdt, ups, N, H, W):
    for relu, mask in ((0, False), (1, True), (1, False), (2, True), (2, False)):
        modes = [AF if j % 2 == 0 else ID for j in range(len(ups))]
        P = Prob(tdt, N, H, W, 40, tuple(zip(ups, modes)), relu, mask, seed=relu * 2 + mask).launch()
        P.check_exact(f"relu {relu} mask {mask}")
    # the scalar instance <T, 1, 4> walks the same loops
    Prob(tdt, N, H, W, 5, tuple(zip(ups, [ID] * len(ups))), 1, False, seed=9).launch().check_exact("scalar")


# ---- 1d. backward at every up: bit mask (row-batched pooled_grad_rows<2 / 4 / 8> on the vector path), saved output, no ReLU, pooled
@pytest.mark.parametrize("tdt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("up,how,relu", [(u, h, r) for u in (1, 2, 4, 8) for h, r in (("mask", 1), ("out", 1), ("none", 0), ("pooled", 1))
                                         if not (h == "pooled" and u == 1)])      # (pooled with up == 1 is refused: test_refusals)
def test_exact_backward_maskings(tdt, up, how, relu):
    """pooled: 1, 2, 3 applications of hrp_ew_pool2 for up = 2, 4, 8 (Prob.pooled_level checks every level)."""
    for acc in (0, 1):
        run_chain(tdt, 2, 8, 16, 40, ((1, ID), (up, AF)), relu=relu, how=how, acc=acc, din2=acc, js=[1])
    run_chain(tdt, 2, 8, 16, 5, ((1, ID), (up, AF)), relu=relu, how="out" if relu else "none", acc=1, js=[1])   # scalar instance


@pytest.mark.parametrize("tdt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("how", ["mask", "out"])
def test_exact_backward_leaky(tdt, how):
    """relu == 2: the LEAKY apply instance and reduce_pixels<.., 1 | 2, 1, true>, vector and scalar."""
    for Cn in (40, 5):
        for acc in (0, 1):
            run_chain(tdt, 2, 5, 7, Cn, ((1, AF), (1, ID)), relu=2, how=how, acc=acc, din2=acc)


@pytest.mark.parametrize("tdt", [BF, F32], ids=["bf16", "f32"])
def test_exact_apply_identity_without_input_pointer(tdt):
    for up in (1, 2):
        run_chain(tdt, 2, 4, 6, 40, ((1, AF), (up, ID)), relu=1, how="mask", null_in=True, js=[1])


# up > 1 grid-stride loops: caps 1024 (forward, apply) and 512 (reduce).  Small: one step.  Large (bf16 C = 512, ppb 4): 8400
# output pixels > 4096 repeat the forward; 2100 input pixels > 2048 repeat the reduce; scalar C = 36 with 4800 input pixels > 4096
# repeats the apply as well.
@pytest.mark.parametrize("tdt,N,H,W,Cn", [(BF, 1, 4, 4, 512), (BF, 1, 84, 100, 512), (BF, 1, 96, 200, 36), (F32, 1, 84, 100, 256)],
                         ids=["one-step", "fwd-and-reduce-repeat", "scalar-all-repeat", "f32-fwd-and-reduce-repeat"])
def test_exact_upsampled_grid_stride(tdt, N, H, W, Cn):
    run_chain(tdt, N, H, W, Cn, ((1, ID), (2, AF)), relu=1, how="mask", js=[1])


# ---- 1e. hrp_ew_pool2 alone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tdt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("N,H,W,Cn", [(2, 4, 6, 8), (1, 6, 4, 40)], ids=["C8", "C40"])
@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
def test_exact_pool2(tdt, N, H, W, Cn, masked):
    """src_pitch > C; the fp32 mask layout is two nibbles per 8 channels."""
    pool2_case(tdt, N, H, W, Cn, masked)


@pytest.mark.parametrize("tdt,masked", [(BF, True), (F32, False)], ids=["bf16-mask", "f32-nomask"])
def test_exact_pool2_grid_stride(tdt, masked):
    """256 * 260 * 8 = 532 480 work items > 2048 * 256: the grid-stride loop repeats (the smallest such source is 33 MB in bf16)."""
    pool2_case(tdt, 1, 512, 520, 64, masked)


def pool2_case(tdt, N, H, W, Cn, masked):
    gen = torch.Generator().manual_seed(H)
    src_ref = rint(gen, (N, H, W, Cn))
    pos = torch.rand((N, H, W, Cn), generator=gen) > 0.5
    vec = O.VEC[tdt]
    src = Buf(N * H * W, Cn, Cn + 2 * vec, tdt, DEV).put(src_ref)
    mk = Buf(N * H * W, Cn // vec, Cn // vec + 3, torch.uint8, DEV).put(O.pack_bits(pos, vec)) if masked else None
    dst = Buf(N * (H // 2) * (W // 2), Cn, Cn, F32, DEV)
    rc = nv.lib().hrp_ew_pool2(src.ptr, DT[tdt], src.pitch, mk.ptr if masked else None, mk.pitch if masked else 0, N, H, W, Cn, dst.ptr, None)
    assert rc == 0, nv.lib().hrp_last_error()
    torch.cuda.synchronize()
    assert torch.equal(dst.get(), O.pool2(src_ref, pos if masked else None).float().reshape(-1, Cn))
    assert dst.outside_untouched()


def test_pool2_real_values_keep_the_fixed_order():
    """((a + b) + (c + d)) in fp32 is one definite number: real values must match the fp32 restatement bit for bit."""
    gen = torch.Generator().manual_seed(4)
    ref = torch.randn(2, 6, 8, 16, generator=gen)
    src, dst = Buf(96, 16, 24, F32, DEV).put(ref), Buf(24, 16, 16, F32, DEV)
    assert nv.lib().hrp_ew_pool2(src.ptr, nv.HRP_F32, 24, None, 0, 2, 6, 8, 16, dst.ptr, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst.get(), O.pool2(ref, None, F32).reshape(-1, 16))


# ---- 1f. batched launches ---------------------------------------------------------------------------------------------------
def batch_problems(tdt, seed):
    """Two large problems (8 MiB each; the second a 3-input fuse sum -> the 4-input variant) and tiny ones whose byte share is
    under 16 / 768: they run on the 16-block floor; the C = 512 one (320 KiB, 64 resp. 32 pixels per step) loops 5 steps - one
    four-pixel trip and a tail.  One 2-slab problem, one with idle lanes, one single pixel."""
    n = 2 if tdt == BF else 1
    two = ((1, AF), (1, ID))
    return [Prob(tdt, n, 128, 128, 128, two, 1, True, seed=seed), Prob(tdt, n, 128, 128, 128, ((1, AF), (2, ID), (4, AF)), 1, True, seed=seed + 1),
            Prob(tdt, 1, 16, 20 if tdt == BF else 10, 512, two, 1, True, seed=seed + 2), Prob(tdt, 1, 4, 6, 576 if tdt == BF else 520, two, 1, True, seed=seed + 3),
            Prob(tdt, 1, 1, 1, 8, ((1, ID),), 0, False, seed=seed + 4), Prob(tdt, 3, 2, 2, 24, two, 1, True, seed=seed + 5)]


@pytest.mark.parametrize("tdt", [BF, F32], ids=["bf16", "f32"])
def test_exact_batched_families(tdt):
    A, S = batch_problems(tdt, 50), batch_problems(tdt, 50)      # batched / single launches of the same problems
    rc, info = O.run_batch(nv, nv.BATCH_EW_FWD, [p.desc for p in A], DEV)
    assert rc == 0, nv.lib().hrp_last_error()
    assert info.variant == nv.EW_MAX_IN and [info.blk0[i + 1] - info.blk0[i] for i in (2, 4, 5)] == [16, 1, 1]
    for i, (a, s) in enumerate(zip(A, S)):
        a.check_exact(f"batched forward, problem {i}")
        s.launch()
        assert torch.equal(a.out.t, s.out.t) and (a.maskb is None or torch.equal(a.maskb.t, s.maskb.t)), f"problem {i}: batched != single"
    # backward of input 0 of every problem that has a mask, and of the up = 2 / up = 4 inputs of the fuse sum
    sel = [(i, 0) for i in (0, 1, 2, 3, 5)] + [(1, 1), (1, 2)]
    BA = [Bwd(A[i], j, "mask", acc=i % 2, din2=(i % 2) if A[i].inputs[j].up == 1 else None) for i, j in sel]
    BS = [Bwd(S[i], j, "mask", acc=i % 2, din2=(i % 2) if S[i].inputs[j].up == 1 else None) for i, j in sel]
    rc, info = O.run_batch(nv, nv.BATCH_EW_BWD_REDUCE, [b.desc for b in BA], DEV)
    assert rc == 0, nv.lib().hrp_last_error()
    for k, b in enumerate(BA):
        b.check_reduce(f"batched reduce, entry {k}")
    rc, info = O.run_batch(nv, nv.BATCH_EW_BWD_APPLY, [b.desc for b in BA], DEV)
    assert rc == 0, nv.lib().hrp_last_error()
    for k, (a, s) in enumerate(zip(BA, BS)):
        a.check_apply(f"batched apply, entry {k}")
        s.apply()
        assert torch.equal(a.din.t, s.din.t) and (a.din2 is None or torch.equal(a.din2.t, s.din2.t)), f"entry {k}: batched != single"
    # n = 1
    one = Prob(tdt, 3, 2, 2, 24, ((1, AF), (1, ID)), 1, True, seed=77)
    assert O.run_batch(nv, nv.BATCH_EW_FWD, [one.desc], DEV)[0] == 0
    one.check_exact("batch of one")
    b1 = Bwd(one, 0, "mask")
    assert O.run_batch(nv, nv.BATCH_EW_BWD_REDUCE, [b1.desc], DEV)[0] == 0 and O.run_batch(nv, nv.BATCH_EW_BWD_APPLY, [b1.desc], DEV)[0] == 0
    b1.check_reduce("batch of one")
    b1.check_apply("batch of one")


# ---- 2. arithmetic ----------------------------------------------------------------------------------------------------------
ULP32 = 2.0 ** -24


def within(case, name, got, ref64, ref32, tdt=F32, scale=None):
    """|got - ref64| <= 8 * floor * scale (+ 2^-8 |ref64| for a bf16 result), floor = max(rel_dev(ref32), 2^-24)."""
    scale = float(ref64.abs().max()) if scale is None else scale
    floor = max(float((ref32.to(F64) - ref64).abs().max()) / scale, ULP32)
    err = (got.to(F64) - ref64).abs()
    bound = 8 * floor * scale + (2.0 ** -8 * ref64.abs() if tdt == BF else 0.0)
    print(f"  {case}: {name}: device deviation {float(err.max()) / scale:.3g} of scale, fp32 floor {floor:.3g}")
    worst = float((err - bound).max())
    assert worst <= 0, f"{case}: {name} exceeds 8 floors{' + one bf16 rounding' if tdt == BF else ''} by {worst:.3g} (floor {floor:.3g}, scale {scale:.3g})"
    return floor * scale


def check_decisions(case, P, floor_abs):
    """-> the device's ReLU decisions.  They may differ from the oracle only within the fp32 floor of zero, on <= 0.1 % of the tensor."""
    N, H, W, Cn = P.shape
    if P.maskb is not None:
        bits = P.maskb.get().to(torch.int32)
        pos = ((bits[:, :, None] >> torch.arange(P.vec)) & 1).reshape(N, H, W, -1)[..., :Cn].bool()
        assert P.maskb.outside_untouched()
        assert torch.equal(pos, P.out.get((N, H, W, Cn)).float() > 0), f"{case}: mask bits and the sign of out disagree"
    else:
        pos = P.out.get((N, H, W, Cn)).float() > 0
    diff = pos != (P.pre > 0)
    assert not bool((diff & (P.pre.abs() > floor_abs)).any()), f"{case}: a ReLU decision differs outside the fp32 floor of zero"
    assert float(diff.double().mean()) <= 1e-3
    return pos


@pytest.mark.parametrize("name", sorted(O.ARITH_FWD))
def test_bn_train_forward(name):
    tdt, shape, inputs = O.arith_fwd_case(name)
    Cn = shape[3]
    P = Prob(tdt, *shape, relu=1, mask=True, inputs=inputs, consts_out=True).launch()
    p32, o32, _ = O.ew_forward(inputs, 1, P.vec, F32)
    floor_abs = within(name, "out", P.out.get(shape), P.ref_out, o32, tdt, scale=float(P.pre.abs().max()))
    assert P.out.outside_untouched()
    check_decisions(name, P, max(float((p32.to(F64) - P.pre).abs().max()), ULP32 * float(P.pre.abs().max())))
    got = P.consts.cpu()
    assert bool((got[2 * Cn:] == O.FSENT).all()), "consts_out written past [2C]"
    _, _, m64, i64 = O.consts(inputs[0], Cn)
    _, _, m32, i32 = O.consts(inputs[0], Cn, F32)
    within(name, "consts_out mean", got[:Cn], m64, m32)
    within(name, "consts_out invstd", got[Cn:2 * Cn], i64, i32)


@pytest.mark.parametrize("name", sorted(O.ARITH_CHAIN))
def test_bn_train_chain(name):
    """ew_fwd (BN_TRAIN + ReLU + mask) -> ew_bwd_reduce -> ew_bwd_apply -> hrp_bn_param_grad against float64 (= autograd)."""
    tdt, shape, inp, dout = O.arith_chain_case(name)
    N, H, W, Cn = shape
    ins = [inp] if inp.up == 1 else [O.OIn(torch.zeros(shape, dtype=tdt), 1, ID), inp]     # an upsampled term rides on a zero identity
    P = Prob(tdt, *shape, relu=1, mask=True, inputs=ins).launch()
    j = len(ins) - 1
    r64, r32 = O.chain_oracle(inp, dout, tdt, F64), O.chain_oracle(inp, dout, tdt, F32)
    floor_abs = within(name, "out", P.out.get(shape), r64[1], r32[1], tdt, scale=float(r64[0].abs().max()))
    pos = check_decisions(name, P, max(float((r32[0].to(F64) - r64[0]).abs().max()), ULP32 * float(r64[0].abs().max())))
    P.dout_ref = dout.to(F64)
    P.dout = P.buf("dout", N * H * W).put(P.dout_ref)
    B = Bwd(P, j, "mask" if P.vector else "out", pos=pos)
    B.sums0.zero_()
    B.sums.zero_()
    B.reduce()
    ref = B.ref                       # float64 with the device's own ReLU decisions
    b32 = O.ew_backward(P.dout_ref, pos, inp, 1, dt=F32)
    within(name, "sum g", B.got_sums()[:Cn], ref["sums"][:Cn], b32["sums"][:Cn])
    within(name, "sum g xhat", B.got_sums()[Cn:], ref["sums"][Cn:], b32["sums"][Cn:])
    B.apply()
    within(name, "din", B.din.get(ref["din"].shape), ref["din"], b32["din"], tdt)
    assert B.din.outside_untouched()
    dg, db = torch.full((Cn + 4,), O.FSENT, device=DEV), torch.full((Cn + 4,), O.FSENT, device=DEV)
    e = nv.BnEntry()
    e.stats, e.a, e.b, e.C, e.count = B.sums.data_ptr(), dg.data_ptr(), db.data_ptr(), Cn, inp.count
    tab = torch.frombuffer(bytearray(bytes(e)), dtype=torch.uint8).to(DEV)
    nv.call("hrp_bn_param_grad", tab.data_ptr(), 1, None)
    torch.cuda.synchronize()
    within(name, "dgamma", dg.cpu()[:Cn], ref["sums"][Cn:], b32["sums"][Cn:])
    within(name, "dbeta", db.cpu()[:Cn], ref["sums"][:Cn], b32["sums"][:Cn])
    assert bool((dg[Cn:] == O.FSENT).all()) and bool((db[Cn:] == O.FSENT).all())


@pytest.mark.parametrize("tdt", [BF, F32], ids=["bf16", "f32"])
def test_affine_reduce_and_apply_with_eval_mode_constants(tdt):
    """(a, b) = (invstd, -mean * invstd) of running statistics: second sum = sum g * xhat (the eval-mode dgamma), din = a * g."""
    gen = torch.Generator().manual_seed(21)
    shape, Cn = (2, 8, 12, 40), 40
    x = rounded(torch.randn(shape, generator=gen, dtype=F64) * 2 + 1, tdt)
    rm, rv = torch.randn(Cn, generator=gen, dtype=F64), 0.5 + torch.rand(Cn, generator=gen, dtype=F64)
    inv = (1 / torch.sqrt(rv + 1e-5)).float()
    inp = O.OIn(x, 1, AF, inv, (-rm * inv.to(F64)).float())
    P = Prob(tdt, *shape, relu=1, mask=True, inputs=[inp]).launch()
    pos = check_decisions("affine", P, 8 * ULP32 * float(P.pre.abs().max()))
    P.make_dout(real=True)
    B = Bwd(P, 0, "mask", pos=pos)
    B.reduce()
    b32 = O.ew_backward(P.dout_ref, pos, inp, 1, dt=F32)
    within(f"affine-{TN[tdt]}", "sum g", B.got_sums()[:Cn], B.ref["sums"][:Cn], b32["sums"][:Cn])
    within(f"affine-{TN[tdt]}", "sum g xhat", B.got_sums()[Cn:], B.ref["sums"][Cn:], b32["sums"][Cn:])
    B.apply()          # din = a * g with a != 1 (the exact tests only have a = 1)
    within(f"affine-{TN[tdt]}", "din", B.din.get(shape), B.ref["din"], b32["din"], tdt)
    assert B.din.outside_untouched()


def bn_table(entries):
    arr = (nv.BnEntry * len(entries))(*entries)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)


TABLE_C = (1, 33, 2048)


@pytest.mark.parametrize("count", [1.0, 96.0])
def test_bn_running_update(count):
    gen = torch.Generator().manual_seed(int(count))
    ents, keep, want = [], [], []
    for k, Cn in enumerate(TABLE_C):
        x = torch.randn(int(count), Cn, generator=gen, dtype=F64) * 2 + 1.5
        stats = O.spread_slots(O.batch_stats(x), gen)
        rm, rv = torch.randn(Cn, generator=gen), 0.5 + torch.rand(Cn, generator=gen)
        d = [stats.to(DEV), torch.cat([rm, torch.full((4,), O.FSENT)]).to(DEV), torch.cat([rv, torch.full((4,), O.FSENT)]).to(DEV),
             torch.tensor([41], dtype=torch.int64, device=DEV)]
        e = nv.BnEntry()
        e.stats, e.a, e.b, e.C, e.count, e.momentum = d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), Cn, count, 0.1
        e.counter = d[3].data_ptr() if k != 1 else None
        ents.append(e)
        keep.append(d)
        want.append((O.bn_running_update(stats, rm, rv, count, 0.1), O.bn_running_update(stats, rm, rv, count, 0.1, F32)))
    tab = bn_table(ents)
    nv.call("hrp_bn_running_update", tab.data_ptr(), len(ents), None)
    torch.cuda.synchronize()
    for k, Cn in enumerate(TABLE_C):
        d, (w64, w32) = keep[k], want[k]
        within(f"running_update-count{int(count)}-C{Cn}", "running_mean", d[1].cpu()[:Cn], w64[0], w32[0])
        within(f"running_update-count{int(count)}-C{Cn}", "running_var", d[2].cpu()[:Cn], w64[1], w32[1])
        assert bool((d[1][Cn:] == O.FSENT).all()) and bool((d[2][Cn:] == O.FSENT).all())
        assert int(d[3]) == (42 if k != 1 else 41)


@pytest.mark.parametrize("accumulate", [0, 1])
def test_bn_fold_and_param_grad(accumulate):
    gen = torch.Generator().manual_seed(5 + accumulate)
    fold, grad, keep = [], [], []
    for Cn in TABLE_C:
        gamma, beta = 0.5 + torch.rand(Cn, generator=gen), torch.randn(Cn, generator=gen)
        rm, rv = torch.randn(Cn, generator=gen), 0.5 + torch.rand(Cn, generator=gen)
        sums = O.spread_slots(torch.randn(2 * Cn, generator=gen, dtype=F64) * 30, gen)
        old = [torch.randn(Cn, generator=gen), torch.randn(Cn, generator=gen)]
        pad = torch.full((4,), O.FSENT)
        d = [t.to(DEV) for t in (gamma, beta, rm, rv)] + [torch.full((Cn + 4,), O.FSENT, device=DEV) for _ in range(2)] + \
            [sums.to(DEV), torch.cat([old[0], pad]).to(DEV), torch.cat([old[1], pad]).to(DEV)]
        e = nv.BnEntry()
        e.a, e.b, e.c, e.d, e.out_scale, e.out_shift, e.C, e.eps, e.accumulate = *[t.data_ptr() for t in d[:6]], Cn, 1e-5, accumulate
        fold.append(e)
        g = nv.BnEntry()
        g.stats, g.a, g.b, g.C, g.accumulate = d[6].data_ptr(), d[7].data_ptr(), d[8].data_ptr(), Cn, accumulate
        grad.append(g)
        keep.append((d, gamma, beta, rm, rv, sums, old))
    t1, t2 = bn_table(fold), bn_table(grad)
    nv.call("hrp_bn_fold", t1.data_ptr(), len(fold), None)
    nv.call("hrp_bn_param_grad", t2.data_ptr(), len(grad), None)
    torch.cuda.synchronize()
    for Cn, (d, gamma, beta, rm, rv, sums, old) in zip(TABLE_C, keep):
        case = f"tables-acc{accumulate}-C{Cn}"
        f64, f32 = O.bn_fold(gamma, beta, rm, rv, 1e-5), O.bn_fold(gamma, beta, rm, rv, 1e-5, F32)
        within(case, "fold scale", d[4].cpu()[:Cn], f64[0], f32[0])
        within(case, "fold shift", d[5].cpu()[:Cn], f64[1], f32[1])
        o = old if accumulate else (None, None)
        g64, g32 = O.bn_param_grad(sums, Cn, *o), O.bn_param_grad(sums, Cn, *o, dt=F32)
        within(case, "dgamma", d[7].cpu()[:Cn], g64[0], g32[0])
        within(case, "dbeta", d[8].cpu()[:Cn], g64[1], g32[1])
        for t in (d[4], d[5], d[7], d[8]):
            assert bool((t[Cn:] == O.FSENT).all()), "table kernel wrote past [C]"


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------
MASK_MSG = "ReLU bit mask needs relu and the 16-byte vector path"


def refused(why, fn, *args):
    """The call returns non-zero and hrp_last_error names the reason of THIS case (the message is never cleared, so its mere
    presence says nothing)."""
    rc = fn(*args)
    torch.cuda.synchronize()
    msg = nv.lib().hrp_last_error().decode()
    assert rc != 0 and why in msg, f"expected a refusal with '{why}', got rc {rc}: '{msg}'"
    return True


def batch_refused(why, fam, descs):
    rc, _ = O.run_batch(nv, fam, descs, DEV)
    msg = nv.lib().hrp_last_error().decode()
    assert rc != 0 and why in msg, f"expected a refusal with '{why}', got rc {rc}: '{msg}'"
    return True


@pytest.mark.parametrize("tdt", [BF, F32], ids=["bf16", "f32"])
def test_refusals(tdt):
    lib = nv.lib()
    two = ((1, AF), (1, ID))

    def fwd(why, P, **kw):
        d = nv.EwDesc()
        O.copy_struct(d, P.desc)
        for k, v in kw.items():
            setattr(d, k, v)
        return refused(why, lib.hrp_ew_fwd, C.byref(d), None) and P.out.untouched() and (P.maskb is None or P.maskb.untouched())

    P = Prob(tdt, 2, 4, 8, 40, two, 1, True)
    spare = Buf(64, 5, 8, torch.uint8, DEV)
    assert fwd(MASK_MSG, P, relu=0), "mask without relu"
    assert fwd("bad descriptor", P, nin=0) and fwd("bad descriptor", P, nin=5), "nin out of range"
    cbuf = torch.full((96,), O.FSENT, device=DEV)
    assert fwd("consts_out needs", P, consts_out=cbuf.data_ptr()) and bool((cbuf == O.FSENT).all()), "consts_out without BN_TRAIN on input 0"
    Pu = Prob(tdt, 2, 4, 8, 40, ((1, AF), (2, ID)), 1, True)
    assert fwd("input 1 geometry", Pu, H=5) and fwd("input 1 geometry", Pu, W=7), "H % up != 0"
    for bad in (Prob(tdt, 2, 4, 8, 5, two, 1, False), Prob(tdt, 2, 4, 8, 40, two, 1, False, mis=("in1", "pitch")),
                Prob(tdt, 2, 4, 8, 40, two, 1, False, mis=("out", "ptr"))):
        assert fwd(MASK_MSG, bad, mask=spare.ptr, mask_pitch=8) and spare.untouched(), "mask on a scalar-path forward"
    d = nv.EwDesc()
    O.copy_struct(d, P.desc)
    d.inp[0].mode, d.inp[0].stats = BN_TRAIN, None
    assert refused("input 0 needs stats", lib.hrp_ew_fwd, C.byref(d), None) and P.out.untouched(), "BN_TRAIN without stats"

    P.launch()
    Pu.launch()

    def bwd(why, B, apply, **kw):
        d = nv.EwBwdDesc()
        O.copy_struct(d, B.desc)
        for k, v in kw.items():
            setattr(d, k, v)
        before = B.sums.clone()
        ok = refused(why, lib.hrp_ew_bwd_apply if apply else lib.hrp_ew_bwd_reduce, C.byref(d), None)
        return ok and B.din.untouched() and (B.din2 is None or B.din2.untouched()) and torch.equal(before, B.sums)

    B = Bwd(P, 0, "mask", din2=0)
    Bu = Bwd(Pu, 1, "mask")
    pooled = torch.zeros(2 * 4 * 8 * 40 + 8, device=DEV)
    for apply in (False, True):
        assert bwd(MASK_MSG, B, apply, relu=0), "mask without relu"
        assert bwd("pooled needs", B, apply, pooled=pooled.data_ptr()), "pooled with up == 1"
        assert bwd("pooled needs", Bu, apply, pooled=pooled.data_ptr(), C=36), "pooled with C % 8 != 0"
        assert bwd("ew_bwd: geometry", Bu, apply, H=5), "H % up != 0"
        assert bwd("din2 needs up == 1", Bu, apply, din2=B.din2.ptr, din2_pitch=B.din2.pitch) and B.din2.untouched(), "din2 with up > 1"
        assert bwd(MASK_MSG, B, apply, dout_pitch=B.desc.dout_pitch + 1), "mask on a scalar-path backward (pitch)"
        assert bwd(MASK_MSG, B, apply, dout=B.desc.dout + B.P.dout.t.element_size()), "mask on a scalar-path backward (pointer)"
    d = nv.EwBwdDesc()
    O.copy_struct(d, B.desc)
    d.inp.mode, d.inp.stats = BN_TRAIN, None
    for fn in (lib.hrp_ew_bwd_reduce, lib.hrp_ew_bwd_apply):
        assert refused("bn needs sums/stats", fn, C.byref(d), None) and B.din.untouched(), "BN_TRAIN without stats"

    # batched launches: LeakyReLU, scalar path (by C, by a misaligned pointer), mixed element types
    ok = Prob(tdt, 2, 4, 8, 40, two, 1, True)
    other = Prob(F32 if tdt == BF else BF, 2, 4, 8, 40, two, 1, True)
    vecmsg = "problem 1 is not on the 16-byte vector path"
    for why, bad in (("LeakyReLU", Prob(tdt, 2, 4, 8, 40, two, 2, True)), (vecmsg, Prob(tdt, 2, 4, 8, 5, two, 1, False)),
                     (vecmsg, Prob(tdt, 2, 4, 8, 40, two, 1, False, mis=("in0", "ptr"))), ("mixed element types", other)):
        assert batch_refused(why, nv.BATCH_EW_FWD, [ok.desc, bad.desc])
        assert ok.out.untouched() and bad.out.untouched()
        bad.launch()
        ok_b, bad_b = Bwd(ok, 0, "mask"), Bwd(bad, 0, "mask" if bad.maskb is not None else "out")
        for fam in (nv.BATCH_EW_BWD_REDUCE, nv.BATCH_EW_BWD_APPLY):
            assert batch_refused(why, fam, [ok_b.desc, bad_b.desc])
            assert ok_b.din.untouched() and bad_b.din.untouched() and torch.equal(ok_b.sums.cpu(), ok_b.sums0)

    # hrp_ew_pool2: odd H, C % 8, misaligned pitch
    esz = 2 if tdt == BF else 4
    src, dst = Buf(2 * 6 * 8, 40, 48, tdt, DEV), Buf(2 * 3 * 4, 40, 40, F32, DEV)
    for why, H, Cn, pitch in (("ew_pool2: geometry", 5, 40, 48), ("ew_pool2: geometry", 6, 36, 48), ("ew_pool2: alignment", 6, 40, 48 + 8 // esz)):
        assert refused(why, lib.hrp_ew_pool2, src.ptr, DT[tdt], pitch, None, 0, 2, H, 8, Cn, dst.ptr, None) and dst.untouched()
