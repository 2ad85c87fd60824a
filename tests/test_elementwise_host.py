"""The float64 oracle of the fused element-wise and BatchNorm kernels (tests/ew_oracle.py) proved against torch autograd in double
on the CPU: no GPU, no call into the library.  The GPU tests (test_gpu_elementwise.py) then compare the kernels with this oracle.

Also here: the fp32 noise floors of the arithmetic cases (max deviation of the fp32 restatement from float64, relative to the
tensor's scale) and the check that, for the seeds in use, the share of pre-activations within that floor of zero stays under the
0.1 % the GPU tests may excuse."""
import pytest
import torch
import torch.nn.functional as F

import ew_oracle as O
from ew_oracle import AFFINE, BN_TRAIN, F64, IDENTITY


def nchw(x):
    return x.permute(0, 3, 1, 2)


def nhwc(x):
    return x.permute(0, 2, 3, 1)


def make_inputs(gen, shape, spec):
    return [O.real_input(gen, shape, F64, up, mode) for up, mode in spec]


def torch_forward(inputs, relu):
    """relu(sum of batch_norm(training) / affine / identity terms, each nearest-upsampled) with autograd leaves."""
    leaves, total = [], None
    for inp in inputs:
        x = nchw(inp.x).clone().requires_grad_(True)
        leaf = {"x": x}
        if inp.mode == BN_TRAIN:
            g, b = inp.a.to(F64).clone().requires_grad_(True), inp.b.to(F64).clone().requires_grad_(True)
            t = F.batch_norm(x, None, None, g, b, training=True, eps=inp.eps)
            leaf.update(gamma=g, beta=b)
        elif inp.mode == AFFINE:
            t = x * inp.a.to(F64)[None, :, None, None] + inp.b.to(F64)[None, :, None, None]
        else:
            t = x
        if inp.up > 1:
            t = F.interpolate(t, scale_factor=inp.up, mode="nearest")
        total = t if total is None else total + t
        leaves.append(leaf)
    out = total if relu == 0 else F.relu(total) if relu == 1 else F.leaky_relu(total, O.SLOPE)
    return total, out, leaves


SPECS = {"bn": [(1, BN_TRAIN)], "residual": [(1, BN_TRAIN), (1, IDENTITY)], "affine-up2": [(2, AFFINE), (1, IDENTITY)],
         "fuse4": [(1, BN_TRAIN), (2, BN_TRAIN), (4, AFFINE), (8, BN_TRAIN)], "up-first": [(2, BN_TRAIN), (1, AFFINE)]}


@pytest.mark.parametrize("relu", [0, 1, 2])
@pytest.mark.parametrize("spec", sorted(SPECS))
def test_oracle_matches_autograd(spec, relu):
    gen = torch.Generator().manual_seed(7 + relu)
    shape = (3, 8, 16, 5)
    inputs = make_inputs(gen, shape, SPECS[spec])
    dout = torch.randn(shape, generator=gen, dtype=F64)
    pre, out, bits = O.ew_forward(inputs, relu, 4)
    tpre, tout, leaves = torch_forward(inputs, relu)
    assert torch.allclose(pre, nhwc(tpre), rtol=0, atol=1e-12) and torch.allclose(out, nhwc(tout), rtol=0, atol=1e-12)
    assert torch.equal(bits, O.pack_bits(nhwc(tout) > 0, 4) if relu else bits)
    tout.backward(nchw(dout))
    for inp, leaf in zip(inputs, leaves):
        b = O.ew_backward(dout, pre > 0, inp, relu)
        assert torch.allclose(b["din"], nhwc(leaf["x"].grad), rtol=0, atol=1e-11), spec
        assert torch.equal(b["din2"], b["g"])
        if inp.mode == BN_TRAIN:
            dgamma, dbeta = O.bn_param_grad(O.spread_slots(b["sums"], gen), shape[-1])
            assert torch.allclose(dgamma, leaf["gamma"].grad, rtol=0, atol=1e-10)
            assert torch.allclose(dbeta, leaf["beta"].grad, rtol=0, atol=1e-10)
        old = torch.randn(b["din"].shape, generator=gen, dtype=F64)
        acc = O.ew_backward(dout, pre > 0, inp, relu, din_old=old, din2_old=old)
        assert torch.allclose(acc["din"], b["din"] + old) and torch.allclose(acc["din2"], b["g"] + old)


def test_affine_reduce_is_the_eval_mode_dgamma():
    """(a, b) = (invstd, -mean * invstd) of running statistics: the second sum is sum g * xhat = dgamma of an eval-mode BatchNorm."""
    gen = torch.Generator().manual_seed(3)
    shape = (2, 6, 4, 9)
    x = torch.randn(shape, generator=gen, dtype=F64) * 2 + 1
    rm, rv = torch.randn(9, generator=gen, dtype=F64), 0.5 + torch.rand(9, generator=gen, dtype=F64)
    inv = 1 / torch.sqrt(rv + 1e-5)
    dout = torch.randn(shape, generator=gen, dtype=F64)
    gamma = torch.ones(9, dtype=F64, requires_grad=True)
    beta = torch.zeros(9, dtype=F64, requires_grad=True)
    y = F.relu(F.batch_norm(nchw(x), rm, rv, gamma, beta, training=False, eps=1e-5))
    y.backward(nchw(dout))
    inp = O.OIn(x, 1, AFFINE, inv, -rm * inv)
    pre, _, _ = O.ew_forward([inp], 1, 8)
    b = O.ew_backward(dout, pre > 0, inp, 1)
    assert torch.allclose(b["sums"][9:], gamma.grad, rtol=0, atol=1e-11) and torch.allclose(b["sums"][:9], beta.grad, rtol=0, atol=1e-11)


def test_mask_layout():
    pos = torch.zeros(1, 1, 2, 11, dtype=torch.bool)
    pos[0, 0, 0, 0] = pos[0, 0, 0, 9] = pos[0, 0, 1, 7] = pos[0, 0, 1, 10] = True
    assert O.pack_bits(pos, 8).tolist() == [[[[1, 2], [128, 4]]]]
    assert O.pack_bits(pos, 4).tolist() == [[[[1, 0, 2], [0, 8, 4]]]]


def test_pool2_matches_avg_pool_and_window_sum():
    gen = torch.Generator().manual_seed(5)
    g = torch.randn(2, 8, 16, 6, generator=gen, dtype=F64)
    pos = torch.rand(2, 8, 16, 6, generator=gen) > 0.4
    p1 = O.pool2(g, pos)
    assert torch.allclose(p1, nhwc(F.avg_pool2d(nchw(g * pos), 2)) * 4, rtol=0, atol=1e-13)
    p3 = O.pool2(O.pool2(p1))
    assert torch.allclose(p3, O.window_sum(O.masked_grad(g, pos, 1), 8), rtol=0, atol=1e-12)


@pytest.mark.parametrize("shape", [(4, 3, 5, 6), (1, 1, 2, 3)])
def test_bn_tables_match_batchnorm2d(shape):
    gen = torch.Generator().manual_seed(11)
    Cn = shape[-1]
    x = torch.randn(shape, generator=gen, dtype=F64) * 3 + 2
    bn = torch.nn.BatchNorm2d(Cn, eps=1e-5, momentum=0.1).double()
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(Cn, generator=gen, dtype=F64))
        bn.running_var.copy_(0.5 + torch.rand(Cn, generator=gen, dtype=F64))
        bn.weight.copy_(0.5 + torch.rand(Cn, generator=gen, dtype=F64))
        bn.bias.copy_(torch.randn(Cn, generator=gen, dtype=F64))
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    bn.train()
    bn(nchw(x))
    count = float(shape[0] * shape[1] * shape[2])
    rm, rv = O.bn_running_update(O.spread_slots(O.batch_stats(x), gen), rm0, rv0, count, 0.1)
    assert torch.allclose(rm, bn.running_mean, rtol=0, atol=1e-12) and torch.allclose(rv, bn.running_var, rtol=0, atol=1e-11)
    sc, sh = O.bn_fold(bn.weight.detach(), bn.bias.detach(), rm, rv, 1e-5)
    bn.eval()
    y = nhwc(bn(nchw(x))).detach()
    assert torch.allclose(x * sc + sh, y, rtol=0, atol=1e-11)


def test_bn_running_update_of_one_value_has_no_bessel_factor():
    """count == 1 (BatchNorm2d refuses it in train mode): biased variance 0 enters the running variance as it is."""
    x = torch.tensor([[[[3.0, -2.0]]]], dtype=F64)
    rm, rv = O.bn_running_update(O.batch_stats(x)[None, :].repeat(O.SLOTS, 1) / O.SLOTS, torch.ones(2, dtype=F64),
                                 torch.full((2,), 2.0, dtype=F64), 1.0, 0.1)
    assert torch.allclose(rm, torch.tensor([1.2, 0.7], dtype=F64)) and torch.allclose(rv, torch.tensor([1.8, 1.8], dtype=F64))


def test_exact_cases_are_exact_in_fp32():
    """Integer data in [-8, 8] with IDENTITY / AFFINE(1, 0): the fp32 restatement equals the float64 oracle bit for bit, so the
    exact GPU tests need no tolerance."""
    gen = torch.Generator().manual_seed(2)
    shape = (2, 8, 8, 12)
    ri = lambda s: torch.randint(-8, 9, s, generator=gen).to(F64)   # noqa: E731
    one, zero = torch.ones(12), torch.zeros(12)
    inputs = [O.OIn(ri(shape), 1, AFFINE, one, zero), O.OIn(ri((2, 4, 4, 12)), 2), O.OIn(ri((2, 1, 1, 12)), 8, AFFINE, one, zero)]
    dout = ri(shape)
    for relu in (0, 1, 2):
        p64, o64, b64 = O.ew_forward(inputs, relu, 8)
        p32, o32, b32 = O.ew_forward(inputs, relu, 8, torch.float32)
        assert torch.equal(o64.float(), o32) and torch.equal(b64, b32)
        for inp in inputs:
            r64, r32 = O.ew_backward(dout, p64 > 0, inp, relu), O.ew_backward(dout, p32 > 0, inp, relu, dt=torch.float32)
            # (LeakyReLU: slope * integer is one rounding, so a single term is exact; sums of such terms are not)
            if relu != 2 or inp.up == 1:
                assert torch.equal(r64["din"].float(), r32["din"])
            if relu != 2:
                assert torch.equal(r64["sums"].float(), r32["sums"])


def fwd_floor(name):
    tdt, shape, inputs = O.arith_fwd_case(name)
    p64, o64, _ = O.ew_forward(inputs, 1, O.VEC[tdt])
    p32, o32, _ = O.ew_forward(inputs, 1, O.VEC[tdt], torch.float32)
    return p64, O.rel_dev(p32, p64) * float(p64.abs().max())


@pytest.mark.parametrize("name", sorted(O.ARITH_FWD))
def test_near_zero_share_of_the_forward_cases(name, capsys):
    pre, floor = fwd_floor(name)
    share = O.near_zero_share(pre, floor)
    with capsys.disabled():
        print(f"\n  {name}: fp32 floor {floor / float(pre.abs().max()):.3g} of scale, share of |pre| <= floor {share:.5f}")
    assert share < 1e-3


@pytest.mark.parametrize("name", sorted(O.ARITH_CHAIN))
def test_floors_of_the_chain_cases(name, capsys):
    tdt, shape, inp, dout = O.arith_chain_case(name)
    r64, r32 = O.chain_oracle(inp, dout, tdt, F64), O.chain_oracle(inp, dout, tdt, torch.float32)
    floors = [O.rel_dev(a, b) for a, b in zip(r32, r64)]
    share = O.near_zero_share(r64[0], floors[0] * float(r64[0].abs().max()))
    with capsys.disabled():
        print(f"\n  {name}: fp32 floors pre {floors[0]:.3g} sums {floors[2]:.3g} din {floors[3]:.3g} dgamma {floors[4]:.3g} "
              f"dbeta {floors[5]:.3g}; near-zero share {share:.5f}")
    assert share < 1e-3 and all(f < 1e-3 for f in floors)
