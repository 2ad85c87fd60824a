"""Gradient accumulation over micro-batches on the device: hrp_grad_accumulate bit for bit against torch, and
PlannedModule.set_grad_accumulation against the default single-backward path of the same build (the DepthNet of
tests/test_gpu_model.py, B <= 2, fp32, no dropout).  Training steps are bit-reproducible (README), so the gradients of micro-batch
A and of micro-batch B taken one backward at a time are the reference and every comparison is exact; the only tolerance is the one
of test_gpu_kernels.py::test_fused_clip_adam_matches_torch for the optimizer step."""
import pytest
import torch

from synth import synth_inputs, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- 1. the kernel --------------------------------------------------------------------------------------------------
# n = 1, 3: below one 16-byte vector (scalar tail only); 4: one vector, no tail; 1023: vectors and a tail of 3 in one workgroup;
# 1024 * 256 + 5: 129 workgroups, a ragged last one and a tail of 1.  The launch caps its grid at 2048 workgroups of 256 threads
# that take two vectors per trip, so only the last size makes the grid stride: every thread runs two trips, 300 threads a
# third one, the others the single-vector remainder, and a tail of 2 follows (42 MB).
KERNEL_N = [1, 3, 4, 1023, 1024 * 256 + 5, 4 * (2 * 2048 * 512 + 2048 * 256 + 300) + 2]


def _accumulate(src, acc, first, scale):
    from hrpe_amd import _native as nv
    nv.call("hrp_grad_accumulate", src.data_ptr(), acc.data_ptr(), src.numel(), first, scale,
            torch.cuda.current_stream(src.device).cuda_stream)
    torch.cuda.synchronize()


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("n", KERNEL_N)
def test_kernel_is_bit_exact(n):
    g = torch.Generator(device="cpu").manual_seed(n)
    src = (torch.randn(n, generator=g) * 3.0).to(DEV)
    acc0 = torch.randn(n, generator=g).to(DEV)
    src0 = src.clone()
    guard = 8      # floats behind the n elements: must keep their contents
    buf = torch.full((n + guard,), 7.0, device=DEV)
    # first = 1 over NaNs: acc is not read, the result is src itself
    for scale, want in ((1.0, src), (0.25, src * 0.25)):
        buf[:n] = float("nan")
        _accumulate(src, buf[:n], 1, scale)
        assert torch.equal(_bits(buf[:n]), _bits(want)), f"first=1 scale={scale}"
    # first = 0, scale = 1: the fp32 sum
    buf[:n] = acc0
    _accumulate(src, buf[:n], 0, 1.0)
    assert torch.equal(_bits(buf[:n]), _bits(torch.add(acc0, src)))
    # scale = 0.25: product and sum rounded separately (the kernel forms no FMA), as two fp32 torch ops
    buf[:n] = acc0
    _accumulate(src, buf[:n], 0, 0.25)
    scaled = src * 0.25
    assert torch.equal(_bits(buf[:n]), _bits(acc0 + scaled))
    # a scale whose product is inexact: an FMA would differ from the two roundings in some element
    buf[:n] = acc0
    _accumulate(src, buf[:n], 0, 1.0 / 3.0)
    third = src * torch.tensor(1.0 / 3.0, dtype=torch.float32, device=DEV)
    assert torch.equal(_bits(buf[:n]), _bits(acc0 + third))
    assert bool((buf[n:] == 7.0).all()), "wrote behind the n elements"
    assert torch.equal(_bits(src), _bits(src0)), "src changed"


# ---- 2 .. 7. the plan ------------------------------------------------------------------------------------------------
def _grads(m):
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()}


def _in_buffer(t, buf):
    return buf.data_ptr() <= t.data_ptr() and t.data_ptr() + 4 * t.numel() <= buf.data_ptr() + 4 * buf.numel()


@pytest.fixture(scope="module")
def runs():
    """Every scenario once, on one DepthNet; the tests below only compare what this recorded."""
    from hrpe_amd.lib.models.depth_net import get_rootnet
    from hrpe_amd.optim import FusedClipAdam
    m = get_rootnet("hrnet32")
    sd0 = synth_state_dict(m.state_dict())
    m.load_state_dict(sd0)
    m = m.to(DEV).train()
    xa, _, kva, _ = synth_inputs(2, seed=808)
    xb, _, kvb, _ = synth_inputs(2, seed=909)
    A = (xa.to(DEV), kva.to(DEV), torch.tensor([[1.1], [0.7]], device=DEV))
    B = (xb.to(DEV), kvb.to(DEV), torch.tensor([[0.6], [1.4]], device=DEV))
    C1 = tuple(t[:1].contiguous() for t in B)       # a trailing partial batch: builds a second training plan

    def reset():
        m.load_state_dict(sd0)      # parameters, running statistics, num_batches_tracked (no dropout: no RNG state)

    def fwd(batch):
        x, kv, gt = batch
        return torch.nn.functional.l1_loss(m(x, kv) / 1000.0, gt)

    def step(batch):
        fwd(batch).backward()

    r = {}
    # the default path, one backward at a time: the reference
    reset(); step(A); r["gA"] = _grads(m)
    r["plain_in_arena"] = all(_in_buffer(p.grad, m.flat_grads()[0]) for p in m.parameters() if p.grad is not None)
    opt = FusedClipAdam([p for p in m.parameters() if p.grad is not None], lr=1e-4, max_norm=5.0)
    opt.prepare()                    # tables built over the ARENA views: the accumulated step below must rebuild them
    r["ptrs_plain"] = opt._grad_ptrs
    step(B); r["gB"] = _grads(m)
    reset(); step(A); r["gA_again"] = _grads(m); step(C1); r["gC"] = _grads(m)

    # 2. two micro-batches through one plan
    reset(); m.set_grad_accumulation(2)
    r["no_buffer_before_backward"] = m.flat_grads() == []
    step(A); r["acc_A_only"] = _grads(m)
    step(B); r["acc_AB"] = _grads(m)
    (buf,) = m.flat_grads()
    r["acc_in_buffer"] = all(_in_buffer(p.grad, buf) and getattr(p.grad, "_hrp_plan_grad", False)
                             for p in m.parameters() if p.grad is not None)
    r["complete_after_2"] = m.accumulation_complete()
    try:
        step(A)
        r["third_raises"] = False
    except RuntimeError as e:
        r["third_raises"] = "begin_accumulation" in str(e)
    r["acc_after_refused_third"] = _grads(m)
    # 5. optimizer step on the accumulated gradient
    r["before"] = {n: p.detach().clone() for n, p in m.named_parameters()}
    opt.step()
    r["ptrs_accum"] = opt._grad_ptrs
    r["ptrs_are_views"] = opt._grad_ptrs == tuple(p.grad.data_ptr() for p in opt.params)
    r["after"] = {n: p.detach().clone() for n, p in m.named_parameters()}
    r["total_norm"] = opt.total_norm().item()

    # 3. two plans, one parameter set
    reset(); m.begin_accumulation(); step(A); step(C1); r["acc_AC"] = _grads(m)
    r["one_buffer"] = m.flat_grads()[0] is buf
    # 4. a second grad-enabled forward leaves the gradients alone
    reset(); m.begin_accumulation(); step(A); loss = fwd(B); torch.cuda.synchronize(); r["acc_A_fwdB"] = _grads(m)
    del loss
    # 7. average=True
    m.set_grad_accumulation(2, average=True); reset(); step(A); step(B); r["avg_AB"] = _grads(m)
    # 6. steps == 1 is the default path
    m.set_grad_accumulation(1); reset(); step(A); r["g1"] = _grads(m)
    r["accum_attr_none"] = m._accum is None and all(run.plan.accum is None for run in m._plans.values())
    r["g1_in_arena"] = all(any(_in_buffer(p.grad, a) for a in m.flat_grads()) for p in m.parameters() if p.grad is not None)
    r["n_train_plans"] = len(m.flat_grads())
    return r


def _assert_equal(got, want, what):
    assert got.keys() == want.keys()
    n_checked = 0
    for name in want:
        assert (got[name] is None) == (want[name] is None), f"{what}: {name}"
        if want[name] is not None:
            assert torch.equal(_bits(got[name]), _bits(want[name])), \
                f"{what}: {name} differs, max {(got[name] - want[name]).abs().max().item():.3e}"
            n_checked += 1
    assert n_checked > 100


def _sum(a, b):
    return {n: (None if a[n] is None else torch.add(a[n], b[n])) for n in a}


def test_reference_steps_are_reproducible(runs):
    """The one assumption of the exact comparisons: the same micro-batch from the same state gives the same bits."""
    _assert_equal(runs["gA_again"], runs["gA"], "A twice")
    assert any(g is not None and bool((g != 0).any()) for g in runs["gA"].values())
    live = {n for n, g in runs["gA"].items() if g is not None and bool((g != 0).any())}
    # the linear head (a 1x1 convolution of the pooled [N, 2048, 1, 1] feature), its bias, BatchNorm weight / bias, conv weights
    assert {"depth_layer.weight", "depth_layer.bias", "backbone.bn1.weight", "backbone.bn1.bias", "backbone.conv1.weight"} <= live
    assert sum(runs["gA"][n].dim() == 4 for n in live) > 100 and sum(runs["gA"][n].dim() == 1 for n in live) > 100


def test_two_micro_batches_sum_exactly(runs):
    assert runs["plain_in_arena"] and runs["no_buffer_before_backward"] and runs["acc_in_buffer"] and runs["complete_after_2"]
    _assert_equal(runs["acc_A_only"], runs["gA"], "after the first micro-batch")
    _assert_equal(runs["acc_AB"], _sum(runs["gA"], runs["gB"]), "A + B")


def test_a_backward_beyond_steps_is_refused_and_changes_nothing(runs):
    assert runs["third_raises"]
    _assert_equal(runs["acc_after_refused_third"], runs["acc_AB"], "after the refused third backward")


def test_two_plans_accumulate_into_one_buffer(runs):
    assert runs["one_buffer"] and runs["n_train_plans"] == 2
    _assert_equal(runs["acc_AC"], _sum(runs["gA"], runs["gC"]), "A (B = 2) + C (B = 1)")


def test_second_forward_keeps_the_gradients(runs):
    _assert_equal(runs["acc_A_fwdB"], runs["gA"], "backward A, then a grad-enabled forward of B")


def test_optimizer_steps_on_the_accumulated_gradient(runs):
    """FusedClipAdam on the accumulation views == clip_grad_norm_(5) + torch.optim.Adam on clones carrying gA + gB; tolerances of
    test_gpu_kernels.py::test_fused_clip_adam_matches_torch (rtol 1e-5 / atol 1e-6 on the parameters, 1e-4 relative on the norm)."""
    assert runs["ptrs_accum"] != runs["ptrs_plain"] and runs["ptrs_are_views"]       # the tables were rebuilt over the buffer
    want = _sum(runs["gA"], runs["gB"])
    names = [n for n in want if want[n] is not None]
    ref = [torch.nn.Parameter(runs["before"][n].clone()) for n in names]
    for p, n in zip(ref, names):
        p.grad = want[n].clone()
    tn = torch.nn.utils.clip_grad_norm_(ref, 5.0)
    torch.optim.Adam(ref, lr=1e-4).step()
    flat = torch.cat([want[n].reshape(-1) for n in names])
    assert abs(tn.item() - flat.double().norm().item()) <= 1e-4 * tn.item()
    assert abs(runs["total_norm"] - tn.item()) <= 1e-4 * tn.item(), (runs["total_norm"], tn.item())
    moved = 0
    for p, n in zip(ref, names):
        q = runs["after"][n]
        assert torch.allclose(p, q, rtol=1e-5, atol=1e-6), (n, (p - q).abs().max().item())
        moved += int(not torch.equal(q, runs["before"][n]))
    assert moved > 100


def test_steps_1_is_the_default_path(runs):
    assert runs["accum_attr_none"] and runs["g1_in_arena"]
    _assert_equal(runs["g1"], runs["gA"], "set_grad_accumulation(1)")


def test_average_scales_every_micro_batch(runs):
    """scale = 1 / 2 is a power of two: gA / 2 + gB / 2 == (gA + gB) / 2 bit for bit barring underflow, and the kernel's
    two-rounding form is what torch computes below in any case."""
    want = {n: (None if g is None else g * 0.5 + runs["gB"][n] * 0.5) for n, g in runs["gA"].items()}
    _assert_equal(runs["avg_AB"], want, "average=True")
    half = {n: (None if g is None else torch.add(g, runs["gB"][n]) * 0.5) for n, g in runs["gA"].items()}
    for n, g in half.items():
        if g is not None:
            normal = g.abs() > 1e-30
            assert torch.equal(_bits(runs["avg_AB"][n][normal]), _bits(g[normal])), n
