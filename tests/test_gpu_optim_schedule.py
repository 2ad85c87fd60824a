"""FusedClipAdam with its hyper-parameters in device memory (hrp_opt_adam_step_groups / hrp_opt_set_group): the same bits as the
launch-argument path, a learning-rate schedule applied through a replayed HIP graph, the capture rule, parameter groups with
torch.optim.Adam's weight decay, and checkpoint interchange of several groups.

Tolerances are the optimizer's own (test_fused_clip_adam_matches_torch): rtol 1e-5 / atol 1e-6 on parameters, rtol 1e-5 / atol 1e-7
on clipped gradients, 1e-4 relative on the norm.  The shapes cover a chunk boundary at 4096 elements, tails that are no multiple of
four and a tensor that starts 4 bytes off a 16-byte boundary (the (5000,) one: a view one float into its buffer)."""
import io
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import hrpe_amd  # noqa: F401

DEV = torch.device("cuda:0")
SHAPES = [(64, 32, 3, 3), (64,), (1000, 7), (5000,), (3,), (4097,)]
UNALIGNED = 3


class A(dict):
    __getattr__ = dict.__getitem__


def initial(seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [torch.randn(s, generator=g).to(DEV) for s in SHAPES]


def params_of(init):
    """Fresh parameters holding `init`; the UNALIGNED one lives one float into a larger buffer."""
    out = []
    for i, t in enumerate(init):
        if i == UNALIGNED:
            buf = torch.zeros(t.numel() + 1, device=DEV)
            v = buf[1:].view(t.shape)
            v.copy_(t)
            assert v.data_ptr() % 16 == 4
            out.append(torch.nn.Parameter(v))
        else:
            out.append(torch.nn.Parameter(t.clone()))
    return out


def grads(it, scale=None):
    g = torch.Generator(device="cpu").manual_seed(1000 + it)
    scale = (3.0 if it % 2 == 0 else 0.01) if scale is None else scale
    return [torch.randn(s, generator=g).to(DEV) * scale for s in SHAPES]


def give(params, gs):
    for p, g in zip(params, gs):
        p.grad = g.clone()


def moments(opt):
    return [t for mv in opt.state_views for t in mv]


def all_equal(xs, ys):
    return all(torch.equal(x, y) for x, y in zip(xs, ys))


def assert_close(ps, qs, rtol=1e-5, atol=1e-6, what=""):
    for i, (p, q) in enumerate(zip(ps, qs)):
        assert torch.allclose(p, q, rtol=rtol, atol=atol), (what, i, (p - q).abs().max().item())


def expo_args(**over):
    return A(dict(use_schedule=True, schedule_type="exponential", n_epochs_warmup=0, start_decay=1, end_decay=100, exponent=0.5), **over)


@pytest.mark.gpu
def test_device_hyper_one_group_no_decay_gives_the_bits_of_the_default_path():
    from hrpe_amd.optim import FusedClipAdam
    init = initial(3)
    a, b = params_of(init), params_of(init)
    opt_a = FusedClipAdam(a, lr=1e-2, max_norm=5.0)
    opt_b = FusedClipAdam(b, lr=1e-2, max_norm=5.0, device_hyper=True)
    assert not opt_a._device_hyper and opt_b._device_hyper and opt_a.param_groups[0]["weight_decay"] == 0
    for it in range(4):
        gs = grads(it)
        give(a, gs)
        give(b, gs)
        opt_a.step()
        opt_b.step()
        assert all_equal(a, b) and all_equal([p.grad for p in a], [p.grad for p in b]), it
        assert all_equal(moments(opt_a), moments(opt_b)), it
        assert torch.equal(opt_a.total_norm(), opt_b.total_norm())
    assert float(opt_b.step_count) == 4.0 and not all_equal(a, init)


@pytest.mark.gpu
def test_schedule_reaches_a_replayed_graph():
    """One captured step(), six epochs of copy gradients in / replay / scheduler.step(): the replayed step applies the scheduled
    rate (the same bits as the eager default path under the same scheduler), not the captured one."""
    from hrpe_amd.lib.utils.utils import get_scheduler
    from hrpe_amd.optim import FusedClipAdam
    init = initial(5)
    pg, pe, pt, pc = params_of(init), params_of(init), [torch.nn.Parameter(t.clone()) for t in init], params_of(init)
    opt_g = FusedClipAdam(pg, lr=1e-2, max_norm=5.0, device_hyper=True)
    opt_e = FusedClipAdam(pe, lr=1e-2, max_norm=5.0)
    opt_t = torch.optim.Adam(pt, lr=1e-2)
    opt_c = FusedClipAdam(pc, lr=1e-2, max_norm=5.0)                    # the constant initial rate: what a baked launch argument gives
    static = [torch.zeros(s, device=DEV) for s in SHAPES]
    for p, g in zip(pg, static):
        p.grad = g
    sch_g, sch_e, sch_t = [get_scheduler(expo_args(), o, -1) for o in (opt_g, opt_e, opt_t)]
    opt_g.prepare()                                                     # tables are built outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt_g.step()
    assert float(opt_g.step_count) == 0.0 and all_equal(pg, init)       # capturing ran nothing
    rates = []
    for epoch in range(6):
        gs = grads(epoch)
        for s, g in zip(static, gs):
            s.copy_(g)
        graph.replay()
        rates.append(opt_g.param_groups[0]["lr"])
        sch_g.step()                                                    # publishes the next epoch's rate, after the replay
        give(pe, gs)
        opt_e.step()
        sch_e.step()
        give(pt, gs)
        tn = torch.nn.utils.clip_grad_norm_(pt, 5.0)
        opt_t.step()
        sch_t.step()
        give(pc, gs)
        opt_c.step()
        assert all_equal(pg, pe) and all_equal(moments(opt_g), moments(opt_e)), epoch
        assert all_equal(static, [p.grad for p in pe]), epoch
        assert abs(opt_g.total_norm().item() - tn.item()) <= 1e-4 * tn.item()
        assert_close(pt, pg, what=f"epoch {epoch}")
        assert_close([p.grad for p in pt], static, atol=1e-7, what=f"grad, epoch {epoch}")
    assert rates == [1e-2, 1e-2, 5e-3, 2.5e-3, 1.25e-3, 6.25e-4] and float(opt_g.step_count) == 6.0
    # Adam moves an element by about lr per step: from the third epoch on the constant rate moves 1e-2 where the schedule moves
    # 5e-3 and less, so the two runs are apart by far more than the comparison tolerance
    apart = max((p - c).abs().max().item() for p, c in zip(pg, pc))
    assert apart > 1e-3, apart


@pytest.mark.gpu
def test_capture_with_a_stale_table_raises_and_leaves_the_optimizer_usable():
    from hrpe_amd.optim import FusedClipAdam
    init = initial(7)
    a, b = params_of(init), params_of(init)
    opt = FusedClipAdam(a, lr=1e-2, max_norm=5.0, device_hyper=True)
    ref = FusedClipAdam(b, lr=1e-2, max_norm=5.0)
    gs = grads(0)
    give(a, gs)
    give(b, gs)
    opt.step()
    ref.step()
    opt.param_groups[0]["lr"] = ref.param_groups[0]["lr"] = 5e-3        # what a scheduler does; nothing published yet
    assert opt.hyper_is_stale()
    give(a, grads(1))
    give(b, grads(1))
    opt.prepare()                                                        # new gradient tensors: the tables follow, outside the capture
    scratch = torch.zeros(4, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="publish_hyper"):
        with torch.cuda.graph(graph):
            scratch += 1                                                 # (the graph that is thrown away is not an empty one)
            opt.step()
    assert not torch.cuda.is_current_stream_capturing()
    with pytest.raises(RuntimeError, match="capture"):                   # the setter itself refuses to be captured
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            scratch += 1
            opt.publish_hyper()
    torch.cuda.synchronize()
    assert float(opt.step_count) == 1.0 and opt.hyper_is_stale()
    opt.step()                                                           # eager: publishes 5e-3, then steps
    ref.step()
    assert not opt.hyper_is_stale() and float(opt.step_count) == 2.0
    assert all_equal(a, b) and all_equal(moments(opt), moments(ref))


def two_groups(params):
    return [{"params": params[:3], "lr": 1e-2, "weight_decay": 0.0},
            {"params": params[3:], "lr": 3e-3, "weight_decay": 1e-2, "betas": (0.8, 0.99), "eps": 1e-6}]


@pytest.mark.gpu
def test_two_groups_with_weight_decay_match_torch_adam():
    """Global clip over both groups, per-group lr / betas / eps, L2 weight decay as torch.optim.Adam: the moments see
    g + weight_decay * p, the gradient written back is the clipped one without that term."""
    from hrpe_amd.optim import FusedClipAdam
    init = initial(9)
    ref, mine = [torch.nn.Parameter(t.clone()) for t in init], params_of(init)
    opt_ref = torch.optim.Adam(two_groups(ref), lr=1.0)
    opt = FusedClipAdam(two_groups(mine), lr=1.0, max_norm=5.0)
    assert len(opt.param_groups) == 2 and opt.param_groups[1]["betas"] == (0.8, 0.99) and opt.param_groups[0]["betas"] == (0.9, 0.999)
    for it in range(4):
        gs = grads(it)
        give(ref, gs)
        give(mine, gs)
        tn = torch.nn.utils.clip_grad_norm_(ref, 5.0)
        opt_ref.step()
        opt.step()
        assert abs(opt.total_norm().item() - tn.item()) <= 1e-4 * tn.item()
        coef = min(1.0, 5.0 / (tn.item() + 1e-6))
        assert (coef < 1.0) == (it % 2 == 0)                             # both sides of the clip are exercised
        assert_close([p.grad for p in ref], [q.grad for q in mine], atol=1e-7, what=f"grad {it}")
        assert_close([g * coef for g in gs], [q.grad for q in mine], atol=1e-7, what=f"clipped grad {it}")
        assert_close(ref, mine, what=f"param {it}")
    # the decay did act: the same run without it ends elsewhere in group 1 and at the same bits in group 0
    plain = params_of(init)
    groups = two_groups(plain)
    groups[1]["weight_decay"] = 0.0
    opt_plain = FusedClipAdam(groups, lr=1.0, max_norm=5.0)
    for it in range(4):
        give(plain, grads(it))
        opt_plain.step()
    assert all_equal(plain[:3], mine[:3])
    assert all((p - q).abs().max().item() > 1e-5 for p, q in zip(plain[3:], mine[3:]))


@pytest.mark.gpu
def test_two_group_checkpoint_interchange_with_torch_adam_and_resumed_schedule():
    """torch.optim.Adam (two groups, weight decay, a LambdaLR that left ``initial_lr``) -> torch.save / torch.load -> FusedClipAdam and
    back; training continues within tolerance on each side and a resumed get_scheduler gives the fixture's next rate."""
    from hrpe_amd.lib.utils.utils import get_scheduler
    from hrpe_amd.optim import FusedClipAdam
    gold = np.load(os.path.join(GOLDEN, "golden_lr_schedule.npz"))
    name = "exponential_panda"
    args = A({k.split(":cfg:")[1]: gold[k].item() for k in gold.files if k.startswith(name + ":cfg:")}, use_schedule=True)
    lr0, resume = float(gold["lr"]), int(gold["resume_epoch"])

    def groups(params):
        return [{"params": params[:3]}, {"params": params[3:], "lr": 0.3 * lr0, "weight_decay": 1e-2, "betas": (0.8, 0.99), "eps": 1e-6}]

    def run(opt, params, its):
        for it in its:
            give(params, grads(it, scale=0.1))
            opt.step()

    def through_file(obj):
        buf = io.BytesIO()
        torch.save(obj, buf)
        buf.seek(0)
        return torch.load(buf, map_location=DEV, weights_only=False)

    init = initial(11)
    ref = [torch.nn.Parameter(t.clone()) for t in init]
    opt_ref = torch.optim.Adam(groups(ref), lr=lr0)
    sch_ref = get_scheduler(args, opt_ref, -1)
    run(opt_ref, ref, range(3))
    for _ in range(resume):
        sch_ref.step()
    ckpt = through_file({"model": [p.detach().clone() for p in ref], "optimizer_state_dict": opt_ref.state_dict()})
    # torch -> FusedClipAdam
    mine = params_of(ckpt["model"])
    opt = FusedClipAdam(groups(mine), lr=1.0)                            # rates and decay come from the checkpoint
    opt.load_state_dict(ckpt["optimizer_state_dict"])
    g0, g1 = opt.param_groups
    assert g1["weight_decay"] == 1e-2 and g0["weight_decay"] == 0 and g1["betas"] == (0.8, 0.99) and float(opt.step_count) == 3.0
    assert g0["initial_lr"] == lr0 and g1["initial_lr"] == 0.3 * lr0
    np.testing.assert_allclose(g0["lr"], gold[f"{name}:lr"][resume - 1], rtol=1e-12)
    sch = get_scheduler(args, opt, resume)
    np.testing.assert_allclose([g0["lr"], g1["lr"]], [gold[f"{name}:resumed:lr0"], 0.3 * gold[f"{name}:resumed:lr0"]], rtol=1e-12)
    sch_ref2 = get_scheduler(args, opt_ref, resume)
    run(opt_ref, ref, range(3, 5))
    run(opt, mine, range(3, 5))
    assert_close(ref, mine, what="torch -> fused")
    sch.step()
    sch_ref2.step()
    np.testing.assert_allclose(opt.param_groups[0]["lr"], gold[f"{name}:resumed:lr"][0], rtol=1e-12)
    assert not opt.hyper_is_stale()                                      # the scheduler published
    # FusedClipAdam -> torch
    sd = opt.state_dict()
    assert len(sd["param_groups"]) == 2 and sd["param_groups"][1]["params"] == [3, 4, 5] and len(sd["state"]) == len(SHAPES)
    ckpt = through_file({"model": [p.detach().clone() for p in mine], "optimizer_state_dict": sd})
    back = [torch.nn.Parameter(t.clone()) for t in ckpt["model"]]
    opt_back = torch.optim.Adam(groups(back), lr=1.0)
    opt_back.load_state_dict(ckpt["optimizer_state_dict"])
    b0, b1 = opt_back.param_groups
    assert b1["weight_decay"] == 1e-2 and b1["initial_lr"] == 0.3 * lr0 and b0["initial_lr"] == lr0
    assert b0["lr"] == opt.param_groups[0]["lr"] and b1["lr"] == opt.param_groups[1]["lr"]
    run(opt, mine, range(5, 7))
    run(opt_back, back, range(5, 7))
    assert_close(back, mine, what="fused -> torch")
    # what the one-group class refuses stays refused there; amsgrad stays refused everywhere
    one = FusedClipAdam(params_of(init), lr=1e-3)
    with pytest.raises(ValueError):
        one.load_state_dict(sd)
    bad = opt.state_dict()
    bad["param_groups"][0]["amsgrad"] = True
    with pytest.raises(ValueError, match="amsgrad"):
        opt.load_state_dict(bad)
