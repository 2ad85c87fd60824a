"""CPU-only checks of the learning-rate schedule and of the host side of the group-table Adam step:
``hrpe_amd.lib.utils.utils.get_scheduler`` against the rates the reference's own function produced (tests/golden/golden_lr_schedule.npz,
written by tests/golden/gen_golden_schedule.py), the C layout of ``hrp_opt_group``, and the refusals of ``hrp_opt_adam_step_groups`` /
``hrp_opt_set_group``, which validate on the host before they launch."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

import hrpe_amd  # noqa: F401
from hrpe_amd import _native as nv

SCHEDULES = ["exponential_panda", "exponential_orb", "linear_depthnet", "everyXepoch"]


class A(dict):
    __getattr__ = dict.__getitem__


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "golden_lr_schedule.npz"))


def schedule_args(golden, name):
    keys = [k.split(":cfg:")[1] for k in golden.files if k.startswith(name + ":cfg:")]
    a = A({k: golden[f"{name}:cfg:{k}"].item() for k in keys}, use_schedule=True)
    return a, a.pop("steps")


def adam(lr):
    return torch.optim.Adam([torch.nn.Parameter(torch.zeros(3))], lr=lr)


@pytest.mark.parametrize("name", SCHEDULES)
def test_get_scheduler_reproduces_the_reference_rates(golden, name):
    """Every recorded rate, fresh and resumed at epoch 50 from a state dict with ``initial_lr``, to rtol 1e-12: both sides are
    the same few double operations (lib/utils/utils.py:147-189)."""
    from hrpe_amd.lib.utils.utils import get_scheduler
    args, steps = schedule_args(golden, name)
    lr, resume = float(golden["lr"]), int(golden["resume_epoch"])
    assert len(golden[f"{name}:lr"]) == steps
    opt = adam(lr)
    sched = get_scheduler(args, opt, -1)
    assert isinstance(sched, torch.optim.lr_scheduler.LambdaLR)
    np.testing.assert_allclose(opt.param_groups[0]["lr"], golden[f"{name}:lr0"], rtol=1e-12, atol=0)
    got, saved = [], None
    for e in range(max(steps, resume)):
        opt.step()
        sched.step()
        got.append(opt.param_groups[0]["lr"])
        if e + 1 == resume:
            saved = opt.state_dict()
    np.testing.assert_allclose(got[:steps], golden[f"{name}:lr"], rtol=1e-12, atol=0)
    assert sched.get_last_lr() == [got[-1]]
    opt2 = adam(1.0)
    opt2.load_state_dict(saved)
    sched2 = get_scheduler(args, opt2, resume)
    np.testing.assert_allclose(opt2.param_groups[0]["lr"], golden[f"{name}:resumed:lr0"], rtol=1e-12, atol=0)
    got2 = []
    for _ in golden[f"{name}:resumed:lr"]:
        opt2.step()
        sched2.step()
        got2.append(opt2.param_groups[0]["lr"])
    assert len(got2) >= 5
    np.testing.assert_allclose(got2, golden[f"{name}:resumed:lr"], rtol=1e-12, atol=0)


def test_get_scheduler_scales_every_group_and_returns_none_without_a_schedule(golden):
    from hrpe_amd.lib.utils.utils import get_scheduler
    assert get_scheduler(A(use_schedule=False), adam(1e-4), -1) is None
    args, _ = schedule_args(golden, "exponential_panda")
    a, b = torch.nn.Parameter(torch.zeros(2)), torch.nn.Parameter(torch.zeros(2))
    opt = torch.optim.Adam([{"params": [a]}, {"params": [b], "lr": 3e-5}], lr=1e-4)
    sched = get_scheduler(args, opt, -1)
    for _ in range(60):
        opt.step()
        sched.step()
    want = golden["exponential_panda:lr"][59]
    np.testing.assert_allclose([g["lr"] for g in opt.param_groups], [want, want * 0.3], rtol=1e-12, atol=0)


def test_get_scheduler_unknown_schedule_type_behaves_as_the_reference(golden):
    """The reference reaches its return statement with the name unbound; the fixture recorded the exception's name."""
    from hrpe_amd.lib.utils.utils import get_scheduler
    assert str(golden["unknown_schedule_type"]) == "UnboundLocalError"
    with pytest.raises(UnboundLocalError):
        get_scheduler(A(use_schedule=True, schedule_type="cosine"), adam(1e-4), -1)


def test_scheduler_publishes_to_an_optimizer_that_asks_for_it():
    """The returned scheduler ends ``step()`` with ``optimizer.publish_hyper()`` where the optimizer has one - with the new rate
    already in ``param_groups`` - and leaves a plain ``torch.optim.Adam`` alone."""
    from hrpe_amd.lib.utils.utils import get_scheduler

    class Publishing(torch.optim.Adam):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.published = []

        def publish_hyper(self):
            self.published.append(self.param_groups[0]["lr"])

    args = A(use_schedule=True, schedule_type="exponential", n_epochs_warmup=0, start_decay=1, end_decay=100, exponent=0.5)
    opt = Publishing([torch.nn.Parameter(torch.zeros(3))], lr=1e-2)
    sched = get_scheduler(args, opt, -1)
    assert opt.published == [1e-2]                     # LambdaLR's constructor takes the first step
    for _ in range(3):
        opt.step()
        sched.step()
    assert opt.published == [1e-2, 1e-2, 5e-3, 2.5e-3]


def test_opt_group_struct_size_matches_c():
    """Compile a tiny C program against include/hrp.h and compare sizeof(hrp_opt_group) with the ctypes mirror (32 bytes)."""
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "hrp.h"
int main(void) {
  printf("%zu %zu %zu\n", sizeof(hrp_opt_group), offsetof(hrp_opt_group, weight_decay), offsetof(hrp_opt_group, reserved));
  return 0;
}'''
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "s.c"), "w").write(prog)
        exe = os.path.join(td, "s")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "s.c"), "-o", exe], check=True)
        out = [int(v) for v in subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert out == [C.sizeof(nv.OptGroup), nv.OptGroup.weight_decay.offset, nv.OptGroup.reserved.offset] == [32, 16, 20]


def test_group_entry_points_reject_bad_arguments_without_a_gpu():
    """hrp_opt_adam_step_groups / hrp_opt_set_group return -1 with a text for null tables, ngroups < 1, an index outside
    [0, ngroups) and clipping without slots; nothing is launched (the pointers below are never dereferenced)."""
    lib = nv.lib()
    P = 0x1000                                          # any non-null address

    def step(tensors=P, chunks=P, nchunks=1, slots=P, max_norm=5.0, step_dev=P, groups=P, ngroups=1, tensor_group=P):
        return lib.hrp_opt_adam_step_groups(tensors, chunks, nchunks, slots, max_norm, step_dev, groups, ngroups, tensor_group, None)

    for bad in (dict(tensors=None), dict(chunks=None), dict(step_dev=None), dict(nchunks=0)):
        assert step(**bad) == -1 and b"opt_adam_step_groups: bad args" in lib.hrp_last_error(), bad
    for bad in (dict(groups=None), dict(tensor_group=None)):
        assert step(**bad) == -1 and b"null group table" in lib.hrp_last_error(), bad
    for n in (0, -3):
        assert step(ngroups=n) == -1 and b"ngroups" in lib.hrp_last_error() and b"< 1" in lib.hrp_last_error()
    assert step(slots=None) == -1 and b"clipping needs the sum-of-squares slots" in lib.hrp_last_error()

    def put(groups=P, ngroups=2, index=0):
        return lib.hrp_opt_set_group(groups, ngroups, index, 1e-3, 0.9, 0.999, 1e-8, 0.0, None)

    assert put(groups=None) == -1 and b"null group table" in lib.hrp_last_error()
    assert put(ngroups=0) == -1 and b"ngroups" in lib.hrp_last_error()
    for i in (-1, 2, 7):
        assert put(index=i) == -1 and b"outside [0, 2)" in lib.hrp_last_error(), i
    with pytest.raises(nv.HrpError, match="outside"):
        nv.call("hrp_opt_set_group", P, 2, 2, 1e-3, 0.9, 0.999, 1e-8, 0.0, None)
