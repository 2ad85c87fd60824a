"""Host side of gradient accumulation over micro-batches (no GPU): the hrp_grad_accumulate entry point is exported, bound with the
header's signature and validates its arguments before it launches; PlannedModule.set_grad_accumulation validates `steps`, keeps
per-module state and refuses the combination with enable_split_backward() - none of which touches a device."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

import hrpe_amd  # noqa: F401
from hrpe_amd import _native as nv
from hrpe_amd.runtime import PlannedModule


class _Leaf(PlannedModule):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(3))


class _Tree(PlannedModule):
    def __init__(self):
        super().__init__()
        self.a, self.b = _Leaf(), _Leaf()


def test_abi_symbol_and_ctypes_signature_match_the_header():
    assert hasattr(nv.lib(), "hrp_grad_accumulate")
    assert nv.PROTOTYPES["hrp_grad_accumulate"] == [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_void_p]
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hrp.h")).read(), flags=re.S)
    m = re.search(r"int\s+hrp_grad_accumulate\s*\(([^)]*)\)", src)
    assert m, "hrp_grad_accumulate is not declared in include/hrp.h"
    types = [re.sub(r"\s*\w+$", "", a.strip()) for a in m.group(1).split(",")]
    assert types == ["const float*", "float*", "int64_t", "int", "float", "void*"]
    fn = nv.lib().hrp_grad_accumulate
    assert fn.argtypes == nv.PROTOTYPES["hrp_grad_accumulate"] and fn.restype is C.c_int


def test_entry_point_rejects_bad_arguments_before_launching():
    fn = nv.lib().hrp_grad_accumulate
    assert fn(None, 1024, 8, 1, 1.0, None) == -1 and b"grad_accumulate" in nv.lib().hrp_last_error()
    assert fn(1024, None, 8, 0, 1.0, None) == -1
    assert fn(1024, 2048, 0, 0, 1.0, None) == -1
    assert fn(1024, 2048, -4, 0, 1.0, None) == -1
    assert fn(1028, 2048, 8, 0, 1.0, None) == -1 and b"aligned" in nv.lib().hrp_last_error()
    assert fn(1024, 2056, 8, 0, 1.0, None) == -1 and b"aligned" in nv.lib().hrp_last_error()
    assert fn(1024, 1024, 8, 0, 1.0, None) == -1 and b"same buffer" in nv.lib().hrp_last_error()


@pytest.mark.parametrize("steps", [0, -1, -8, 1.5, "2", None, True])
def test_steps_below_one_or_not_an_integer_raise(steps):
    m = _Tree()
    with pytest.raises(ValueError, match="steps"):
        m.set_grad_accumulation(steps)
    assert m._accum is None and m.a._accum is None


def test_mode_is_per_module_state_and_steps_1_restores_the_default():
    m = _Tree()
    assert m.accumulation_complete() and m.flat_grads() == []
    assert m.set_grad_accumulation(4, average=True) is m
    for sub in (m, m.a, m.b):
        assert sub._accum.steps == 4 and sub._accum.scale == 0.25 and sub._accum.index == 0 and sub._accum.buf is None
    assert m._accum is not m.a._accum and m.a._accum is not m.b._accum
    assert not m.accumulation_complete() and m.flat_grads() == []     # (the buffer is allocated by the first backward)
    m.set_grad_accumulation(3)
    assert m._accum.scale == 1.0 and m.a._accum.steps == 3
    m._accum.index = 3                                                # as after three backward passes
    assert m.accumulation_complete()
    assert m.begin_accumulation() is m and m._accum.index == 0 and not m.accumulation_complete()
    m.set_grad_accumulation(1)
    assert m._accum is None and m.a._accum is None and m.b._accum is None and m.accumulation_complete()
    m.begin_accumulation()                                            # a no-op in the default mode


def test_accumulation_with_split_backward_raises_and_names_both():
    m = _Tree()
    m.set_grad_accumulation(2)
    with pytest.raises(ValueError) as e:
        m.enable_split_backward()
    assert "enable_split_backward" in str(e.value) and "set_grad_accumulation" in str(e.value)
    with pytest.raises(ValueError):
        m.enable_split_backward(fracs=(0.25, 0.5))
    m.set_grad_accumulation(1)
    assert m.enable_split_backward() is None      # default mode again: no training plan yet, so no split - and no error
    # the other order: a plan with an active split (a stand-in: no device) refuses the mode, steps == 1 stays allowed
    import types
    m.b._plans["k"] = types.SimpleNamespace(plan=types.SimpleNamespace(split_active=True, need_grad=True, accum=None))
    with pytest.raises(ValueError) as e:
        m.set_grad_accumulation(2)
    assert "enable_split_backward" in str(e.value) and "set_grad_accumulation" in str(e.value)
    assert m._accum is None and m.b._accum is None
    m.set_grad_accumulation(1)


def test_reducer_skips_incomplete_cycles_without_a_process_group():
    from hrpe_amd.parallel import GradAllReducer
    m = _Tree()
    red = GradAllReducer(bucket_mb=1)
    assert red.reduce_module(m) is True           # default mode: every backward is complete
    m.set_grad_accumulation(2)
    assert red.reduce_module(m) is False
    m._accum.index = 2
    assert red.reduce_module(m) is True
