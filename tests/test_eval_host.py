"""Host-side checks of the validation pass: the hrp_eval_desc mirror, the reference's signatures, option errors (no GPU needed)."""
import ctypes as C
import inspect
import os
import subprocess
import tempfile

import pytest

from conftest import ROOT
from hrpe_amd import _native as nv


class Args(dict):
    __getattr__ = dict.__getitem__


def test_eval_desc_size_matches_c():
    """Compile a tiny C program against include/hrp.h and compare sizeof(hrp_eval_desc) with the ctypes mirror."""
    prog = '#include <stdio.h>\n#include "hrp.h"\nint main(void) { printf("%zu\\n", sizeof(hrp_eval_desc)); return 0; }\n'
    with tempfile.TemporaryDirectory() as td:
        with open(os.path.join(td, "s.c"), "w") as fh:
            fh.write(prog)
        exe = os.path.join(td, "s")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(td, "s.c"), "-o", exe], check=True)
        size = int(subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout)
    assert size == C.sizeof(nv.EvalDesc)
    names = [n for n, _ in nv.EvalDesc._fields_]
    assert names[:9] == list(nv.EvalDesc.INPUTS) and len(nv.EvalDesc.PER_IMAGE) == 11 and len(nv.EvalDesc.PER_BATCH) == 6


def test_eval_batch_rejects_bad_descriptors_without_a_gpu():
    """Null pointers, B == 0, rot_dim outside {4, 6} and a batch past the capacity are HRP_ERR_ARG before anything launches."""
    lib = nv.lib()
    assert lib.hrp_eval_batch(None, None) == -1
    d = nv.EvalDesc()
    assert lib.hrp_eval_batch(C.byref(d), None) == -1 and b"null" in lib.hrp_last_error()
    for n, _ in nv.EvalDesc._fields_[:26]:
        setattr(d, n, 64)                                   # never dereferenced: every case below fails validation
    d.nkp, d.dof, d.rot_dim, d.root, d.capacity, d.batch_capacity = 7, 8, 6, 3, 16, 2
    assert lib.hrp_eval_batch(C.byref(d), None) == -1 and b"B=0" in lib.hrp_last_error()
    d.B, d.rot_dim = 4, 9
    assert lib.hrp_eval_batch(C.byref(d), None) == -1 and b"rot_dim=9" in lib.hrp_last_error()
    d.rot_dim, d.offset = 6, 13
    assert lib.hrp_eval_batch(C.byref(d), None) == -1 and b"capacity" in lib.hrp_last_error()
    d.offset, d.batch_index = 12, 2
    assert lib.hrp_eval_batch(C.byref(d), None) == -1 and b"batch 2" in lib.hrp_last_error()
    d.batch_index, d.root = 0, 7
    assert lib.hrp_eval_batch(C.byref(d), None) == -1 and b"root=7" in lib.hrp_last_error()


def test_step_functions_keep_the_reference_signatures():
    from hrpe_amd.lib.core.function import farward_loss, validate
    p = list(inspect.signature(farward_loss).parameters.values())
    assert [q.name for q in p[:7]] == ["args", "input_batch", "model", "robot", "device", "device_id", "train"]
    assert p[6].default is True and all(q.default is not inspect.Parameter.empty for q in p[7:])
    assert list(inspect.signature(validate).parameters) == ["args", "epoch", "dsname", "loader", "model", "robot", "writer", "device",
                                                            "device_id"]


@pytest.mark.parametrize("option", [dict(pose_loss_func="l1"), dict(rot_loss_func="mat_mse"), dict(trans_loss_func="mse"),
                                    dict(fix_mask=True)])
def test_unsupported_loss_options_raise_before_the_device_is_touched(option):
    """The model, the batch and the robot are None: an option the fused loss does not cover is refused before any of them is used."""
    from hrpe_amd.lib.core.function import SHIPPED_LOSS_FUNCS, farward_loss
    args = Args(SHIPPED_LOSS_FUNCS, fix_mask=False)
    args.update(option)
    with pytest.raises(NotImplementedError, match=next(iter(option))):
        farward_loss(args, None, None, None, "cuda:0", [0], train=False)
