"""CPU-only checks around the key-point read-out (csrc/kp_readout.hip): the float64 oracle (tests/kp_readout_oracle.py) against the
reference's own ``KeypointUpSample`` + ``SpatialSoftArgmax`` as recorded in tests/golden/golden_kp_readout.npz, the exactness
argument of the test operands, and the argument checks of the entry points (which refuse before they launch)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hrpe_amd  # noqa: E402,F401
from hrpe_amd import _native as nv  # noqa: E402
import kp_readout_oracle as O  # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "golden_kp_readout.npz"))
SCALE = np.array([O.SIZE[0] // 2, O.SIZE[1] // 2], np.float64)


def fixture_cases():
    return O.all_cases(int(GOLD["strip"]))


def test_oracle_equals_the_reference_fixture():
    """5e-6 * scale: the reference computes the soft-argmax in fp32 (its own error against float64 is 1.3e-7 normalised, printed
    by the generator); the recorded maximum of its fp32 heat-map equals the float64 one exactly."""
    assert np.array_equal(GOLD["lim"], np.array(O.LIM, np.float32)) and tuple(GOLD["size"]) == O.SIZE
    for shape, spikes in fixture_cases():
        k = O.key(shape, spikes)
        assert tuple(GOLD[k + "_shape"]) == shape and int(GOLD[k + "_seed"]) == O.seed_of(shape, spikes)
        x, w, b, s = O.operands(shape, spikes)
        assert s == int(GOLD[k + "_s"])
        want = O.readout64(x, w, b)
        err = np.abs(want["kp"].numpy() - GOLD[k + "_kp"].astype(np.float64)) / SCALE
        assert err.max() <= 5e-6, (k, err.max())
        assert np.array_equal(want["max"].numpy(), GOLD[k + "_heat_max"].astype(np.float64)), k


def test_operands_are_exact_in_both_element_types():
    """Every operand survives bf16, and every logit is an integer below 2^24 in units of 2^-s: the premise of the exact gates."""
    for shape, spikes in fixture_cases():
        x, w, b, s = O.operands(shape, spikes)
        for t in (x, w):
            assert torch.equal(t.to(torch.bfloat16).double(), t)
        assert torch.equal(b * 4, (b * 4).round())
        heat = O.readout64(x, w, b)["heat"]
        units = heat * 2.0 ** max(s, 2)
        assert torch.equal(units, units.round()) and float(units.abs().max()) < 2 ** 24
        assert float((x.abs().amax())) <= 2 and float((w.abs().amax())) <= 2 * 2.0 ** -s
    for shape in O.SPIKE_SHAPES:
        x, w, b, _ = O.operands(shape, True)
        heat = O.readout64(x, w, b)["heat"]
        k = shape[2]
        last, first = heat[:, 0].flatten(1), heat[:, k - 1].flatten(1)
        assert bool((last.argmax(1) == last.shape[1] - 1).all()) and bool((first.argmax(1) == 0).all())
        assert float((last[:, -1] - last[:, :-1].amax(1)).min()) >= 40 and float((first[:, 0] - first[:, 1:].amax(1)).min()) >= 40
    assert float(O.readout64(*O.operands(O.SHAPES[0])[:3])["pmax"].max()) > 0.96


def _fwd_args(**over):
    """Arguments of hrp_kp_readout_fwd that pass every host check (the pointers are never followed on the host)."""
    a = dict(x=256, dtype=nv.HRP_BF16, B=1, Hin=6, Win=8, Cin=2048, pitch=2048, packed=256, bias=64, k=7, lim0=-1.0, lim2=-1.0, sx=320.0,
             sy=240.0, kp=64, ms=None, ws=64, ws_bytes=1 << 20, stream=None)
    a.update(over)
    return list(a.values())


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = nv.lib()
    bad = [dict(x=None), dict(packed=None), dict(bias=None), dict(kp=None), dict(ws=None), dict(Cin=2040), dict(Cin=16), dict(Cin=0),
           dict(k=0), dict(k=33), dict(k=-1), dict(B=0), dict(Hin=0), dict(Win=0), dict(Hin=4097), dict(pitch=2047), dict(pitch=2044),
           dict(x=260), dict(dtype=3), dict(ws_bytes=8), dict(dtype=nv.HRP_F32, pitch=2050)]
    for over in bad:
        assert lib.hrp_kp_readout_fwd(*_fwd_args(**over)) == -1, over
        assert b"kp_readout_fwd" in lib.hrp_last_error(), over
    for over in [dict(w=None), dict(out=None), dict(Cin=48), dict(k=0), dict(k=33), dict(dtype=7)]:
        a = dict(w=64, Cin=64, k=7, out=64, dtype=nv.HRP_F32, stream=None)
        a.update(over)
        assert lib.hrp_kp_readout_pack(*a.values()) == -1, over
        assert b"kp_readout_pack" in lib.hrp_last_error(), over
    with pytest.raises(nv.HrpError):
        nv.call("hrp_kp_readout_fwd", *_fwd_args(k=33))
    strips = -(-9 // nv.KP_STRIP_ROWS)
    assert lib.hrp_kp_readout_ws(3, 9) == 3 * strips * 32 * 16 and lib.hrp_kp_readout_ws(0, 9) == 0
    assert nv.KP_STRIP_ROWS >= 1 and nv.TRACK_MAX_KP == 32
