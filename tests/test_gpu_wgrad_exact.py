"""Exact-arithmetic tests of every weight-gradient kernel path (csrc/conv_wgrad.hip) through the C ABI: the four-wave program
conv_wgrad_body<T, NT, NKS, NB>, the eight-wave bf16 and fp32x3 programs, the fp32 atomics path and the fold, as single launches,
batched launches and phase-1 launches folded by a HRP_BATCH_WGRAD_FOLD launch.

The cases, the paths of each and the configuration the launcher must choose for it are tests/wgrad_exact_cases.py (what the table
reaches is asserted without a GPU in tests/test_wgrad_exact_host.py).  Operands are non-zero integers of the case's value class
(tests/conv_exact_oracle.py), so every product and every partial sum - per wave, per slab, per atomic, in the fold - is an integer
below 2^24, the float64 oracle evaluate_wgrad is exact, and the whole dw buffer is compared with torch.equal.  Around the operands:

  x channels at or beyond dw_cin, dy channels at or beyond Cout       NaN (the lanes include/hrp.h promises are masked at the store)
  dw, at the oracle's full [Cout][dw_cin][T]                          the sentinel 7.0 (accumulate = 0) or integers in [-3, 3]
  workspace, exactly the bytes the library asks for                   NaN: a slab element no workgroup writes folds as NaN
  guard behind the workspace                                          5.0, must come back unchanged

Right before its launch every test asks hrp_wgrad_config_of / hrp_batch_wgrad_configs what will run and requires the table's answer.
In phase 1 dw must be bit-unchanged before the fold.

Measured on an MI355X (wall time of the test call, float64 oracle included): the slowest case is the first one, 0.30 s with the library's
first launch in it; the heaviest, the eight-wave bf16 batch with its 12 x 32 x 32 image 128 -> 128 companion (1.8e9 multiply-adds),
takes 0.05 s; every other case 0.03 s or less; the whole module (199 tests) 3.0 - 3.7 s."""
import ctypes as C
import zlib

import pytest
import torch

import conv_exact_oracle as O
import wgrad_exact_cases as T
from conv_exact_oracle import F64
from test_gpu_rowconv import DEV, nvmod

pytestmark = pytest.mark.gpu
SENTINEL, GUARD_VALUE, GUARD = 7.0, 5.0, 1024
_cache = {}


def tdtype(dt):
    return torch.bfloat16 if dt == "bf16" else torch.float32


def operands(case, i, p):
    """Problem i of a case: max|x|, max|dy|, the device copies of the operands with their NaN lanes, the oracle's gradient and written
    mask - made once, never written."""
    key = (case.name, i)
    if key not in _cache:
        g = torch.Generator(device="cpu").manual_seed(zlib.crc32(f"{case.name}/{i}".encode()))
        x, dy = O.wgrad_operands(g, p.dt, p.split, p.N, p.H, p.W, p.Cc, p.Ho, p.Wo, p.Cout)
        if p.dt != "bf16":
            O.assert_value_class(x, p.split == "x", f"{case.name}: x")
            O.assert_value_class(dy, p.split == "dy", f"{case.name}: dy")
        else:
            O.assert_value_class(x, False, f"{case.name}: x")
            O.assert_value_class(dy, False, f"{case.name}: dy")
        xd = torch.full((p.N, p.H, p.W, p.x_pitch), float("nan"), dtype=F64)
        xd[..., :p.Cc] = x
        dyd = torch.full((p.N, p.Ho, p.Wo, p.dy_pitch), float("nan"), dtype=F64)
        dyd[..., :p.Cout] = dy
        grad, wr = O.evaluate_wgrad(T.fill(p, 0, 0, 0, 0), x, dy)
        _cache[key] = (x.abs().max(), dy.abs().max(), xd.to(tdtype(p.dt)).to(DEV), dyd.to(tdtype(p.dt)).to(DEV), grad, wr)
    return _cache[key]


def workspace(nbytes):
    """NaN-filled workspace of exactly nbytes with a guard behind it."""
    assert nbytes % 4 == 0
    ws = torch.full((nbytes // 4 + GUARD,), GUARD_VALUE, dtype=torch.float32, device=DEV)
    ws[:nbytes // 4] = float("nan")
    return ws


def check_guard(ws, nbytes, what):
    assert bool((ws[nbytes // 4:] == GUARD_VALUE).all()), f"{what}: the launch wrote behind its workspace"


def check_equal(got, want, what):
    """torch.equal on dw [Cout, dw_cin, T], with the count and the first differing (co, ci, tap) when it fails."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    i = tuple(bad[0].tolist())
    msg = (f"{what}: {len(bad)} of {got.numel()} elements differ; first at (co, ci, tap) = {i}: got {got[i].item()}, "
           f"oracle {want[i].item()}")
    print(msg)
    raise AssertionError(msg)


def fold(nv, folds, what):
    """One HRP_BATCH_WGRAD_FOLD launch of the given fold descriptors."""
    L = nv.lib()
    n = len(folds)
    arr = (nv.WgradFoldDesc * n)(*folds)
    info = nv.BatchInfo()
    host = (C.c_char * int(L.hrp_batch_table_bytes(nv.BATCH_WGRAD_FOLD, n)))()
    nv.check(L.hrp_batch_prepare(nv.BATCH_WGRAD_FOLD, arr, n, host, C.byref(info)), f"{what}: fold prepare")
    tab = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(DEV)
    nv.check(L.hrp_batch_launch(tab.data_ptr(), C.byref(info), None), f"{what}: fold launch")
    torch.cuda.synchronize()


def run(nv, case, path):
    L = nv.lib()
    ps = T.problems(case, path)
    want_cfg = T.expected(case, path)
    ops = [operands(case, i, p) for i, p in enumerate(ps)]
    acc = int(path in ("S-ws1", "S-atom1"))
    phase = int(path.endswith("ph1"))
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(f"{case.name}/{path}".encode()))
    # dw buffers (one per problem, or one for all tap groups) and what they must hold afterwards
    nbuf = 1 if case.shared else len(ps)
    dw0 = [O.signed(g, (ps[i].Cout, ps[i].dw_cin, ps[i].T), (1, 2, 3)) if acc else torch.full((ps[i].Cout, ps[i].dw_cin, ps[i].T), SENTINEL, dtype=F64)
           for i in range(nbuf)]
    want = [d.clone() for d in dw0]
    for i, (p, (xmax, dymax, _, _, grad, wr)) in enumerate(zip(ps, ops)):
        b = 0 if case.shared else i
        O.assert_wgrad_exact(xmax, dymax, want[b], p.pixels)                      # precondition, on the operands alone
        want[b][wr] = grad[wr] + (want[b][wr] if acc else 0)
    dws = [d.float().to(DEV) for d in dw0]
    descs = [T.fill(p, o[2].data_ptr(), o[3].data_ptr(), dws[0 if case.shared else i].data_ptr(), acc, phase) for i, (p, o) in enumerate(zip(ps, ops))]
    wss = []
    if path.startswith("B"):
        def alloc(i, nbytes):
            wss.append((workspace(nbytes), nbytes))
            return wss[-1][0].data_ptr()
        arr, info, host, cfgs = T.prepare_batch(descs, alloc)
        assert cfgs == want_cfg, f"{case.name} {path}: the launcher chose {cfgs}, the table expects {want_cfg}"
        tab = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(DEV)
        nv.check(L.hrp_batch_launch(tab.data_ptr(), C.byref(info), None), "hrp_batch_launch")
        torch.cuda.synchronize()
        if phase:
            for d, d0 in zip(dws, dw0):
                assert torch.equal(d.cpu().double(), d0), f"{case.name} {path}: phase 1 touched dw"
            folds = (nv.WgradFoldDesc * len(ps))()
            nv.check(L.hrp_batch_wgrad_fold_descs(host, C.byref(info), folds), "hrp_batch_wgrad_fold_descs")
            fold(nv, list(folds), case.name)
    else:
        for d, cfg in zip(descs, want_cfg):
            if not path.startswith("S-atom"):
                nbytes = int(L.hrp_wgrad_workspace_bytes(C.byref(d)))
                assert nbytes > 0
                wss.append((workspace(nbytes), nbytes))
                d.workspace, d.workspace_bytes = wss[-1][0].data_ptr(), nbytes
            got_cfg = T.config_of(d)
            assert got_cfg == cfg, f"{case.name} {path}: the launcher chose {got_cfg}, the table expects {cfg}"
            nv.check(L.hrp_conv2d_bwd_weight(C.byref(d), None), "hrp_conv2d_bwd_weight")
            torch.cuda.synchronize()
            if phase:
                assert torch.equal(dws[0].cpu().double(), dw0[0]), f"{case.name} {path}: phase 1 touched dw"
                f = nv.WgradFoldDesc()
                nv.check(L.hrp_wgrad_fold_desc_of(C.byref(d), C.byref(f)), "hrp_wgrad_fold_desc_of")
                assert f.G == cfg.G
                fold(nv, [f], case.name)
    torch.cuda.synchronize()
    for i, (d, w) in enumerate(zip(dws, want)):
        check_equal(d.cpu().double(), w, f"{case.name} {path} dw[{i}]")
    for ws, nbytes in wss:
        check_guard(ws, nbytes, f"{case.name} {path}")


@pytest.mark.parametrize("case,path", T.gpu_cases(), ids=[f"{c.name}-{p}" for c, p in T.gpu_cases()])
def test_wgrad_exact(case, path):
    run(nvmod(), case, path)


def test_tap_group_without_workspace_must_accumulate():
    """accumulate = 0 zeroes the whole dw before the atomics: refused for a tap group, by the launch and by the query alike."""
    nv = nvmod()
    case = next(c for c in T.TABLE if c.name == "stem_b_g1")
    p = case.prob
    _, _, xd, dyd, _, _ = operands(case, 0, p)
    dw = torch.full((p.Cout, p.dw_cin, p.T), SENTINEL, device=DEV)
    d = T.fill(p, xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), 0)
    assert nv.lib().hrp_conv2d_bwd_weight(C.byref(d), None) == -1 and b"a tap group without a workspace must accumulate" in nv.lib().hrp_last_error()
    with pytest.raises(nv.HrpError, match="a tap group without a workspace must accumulate"):
        T.config_of(d)
    torch.cuda.synchronize()
    assert bool((dw == SENTINEL).all())
