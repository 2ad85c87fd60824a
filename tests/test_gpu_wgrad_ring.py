"""GPU tests of the tile ring of the eight-wave weight-gradient program (csrc/conv_wgrad.hip: conv_wgrad_octo_body - the 64 x 64
arrangement keeps two tiles of DMA in flight in three stage buffers and waits with a counted vmcnt; the 32 x 32 arrangement keeps
its two buffers).  What can go wrong is the ring's start (one or two tiles in the prologue), its wrap (the fourth tile reuses the
first buffer) and its tail (the last tiles wait for everything), so the batches are chosen by TILES PER WORKGROUP: the tests work
that number out from the plan (G partial slabs per problem, from the workspace size) and the shape, and require that workgroups
with exactly 1, 2, 3 and at least 5 tiles, and problems whose workgroups get different counts, have all been run.

Through the C ABI's batched launch as tests/test_gpu_wgrad8.py does, against torch's conv2d weight gradient in float64 on the same
bf16 operands (exact bf16 products, fp32 accumulation: 2e-5 of the range).  Every batch is launched twice into fresh outputs and
the two results must be equal bit for bit: a stage buffer reused too early shows up there or against the reference."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-5

# N, H, W (the OUTPUT map), cin, cout, stride
BATCHES = {
    "wrap": [(16, 64, 64, 64, 64, 1), (6, 20, 24, 64, 128, 1), (5, 8, 8, 256, 256, 1)],
    "start": [(8, 64, 64, 64, 64, 1), (4, 32, 32, 128, 128, 1), (3, 16, 16, 128, 256, 2)],
    "single": [(4, 64, 64, 64, 64, 1), (3, 64, 64, 32, 32, 1), (2, 40, 24, 32, 32, 1)],
    "long": [(16, 64, 64, 64, 64, 1), (3, 16, 16, 128, 256, 2), (2, 40, 24, 32, 32, 1)],
}
_cache = {}


def _operands(name):
    """The operands and the float64 reference of a batch, made once and never written to."""
    if name not in _cache:
        out = []
        for i, (N, H, W, cin, cout, st) in enumerate(BATCHES[name]):
            g = torch.Generator(device="cpu").manual_seed(7000 + 10 * len(_cache) + i)
            x = torch.randn(N, H * st, W * st, cin, generator=g).to(torch.bfloat16).to(DEV).contiguous()
            dy = (torch.randn(N, H, W, cout, generator=g) / 8).to(torch.bfloat16).to(DEV).contiguous()
            ref = torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2), (cout, cin, 3, 3), dy.double().permute(0, 3, 1, 2),
                                              stride=st, padding=1).reshape(cout, cin, 9)
            out.append((x, dy, ref))
        _cache[name] = out
    return _cache[name]


def _ntiles(N, H, W, cin, cout, st):
    """wgrad_tiling_octo: pixels per tile 512 (32 x 32 arrangement), 128, or 64 (stride 2); tile = TI images x TH x TW"""
    BM = 512 if (cin == 32 and cout == 32) else (64 if st == 2 else 128)
    TW = 1
    while TW < W and TW < 16:
        TW *= 2
    TH = 1
    while TH < H and TH * TW < BM:
        TH *= 2
    TI = min(BM // (TW * TH), N)
    return -(-W // TW) * -(-H // TH) * -(-N // TI)


def _tiles_per_workgroup(info, name):
    """Per problem: the set of tile counts of its workgroups (workgroup g walks tiles g, g + G, ...)."""
    res = []
    for i, s in enumerate(BATCHES[name]):
        fold_pairs = (s[4] // 32) * (s[3] // 32)
        G = int(info.ws_bytes[i]) // (fold_pairs * 9 * 4096)
        nt = _ntiles(*s)
        assert 1 <= G <= nt
        res.append({(nt - 1 - g) // G + 1 for g in range(G)})
    return res


def _run(nv, name, phase, accumulate, fill):
    """One batched launch (+ the deferred fold for phase 1) into fresh outputs -> (dws, info)."""
    L = nv.lib()
    ops = _operands(name)
    n = len(ops)
    arr = (nv.WgradDesc * n)()
    dws, wss = [], []
    for d, (x, dy, _), (N, H, W, cin, cout, st) in zip(arr, ops, BATCHES[name]):
        d.x, d.dy, d.dtype = x.data_ptr(), dy.data_ptr(), nv.HRP_BF16
        d.N, d.H, d.W, d.Cin, d.x_pitch = N, H * st, W * st, cin, cin
        d.Ho, d.Wo, d.Cout, d.dy_pitch = H, W, cout, cout
        d.in_stride, d.ntaps = st, 9
        for i, (a, b) in enumerate([(ky - 1, kx - 1) for ky in range(3) for kx in range(3)]):
            d.dy_t[i], d.dx_t[i] = a, b
        d.dw_cin, d.phase, d.accumulate = cin, phase, accumulate
        dws.append(torch.full((cout * cin * 9,), fill, device=DEV))
        d.dw = dws[-1].data_ptr()
    info = nv.BatchInfo()
    nv.check(L.hrp_batch_prepare(nv.BATCH_WGRAD, arr, n, None, C.byref(info)), "query")
    for i, d in enumerate(arr):
        ws = torch.full((int(info.ws_bytes[i]) // 4 + 4,), float("nan"), device=DEV)      # a slab element no workgroup writes folds as NaN
        d.workspace, d.workspace_bytes = ws.data_ptr(), int(info.ws_bytes[i])
        wss.append(ws)
    host = (C.c_char * int(L.hrp_batch_table_bytes(nv.BATCH_WGRAD, n)))()
    nv.check(L.hrp_batch_prepare(nv.BATCH_WGRAD, arr, n, host, C.byref(info)), "prepare")
    assert info.grid == 0 and info.grid3 > 0, "every problem of these batches runs the eight-wave program"
    assert info.lds_bytes3 <= 160 * 1024
    tab = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(DEV)
    nv.check(L.hrp_batch_launch(tab.data_ptr(), C.byref(info), None), "launch")
    if phase == 1:
        folds = (nv.WgradFoldDesc * n)()
        nv.check(L.hrp_batch_wgrad_fold_descs(host, C.byref(info), folds), "fold descs")
        finfo = nv.BatchInfo()
        fhost = (C.c_char * int(L.hrp_batch_table_bytes(nv.BATCH_WGRAD_FOLD, n)))()
        nv.check(L.hrp_batch_prepare(nv.BATCH_WGRAD_FOLD, folds, n, fhost, C.byref(finfo)), "fold prepare")
        ftab = torch.frombuffer(bytearray(bytes(fhost)), dtype=torch.uint8).to(DEV)
        nv.check(L.hrp_batch_launch(ftab.data_ptr(), C.byref(finfo), None), "fold launch")
    torch.cuda.synchronize()
    return dws, info


def _check(nv, name, phase, accumulate=0, fill=3.0):
    first, info = _run(nv, name, phase, accumulate, fill)
    again, _ = _run(nv, name, phase, accumulate, fill)
    counts = _tiles_per_workgroup(info, name)
    for s, (x, dy, ref), a, b, c in zip(BATCHES[name], _operands(name), first, again, counts):
        want = ref + fill if accumulate else ref
        err = float((a.view(s[4], s[3], 9).double() - want).abs().max() / want.abs().max())
        print(f"{name} phase {phase} {s}: tiles per workgroup {sorted(c)}, error {err:.2e} of the range")
        assert torch.equal(a, b), f"{name} {s}: two launches of the same batch differ (tiles per workgroup {sorted(c)})"
        assert err < TOL, f"{name} {s}: weight gradient off by {err:.2e} of its range (tiles per workgroup {sorted(c)})"
    return counts


@pytest.mark.parametrize("phase", [0, 1])
def test_ring_start_wrap_and_tail(phase):
    """All four batches, phase 0 (fold in the same launch sequence) and phase 1 (deferred fold).  The coverage assertions look at
    the problems of the ring (multiples of 64 channels) only."""
    from hrpe_amd import _native as nv
    seen, uneven, seen32 = set(), 0, set()
    for name in BATCHES:
        for s, c in zip(BATCHES[name], _check(nv, name, phase)):
            if s[3] == 32:
                seen32 |= c
                continue
            seen |= c
            uneven += len(c) > 1
    assert {1, 2, 3} <= seen and max(seen) >= 5, f"ring problems ran {sorted(seen)} tiles per workgroup: start, wrap or tail missing"
    assert uneven >= 1, "no ring problem whose workgroups get different tile counts"
    assert {1, 2} <= seen32 and max(seen32) >= 4, f"32-channel problems ran {sorted(seen32)} tiles per workgroup"


def test_ring_accumulates_into_dw():
    """accumulate = 1: the fold adds to what dw holds."""
    from hrpe_amd import _native as nv
    _check(nv, "wrap", 0, accumulate=1, fill=0.5)
