"""What tests/wgrad_exact_cases.py reaches, asserted without a GPU: hrp_batch_prepare, hrp_wgrad_config_of and hrp_batch_wgrad_configs are
host code, so a change of wgrad_tiling / wgrad_tiling_octo / wgrad_batch_prepare_nt that sends the table's shapes to other programs
fails here, on the machine without a GPU.  Also here: the literal oracle evaluate_wgrad against torch.nn.grad.conv2d_weight in float64
for the descriptor forms tests/test_plan_conv_desc_host.py does not build, and the value classes of the operand generators."""
import ctypes as C

import pytest
import torch

import conv_exact_oracle as O
import wgrad_exact_cases as T
from conv_exact_oracle import F64

import hrpe_amd  # noqa: F401
from hrpe_amd import _native as nv

_asked = {}


def asked(case, path):
    """The library's answer for a path of a case (asked once)."""
    key = (case.name, path)
    if key not in _asked:
        _asked[key] = T.host_configs(case, path)
    return _asked[key]


def reached(paths):
    """[(problem, Config)] over the table's cases on the given paths."""
    return [(p, c) for case in T.TABLE for path in case.paths if path in paths for p, c in zip(T.problems(case, path), asked(case, path))]


def test_every_case_runs_what_the_table_says():
    names = [c.name for c in T.TABLE]
    assert len(set(names)) == len(names)
    for case in T.TABLE:
        for path in case.paths:
            assert asked(case, path) == T.expected(case, path), f"{case.name} {path}: the launcher chose {asked(case, path)}"
            for p in T.problems(case, path):
                assert p.cost <= T.COST_CAP, f"{case.name}: {p.cost:.2e} multiply-adds"
                assert p.dw_cin <= p.Cin <= p.x_pitch and p.Cout <= p.dy_pitch
    assert len(T.gpu_cases()) <= 200


def four_wave_key(p, c):
    return (p.dt, p.ntaps, c.BM if p.dt == "f32" else c.nks, c.arrange)


FOUR_WAVE = ({("bf16", nt, nks, 1) for nt in (1, 4, 9) for nks in (1, 2, 4)} | {("bf16", 1, nks, 2) for nks in (1, 2)}
             | {("f32", nt, bm, 1) for nt in (1, 4, 9) for bm in (16, 64, 128)} | {("f32x3", nt, nks, 1) for nt in (1, 4, 9) for nks in (1, 2)})
# program, taps, PAIRS, k-steps, ring
EIGHT_WAVE = {(1, 9, 1, 4, 2), (1, 9, 4, 4, 3), (1, 9, 4, 4, 2), (1, 9, 4, 2, 3),
              (2, 9, 4, 4, 0), (2, 9, 4, 2, 0), (2, 9, 4, 1, 0), (2, 1, 4, 4, 0)}


@pytest.mark.parametrize("paths", [("S-ws",), ("B",)], ids=["single", "batched"])
def test_four_wave_instantiations_reached(paths):
    got = {four_wave_key(p, c) for p, c in reached(paths) if c.program == nv.WGRAD_FOUR_WAVE}
    assert FOUR_WAVE <= got, f"four-wave instantiations (type, taps, k-steps or BM, NB) no case reaches on {paths}: {sorted(FOUR_WAVE - got)}"
    assert max(k[2] for k in got if k[0] == "f32") == 128, "fp32 tiles grew: add the new largest BM to the table"


@pytest.mark.parametrize("path", ["B", "B-ph1"])
def test_eight_wave_instantiations_reached(path):
    got = {(c.program, p.ntaps, c.arrange, c.nks, c.ring) for p, c in reached((path,)) if c.program != nv.WGRAD_FOUR_WAVE}
    assert EIGHT_WAVE <= got, f"eight-wave instantiations (program, taps, PAIRS, k-steps, ring) no case reaches on {path}: {sorted(EIGHT_WAVE - got)}"


def test_instantiations_declared_unreachable_are_not_reached():
    """The two the table leaves out (module docstring of wgrad_exact_cases): over a sweep of image shapes the launcher never picks them."""
    for N in (1, 2, 3, 5, 8, 33):
        for H, W in ((1, 1), (1, 40), (8, 8), (13, 9), (16, 16), (33, 17), (64, 2), (40, 64)):
            b = T.P(T.W1, "bf16", N, H, W, 64, 72)
            for c in (T.host_single(b), T.host_batch([b])[0]):
                assert (c.arrange, c.nks) in ((2, 1), (2, 2)), f"bf16 1x1 NB = 2 at {N} x {H} x {W}: {c} - now reachable, add a case"
            x = T.host_batch([T.P(T.W1, "f32x3", N, H, W, 64, 128)])[0]
            assert (x.program, x.nks) == (nv.WGRAD_EIGHT_WAVE_F32X3, 4), f"fp32x3 1x1 eight-wave at {N} x {H} x {W}: {x} - add a case"


def test_atomics_path_reached_for_every_type_and_tap_count():
    for acc, path in ((0, "S-atom0"), (1, "S-atom1")):
        got = {(p.dt, p.ntaps) for p, c in reached((path,)) if c.use_ws == 0}
        assert got == {(dt, nt) for dt in T.DT for nt in (1, 4, 9)}, f"accumulate = {acc} without a workspace: {sorted(got)}"


def test_tiles_per_workgroup_reached():
    """Per program: workgroups with exactly 1, exactly 2 and at least 3 tiles, and a problem whose workgroups get different counts."""
    seen = {}
    for p, c in reached(("S-ws", "B", "B-ph1")):
        key = (c.program, p.dt if c.program == nv.WGRAD_FOUR_WAVE else "")
        counts = T.tiles_per_workgroup(c)
        s = seen.setdefault(key, [set(), 0])
        s[0] |= counts
        s[1] += len(counts) > 1
    assert set(seen) == {(0, "bf16"), (0, "f32"), (0, "f32x3"), (1, ""), (2, "")}
    for key, (counts, uneven) in seen.items():
        assert {1, 2} <= counts and max(counts) >= 3, f"program {key}: workgroups walk {sorted(counts)} tiles"
        assert uneven >= 1, f"program {key}: no problem whose workgroups get different tile counts"


def test_xmode_and_fold_shares_reached():
    batched = reached(("B", "B-ph1"))
    assert {c.xmode for _, c in batched if c.program == nv.WGRAD_FOUR_WAVE} == {0, 2}, "mode 1 is switched off for the four-wave program (xmask)"
    assert {c.xmode for _, c in batched} == {0, 2}
    assert all(c.xmode == 0 for _, c in reached(("S-ws", "S-ws1", "S-ph1", "S-atom0", "S-atom1")))
    gs = {c.G for _, c in reached(("S-ws", "S-ws1", "S-ph1", "B", "B-ph1"))}
    # wgrad_fold_body: phases without a slab (G < 4), the tail loop alone, the unrolled eight-slab loop entered by some phases only
    # (G in 29 .. 32), and the unrolled loop followed by a tail
    assert 1 in gs and gs & {2, 3} and any(5 <= g <= 28 and g % 4 for g in gs) and any(29 <= g <= 32 for g in gs) \
        and any(g >= 33 and g % 4 for g in gs), sorted(gs)


def test_descriptor_forms_reached():
    ps = {case.name: case for case in T.TABLE}
    every = [(case, p) for case in T.TABLE for p in (case.prob,) + tuple(case.companions)]

    def some(pred, what, paths=None):
        assert any(pred(p) and (paths is None or set(paths) <= set(c.paths)) for c, p in every), f"no case with {what}"
    for geos in (T.STEM, T.DECONV):
        for i, geo in enumerate(geos):
            some(lambda p: p.geo == geo, f"tap group {i} alone", T.GROUP)
        assert any(c.shared and [p.geo for p in (c.prob,) + tuple(c.companions)] == list(geos) and set(T.GROUP) <= set(c.paths) for c in T.TABLE)
    some(lambda p: p.dt == "bf16" and (p.dw_cin, p.Cin) == (12, 16), "dw_cin = 12, Cin = 16 in bf16")
    some(lambda p: p.dt == "f32" and p.dw_cin < p.Cin, "dw_cin < Cin in fp32")
    some(lambda p: (p.Cout, p.dy_pitch) == (17, 24), "Cout = 17, dy_pitch = 24")
    some(lambda p: p.Cc == 40 and p.x_pitch > p.Cin, "Cin = 40 with a padded pitch")
    some(lambda p: p.dt == "bf16" and p.ntaps == 1 and (p.Cc, p.Cout) == (64, 72), "Cout = 72, Cin = 64 (NB = 2)")
    some(lambda p: (p.H, p.W) == (13, 9), "ragged 13 x 9 images")
    some(lambda p: (p.H, p.W) == (1, 1), "1 x 1 images")
    some(lambda p: p.geo == T.W3 and p.H in (1, 2), "H = 1 or 2 under 3x3")
    some(lambda p: p.geo == T.W3S2 and p.H % 2 and (p.Ho, p.Wo) == (9, 11), "odd H under stride 2")
    some(lambda p: p.geo == T.W3D2, "dilation 2")
    some(lambda p: p.geo == T.W1S2, "a 1x1 stride-2 layer")
    some(lambda p: p.dt == "f32" and p.ntaps == 9 and (p.H, p.W) == (13, 9) and p.Cout == 17, "HRP_F32 on 9 taps with ragged edges")
    assert any(p.N % c.TI for p, c in reached(("S-ws", "B"))), "no case whose N is no multiple of TI"
    assert any("S-ws1" in c.paths for c in T.TABLE) and any("S-ph1" in c.paths for c in T.TABLE)
    assert "b9_G33" in ps
    for dt in ("f32x3",):       # both orientations of the split operand for each fp32x3 program
        for prog in (0, 2):
            got = {p.split for p, c in reached(("S-ws", "B", "B-ph1")) if p.dt == dt and c.program == prog}
            assert got == {"x", "dy"}, f"fp32x3 program {prog}: split operand {sorted(got)} only"


def test_tap_group_without_workspace_must_accumulate():
    """An invalid problem returns the launcher's own error from the query."""
    p = next(c for c in T.TABLE if c.name == "stem_b_g1").prob
    with pytest.raises(nv.HrpError, match="a tap group without a workspace must accumulate"):
        T.host_single(p, ws=False, accumulate=0)
    assert T.host_single(p, ws=False, accumulate=1).use_ws == 0
    g = T.fill(p, 0x100000, 0x200000, 0x300000, 0)
    g.dw_cin = p.Cin + 8
    with pytest.raises(nv.HrpError, match="dw_cin > Cin"):
        T.config_of(g)
    c = nv.WgradConfig()
    assert nv.lib().hrp_batch_wgrad_configs(None, None, C.byref(c)) == -1


def test_value_classes_and_precondition_of_every_case():
    for case in T.TABLE:
        for p in (case.prob,) + tuple(case.companions):
            xm, dm = O.wgrad_values(p.dt, p.split, p.pixels)
            O.assert_value_class(torch.tensor(xm, dtype=F64), p.dt != "bf16" and p.split == "x", f"{case.name}: x")
            O.assert_value_class(torch.tensor(dm, dtype=F64), p.dt != "bf16" and p.split == "dy", f"{case.name}: dy")
            assert p.pixels * max(xm) * max(dm) + 7 < 2 ** 24
    # a generated pair, and what the fp32x3 kernels keep of it: hi.hi + hi.lo + lo.hi is the product, lo.lo is zero
    g = torch.Generator().manual_seed(5)
    for split in ("x", "dy"):
        x, dy = O.wgrad_operands(g, "f32x3", split, 2, 5, 4, 8, 5, 4, 8)
        O.assert_value_class(x, split == "x", "x")
        O.assert_value_class(dy, split == "dy", "dy")
        (xh, xl), (dh, dl) = O.split_planes(x), O.split_planes(dy)
        assert bool((xl != 0).all() and (dl == 0).all()) if split == "x" else bool((dl != 0).all() and (xl == 0).all())
        kept = xh.double() * dh.double() + xh.double() * dl.double() + xl.double() * dh.double()
        assert torch.equal(kept, x * dy)
    with pytest.raises(AssertionError):
        O.assert_value_class(torch.tensor([256.0, 257.0]), True, "256 is a bf16 number")
    with pytest.raises(AssertionError):
        O.assert_value_class(torch.tensor([1052671.0]), True, "2^20 + 4095: lo = 4095 is no bf16 number, hi + lo is off by one")


def _torch_wgrad(x, dy, k, stride, dilation):
    xr, gr = x.to(F64).permute(0, 3, 1, 2), dy.to(F64).permute(0, 3, 1, 2)
    w = torch.nn.grad.conv2d_weight(xr, (dy.shape[-1], x.shape[-1], k, k), gr, stride=stride, padding=dilation * (k // 2), dilation=dilation)
    return w.reshape(dy.shape[-1], x.shape[-1], k * k)


def test_oracle_matches_torch_on_the_forms_the_plan_test_does_not_build():
    g = torch.Generator().manual_seed(11)
    # dw_cin < Cin, accumulate onto integers, dilation 2
    for geo, k, st, dil, Cc, dt in ((T.W3D2, 3, 1, 2, 12, "bf16"), (T.W3S2, 3, 2, 1, 10, "f32"), (T.W1S2, 1, 2, 1, 12, "bf16")):
        p = T.P(geo, dt, 2, 9, 7, Cc, 5)
        assert p.dw_cin < p.Cin
        x, dy = O.wgrad_operands(g, dt, "x", p.N, p.H, p.W, p.Cc, p.Ho, p.Wo, p.Cout)
        dw0 = O.signed(g, (p.Cout, p.dw_cin, p.T), (1, 2, 3))
        ref = _torch_wgrad(x, dy, k, st, dil)
        for acc in (0, 1):
            got, wr = O.evaluate_wgrad(T.fill(p, 0, 0, 0, acc), x, dy, dw0)
            assert bool(wr.all()) and torch.equal(got, ref + (dw0 if acc else 0))
    # a tap group: row r of the 4x4 stride-2 kernel V (padding 1) lands in taps 4 r .. 4 r + 3, the other twelve keep dw0
    x, dy = O.wgrad_operands(g, "bf16", "x", 2, 12, 10, 8, 6, 5, 5)
    xr, gr = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)
    ref = torch.nn.grad.conv2d_weight(xr, (5, 8, 4, 4), gr, stride=2, padding=1).reshape(5, 8, 16)
    dw0 = O.signed(g, (5, 8, 16), (1, 2, 3))
    for r, geo in enumerate(T.DECONV):
        p = T.P(geo, "bf16", 2, 12, 10, 8, 5)
        for acc in (0, 1):
            got, wr = O.evaluate_wgrad(T.fill(p, 0, 0, 0, acc), x, dy, dw0)
            mask = torch.zeros(5, 8, 16, dtype=torch.bool)
            mask[:, :, 4 * r:4 * r + 4] = True
            assert torch.equal(wr, mask) and torch.equal(got[~mask], dw0[~mask])
            assert torch.equal(got[mask], (ref + (dw0 if acc else 0))[mask])
