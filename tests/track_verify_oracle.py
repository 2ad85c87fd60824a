"""Float64 numpy statement of the tracker's verification rule (include/hrp.h hrp_track_verify) and the case list the host program
(tests/test_track_verify_host.py) and the kernel (tests/test_gpu_track_verify.py) are both held to."""
import itertools

import numpy as np

SKIPPED, KEPT, UNDECIDED, DROPPED, FAIL_SUPPORT, FAIL_COVERAGE, FAIL_IOU = 1, 2, 4, 8, 16, 32, 64
MAX_KP, MAX_BONES, MAX_SAMPLES = 32, 32, 64
ARGS = ("state", "have", "scale", "mask", "alpha", "bones", "samples", "extend_ratio", "min_prob", "min_fg", "min_samples",
        "min_support", "min_coverage", "min_iou")
SIZES = ((1, 1), (5, 7), (17, 33), (60, 80), (240, 320))
F32, F64 = np.float32, np.float64


def measure(state, scale, mask, alpha, bones, samples, extend_ratio, min_prob):
    """Steps 1 - 5 for a stream that has an estimate: None when the state is not finite, else (counts [4] = (h_s, n_s, n_in, n_fg),
    sums [3] = (I, S, R))."""
    u = np.asarray(state, F64)
    with np.errstate(all="ignore"):
        d = u * np.asarray(scale, F64)[None, :]
        if not (np.isfinite(u).all() and np.isfinite(d).all()):
            return None
        mask = np.asarray(mask, F32)
        hm, wm = mask.shape
        pts = [d]
        t = (np.arange(samples, dtype=F64) + 0.5) / F64(samples)
        for a, b in bones:
            pts.append(d[a][None, :] + t[:, None] * (d[b] - d[a])[None, :])
        p = np.concatenate(pts)
        ok = (p[:, 0] >= 0.0) & (p[:, 0] < wm) & (p[:, 1] >= 0.0) & (p[:, 1] < hm)
        q = p[ok]
        fg = mask >= F32(min_prob)                                   # (a NaN pixel compares false)
        h_s = int(fg[q[:, 1].astype(np.int64), q[:, 0].astype(np.int64)].sum())
        x0, y0, x1, y1 = d[:, 0].min(), d[:, 1].min(), d[:, 0].max(), d[:, 1].max()
        w, h = x1 - x0, y1 - y0
        e0, e1 = F64(extend_ratio[0]), F64(extend_ratio[1])
        box = (x0 - e0 * w, y0 - e1 * h, x1 + e0 * w, y1 + e1 * h)
        cx, cy = np.arange(wm, dtype=F64) + 0.5, np.arange(hm, dtype=F64) + 0.5
        inside = ((cy >= box[1]) & (cy <= box[3]))[:, None] & ((cx >= box[0]) & (cx <= box[2]))[None, :]
        m64 = mask.astype(F64)
        sums = np.zeros(3)
        sums[1] = m64.sum()
        if alpha is not None:
            a64 = np.asarray(alpha, F32).astype(F64)
            sums[0], sums[2] = (m64 * a64).sum(), a64.sum()
    return np.array([h_s, int(ok.sum()), int((fg & inside).sum()), int(fg.sum())], np.int64), sums


def scores(counts, sums):
    with np.errstate(all="ignore"):
        c = counts.astype(F64)
        return c[0] / c[1], c[2] / c[3], sums[0] / (sums[1] + sums[2] - sums[0])


def verify(state, have, scale, mask, alpha, bones, samples, extend_ratio, min_prob, min_fg, min_samples, min_support, min_coverage,
           min_iou):
    """One stream -> (status, have, counts [4] int64, sums [3] float64).  The state itself is never written."""
    zero = np.zeros(4, np.int64), np.zeros(3)
    if not have:
        return (SKIPPED, 0) + zero
    got = measure(state, scale, mask, alpha, bones, samples, extend_ratio, min_prob)
    if got is None:
        return (DROPPED, 0) + zero
    counts, sums = got
    if counts[3] < min_fg:
        return UNDECIDED, 1, counts, sums
    support, coverage, iou = scores(counts, sums)
    fail = 0
    if min_support >= 0 and counts[1] >= min_samples and not support >= min_support:
        fail |= FAIL_SUPPORT
    if min_coverage >= 0 and not coverage >= min_coverage:
        fail |= FAIL_COVERAGE
    if min_iou >= 0 and alpha is not None and not iou >= min_iou:
        fail |= FAIL_IOU
    return (DROPPED | fail, 0, counts, sums) if fail else (KEPT, 1, counts, sums)


def margin(c):
    """The smallest distance of an applied score from its threshold (inf when the decision does not depend on a score)."""
    if not c["have"]:
        return np.inf
    got = measure(*[c[k] for k in ("state", "scale", "mask", "alpha", "bones", "samples", "extend_ratio", "min_prob")])
    if got is None or got[0][3] < c["min_fg"]:
        return np.inf
    counts, _ = got
    s = scores(*got)
    used = [c["min_support"] >= 0 and counts[1] >= c["min_samples"], c["min_coverage"] >= 0, c["min_iou"] >= 0 and c["alpha"] is not None]
    with np.errstate(all="ignore"):
        dist = [abs(v - t) for v, t, on in zip(s, (c["min_support"], c["min_coverage"], c["min_iou"]), used) if on and np.isfinite(v)]
    return min(dist, default=np.inf)


def sums_ok(got, want, n, exact):
    """exact: bit-equal (binary maps: the sums are integers below 2^53).  Otherwise within n * 2^-53 relative: the bound of any
    summation order over n non-negative float64 terms (every term of I, S, R is a product or a widening of fp32 values >= 0;
    a map with a NaN pixel gives NaN in both)."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    if exact:
        return np.array_equal(got, want, equal_nan=True)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and bool(np.all(np.abs(got - want)[~nan] <= n * 2.0 ** -53 * np.abs(want)[~nan]))


def chain(nkp):
    return [(i, i + 1) for i in range(nkp - 1)]


def ellipse(hm, wm, cx, cy, rx, ry):
    y, x = np.mgrid[0:hm, 0:wm]
    return ((x + 0.5 - cx) / max(rx, 0.5)) ** 2 + ((y + 0.5 - cy) / max(ry, 0.5)) ** 2 <= 1.0


def soften(rng, inside, lo=0.4, hi=0.6):
    """A random fp32 map that is >= hi inside and <= lo outside."""
    return np.where(inside, rng.uniform(hi, 1.0, inside.shape), rng.uniform(0.0, lo, inside.shape)).astype(F32)


def base(state, mask, **kw):
    hm, wm = mask.shape
    c = dict(state=np.asarray(state, F64), have=1, scale=(0.5, 0.5), mask=np.ascontiguousarray(mask, F32), alpha=None, bones=[],
             samples=16, extend_ratio=(0.2, 0.13), min_prob=0.5, min_fg=min(16, max(1, hm * wm // 8)), min_samples=1,
             min_support=0.5, min_coverage=0.5, min_iou=-1.0, exact=False, near=False)
    c.update(kw)
    if c["alpha"] is not None:
        c["alpha"] = np.ascontiguousarray(c["alpha"], F32)
    return c


def call_args(c):
    return {k: c[k] for k in ARGS}


def general_cases(rng):
    """Every map size with key-point counts, bone counts and sample counts in rotation; silhouettes absent and given, binary and
    random maps.  A draw whose score lies within 1e-6 of its threshold is drawn again."""
    combos = list(itertools.product((1, 7, 32), (0, 1, 2), (1, 16, 64)))
    picked = [combos[i] for i in (0, 4, 8, 10, 14, 15, 20, 22, 24)]     # every value of every axis three times
    out = []
    for si, (hm, wm) in enumerate(SIZES):
        for ci, (nkp, nbk, S) in enumerate(picked):
            use_alpha, binary = bool((ci + si) & 1), bool((ci + si) & 2)
            for _ in range(50):
                cx, cy = rng.uniform(0.2, 0.8) * wm, rng.uniform(0.2, 0.8) * hm
                rx, ry = rng.uniform(0.1, 0.3) * wm, rng.uniform(0.1, 0.3) * hm
                inside = ellipse(hm, wm, cx, cy, rx, ry)
                on = rng.uniform() < 0.6                                 # the estimate on the blob, or somewhere in the map
                kx, ky = (cx, cy) if on else (rng.uniform(-0.2, 1.2) * wm, rng.uniform(-0.2, 1.2) * hm)
                det = np.stack([kx + rng.uniform(-1, 1, nkp) * rx * 0.8, ky + rng.uniform(-1, 1, nkp) * ry * 0.8], 1)
                bones = [[], chain(nkp), [tuple(rng.integers(0, nkp, 2)) for _ in range(MAX_BONES)]][nbk]
                shift = ellipse(hm, wm, cx + rng.uniform(-0.5, 0.5) * rx, cy + rng.uniform(-0.5, 0.5) * ry, rx, ry)
                mask = inside.astype(F32) if binary else soften(rng, inside)
                alpha = None if not use_alpha else (shift.astype(F32) if binary else soften(rng, shift))
                c = base(det * 2.0, mask, alpha=alpha, bones=bones, samples=S, exact=binary, min_iou=0.5 if use_alpha else -1.0)
                if margin(c) > 1e-6:
                    break
            else:
                raise AssertionError("no draw away from the thresholds")
            out.append(c)
    return out


def outcome_cases(rng, hm=60, wm=80):
    """One case per outcome: skipped, kept, undecided, dropped for a state that is not finite, and the seven combinations of the
    three criteria."""
    blob = ellipse(hm, wm, 0.5 * wm, 0.5 * hm, 0.2 * wm, 0.2 * hm)
    mask = soften(rng, blob, 0.01, 0.9)
    far = soften(rng, ellipse(hm, wm, 0.15 * wm, 0.15 * hm, 0.1 * wm, 0.1 * hm), 0.01, 0.9)
    good = soften(rng, blob, 0.01, 0.9)
    on = np.stack([np.linspace(0.35, 0.65, 7) * wm, np.linspace(0.35, 0.65, 7) * hm], 1)              # on the blob, box around it
    rim = np.array([[0.2, 0.2], [0.5, 0.2], [0.8, 0.2], [0.8, 0.5], [0.8, 0.8], [0.5, 0.8], [0.2, 0.8]]) * [wm, hm]  # around it
    part = np.stack([np.linspace(0.49, 0.51, 7) * wm, np.linspace(0.49, 0.51, 7) * hm], 1)            # a small part of it
    away = np.stack([np.linspace(0.05, 0.2, 7) * wm, np.linspace(0.8, 0.95, 7) * hm], 1)              # beside it
    kw = dict(bones=chain(7), min_iou=0.5)
    out = [base(on * 2, mask, have=0, alpha=good, **kw), base(on * 2, mask, alpha=good, **kw),
           base(on * 2, np.zeros((hm, wm), F32), alpha=good, **kw)]
    bad = on * 2
    bad[3, 1] = np.nan
    out.append(base(bad, mask, alpha=good, **kw))
    want = [KEPT]
    for det, alpha, fails in ((rim, good, FAIL_SUPPORT), (part, good, FAIL_COVERAGE), (on, far, FAIL_IOU), (away, good, FAIL_SUPPORT | FAIL_COVERAGE),
                             (rim, far, FAIL_SUPPORT | FAIL_IOU), (part, far, FAIL_COVERAGE | FAIL_IOU),
                             (away, far, FAIL_SUPPORT | FAIL_COVERAGE | FAIL_IOU)):
        out.append(base(det * 2, mask, alpha=alpha, **kw))
        want.append(DROPPED | fails)
    got = [verify(**call_args(c))[0] for c in out]
    assert got == [SKIPPED, KEPT, UNDECIDED, DROPPED] + want[1:], got
    assert all(margin(c) > 1e-6 for c in out)
    return out


def hostile_cases(rng, hm=17, wm=33):
    blob = ellipse(hm, wm, 0.5 * wm, 0.5 * hm, 0.3 * wm, 0.3 * hm)
    mask = blob.astype(F32)
    on = np.stack([np.linspace(0.3, 0.7, 7) * wm, np.linspace(0.3, 0.7, 7) * hm], 1) * 2.0
    out = []
    for v in (np.nan, np.inf, -np.inf, 1e300, -1e300, -1e9, 1.7e308):
        for col in (0, 1):
            s = on.copy()
            s[2, col] = v
            out.append(base(s, mask, bones=chain(7), exact=True))
            out.append(base(s, mask, bones=chain(7), exact=True, scale=(4.0, 4.0)))      # (1.7e308 * 4 overflows: dropped)
    s = on.copy()
    s[0], s[6] = (1e300, -1e300), (-1e300, 1e300)
    out.append(base(s, mask, bones=[(0, 6), (6, 0), (0, 3)], samples=64, exact=True, extend_ratio=(0.0, 0.0)))
    out.append(base(s, mask, bones=[(0, 6)], exact=True, extend_ratio=(1e10, 1e10)))        # the box overflows to +-inf
    for dx, dy in ((-3.0, 0.0), (3.0, 0.0), (0.0, -3.0), (0.0, 3.0)):                      # beyond every side of the map
        s = on + np.array([dx * wm, dy * hm])
        out.append(base(s, mask, bones=chain(7), exact=True))
        half = on.copy()
        half[:4] = s[:4]
        out.append(base(half, mask, bones=chain(7), exact=True, min_samples=4))
    edge = on.copy()
    edge[0], edge[1], edge[2] = (0.0, 0.0), (np.nextafter(2.0 * wm, 0.0), np.nextafter(2.0 * hm, 0.0)), (2.0 * wm, 2.0 * hm)
    out.append(base(edge, np.ones((hm, wm), F32), bones=chain(7), samples=1, exact=True))
    one = np.tile(on[3], (7, 1))                                                            # all key-points on one point: an empty box
    out.append(base(one, mask, bones=chain(7), exact=True))
    out.append(base(one, mask, bones=chain(7), exact=True, min_coverage=-1.0))
    nanmask = soften(rng, blob)
    nanmask[5, 9] = nanmask[0, 0] = np.nan
    out.append(base(on, nanmask, bones=chain(7)))
    out.append(base(on, nanmask, alpha=soften(rng, blob), bones=chain(7), min_iou=0.5))     # the sums are NaN: IoU fails
    out.append(base(on, np.full((hm, wm), np.nan, F32), bones=chain(7)))
    out.append(base(on, np.zeros((hm, wm), F32), bones=chain(7), exact=True))               # n_fg = 0: undecided
    out.append(base(on, np.zeros((hm, wm), F32), bones=chain(7), exact=True, min_fg=0))     # 0 / 0 is NaN: coverage fails
    out.append(base(on, np.ones((hm, wm), F32), bones=chain(7), exact=True))                # all foreground
    out.append(base(on, np.ones((hm, wm), F32), alpha=np.ones((hm, wm), F32), bones=chain(7), exact=True, min_iou=1.0, near=True))
    out.append(base(on, mask, bones=chain(7), exact=True, min_samples=1000))                # support is not applied
    out.append(base(on, mask, bones=chain(7), exact=True, min_support=-1.0, min_coverage=-1.0))
    return out


def threshold_cases():
    """h_s / n_s == 0.5 exactly: two key-points, one on the foreground.  min_support = 0.5 keeps, 0.5 + 2^-52 drops."""
    mask = np.zeros((5, 7), F32)
    mask[:, :3] = 1.0
    state = np.array([[1.5, 2.5], [5.5, 2.5]]) * 2.0
    kw = dict(min_coverage=-1.0, min_fg=1, min_samples=2, exact=True, near=True)
    out = [base(state, mask, min_support=0.5, **kw), base(state, mask, min_support=0.5 + 2.0 ** -52, **kw)]
    assert [verify(**call_args(c))[0] for c in out] == [KEPT, DROPPED | FAIL_SUPPORT]
    return out


def cases(seed=21):
    rng = np.random.default_rng(seed)
    out = general_cases(rng) + outcome_cases(rng) + hostile_cases(rng) + threshold_cases()
    assert all(c["near"] or margin(c) > 1e-6 for c in out)
    return out


ALL_OUTCOMES = {SKIPPED, KEPT, UNDECIDED, DROPPED} | {DROPPED | f for f in range(FAIL_SUPPORT, 2 * FAIL_IOU, FAIL_SUPPORT)}
