"""Float64 numpy statement of the tracker's acquisition rule (include/hrp.h hrp_track_seed) and the case list the host program
(tests/test_track_seed_host.py) and the kernel (tests/test_gpu_track_acquire.py) are both held to."""
import numpy as np

SKIPPED, TAKEN, REFUSED = 1, 2, 4


def seed(det, inv, mask, min_prob, ms, min_peak, min_inside, force, W, H, state, have):
    """One stream.  det [nkp, 2] fp32, inv (x, y) float64, mask [hm, wm] fp32 or None, ms [nkp, 2] fp32 or None, state [nkp, 2]
    float64 -> (status, have, state)."""
    det = np.asarray(det, np.float32)
    if have and not force:
        return SKIPPED, have, state
    with np.errstate(all="ignore"):
        u = det.astype(np.float64) * np.asarray(inv, np.float64)[None, :]
        finite = np.isfinite(det).all() and np.isfinite(u).all() and np.isfinite(inv).all()
        counted = 0
        for i in range(len(det)):
            if not (np.isfinite(det[i]).all() and np.isfinite(u[i]).all()):
                continue
            ok = 0.0 <= u[i, 0] < W and 0.0 <= u[i, 1] < H
            if ok and mask is not None:
                hm, wm = mask.shape
                ok = 0 <= det[i, 0] < wm and 0 <= det[i, 1] < hm
                if ok:
                    ok = bool(mask[int(det[i, 1]), int(det[i, 0])] >= np.float32(min_prob))
            if ok and ms is not None:
                ok = bool(np.float32(1.0) / np.float32(ms[i, 1]) >= np.float32(min_peak))
            counted += bool(ok)
    if not finite or counted < min_inside:
        return REFUSED, have, state
    return TAKEN, 1, u


def cases(rng, nkp=7, W=640, H=480, hm=240, wm=320):
    """dicts of one stream each: hostile values, every side of the frame, masks, peaks, skipped and forced streams."""
    inv = (2.0, 2.0)

    def inside(n=nkp):
        return np.stack([rng.uniform(1, wm - 1, n), rng.uniform(1, hm - 1, n)], 1).astype(np.float32)

    def base(**kw):
        c = dict(det=inside(), inv=inv, mask=None, min_prob=0.5, ms=None, min_peak=0.0, min_inside=1, force=0, W=W, H=H,
                 state=rng.normal(size=(nkp, 2)) * 100.0, have=0)
        c.update(kw)
        return c

    out = [base(), base(have=1), base(have=1, force=1), base(min_inside=nkp), base(min_inside=nkp + 1)]
    for bad in (np.nan, np.inf, -np.inf, 1e300, -1e300):
        d = inside()
        with np.errstate(over="ignore"):
            d[min(3, nkp - 1), 1] = np.float32(bad)          # (1e300 becomes inf in fp32: what a caller's cast would hand over)
        out.append(base(det=d))
        out.append(base(det=d, have=1))
    for huge in (3e38, -3e38):
        d = inside()
        d[0, 0] = huge
        out.append(base(det=d))                    # finite in fp32 and in float64, far outside: not counted, still taken
        out.append(base(det=d, inv=(1e300, 1e300)))   # the product overflows float64
    for side in ("left", "right", "above", "below"):
        d = inside()
        d[:, 0 if side in ("left", "right") else 1] = {"left": -3.0, "right": wm + 2.0, "above": -0.5, "below": hm + 0.25}[side]
        out.append(base(det=d))
        d2 = inside()
        d2[:3] = d[:3]
        out.append(base(det=d2, min_inside=nkp - 3))
        out.append(base(det=d2, min_inside=nkp - 2))
    edge = inside()
    edge[0] = (0.0, 0.0)
    edge[1 % nkp] = (np.nextafter(np.float32(wm), np.float32(0)), np.nextafter(np.float32(hm), np.float32(0)))
    edge[2 % nkp] = (wm, hm)
    mask = rng.uniform(0, 1, (hm, wm)).astype(np.float32)
    out.append(base(det=edge, mask=mask, min_inside=nkp - 1))
    out.append(base(det=edge, mask=mask, min_inside=nkp))
    out.append(base(det=edge, mask=np.ones((hm, wm), np.float32), min_inside=nkp - 1))
    out.append(base(det=edge, mask=np.zeros((hm, wm), np.float32)))
    out.append(base(det=edge, mask=np.full((hm, wm), np.nan, np.float32)))
    out.append(base(det=inside() * np.float32(1.9), inv=(1.0, 1.0), mask=np.ones((hm, wm), np.float32), min_inside=2))   # in the frame, partly off the mask
    out.append(base(det=inside(), mask=np.ones((1, 1), np.float32)))
    ms = np.stack([rng.normal(size=nkp), rng.uniform(1.0, 50.0, nkp)], 1).astype(np.float32)
    out.append(base(ms=ms, min_peak=0.1, min_inside=3))
    out.append(base(ms=ms, min_peak=0.1, min_inside=nkp))
    bad_ms = ms.copy()
    bad_ms[:, 1] = np.resize(np.array([np.nan, np.inf, 0.0, -1.0, 1.0, 1e-30, 2.0], np.float32), nkp)
    out.append(base(ms=bad_ms, min_peak=0.4, min_inside=3))
    out.append(base(ms=bad_ms, min_peak=0.4, min_inside=4, mask=mask, min_prob=0.0))
    out.append(base(inv=(np.nan, 2.0)))
    return out
