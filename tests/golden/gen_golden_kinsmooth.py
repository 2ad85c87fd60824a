"""Writes tests/golden/golden_kinsmooth.npz: what the smoother's tests need besides golden_kinfilter.npz - per case the oracle-alone
figures, the flags and link counts, the errors against the ground truth - a few KB.  The histories themselves are regenerated: the golden
sequences' from kinfilter_oracle.replay, the synthetic cases' from kinsmooth_oracle.synthetic_cases' seeds.

Asserted here, so that the fixture cannot be written from an oracle that is wrong:
 (a) on a linear-Gaussian toy with constant H, kinsmooth_oracle.rts' means equal the batch weighted least-squares solution over the
     whole sequence to 1e-9;
 (b) on every *_smooth, *_dropout, *_outlier, *_limit sequence and panda_holistic the smoothed largest-joint error (RMS over the frames,
     against the ground truth redrawn from the sequence's seed) is below the filter's; nothing is asserted for restart / lost;
 (c) every smoothed covariance is positive definite;
 (d) on each *_limit sequence a smoothed joint lies beyond its bound by more than 1e-6, and no joint of a smoothed frame lies within
     1e-9 of a bound (a tail's joints are the history's bytes: one exactly on its bound is not moved by the clamp, here and there);
 (e) the oracle-alone figures (kinsmooth_oracle.own_figures, against 80-bit arithmetic) are stored per case.

  python tests/golden/gen_golden_kinsmooth.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import hrpe_amd  # noqa: E402,F401
import gen_golden_kinfilter as gk  # noqa: E402
import kinfilter_oracle as kf  # noqa: E402
import kinfit_oracle as ko  # noqa: E402
import kinsmooth_oracle as ks  # noqa: E402
from hrpe_amd.lib.utils.urdf_robot import URDFRobot  # noqa: E402

CLAIMED = ("smooth", "dropout", "outlier", "limit", "holistic")


def joint_error(p, truth, nf):
    """The largest joint error per frame, RMS over the frames."""
    return float(np.sqrt(np.mean(np.abs(p[:, :nf] - truth[:, :nf]).max(1) ** 2)))


def main():
    assert ks.HAVE_LD, "the stored figures are against 80-bit arithmetic: this host's long double has no 63-bit mantissa"
    # (a) the oracle itself
    for n, L, seed, dts in ((1, 6, 0, None), (3, 20, 1, None), (6, 12, 2, np.linspace(0.01, 0.08, 12))):
        hist, q_acc, toy = ks.synthetic(n, L, seed, dts=dts, return_toy=True)
        d = np.abs(ks.rts(hist, q_acc)["mean"] - ks.batch_wls(hist, q_acc, toy)).max()
        print(f"toy n {n} L {L}: |rts - batch WLS| {d:.1e}")
        assert d < 1e-9

    robots = {n: URDFRobot(n) for n in kf.ROBOTS}
    seqs = kf.load_fixture(os.path.join(HERE, "golden_kinfilter.npz"), lambda n: robots[n].chain)
    bases = ko.load_fixture(os.path.join(HERE, "golden_kinfit.npz"), lambda n: robots[n].chain)
    seeds = np.load(os.path.join(HERE, "golden_kinfilter.npz"))
    names, own, err, flags, count, beyond = [], [], [], [], [], []
    for name, seq in seqs.items():
        rname, kind = name.split("_", 1)
        F = seq["filter"]
        res = kf.replay(seq)
        hist = ks.history_of([s for s, _ in res], [o["flags"] for _, o in res], [F.dt] * len(res))
        ref = ks.rts(hist, F.q_acc)
        _, frames, truth = gk.draw(robots[rname], bases[f"{rname}_qonly_noise"][0], kind, int(seeds[f"{name}_i"][8]))
        assert all(np.array_equal(a["pts2d"], b["pts2d"], equal_nan=True) for a, b in zip(frames, seq["frames"])), name
        e = (joint_error(hist["mean"], truth, F.nfree), joint_error(ref["mean"], truth, F.nfree))
        tr = []
        far = 0.0
        for t in range(len(res)):
            if ref["flags"][t] & ks.INVALID:
                continue
            assert np.linalg.eigvalsh(ref["cov"][t]).min() > 0, (name, t)                                    # (c)
            if t + 1 < len(res) and ref["flags"][t] & ks.SMOOTHED:
                tr.append(np.trace(ref["cov"][t][:F.nfree, :F.nfree]) / np.trace(hist["cov"][t][:F.nfree, :F.nfree]))
            fr = seq["frames"][t]
            o = ks.outputs(F, ref["mean"][t], fr["q_in"], (fr["rot_in"], fr["trans_in"]))
            # (d) the decision's margin; a tail's value is the history's bytes, so a joint exactly ON its bound decides the same everywhere
            assert ref["flags"][t] & ks.TAIL or np.abs(o["beyond"]).min() > 1e-9, (name, t)
            far = max(far, float(o["beyond"].max()))
        if kind in CLAIMED:
            assert e[1] < e[0], (name, e)                                                                    # (b)
        if kind == "limit":
            assert far > 1e-6, (name, far)                                                                   # (d)
        fig = ks.own_figures(hist, F.q_acc)
        assert fig[0] > 0 and fig[1] > 0, name
        print(f"{name}: joint error {e[0]:.3f} -> {e[1]:.3f} rad, cov trace ratio {np.mean(tr):.2f}, beyond {far:+.4f}, flags "
              f"{ref['flags'].tolist()}, own {fig[0]:.1e} {fig[1]:.1e}")
        names.append(name); own.append(fig); err.append(e); flags.append(ref["flags"]); count.append(ref["count"]); beyond.append(far)
    for name, c in ks.synthetic_cases().items():
        ref = ks.rts(c["hist"], c["q_acc"])
        fig = ks.own_figures(c["hist"], c["q_acc"])
        assert (fig[0] > 0 and fig[1] > 0) or not (ref["flags"] & ks.SMOOTHED).any(), name
        for t in range(len(ref["flags"])):
            if ref["flags"][t] & ks.SMOOTHED:
                assert np.linalg.eigvalsh(ref["cov"][t]).min() > 0, (name, t)
        print(f"{name}: flags {ref['flags'].tolist()}, count {ref['count'].tolist()}, own {fig[0]:.1e} {fig[1]:.1e}")
        names.append(name); own.append(fig); err.append((0.0, 0.0)); flags.append(ref["flags"]); count.append(ref["count"]); beyond.append(0.0)
    path = os.path.join(HERE, "golden_kinsmooth.npz")
    np.savez_compressed(path, names=np.array(names), own=np.array(own, np.float64), err=np.array(err, np.float64),
                        offsets=np.cumsum([0] + [len(f) for f in flags]).astype(np.int32), flags=np.concatenate(flags).astype(np.int32),
                        count=np.concatenate(count).astype(np.int32), beyond=np.array(beyond, np.float64))
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 64 * 1024


if __name__ == "__main__":
    main()
