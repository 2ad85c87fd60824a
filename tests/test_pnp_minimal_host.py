"""CPU-only checks of the robust PnP's per-hypothesis core (csrc/pnp_minimal.h) under tests/pnp_minimal_host_check.cpp, built with the
host compiler and -fsanitize=address,undefined -fno-sanitize-recover (a plain executable): P3P on exact and degenerate triples, the
enumeration of the minimal sets, the kernel's hypothesise / score / re-score loop on every sample of golden_pnp_robust.npz, the
fixture's own conditions, and the C ABI declarations."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

import hrpe_amd  # noqa: F401
from hrpe_amd import _native as nv

HYPOTHESES = {"panda_s0": 35, "kuka_s1": 56, "baxter_s1": 680, "cloud24": 1024}


def load_robust():
    return np.load(os.path.join(GOLDEN, "golden_pnp_robust.npz"))


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    td = tmp_path_factory.mktemp("pnp_minimal_host")
    exe = str(td / "pnp_minimal_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                    "-I", os.path.join(ROOT, "holistic-robot-pose-estimation_amd", "csrc"),
                    os.path.join(ROOT, "tests", "pnp_minimal_host_check.cpp"), "-o", exe], check=True)
    return exe, td


@pytest.fixture(scope="module")
def self_output(check_exe):
    exe, _ = check_exe
    r = subprocess.run([exe, "self"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().splitlines()[-1] == "failures 0", r.stdout
    return r.stdout


def test_p3p_recovers_exact_poses(self_output):
    """2000 noise-free triples: the generating pose is among the roots to 1e-9, every root reprojects its points below 1e-6 px."""
    w = [ln for ln in self_output.splitlines() if ln.startswith("p3p exact")][0].replace(",", "").split()
    assert float(w[5]) < 1e-9 and float(w[8]) < 1e-6 and int(w[10]) > 2000, w


def test_p3p_degenerate_triples_return_nothing(self_output):
    roots = {ln.split()[1]: int(ln.split()[3]) for ln in self_output.splitlines() if ln.startswith("degenerate")}
    assert len(roots) == 11 and all(v == 0 for v in roots.values()), roots
    for name in ("collinear", "coincident_points", "nan_point", "inf_bearing"):
        assert name in roots


def test_unranking_and_sampled_triples(self_output):
    got = {int(ln.split()[2][:-1]): int(ln.split()[3]) for ln in self_output.splitlines() if ln.startswith("unrank")}
    assert got == {4: 4, 7: 35, 8: 56, 17: 680, 19: 969}


def test_fixture_conditions():
    """What gen_golden_pnp_robust.py asserts, checked again on the committed file with the host projection of test_pnp_host."""
    from test_pnp_host import rodrigues_np
    g = load_robust()
    assert os.path.getsize(os.path.join(GOLDEN, "golden_pnp_robust.npz")) < 1 << 17
    assert list(g["cases"]) == list(HYPOTHESES)
    for c in g["cases"]:
        x, X, K, P, Pa, mask = (g[f"{c}_{k}"].astype(np.float64) for k in ("pts2d", "pts3d", "K", "P6d", "P6d_all", "mask"))
        mask = mask.astype(bool)
        assert x.shape[0] == 8 and mask.sum(1).min() >= 5
        cam = np.einsum("bij,bnj->bni", rodrigues_np(P[:, :3]), X) + P[:, None, 3:]
        p = np.einsum("bnj,ij->bni", cam, K)
        e = np.sqrt(((p[..., :2] / p[..., 2:3] - x) ** 2).sum(-1))
        assert e[mask].max() < 2 and e[~mask].min() > 10, c
        gap = np.maximum(np.abs(P[:, 3:] - Pa[:, 3:]).max(1), np.sqrt(((P[:, :3] - Pa[:, :3]) ** 2).sum(1)))
        assert (gap > 1e-3).all(), (c, gap)


def test_whole_loop_ends_on_the_planted_mask(check_exe):
    """Every sample of every case: hypothesise, score, pick the winner, then re-score with the fixture's optimum in place of the LM
    refit until the mask stops changing.  The winner's consensus holds no planted outlier and at least four points (what the refit
    starts from), and the loop ends on exactly the planted mask."""
    exe, td = check_exe
    g = load_robust()
    blob, want = [], []
    for c in g["cases"]:
        x, X, K, P, mask = (g[f"{c}_{k}"] for k in ("pts2d", "pts3d", "K", "P6d", "mask"))
        for i in range(x.shape[0]):
            n = x.shape[1]
            blob.append(np.array([n, 1024, 0, 4], np.int32).tobytes() + np.float64(3.0).tobytes() +
                        b"".join(np.ascontiguousarray(a, dtype=np.float64).tobytes() for a in (K, X[i], x[i], P[i])))
            want.append((str(c), i, mask[i]))
    src, dst = td / "loop.in", td / "loop.out"
    src.write_bytes(np.int32(len(blob)).tobytes() + b"".join(blob))
    r = subprocess.run([exe, "loop", str(src), str(dst)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    raw, off = dst.read_bytes(), 0
    for c, i, mask in want:
        n = len(mask)
        H, count, rounds = np.frombuffer(raw[off:off + 12], np.int32)
        m0 = np.frombuffer(raw[off + 12:off + 12 + n], np.uint8)
        m1 = np.frombuffer(raw[off + 12 + n:off + 12 + 2 * n], np.uint8)
        off += 12 + 2 * n
        assert H == HYPOTHESES[c], (c, i, H)
        assert count == m0.sum() >= 4 and not (m0 & (1 - mask)).any(), (c, i, m0, mask)
        assert np.array_equal(m1, mask), (c, i, m1, mask)
        assert 1 <= rounds <= 3, (c, i, rounds)
    assert off == len(raw)


def test_robust_pnp_abi_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "hrp.h")).read()
    for name in ("hrp_pnp_solve_robust", "hrp_pnp_bwd_masked"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in nv.PROTOTYPES
    assert len(nv.PROTOTYPES["hrp_pnp_solve_robust"]) == 18 and len(nv.PROTOTYPES["hrp_pnp_bwd_masked"]) == 18
    assert len(nv.PROTOTYPES["hrp_pnp_bwd"]) == 17
    assert re.search(r"HRP_PNP_NO_CONSENSUS\s*=\s*1\b", src) and nv.PNP_NO_CONSENSUS == 1
    lib = nv.lib()
    assert lib.hrp_pnp_solve_robust(None, None, 0, None, 0, None, 1, 7, 3.0, 4, 1024, 0, 0, None, None, None, None, None) == -1
    assert b"pnp_solve_robust" in lib.hrp_last_error()
    for bad in (dict(n=3), dict(n=65), dict(thr=0.0), dict(thr=float("nan")), dict(min_inliers=3), dict(max_hypotheses=0)):
        a = dict(n=7, thr=3.0, min_inliers=4, max_hypotheses=1024)
        a.update(bad)
        assert lib.hrp_pnp_solve_robust(64, 64, 0, 64, 0, None, 1, a["n"], a["thr"], a["min_inliers"], a["max_hypotheses"], 0, 0, 64, 64, 64,
                                        64, None) == -1, bad


def test_module_surface():
    from hrpe_amd.lib.models.ctrnet.CtRNet import CtRNet
    from hrpe_amd.lib.utils import BPnP as M
    assert issubclass(M.BPnP_robust, torch.autograd.Function)
    assert list(inspect.signature(M.BPnP_robust.forward).parameters) == ["ctx", "pts2d", "pts3d", "K", "reproj_error", "refine_all"]
    p = inspect.signature(M.pnp_solve_robust).parameters
    assert list(p) == ["pts2d", "pts3d", "K", "reproj_error", "valid", "min_inliers", "max_hypotheses", "seed", "refine_all"]
    assert (p["reproj_error"].default, p["min_inliers"].default, p["max_hypotheses"].default, p["seed"].default) == (3.0, 4, 1024, 0)
    for fn in (CtRNet.inference_batch_images, CtRNet.inference_single_image):
        assert inspect.signature(fn).parameters["reproj_error"].default is None
