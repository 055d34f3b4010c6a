"""Optimizer::OptimizeSim3 without a GPU: the restatement's self-checks, the C ABI's presence and its loud failure without a
device, the -DSIVO_SIM3_ON_DEVICE routing of the C++ member, and the gather step against the restatement of
Optimizer.cc:1294-1383 (bit-exact floats)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import host_prog
import sim3_restatement as R

API = os.path.join(ROOT, "sivo_amd", "api")


def _close(A, B, tol):
    (qa, ta, sa), (qb, tb, sb) = A, B
    return (np.max(np.abs(np.array(qa) - qb)) < tol and np.max(np.abs(np.array(ta) - tb)) < tol and abs(sa - sb) < tol)


def test_exponential_identity_and_inverse_update():
    I = R.sim3_exp([0.0] * 7)
    assert I[0] == [0.0, 0.0, 0.0, 1.0] and list(I[1]) == [0.0, 0.0, 0.0] and I[2] == 1.0
    rng = np.random.default_rng(3)
    # the four branches of Sim3(const Vector7d &): |sigma| < 1e-5 or not, theta < 1e-5 or not.  In (theta < 1e-5, sigma != 0) g2o's
    # B lacks the "- 1" of the series ((sigma^2/2 - sigma + 1) e^sigma - 1) / sigma^3, restated as it is: a second-order error
    # B theta^2 |upsilon| there, hence the wider bound for that branch.
    for sigma, mag, tol in ((0.0, 1e-7, 1e-12), (0.0, 0.4, 1e-12), (0.3, 0.4, 1e-12), (0.3, 1e-7, 1e-9)):
        u = np.concatenate([rng.normal(size=3) * mag, rng.normal(size=3), [sigma]])
        S = R.sim3_mul(R.sim3_exp(-u), R.sim3_exp(u))
        assert _close(S, I, tol), (sigma, mag, S)
        assert _close(R.sim3_mul(R.sim3_inv(R.sim3_exp(u)), R.sim3_exp(u)), I, 1e-12)


def test_numeric_jacobian_matches_a_wide_step_difference():
    sc = R.make_scene(40, 11, scale=1.2, fix_scale=False)
    prob = R.Problem(sc["matches"], sc["k1"], sc["k2"], 10.0, False)
    S = R.sim3_from_state(sc["s12"])
    J12, J21 = prob.jacobians(S)
    h = 1e-5
    for d in range(7):
        up, um = [0.0] * 7, [0.0] * 7
        up[d], um[d] = h, -h
        Sp, Sm = R.sim3_oplus(S, up, False), R.sim3_oplus(S, um, False)
        e12p, e21p = prob.errors(Sp)
        e12m, e21m = prob.errors(Sm)
        for J, ep, em in ((J12, e12p, e12m), (J21, e21p, e21m)):
            ref = np.stack([(ep[0] - em[0]) / (2 * h), (ep[1] - em[1]) / (2 * h)], 1)
            # delta = 1e-9 differences of ~600 px values: an ulp of the error (1.1e-13) is 5.7e-5 in J — the cancellation noise g2o
            # has too, a few 1e-4 absolute against entries up to ~1e3
            assert np.max(np.abs(J[:, :, d] - ref) - 1e-6 * np.abs(ref)) < 5e-4, d


@pytest.mark.parametrize("fix_scale", [True, False])
def test_restatement_recovers_the_true_sim3_noise_free(fix_scale):
    sc = R.make_scene(120, 21, scale=1.0 if fix_scale else 1.25, noise=0.0, fix_scale=fix_scale)
    res = sc["expect"]
    assert res["inliers"] == 120 and not res["outlier"].any()
    truth = sc["truth"]
    q = res["s12"][:4] * np.sign(res["s12"][3] * truth[3])
    assert np.max(np.abs(q - truth[:4])) < 1e-6
    assert np.max(np.abs(res["s12"][4:7] - truth[4:7])) < 1e-5 * (1 + np.max(np.abs(truth[4:7])))
    assert abs(res["s12"][7] - truth[7]) < 1e-6
    assert np.max(np.abs(sc["s12"] - truth)) > 1e-3          # (it did start away from the truth)


def test_header_declares_and_library_exports_the_entry_points():
    h = open(os.path.join(ROOT, "include", "sivo_hip.h")).read()
    assert re.search(r"int sivo_sim3_optimize\(double s12\[8\]", h) and "int sivo_sim3_optimize_batch(" in h
    assert "SivoSim3Match" in h and "SivoSim3Problem" in h
    from sivo_amd import _lib
    from sivo_amd.optimizer import SIM3_MATCH_DTYPE
    L = _lib.lib()
    assert hasattr(L, "sivo_sim3_optimize") and hasattr(L, "sivo_sim3_optimize_batch")
    assert SIM3_MATCH_DTYPE.itemsize == C.sizeof(_lib.Sim3Match) == 96
    assert C.sizeof(_lib.Sim3Problem) == 184


def test_entry_points_fail_loudly_without_a_device():
    from sivo_amd import _lib, optimizer
    sc = R.make_scene(12, 5)
    if _lib.lib().sivo_device_count() >= 1:            # (a device is visible: the call runs; tests/test_gpu_sim3.py checks what it computes)
        assert optimizer.sim3_optimize(sc["s12"], sc["k1"], sc["k2"], sc["matches"])["inliers"] >= 0
        return
    with pytest.raises(_lib.SivoError) as e:
        optimizer.sim3_optimize(sc["s12"], sc["k1"], sc["k2"], sc["matches"])
    assert e.value.code == _lib.ERR_RUNTIME
    with pytest.raises(_lib.SivoError):
        optimizer.sim3_optimize_batch([{"s12": sc["s12"], "k1": sc["k1"], "k2": sc["k2"], "matches": sc["matches"]}])
    # invalid arguments are reported as such before any device is needed
    with pytest.raises(_lib.SivoInvalidArgument):
        optimizer.sim3_optimize(np.r_[sc["s12"][:7], -1.0], sc["k1"], sc["k2"], sc["matches"])


def test_optimize_sim3_member_instantiates_on_device(tmp_path):
    """-DSIVO_SIM3_ON_DEVICE routes Optimizer::OptimizeSim3 to the device (no g2o): the member instantiates over stand-ins."""
    tu = tmp_path / "use.cpp"
    tu.write_text(r'''#include "orbslam/Optimizer.h"
struct KF;
struct MP { cv::Mat GetWorldPos() const { return cv::Mat(3, 1, CV_32F); } bool isBad() const { return false; }
            int GetIndexInKeyFrame(KF *) const { return 0; } };
struct KF { cv::Mat mK; std::vector<cv::KeyPoint> mvKeysSemantic; std::vector<float> mvInvLevelSigma2;
            cv::Mat GetRotation() const { return cv::Mat(3, 3, CV_32F); } cv::Mat GetTranslation() const { return cv::Mat(3, 1, CV_32F); }
            std::vector<MP *> GetMapPointMatches() const { return {}; } };
struct Q { double c[4]; double &x() { return c[0]; } double &y() { return c[1]; } double &z() { return c[2]; } double &w() { return c[3]; }
           double x() const { return c[0]; } double y() const { return c[1]; } double z() const { return c[2]; } double w() const { return c[3]; } };
struct V { double c[3]; double &operator[](int i) { return c[i]; } double operator[](int i) const { return c[i]; } };
struct S3 { Q r; V t; double s; S3(const Q &a, const V &b, double c) : r(a), t(b), s(c) {}
            Q rotation() const { return r; } V translation() const { return t; } double scale() const { return s; } };
int f(KF *a, KF *b, std::vector<MP *> &m, S3 &s) { return SIVO::Optimizer::OptimizeSim3(a, b, m, s, 10.f, true); }
''')
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-DSIVO_SIM3_ON_DEVICE", "-I" + API, str(tu)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.parametrize("random_pose", [False, True])
def test_gather_matches_the_reference_walk(tmp_path, random_pose):
    sc = R.make_scene(30, 8)
    kf1, kf2, pts, m1 = R.keyframe_pair(sc, 9, random_pose=random_pose, n_extra=15)
    exe = host_prog.build("sim3_adapter_prog", tmp_path)
    rows = [ln.split() for ln in host_prog.run_text(exe, ["gather"], R.scene_text(sc, kf1, kf2, pts, m1), 60).strip().splitlines()]
    idx, recs = R.gather(kf1, kf2, m1, pts)
    assert [int(w[0]) for w in rows] == list(idx)
    assert len(idx) == 30                                    # every pair of the scene, none of the 15 entries to skip
    got = np.array([[float.fromhex(v) for v in w[1:]] for w in rows])
    want = np.concatenate([recs["x1c"], recs["x2c"], recs["obs1"], recs["inv_sigma2_1"][:, None], recs["obs2"],
                           recs["inv_sigma2_2"][:, None]], 1)
    assert got.tobytes() == want.tobytes()
    if not random_pose:                                      # identity poses: the scene's own pairs come back
        order = np.argsort([kf1["mp"][i] for i in idx])
        assert np.array_equal(recs[order].tobytes(), sc["matches"].tobytes())
