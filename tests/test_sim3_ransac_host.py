"""Sim3Solver's RANSAC without a GPU: the restatement's self-checks (Horn's closed form, the sequential semantics of iterate /
find / SetRansacParameters, degenerate samples), the C ABI's presence, its argument checks and its loud failure without a
device, SIVO::Sim3Solver's interface over stand-in types, and its gather against the restatement of Sim3Solver.cc:43-110
(bit-exact floats)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import host_prog
import sim3_ransac_restatement as R

API = os.path.join(ROOT, "sivo_amd", "api")

# Horn on exact correspondences in float32.  The inputs carry a relative rounding of 2^-24 = 6e-8 on coordinates up to ~35; the
# rotation comes from differences to the centroid, so its error is that rounding divided by the relative spread of the sample
# (samples are drawn from all pairs: some triples are close to collinear), and t = O1 - s R O2 multiplies it by |O2| <= ~35.
# The restatement's own worst case over 6 seeds x 300 triples x both scale modes of the generator's scenes is 6e-5 (R), 5.5e-4
# (t), 3.1e-7 (s, 2.6 ulp at 1.3); the bounds are ten times that, rounded.
HORN_TOL = {"R": 5e-4, "t": 5e-3, "s": 5e-6}


@pytest.mark.parametrize("fix_scale", [True, False])
def test_horn_recovers_the_true_sim3_noise_free(fix_scale):
    for seed in (31, 32):
        sc = R.make_scene(150, seed, scale=1.0 if fix_scale else 1.3, noise=0.0)
        res = R.ransac(sc["pairs"], sc["k1"], sc["k2"], sc["triples"], 20, fix_scale)
        T = res["T"].astype(np.float64)
        assert np.max(np.abs(T[:, :9].reshape(-1, 3, 3) - sc["R"])) < HORN_TOL["R"]
        assert np.max(np.abs(T[:, 9:12] - sc["t"])) < HORN_TOL["t"]
        assert np.max(np.abs(T[:, 12] - sc["s"])) < HORN_TOL["s"]
        assert fix_scale is False or np.all(res["T"][:, 12] == 1.0)
        assert np.all(res["count"] == 150) and res["first_accept"] == 0 and res["best"] == 299


def _seq(counts, N=50, **kw):
    calls = []

    def evaluate(h):
        calls.append(h)
        return counts[h], h
    return R.Sequential(N, evaluate, **kw), calls


def test_first_count_above_min_inliers_returns():
    s, calls = _seq([3, 20, 7, 21, 40], probability=0.99, min_inliers=20, max_iterations=5)
    assert s.max_its == 5
    assert s.iterate(10) == (3, False, 21)            # 20 is not above 20; hypothesis 3 (count 21) is the first that is
    assert calls == [0, 1, 2, 3] and s.best == 3 and s.best_inliers == 21
    assert s.iterate(10) == (4, False, 40) and s.iterate(10) == (None, True, 0)


def test_later_of_equal_bests_is_kept():
    s, _ = _seq([5, 9, 2, 9, 4], min_inliers=20, max_iterations=5)
    assert s.find() == (None, 0)
    assert s.best == 3 and s.best_inliers == 9


def test_repeated_iterate_equals_one_find_and_no_more_is_exact():
    counts = list(np.random.default_rng(4).integers(0, 15, 23))
    a, _ = _seq(counts, min_inliers=20, max_iterations=23)
    b, _ = _seq(counts, min_inliers=20, max_iterations=23)
    assert a.max_its == 23
    flags = [a.iterate(5)[1] for _ in range(5)]
    assert flags == [False, False, False, False, True]            # 5, 10, 15, 20: not yet; 23 = mRansacMaxIts: bNoMore
    b.find()
    assert (a.best, a.best_inliers, a.iterations) == (b.best, b.best_inliers, b.iterations) == (b.best, max(counts), 23)
    c, _ = _seq(counts[:20], min_inliers=20, max_iterations=20)
    assert [c.iterate(5)[1] for _ in range(4)] == [False, False, False, True]       # set exactly when the maximum is reached


def test_fewer_pairs_than_min_inliers_returns_at_once():
    s, calls = _seq([50] * 10, N=19, min_inliers=20, max_iterations=10)
    assert s.iterate(5) == (None, True, 0) and calls == [] and s.iterations == 0


def test_set_ransac_parameters():
    assert R.ransac_iterations(0.99, 20, 300, 20) == 1                                  # minInliers == N
    for p, m, N in ((0.99, 20, 100), (0.99, 20, 40), (0.9, 6, 30), (0.999, 20, 25)):
        eps = float(np.float32(m) / np.float32(N))
        want = int(np.ceil(np.log(1 - p) / np.log(1 - eps ** 3)))
        assert R.ransac_iterations(p, m, 10 ** 6, N) == want
        assert R.ransac_iterations(p, m, 300, N) == max(1, min(want, 300))
    assert R.ransac_iterations(0.99, 20, 300, 100) == 300 and R.ransac_iterations(0.99, 20, 300, 25) == 7   # ln 0.01 / ln (1 - 0.8^3) = 6.42
    assert R.ransac_iterations(0.99, 20, 0, 100) == 1                                   # clamped from below
    assert R.ransac_iterations(0.99, 20, 300, 19) == 1                                  # log of a negative number: one iteration


def _fake_result(counts, N):
    """What sivo_sim3_ransac would hand the class for these counts: hypothesis h has T = h + 1 everywhere and inliers 0 .. count-1."""
    counts = np.asarray(counts, np.int32)
    T = np.repeat(np.arange(1, len(counts) + 1, dtype=np.float32)[:, None], 13, 1)
    bits = R.pack_bits(np.arange(N)[None, :] < counts[:, None])
    return {"count": counts, "T": T, "inlier_bits": bits, "first_accept": -1, "best": -1}


def _class_and_checker(counts, N, par):
    """The shipped Python class over injected counts (no device: solve_all skips a solver that has its result) next to the checker."""
    from sivo_amd import sim3_solver
    sc = R.make_scene(N, 3, n_hyp=1)
    idx = np.arange(N)[::-1] * 2                          # mvnIndices1: pair i came from entry 2 (N - 1 - i) of 2 N matches
    s = sim3_solver.Sim3Solver(sc["pairs"], sc["k1"], sc["k2"], True, indices1=idx, n_matches=2 * N, randint=R.seeded_randint(2))
    q = R.Sequential(N, lambda h: (int(counts[h]), h))
    for o in (s, q):
        o.set_ransac_parameters(*par)
    s.result = _fake_result(counts[:s.max_its], N)
    return s, q, idx


def _same_call(s, q, idx, counts, n_it):
    """One iterate(n_it) of both; the class' return checked against the checker's and against the injected hypothesis."""
    T, no_more, inl, n = s.iterate(n_it)
    h, q_no_more, q_n = q.iterate(n_it)
    assert (T is not None, no_more, n, s.iterations, s.best_inliers) == (h is not None, q_no_more, q_n, q.iterations, q.best_inliers)
    assert len(inl) == 2 * len(idx)
    if h is None:
        assert not inl.any()
    else:
        assert T[0, 3] == h + 1 and T[3].tolist() == [0, 0, 0, 1]                      # that hypothesis' transform ...
        assert sorted(np.flatnonzero(inl)) == sorted(idx[:counts[h]])                  # ... and its inliers through mvnIndices1
    if q.best is not None:                                                             # GetEstimated*: the running best, kept
        assert s.estimated_translation()[0] == q.best + 1 and s.estimated_scale() == q.best + 1
    return h, no_more


@pytest.mark.parametrize("case", ["accepts", "never", "accept_on_last", "random"])
def test_python_class_follows_the_sequential_semantics(case):
    """Sim3Solver.iterate / find / set_ransac_parameters of sivo_amd/sim3_solver.py (what SIVO::Sim3Solver is compared with on the
    GPU) against the checker, call by call, on hand-made counts."""
    N = 50
    counts, par, step = {
        "accepts": ([3, 20, 7, 21, 21, 40, 2, 40], (0.99, 20, 8), 3),       # 20 is not above 20; equal counts; several accepts
        "never": ([5, 9, 2, 9, 4, 0, 9], (0.99, 20, 7), 5),                 # the later of equal bests, bNoMore at 7
        "accept_on_last": ([1, 2, 30], (0.99, 20, 3), 5),                   # the accepting call says bNoMore = false, the next true
        "random": (list(np.random.default_rng(4).integers(0, 24, 23)), (0.99, 20, 23), 5),
    }[case]
    s, q, idx = _class_and_checker(counts, N, par)
    assert s.max_its == q.max_its == len(counts)
    seen = []
    for _ in range(len(counts) + 2):
        seen.append(_same_call(s, q, idx, counts, step))
    assert seen[-1] == (None, True) and s.iterations == len(counts)
    if case == "accept_on_last":
        assert seen[:2] == [(2, False), (None, True)]
    # SetRansacParameters starts the count again and keeps mnBestInliers (:115-141 touch mnIterations only): a second pass
    # accepts only what reaches the first pass' best
    best_before = s.best_inliers
    for o in (s, q):
        o.set_ransac_parameters(*par)
    assert s.result is None and (s.iterations, s.best_inliers) == (0, best_before)
    s.result = _fake_result(counts, N)
    T, _, n = s.find()
    h, q_n = q.find()
    assert (T is not None, n, s.best_inliers) == (h is not None, q_n, q.best_inliers)
    assert case != "never" or (h is None and q.best == 6)                             # 9 >= 9: the last 9 of the second pass


def test_python_class_exits():
    s, q, idx = _class_and_checker([50] * 10, 19, (0.99, 20, 10))                     # N < minInliers: at once, nothing evaluated
    s.result = None
    T, no_more, inl, n = s.iterate(5)
    assert (T, no_more, n, s.iterations, len(inl)) == (None, True, 0, 0, 38) and q.iterate(5) == (None, True, 0)
    s, q, idx = _class_and_checker([20], 20, (0.99, 20, 300))                         # minInliers == N: one iteration
    assert s.max_its == q.max_its == 1 and _same_call(s, q, idx, [20], 5) == (None, True)
    for p, m, N in ((0.99, 20, 100), (0.99, 20, 25), (0.9, 6, 30), (0.99, 20, 19)):
        s, q, idx = _class_and_checker([0] * 300, N, (p, m, 300))
        assert s.max_its == q.max_its == R.ransac_iterations(p, m, 300, N)


@pytest.mark.parametrize("fix_scale", [True, False])
def test_coincident_sample_gives_no_inliers(fix_scale):
    sc = R.make_scene(40, 41, noise=0.0, duplicates=3)
    with np.errstate(all="raise"):                                                       # (the restatement silences its own NaNs)
        res = R.ransac(sc["pairs"], sc["k1"], sc["k2"], [[0, 1, 2], [2, 0, 1], [5, 6, 7]], 20, fix_scale)
    assert list(res["count"]) == [0, 0, 40] and not res["inliers"][:2].any()
    assert np.isnan(res["T"][:2, :12]).all()             # |v| = 0: the reference's axis is 0 / 0 and its matrix NaN


def test_header_declares_and_library_exports_the_entry_points():
    h = open(os.path.join(ROOT, "include", "sivo_hip.h")).read()
    assert "int sivo_sim3_ransac_batch(SivoSim3RansacProblem *problems, int n_problems);" in h
    assert "int sivo_sim3_ransac(SivoSim3RansacProblem *problem);" in h and "} SivoSim3Pair;" in h
    from sivo_amd import _lib, sim3_solver
    L = _lib.lib()
    assert hasattr(L, "sivo_sim3_ransac") and hasattr(L, "sivo_sim3_ransac_batch")
    assert sim3_solver.SIM3_PAIR_DTYPE.itemsize == R.PAIR_DTYPE.itemsize == C.sizeof(_lib.Sim3Pair) == 32


def test_ctypes_structs_match_the_header(tmp_path):
    from sivo_amd import _lib
    host_prog.c_layout(tmp_path, "SivoSim3Pair", _lib.Sim3Pair)
    host_prog.c_layout(tmp_path, "SivoSim3RansacProblem", _lib.Sim3RansacProblem)
    assert C.sizeof(_lib.Sim3Pair) == 32


def test_entry_points_check_arguments_and_fail_loudly_without_a_device():
    from sivo_amd import _lib, sim3_solver
    sc = R.make_scene(12, 5, n_hyp=4)
    args = (sc["pairs"], sc["k1"], sc["k2"])
    # invalid arguments are reported as such before any device is needed
    for tri in ([[0, 1, 1]], [[0, 1, 2], [3, 3, 4]], [[0, 1, 12]], [[-1, 1, 2]]):
        with pytest.raises(_lib.SivoInvalidArgument):
            sim3_solver.sim3_ransac(*args, tri)
    with pytest.raises(_lib.SivoInvalidArgument):
        sim3_solver.sim3_ransac(sc["pairs"][:2], sc["k1"], sc["k2"], [[0, 1, 0]])
    with pytest.raises(_lib.SivoInvalidArgument):
        sim3_solver.sim3_ransac(sc["pairs"][:2], sc["k1"], sc["k2"], [[0, 1, 1]])            # n = 2
    P = _lib.Sim3RansacProblem()
    P.n, P.n_hyp = 5, 0                                                                      # a NULL array with a non-zero count
    assert _lib.lib().sivo_sim3_ransac(C.byref(P)) == _lib.ERR_INVALID_ARGUMENT
    # nothing to do: no launch, no device needed
    assert sim3_solver.sim3_ransac_batch([]) == []
    empty = sim3_solver.sim3_ransac(*args, np.zeros((0, 3), np.int32))
    assert (empty["first_accept"], empty["best"]) == (-1, -1) and len(empty["count"]) == 0
    if _lib.lib().sivo_device_count() >= 1:            # (a device is visible: the call runs; tests/test_gpu_sim3_ransac.py checks what it computes)
        assert len(sim3_solver.sim3_ransac(*args, sc["triples"])["count"]) == 4
        return
    with pytest.raises(_lib.SivoError) as e:
        sim3_solver.sim3_ransac(*args, sc["triples"])
    assert e.value.code == _lib.ERR_RUNTIME
    with pytest.raises(_lib.SivoError) as e:
        sim3_solver.sim3_ransac_batch([{"pairs": sc["pairs"], "k1": sc["k1"], "k2": sc["k2"], "triples": sc["triples"]}])
    assert e.value.code == _lib.ERR_RUNTIME
    s = sim3_solver.Sim3Solver(*args, randint=R.seeded_randint(1))
    with pytest.raises(_lib.SivoError):
        s.find()


STAND_INS = r'''#include "orbslam/Sim3Solver.h"
struct KeyFrame;
struct MapPoint { cv::Mat GetWorldPos() const { return cv::Mat(3, 1, CV_32F); } bool isBad() const { return false; }
                  int GetIndexInKeyFrame(KeyFrame *) const { return 0; } };
struct KeyFrame { cv::Mat mK; std::vector<cv::KeyPoint> mvKeysSemantic; std::vector<float> mvLevelSigma2;
                  cv::Mat GetRotation() const { return cv::Mat(3, 3, CV_32F); } cv::Mat GetTranslation() const { return cv::Mat(3, 1, CV_32F); }
                  std::vector<MapPoint *> GetMapPointMatches() const { return {}; } };
using namespace SIVO;
using namespace std;
'''
SNIPPETS = {
    # LoopClosing.cc:281-283, :302-307, :325-327
    "loop": r'''float f(KeyFrame *mpCurrentKF, KeyFrame *pKF, vector<vector<MapPoint *> > &vvpMapPointMatches, int i, bool mbFixScale) {
    Sim3Solver *pSolver = new Sim3Solver(mpCurrentKF, pKF, vvpMapPointMatches[i], mbFixScale);
    pSolver->SetRansacParameters(0.99, 20, 300);
    vector<bool> vbInliers;
    int nInliers;
    bool bNoMore;
    cv::Mat Scm = pSolver->iterate(5, bNoMore, vbInliers, nInliers);
    cv::Mat R = pSolver->GetEstimatedRotation();
    cv::Mat t = pSolver->GetEstimatedTranslation();
    const float s = pSolver->GetEstimatedScale();
    Sim3Solver second(mpCurrentKF, pKF, vvpMapPointMatches[i]);
    Scm = second.find(vbInliers, nInliers);
    return Scm.empty() || bNoMore ? s : R.at<float>(0, 0) + t.at<float>(0);
}
''',
    "solve_all": r'''void g(vector<Sim3Solver *> &vpSim3Solvers) {
    Sim3Solver::SolveAll(vpSim3Solvers);
    vpSim3Solvers[0]->SetDraw([](int lo, int hi) { return (lo + hi) / 2; });
}
''',
}


@pytest.mark.parametrize("snippet", list(SNIPPETS))
def test_class_instantiates_over_stand_in_types(tmp_path, snippet):
    tu = tmp_path / "use.cpp"
    tu.write_text(STAND_INS + SNIPPETS[snippet])
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-I" + API, str(tu)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.parametrize("random_pose", [False, True])
def test_gather_matches_the_reference_walk(tmp_path, random_pose):
    sc = R.make_scene(30, 8)
    kf1, kf2, pts, m12 = R.keyframe_pair(sc, 9, random_pose=random_pose, n_extra=18)
    exe = host_prog.build("sim3_ransac_prog", tmp_path, link_lib=True)
    out = host_prog.run_text(exe, ["gather"], "1\n" + R.scene_text(sc, kf1, kf2, pts, m12, True), 60)
    rows = [ln.split() for ln in out.strip().splitlines()]
    idx, recs = R.gather(kf1, kf2, m12, pts)
    assert [int(w[1]) for w in rows] == list(idx)
    assert len(idx) == 30 and len(m12) == 48                 # every pair of the scene, none of the 18 entries to skip
    got = np.array([[float.fromhex(v) for v in w[2:]] for w in rows], np.float32)
    want = np.concatenate([recs["x1c"], recs["x2c"], recs["max_err1"][:, None], recs["max_err2"][:, None]], 1)
    assert got.tobytes() == want.tobytes()
    assert set(recs["max_err1"].tolist()) > {9.0, 13.0}      # (unsigned long)(9.210 * sigma2): octave-dependent, truncated
    if not random_pose:                                      # identity poses: the scene's own pairs come back
        order = np.argsort([kf1["mp"][i] for i in idx])
        assert recs[order].tobytes() == sc["pairs"].tobytes()
