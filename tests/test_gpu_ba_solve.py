"""GPU parity of the LM / Schur loops (sivo_ba_optimize, sivo_local_ba, sivo_pose_optimize) vs the oracle.
fp64 with a different (but fixed) summation order than the oracle's sequential loops: tolerances are stated per
quantity; inlier/outlier decisions must be identical."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_ba_scene, perturb_pose
from sivo_amd import optimizer

pytestmark = pytest.mark.gpu


def _start(poses, pts, n_fixed, seed, rot=0.002, trans=0.02, dx=0.05):
    rng = np.random.default_rng(seed)
    fixed = np.zeros(len(poses), np.uint8); fixed[:n_fixed] = 1
    P0 = poses.copy()
    for i in range(n_fixed, len(poses)):
        P0[i] = perturb_pose(poses[i], rng, rot, trans)
    return P0, fixed, pts + rng.normal(0, dx, pts.shape)


@pytest.mark.parametrize("iters", [1, 4])
def test_ba_optimize_matches_oracle(oracle, iters):
    poses, pts, edges, intr = make_ba_scene(seed=4, n_kf=6, n_pts=300)
    P0, fixed, X0 = _start(poses, pts, 2, 0)
    g = optimizer.ba_optimize(P0, fixed, X0, edges, intr, iters)
    o = oracle.ba_optimize(P0, fixed, X0, edges, intr, iters)
    assert (g["iterations"], g["trials"]) == (o["iterations"], o["trials"])
    np.testing.assert_allclose(g["poses"], o["poses"], atol=1e-10, rtol=0)
    np.testing.assert_allclose(g["points"], o["points"], atol=1e-9, rtol=0)
    np.testing.assert_allclose(g["err"], o["err"], atol=1e-8, rtol=0)
    np.testing.assert_allclose(g["hpp"], o["hpp"], rtol=1e-9, atol=1e-6)
    assert np.array_equal(g["poses"][:2], P0[:2])


def test_ba_optimize_levels_kernels_and_degenerate_graphs(oracle):
    poses, pts, edges, intr = make_ba_scene(seed=7, n_kf=5, n_pts=200)
    P0, fixed, X0 = _start(poses, pts, 1, 1)
    rng = np.random.default_rng(2)
    level = (rng.random(len(edges)) < 0.2).astype(np.uint8); robust = (rng.random(len(edges)) < 0.5).astype(np.uint8)
    g = optimizer.ba_optimize(P0, fixed, X0, edges, intr, 3, level, robust)
    o = oracle.ba_optimize(P0, fixed, X0, edges, intr, 3, level, robust)
    assert (g["iterations"], g["trials"]) == (o["iterations"], o["trials"])
    np.testing.assert_allclose(g["poses"], o["poses"], atol=1e-10, rtol=0)
    np.testing.assert_allclose(g["points"], o["points"], atol=1e-9, rtol=0)
    assert np.array_equal(g["err"][level == 1], np.zeros((int(level.sum()), 3)))       # inactive edges are never evaluated
    # every keyframe fixed: structure-only refinement
    allfixed = np.ones(len(poses), np.uint8)
    g = optimizer.ba_optimize(poses, allfixed, X0, edges, intr, 2)
    o = oracle.ba_optimize(poses, allfixed, X0, edges, intr, 2)
    np.testing.assert_allclose(g["points"], o["points"], atol=1e-9, rtol=0)
    assert np.array_equal(g["poses"], poses)
    # no edges: nothing to do, nothing crashes
    g = optimizer.ba_optimize(P0, fixed, X0, edges[:0], intr, 2)
    assert np.array_equal(g["poses"], P0) and np.array_equal(g["points"], X0)
    # duplicate (keyframe, map point) observation is refused
    dup = np.concatenate([edges, edges[edges["pose"] == 2][:1]])           # a free keyframe's observation, twice
    with pytest.raises(ValueError, match="same"):
        optimizer.ba_optimize(P0, fixed, X0, dup, intr, 1)


def test_ba_optimize_more_than_21_free_keyframes(oracle):
    """28 free keyframes: the reduced system (168 x 168) no longer fits the LDS-resident Cholesky and takes the
    global-memory path of the same blocked solver."""
    poses, pts, edges, intr = make_ba_scene(seed=12, n_kf=30, n_pts=400)
    P0, fixed, X0 = _start(poses, pts, 2, 5)
    g = optimizer.ba_optimize(P0, fixed, X0, edges, intr, 3)
    o = oracle.ba_optimize(P0, fixed, X0, edges, intr, 3)
    assert (g["iterations"], g["trials"]) == (o["iterations"], o["trials"])
    np.testing.assert_allclose(g["poses"], o["poses"], atol=1e-9, rtol=0)
    np.testing.assert_allclose(g["points"], o["points"], atol=1e-8, rtol=0)


def test_local_ba_config5_matches_oracle(oracle):
    """20 keyframes x 3000 map points (~36 k edges), the first two keyframes fixed."""
    poses, pts, edges, intr = make_ba_scene()
    P0, fixed, X0 = _start(poses, pts, 2, 3)
    g = optimizer.local_ba(P0, fixed, X0, edges, intr, cov_pose=19)
    o = oracle.local_ba(P0, fixed, X0, edges, intr, cov_pose=19)
    assert (g["iterations"], g["trials"]) == (o["iterations"], o["trials"])
    np.testing.assert_allclose(g["poses"], o["poses"], atol=1e-9, rtol=0)
    np.testing.assert_allclose(g["points"], o["points"], atol=1e-7, rtol=0)
    # device and oracle err agree to 1e-8 (test_ba_optimize_matches_oracle): < 6e-8 in chi2 at the thresholds, so only an edge whose
    # chi2 lies within 1e-6 of 5.991 / 7.815 may flip, and every observation the first classification excluded is reported
    decided = np.abs(o["chi2"] - np.where(edges["stereo"] != 0, 7.815, 5.991)) > 1e-6
    assert np.array_equal(g["outlier"][decided], o["outlier"][decided])
    assert g["outlier"][o["level"] != 0].all()
    assert g["cov_ok"] and o["cov_ok"]
    np.testing.assert_allclose(g["cov"], o["cov"], rtol=1e-7, atol=1e-16)
    assert np.abs(g["poses"] - poses).max() < np.abs(P0 - poses).max()
    # reproducible run to run (fixed summation order, no atomics)
    g2 = optimizer.local_ba(P0, fixed, X0, edges, intr, cov_pose=19)
    assert np.array_equal(g2["poses"], g["poses"]) and np.array_equal(g2["points"], g["points"])
    # pbStopFlag raised before the call: untouched (Optimizer.cc:757-761)
    stop = C.c_uint8(1)
    s = optimizer.local_ba(P0, fixed, X0, edges, intr, stop=stop)
    assert np.array_equal(s["poses"], P0) and s["iterations"] == 0 and not s["outlier"].any()


@pytest.mark.parametrize("kf,seed", [(5, 0), (0, 1), (19, 2)])
def test_pose_optimization_matches_oracle(oracle, kf, seed):
    poses, pts, edges, intr = make_ba_scene()
    ek = edges[edges["pose"] == kf].copy()
    p0 = perturb_pose(poses[kf], np.random.default_rng(seed))
    g = optimizer.pose_optimize(p0, pts, ek, intr)
    o = oracle.pose_optimize(p0, pts, ek, intr)
    # Once converged, chi_new - chi is rounding noise, so the accept/reject sign of the last trials (and with it
    # the trial COUNT) depends on the summation order; the state they converge to does not.
    assert 4 <= g["iterations"] <= 40 and g["iterations"] <= g["trials"] <= 400
    np.testing.assert_allclose(g["pose"], o["pose"], atol=1e-7, rtol=0)
    assert np.array_equal(g["outlier"], o["outlier"]) and g["inliers"] == o["inliers"]
    np.testing.assert_allclose(g["chi2"], o["chi2"], rtol=1e-4, atol=1e-4)
    assert g["cov_ok"] and o["cov_ok"]
    np.testing.assert_allclose(g["cov"], o["cov"], rtol=1e-6, atol=1e-18)
    g2 = optimizer.pose_optimize(p0, pts, ek, intr)                       # fixed summation order: reproducible
    assert np.array_equal(g2["pose"], g["pose"]) and g2["trials"] == g["trials"]
    assert np.abs(g["pose"] - poses[kf]).max() < 2e-2 < np.abs(p0 - poses[kf]).max()


def test_pose_optimization_more_edges_than_the_lds_copy_holds(oracle):
    """pose_optimize_kernel keeps 2560 edges in LDS and reads the rest from memory in every pass: one keyframe seeing ~5000 points
    (with planted outliers, so that flags beyond the LDS copy change), then the same call timed at a tracking-sized problem."""
    import time
    poses, pts, edges, intr = make_ba_scene(seed=11, n_kf=2, n_pts=9000)
    ek = edges[edges["pose"] == 1].copy()
    assert len(ek) > 3000
    rng = np.random.default_rng(5)
    planted = rng.choice(len(ek), 150, replace=False)
    ek["obs"][planted, 0] += rng.choice([-1, 1], 150) * rng.uniform(8, 30, 150)
    p0 = perturb_pose(poses[1], np.random.default_rng(6))
    g = optimizer.pose_optimize(p0, pts, ek, intr); o = oracle.pose_optimize(p0, pts, ek, intr)
    np.testing.assert_allclose(g["pose"], o["pose"], atol=1e-7, rtol=0)
    assert np.array_equal(g["outlier"], o["outlier"]) and g["inliers"] == o["inliers"] and g["outlier"][2560:].any()
    np.testing.assert_allclose(g["chi2"], o["chi2"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(g["cov"], o["cov"], rtol=1e-6, atol=1e-18)
    for n in (300, 1000, 2000, len(ek)):
        sub = ek[:n]
        optimizer.pose_optimize(p0, pts, sub, intr)
        t0 = time.perf_counter()
        for _ in range(20):
            r = optimizer.pose_optimize(p0, pts, sub, intr)
        print(f"[pose_optimize {n} edges] {(time.perf_counter() - t0) / 20 * 1e3:.3f} ms per call (through ctypes), {r['iterations']} iterations, {r['trials']} trials")


def test_pose_optimization_edge_cases(oracle):
    poses, pts, edges, intr = make_ba_scene(seed=3, n_kf=2, n_pts=60)
    ek = edges[edges["pose"] == 1].copy()
    p0 = perturb_pose(poses[1], np.random.default_rng(4), 0.005, 0.05)
    r = optimizer.pose_optimize(p0, pts, ek[:2], intr)                    # < 3 correspondences (:409-411)
    assert r["inliers"] == 0 and np.array_equal(r["pose"], p0) and not r["cov_ok"]
    for n in (3, 9, 10, len(ek)):                                          # < 10 edges: a single round (:469-471)
        g = optimizer.pose_optimize(p0, pts, ek[:n], intr); o = oracle.pose_optimize(p0, pts, ek[:n], intr)
        assert (g["iterations"] <= 10) == (n < 10)                         # one round only when < 10 edges
        np.testing.assert_allclose(g["pose"], o["pose"], atol=1e-6, rtol=0)
        assert np.array_equal(g["outlier"], o["outlier"])
    mono = ek.copy(); mono["stereo"] = 0                                   # mono only: never re-classified
    g = optimizer.pose_optimize(p0, pts, mono, intr); o = oracle.pose_optimize(p0, pts, mono, intr)
    assert not g["outlier"].any() and g["inliers"] == len(mono) == o["inliers"]
    np.testing.assert_allclose(g["pose"], o["pose"], atol=1e-7, rtol=0)
    bad = ek.copy(); bad["point"][0] = 10 ** 6
    with pytest.raises(ValueError):
        optimizer.pose_optimize(p0, pts, bad, intr)


def _small_scene():
    poses, pts, edges, intr = make_ba_scene(seed=4, n_kf=6, n_pts=300)
    P0, fixed, X0 = _start(poses, pts, 2, 0)
    return P0, fixed, X0, edges, intr


def _in_new_thread(fn):
    """fn() on a thread of its own: the solvers' buffers are per thread, so they start empty there."""
    import threading
    box = {}

    def run():
        try:
            box["result"] = fn()
        except BaseException as e:       # noqa: BLE001 (handed to the caller's thread)
            box["error"] = e
    t = threading.Thread(target=run); t.start(); t.join()
    if "error" in box:
        raise box["error"]
    return box["result"]


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_solves_do_not_wait_for_the_default_stream():
    """LocalBundleAdjustment (both paths), BundleAdjustment with a stop flag and PoseOptimization beyond the LDS copy run on streams of
    their own and read their results through pinned memory: behind a kernel that occupies PyTorch's default (null) stream they return,
    with the results of an undisturbed run, while that kernel is still running."""
    import time
    import torch
    small = _small_scene()
    rng = np.random.default_rng(2)
    nE = len(small[3])
    level = (rng.random(nE) < 0.2).astype(np.uint8); robust = (rng.random(nE) < 0.5).astype(np.uint8)
    stop = C.c_uint8(0)                                                     # passed, never raised
    poses, pts, edges, intr = make_ba_scene(seed=11, n_kf=2, n_pts=9000)
    ek = edges[edges["pose"] == 1].copy()
    assert len(ek) > 3000                                                   # more than pose_optimize_kernel keeps in LDS
    p0 = perturb_pose(poses[1], np.random.default_rng(6))
    calls = [lambda: optimizer.local_ba(*small, cov_pose=5, solver="dense"),
             lambda: optimizer.local_ba(*small, cov_pose=5, solver="sparse"),
             lambda: optimizer.ba_optimize(*small, 2, level, robust, stop=stop),
             lambda: optimizer.pose_optimize(p0, pts, ek, intr)]
    warm = [f() for f in calls]                  # buffers, the stop word and event, the kernel attributes now exist
    t0 = time.perf_counter()
    for f, w in zip(calls, warm):
        _assert_same(f(), w)
    t_warm = time.perf_counter() - t0
    torch.cuda._sleep(1000)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    probe = 2_000_000
    e0.record(); torch.cuda._sleep(probe); e1.record(); torch.cuda.synchronize()
    per_cycle = e0.elapsed_time(e1) * 1e-3 / probe
    want = min(max(0.3, 20 * t_warm), 2.0)
    print(f"[default stream] warm calls {t_warm * 1e3:.2f} ms, spin {want:.2f} s ({per_cycle * 1e9:.2f} ns per cycle)")
    busy = torch.cuda.Event()
    torch.cuda._sleep(int(want / per_cycle)); busy.record()
    try:
        for f, w in zip(calls, warm):
            r = f()
            assert not busy.query()              # the call returned while the default stream was still busy
            _assert_same(r, w)
    finally:
        torch.cuda.synchronize()


@pytest.mark.parametrize("solver", ["dense", "sparse"])
def test_ba_buffers_regrown_for_a_larger_problem_keep_no_state(solver):
    """A small problem, config 5 (~36 k edges: the device and pinned buffers the small one left do not hold it), the small one again —
    on a fresh thread, whose buffers start empty."""
    small = _small_scene()
    poses, pts, edges, intr = make_ba_scene()
    big = (*_start(poses, pts, 2, 3), edges, intr)

    def run():
        return [optimizer.local_ba(*s, cov_pose=len(s[0]) - 1, solver=solver) for s in (small, big, small)]
    first, mid, third = _in_new_thread(run)
    assert first["iterations"] > 0 and mid["iterations"] > 0 and first["cov_ok"]
    _assert_same(first, third)


def test_ba_follows_the_calling_threads_device():
    """The stream, the buffers, the stop word and its event belong to the device they were made on: all are rebuilt when the calling
    thread's current device has changed."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    small = _small_scene()
    stop = C.c_uint8(0)
    before = torch.cuda.current_device()
    try:
        res = []
        for dev in (0, 1, 0):
            torch.cuda.set_device(dev)
            res.append(optimizer.local_ba(*small, cov_pose=5, stop=stop))
    finally:
        torch.cuda.set_device(before)
    _assert_same(res[0], res[1])
    _assert_same(res[0], res[2])
