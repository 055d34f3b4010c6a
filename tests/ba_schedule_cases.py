"""LocalBundleAdjustment under other iteration budgets than the reference's (5, 10): the case table shared by tests/test_ba_schedule_host.py
and tests/test_gpu_ba_schedule.py, the oracle's run of every case (computed once), a NumPy model of the device solver's two per-edge error
sets fed by the oracle's trace, and the binding of the debug entry that runs the product's function under a budget.

Why budgets: g2o's edges keep ONE error vector each, and an edge that the first classification put at level 1 is never evaluated again, so
the chi2 the final classification reads is the one that excluded it (Optimizer.cc:786-810, :837 / :853).  The device solver
(sivo_amd/csrc/ba_solve.hip) keeps one per-edge set per estimate buffer and classifies on the set written last.  Whether that is the same
set at both classifications depends on the parity of the accepted trials of the second optimize() call: even under (5, 10) on every scene
tried, odd half the time when tracking raises pbStopFlag during optimize(10).  A budget is that abort at an iteration boundary, reached
without a second thread."""
import ctypes as C
import functools

import numpy as np

from conftest import make_ba_scene, perturb_pose

CHI2_MONO, CHI2_STEREO = 5.991, 7.815          # Optimizer.cc:786-810, :837 / :853
# Device and oracle err agree to 1e-8 (test_ba_optimize_matches_oracle); at chi2 ~ 6-8 and inv_sigma2 <= 1 that is < 6e-8 in chi2.  No
# case may have an edge this close to its threshold, at either classification: the flags are then comparable exactly.
BAND = 1e-6

# (seed, (it_first, it_second)).  ODD: the final classification reads the other set than the first (one accepted trial per iteration, an
# odd it_second); the seeds are those whose modelled flags differ from the oracle's in at least 2 edges, and at least 1 for the budget-5
# cases (5 is the product's first call).  CONTROLS: an even it_second, the same set twice.
ODD = [(1, (1, 1)), (5, (1, 1)), (1, (2, 1)), (2, (2, 1)), (0, (3, 7)), (5, (3, 7)), (2, (5, 1)), (3, (5, 3))]
MIN_FLIPS = {(1, 1): 2, (2, 1): 2, (3, 7): 2, (5, 1): 1, (5, 3): 1}
CONTROLS = [(2, (5, 10)), (3, (5, 2))]
CASES = ODD + CONTROLS


def case_id(case):
    seed, (a, b) = case
    return f"seed{seed}-{a}x{b}"


@functools.lru_cache(maxsize=None)
def scene(seed):
    """make_ba_scene(seed, 6 keyframes, 300 points): 1200-1330 edges, the first two keyframes fixed, the start perturbed from seed + 100."""
    poses, pts, edges, intr = make_ba_scene(seed, n_kf=6, n_pts=300)
    rng = np.random.default_rng(seed + 100)
    fixed = np.zeros(len(poses), np.uint8); fixed[:2] = 1
    P0 = poses.copy()
    for i in range(2, len(poses)):
        P0[i] = perturb_pose(poses[i], rng, 0.002, 0.02)
    X0 = pts + rng.normal(0, 0.05, pts.shape)
    for a in (P0, fixed, X0, edges):
        a.setflags(write=False)
    return P0, fixed, X0, edges, intr


@functools.lru_cache(maxsize=None)
def reference(case):
    """The oracle's run of a case, with its trace.  Shared between the tests: read-only."""
    from oracle import oracle as O
    seed, budget = case
    o = O.local_ba(*scene(seed), budget=budget, trace=True)
    for v in o.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return o


def thresholds(edges):
    return np.where(edges["stereo"] != 0, CHI2_STEREO, CHI2_MONO)


def chi2_of(err, edges):
    return (err[:, 0] * err[:, 0] + err[:, 1] * err[:, 1] + err[:, 2] * err[:, 2]) * edges["inv_sigma2"]


def two_set_model(o, edges, mirror_on_level):
    """The device solver's bookkeeping replayed on the oracle's trace: two per-edge error sets; the first linearisation of a call writes
    set `cur`; every trial writes `cur ^ 1`, which becomes `last_set`; an accepted trial flips `cur`; a later linearisation evaluates
    nothing (the accepted trial left its errors); an edge at level 1 is skipped by every write.  The first classification reads set S1,
    the `last_set` after the first call, the final one S2.  mirror_on_level: the first classification copies the errors of every edge it
    levels into the other set as well.  Returns S1, S2, the final flags, and chi2 of set S1 as the first classification read it."""
    nE = len(edges)
    err = np.zeros((2, nE, 3)); cur = last = 0
    active = np.ones(nE, bool)
    calls = 0; s1 = None; chi2_first = None
    for kind, e in o["trace"]:
        if kind == "call_start":
            calls += 1
            if calls == 2:
                s1 = last
                chi2_first = chi2_of(err[s1], edges)
                leveled = o["level"] != 0
                assert not ((chi2_first > thresholds(edges)) & ~leveled).any()      # (the rest of `level` is the depth test)
                if mirror_on_level:
                    err[s1 ^ 1][leveled] = err[s1][leveled]
                active = ~leveled
            err[cur][active] = e[active]; last = cur
        elif kind == "linearisation":
            assert last == cur and np.array_equal(err[cur][active], e[active])      # the same estimate: nothing new to write
        else:
            err[cur ^ 1][active] = e[active]; last = cur ^ 1
            if kind == "trial_accepted":
                cur ^= 1
    assert calls == 2
    flags = (chi2_of(err[last], edges) > thresholds(edges)) | (o["depth_ok"] == 0)
    return s1, last, flags.astype(np.uint8), chi2_first


def device_local_ba(poses, fixed, points, edges, intr, budget, cov_pose=-1, solver="auto"):
    """sivo_debug_local_ba_budget (libsivo_hip_dbg.so): the product's LocalBundleAdjustment under an iteration budget."""
    from sivo_amd import _lib, optimizer
    poses = np.array(poses, np.float64).reshape(-1, 12).copy(); points = np.array(points, np.float64).reshape(-1, 3).copy()
    fixed = np.ascontiguousarray(fixed, np.uint8); edges = np.ascontiguousarray(edges, optimizer.EDGE_DTYPE)
    nE = edges.shape[0]
    outlier = np.zeros(nE, np.uint8); cov = np.zeros((6, 6)); ok = C.c_int(0); n = C.c_int(0); tr = C.c_int(0)
    opts = optimizer._ba_options(solver)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = _lib.dbg().sivo_debug_local_ba_budget(vp(poses), vp(fixed), poses.shape[0], vp(points), points.shape[0], vp(edges), nE,
                                               (C.c_double * 5)(*[float(v) for v in intr]), None, vp(outlier), cov_pose, vp(cov),
                                               C.byref(ok), C.byref(n), C.byref(tr), int(budget[0]), int(budget[1]),
                                               None if opts is None else C.addressof(opts))
    if rc != _lib.OK:
        raise _lib.SivoError(rc, _lib.lib().sivo_last_error().decode(errors="replace"))
    return {"poses": poses, "points": points, "outlier": outlier, "cov": cov, "cov_ok": bool(ok.value),
            "iterations": n.value, "trials": tr.value}
