"""PnPsolver's EPnP RANSAC without a GPU: the sequential semantics of iterate / find / Refine on hand-made counts,
SetRansacParameters against its formula, the shipped Python class against the checker, the restatement against an independent
EPnP written with LAPACK (numpy.linalg) and against the true pose, the kernel's arithmetic compiled for the host against the
restatement (bit for bit), the C ABI's presence, argument checks and loud failure without a device, SIVO::PnPsolver's interface
over stand-in types, and its gather against the restatement of PnPsolver.cc:72-121 (bit-exact floats)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import host_prog
import pnp_ransac_restatement as R

API = os.path.join(ROOT, "sivo_amd", "api")
CSRC = os.path.join(ROOT, "sivo_amd", "csrc")

# EPnP on exact correspondences, the restatement against the LAPACK form (lapack_epnp below) and against the true pose, measured
# here on the CPU over 6 seeds x 300 samples of the generator's noise-free scenes (seeds 11 .. 16, 60 points, every sample
# all-inlier).  A sample is well-conditioned when the smallest PCA eigenvalue of its 4 points is above COND_MIN of the largest:
# 80.9 % of the samples are.
#
# What the measurement shows: compute_pose on FOUR points is not a reliable solver, in either form.  M'M has a 4-dimensional null
# space there, find_betas_approx_1/2/3 each assume that one, two or three vectors of its basis carry the solution, and five
# Gauss-Newton iterations from those starts reach the pose only when the basis happens to suit: the restatement reproduces its
# sample within 1e-3 px on 36.7 % of the samples, the LAPACK form on 34.2 %, on DIFFERENT samples (both on 13 % of them), because
# Jacobi and LAPACK return different bases; rotating LAPACK's basis by a random orthogonal matrix changes which samples succeed in
# the same way.  (The reference has the same property with cvSVD's basis; its RANSAC loop absorbs it.)  So the worst deviation
# between the two forms over the well-conditioned samples is a wrong minimum of one of them: 1.99 (R) and 27.1 (t), against the
# true pose 1.99 and 24.8, and ten times that, rounded, is a bound that nothing can miss.  It is asserted as asked (EPNP_TOL),
# and beside it the statement that does hold: where BOTH forms reproduce their sample within CONV_PX = 1e-3 px they found the
# same minimum and agree within rounding through the sample's conditioning.  Measured worst case there: 2.9e-6 (R), 3.5e-5 (t)
# between the forms; 2.4e-5 (R), 1.7e-4 (t) between the restatement and the true pose wherever the restatement converged.
# CONV_TOL / TRUE_TOL are ten times those, rounded.  The shares of converged samples are compared too: the bases are equally
# arbitrary, so the shares differ by sampling only (sigma = sqrt(2 * 0.35 * 0.65 / 1800) = 0.016; three sigma = 0.05).
COND_MIN = 2e-3
CONV_PX = 1e-3
EPNP_TOL = {"R": 20.0, "t": 300.0}
CONV_TOL = {"R": 3e-5, "t": 4e-4}
TRUE_TOL = {"R": 3e-4, "t": 2e-3}
SEEDS = (11, 12, 13, 14, 15, 16)


def source_constants():
    src = open(os.path.join(CSRC, "pnp_epnp.hpp")).read()
    m = re.search(r"PNP_SWEEPS3 = (\d+), PNP_SWEEPS12 = (\d+), PNP_SWEEPS_SVD = (\d+);", src)
    return tuple(int(v) for v in m.groups())


def test_restatement_reads_the_sources_sweep_counts():
    assert source_constants() == (R.SWEEPS3, R.SWEEPS12, R.SWEEPS_SVD)


# ---------------------------------------------------------------------------------------------------------------------
# sequential semantics
# ---------------------------------------------------------------------------------------------------------------------
def _bits(N, c):
    return np.arange(N) < c


def _seq(counts, refined_of, N=50, min_inliers=10, max_its=None):
    """counts[h]: the count of hypothesis h (inliers 0 .. count-1, T = h + 1 everywhere); refined_of: best count -> refined count."""
    calls, refines = [], []

    def evaluate(h):
        calls.append(h)
        return counts[h], np.full(12, h + 1, np.float32), _bits(N, counts[h])

    def refine(bits):
        c = int(np.sum(bits))
        refines.append(c)
        return refined_of[c], np.full(12, -c, np.float32), _bits(N, refined_of[c])
    return R.Sequential(N, min_inliers, len(counts) if max_its is None else max_its, evaluate, refine), calls, refines


def test_count_equal_to_min_inliers_refines_and_equal_refined_count_is_not_accepted():
    s, calls, refines = _seq([3, 10, 4, 12], {10: 10, 12: 13})
    T, no_more, inl, n = s.iterate(5)
    assert refines == [10, 12]                        # 10 >= minInliers triggers Refine; its refined 10 is not > 10
    assert (no_more, n, calls) == (False, 13, [0, 1, 2, 3]) and T[0, 0] == -12 and inl.sum() == 13


def test_non_record_count_reuses_the_refinement_of_the_unchanged_best():
    s, calls, refines = _seq([20, 11, 3, 12, 20], {20: 25}, max_its=5)
    r = [s.iterate(5) for _ in range(4)]
    # 20 is a record: accepted; 11 and 12 are no records but >= minInliers: Refine of the unchanged best returns again; the second
    # 20 is no record either (strict >)
    assert [x[3] for x in r] == [25, 25, 25, 25] and [x[1] for x in r] == [False] * 4
    assert calls == [0, 1, 2, 3, 4] and refines == [20, 20, 20, 20] and s.best_T[0, 0] == 1
    assert s.iterations == 5


def test_without_acceptance_the_first_iterate_runs_all_and_returns_the_best():
    counts = [3, 12, 5, 14, 14, 2, 0]
    s, calls, _ = _seq(counts, {12: 9, 14: 10})
    T, no_more, inl, n = s.iterate(5)                 # the loop condition is an OR: 5 iterations are not enough to stop it
    assert calls == list(range(7)) and (no_more, n) == (True, 14) and T[0, 0] == 4 and inl.sum() == 14      # the first 14


def test_a_call_after_the_maximum_runs_exactly_n_iterations_more():
    counts = [1, 2, 3] + [0] * 12
    s, calls, _ = _seq(counts, {}, max_its=3)
    assert s.iterate(5)[:2] == (None, True) and calls == [0, 1, 2, 3, 4]       # mnIterations < 3 OR nCurrent < 5
    assert s.iterate(5)[:2] == (None, True) and calls == list(range(10))
    assert s.iterate(2)[:2] == (None, True) and calls == list(range(12))


def test_fewer_points_than_min_inliers_returns_at_once():
    s, calls, _ = _seq([50] * 10, {}, N=9)
    assert s.iterate(5)[:2] == (None, True) and calls == [] and s.iterations == 0


def _formula(N, p, m, max_its, eps):
    f32 = np.float32
    n_min = max(int(f32(N) * f32(eps)), m, 4)
    e = max(f32(eps), f32(n_min) / f32(N))
    if n_min == N:
        return n_min, 1
    return n_min, max(1, min(int(np.ceil(np.log(1 - p) / np.log(1 - float(e) ** 3))), max_its))


def test_set_ransac_parameters():
    assert R.ransac_iterations(10, 0.99, 10, 300, 4, 0.5)[:2] == (10, 1)                    # minInliers == N
    m, its, eps = R.ransac_iterations(15, 0.99, 10, 300, 4, 0.5)                             # epsilon raised to minInliers / N
    assert (m, eps) == (10, np.float32(10) / np.float32(15)) and its == int(np.ceil(np.log(0.01) / np.log(1 - float(eps) ** 3))) == 14
    for N, want in ((15, (10, 14)), (40, (20, 35)), (400, (200, 35))):                        # the Tracking call
        assert R.ransac_iterations(N, 0.99, 10, 300, 4, 0.5)[:2] == _formula(N, 0.99, 10, 300, 0.5) == want
    assert R.ransac_iterations(100, 0.99, 8, 300, 4, 0.4)[:2] == _formula(100, 0.99, 8, 300, 0.4) == (40, 70)
    assert R.ransac_iterations(1000, 0.99, 8, 300, 4, 0.1)[:2] == (100, 300)                 # clamped by maxIterations
    assert R.ransac_iterations(100, 0.99, 8, 0, 4, 0.4)[1] == 1                               # clamped from below
    assert R.ransac_iterations(3, 0.99, 2, 300, 4, 0.4)[0] == 4                               # never below minSet


# ---------------------------------------------------------------------------------------------------------------------
# the Python class against the checker
# ---------------------------------------------------------------------------------------------------------------------
def _fake_eval(counts, refined_of, N):
    """What sivo_pnp_ransac would hand the class for these counts: `counts` is consumed in the order the hypotheses are drawn."""
    state = {"next": 0}

    def evaluate(p):
        nh = len(p["samples"])
        c = np.asarray(counts[state["next"]:state["next"] + nh], np.int32)
        assert len(c) == nh
        h0 = state["next"]
        state["next"] += nh
        out = {"count": c, "T": np.repeat(np.arange(h0 + 1, h0 + nh + 1, dtype=np.float32)[:, None], 12, 1),
               "inlier_bits": R.pack_bits(np.arange(N)[None, :] < c[:, None]), "refined": np.full(nh, -1, np.int32),
               "refined_T": np.zeros((nh, 12), np.float32), "refined_bits": np.zeros((nh, (N + 63) // 64), np.uint64)}
        best = p["best_in"]
        for h in range(nh):
            if c[h] >= p["min_inliers"] and c[h] > best:
                best = int(c[h])
                out["refined"][h] = refined_of[best]
                out["refined_T"][h] = -best
                out["refined_bits"][h] = R.pack_bits((np.arange(N) < refined_of[best])[None, :])[0]
        return out
    return evaluate


CASES = {
    # counts, refined_of, (min_inliers, max_its), iterate step
    "accepts": ([3, 20, 7, 21, 21, 40, 2, 40] + [0] * 40, {20: 20, 21: 22, 40: 41}, (20, 8), 3),
    "never": ([5, 19, 2, 25, 4, 0, 25] + [1] * 40, {25: 20}, (20, 7), 5),
    "accept_on_last": ([1, 2, 30] + [0] * 40, {30: 31}, (20, 3), 5),
    "accept_after_the_maximum": ([1, 2, 3, 0, 0, 0, 26, 0, 22, 0] + [0] * 40, {26: 27}, (20, 3), 5),
    "random": (list(np.random.default_rng(4).integers(0, 30, 60)), {c: (c * 7) % 31 for c in range(31)}, (20, 23), 5),
}


@pytest.mark.parametrize("case", list(CASES))
def test_python_class_follows_the_sequential_semantics(case):
    from sivo_amd import pnp_solver
    counts, refined_of, (min_in, max_its), step = CASES[case]
    N = 50
    idx = np.arange(N)[::-1] * 2                          # mvKeyPointIndices: point i came from entry 2 (N - 1 - i) of 2 N matches
    rng = np.random.RandomState(1)
    s = pnp_solver.PnPsolver(np.zeros((N, 3)), np.zeros((N, 2)), np.ones(N), R.K_DEFAULT, indices=idx, n_matches=2 * N,
                             randint=lambda lo, hi: rng.randint(lo, hi + 1), evaluate=_fake_eval(counts, refined_of, N))
    s.set_ransac_parameters(0.99, min_in, max_its, 4, 0.0)
    s.max_its = max_its                                   # (the formula's own count is checked in test_set_ransac_parameters)
    assert s.min_inliers == min_in
    q, calls, _ = _seq(counts, refined_of, N=N, min_inliers=min_in, max_its=max_its)
    q.indices, q.n_matches = idx, 2 * N
    seen = []
    for _ in range(6):
        T, no_more, inl, n = s.iterate(step)
        qT, q_no_more, q_inl, q_n = q.iterate(step)
        assert (T is None, no_more, n, s.iterations, s.best_inliers) == (qT is None, q_no_more, q_n, q.iterations, q.best_inliers)
        assert inl.tolist() == q_inl.tolist() and (T is None or T.tobytes() == qT.tobytes())
        assert len(s.result["count"]) <= max(max_its, q.iterations - 1 + step)        # never more drawn than the call could have run
        seen.append((None if T is None else float(T[0, 0]), no_more, n))
    assert len(s.samples) == len(s.result["count"]) and all(len(set(x)) == 4 for x in s.samples.tolist())
    if case == "accepts":
        assert seen[:4] == [(-21.0, False, 22), (-21.0, False, 22), (-40.0, False, 41), (-40.0, False, 41)]
    if case == "never":
        assert seen[0] == (4.0, True, 25) and seen[1] == (4.0, True, 25)
    if case == "accept_after_the_maximum":
        assert seen[:3] == [(None, True, 0), (-26.0, False, 27), (-26.0, False, 27)]


def test_python_class_exits():
    from sivo_amd import pnp_solver
    s = pnp_solver.PnPsolver(np.zeros((9, 3)), np.zeros((9, 2)), np.ones(9), R.K_DEFAULT, evaluate=lambda p: 1 / 0)
    s.set_ransac_parameters(0.99, 10, 300, 4, 0.5)
    assert s.iterate(5)[:2] == (None, True) and s.iterations == 0 and s.result is None        # N < minInliers: nothing evaluated
    with pytest.raises(ValueError):
        s.set_ransac_parameters(0.99, 10, 300, 5, 0.5)
    for N in (15, 40, 400):
        s = pnp_solver.PnPsolver(np.zeros((N, 3)), np.zeros((N, 2)), np.full(N, 1.44), R.K_DEFAULT)
        s.set_ransac_parameters(0.99, 10, 300, 4, 0.5, 5.991)
        assert (s.min_inliers, s.max_its) == R.ransac_iterations(N, 0.99, 10, 300, 4, 0.5)[:2]
        assert s.points["max_err"][0] == np.float32(1.44) * np.float32(5.991)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement against a second opinion and the truth
# ---------------------------------------------------------------------------------------------------------------------
def lapack_epnp(P, K):
    """EPnP (Lepetit, Moreno-Noguer, Fua) on one set of correspondences P (n, 5) with numpy.linalg in float64: the structure of
    PnPsolver.cc, every cv* call by its LAPACK counterpart."""
    fu, fv, uc, vc = K
    pw, us = P[:, :3], P[:, 3:]
    n = len(P)
    c0 = pw.mean(axis=0)
    d = pw - c0
    _, dc, uct = np.linalg.svd(d.T @ d)
    cws = np.vstack([c0, c0 + np.sqrt(dc / n)[:, None] * uct])
    cc = (cws[1:] - cws[0]).T
    al = (np.linalg.inv(cc) @ d.T).T
    al = np.hstack([1 - al.sum(axis=1, keepdims=True), al])
    M = np.zeros((2 * n, 12))
    for j in range(4):
        M[0::2, 3 * j] = al[:, j] * fu
        M[0::2, 3 * j + 2] = al[:, j] * (uc - us[:, 0])
        M[1::2, 3 * j + 1] = al[:, j] * fv
        M[1::2, 3 * j + 2] = al[:, j] * (vc - us[:, 1])
    _, _, ut = np.linalg.svd(M.T @ M)
    v = ut[[11, 10, 9, 8]]
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    dv = np.array([[v[i, 3 * a:3 * a + 3] - v[i, 3 * b:3 * b + 3] for (a, b) in pairs] for i in range(4)])
    L = np.zeros((6, 10))
    for r in range(6):
        g = lambda i, j: dv[i, r] @ dv[j, r]
        L[r] = [g(0, 0), 2 * g(0, 1), g(1, 1), 2 * g(0, 2), 2 * g(1, 2), g(2, 2), 2 * g(0, 3), 2 * g(1, 3), 2 * g(2, 3), g(3, 3)]
    rho = np.array([np.sum((cws[a] - cws[b]) ** 2) for (a, b) in pairs])
    best = None
    for kind, cols in ((1, [0, 1, 3, 6]), (2, [0, 1, 2]), (3, [0, 1, 2, 3, 4])):
        b = np.linalg.lstsq(L[:, cols], rho, rcond=None)[0]
        be = np.zeros(4)
        s = -1.0 if b[0] < 0 else 1.0
        be[0] = np.sqrt(s * b[0])
        if kind == 1:
            be[1:] = s * b[1:] / be[0]
        else:
            be[1] = np.sqrt(s * b[2]) if s * b[2] > 0 else 0.0
            if b[1] < 0:
                be[0] = -be[0]
            if kind == 3:
                be[2] = b[3] / be[0]
        for _ in range(5):
            A = np.zeros((6, 4))
            A[:, 0] = 2 * L[:, 0] * be[0] + L[:, 1] * be[1] + L[:, 3] * be[2] + L[:, 6] * be[3]
            A[:, 1] = L[:, 1] * be[0] + 2 * L[:, 2] * be[1] + L[:, 4] * be[2] + L[:, 7] * be[3]
            A[:, 2] = L[:, 3] * be[0] + L[:, 4] * be[1] + 2 * L[:, 5] * be[2] + L[:, 8] * be[3]
            A[:, 3] = L[:, 6] * be[0] + L[:, 7] * be[1] + L[:, 8] * be[2] + 2 * L[:, 9] * be[3]
            bb = np.array([be[0] * be[0], be[0] * be[1], be[1] * be[1], be[0] * be[2], be[1] * be[2], be[2] * be[2], be[0] * be[3],
                           be[1] * be[3], be[2] * be[3], be[3] * be[3]])
            be = be + np.linalg.lstsq(A, rho - L @ bb, rcond=None)[0]
        ccs = (be[:, None] * v).sum(axis=0).reshape(4, 3)
        pcs = al @ ccs
        if pcs[0, 2] < 0:
            pcs = -pcs
        pc0, pw0 = pcs.mean(axis=0), pw.mean(axis=0)
        U, _, Vt = np.linalg.svd((pcs - pc0).T @ (pw - pw0))
        Rm = U @ Vt
        if np.linalg.det(Rm) < 0:
            Rm[2] = -Rm[2]
        t = pc0 - Rm @ pw0
        Pc = pw @ Rm.T + t
        err = np.mean(np.hypot(us[:, 0] - (uc + fu * Pc[:, 0] / Pc[:, 2]), us[:, 1] - (vc + fv * Pc[:, 1] / Pc[:, 2])))
        if best is None or err < best[0]:
            best = (err, Rm, t)
    return best[1], best[2]


def conditioning(P):
    d = P[:, :3] - P[:, :3].mean(axis=0)
    e = np.linalg.eigvalsh(d.T @ d)
    return e[0] / e[2]


@pytest.fixture(scope="module")
def noise_free():
    """6 seeds x 300 samples of noise-free scenes: the restatement's poses, computed once."""
    out = []
    for seed in SEEDS:
        sc = R.make_scene(seed, 60)
        S = R.draw_samples(np.random.RandomState(seed), 60, 300)
        P = R._points64(sc["pts"], S.astype(np.int64))
        Rr, tr = R.epnp(P, np.asarray(sc["K"], np.float32).astype(np.float64))
        out.append((sc, S, P, Rr, tr))
    return out


def sample_error(P, K, Rm, t):
    """The largest reprojection error (px) of a pose over its own sample, in float64."""
    Pc = P[:, :3] @ Rm.T + t
    return np.max(np.hypot(P[:, 3] - (K[2] + K[0] * Pc[:, 0] / Pc[:, 2]), P[:, 4] - (K[3] + K[1] * Pc[:, 1] / Pc[:, 2])))


def test_restatement_agrees_with_lapack_epnp_and_the_true_pose(noise_free):
    rows = []
    for sc, S, P, Rr, tr in noise_free:
        K = np.asarray(sc["K"], np.float32).astype(np.float64)
        for h in range(len(S)):
            Rl, tl = lapack_epnp(P[h], K)
            rows.append((conditioning(P[h]), np.max(np.abs(Rr[h] - Rl)), np.max(np.abs(tr[h] - tl)), np.max(np.abs(Rr[h] - sc["R"])),
                         np.max(np.abs(tr[h] - sc["t"])), sample_error(P[h], K, Rr[h], tr[h]), sample_error(P[h], K, Rl, tl)))
    a = np.array(rows)
    kept = a[:, 0] > COND_MIN
    conv_r, conv_l = a[:, 5] < CONV_PX, a[:, 6] < CONV_PX
    both = kept & conv_r & conv_l
    worst = lambda m, i: float(np.max(a[m][:, i]))
    print("kept", kept.mean(), "worst on kept", [worst(kept, i) for i in (1, 2, 3, 4)], "converged", conv_r.mean(), conv_l.mean(), both.mean(),
          "worst where both converged", [worst(both, i) for i in (1, 2)], "restatement converged, against the truth",
          [worst(kept & conv_r, i) for i in (3, 4)])
    assert len(a) == 1800 and not np.isnan(a).any()
    assert (~kept).mean() <= 0.2                          # at most 20 % of the all-inlier samples are excluded as ill-conditioned
    # the bound as defined from the worst deviation over the well-conditioned samples (see above: it cannot fail)
    assert worst(kept, 1) < EPNP_TOL["R"] and worst(kept, 2) < EPNP_TOL["t"]
    assert worst(kept, 3) < EPNP_TOL["R"] and worst(kept, 4) < EPNP_TOL["t"]
    # where both forms found the pose that reproduces the sample, it is the same pose, and the true one
    assert both.sum() >= 150
    assert worst(both, 1) < CONV_TOL["R"] and worst(both, 2) < CONV_TOL["t"]
    assert worst(kept & conv_r, 3) < TRUE_TOL["R"] and worst(kept & conv_r, 4) < TRUE_TOL["t"]
    # and the Jacobi basis suits the approximations as often as LAPACK's does
    assert conv_r.mean() >= conv_l.mean() - 0.05


def test_noise_free_scene_with_outliers_accepts_the_true_pose():
    sc = R.make_scene(21, 120, outliers=0.3)
    S = R.draw_samples(np.random.RandomState(21), 120, 60)
    m, its, _ = R.ransac_iterations(120, 0.99, 10, 300, 4, 0.5)
    res = R.pnp_ransac(sc["pts"], sc["K"], S, m)

    def ev(h):
        return int(res["count"][h]), res["T"][h], R.unpack_bits(res["inlier_bits"][h], 120)

    def refine(bits):
        c, T, b = R.evaluate(sc["pts"], sc["K"], np.flatnonzero(bits)[None, :])
        return int(c[0]), T[0], R.unpack_bits(b[0], 120)
    T, no_more, inl, n = R.Sequential(120, m, its, ev, refine).iterate(5)
    assert T is not None and not no_more and n > m
    assert np.max(np.abs(T[:3, :3] - sc["R"])) < TRUE_TOL["R"] and np.max(np.abs(T[:3, 3] - sc["t"])) < TRUE_TOL["t"]
    assert not (inl & ~sc["true_inlier"]).any() and n == inl.sum() == sc["true_inlier"].sum()
    # the records are the refinements the ABI hands out: the accepted one is among them
    rec = np.flatnonzero(res["refined"] >= 0)
    assert len(rec) >= 1 and any(R.Sequential._mat(res["refined_T"][h]).tobytes() == T.tobytes() for h in rec)


def test_degenerate_samples_count_nothing():
    sc = R.make_scene(41, 40, duplicates=3)
    with np.errstate(all="raise"):                        # (the restatement silences its own NaNs)
        c, T, _ = R.evaluate(sc["pts"], sc["K"], [[0, 1, 2, 3], [20, 21, 22, 23]])
    assert c[0] == 0 and np.isnan(T[0]).any() and c[1] == 40      # points 0 and 1 coincide


# ---------------------------------------------------------------------------------------------------------------------
# the kernel's arithmetic, compiled for the host
# ---------------------------------------------------------------------------------------------------------------------
def core_text(pts, K, sets):
    out = [str(len(pts)), " ".join(float(np.float32(v)).hex() for v in K)]
    out += [" ".join(float(v).hex() for v in (*p["xw"], p["u"], p["v"], p["max_err"])) for p in pts]
    out.append(str(len(sets)))
    out += [str(len(s)) + " " + " ".join(str(int(i)) for i in s) for s in sets]
    return "\n".join(out) + "\n"


def test_host_build_of_the_kernel_arithmetic_equals_the_restatement(tmp_path):
    """pnp_epnp.hpp with a team of one lane (g++, no contraction) against the restatement: samples of 4, refinement sets of other
    sizes, a duplicated and a coplanar scene (NaN poses)."""
    exe = host_prog.build("pnp_ransac_prog", tmp_path, link_lib=True)
    nans = 0
    for seed, n, kw in ((1, 70, dict(outliers=0.3)), (3, 40, dict(duplicates=5)), (4, 50, dict(coplanar=True))):
        sc = R.make_scene(seed, n, **kw)
        S = R.draw_samples(np.random.RandomState(seed), n, 40)
        res = R.pnp_ransac(sc["pts"], sc["K"], S, 8)
        rec = np.flatnonzero(res["refined"] >= 0)
        sets = [list(s) for s in S] + [list(np.flatnonzero(R.unpack_bits(res["inlier_bits"][h], n))) for h in rec]
        rows = [ln.split() for ln in host_prog.run_text(exe, ["core"], core_text(sc["pts"], sc["K"], sets), 120).strip().splitlines()]
        T = np.array([[float.fromhex(v) for v in w[1:13]] for w in rows])
        T = R.store_T(T[:, :9], T[:, 9:])
        want_T = np.concatenate([res["T"], res["refined_T"][rec]])
        assert [int(w[0]) for w in rows] == list(res["count"]) + list(res["refined"][rec])
        assert T.tobytes() == want_T.tobytes()
        assert [[int(v, 16) for v in w[13:]] for w in rows] == np.concatenate([res["inlier_bits"], res["refined_bits"][rec]]).tolist()
        nans += int(np.isnan(want_T).any(axis=1).sum())
        assert seed != 1 or len(rec) >= 1
    assert nans > 0


# ---------------------------------------------------------------------------------------------------------------------
# header, exports, argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    h = open(os.path.join(ROOT, "include", "sivo_hip.h")).read()
    assert "int sivo_pnp_ransac_batch(SivoPnpRansacProblem *problems, int n_problems);" in h
    assert "int sivo_pnp_ransac(SivoPnpRansacProblem *problem);" in h and "} SivoPnpPoint;" in h
    from sivo_amd import _lib, pnp_solver
    L = _lib.lib()
    assert hasattr(L, "sivo_pnp_ransac") and hasattr(L, "sivo_pnp_ransac_batch")
    assert pnp_solver.PNP_POINT_DTYPE.itemsize == R.PNP_POINT_DTYPE.itemsize == C.sizeof(_lib.PnpPoint) == 24


def test_ctypes_structs_match_the_header(tmp_path):
    from sivo_amd import _lib
    host_prog.c_layout(tmp_path, "SivoPnpPoint", _lib.PnpPoint)
    host_prog.c_layout(tmp_path, "SivoPnpRansacProblem", _lib.PnpRansacProblem)
    assert C.sizeof(_lib.PnpPoint) == 24


def test_entry_points_check_arguments_and_fail_loudly_without_a_device():
    from sivo_amd import _lib, pnp_solver
    sc = R.make_scene(5, 12)
    S = R.draw_samples(np.random.RandomState(5), 12, 4)
    args = (sc["pts"], sc["K"])
    # invalid arguments are reported as such before any device is needed
    for smp in ([[0, 1, 1, 2]], [[0, 1, 2, 3], [3, 4, 5, 3]], [[0, 1, 2, 12]], [[-1, 1, 2, 3]]):
        with pytest.raises(_lib.SivoInvalidArgument):
            pnp_solver.pnp_ransac(*args, smp)
    with pytest.raises(_lib.SivoInvalidArgument):
        pnp_solver.pnp_ransac(sc["pts"][:3], sc["K"], [[0, 1, 2, 0]])                        # n = 3
    with pytest.raises(_lib.SivoInvalidArgument):
        pnp_solver.pnp_ransac(*args, S, min_inliers=3)
    P = _lib.PnpRansacProblem()
    P.n, P.n_hyp = 5, 0                                                                      # a NULL array with a non-zero count
    assert _lib.lib().sivo_pnp_ransac(C.byref(P)) == _lib.ERR_INVALID_ARGUMENT
    assert _lib.lib().sivo_pnp_ransac(None) == _lib.ERR_INVALID_ARGUMENT
    # nothing to do: no launch, no device needed
    assert pnp_solver.pnp_ransac_batch([]) == []
    empty = pnp_solver.pnp_ransac(*args, np.zeros((0, 4), np.int32))
    assert empty["n_records"] == 0 and len(empty["count"]) == 0
    if _lib.lib().sivo_device_count() >= 1:            # (a device is visible: the call runs; tests/test_gpu_pnp_ransac.py checks what it computes)
        assert len(pnp_solver.pnp_ransac(*args, S)["count"]) == 4
        return
    with pytest.raises(_lib.SivoError) as e:
        pnp_solver.pnp_ransac(*args, S)
    assert e.value.code == _lib.ERR_RUNTIME
    with pytest.raises(_lib.SivoError) as e:
        pnp_solver.pnp_ransac_batch([{"points": sc["pts"], "K": sc["K"], "samples": S}])
    assert e.value.code == _lib.ERR_RUNTIME
    s = pnp_solver.PnPsolver(sc["pts"]["xw"], np.stack([sc["pts"]["u"], sc["pts"]["v"]], 1), np.ones(12), sc["K"])
    with pytest.raises(_lib.SivoError):
        s.find()


# ---------------------------------------------------------------------------------------------------------------------
# SIVO::PnPsolver
# ---------------------------------------------------------------------------------------------------------------------
STAND_INS = r'''#include "orbslam/PnPsolver.h"
struct MapPoint { cv::Mat GetWorldPos() const { return cv::Mat(3, 1, CV_32F); } bool isBad() const { return false; } };
struct Frame { float fx, fy, cx, cy; std::vector<cv::KeyPoint> mvKeysSemantic; std::vector<float> mvLevelSigma2;
               std::vector<MapPoint *> mvpMapPoints; };
using namespace SIVO;
using namespace std;
'''
SNIPPETS = {
    # Tracking.cc:1279-1283, :1298-1310
    "relocalization": r'''int f(Frame &mCurrentFrame, vector<vector<MapPoint *> > &vvpMapPointMatches, vector<PnPsolver *> &vpPnPsolvers, int i) {
    PnPsolver *pSolver = new PnPsolver(mCurrentFrame, vvpMapPointMatches[i]);
    pSolver->SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991);
    vpPnPsolvers[i] = pSolver;
    std::vector<bool> vbInliers;
    int nInliers;
    bool bNoMore;
    pSolver = vpPnPsolvers[i];
    cv::Mat Tcw = pSolver->iterate(5, bNoMore, vbInliers, nInliers);
    if (bNoMore) return -1;
    if (!Tcw.empty()) { const int np = vbInliers.size(); return np + nInliers; }
    Tcw = pSolver->find(vbInliers, nInliers);
    return 0;
}
''',
    "solve_all": r'''void g(vector<PnPsolver *> &vpPnPsolvers) {
    PnPsolver::SolveAll(vpPnPsolvers);
    vpPnPsolvers[0]->SetDraw([](int lo, int hi) { return (lo + hi) / 2; });
}
''',
}


@pytest.mark.parametrize("snippet", list(SNIPPETS))
def test_class_instantiates_over_stand_in_types(tmp_path, snippet):
    tu = tmp_path / "use.cpp"
    tu.write_text(STAND_INS + SNIPPETS[snippet])
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-I" + API, str(tu)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


def make_frame(seed, n, n_extra=10, outliers=0.2):
    """A frame whose matches hold the scene's n points among null and bad entries."""
    sc = R.make_scene(seed, n, outliers=outliers)
    rng = np.random.RandomState(seed + 100)
    m = n + n_extra
    slots = rng.permutation(m)
    sigma2 = (np.float32(1.2) ** (2 * np.arange(8))).astype(np.float32)
    keys = np.zeros((m, 3))
    keys[:, 0], keys[:, 1], keys[:, 2] = rng.uniform(0, 640, m), rng.uniform(0, 480, m), rng.randint(0, 8, m)
    matches = np.full(m, -1)
    points = np.zeros((n + n_extra // 2, 3), np.float32)
    bad = np.zeros(len(points), bool)
    points[:n] = sc["pts"]["xw"]
    for i in range(n):
        keys[slots[i], 0], keys[slots[i], 1] = sc["pts"]["u"][i], sc["pts"]["v"][i]
        matches[slots[i]] = i
    for j in range(n_extra // 2):                         # bad map points; the other extra entries stay null
        points[n + j] = rng.standard_normal(3)
        bad[n + j] = True
        matches[slots[n + j]] = n + j
    return {"keys": keys, "sigma2": sigma2, "matches": matches, "points": points, "bad": bad, "K": sc["K"]}


def frame_text(fr):
    out = [" ".join(float(np.float32(v)).hex() for v in fr["K"]) + f" {len(fr['keys'])} {len(fr['points'])}",
           " ".join(float(v).hex() for v in fr["sigma2"])]
    out += [f"{float(np.float32(k[0])).hex()} {float(np.float32(k[1])).hex()} {int(k[2])} {int(m)}" for k, m in zip(fr["keys"], fr["matches"])]
    out += [" ".join(float(v).hex() for v in p) + f" {int(b)}" for p, b in zip(fr["points"], fr["bad"])]
    return "\n".join(out) + "\n"


def test_gather_matches_the_reference_walk(tmp_path):
    fr = make_frame(8, 30)
    exe = host_prog.build("pnp_ransac_prog", tmp_path, link_lib=True)
    rows = [ln.split() for ln in host_prog.run_text(exe, ["gather"], "1\n" + frame_text(fr), 60).strip().splitlines()]
    pts, idx, _ = R.gather(fr)
    assert [int(w[1]) for w in rows] == list(idx) and len(idx) == 30 and len(fr["matches"]) == 40
    assert (fr["matches"] < 0).sum() == 5 and fr["bad"].sum() == 5           # null and bad entries among the matches
    got = np.array([[float.fromhex(v) for v in w[2:]] for w in rows], np.float32)
    want = np.concatenate([pts["xw"], pts["u"][:, None], pts["v"][:, None], pts["max_err"][:, None]], 1)
    assert got.tobytes() == want.tobytes()
    assert len(set(pts["max_err"].tolist())) > 3                              # octave-dependent thresholds
