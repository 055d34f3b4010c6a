"""PnPsolver's EPnP RANSAC and Sim3Solver's RANSAC pinned against the reference's OWN src/orbslam/PnPsolver.cc and Sim3Solver.cc.

oracle/Makefile compiles the two sources untouched, with their own headers (the classes keep the reference's members and layout),
over stand-ins for cv::Mat / the legacy C API / DUtils::Random (oracle/ref_shims_solvers) and links them with two drivers
(oracle/ref_pnp_driver.cpp, oracle/ref_sim3_driver.cpp) into oracle/_ref/.  The kernels, their host build, the numpy restatements
and the Python / C++ classes were written from one reading of those sources and are tested against each other bit for bit; this
file holds all of them against what the sources themselves compute:
  * primitives: the OpenCV routines under the sources are not available; oracle/cv_primitives.cpp states the substitutions DESIGN.md
    3.6c / 3.6d name a third time, and is compared byte for byte with the restatements' and within a measured bound with numpy.linalg;
  * arithmetic: compute_pose + CheckInliers / ComputeSim3 + CheckInliers on every hypothesis (and every refinement set) of every scene
    of tests/test_gpu_pnp_ransac.py and tests/test_gpu_sim3_ransac.py;
  * semantics: iterate / find call by call under scripted draws, SetRansacParameters over a grid;
  * gather: what the constructors keep.
Pinned by this: everything the two sources do around the OpenCV primitives, and the sequential semantics.  Still substitutions: the
primitives themselves (cvSVD, cvSolve, cvInvert, cvMulTransposed, cv::eigen, atan2 + cv::Rodrigues).
Where the reference is absent the same assertions read tests/golden/*_solver_reference.npz (tests/golden/make_solver_reference.py
wrote them from the live run); the tests marked gpu hold the device and the C++ classes against the same facts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import host_prog
import pnp_ransac_restatement as RP
import sim3_ransac_restatement as RS
import solver_pin_cases as S
import test_pnp_ransac_host as HP
import test_gpu_pnp_ransac as GP
import test_gpu_sim3_ransac as GS

D = C.POINTER(C.c_double)
F = C.POINTER(C.c_float)


# ---------------------------------------------------------------------------------------------------------------------
# the live comparison runs where the reference is; the fixtures are what it computes
# ---------------------------------------------------------------------------------------------------------------------
def test_with_the_reference_present_the_live_comparison_runs():
    for which in ("pnp", "sim3"):
        entries, live = S.reference_entries(which)
        assert live or not S.reference_present(), "the reference is here: the live comparison must run"
        assert len(entries) == len(S.load_fixture(which))


def test_fixtures_are_what_the_reference_computes(tmp_path):
    """The committed fixtures, byte for byte, from a fresh run of the reference programs; and what they cover."""
    for which, scenes, cases in (("pnp", len(GP.SCENES), S.PNP_RUN_CASES), ("sim3", 2 * len(GS.SCENES), S.SIM3_RUN_CASES)):
        names = sorted(S.load_fixture(which))
        assert sum(n.startswith("core.") for n in names) == scenes and [n for n in names if n.startswith("run.")] == sorted("run." + c for c in cases)
        assert "gather" in names and "params" in names
    assert sum(os.path.getsize(p) for p in S.GOLDEN.values()) < 160 * 1024
    if S.reference_program("ref_pnp") and S.reference_program("ref_sim3"):
        import importlib.util
        spec = importlib.util.spec_from_file_location("make_solver_reference", os.path.join(ROOT, "tests", "golden", "make_solver_reference.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        for which, path in mod.write(str(tmp_path)).items():
            assert open(path, "rb").read() == open(S.GOLDEN[which], "rb").read(), which


# ---------------------------------------------------------------------------------------------------------------------
# primitives
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prim():
    path = os.path.join(ROOT, "oracle", "libcvprim.so")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "libcvprim.so"], check=True)
    return C.CDLL(path)


def dp(a):
    return a.ctypes.data_as(D)


def symmetric_inputs(m):
    """random symmetric matrices and the shapes a Jacobi can get wrong: an exactly zero off-diagonal entry, a repeated eigenvalue, a
    zero row and column, and (m = 12) M'M of an 8 x 12 M, rank 8"""
    rng = np.random.RandomState(100 + m)
    out = []
    for _ in range(6):
        B = rng.standard_normal((m, m))
        out.append(B + B.T)
    Z = out[0].copy(); Z[0, 1] = Z[1, 0] = 0.0; Z[m - 2, m - 1] = Z[m - 1, m - 2] = 0.0
    v = rng.standard_normal(m)
    rep = 2.0 * np.eye(m) + np.outer(v, v)                     # eigenvalue 2, m - 1 times
    zc = out[1].copy(); zc[:, 2] = 0.0; zc[2, :] = 0.0
    out += [Z, rep, np.diag(np.arange(1.0, m + 1)), zc]
    if m == 12:
        M = rng.standard_normal((8, 12))
        out.append(M.T @ M)
    return [np.ascontiguousarray(A) for A in out]


def sweeps_of(prim):
    s = (C.c_int * 4)()
    prim.cvp_sweeps(s)
    return tuple(s)


def test_primitives_use_the_sources_sweep_counts(prim):
    assert sweeps_of(prim) == HP.source_constants() + (RS.SWEEPS,) == (RP.SWEEPS3, RP.SWEEPS12, RP.SWEEPS_SVD, RS.SWEEPS)


# eigenvalues / singular values of the primitives against numpy.linalg, relative to the largest, measured on the inputs of this file on
# the CPU (the worst value seen is in the comment); asserted at ten times that, for compiler and libm differences between machines
LINALG_TOL = {
    3: 10 * 9.4e-16,         # cvSVD of a symmetric 3 x 3, 4 sweeps: measured 9.36e-16
    12: 10 * 1.2e-15,        # cvSVD of a symmetric 12 x 12, 8 sweeps: measured 1.11e-15
    "svd3": 10 * 4.5e-16,    # cvSVD of a general 3 x 3, 3 one-sided sweeps: measured 4.48e-16
    4: 10 * 5.2e-8,          # cv::eigen of a 4 x 4, eigenvalues rounded to float: measured 5.18e-8 (half a float ulp of the largest is up to 6e-8)
}


def _relative(got, want):
    return float(np.max(np.abs(np.asarray(got, np.float64) - want)) / np.max(np.abs(want)))


@pytest.mark.parametrize("m", [3, 12])
def test_symmetric_svd_equals_the_restatements_jacobi_and_order(prim, m):
    sweeps = sweeps_of(prim)[0 if m == 3 else 1]
    worst = 0.0
    for A0 in symmetric_inputs(m):
        A, V = A0.copy(), np.eye(m)
        prim.cvp_jacobi(dp(A), dp(V), m, sweeps)
        rA, rV = A0.copy()[None], np.eye(m)[None].copy()
        with np.errstate(all="ignore"):
            RP._jacobi(rA, rV, sweeps)
        assert A.tobytes() == rA[0].tobytes() and V.tobytes() == rV[0].tobytes()
        dg = np.ascontiguousarray(np.diag(rA[0]))
        order = (C.c_int * m)()
        prim.cvp_order(dp(dg), m, order)
        want_order = RP._order(dg[None])[0]
        assert list(order) == list(want_order)
        A, W, Ut = A0.copy(), np.zeros(m), np.zeros((m, m))
        prim.cvp_svd_symmetric(dp(A), m, dp(W), dp(Ut))
        assert W.tobytes() == dg[want_order].tobytes() and Ut.tobytes() == np.ascontiguousarray(rV[0][:, want_order].T).tobytes()
        ev = np.linalg.eigvalsh(A0)
        worst = max(worst, _relative(W, ev[np.argsort(-np.abs(ev), kind="stable")]))
        assert np.max(np.abs(Ut.T * W @ Ut - A0)) < 1e-12 * max(1.0, np.max(np.abs(A0)))     # and it IS a decomposition of A
    print("symmetric", m, "worst relative eigenvalue difference to numpy.linalg", worst)
    assert worst < LINALG_TOL[m]


def test_order_ties_and_nans_go_to_the_lower_index(prim):
    for d in ([3.0, -3.0, 1.0, 3.0], [np.nan, 1.0, 2.0], [1.0, np.nan, 1.0], [0.0, 0.0, 0.0], [-5.0, 4.0, 5.0, np.nan, 0.0]):
        d = np.array(d)
        order = (C.c_int * len(d))()
        prim.cvp_order(dp(d), len(d), order)
        assert list(order) == list(RP._order(d[None])[0]), d
    d = np.array([3.0, -3.0, 1.0, 3.0])
    order = (C.c_int * 4)()
    prim.cvp_order(dp(d), 4, order)
    assert list(order) == [0, 1, 3, 2]


def test_general_svd3_equals_the_restatements_rotation(prim):
    rng = np.random.RandomState(7)
    mats = [rng.standard_normal((3, 3)) for _ in range(8)]
    mats.append(np.outer(rng.standard_normal(3), rng.standard_normal(3)))          # rank 1: two singular values at rounding level
    Z = mats[0].copy(); Z[:, 1] = 0.0
    mats += [Z, np.diag([3.0, 2.0, 1.0]), -np.eye(3)]                                # a zero column; gamma exactly zero; det < 0
    worst, nans = 0.0, 0
    for A0 in mats:
        A, W, U, V = np.ascontiguousarray(A0).copy(), np.zeros(3), np.zeros((3, 3)), np.zeros((3, 3))
        prim.cvp_svd3(dp(A), dp(W), dp(U), dp(V))
        with np.errstate(all="ignore"):
            R = np.array([[U[i, 0] * V[j, 0] + U[i, 1] * V[j, 1] + U[i, 2] * V[j, 2] for j in range(3)] for i in range(3)])     # estimate_R_and_t's dot
            r = R.reshape(9)
            det = r[0] * r[4] * r[8] + r[1] * r[5] * r[6] + r[2] * r[3] * r[7] - r[2] * r[4] * r[6] - r[1] * r[3] * r[8] - r[0] * r[5] * r[7]
            if det < 0:
                R[2] = -R[2]
            want, _ = RP._rotation(np.ascontiguousarray(A0)[None].copy(), np.zeros((1, 3)), np.zeros((1, 3)), sweeps_of(prim)[2])
        assert S.canon64(R).tobytes() == S.canon64(want[0]).tobytes()
        if np.isnan(R).any():
            nans += 1
            continue
        worst = max(worst, _relative(np.sort(W)[::-1], np.linalg.svd(A0, compute_uv=False)))
        assert np.max(np.abs(U * W @ V.T - A0)) < 1e-12
        if W.min() > 1e-6 * W.max():                                                 # (the U columns of vanishing singular values are rounding noise over itself)
            assert abs(np.linalg.det(R) - 1.0) < 1e-12 and np.max(np.abs(R @ R.T - np.eye(3))) < 1e-12
    print("svd3 worst relative singular value difference to numpy.linalg", worst, "NaN cases", nans)
    assert nans >= 1 and worst < LINALG_TOL["svd3"]


@pytest.mark.parametrize("nc", [3, 4, 5])
def test_solve_equals_the_restatements_qr_solve(prim, nc):
    rng = np.random.RandomState(20 + nc)
    systems = [(rng.standard_normal((6, nc)), rng.standard_normal(6)) for _ in range(8)]
    Z = systems[0][0].copy(); Z[:, 1] = 0.0                                          # a zero column: the reference's scheme returns early
    Z2 = systems[1][0].copy(); Z2[:5, 0] = 0.0                                       # its scan misses the last row: early return although A[5, 0] != 0
    N = systems[2][0].copy(); N[0, 0] = -abs(N[0, 0])
    systems += [(Z, systems[0][1]), (Z2, systems[1][1]), (N, systems[2][1])]
    nans = 0
    for A, b in systems:
        A, b, x = np.ascontiguousarray(A), np.ascontiguousarray(b), np.zeros(nc)
        prim.cvp_solve(dp(A), 6, nc, dp(b), dp(x))
        with np.errstate(all="ignore"):
            want = RP._qr_solve(A[None], b[None])[0]
        assert S.canon64(x).tobytes() == S.canon64(want).tobytes()
        if np.isnan(x).any():
            nans += 1
            assert np.isnan(x).all()
        else:
            assert np.allclose(x, np.linalg.lstsq(A, b, rcond=None)[0], rtol=0, atol=1e-9)     # full rank: the least-squares solution
    assert nans == 2


def test_mul_transposed_invert_and_the_quaternion_rotation(prim):
    rng = np.random.RandomState(3)
    M = np.ascontiguousarray(rng.standard_normal((8, 12)))
    out = np.zeros((12, 12))
    prim.cvp_mul_transposed(dp(M), 8, 12, dp(out))
    want = np.zeros((12, 12))
    for i in range(8):                                                               # the rows in order
        want = want + M[i][:, None] * M[i][None, :]
    assert out.tobytes() == want.tobytes()
    for _ in range(5):
        A, inv = np.ascontiguousarray(rng.standard_normal((3, 3))), np.zeros((3, 3))
        prim.cvp_invert3(dp(A), dp(inv))
        assert np.max(np.abs(inv @ A - np.eye(3))) < 1e-11
    sing, inv = np.ones((3, 3)), np.zeros((3, 3))
    prim.cvp_invert3(dp(sing), dp(inv))
    assert not np.isfinite(inv).any()                                                # det == 0: inf / NaN, as adjugate / determinant gives
    for q in (rng.standard_normal(4), [2.0, 0.0, 0.0, 0.0], [0.0, 0.0, 3.0, 0.0]):
        q, Rm = np.array(q, np.float32), np.zeros(9, np.float32)
        prim.cvp_quaternion_rotation(q.ctypes.data_as(F), Rm.ctypes.data_as(F))
        if not q[1:].any():
            assert np.isnan(Rm).all()                                                # no imaginary part: the reference's axis is 0 / 0
            continue
        w, x, y, z = q.astype(np.float64) / np.linalg.norm(q.astype(np.float64))
        want = np.array([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                         2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)])
        assert np.max(np.abs(Rm - want)) <= 2.0 ** -24                               # rounded once to float: half an ulp of 1


def test_eigen4_equals_the_restatements_jacobi(prim):
    worst = 0.0
    for A0 in symmetric_inputs(4):
        N = A0.astype(np.float32)
        N = np.ascontiguousarray((N + N.T) / np.float32(2))
        ev, evec = np.zeros(4, np.float32), np.zeros((4, 4), np.float32)
        prim.cvp_eigen4(N.ctypes.data_as(F), ev.ctypes.data_as(F), evec.ctypes.data_as(F))
        A, V = N.astype(np.float64)[None].copy(), np.eye(4)[None].copy()
        with np.errstate(all="ignore"):
            for _ in range(RS.SWEEPS):
                for p, q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
                    RS.jacobi_rot(A, V, p, q)
        best, e = A[0, 0, 0], V[0, :, 0]                                             # horn()'s choice: the largest, ties to the lower index
        for k in range(1, 4):
            if A[0, k, k] > best:
                best, e = A[0, k, k], V[0, :, k]
        assert evec[0].tobytes() == e.astype(np.float32).tobytes() and ev[0] == np.float32(best)
        worst = max(worst, _relative(ev, np.linalg.eigvalsh(N.astype(np.float64))[::-1]))
    print("eigen4 worst relative eigenvalue difference to numpy.linalg", worst)
    assert worst < LINALG_TOL[4]


# ---------------------------------------------------------------------------------------------------------------------
# arithmetic: every hypothesis and every refinement set of every scene
# ---------------------------------------------------------------------------------------------------------------------
def pnp_facts(name):
    return S.reference_entries("pnp")[0]["core." + name]


def sim3_facts(name, fix_scale):
    return S.reference_entries("sim3")[0][f"core.{name}.{'fix' if fix_scale else 'free'}"]


def restatement_doubles(sc):
    """mRi / mti of every hypothesis and of every record's refinement as the restatement holds them before the ABI narrows them"""
    n, want = len(sc["pts"]), sc["expect"]
    Kd = np.asarray(sc["K"], np.float32).astype(np.float64)
    both = []
    sets = [np.asarray(sc["samples"], np.int64)] + [np.flatnonzero(RP.unpack_bits(want["inlier_bits"][h], n))[None, :]
                                                    for h in np.flatnonzero(want["refined"] >= 0)]
    for s in sets:
        R, t = RP.epnp(RP._points64(sc["pts"], s), Kd)
        both.append(np.concatenate([R.reshape(-1, 9), t], 1))
    return both[0], np.concatenate(both[1:]) if len(both) > 1 else np.zeros((0, 12))


@pytest.mark.parametrize("name", list(GP.SCENES))
def test_pnp_restatement_equals_the_reference(name):
    """compute_pose + CheckInliers of PnPsolver.cc on every sample, Refine's on the inliers of every record: counts, the poses as the
    doubles mRi / mti hold and as the floats stored, the inlier words, of tests/pnp_ransac_restatement.py."""
    sc, facts = GP.scene(name), pnp_facts(name)
    S.check_pnp(facts, sc["expect"], sc, doubles=restatement_doubles(sc))
    # the reference's output shows what the scene's row of the table says (the comparison is not vacuous)
    count, refined, T = facts["counts"][:, 0], facts["counts"][:, 1], facts["T"]
    rec = np.flatnonzero(refined >= 0)
    assert len(count) == len(sc["samples"]) == SCENE_HYPOTHESES[name]                          # no hypothesis is left out
    if name == "minimum":
        assert count.tolist() == [4] and refined.tolist() == [4]
    elif name in ("all_outliers", "best_in_above"):
        assert len(rec) == 0
    elif name in ("duplicates", "coplanar"):
        nan = np.isnan(T).any(axis=1)
        assert nan.any() and not nan.all() and (count[nan] == 0).all()
    elif name == "outliers30":
        assert len(rec) >= 2
    else:
        assert len(rec) >= 1 and len(set(count.tolist())) >= 3


SCENE_HYPOTHESES = {name: row[1] for name, row in GP.SCENES.items()}


@pytest.fixture(scope="module")
def pnp_prog(tmp_path_factory):
    return host_prog.build("pnp_ransac_prog", tmp_path_factory.mktemp("pnp_prog"), link_lib=True)


@pytest.mark.parametrize("name", list(GP.SCENES))
def test_pnp_host_build_of_the_kernel_arithmetic_equals_the_reference(name, pnp_prog):
    """sivo_amd/csrc/pnp_epnp.hpp compiled for the host (tests/pnp_ransac_prog.cpp core64) on the same sets: counts, the poses as
    doubles and as the stored floats, words."""
    sc = GP.scene(name)

    def run(sets):
        return host_prog.run_text(pnp_prog, ["core64"], HP.core_text(sc["pts"], sc["K"], sets), 120)
    got = S.pnp_core(sc, run)
    count, refined = got["counts"][:, 0], got["counts"][:, 1]
    rec = np.flatnonzero(refined >= 0)
    W = got["all_words"]
    rT, rW = np.zeros((len(count), 12), np.float32), np.zeros((len(count), W.shape[1]), np.uint64)
    rT[rec], rW[rec] = got["refined_T"], W[len(count):]
    S.check_pnp(pnp_facts(name), {"count": count, "refined": refined, "T": got["T"], "refined_T": rT, "inlier_bits": W[:len(count)], "refined_bits": rW}, sc,
                doubles=(got["Rt"], got["refined_Rt"]))


@pytest.mark.parametrize("fix_scale", [True, False])
@pytest.mark.parametrize("name", list(GS.SCENES))
def test_sim3_restatement_equals_the_reference(name, fix_scale):
    """ComputeSim3 + CheckInliers of Sim3Solver.cc on every triple: counts, mR12i / mt12i / ms12i, mT12i and mT21i, the inlier words, of
    tests/sim3_ransac_restatement.py."""
    sc, facts = GS.scene(name, fix_scale), sim3_facts(name, fix_scale)
    tri = np.asarray(sc["triples"], np.int64)
    hyp = RS.horn(sc["pairs"]["x1c"][tri].transpose(0, 2, 1), sc["pairs"]["x2c"][tri].transpose(0, 2, 1), fix_scale)
    rows = lambda sR, t: np.concatenate([sR.reshape(-1, 3, 3), t[:, :, None]], 2).reshape(-1, 12)
    S.check_sim3(facts, sc["expect"], sc, t12_t21=(rows(hyp["sR"], hyp["t"]), rows(hyp["sRinv"], hyp["tinv"])))
    count = facts["counts"]
    assert len(count) == len(sc["triples"]) == (1 if name == "minimum" else 300)               # no hypothesis is left out
    first, _ = S.sim3_scans(count, sc["min_inliers"])
    if name == "all_outliers":
        assert first == -1
    elif name == "duplicates":
        assert 0 < len(facts["nan_rows"]) < len(count) and (count[facts["nan_rows"]] == 0).all()
    elif name not in ("minimum", "min_inliers_is_n"):
        assert first >= 0 and len(set(count.tolist())) > 5


# ---------------------------------------------------------------------------------------------------------------------
# semantics: iterate / find call by call
# ---------------------------------------------------------------------------------------------------------------------
def reference_transcript(which, case):
    return S.parse_transcript(S.text_of(S.reference_entries(which)[0]["run." + case]["transcript"]))


def calls_of(t, i=None):
    return [x for x in t if x[0] == "call" and (i is None or x[1] == i)]


@pytest.mark.parametrize("name", S.PNP_RUN_CASES)
def test_pnp_iterate_follows_the_reference_call_by_call(name):
    """PnPsolver::iterate / find of the reference under scripted draws against tests/pnp_ransac_restatement.py Sequential (each
    sample drawn when its iteration runs) and sivo_amd.pnp_solver.PnPsolver (all samples drawn at the first evaluation), both over
    the restatement's arithmetic: bNoMore, nInliers, the matrix bytes, vbInliers, mRansacMaxIts and mRansacMinInliers of every call."""
    case, ref = S.pnp_run_case(name), reference_transcript("pnp", name)
    lazy, traces, solvers = S.pnp_python_run(case)
    assert lazy == ref
    tr, s = traces[0], solvers[0]
    if name == "shared":
        # the documented deviation: several solvers on ONE stream.  The reference consumes it in the order the iterations run
        # (Sequential above, drawing lazily, follows it); the classes draw a solver's mRansacMaxIts samples at its first evaluation,
        # so the second solver sees other draws.  With a list per solver (every other case) the samples are the same.
        _, eager_traces, eager_solvers = S.pnp_python_run(case, eager=True)
        assert [int(v) for v in eager_traces[0]["samples"][0]] == tr["samples"][0]            # the first solver's first sample is the stream's first
        assert len(eager_traces[0]["samples"]) == eager_solvers[0].max_its > len(tr["samples"])
        assert [int(v) for v in eager_traces[1]["samples"][0]] != traces[1]["samples"][0]
        return
    eager, _, _ = S.pnp_python_run(case, eager=True)
    assert eager == ref
    if name == "accept_first":       # acceptance at the first qualifying iteration: no earlier count reached minInliers, the call returned there
        assert all(c < s.min_inliers for c in tr["counts"][:-1]) and tr["counts"][-1] >= s.min_inliers
        assert len(tr["refines"]) == 1 and tr["refines"][0][1] > s.min_inliers and s.iterations == len(tr["counts"]) < s.max_its
        assert calls_of(ref) == [("call", 0, 0, tr["refines"][0][1], 1, s.max_its, s.min_inliers)]
    elif name == "round_robin":
        assert [c[2] for c in calls_of(ref, 1)] == [1] and len(traces[1]["counts"]) == 5 and solvers[1].max_its == 3     # the loop is an OR
        assert sum(c[4] for c in calls_of(ref, 0)) >= 2 and sum(c[4] for c in calls_of(ref, 2)) >= 2
        assert traces[2]["refines"][0][0] < traces[2]["refines"][1][0]                         # a second record: Refine on another set
    elif name == "equal_min":
        m = s.min_inliers
        assert m == 18 and tr["counts"].count(m) >= 2 and max(tr["counts"]) == m               # a count equal to minInliers refines ...
        assert tr["refines"] == [(m, m)] * tr["counts"].count(m)                               # ... a non-record count re-uses the unchanged best ...
        assert calls_of(ref) == [("call", 0, 1, m, 1, s.max_its, m)] and len(tr["counts"]) == s.max_its    # ... an equal refined count is not accepted
    elif name == "too_few":
        assert calls_of(ref) == [("call", 0, 1, 0, 0, 1, 10)] and tr["counts"] == []           # N < minInliers
    elif name == "find":
        assert [c[1:5] for c in calls_of(ref)] == [(0, 1, tr["refines"][0][1], 1), (1, 1, 0, 0)] and len(traces[1]["counts"]) == 7
    elif name == "past_max":         # three calls on a solver of 3 iterations: 5 each (the loop is an OR), every one says bNoMore
        assert [c[2:5] for c in calls_of(ref)] == [(1, 0, 0)] * 3 and len(tr["counts"]) == 15 and s.max_its == 3


@pytest.mark.parametrize("name", S.SIM3_RUN_CASES)
def test_sim3_iterate_follows_the_reference_call_by_call(name):
    """Sim3Solver::iterate / find of the reference under scripted draws against tests/sim3_ransac_restatement.py Sequential (each
    triple drawn when its iteration runs) and sivo_amd.sim3_solver.Sim3Solver (all triples drawn at the first call), both over the
    restatement's arithmetic: bNoMore, nInliers, T12, GetEstimatedRotation / Translation / Scale, vbInliers, mRansacMaxIts of every call."""
    case, ref = S.sim3_run_case(name), reference_transcript("sim3", name)
    lazy, solvers = S.sim3_python_run(case)
    assert lazy == ref
    s = solvers[0]
    assert all(x.seq.N >= 3 for x in solvers)              # (a solver of fewer than 3 pairs is never handed to the reference: below)
    if name == "shared":
        _, eager = S.sim3_python_run(case, eager=True)     # the documented deviation, as for PnP
        assert eager[0].triples[0].tolist() == s.triples[0] and len(eager[0].triples) == eager[0].max_its > len(s.triples)
        assert eager[1].triples[0].tolist() != solvers[1].triples[0]
        return
    eager, _ = S.sim3_python_run(case, eager=True)
    assert eager == ref
    if name == "round_robin":
        accepted = [c[3] for c in calls_of(ref, 1) if c[4]]
        assert len(accepted) >= 2 and len(set(accepted)) == 1          # mnBestInliers under >=: an equal count is accepted again
        first = next(h for h, c in enumerate(solvers[0].counts) if c > 20)
        assert calls_of(ref, 0)[0][2:5] == (0, solvers[0].counts[first], 1) and all(c <= 20 for c in solvers[0].counts[:first])    # the first count above minInliers
        assert len(solvers[2].counts) == 23 and [c[2] for c in calls_of(ref, 2)] == [0, 0, 0, 0, 1]    # no acceptance until the maximum
    elif name == "equal_min":
        assert 140 in s.counts and max(s.counts) == 140 and not any(c[4] for c in calls_of(ref))       # strictly more than minInliers
        assert s.seq.best_inliers == 140 and s.seq.best == max(h for h, c in enumerate(s.counts) if c == 140)   # the later of equal bests
    elif name == "too_few":
        assert calls_of(ref) == [("call", 0, 1, 0, 0, 1)] and s.counts == []
    elif name == "find":
        assert [c[2:5] for c in calls_of(ref)] == [(1, s.counts[-1], 1), (1, 0, 0)] and len(solvers[1].counts) == 9
    elif name == "stops":            # seven calls on a solver of 23 iterations: 5 5 5 5 3 0 0 (the loop is an AND)
        assert len(s.counts) == 23 and [c[2] for c in calls_of(ref)] == [0, 0, 0, 0, 1, 1, 1]


def test_sim3_with_fewer_than_three_pairs_says_no_more():
    """The other documented deviation: the reference requires only N >= minInliers and would index an empty vector when it samples
    three of two pairs, so such a solver is not run on it; the classes say bNoMore."""
    from sivo_amd import sim3_solver
    sc = RS.make_scene(3, 11, n_hyp=1)
    s = sim3_solver.Sim3Solver(sc["pairs"][:2], sc["k1"], sc["k2"], True, randint=S.replay([0] * 9))
    s.set_ransac_parameters(0.99, 2, 300)
    T, no_more, inl, n = s.iterate(5)
    assert (T, no_more, n, s.iterations, len(inl)) == (None, True, 0, 0, 2)


def test_set_ransac_parameters_over_a_grid():
    """mRansacMinInliers / mRansacMaxIts / mRansacEpsilon of the reference after SetRansacParameters over (N, probability, minInliers,
    maxIterations, minSet, epsilon): minInliers == N, epsilon raised to minInliers / N, minSet above minInliers, N below minInliers."""
    from sivo_amd import pnp_solver, sim3_solver
    p = S.reference_entries("pnp")[0]["params"]
    assert p["grid"].tobytes() == S.sha(np.array(S.PNP_GRID, np.float64)).tobytes() and len(p["values"]) == len(S.PNP_GRID)
    seen = set()
    for (N, prob, m, its, ms, eps), (ref_min, ref_its, ref_eps) in zip(S.PNP_GRID, p["values"]):
        n_min, max_its, e = RP.ransac_iterations(N, prob, m, its, ms, eps)
        assert (n_min, max_its, np.float32(e).tobytes()) == (int(ref_min), int(ref_its), np.float32(ref_eps).tobytes()), (N, prob, m, its, ms, eps)
        if ms == 4:
            s = pnp_solver.PnPsolver(np.zeros((N, 3)), np.zeros((N, 2)), np.ones(N), RP.K_DEFAULT)
            s.set_ransac_parameters(prob, m, its, ms, eps)
            assert (s.min_inliers, s.max_its, np.float32(s.epsilon).tobytes()) == (int(ref_min), int(ref_its), np.float32(ref_eps).tobytes())
        seen |= {"min==N"} if n_min == N else set()
        seen |= {"eps raised"} if np.float32(e) > np.float32(eps) else set()
        seen |= {"minSet above"} if ms > max(m, int(N * eps)) else set()
        seen |= {"N below"} if N < n_min else set()
        seen |= {"formula"} if 1 < max_its < its else set()
    assert seen == {"min==N", "eps raised", "minSet above", "N below", "formula"}
    q = S.reference_entries("sim3")[0]["params"]
    assert q["grid"].tobytes() == S.sha(np.array(S.SIM3_GRID, np.float64)).tobytes() and len(q["values"]) == len(S.SIM3_GRID)
    sc = RS.make_scene(3, 11, n_hyp=1)
    for (N, prob, m, its), ref_its in zip(S.SIM3_GRID, q["values"]):
        assert RS.ransac_iterations(prob, m, its, N) == int(ref_its), (N, prob, m, its)
        s = sim3_solver.Sim3Solver(np.zeros(N, RS.PAIR_DTYPE), sc["k1"], sc["k2"])
        s.set_ransac_parameters(prob, m, its)
        assert s.max_its == int(ref_its)
    assert len({int(v) for v in q["values"]}) > 8


# ---------------------------------------------------------------------------------------------------------------------
# gather
# ---------------------------------------------------------------------------------------------------------------------
def test_pnp_constructor_gather_equals_the_reference():
    """mvKeyPointIndices, mvP3Dw, mvP2D, mvMaxError, mvSigma2 of the reference's constructor + SetRansacParameters(.., th2 = 5.991) over
    frames with null entries, bad map points and keys on several octaves."""
    g = S.reference_entries("pnp")[0]["gather"]
    frames = S.pnp_gather_frames()
    index, values = [], []
    for k, fr in enumerate(frames):
        pts, idx, sig2 = RP.gather(fr)
        index += [[k, i] for i in idx]
        values.append(np.concatenate([pts["xw"], pts["u"][:, None], pts["v"][:, None], pts["max_err"][:, None], sig2[:, None]], 1))
        assert (fr["matches"] < 0).any() and fr["bad"].any() and len(set(sig2.tolist())) > 3 and len(idx) < len(fr["matches"])
    assert np.array_equal(g["index"], np.array(index)) and g["values"].tobytes() == np.concatenate(values).astype(np.float32).tobytes()


def test_sim3_constructor_gather_equals_the_reference():
    """mvnIndices1, mvX3Dc1 / 2, mvnMaxError1 / 2, mvP1im1, mvP2im2 of the reference's constructor over keyframe pairs with null matches,
    bad points, no own point in KF1 and points missing in either keyframe (GetIndexInKeyFrame < 0)."""
    g = S.reference_entries("sim3")[0]["gather"]
    index, values = [], []
    for k, c in enumerate(S.sim3_gather_candidates()):
        idx, recs = RS.gather(c["kf1"], c["kf2"], c["matched12"], c["points"])
        sc = c["sc"]
        with np.errstate(all="ignore"):
            u1, v1 = RS.to_image(recs["x1c"][:, 0], recs["x1c"][:, 1], recs["x1c"][:, 2], np.asarray(sc["k1"], np.float32))
            u2, v2 = RS.to_image(recs["x2c"][:, 0], recs["x2c"][:, 1], recs["x2c"][:, 2], np.asarray(sc["k2"], np.float32))
        index += [[k, i] for i in idx]
        values.append(np.concatenate([recs["x1c"], recs["x2c"], recs["max_err1"][:, None], recs["max_err2"][:, None], np.stack([u1, v1, u2, v2], 1)], 1))
        pts = c["points"]
        assert len(idx) == len(sc["pairs"]) == len(c["matched12"]) - 18 and pts["bad"].any() and (c["matched12"] < 0).any() and (c["kf1"]["mp"] < 0).any()
        matched = c["matched12"][c["matched12"] >= 0]
        assert (pts["index_in_kf2"][matched] < 0).any() and len(set(recs["max_err1"].tolist())) > 3      # a point missing in the other keyframe
    assert np.array_equal(g["index"], np.array(index)) and g["values"].tobytes() == np.concatenate(values).astype(np.float32).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# the device and the C++ classes against the same facts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GP.SCENES))
def test_device_pnp_ransac_equals_the_reference(name):
    """sivo_pnp_ransac: count, T, inlier words, refined, the refined T and words of every hypothesis."""
    sc = GP.scene(name)
    S.check_pnp(pnp_facts(name), GP.run(sc), sc)


@pytest.mark.gpu
@pytest.mark.parametrize("fix_scale", [True, False])
@pytest.mark.parametrize("name", list(GS.SCENES))
def test_device_sim3_ransac_equals_the_reference(name, fix_scale):
    """sivo_sim3_ransac: count, T, inlier words, first_accept / best of every hypothesis."""
    sc = GS.scene(name, fix_scale)
    S.check_sim3(sim3_facts(name, fix_scale), GS.run(sc), sc)


@pytest.mark.gpu
def test_cpp_pnpsolver_reproduces_the_reference_transcripts(pnp_prog):
    """SIVO::PnPsolver over libsivo_hip.so (tests/pnp_ransac_prog.cpp run) on every case that program's protocol can express."""
    plain = [n for n in S.PNP_RUN_CASES if S.pnp_run_case(n).get("plain")]
    assert plain == ["round_robin", "accept_first", "equal_min", "too_few"]
    for name in plain:
        case = S.pnp_run_case(name)
        r = subprocess.run([pnp_prog, "run", str(case["max_calls"])], input=S.pnp_run_text(case), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (name, r.stderr)
        assert S.parse_transcript(r.stdout) == reference_transcript("pnp", name), name


@pytest.mark.gpu
def test_cpp_sim3solver_reproduces_the_reference_transcripts(tmp_path):
    """SIVO::Sim3Solver over libsivo_hip.so (tests/sim3_ransac_prog.cpp run) on every case that program's protocol can express."""
    exe = host_prog.build("sim3_ransac_prog", tmp_path, link_lib=True)
    plain = [n for n in S.SIM3_RUN_CASES if S.sim3_run_case(n).get("plain")]
    assert plain == ["round_robin", "equal_min", "too_few"]
    for name in plain:
        r = subprocess.run([exe, "run"], input=S.sim3_run_text(S.sim3_run_case(name)), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (name, r.stderr)
        assert S.parse_transcript(r.stdout) == reference_transcript("sim3", name), name
