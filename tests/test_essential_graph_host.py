"""Optimizer::OptimizeEssentialGraph without a GPU: the restatement's self-checks (Sim3::log, the numeric Jacobian, convergence to
a known truth), the C ABI's presence, argument checks and loud failure without a device, the host ordering / symbolic factorisation,
the -DSIVO_ESSENTIAL_GRAPH_ON_DEVICE routing of the C++ member, and the gather and pose write-back against the restatement of
Optimizer.cc:964-1203 (bit-exact)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import essential_graph_restatement as E
import host_prog

API = os.path.join(ROOT, "sivo_amd", "api")
PROG = os.path.join(ROOT, "tests", "essential_graph_prog.cpp")


@pytest.mark.parametrize("sigma", [0.0, 0.3])
@pytest.mark.parametrize("mag", [1e-7, 0.4])
def test_log_inverts_exp_in_each_branch(sigma, mag):
    rng = np.random.default_rng(int(sigma * 10 + mag * 100))
    for _ in range(5):
        u = np.concatenate([rng.normal(size=3) * mag, rng.normal(size=3), [sigma * rng.uniform(0.5, 1.5)]])
        S = E.exp(u)
        # exp(log(S)) = S in all four branches (|sigma| < 1e-5 or not, d > 1 - 1e-5 or not)
        back = E.exp(E.sim3_log(S[None])[0])
        assert np.max(np.abs(back - S)) < 1e-12, (u, back, S)
        if mag > 1e-3:                    # log(exp(u)) = u away from the first-order rotation branch
            assert np.max(np.abs(E.sim3_log(S[None])[0] - u)) < 1e-12
    # the branch of d > 1 - 1e-5 with |sigma| > 1e-5 is reached (0.5 deltaR, the series A / B)
    S = E.exp([1e-4, 0, 0, 1.0, 2.0, 3.0, 0.2])
    R = E.quat_to_matrix(S[:4])
    assert 0.5 * (np.trace(R) - 1) > 1 - 1e-5


def test_numeric_jacobian_matches_a_wide_step_difference():
    # a map without scale drift: every residual's sigma is ~0, inside g2o's |sigma| < 1e-5 branch of Sim3::log.  (Just above 1e-5,
    # with a near-identity rotation, g2o's log has B = ((sigma^2/2 - sigma + 1) s) / sigma^3 without the series' "- 1": W is of order
    # 1 / sigma^3 there and no finite difference wider than that band means anything — restated as it is)
    m = E.make_map(40, 4, fix_scale=True)
    siw, fixed, vertex, e = E.gather(m)
    free = vertex & ~fixed
    ei, ej = e["i"].astype(np.int64), e["j"].astype(np.int64)
    Ji, Jj, _ = E.jacobians(siw, ei, ej, e["meas"], free, False)
    h = 1e-6
    for d in range(7):
        u = np.zeros(7)
        u[d] = h
        for side, J in ((0, Ji), (1, Jj)):
            ep, em = siw.copy(), siw.copy()
            for v in np.flatnonzero(free):
                ep[v] = E.mul(E.exp(u)[None], siw[v][None])[0]
                em[v] = E.mul(E.exp(-u)[None], siw[v][None])[0]
            # one side perturbed at a time
            if side == 0:
                ref = (E.sim3_log(E.mul(E.mul(e["meas"], ep[ei]), E.inv(siw[ej]))) -
                       E.sim3_log(E.mul(E.mul(e["meas"], em[ei]), E.inv(siw[ej])))) / (2 * h)
            else:
                ref = (E.sim3_log(E.mul(E.mul(e["meas"], siw[ei]), E.inv(ep[ej]))) -
                       E.sim3_log(E.mul(E.mul(e["meas"], siw[ei]), E.inv(em[ej])))) / (2 * h)
            mask = free[ei] if side == 0 else free[ej]
            # delta = 1e-9 differences: an ulp of an O(1) error is ~1e-7 in J; in the acos branch just above theta = 4.5e-3,
            # theta / (2 sqrt(1 - d^2)) carries ~5e-12 relative noise from 1 - d^2 ~ theta^2: ~1e-5 in J (g2o has it too)
            assert np.max(np.abs(J[mask, :, d] - ref[mask])) < 3e-5, (side, d)
    # under fix_scale the scale column is exactly zero (oplus zeroes update[6] of the perturbation)
    Ji, Jj, _ = E.jacobians(siw, ei, ej, e["meas"], free, True)
    assert not Ji[:, :, 6].any() and not Jj[:, :, 6].any()


@pytest.mark.parametrize("fix_scale", [True, False])
def test_restatement_converges_to_the_truth(fix_scale):
    truth, init, fixed, e = E.true_graph(30, 7, fix_scale)
    r = E.optimize(init, fixed, e, fix_scale)
    assert r["chi2_start"] > 1e-3 and r["chi2"] < 1e-20
    assert 1 <= r["iterations"] <= 20
    assert np.max(np.abs(r["siw"] - truth)) < 1e-9
    assert np.array_equal(r["siw"][0], init[0])          # the fixed vertex stays


def test_one_ulp_sensitivity():
    """The parity tolerance of tests/test_gpu_essential_graph.py: g2o's numeric Jacobian amplifies a one-ulp change of acos by
    1 / (2 delta) = 5e8, so the restatement with every acos result one ulp larger stops elsewhere near the optimum — by more than
    rounding, by less than the parity bounds."""
    from test_gpu_essential_graph import TOL_QS, TOL_T_REL
    m = E.make_map(30, 11, fix_scale=True)
    siw, fixed, vertex, e = E.gather(m)
    a = E.optimize(siw, fixed, e, True)
    try:
        E.ACOS_JITTER = 2.0 ** -52
        b = E.optimize(siw, fixed, e, True)
    finally:
        E.ACOS_JITTER = 0.0
    dq = np.max(np.abs(a["siw"][:, :4] - b["siw"][:, :4]))
    dt = np.max(np.abs(a["siw"][:, 4:7] - b["siw"][:, 4:7])) / np.max(np.abs(siw[:, 4:7]))
    assert 1e-9 < dq < TOL_QS / 10 and 1e-9 < dt < TOL_T_REL / 10


def test_header_declares_and_library_exports_the_entry_points():
    h = open(os.path.join(ROOT, "include", "sivo_hip.h")).read()
    assert re.search(r"int sivo_essential_graph_optimize\(double \*siw, const uint8_t \*fixed, int n, const SivoSim3Edge \*e", h)
    assert re.search(r"int sivo_sim3_correct_points\(const float \*xyz, const int32_t \*ref, int np", h)
    assert "SivoSim3Edge" in h and "Optimizer.cc:928" in h
    from sivo_amd import _lib
    from sivo_amd.optimizer import SIM3_EDGE_DTYPE
    L = _lib.lib()
    for name in ("sivo_essential_graph_optimize", "sivo_essential_graph_analyze", "sivo_sim3_correct_points"):
        assert hasattr(L, name)
    assert SIM3_EDGE_DTYPE.itemsize == C.sizeof(_lib.Sim3Edge) == 72


def _small_graph():
    truth, init, fixed, e = E.true_graph(12, 2, True)
    return init, fixed, e


def test_invalid_arguments_are_reported_before_any_device():
    from sivo_amd import _lib, optimizer
    siw, fixed, e = _small_graph()
    bad = e.copy()
    bad[3]["j"] = len(siw)
    with pytest.raises(_lib.SivoInvalidArgument):
        optimizer.essential_graph_optimize(siw, fixed, bad)
    bad = e.copy()
    bad[2]["j"] = bad[2]["i"]
    with pytest.raises(_lib.SivoInvalidArgument):
        optimizer.essential_graph_optimize(siw, fixed, bad)
    bad = e.copy()
    bad[1]["meas"][7] = 0.0
    with pytest.raises(_lib.SivoInvalidArgument):
        optimizer.essential_graph_optimize(siw, fixed, bad)
    s = siw.copy()
    s[4, 7] = -1.0
    with pytest.raises(_lib.SivoInvalidArgument):
        optimizer.essential_graph_optimize(s, fixed, e)
    L = _lib.lib()
    assert L.sivo_essential_graph_optimize(None, None, 3, None, 0, 1, 20, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert L.sivo_essential_graph_optimize(siw.ctypes.data, fixed.astype(np.uint8).ctypes.data, len(siw), None, 5, 1, 20, None, None,
                                           None) == _lib.ERR_INVALID_ARGUMENT
    xyz = np.zeros((4, 3), np.float32)
    with pytest.raises(_lib.SivoInvalidArgument):
        optimizer.sim3_correct_points(xyz, [0, 1, len(siw), -1], siw, siw)
    with pytest.raises(_lib.SivoInvalidArgument):
        optimizer.sim3_correct_points(xyz, [0, 1, -2, -1], siw, siw)
    assert L.sivo_sim3_correct_points(None, None, 4, siw.ctypes.data, siw.ctypes.data, len(siw), None) == _lib.ERR_INVALID_ARGUMENT


def test_entry_points_fail_loudly_without_a_device():
    from sivo_amd import _lib, optimizer
    siw, fixed, e = _small_graph()
    if _lib.lib().sivo_device_count() >= 1:       # (a device is visible: the call runs; tests/test_gpu_essential_graph.py checks it)
        assert optimizer.essential_graph_optimize(siw, fixed, e)["iterations"] >= 1
        return
    with pytest.raises(_lib.SivoError) as ex:
        optimizer.essential_graph_optimize(siw, fixed, e)
    assert ex.value.code == _lib.ERR_RUNTIME
    with pytest.raises(_lib.SivoError) as ex:
        optimizer.sim3_correct_points(np.zeros((2, 3), np.float32), [0, -1], siw, siw)
    assert ex.value.code == _lib.ERR_RUNTIME


def test_symbolic_factorisation_is_sparse_and_deterministic():
    from sivo_amd import optimizer
    m = E.make_map(300, 5, n_loops=3)
    siw, fixed, vertex, e = E.gather(m)
    a = optimizer.essential_graph_analyze(fixed, e)
    assert a == optimizer.essential_graph_analyze(fixed, e)
    assert a["variables"] == int((vertex & ~fixed).sum())
    na = a["variables"]
    dense_nnz = 7 * na * (7 * na + 1) // 2
    assert a["nnz_l"] < dense_nnz / 20                       # far from the dense 7N x 7N factor
    assert a["h_blocks"] <= a["l_blocks"] and 1 < a["levels"] < na
    # every vertex fixed: nothing to factor
    assert optimizer.essential_graph_analyze(np.ones(len(fixed), bool), e)["variables"] == 0


def test_optimize_essential_graph_member_instantiates_on_device(tmp_path):
    """-DSIVO_ESSENTIAL_GRAPH_ON_DEVICE routes Optimizer::OptimizeEssentialGraph to the device (no g2o): the member instantiates
    over the stand-ins of tests/essential_graph_prog.cpp, beside OptimizeSim3 under -DSIVO_SIM3_ON_DEVICE."""
    src = open(PROG).read()
    tu = tmp_path / "use.cpp"
    tu.write_text(src.split("static double rd()")[0] + r'''
void f(TMap *m, TKeyFrame *a, TKeyFrame *b, const std::map<TKeyFrame *, TSim3> &p, const std::map<TKeyFrame *, std::set<TKeyFrame *>> &c) {
    SIVO::Optimizer::OptimizeEssentialGraph(m, a, b, p, p, c, true);
}
''')
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-DSIVO_ESSENTIAL_GRAPH_ON_DEVICE", "-DSIVO_SIM3_ON_DEVICE",
                        "-I" + API, str(tu)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    # without the macro (and without g2o) the member is still a compile-time error that names it
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-I" + API, str(tu)], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "SIVO_ESSENTIAL_GRAPH_ON_DEVICE" in r.stderr


def _parse_gather(out):
    lines = out.strip().splitlines()
    n, ne = (int(v) for v in lines[0].split())
    V = [ln.split() for ln in lines[1:1 + n]]
    vertex = np.array([int(w[0]) for w in V], bool)
    fixed = np.array([int(w[1]) for w in V], bool)
    siw = np.array([[float.fromhex(v) for v in w[2:]] for w in V])
    Ed = [ln.split() for ln in lines[1 + n:1 + n + ne]]
    ij = np.array([[int(w[0]), int(w[1])] for w in Ed], np.int64).reshape(-1, 2)
    meas = np.array([[float.fromhex(v) for v in w[2:]] for w in Ed]).reshape(-1, 8)
    return siw, fixed, vertex, ij, meas


@pytest.mark.parametrize("n_kf,seed,fix_scale", [(30, 1, True), (150, 2, False)])
def test_gather_matches_the_reference_walk(tmp_path, n_kf, seed, fix_scale):
    m = E.make_map(n_kf, seed, fix_scale=fix_scale, n_points=20)
    exe = host_prog.build("essential_graph_prog", tmp_path)
    siw, fixed, vertex, ij, meas = _parse_gather(host_prog.run_text(exe, ["gather"], E.map_text(m), 60))
    want_siw, want_fixed, want_vertex, e = E.gather(m)
    assert np.array_equal(vertex, want_vertex) and np.array_equal(fixed, want_fixed)
    assert siw.tobytes() == want_siw.tobytes()
    assert ij.tolist() == np.stack([e["i"], e["j"]], 1).tolist()
    assert meas.tobytes() == np.ascontiguousarray(e["meas"]).tobytes()
    # the scene exercises every rule: a LoopConnections pair below 100 skipped, the (cur, loop) pair below 100 kept, a duplicated
    # vertex pair, a bad keyframe (no vertex, no edge), identity for the ids without a keyframe
    ids = m["ids"]
    cur, lp = ids[m["cur"]], ids[m["loop"]]
    pairs = [tuple(p) for p in ij.tolist()]
    assert (cur, lp) in pairs
    assert (ids[m["cur"] - 1], ids[m["loop"] + 2]) not in pairs
    keys = [(min(p), max(p)) for p in pairs]
    assert len(keys) > len(set(keys))
    bad = [ids[k] for k, kf in enumerate(m["kfs"]) if kf["bad"]]
    assert bad and not vertex[bad[0]] and all(bad[0] not in p for p in pairs)
    assert len(vertex) > len(ids) or not vertex.all()
    assert sum(1 for k in m["order"] if m["kfs"][k]["loop"]) >= 2


def test_pose_write_back_is_bit_exact(tmp_path):
    m = E.make_map(12, 3, n_points=0)
    rng = np.random.default_rng(5)
    S = np.stack([E.exp(np.concatenate([rng.normal(size=3), rng.normal(size=3) * 4, [rng.normal() * 0.3]])) for _ in range(20)])
    exe = host_prog.build("essential_graph_prog", tmp_path)
    text = E.map_text(m) + "\n".join(" ".join(repr(float(v)) for v in s) for s in S) + "\n"
    out = host_prog.run_text(exe, ["pose"], text, 60)
    got = np.array([[float.fromhex(v) for v in ln.split()] for ln in out.strip().splitlines()], np.float32)
    want = np.stack([E.pose_from_sim3(s)[:3].reshape(12) for s in S])
    assert got.tobytes() == want.tobytes()
