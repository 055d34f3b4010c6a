"""Optimizer::OptimizeEssentialGraph on the device (sivo_amd/csrc/essential_graph.hip) against the float64 restatement
(tests/essential_graph_restatement.py): parity on synthetic maps for both scale settings, convergence to a known truth, a 2000-keyframe
map (run-to-run bit identity, chi2 reduction, scipy.sparse parity), the edge cases, the point correction (bit-exact) and the C++ member
over the stand-in map against the Python binding (bit-exact)."""
import numpy as np
import pytest

import essential_graph_restatement as E
import host_prog

pytestmark = pytest.mark.gpu

# the two sides evaluate the same g2o arithmetic and differ only by the device's and the C library's acos / sin / cos /
# exp / log (an ulp now and then), the summation order of H and the factorisation.  g2o's numeric Jacobian (delta = 1e-9) turns one
# ulp of acos into ~1e-7 .. 1e-5 of J, and near the optimum that moves where Gauss-Newton stops: the restatement itself, with every
# acos result changed by one ulp, moves by 3e-8 .. 3.4e-7 in q and 7e-7 .. 7.4e-6 in t on these scenes (extent 10 .. 20), chi2 by up
# to 2.5e-5 relative (test_essential_graph_host.py::test_one_ulp_sensitivity).  The bounds are that noise floor with a margin.
TOL_QS = 2e-6
TOL_T_REL = 2e-6
TOL_CHI2_REL = 1e-4
# the 2000-keyframe map sits on a higher floor: one ulp of acos moves the restatement by 8.9e-6 in q and 4.2e-6 of the extent in t
# (and its iteration count from 9 to 20); chi2 by 1.2e-8 relative
TOL_LARGE = 5e-5


def _opt():
    from sivo_amd import optimizer
    return optimizer


def _compare(got, want, siw0, tol_qs=TOL_QS, tol_t=TOL_T_REL):
    extent = max(1.0, float(np.max(np.abs(siw0[:, 4:7]))))
    g, w = got["siw"], want["siw"]
    sign = np.where(np.sum(g[:, :4] * w[:, :4], 1) < 0, -1.0, 1.0)[:, None]
    assert np.max(np.abs(g[:, :4] - sign * w[:, :4])) < tol_qs
    assert np.max(np.abs(g[:, 7] - w[:, 7])) < tol_qs
    assert np.max(np.abs(g[:, 4:7] - w[:, 4:7])) < tol_t * extent
    assert abs(got["chi2"] - want["chi2"]) <= TOL_CHI2_REL * max(want["chi2"], 1e-12) + 1e-14
    assert got["chi2_start"] == pytest.approx(want["chi2_start"], rel=1e-12)
    assert 1 <= got["iterations"] <= 20 and 1 <= want["iterations"] <= 20


@pytest.mark.parametrize("fix_scale", [True, False])
@pytest.mark.parametrize("n_kf,seed", [(30, 11), (150, 12), (400, 13)])
def test_parity_with_the_restatement(n_kf, seed, fix_scale):
    m = E.make_map(n_kf, seed, fix_scale=fix_scale)
    siw, fixed, vertex, e = E.gather(m)
    got = _opt().essential_graph_optimize(siw, fixed, e, fix_scale=fix_scale)
    want = E.optimize(siw, fixed, e, fix_scale)
    _compare(got, want, siw)
    assert got["chi2"] < got["chi2_start"]
    # vertices without a keyframe (identity) and the fixed loop keyframe keep their estimates bit for bit
    keep = ~vertex | fixed
    assert got["siw"][keep].tobytes() == siw[keep].tobytes()


@pytest.mark.parametrize("fix_scale", [True, False])
def test_converges_to_the_truth(fix_scale):
    truth, init, fixed, e = E.true_graph(60, 17, fix_scale)
    got = _opt().essential_graph_optimize(init, fixed, e, fix_scale=fix_scale)
    assert got["chi2_start"] > 1e-3 and got["chi2"] < 1e-20
    assert np.max(np.abs(got["siw"] - truth)) < 1e-9


def test_large_map_bit_identical_and_parity():
    m = E.make_map(2000, 21, n_loops=3, covis=8, falloff=25, fix_scale=True)
    siw, fixed, vertex, e = E.gather(m)
    assert len(e) > 5 * 1900
    opt = _opt()
    a = opt.essential_graph_optimize(siw, fixed, e)
    b = opt.essential_graph_optimize(siw, fixed, e)
    assert a["siw"].tobytes() == b["siw"].tobytes() and a["chi2"] == b["chi2"] and a["trials"] == b["trials"]
    assert a["chi2"] < 0.05 * a["chi2_start"]
    pytest.importorskip("scipy.sparse")
    want = E.optimize(siw, fixed, e, True, sparse=True)
    _compare(a, want, siw, TOL_LARGE, TOL_LARGE)


def test_edge_cases():
    opt = _opt()
    truth, init, fixed, e = E.true_graph(20, 5, True)
    # no edges: nothing moves, no iteration
    r = opt.essential_graph_optimize(init, fixed, e[:0])
    assert r["siw"].tobytes() == init.tobytes() and r["iterations"] == 0 and r["trials"] == 0 and r["chi2"] == 0.0
    # every vertex fixed: g2o's optimize() has nothing to do; chi2 is that of the input
    r = opt.essential_graph_optimize(init, np.ones(20, bool), e)
    assert r["siw"].tobytes() == init.tobytes() and r["iterations"] == 0 and r["trials"] == 0
    assert r["chi2"] == r["chi2_start"] == pytest.approx(E.chi2(init, e["i"].astype(int), e["j"].astype(int), e["meas"]), rel=1e-12)
    # an isolated vertex keeps its estimate, the rest is solved as without it
    iso = np.concatenate([init, E.exp([0.1, 0.2, 0.3, 1, 2, 3, 0.1])[None]])
    r = opt.essential_graph_optimize(iso, np.r_[fixed, False], e)
    assert r["siw"][20].tobytes() == iso[20].tobytes()
    r0 = opt.essential_graph_optimize(init, fixed, e)
    assert r["siw"][:20].tobytes() == r0["siw"].tobytes()
    assert np.max(np.abs(r0["siw"] - truth)) < 1e-9


def test_point_correction_bit_exact():
    rng = np.random.default_rng(3)
    n = 40
    before = np.stack([E.exp(np.concatenate([rng.normal(size=3), rng.normal(size=3) * 5, [rng.normal() * 0.2]])) for _ in range(n)])
    after = np.stack([E.mul(E.exp(np.concatenate([rng.normal(size=3) * 0.05, rng.normal(size=3) * 0.3, [rng.normal() * 0.05]]))[None],
                            before[k][None])[0] for k in range(n)])
    xyz = (rng.normal(size=(5000, 3)) * 20).astype(np.float32)
    ref = rng.integers(-1, n, 5000)
    got = _opt().sim3_correct_points(xyz, ref, before, after)
    want = E.correct_points(xyz, ref, before, after)
    assert got.tobytes() == want.tobytes()
    assert got[ref < 0].tobytes() == xyz[ref < 0].tobytes()
    assert np.any(got[ref >= 0] != xyz[ref >= 0])


@pytest.mark.parametrize("fix_scale", [True, False])
def test_cpp_member_matches_the_binding(tmp_path, fix_scale):
    m = E.make_map(120, 31, fix_scale=fix_scale, n_points=300)
    exe = host_prog.build("essential_graph_prog", tmp_path, link_lib=True, defines=("SIVO_ESSENTIAL_GRAPH_ON_DEVICE",))
    lines = host_prog.run_text(exe, ["run"], E.map_text(m), 300).strip().splitlines()
    nk = len(m["kfs"])
    poses = np.array([[float.fromhex(v) for v in ln.split()] for ln in lines[:nk]], np.float32)
    pts = np.array([[float.fromhex(v) for v in ln.split()] for ln in lines[nk:]], np.float32)
    siw, fixed, vertex, e = E.gather(m)
    got = _opt().essential_graph_optimize(siw, fixed, e, fix_scale=fix_scale)
    for k, kf in enumerate(m["kfs"]):
        i = m["ids"][k]
        want = E.pose_from_sim3(got["siw"][i])[:3].reshape(12) if vertex[i] and not kf["bad"] else kf["Tcw"][:3].reshape(12)
        assert poses[k].tobytes() == np.asarray(want, np.float32).tobytes(), k
    xyz = np.array([p["pos"] for p in m["points"]], np.float32)
    ref = E.point_refs(m, vertex)
    want = _opt().sim3_correct_points(xyz, ref, siw, got["siw"])
    assert pts.tobytes() == want.tobytes()
    assert want.tobytes() == E.correct_points(xyz, ref, siw, got["siw"]).tobytes()
