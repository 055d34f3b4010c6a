"""sivo_sim3_optimize / sivo_sim3_optimize_batch (sivo_amd/csrc/sim3.hip) against the float64 restatement of
Optimizer::OptimizeSim3 (tests/sim3_restatement.py), and Optimizer::OptimizeSim3 over stand-in keyframes
(-DSIVO_SIM3_ON_DEVICE) against the Python binding."""
import numpy as np
import pytest

import host_prog
import sim3_restatement as R

pytestmark = pytest.mark.gpu

# S12 against the restatement: the per-edge arithmetic is the same operation for operation, the sums over the pairs and the 7 x 7
# solve are not (butterfly vs numpy order, Cholesky vs the restatement's) and sin / cos / exp are the device's: 1e-16 differences
# in the estimate move the delta = 1e-9 numeric Jacobians by ~1e-7 relative (OptimizeSim3), which the LM fixed point
# feels in proportion to the residuals.
S12_TOL = 1e-7

SCENES = {   # name -> make_scene arguments
    "inliers": dict(n=200, seed=101),
    "outliers20": dict(n=200, seed=202, outliers=0.2),
    "few_survivors": dict(n=15, seed=303, outliers=0.5),
    "one": dict(n=1, seed=404),
    "above_lds_cap": dict(n=2000, seed=505, outliers=0.1),
}


def scene(name, fix_scale):
    if name == "zero":
        sc = R.make_scene(12, 606, fix_scale=fix_scale)
        sc["matches"] = sc["matches"][:0]
        sc["expect"] = R.optimize_sim3(sc["s12"], sc["k1"], sc["k2"], sc["matches"], 10.0, fix_scale)
        return sc
    kw = dict(SCENES[name])
    n, seed = kw.pop("n"), kw.pop("seed")
    return R.make_scene(n, seed, scale=1.0 if fix_scale else 1.15, fix_scale=fix_scale, **kw)


def run(sc):
    from sivo_amd import optimizer
    return optimizer.sim3_optimize(sc["s12"], sc["k1"], sc["k2"], sc["matches"], sc["th2"], sc["fix_scale"])


def same_bits(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes()
               for k in ("s12", "outlier", "inliers", "chi2_12", "chi2_21", "iterations", "trials"))


@pytest.mark.parametrize("fix_scale", [True, False])
@pytest.mark.parametrize("name", list(SCENES) + ["zero"])
def test_sim3_matches_restatement(name, fix_scale):
    sc = scene(name, fix_scale)
    want = sc["expect"]
    got = run(sc)
    n = len(sc["matches"])
    assert np.array_equal(got["outlier"], want["outlier"])
    assert got["inliers"] == want["inliers"]
    assert (got["iterations"], got["trials"]) == (want["iterations"], want["trials"])
    if name in ("few_survivors", "one", "zero"):
        assert got["inliers"] == 0 and got["s12"].tobytes() == np.asarray(sc["s12"], np.float64).tobytes()
        assert name == "zero" or (got["iterations"] > 0 and got["trials"] > 0)
    else:
        assert got["inliers"] > 0
        d = got["s12"] - want["s12"]
        assert np.max(np.abs(d[:4])) <= S12_TOL and abs(d[7]) <= S12_TOL * want["s12"][7], d
        assert np.max(np.abs(d[4:7])) <= S12_TOL * max(1.0, np.max(np.abs(want["s12"][4:7]))), d
        assert np.max(np.abs(got["s12"] - sc["truth"])) < 0.05 * max(1.0, np.max(np.abs(sc["truth"])))
    if n:
        c = np.concatenate([got["chi2_12"], got["chi2_21"]])
        w = np.concatenate([want["chi2_12"], want["chi2_21"]])
        assert np.all(np.abs(c - w) <= 1e-5 * (1 + np.abs(w)))
    if name == "outliers20":
        assert want["iterations"] > 5                          # the optimize(10) branch ran


def test_sim3_is_deterministic():
    sc = scene("above_lds_cap", False)
    a, b = run(sc), run(sc)
    assert same_bits(a, b)


def test_sim3_batch_equals_single_calls():
    from sivo_amd import optimizer
    names = [("outliers20", True), ("one", False), ("above_lds_cap", True), ("zero", True), ("few_survivors", False), ("inliers", False)]
    scs = [scene(n, f) for n, f in names]
    singles = [run(sc) for sc in scs]
    batch = optimizer.sim3_optimize_batch([{k: sc[k] for k in ("s12", "k1", "k2", "matches", "th2", "fix_scale")} for sc in scs])
    for s, b in zip(singles, batch):
        assert same_bits(s, b)


@pytest.mark.parametrize("fix_scale", [True, False])
def test_cpp_member_equals_python_binding(tmp_path, fix_scale):
    from sivo_amd import optimizer
    sc = R.make_scene(150, 707, scale=1.0 if fix_scale else 1.1, outliers=0.15, fix_scale=fix_scale)
    kf1, kf2, pts, m1 = R.keyframe_pair(sc, 708, random_pose=False, n_extra=20)
    exe = host_prog.build("sim3_adapter_prog", tmp_path, link_lib=True, defines=("SIVO_SIM3_ON_DEVICE",))
    lines = host_prog.run_text(exe, ["run"], R.scene_text(sc, kf1, kf2, pts, m1), 120).strip().splitlines()
    n_in = int(lines[0])
    s12 = np.array([float.fromhex(v) for v in lines[1].split()])
    kept = np.array([int(v) for v in lines[2].split()])
    idx, recs = R.gather(kf1, kf2, m1, pts)
    py = optimizer.sim3_optimize(sc["s12"], sc["k1"], sc["k2"], recs, sc["th2"], fix_scale)
    assert n_in == py["inliers"] > 0
    assert s12.tobytes() == py["s12"].tobytes()
    want_kept = (m1 >= 0).astype(int)
    want_kept[idx[py["outlier"] != 0]] = 0
    assert np.array_equal(kept, want_kept)
