"""sivo_sim3_ransac / sivo_sim3_ransac_batch (sivo_amd/csrc/sim3_ransac.hip) against the numpy restatement of Sim3Solver
(tests/sim3_ransac_restatement.py) BIT FOR BIT, and SIVO::Sim3Solver over stand-in keyframes against the Python class."""
import functools
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import host_prog
import sim3_ransac_restatement as R

pytestmark = pytest.mark.gpu

# the LDS cap of the kernel: the scene one pair above it takes the memory path for exactly one pair
CAP = int(re.search(r"RS_CAP = (\d+)", open(os.path.join(ROOT, "sivo_amd", "csrc", "sim3_ransac.hip")).read()).group(1))

SCENES = {   # name -> (make_scene arguments, min_inliers)
    "minimum": (dict(n=3, seed=11, n_hyp=1), 2),
    "min_inliers_is_n": (dict(n=20, seed=12, outliers=0.2), 20),
    "word_64": (dict(n=64, seed=13, outliers=0.25), 20),
    "word_65": (dict(n=65, seed=14, outliers=0.25), 20),
    "outliers30": (dict(n=200, seed=15, outliers=0.3, noise=0.0), 100),
    "outliers30_noisy": (dict(n=200, seed=20, outliers=0.3), 20),          # the same table row with the generator's pixel noise
    "cap_plus_1": (dict(n=CAP + 1, seed=16, outliers=0.4), 20),
    "n2000": (dict(n=2000, seed=17, outliers=0.5), 20),
    "duplicates": (dict(n=60, seed=18, outliers=0.2, duplicates=12), 20),
    "all_outliers": (dict(n=120, seed=19, outliers=1.0), 20),
}


@functools.lru_cache(maxsize=None)
def scene(name, fix_scale):
    kw, min_inliers = SCENES[name]
    sc = R.make_scene(scale=1.0 if fix_scale else 1.2, **kw)
    sc["min_inliers"], sc["fix_scale"] = min_inliers, fix_scale
    sc["expect"] = R.ransac(sc["pairs"], sc["k1"], sc["k2"], sc["triples"], min_inliers, fix_scale)
    return sc


def run(sc):
    from sivo_amd import sim3_solver
    return sim3_solver.sim3_ransac(sc["pairs"], sc["k1"], sc["k2"], sc["triples"], sc["min_inliers"], sc["fix_scale"])


def problem(sc):
    return {k: sc[k] for k in ("pairs", "k1", "k2", "triples", "min_inliers", "fix_scale")}


def same_bits(a, b):
    return (all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("count", "T", "inlier_bits"))
            and (a["first_accept"], a["best"]) == (b["first_accept"], b["best"]))


def first_difference(got, want):
    """Where the transforms differ, for the report of a failing parity: (hypothesis, float index, got, want) as hex."""
    g, w = np.asarray(got["T"]).view(np.uint32), np.asarray(want["T"]).view(np.uint32)
    bad = np.argwhere(g != w)
    return [(int(h), int(i), float(got["T"][h, i]).hex(), float(want["T"][h, i]).hex()) for h, i in bad[:8]], len(bad)


@pytest.mark.parametrize("fix_scale", [True, False])
@pytest.mark.parametrize("name", list(SCENES))
def test_ransac_equals_restatement_bit_for_bit(name, fix_scale):
    sc = scene(name, fix_scale)
    want, got = sc["expect"], run(sc)
    print(name, fix_scale, "counts differing:", int((got["count"] != want["count"]).sum()), "T:", first_difference(got, want))
    assert got["T"].tobytes() == want["T"].tobytes(), first_difference(got, want)          # (NaN-bearing transforms too: bytes)
    assert np.array_equal(got["count"], want["count"])
    assert got["inlier_bits"].tobytes() == want["inlier_bits"].tobytes()
    assert (got["first_accept"], got["best"]) == (want["first_accept"], want["best"])
    # the scene does what its row of the table says
    if name == "all_outliers":
        assert got["first_accept"] == -1
    elif name == "duplicates":
        assert np.isnan(got["T"]).any() and not np.isnan(got["T"]).all()
    elif name not in ("minimum", "min_inliers_is_n"):
        assert got["first_accept"] >= 0 and len(set(got["count"].tolist())) > 5        # counts differ between hypotheses


def test_min_inliers_equal_to_n_is_one_iteration():
    from sivo_amd import sim3_solver
    sc = scene("min_inliers_is_n", True)
    s = sim3_solver.Sim3Solver(sc["pairs"], sc["k1"], sc["k2"], True, randint=R.seeded_randint(5))
    s.set_ransac_parameters(0.99, 20, 300)
    assert s.max_its == 1
    T, no_more, inl, n = s.iterate(5)
    assert T is None and no_more and n == 0 and s.iterations == 1 and s.triples.shape == (1, 3)


def test_accepted_hypothesis_is_plausible():
    """200 pairs, 30 % gross outliers (>= 30 px in image 1, thresholds <= 10.9 px), no pixel noise, acceptance above 100 inliers:
    a hypothesis that explains more than 100 of the 140 true inliers is the true transform up to float rounding, so its inliers are
    true inliers (with zero pixel noise no pair lies within the noise of its threshold), and S12 is the truth within the float32
    bound of the host test (tests/test_sim3_ransac_host.py, HORN_TOL: the same generator, the same kind of samples)."""
    from test_sim3_ransac_host import HORN_TOL
    for fix_scale in (True, False):
        sc = scene("outliers30", fix_scale)
        got = run(sc)
        h = got["first_accept"]
        assert h >= 0 and got["count"][h] > 100
        inl = np.unpackbits(got["inlier_bits"][h].view(np.uint8), bitorder="little")[:200].astype(bool)
        e1, e2 = R.true_errors(sc)
        true_inlier = ~sc["outlier"]
        assert np.all(e1[true_inlier] < 0.01) and np.all(e2[true_inlier] < 0.01) and np.all(e1[sc["outlier"]] > 25.0)
        assert not np.any(inl & ~true_inlier)
        T = got["T"][h].astype(np.float64)
        assert np.max(np.abs(T[:9].reshape(3, 3) - sc["R"])) < HORN_TOL["R"]
        assert np.max(np.abs(T[9:12] - sc["t"])) < HORN_TOL["t"]
        assert abs(T[12] - sc["s"]) < HORN_TOL["s"]


def test_batch_equals_single_calls():
    from sivo_amd import sim3_solver
    names = [("outliers30", True), ("minimum", False), ("cap_plus_1", True), ("word_65", False), ("duplicates", True), ("n2000", False)]
    scs = []
    for i, (n, f) in enumerate(names):
        sc = dict(scene(n, f))
        sc["k1"] = sc["k1"] * np.float32(1 + 0.01 * i); sc["k2"] = sc["k2"] * np.float32(1 - 0.01 * i)     # different intrinsics
        sc["triples"] = sc["triples"][:max(1, 300 - 37 * i)]                                               # and hypothesis counts
        scs.append(sc)
    singles = [run(sc) for sc in scs]
    batch = sim3_solver.sim3_ransac_batch([problem(sc) for sc in scs])
    for s, b in zip(singles, batch):
        assert same_bits(s, b)
    assert len({len(s["count"]) for s in singles}) > 3 and any(s["first_accept"] >= 0 for s in singles)


def test_ransac_is_deterministic():
    sc = scene("n2000", False)
    assert same_bits(run(sc), run(sc))


def test_cpp_class_equals_python_class(tmp_path):
    """Three candidates, one SolveAll, the round-robin iterate(5) of LoopClosing.cc:294-313 until every candidate said bNoMore: the
    C++ class (through tests/sim3_ransac_prog.cpp) and the Python class, given the same draws, return the same matrices (hex
    floats), inlier vectors and bNoMore at every call."""
    from sivo_amd import sim3_solver
    exe = host_prog.build("sim3_ransac_prog", tmp_path, link_lib=True)
    cands = [("word_65", True, (0.99, 20, 300)), ("outliers30", False, (0.99, 100, 40)), ("all_outliers", True, (0.99, 20, 23))]
    text, solvers, checkers = [str(len(cands))], [], []
    for k, (name, fix, par) in enumerate(cands):
        sc = scene(name, fix)
        kf1, kf2, pts, m12 = R.keyframe_pair(sc, 900 + k, random_pose=True, n_extra=14)
        idx, recs = R.gather(kf1, kf2, m12, pts)
        draws = np.random.default_rng(77 + k).integers(0, 1 << 20, 3 * par[2]).tolist()
        text.append(R.scene_text(sc, kf1, kf2, pts, m12, fix) + f"{par[0]!r} {par[1]} {par[2]} {len(draws)} " + " ".join(map(str, draws)))
        s = sim3_solver.Sim3Solver(recs, sc["k1"], sc["k2"], fix, indices1=idx, n_matches=len(m12), randint=R.replay_randint(draws))
        s.set_ransac_parameters(*par)
        solvers.append(s)
        checkers.append(R.Sequential(len(idx), lambda h, s=s: (int(s.result["count"][h]), h), *par))
    lines = host_prog.run_text(exe, ["run"], "\n".join(text) + "\n", 120).strip().splitlines()
    sim3_solver.Sim3Solver.solve_all(solvers + [None])
    discarded, pos, accepted = [False] * len(cands), 0, 0
    while not all(discarded):
        for i, s in enumerate(solvers):
            if discarded[i]:
                continue
            T, no_more, inl, n = s.iterate(5)
            h, *rest = checkers[i].iterate(5)                    # the checker's sequential semantics over the device's counts
            assert (T is not None, no_more, n) == (h is not None, *rest) and s.iterations == checkers[i].iterations
            discarded[i] = discarded[i] or no_more
            assert lines[pos].split() == ["call", str(i), str(int(no_more)), str(n), str(int(T is not None)), str(s.max_its)], (pos, lines[pos])
            pos += 1
            if T is not None:
                accepted += 1
                want = np.concatenate([T.reshape(-1), s.estimated_rotation().reshape(-1), s.estimated_translation(), [s.estimated_scale()]])
                got = np.array([float.fromhex(v) for v in lines[pos].split()], np.float32)
                assert got.tobytes() == want.astype(np.float32).tobytes()
                assert lines[pos + 1] == "".join("1" if b else "0" for b in inl)
                pos += 2
    assert pos == len(lines) and accepted >= 2
