"""sivo_pnp_ransac / sivo_pnp_ransac_batch (sivo_amd/csrc/pnp_ransac.hip) against the numpy restatement of PnPsolver
(tests/pnp_ransac_restatement.py) BIT FOR BIT, and SIVO::PnPsolver over stand-in frames against the Python class."""
import functools
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import host_prog
import pnp_ransac_restatement as R
import test_pnp_ransac_host as H

pytestmark = pytest.mark.gpu

# the LDS cap of the hypothesis kernel: the scene one point above it takes the memory path for exactly one point
CAP = int(re.search(r"PN_CAP = (\d+)", open(os.path.join(ROOT, "sivo_amd", "csrc", "pnp_ransac.hip")).read()).group(1))
KEYS = ("count", "T", "inlier_bits", "refined", "refined_T", "refined_bits")

SCENES = {   # name -> (make_scene arguments, n_hyp, min_inliers, best_in)
    "minimum": (dict(seed=12, n=4), 1, 4, 0),                                    # the sample is everything, the refine set those 4
    "word_64": (dict(seed=13, n=64, outliers=0.25, noise=0.5), 40, 10, 0),
    "word_65": (dict(seed=14, n=65, outliers=0.25, noise=0.5), 40, 10, 0),
    "cap_plus_1": (dict(seed=16, n=CAP + 1, outliers=0.4, noise=0.5), 24, 20, 0),
    "n2000": (dict(seed=17, n=2000, outliers=0.5), 120, 20, 0),
    "outliers30": (dict(seed=34, n=200, outliers=0.3), 100, 100, 0),            # two records: refinements of different n
    "duplicates": (dict(seed=18, n=60, outliers=0.2, duplicates=12), 40, 10, 0),
    "coplanar": (dict(seed=4, n=50, coplanar=True), 40, 10, 0),
    "all_outliers": (dict(seed=19, n=120, outliers=1.0), 40, 10, 0),
    "best_in_above": (dict(seed=20, n=80, outliers=0.2), 40, 10, 80),
}


@functools.lru_cache(maxsize=None)
def scene(name):
    kw, n_hyp, min_inliers, best_in = SCENES[name]
    sc = R.make_scene(**kw)
    n = kw["n"]
    rng = np.random.RandomState(kw["seed"])
    S = R.draw_samples(rng, n, n_hyp)
    if name == "duplicates":          # samples that hold a world point twice (make_scene: point j repeats point j - 1)
        dup = [1 + (d * 7) % (n - 1) for d in range(12)]
        for h, j in enumerate(dup[:10]):
            rest = [i for i in range(n) if i not in (j, j - 1)]
            S[h] = [j - 1, j, rest[h], rest[h + 20]]
    sc.update(samples=S, min_inliers=min_inliers, best_in=best_in)
    sc["expect"] = R.pnp_ransac(sc["pts"], sc["K"], S, min_inliers, best_in)
    return sc


def run(sc):
    from sivo_amd import pnp_solver
    return pnp_solver.pnp_ransac(sc["pts"], sc["K"], sc["samples"], sc["min_inliers"], sc["best_in"])


def problem(sc):
    return {"points": sc["pts"], "K": sc["K"], "samples": sc["samples"], "min_inliers": sc["min_inliers"], "best_in": sc["best_in"]}


def same_bits(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in KEYS) and a["n_records"] == b["n_records"]


def first_difference(got, want, key="T"):
    """Where the poses differ, for the report of a failing parity: (hypothesis, float index, got, want) as hex words."""
    g, w = np.asarray(got[key]).view(np.uint32), np.asarray(want[key]).view(np.uint32)
    bad = np.argwhere(g != w)
    return [(int(h), int(i), hex(g[h, i]), hex(w[h, i])) for h, i in bad[:8]], len(bad)


@pytest.mark.parametrize("name", list(SCENES))
def test_ransac_equals_restatement_bit_for_bit(name):
    sc = scene(name)
    want, got = sc["expect"], run(sc)
    print(name, "counts differing:", int((got["count"] != want["count"]).sum()), "T:", first_difference(got, want),
          "refined_T:", first_difference(got, want, "refined_T"), "records:", want["n_records"])
    assert got["T"].tobytes() == want["T"].tobytes(), first_difference(got, want)            # (NaN-bearing poses too: bytes)
    assert np.array_equal(got["count"], want["count"])
    assert got["inlier_bits"].tobytes() == want["inlier_bits"].tobytes()
    assert np.array_equal(got["refined"], want["refined"]) and got["n_records"] == want["n_records"]
    assert got["refined_T"].tobytes() == want["refined_T"].tobytes(), first_difference(got, want, "refined_T")
    assert got["refined_bits"].tobytes() == want["refined_bits"].tobytes()
    # the scene does what its row of the table says
    rec = np.flatnonzero(got["refined"] >= 0)
    if name == "minimum":
        assert got["count"].tolist() == [4] and got["refined"].tolist() == [4]
    elif name in ("all_outliers", "best_in_above"):
        assert len(rec) == 0 and (got["refined"] == -1).all()
        assert name != "best_in_above" or (got["count"] >= sc["min_inliers"]).any()
    elif name in ("duplicates", "coplanar"):
        assert np.isnan(got["T"]).any() and not np.isnan(got["T"]).all()
        assert (got["count"][np.isnan(got["T"]).any(axis=1)] == 0).all()
    elif name in ("outliers30", "word_65"):
        # several records, so refinements of different n in one launch.  (A noise-free scene gives few: an all-inlier sample either
        # finds the pose, and then counts every inlier, or lands in a wrong minimum; seed 34 has a 126 in front of the 140.)
        assert len(rec) >= (2 if name == "outliers30" else 3) and len(set(got["count"][rec].tolist())) == len(rec)
    else:
        assert len(rec) >= 1 and len(set(got["count"].tolist())) >= 3                         # counts differ between hypotheses


def test_batch_equals_the_single_calls():
    from sivo_amd import pnp_solver
    names = ["minimum", "word_65", "outliers30", "duplicates", "cap_plus_1", "best_in_above"]
    scs = []
    for i, nm in enumerate(names):
        sc = dict(scene(nm))
        sc["samples"] = sc["samples"][: max(1, len(sc["samples"]) - 3 * i)]       # different n_hyp (and K below)
        sc["K"] = tuple(np.float32(v) + np.float32(i) for v in sc["K"])
        scs.append(sc)
    single = [run(sc) for sc in scs]
    batch = pnp_solver.pnp_ransac_batch([problem(sc) for sc in scs])
    assert len({(len(sc["pts"]), len(sc["samples"])) for sc in scs}) == 6
    for nm, a, b in zip(names, single, batch):
        assert same_bits(a, b), nm
    assert sum(b["n_records"] for b in batch) >= 4


def test_two_runs_give_the_same_bytes():
    sc = scene("n2000")
    a, b = run(sc), run(sc)
    assert same_bits(a, b) and a["n_records"] >= 1


def test_accepted_pose_is_plausible():
    sc = R.make_scene(21, 120, outliers=0.3)
    S = R.draw_samples(np.random.RandomState(21), 120, 60)
    from sivo_amd import pnp_solver
    got = pnp_solver.pnp_ransac(sc["pts"], sc["K"], S, 60)
    rec = np.flatnonzero(got["refined"] > 60)
    assert len(rec) >= 1
    T = got["refined_T"][rec[0]].astype(np.float64)
    assert np.max(np.abs(T[:9].reshape(3, 3) - sc["R"])) < H.TRUE_TOL["R"] and np.max(np.abs(T[9:] - sc["t"])) < H.TRUE_TOL["t"]
    inl = R.unpack_bits(got["refined_bits"][rec[0]], 120)
    assert not (inl & ~sc["true_inlier"]).any() and inl.sum() == sc["true_inlier"].sum()


def test_cpp_class_equals_python_class(tmp_path):
    """Three candidates with the same draws through SetDraw / randint, one of them never accepting: one SolveAll, then the
    round-robin iterate(5) of Tracking.cc:1293-1310; every call agrees on the matrix (hex floats), vbInliers, nInliers, bNoMore."""
    from sivo_amd import pnp_solver
    frames = [H.make_frame(31, 40), H.make_frame(32, 36, outliers=1.0), H.make_frame(33, 50, outliers=0.4)]
    # (the second candidate, all outliers, is cut to 3 iterations: its iterate(5) runs 5, the loop condition being an OR, so it draws
    # and evaluates 2 more in a further call)
    pars = [(0.99, 10, 300, 0.5, 5.991), (0.99, 10, 3, 0.5, 5.991), (0.99, 10, 300, 0.5, 5.991)]
    max_calls = 12
    text = f"{len(frames)}\n"
    solvers = []
    for k, (fr, par) in enumerate(zip(frames, pars)):
        draws = np.random.RandomState(50 + k).randint(0, 1 << 20, 4000)
        text += H.frame_text(fr) + f"{par[0]} {par[1]} {par[2]} {par[3]} {par[4]} {len(draws)} " + " ".join(str(d) for d in draws) + "\n"
        pts, idx, sig2 = R.gather(fr)
        it = iter(draws.tolist())
        s = pnp_solver.PnPsolver(pts["xw"], np.stack([pts["u"], pts["v"]], 1), sig2, fr["K"], indices=idx, n_matches=len(fr["matches"]),
                                 randint=lambda lo, hi, it=it: lo + next(it) % (hi - lo + 1))
        s.set_ransac_parameters(par[0], par[1], par[2], 4, par[3], par[4])
        solvers.append(s)
    exe = host_prog.build("pnp_ransac_prog", tmp_path, link_lib=True)
    lines = host_prog.run_text(exe, ["run", max_calls], text, 120).strip().splitlines()
    pnp_solver.PnPsolver.solve_all(solvers + [None])
    done, calls, pos = [False] * 3, [0] * 3, 0
    accepted, no_more_seen = set(), set()
    while not all(done):
        for i, s in enumerate(solvers):
            if done[i]:
                continue
            T, no_more, inl, n = s.iterate(5)
            calls[i] += 1
            if no_more or calls[i] >= max_calls:
                done[i] = True
            assert lines[pos].split() == ["call", str(i), str(int(no_more)), str(n), str(int(T is not None)), str(s.max_its), str(s.min_inliers)], pos
            pos += 1
            if T is not None:
                got = np.array([float.fromhex(v) for v in lines[pos].split()], np.float32)
                assert got.tobytes() == T.reshape(-1).tobytes(), (lines[pos], [float(v).hex() for v in T.reshape(-1)])
                assert lines[pos + 1] == "".join("1" if b else "0" for b in inl)
                pos += 2
                if not no_more:
                    accepted.add(i)
            if no_more:
                no_more_seen.add(i)
    assert pos == len(lines)
    assert 1 not in accepted and 1 in no_more_seen and accepted >= {0}        # the all-outlier candidate never accepts
    assert solvers[1].max_its == 3 and len(solvers[1].result["count"]) == 5                 # the call past the maximum drew 2 more
