"""sivo_triangulate / sivo_triangulate_batch (sivo_amd/csrc/triangulate.hip) and sivo_mappoint_refresh (sivo_amd/csrc/mappoint.hip)
against the numpy restatements (tests/triangulate_restatement.py, tests/mappoint_restatement.py) BIT FOR BIT."""
import functools

import numpy as np
import pytest

import host_prog
import mappoint_restatement as MR
import test_local_mapping_host as H
import triangulate_restatement as TR

pytestmark = pytest.mark.gpu

KEYS = ("status", "wP", "detected_class")
SCENES = {   # name -> make_problem arguments (min_margin = 0: the comparison is bit for bit, no decision needs a margin)
    "one": dict(seed=41, n=1),
    "wave_64": dict(seed=42, n=64),
    "wave_65": dict(seed=43, n=65),
    "stereo_both": dict(seed=44, n=150, stereo=(1.0, 1.0)),
    "stereo_1_only": dict(seed=45, n=150, stereo=(1.0, 0.0)),
    "stereo_2_only": dict(seed=46, n=150, stereo=(0.0, 1.0)),                   # the `else if` of :310
    "stereo_none": dict(seed=47, n=150, stereo=(0.0, 0.0)),
    "mbf_differs": dict(seed=48, n=150, stereo=(1.0, 1.0), mbf2=250.0),         # :414: keyframe 2's test uses keyframe 1's mbf
    "octave_0": dict(seed=49, n=100, octave=0),
    "octave_last": dict(seed=50, n=100, octave=7),
    "n2000": dict(seed=51, n=2000),
}


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "all_status":
        p = TR.all_status_problem()
    elif name == "nan":
        p = H.nan_problem()
    elif name == "identical_rays":
        rng = np.random.default_rng(52)
        k1, k2 = TR.make_keyframes(rng)
        p = TR.make_problem(52, 20, min_margin=0, extra=TR.special_matches(k1, k2)[1:2])
    else:
        p = TR.make_problem(min_margin=0, **SCENES[name])
    p["expect"] = TR.triangulate(p)
    return p


def run(p):
    from sivo_amd import local_mapping as LM
    return LM.triangulate(p["kf1"], p["kf2"], p["matches"], p["ratio_factor"], p["state_cov"], p["th_confidence"], p["th_entropy"])


@pytest.mark.parametrize("name", list(SCENES) + ["all_status", "nan", "identical_rays"])
def test_triangulate_equals_the_restatement_bit_for_bit(name):
    p = scene(name)
    got, want = run(p), p["expect"]
    for k in KEYS:
        assert got[k].tobytes() == want[k].tobytes(), k
    st, m = want["status"], p["matches"]
    if name == "all_status":
        assert set(st.tolist()) == set(range(10))                    # every `continue` of the loop, and the accepted match
        assert st[0] == TR.W_ZERO
    if name == "nan":
        nan = np.isnan(want["wP"]).any(axis=1)
        assert nan.sum() > 10 and (got["wP"].view(np.uint32)[np.isnan(got["wP"])] == 0x7FC00000).all()
    if name == "identical_rays":
        assert st[0] == TR.LOW_PARALLAX and not want["wP"][0].any()
    if name == "stereo_2_only":
        assert (m["r1"] < 0).all() and (m["r2"] >= 0).all() and (st == TR.ACCEPTED).sum() == 0      # keyframe 1's depth is not > 0: the gate
        assert (st == TR.SEMANTICS).sum() > 10
    if name in ("stereo_both", "mbf_differs", "n2000"):
        assert (st == TR.ACCEPTED).sum() > 5
    if name == "mbf_differs":                                        # with keyframe 2's own mbf the decisions differ
        k1 = np.array(p["kf1"])
        k1["mbf"] = p["kf2"]["mbf"]
        assert not np.array_equal(TR.triangulate(dict(p, kf1=k1))["status"], st)
    if name == "octave_last":
        assert (m["octave1"] == 7).all() and (m["octave2"] == 7).all()


def batch_problems():
    """The six problems of one sivo_triangulate_batch call (tests/local_mapping_pin_cases.py feeds the same six to the reference)."""
    probs = [TR.make_problem(60, 130, min_margin=0), TR.make_problem(61, 1, min_margin=0, stereo=(1.0, 1.0)),
             TR.make_problem(62, 64, min_margin=0, intr=(500.0, 510.0, 320.0, 240.0), mbf=200.0, nlevels=5),
             TR.make_problem(63, 0, min_margin=0), TR.make_problem(64, 65, min_margin=0, stereo=(0.0, 1.0), mbf2=300.0),
             TR.make_problem(65, 333, min_margin=0, nlevels=3)]
    probs[2]["th_confidence"], probs[4]["th_confidence"] = 0.8, 0.0
    return probs


def test_triangulate_batch_equals_the_single_calls_and_repeats():
    from sivo_amd import local_mapping as LM
    probs = batch_problems()
    assert len({len(p["matches"]) for p in probs}) == 6 and len({p["th_entropy"] for p in probs}) >= 5
    singles = [run(p) for p in probs]
    batch = LM.triangulate_batch(probs)
    again = LM.triangulate_batch(probs)
    for p, s, b, a in zip(probs, singles, batch, again):
        want = TR.triangulate(p)
        for k in KEYS:
            assert s[k].tobytes() == b[k].tobytes() == a[k].tobytes() == want[k].tobytes(), k


REFRESH = {
    "one_two": lambda: MR.make_points(71, [1, 2, 2, 1]),
    "lane_edge": lambda: MR.make_points(72, [63, 64, 65]),
    "strided": lambda: MR.make_points(73, [200]),
    "mixed_with_empty": lambda: MR.make_points(1, H.REFRESH_SIZES, bad=0.15),
    "ties": lambda: MR.make_points(74, [5, 9, 12, 2, 31, 64, 70] * 3, ties=True),
    "identical": lambda: MR.make_points(75, [4, 17, 1, 66], identical=True),
    "bad_keyframes_only": lambda: MR.make_points(4, [3, 3], bad=1.0),
    "p3000": lambda: MR.make_points(76, np.random.default_rng(76).integers(1, 31, 3000), bad=0.05),
}


@pytest.mark.parametrize("name", list(REFRESH))
def test_mappoint_refresh_equals_the_restatement_bit_for_bit(name):
    from sivo_amd import local_mapping as LM
    s = REFRESH[name]()
    got, want = LM.refresh_map_points(**s), MR.refresh(**s)
    for k in ("flags", "best_idx", "max_dist", "min_dist", "normal"):
        assert got[k].tobytes() == want[k].tobytes(), k
    if name == "one_two":
        assert not want["best_idx"].any()
    if name == "mixed_with_empty":
        assert want["flags"][5] == 3 and not want["flags"][[4, 6]].any()
        # a flagged point's entries are left as the caller had them
        out = {"best_idx": np.full(10, 77, np.int32), "max_dist": np.full(10, 5, np.float32), "min_dist": np.full(10, 6, np.float32),
               "normal": np.full((10, 3), 7, np.float32)}
        LM.refresh_map_points(out=out, **s)
        assert out["best_idx"][5] == 77 and out["max_dist"][5] == 5 and out["min_dist"][5] == 6 and (out["normal"][5] == 7).all()
        assert out["best_idx"][6] == want["best_idx"][6] and out["normal"][4].tobytes() == want["normal"][4].tobytes()
    if name == "ties":
        tied = sum(int((MR.row_medians(s["desc"][a:b]) == MR.row_medians(s["desc"][a:b]).min()).sum() > 1)
                   for a, b in zip(s["desc_off"][:-1], s["desc_off"][1:]))
        assert tied > 10
    if name == "bad_keyframes_only":
        assert (want["flags"] == 2).all() and want["max_dist"].all()
    if name == "p3000":
        again = LM.refresh_map_points(**s)
        assert all(again[k].tobytes() == got[k].tobytes() for k in got)


# ---------------------------------------------------------------------------------------------------------------------
# SIVO::TriangulateMatches / SIVO::RefreshMapPoints over stand-in SLAM types against the Python path
# ---------------------------------------------------------------------------------------------------------------------
def key_descriptors(frame, n):
    """key_descriptor of tests/local_mapping_adapter_prog.cpp."""
    i, b = np.arange(n)[:, None], np.arange(32)[None, :]
    return ((i * 37 + b * 11 + frame * 101 + (i >> 3) * 7) & 255).astype(np.uint8)


def test_cpp_triangulate_matches_equals_the_python_path(tmp_path):
    from sivo_amd import local_mapping as LM
    p = H.adapter_problem()
    m, n = p["matches"], len(p["matches"])
    raw = host_prog.run(H.adapter_prog(tmp_path), tmp_path, "triangulate", H.tri_blob(p), timeout=120)
    res = run(p)
    acc = np.flatnonzero(res["status"] == TR.ACCEPTED)
    k = len(acc)
    assert k > 10 and np.frombuffer(raw, np.int64, 1)[0] == k
    d1, d2 = key_descriptors(0, n), key_descriptors(1, n)
    k1 = np.asarray(p["kf1"])
    two = 2 * np.arange(k + 1)
    ref = LM.refresh_map_points(two, np.stack([d1[acc], d2[n - 1 - acc]], axis=1).reshape(-1, 32), two,
                                np.tile(np.stack([k1["Ow"], np.asarray(p["kf2"])["Ow"]]), (k, 1)), res["wP"][acc], np.tile(k1["Ow"], (k, 1)),
                                k1["scale_factors"][m["octave1"][acc]], np.full(k, k1["scale_factors"][int(k1["nlevels"]) - 1]))
    rec = np.dtype([("idx", np.int64, 2), ("pos", np.float32, 3), ("geom", np.float32, 5), ("desc", np.uint8, 32)])
    got = np.frombuffer(raw, rec, k, 8)
    assert got["idx"].tolist() == [[int(i), int(n - 1 - i)] for i in acc]                        # match order, both slots
    assert got["pos"].tobytes() == res["wP"][acc].tobytes()
    want_geom = np.concatenate([ref["max_dist"][:, None], ref["min_dist"][:, None], ref["normal"]], axis=1)
    assert got["geom"].tobytes() == want_geom.tobytes()
    both = np.stack([d1[acc], d2[n - 1 - acc]], axis=1)
    assert got["desc"].tobytes() == both[np.arange(k), ref["best_idx"]].tobytes()
    assert np.frombuffer(raw, np.uint8, n, 8 + k * rec.itemsize).tolist() == (res["status"] == TR.ACCEPTED).astype(int).tolist()


def test_cpp_refresh_map_points_equals_the_python_path(tmp_path):
    from sivo_amd import local_mapping as LM
    seed, sizes, bad = 1, H.REFRESH_SIZES, 0.15
    s = MR.make_points(seed, sizes, bad=bad)
    no = int(s["obs_off"][-1])
    is_bad = (np.random.default_rng(seed).random(no) < bad).astype(np.uint8)          # make_points' first draw
    assert int((1 - is_bad).sum()) == int(s["desc_off"][-1])
    n = len(sizes)
    rec = np.concatenate([s["pos"], s["ref_ow"], s["level_scale"][:, None], s["last_scale"][:, None]], axis=1).astype(np.float32)
    blob = b"".join([np.array([n], np.int64).tobytes(), s["desc_off"].astype(np.int64).tobytes(), s["obs_off"].astype(np.int64).tobytes(),
                     s["desc"].tobytes(), s["obs_ow"].tobytes(), rec.tobytes(), is_bad.tobytes()])
    raw = host_prog.run(H.adapter_prog(tmp_path), tmp_path, "refresh", blob, timeout=120)
    got = np.frombuffer(raw, np.dtype([("geom", np.float32, 5), ("desc", np.uint8, 32)]), n)
    ref = LM.refresh_map_points(**s)
    want_geom = np.concatenate([ref["max_dist"][:, None], ref["min_dist"][:, None], ref["normal"]], axis=1)
    assert got["geom"].tobytes() == want_geom.tobytes()
    for p in range(n):
        want = s["desc"][s["desc_off"][p] + ref["best_idx"][p]] if ref["flags"][p] == 0 else np.zeros(32, np.uint8)
        assert got["desc"][p].tobytes() == want.tobytes()


def test_cpp_create_new_map_points_equals_the_python_path(tmp_path):
    """SIVO::CreateNewMapPoints over the stand-in map of three neighbours (the first skipped for its baseline, the third searched after the
    second's points took their slots) against the same walk in Python: ComputeF12, sivo_search_for_triangulation, sivo_triangulate,
    sivo_mappoint_refresh per neighbour."""
    from sivo_amd import local_mapping as LM, matcher as M
    sc = H.map_scene()
    frames = sc["frames"]
    raw = host_prog.run(H.adapter_prog(tmp_path), tmp_path, "create", H.map_blob(sc, 5), timeout=120)
    k1, cur, d1 = frames[0]
    F = np.float32

    def kps(keys):
        k = np.zeros(len(keys), M.KP_DTYPE)
        k["x"], k["y"], k["size"], k["octave"], k["class_id"] = keys["x"], keys["y"], 31, keys["octave"], -1
        return k

    def nodes(keys):
        off, idx = [0], []
        for v in range(17):
            idx += np.flatnonzero(keys["node"] == v).tolist()
            off.append(len(idx))
        return np.array(off, np.int32), np.array(idx, np.int32)

    occ = [np.zeros(len(f[1]), np.uint8) for f in frames]
    recs, per_neighbour, blocked = [], [], None
    for i in range(3):
        kf, nb, d2 = frames[i + 1]
        if H.skipped(k1, kf):
            continue
        F12 = H.compute_f12(k1, kf)
        R2, t2, O1 = np.asarray(kf["Rcw"], F), np.asarray(kf["tcw"], F), np.asarray(k1["Ow"], F)
        C2 = []
        for r in range(3):                         # Pose::apply: the small-matrix path
            a = R2[3 * r] * O1[0]
            a = a + R2[3 * r + 1] * O1[1]
            a = a + R2[3 * r + 2] * O1[2]
            C2.append(a + t2[r])
        invz = F(1) / C2[2]
        ex, ey = kf["fx"] * C2[0] * invz + kf["cx"], kf["fy"] * C2[1] * invz + kf["cy"]
        nl = int(kf["nlevels"])
        sigma2 = np.asarray(kf["level_sigma2"][:nl], F)
        F2 = M.MatchFrame(kps(nb), nb["r"], d2, (0, 1241, 0, 376), np.asarray(kf["scale_factors"][:nl], F), sigma2, F(1) / sigma2)
        (off1, idx1), (off2, idx2) = nodes(cur), nodes(nb)
        search = lambda has1: M.search_for_triangulation(off1, idx1, off2, idx2, kps(cur), cur["r"], has1, d1, F2, occ[i + 1], F12, float(ex),
                                                         float(ey), False, False)[1]
        m12 = search(occ[0])
        if occ[0].any():
            blocked = int((search(np.zeros_like(occ[0])) >= 0).sum()) - int((m12 >= 0).sum())
        i1 = np.flatnonzero(m12 >= 0)
        i2 = m12[i1]
        m = np.zeros(len(i1), LM.MATCH_DTYPE)
        for f, g in (("x", "x"), ("y", "y"), ("octave", "octave"), ("r", "r"), ("depth", "depth")):
            m[f + "1"], m[f + "2"] = cur[g][i1], nb[g][i2]
        m["entropy1"], m["confidence1"], m["class1"], m["class2"] = cur["entropy"][i1], cur["confidence"][i1], cur["cls"][i1], nb["cls"][i2]
        res = LM.triangulate(k1, kf, m, np.float32(1.5) * np.float32(1.2), sc["state_cov"], sc["th_confidence"], sc["th_entropy"])
        acc = np.flatnonzero(res["status"] == TR.ACCEPTED)
        k = len(acc)
        per_neighbour.append((i, len(i1), k))
        two = 2 * np.arange(k + 1)
        both = np.stack([d1[i1[acc]], d2[i2[acc]]], axis=1)
        ref = LM.refresh_map_points(two, both.reshape(-1, 32), two, np.tile(np.stack([k1["Ow"], kf["Ow"]]), (k, 1)), res["wP"][acc],
                                    np.tile(k1["Ow"], (k, 1)), k1["scale_factors"][m["octave1"][acc]],
                                    np.full(k, k1["scale_factors"][int(k1["nlevels"]) - 1]))
        for q in range(k):
            recs.append((i, int(i1[acc[q]]), int(i2[acc[q]]), res["wP"][acc[q]], ref["max_dist"][q], ref["min_dist"][q], ref["normal"][q],
                         both[q, ref["best_idx"][q]]))
        occ[0][i1[acc]] = 1
        occ[i + 1][i2[acc]] = 1
    assert [p[0] for p in per_neighbour] == [1, 2] and all(p[1] > 20 and p[2] > 3 for p in per_neighbour), per_neighbour
    assert blocked is not None and blocked > 0          # neighbour 2's search lost the slots neighbour 1's points took
    rec = np.dtype([("idx", np.int64, 3), ("pos", np.float32, 3), ("geom", np.float32, 5), ("desc", np.uint8, 32)])
    assert np.frombuffer(raw, np.int64, 1)[0] == len(recs) and len(raw) == 8 + len(recs) * rec.itemsize
    got = np.frombuffer(raw, rec, len(recs), 8)
    assert got["idx"].tolist() == [[r[0], r[1], r[2]] for r in recs]
    assert got["pos"].tobytes() == np.array([r[3] for r in recs], np.float32).tobytes()
    assert got["geom"].tobytes() == np.array([[r[4], r[5], *r[6]] for r in recs], np.float32).tobytes()
    assert got["desc"].tobytes() == np.array([r[7] for r in recs], np.uint8).tobytes()
