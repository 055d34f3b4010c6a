"""What tests/test_pin_local_mapping.py and tests/golden/make_local_mapping_reference.py share: the scenes handed to the reference's own
LocalMapping.cc / MapPoint.cc (oracle/_ref/ref_localmapping: oracle/ref_localmapping_driver.cpp), the files that program reads and writes,
and the fixture.  The scenes are those of tests/test_gpu_local_mapping.py (SCENES, all_status, nan, identical_rays, the six batch problems,
every entry of REFRESH) and of tests/test_local_mapping_host.py (SCENES_64), brought into the form the reference's classes can hold:
  * the reference keeps mThConfidence / mThEntropyReduction in float members, so the two thresholds are rounded to float;
  * the reference reads entropy, confidence and class from per-pixel maps, so matches whose keypoints truncate to one pixel of a keyframe
    share the values of the first of them (as tests/test_local_mapping_host.py::map_scene does).
The reference's results are recorded as data only (tests/golden/local_mapping_reference.npz)."""
import functools
import hashlib
import os
import subprocess
import tempfile

import numpy as np

import mappoint_restatement as MR
import solver_pin_cases as S
import test_gpu_local_mapping as G
import test_local_mapping_host as H
import triangulate_restatement as TR

F, D = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "local_mapping_reference.npz")
FULL_ROWS = 64          # a table of up to this many rows is kept whole in the fixture; of a larger one the first rows and a digest


# ---------------------------------------------------------------------------------------------------------------------
# triangulation scenes
# ---------------------------------------------------------------------------------------------------------------------
def pin_problem(p):
    """p with float thresholds and one semantic value per pixel (see the module's docstring)."""
    p = dict(p)
    p.pop("expect", None)
    p["th_confidence"], p["th_entropy"] = float(F(p["th_confidence"])), float(F(p["th_entropy"]))
    m = np.array(p["matches"], TR.MATCH_DTYPE)
    for px, fields in ((("y1", "x1"), ("entropy1", "confidence1", "class1")), (("y2", "x2"), ("class2",))):
        seen = {}
        with np.errstate(all="ignore"):
            rows, cols = m[px[0]].astype(np.int32), m[px[1]].astype(np.int32)      # the truncation of static_cast<int>
        for i in range(len(m)):
            j = seen.setdefault((int(rows[i]), int(cols[i])), i)
            for f in fields:
                m[f][i] = m[f][j]
    p["matches"] = m
    return p


# all_status: for every `continue` of the loop, one more match: a match the restatement rejects with that status, changed by the mildest
# of a fixed list of edits under which the restatement accepts it (another octave pair, a stereo depth, keypoint 2 put where a point at some
# depth along keypoint 1's ray projects; then the semantic values).  The reference must accept exactly the twins among them.
def _twin_edits(m, k1, k2):
    def put(q, **kw):
        q = q.copy()
        for f, v in kw.items():
            q[f] = v
        return q
    R1, t1 = np.asarray(k1["Rcw"], D).reshape(3, 3), np.asarray(k1["tcw"], D)
    R2, t2 = np.asarray(k2["Rcw"], D).reshape(3, 3), np.asarray(k2["tcw"], D)
    geo = [m]
    geo += [put(m, octave1=o1, octave2=o2) for o1 in range(8) for o2 in range(8)]
    for z in (8.0, 15.0, 25.0, 400.0, 2000.0):
        r1 = max(float(m["x1"]) - float(k1["mbf"]) / z, 0.0)
        geo += [put(m, depth1=z, r1=r1), put(m, depth1=z, r1=r1, depth2=-1, r2=-1)]
    for z in (6.0, 12.0, 24.0):
        for dx in (0.0, 40.0, 4000.0, 9000.0):
            x1 = float(m["x1"]) + dx
            Xc = np.array([(x1 - float(k1["cx"])) / float(k1["fx"]), (float(m["y1"]) - float(k1["cy"])) / float(k1["fy"]), 1.0]) * z
            X2 = R2 @ (R1.T @ (Xc - t1)) + t2
            if X2[2] > 0.5:
                geo.append(put(m, x1=x1, x2=float(k2["fx"]) * X2[0] / X2[2] + float(k2["cx"]), y2=float(k2["fy"]) * X2[1] / X2[2] + float(k2["cy"]), octave2=m["octave1"],
                               depth1=-1, r1=-1, depth2=-1, r2=-1))
                geo.append(put(geo[-1], depth1=z, r1=max(x1 - float(k1["mbf"]) / z, 0.0)))
    out = []
    for g in geo:                      # (other semantic values need other pixels: the keypoints move one row down)
        h = put(g, y1=g["y1"] + F(1), y2=g["y2"] + F(1))
        out += [g, put(h, class2=h["class1"]), put(h, class1=2, class2=2, confidence1=0.95, entropy1=0.0), put(h, class1=2, class2=2, confidence1=0.95, entropy1=-50.0)]
    return out


@functools.lru_cache(maxsize=None)
def all_status_with_twins():
    """(the problem with the twins appended, the number of matches before them, the status each twin's original had)."""
    p = pin_problem(TR.all_status_problem())
    base = TR.triangulate(p)["status"]
    k1, k2 = TR._kf(p["kf1"]), TR._kf(p["kf2"])
    twins, of = [], []
    for code in range(10):
        if code == TR.ACCEPTED:
            continue
        for i in np.flatnonzero(base == code):
            cands = np.array(_twin_edits(p["matches"][i], k1, k2), TR.MATCH_DTYPE)
            ok = TR.triangulate(dict(p, matches=cands))["status"] == TR.ACCEPTED
            for j in np.flatnonzero(ok):                 # the mildest edit that is still accepted beside the matches already there
                q = pin_problem(dict(p, matches=np.concatenate([p["matches"], np.array(twins + [cands[j]], TR.MATCH_DTYPE)])))
                if TR.triangulate(q)["status"][-1] == TR.ACCEPTED:
                    twins.append(cands[j])
                    of.append(code)
                    break
            if of and of[-1] == code:
                break
    q = pin_problem(dict(p, matches=np.concatenate([p["matches"], np.array(twins, TR.MATCH_DTYPE)])))
    return q, len(p["matches"]), of


@functools.lru_cache(maxsize=None)
def batch_problems():
    return G.batch_problems()


@functools.lru_cache(maxsize=None)
def tri_scene(name):
    if name == "all_status":
        return all_status_with_twins()[0]
    if name in G.SCENES or name in ("nan", "identical_rays"):
        return pin_problem(G.scene(name))
    kind, i = name.split("_")
    if kind == "batch":
        probs = batch_problems()
        return pin_problem(probs[int(i)])
    return pin_problem(TR.make_problem(**H.SCENES_64[int(i)]))


TRI_NAMES = list(G.SCENES) + ["all_status", "nan", "identical_rays"] + [f"batch_{i}" for i in range(6)] + [f"host_{i}" for i in range(len(H.SCENES_64))]


@functools.lru_cache(maxsize=None)
def tri_restated(name):
    """The restatement on the scene, computed once: what tr_match gives, the refresh of the accepted matches' new points, ComputeF12 and
    the two CheckSemantics results on the restatement's wP."""
    p = tri_scene(name)
    r = TR.triangulate(p)
    m, n = p["matches"], len(p["matches"])
    acc = np.flatnonzero(r["status"] == TR.ACCEPTED)
    k = len(acc)
    d1, d2 = tri_descriptors(n)
    k1, k2 = np.asarray(p["kf1"]), np.asarray(p["kf2"])
    two = 2 * np.arange(k + 1)
    both_d = np.stack([d1[acc], d2[acc]], axis=1)      # std::map<KeyFrame *, size_t> walks keyframe 1 first: the driver puts it first in one array
    both_o = np.stack([k1["Ow"], k2["Ow"]])
    ref = MR.refresh(two, both_d.reshape(-1, 32), two, np.tile(both_o, (k, 1)), r["wP"][acc], np.tile(k1["Ow"], (k, 1)),
                     k1["scale_factors"][m["octave1"][acc]], np.full(k, k1["scale_factors"][int(k1["nlevels"]) - 1]))
    with np.errstate(all="ignore"):
        w = r["wP"].astype(D)
        s1 = np.asarray(k1["level_sigma2"])[m["octave1"]].astype(D)
        mi = TR.mutual_information(p["state_cov"], k1["fx"], k1["fy"], k1["mb"], w[:, 0], w[:, 1], w[:, 2], s1)
        crit = (m["depth1"] > 0) & (m["class1"] <= 8) & (m["confidence1"] >= D(p["th_confidence"]))
        cls1 = np.where(crit & ~(mi - m["entropy1"] < D(p["th_entropy"])), m["class1"], TR.VOID).astype(np.uint8)
    return {"accepted": (r["status"] == TR.ACCEPTED).astype(np.uint8), "status": r["status"], "detected_class": r["detected_class"], "wP": r["wP"], "cls1": cls1, "cls2": m["class2"].astype(np.uint8),
            "F12": H.compute_f12(k1, k2).astype(F), "acc": acc, "desc": both_d[np.arange(k), ref["best_idx"]] if k else np.zeros((0, 32), np.uint8),
            "geom": np.concatenate([ref["normal"], ref["min_dist"][:, None], ref["max_dist"][:, None]], axis=1).astype(F)}


def tri_descriptors(n):
    """The descriptors of match k's two keypoints: those of tests/local_mapping_adapter_prog.cpp, whose keyframe 2 holds match k's
    keypoint as key n - 1 - k."""
    return G.key_descriptors(0, n), G.key_descriptors(1, n)[::-1].copy()


def tri_as_facts(r, k1k2=None):
    """accepted / wP / geom / desc (and F12, cls1, cls2 where r has them) in the form the reference's facts have."""
    acc = np.flatnonzero(r["accepted"])
    out = {"accepted": np.asarray(r["accepted"], np.uint8), "wP": canon(np.asarray(r["wP"], F)[acc]), "geom": canon(r["geom"]), "desc": np.asarray(r["desc"], np.uint8)}
    for k in ("cls1", "cls2"):
        if k in r:
            out[k] = np.asarray(r[k], np.uint8)
    if "F12" in r:
        out["F12"] = canon(r["F12"])
    return out


def tri_from(name, status, wP, refresh):
    """The facts of a scene from an implementation's status and wP and its sivo_mappoint_refresh (`refresh(**arrays)`) of the new points."""
    p = tri_scene(name)
    m, n = p["matches"], len(p["matches"])
    acc = np.flatnonzero(status == TR.ACCEPTED)
    k = len(acc)
    d1, d2 = tri_descriptors(n)
    k1, k2 = np.asarray(p["kf1"]), np.asarray(p["kf2"])
    two = 2 * np.arange(k + 1)
    both_d = np.stack([d1[acc], d2[acc]], axis=1)
    s = dict(desc_off=two, desc=both_d.reshape(-1, 32), obs_off=two, obs_ow=np.tile(np.stack([k1["Ow"], k2["Ow"]]), (k, 1)).astype(F), pos=wP[acc],
             ref_ow=np.tile(k1["Ow"], (k, 1)).astype(F), level_scale=k1["scale_factors"][m["octave1"][acc]],
             last_scale=np.full(k, k1["scale_factors"][int(k1["nlevels"]) - 1], F))
    ref = refresh(**s) if k else {"best_idx": np.zeros(0, np.int32), "normal": np.zeros((0, 3), F), "min_dist": np.zeros(0, F), "max_dist": np.zeros(0, F)}
    return tri_as_facts({"accepted": status == TR.ACCEPTED, "wP": wP, "desc": both_d[np.arange(k), ref["best_idx"]] if k else np.zeros((0, 32), np.uint8),
                         "geom": np.concatenate([ref["normal"], ref["min_dist"][:, None], ref["max_dist"][:, None]], axis=1).astype(F)})


def check_detected_class(want, status, detected_class, what):
    """What an implementation of tr_match reports as CheckSemantics(keyframe 1, ..., true) -- for the matches that reached it, accepted or
    rejected there -- against what the reference's own CheckSemantics returned on the same point."""
    reached = (np.asarray(status) == TR.ACCEPTED) | (np.asarray(status) == TR.SEMANTICS)
    assert np.asarray(detected_class, np.uint8)[reached].tobytes() == np.asarray(want["cls1"], np.uint8)[reached].tobytes(), (what, "detected_class")
    return int(reached.sum())


def tri_blob(name):
    p = tri_scene(name)
    n = len(p["matches"])
    d1, d2 = tri_descriptors(n)
    return b"".join([H.tri_blob(p), d1.tobytes(), d2.tobytes(), np.ascontiguousarray(tri_restated(name)["wP"], F).tobytes()])


def parse_tri(raw, n):
    at = 0

    def take(dtype, count, shape=None):
        nonlocal at
        a = np.frombuffer(raw, dtype, count, at)
        at += a.nbytes
        return a.reshape(shape) if shape else a
    out = {"F12": take(F, 9, (3, 3)), "accepted": take(np.uint8, n), "cls1": take(np.uint8, n), "cls2": take(np.uint8, n)}
    g = take(F, 8 * n, (n, 8))
    out["wP"], out["geom"], out["desc"] = g[:, :3], g[:, 3:], take(np.uint8, 32 * n, (n, 32))
    assert at == len(raw)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# refresh scenes
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def refresh_scene(name):
    """(the CSR scene, per observation: its keyframe is bad, per point: the point is bad, reversed).  `<scene>` is the entry of
    tests/test_gpu_local_mapping.py's REFRESH; `mixed_with_empty_reversed` allocates the keyframes in descending address order;
    `mixed_with_empty_bad_points` marks every third point bad; `even_sizes` is EXTRA_REFRESH's."""
    base = name
    for suffix in ("_reversed", "_bad_points"):
        if name.endswith(suffix):
            base = name[:-len(suffix)]
    calls = []
    real = MR.make_points

    def recording(seed, sizes, bad=0.0, **kw):
        calls.append((seed, bad))
        return real(seed, sizes, bad=bad, **kw)
    MR.make_points = recording
    try:
        s = (EXTRA_REFRESH if base in EXTRA_REFRESH else G.REFRESH)[base]()
    finally:
        MR.make_points = real
    (seed, bad), = calls
    no = int(s["obs_off"][-1])
    kf_bad = (np.random.default_rng(seed).random(no) < bad).astype(np.uint8)       # make_points' first draw
    assert int((1 - kf_bad).sum()) == int(s["desc_off"][-1])
    point_bad = np.zeros(len(s["pos"]), np.uint8)
    if name.endswith("_bad_points"):
        point_bad[::3] = 1
    return s, kf_bad, point_bad, name.endswith("_reversed")


# even_sizes: 120 points with an even number of descriptors, where element int(0.5 * (N - 1)) of the sorted row is not element N / 2
EXTRA_REFRESH = {"even_sizes": lambda: MR.make_points(77, [4, 6, 8, 10, 12, 14] * 20)}
REFRESH_NAMES = list(G.REFRESH) + ["mixed_with_empty_reversed", "mixed_with_empty_bad_points", "even_sizes"]


def refresh_blob(name):
    s, kf_bad, point_bad, rev = refresh_scene(name)
    n = len(s["pos"])
    rec = np.concatenate([s["pos"], s["ref_ow"], s["level_scale"][:, None], s["last_scale"][:, None]], axis=1).astype(F)
    return b"".join([np.array([n, int(rev)], np.int64).tobytes(), np.asarray(s["desc_off"], np.int64).tobytes(), np.asarray(s["obs_off"], np.int64).tobytes(),
                     np.ascontiguousarray(s["desc"], np.uint8).tobytes(), np.ascontiguousarray(s["obs_ow"], F).tobytes(), rec.tobytes(),
                     kf_bad.tobytes(), point_bad.tobytes()])


def walked(name):
    """The scene as std::map<KeyFrame *, size_t> walks it: the observations (and with them the good descriptors) of every point in
    address order — reversed where the keyframes were allocated in descending order."""
    s, kf_bad, point_bad, rev = refresh_scene(name)
    if not rev:
        return s
    s = dict(s)
    desc, ow = s["desc"].copy(), s["obs_ow"].copy()
    for a, b in zip(s["desc_off"][:-1], s["desc_off"][1:]):
        desc[a:b] = s["desc"][a:b][::-1]
    for a, b in zip(s["obs_off"][:-1], s["obs_off"][1:]):
        ow[a:b] = s["obs_ow"][a:b][::-1]
    s["desc"], s["obs_ow"] = desc, ow
    return s


def refresh_expected(name, result):
    """result: best_idx / max_dist / min_dist / normal / flags of sivo_mappoint_refresh on walked(name) (the restatement, the host build
    or the device) -> what the reference's two functions leave in the points: touched (n, 2), desc (n, 32), geom (n, 5)."""
    s, _, point_bad, _ = refresh_scene(name)
    s = walked(name)
    n = len(s["pos"])
    live = point_bad == 0
    touched = np.stack([(result["flags"] == 0) & live, ((result["flags"] & 1) == 0) & live], axis=1).astype(np.uint8)
    desc = np.zeros((n, 32), np.uint8)
    for p in np.flatnonzero(touched[:, 0]):
        desc[p] = s["desc"][s["desc_off"][p] + result["best_idx"][p]]
    geom = np.concatenate([result["normal"], result["min_dist"][:, None], result["max_dist"][:, None]], axis=1).astype(F)
    geom[touched[:, 1] == 0] = [0, 0, 0, -1, -1]
    return {"touched": touched, "desc": desc, "geom": geom}


def parse_refresh(raw, n):
    t = np.frombuffer(raw, np.uint8, 2 * n).reshape(n, 2)
    d = np.frombuffer(raw, np.uint8, 32 * n, 2 * n).reshape(n, 32)
    g = np.frombuffer(raw, F, 5 * n, 34 * n).reshape(n, 5)
    assert len(raw) == 54 * n
    return {"touched": t, "desc": d, "geom": g}


# ---------------------------------------------------------------------------------------------------------------------
# the loop over the neighbours: the three-neighbour map of tests/test_local_mapping_host.py
# ---------------------------------------------------------------------------------------------------------------------
WALKS = {"all": dict(checks=5, monocular=False, median=(10.0, 10.0, 10.0)),          # neighbour 0 skipped for its baseline, 1 and 2 searched
         "keyframe_arrives": dict(checks=1, monocular=False, median=(10.0, 10.0, 10.0)),    # CheckNewKeyFrames() says yes before neighbour 2
         "monocular": dict(checks=5, monocular=True, median=(10.0, 1000.0, 10.0))}     # baseline / median depth < 0.01 skips neighbours 0 and 1
WALK_NAMES = list(WALKS)
# (no scene sits AT the 0.01 of :249: the float quotient baseline / median would have to fall into the 2.4e-10 between 0.01 and the
# midpoint above the float next below it, and with the scene's baseline no float median depth puts it there)


def walk_params(name):
    return WALKS[name]


@functools.lru_cache(maxsize=None)
def walk_scene():
    sc = dict(H.map_scene())
    sc["th_confidence"], sc["th_entropy"] = float(F(sc["th_confidence"])), float(F(sc["th_entropy"]))     # float members in the reference
    return sc


def walk_blob(name):
    w = walk_params(name)
    return H.map_blob(walk_scene(), w["checks"]) + np.array([int(w["monocular"])], np.int64).tobytes() + np.array(w["median"], F).tobytes()


@functools.lru_cache(maxsize=None)
def walk_restated(name):
    """LocalMapping.cc:230-259, :471 line by line over the map, with the driver's scripted search and tr_match's restatement for the
    matches: per searched neighbour (neighbour, F12, pairs, the pairs that became points, their positions)."""
    w, sc = walk_params(name), walk_scene()
    frames = sc["frames"]
    k1, cur, _ = frames[0]
    n = len(cur)
    occ = [np.zeros(len(f[1]), bool) for f in frames]
    out, searched = [], 0
    for i in range(len(frames) - 1):
        if i > 0 and w["checks"] and searched >= w["checks"]:               # CheckNewKeyFrames(): a keyframe arrived during that search
            break
        kf, nb, _ = frames[i + 1]
        if not w["monocular"]:
            if H.skipped(k1, kf):
                continue
        else:
            v = np.asarray(kf["Ow"], F) - np.asarray(k1["Ow"], F)
            s = D(0)
            for a in range(3):
                s = s + D(v[a]) * D(v[a])
            if D(F(np.sqrt(s)) / F(w["median"][i])) < 0.01:
                continue
        searched += 1
        i1 = np.array([j for j in range(n) if not occ[0][j] and not occ[i + 1][n - 1 - j] and j % (i + 2) == 1], np.int64)
        i2 = n - 1 - i1
        m = np.zeros(len(i1), TR.MATCH_DTYPE)
        for f in ("x", "y", "octave", "r", "depth"):
            m[f + "1"], m[f + "2"] = cur[f][i1], nb[f][i2]
        m["entropy1"], m["confidence1"], m["class1"], m["class2"] = cur["entropy"][i1], cur["confidence"][i1], cur["cls"][i1], nb["cls"][i2]
        occupied = occ[0].astype(np.uint8)
        res = TR.triangulate({"kf1": k1, "kf2": kf, "matches": m, "ratio_factor": F(1.5) * F(1.2), "state_cov": sc["state_cov"],
                              "th_confidence": sc["th_confidence"], "th_entropy": sc["th_entropy"]})
        acc = np.flatnonzero(res["status"] == TR.ACCEPTED)
        occ[0][i1[acc]] = True
        occ[i + 1][i2[acc]] = True
        out.append((i, H.compute_f12(k1, kf).astype(F), np.stack([i1, i2], axis=1), np.stack([i1[acc], i2[acc]], axis=1), res["wP"][acc], occupied))
    return out


def walk_blocked(name):
    """How many pairs the LAST searched neighbour lost to slots an earlier neighbour's points took."""
    steps = walk_restated(name)
    n, k = len(walk_scene()["frames"][0][1]), steps[-1][0]
    return len([j for j in range(n) if j % (k + 2) == 1]) - len(steps[-1][2])


def walk_as_facts(steps):
    """One table per kind over the searched neighbours, so that the facts have the form of the other entries."""
    cat = lambda rows, shape, dt: np.concatenate(rows).astype(dt) if rows else np.zeros(shape, dt)
    return {"neighbours": np.array([s[0] for s in steps], np.int64), "F12": canon(cat([s[1].reshape(1, 9) for s in steps], (0, 9), F)),
            "pair_counts": np.array([len(s[2]) for s in steps], np.int64), "pairs": cat([s[2] for s in steps], (0, 2), np.int64),
            "point_counts": np.array([len(s[3]) for s in steps], np.int64), "points": cat([s[3] for s in steps], (0, 2), np.int64),
            "wP": canon(cat([s[4] for s in steps], (0, 3), F)), "occupied": cat([s[5].reshape(1, -1) for s in steps], (0, 0), np.uint8)}


def parse_walk(raw):
    at, steps, n = 0, [], len(walk_scene()["frames"][0][1])
    while at < len(raw):
        k = int(np.frombuffer(raw, np.int64, 1, at)[0]); at += 8
        F12 = np.frombuffer(raw, F, 9, at).reshape(3, 3); at += 36
        occupied = np.frombuffer(raw, np.uint8, n, at); at += n
        npairs = int(np.frombuffer(raw, np.int64, 1, at)[0]); at += 8
        pairs = np.frombuffer(raw, np.int64, 2 * npairs, at).reshape(npairs, 2); at += 16 * npairs
        nmade = int(np.frombuffer(raw, np.int64, 1, at)[0]); at += 8
        made = np.frombuffer(raw, np.int64, 2 * nmade, at).reshape(nmade, 2); at += 16 * nmade
        pos = np.frombuffer(raw, F, 3 * nmade, at).reshape(nmade, 3); at += 12 * nmade
        steps.append((k, F12, pairs, made, pos, occupied))
    return steps


def walk_facts(name, program="ref_localmapping"):
    return walk_as_facts(parse_walk(run_reference("walk", walk_blob(name), program)[0]))


def walk_blob_for_adapter(name):
    """The same bytes: `local_mapping_adapter_prog pinwalk` reads what the reference driver's `walk` reads."""
    return walk_blob(name)


# ---------------------------------------------------------------------------------------------------------------------
# SearchInNeighbors on a small graph
# ---------------------------------------------------------------------------------------------------------------------
def neighbors_graph():
    """13 keyframes (0 is the current one, mnId 10) and 8 map points.  Keyframe 2 is bad, keyframe 3 already carries the current
    keyframe's id as its fuse target; keyframe 1's second neighbours hold the current keyframe, a bad one, a marked one and a sixth entry
    (behind the limit of 5); keyframe 6 is a second neighbour of two first neighbours; the current keyframe has 11 covisible keyframes
    (10 count in the stereo case, 20 when monocular).  Point 1 and 4 are bad, point 6 is already marked as a candidate, points 0 and 2
    are shared with the current keyframe, points 3 and 5 are seen by two targets."""
    ordered = {0: [1, 2, 3, 4, 5, 9, 10, 11, 12, 7, 8], 1: [6, 0, 2, 7, 3, 8], 4: [6, 1, 8], 5: [9]}
    slots = {0: [0, -1, 1, 2], 1: [3, 0, -1, 4], 6: [5, 3, 6], 7: [5], 4: [7], 5: [2]}
    kfs = [dict(bad=int(i == 2), target=10 if i == 3 else 0, ordered=ordered.get(i, []), slots=slots.get(i, [])) for i in range(13)]
    points = [dict(bad=int(p in (1, 4)), candidate=10 if p == 6 else 0) for p in range(8)]
    return kfs, points


NEIGHBOR_NAMES = ["stereo", "monocular"]


def neighbors_blob(name):
    kfs, points = neighbors_graph()
    out = [len(kfs), int(name == "monocular")]
    for k in kfs:
        out += [k["bad"], k["target"], len(k["ordered"]), *k["ordered"], len(k["slots"]), *k["slots"]]
    out.append(len(points))
    for p in points:
        out += [p["bad"], p["candidate"]]
    return np.array(out, np.int64).tobytes()


def neighbors_restated(name):
    """LocalMapping.cc:547-637 line by line over the graph (Fuse changes nothing: the stand-in matcher only records)."""
    kfs, points = neighbors_graph()
    kfs, points = [dict(k) for k in kfs], [dict(p) for p in points]
    cur_id = 10
    targets = []
    for i in kfs[0]["ordered"][:20 if name == "monocular" else 10]:
        k = kfs[i]
        if k["bad"] or k["target"] == cur_id:
            continue
        targets.append(i)
        k["target"] = cur_id
        for j in k["ordered"][:5]:
            k2 = kfs[j]
            if k2["bad"] or k2["target"] == cur_id or 10 + j == cur_id:
                continue
            targets.append(j)
    cands = []
    for i in targets:
        for p in kfs[i]["slots"]:
            if p < 0 or points[p]["bad"] or points[p]["candidate"] == cur_id:
                continue
            points[p]["candidate"] = cur_id
            cands.append(p)
    refreshed = [p for p in kfs[0]["slots"] if p >= 0 and not points[p]["bad"]]
    return {"targets": np.array(targets, np.int64), "candidates": np.array(cands, np.int64), "refreshed": np.array(refreshed, np.int64),
            "update_connections": np.array([1], np.int64)}


def neighbors_facts(name, program="ref_localmapping"):
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.txt")
        with open(fin, "wb") as f:
            f.write(neighbors_blob(name))
        r = subprocess.run([reference_program(program), "neighbors", fin, fout], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        lines = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in open(fout).read().splitlines()}
    return {"targets": np.array(lines["T"], np.int64), "candidates": np.array(lines["C"], np.int64), "refreshed": np.array(lines["R"], np.int64),
            "update_connections": np.array(lines["U"], np.int64)}


# ---------------------------------------------------------------------------------------------------------------------
# cos(2 * atan2(mb / 2, depth)): LocalMapping.cc:308 as g++ resolves it
# ---------------------------------------------------------------------------------------------------------------------
def cosine_inputs():
    """The 75 000 (mb, depth) pairs of tests/test_local_mapping_host.py::test_the_cosine_is_within_one_ulp_of_the_float64_value."""
    rng = np.random.default_rng(0)
    depth = np.concatenate([rng.uniform(0.05, 200, 20000), 10.0 ** rng.uniform(-3, 4, 5000)]).astype(F)
    return np.concatenate([np.stack([np.full(len(depth), F(mb), F), depth], axis=1) for mb in (0.1, 0.5371, 1.0)])


def cosine_worst_ulps(values):
    """The largest distance, in float ulps, of `values` from the float rounding of float64 cos(2 * arctan2(mb / 2, depth)) over cosine_inputs()."""
    v = cosine_inputs()
    exact = np.cos(2 * np.arctan2(v[:, 0].astype(D) / 2, v[:, 1].astype(D))).astype(F)
    return float((np.abs(np.asarray(values, F).astype(D) - exact.astype(D)) / np.spacing(np.abs(exact)).astype(D)).max())


# ---------------------------------------------------------------------------------------------------------------------
# the reference program and the fixture
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference_program(name="ref_localmapping"):
    """oracle/_ref/ref_localmapping (or _san), (re)built where the reference's sources are; None where neither they nor a built program are."""
    if S.reference_present():
        subprocess.run(["make", "-s", "-C", S.ORACLE, "_ref/" + name], check=True)
    exe = os.path.join(S.ORACLE, "_ref", name)
    return exe if os.path.exists(exe) else None


def run_reference(mode, blob, program="ref_localmapping"):
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(blob)
        r = subprocess.run([reference_program(program), mode, fin, fout], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (mode, r.returncode, r.stderr[-3000:])
        with open(fout, "rb") as f:
            return f.read(), r.stdout


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def canon(a):
    """float32 with every NaN the quiet NaN the ABI stores"""
    bits = np.ascontiguousarray(a, F).view(np.uint32).copy()
    bits[np.isnan(a)] = 0x7FC00000
    return bits.view(F)


def reduce_facts(facts):
    """A table of more than FULL_ROWS rows as its first rows and a digest of the whole; small tables and flags whole."""
    out = {}
    for k, v in facts.items():
        v = np.ascontiguousarray(v)
        if v.ndim == 2 and v.shape[0] > FULL_ROWS and k not in ("touched", "pairs", "points", "occupied"):
            out[k + ".head"], out[k + ".sha"] = v[:FULL_ROWS], sha(v)
        else:
            out[k] = v
    return out


def same_facts(want, got, what):
    """want: facts as the reference gave them (live: whole tables; fixture: reduced).  got: whole tables.  Byte for byte."""
    for k, v in got.items():
        v = np.ascontiguousarray(v)
        if k in want:
            assert v.shape == want[k].shape and v.tobytes() == np.ascontiguousarray(want[k]).tobytes(), (what, k)
        else:
            assert v[:FULL_ROWS].tobytes() == want[k + ".head"].tobytes() and sha(v).tobytes() == want[k + ".sha"].tobytes(), (what, k)


def tri_facts(name, program="ref_localmapping"):
    n = len(tri_scene(name)["matches"])
    raw, _ = run_reference("tri", tri_blob(name), program)
    o = parse_tri(raw, n)
    acc = np.flatnonzero(o["accepted"])
    return {"accepted": o["accepted"], "cls1": o["cls1"], "cls2": o["cls2"], "F12": canon(o["F12"]), "wP": canon(o["wP"][acc]), "geom": canon(o["geom"][acc]),
            "desc": o["desc"][acc]}


def refresh_facts(name, program="ref_localmapping"):
    raw, _ = run_reference("refresh", refresh_blob(name), program)
    o = parse_refresh(raw, len(refresh_scene(name)[0]["pos"]))
    return {"touched": o["touched"], "desc": o["desc"], "geom": canon(o["geom"])}


def cosine_facts(program="ref_localmapping"):
    v = cosine_inputs()
    raw, out = run_reference("cos", np.array([len(v)], np.int64).tobytes() + v.tobytes(), program)
    return {"cos": np.frombuffer(raw, F).reshape(-1, 1), "sizeof": np.array([int(out.split()[0])], np.int64)}


@functools.lru_cache(maxsize=None)
def live_entries():
    e = {"tri." + n: dict(tri_facts(n), inputs=sha(np.frombuffer(tri_blob(n), np.uint8))) for n in TRI_NAMES}
    e.update({"refresh." + n: dict(refresh_facts(n), inputs=sha(np.frombuffer(refresh_blob(n), np.uint8))) for n in REFRESH_NAMES})
    e.update({"walk." + n: dict(walk_facts(n), inputs=sha(np.frombuffer(walk_blob(n), np.uint8))) for n in WALK_NAMES})
    e.update({"neighbors." + n: dict(neighbors_facts(n), inputs=sha(np.frombuffer(neighbors_blob(n), np.uint8))) for n in NEIGHBOR_NAMES})
    e["cos"] = cosine_facts()
    return e


@functools.lru_cache(maxsize=None)
def load_fixture():
    entries = {}
    with np.load(GOLDEN, allow_pickle=False) as z:
        for member in z.files:
            name, key = member.split("|")
            entries.setdefault(name, {})[key] = z[member]
    return entries


@functools.lru_cache(maxsize=None)
def reference_facts(entry):
    """(facts, live) of one entry (`tri.<scene>`, `refresh.<scene>`, `cos`): from the reference program where it is, else the fixture."""
    if reference_program():
        kind, _, name = entry.partition(".")
        return (tri_facts(name) if kind == "tri" else refresh_facts(name) if kind == "refresh" else walk_facts(name) if kind == "walk" else neighbors_facts(name) if kind == "neighbors" else cosine_facts()), True
    return recorded_facts(entry), False


def recorded_facts(entry):
    fx = load_fixture()[entry]
    kind, _, name = entry.partition(".")
    if kind != "cos":
        blob = tri_blob(name) if kind == "tri" else refresh_blob(name) if kind == "refresh" else walk_blob(name) if kind == "walk" else neighbors_blob(name)
        assert fx["inputs"].tobytes() == sha(np.frombuffer(blob, np.uint8)).tobytes(), "the scene generator drifted from the recorded fixture: " + entry
    return fx
