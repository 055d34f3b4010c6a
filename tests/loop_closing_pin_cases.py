"""The scenes of tests/test_pin_loop_closing.py and what oracle/_ref/ref_loopclosing (the reference's own LoopClosing.cc, KeyFrame.cc,
MapPoint.cc, Map.cc and Converter.cc over oracle/ref_shims_loopclosing, see oracle/Makefile) leaves on them.

LoopClosing::CorrectLoop takes its keyframe set from the covisibility graph (KeyFrame::UpdateConnections at :432), so a scene must be a real
graph.  The specs of tests/loop_correct_cases.py list observers that hold the point in no slot and their keyframes share fewer than 15
points; `consistent` turns such a spec into a graph in which every observation has its slot (an observer that held none gets one of its
own, the keyframes outside the corrected set included), the reference keyframe of a point observes it, the octave of a point's keypoints
is the point's level, and `common` points held by the current keyframe and by every keyframe meant to be corrected bring their shared
counts to 15 and more (by different amounts, so that the ordered vector is not the address order).  What cannot exist in such a graph is
left to tests/loop_correct_cases.py: a corrected keyframe without slots, a held point without observations.

The trees of the global bundle adjustment's map update are those of tests/loop_correct_cases.py as they are.

Per entry the reference's output is turned into the terms of sivo_loop_correct / sivo_gba_propagate (loop_correct_cases.LOOP_OUT /
GBA_OUT) from the reference's bytes and the scene's inputs alone; the fixture tests/golden/loop_closing_reference.npz keeps those, with a
digest of the entry's inputs (tests/golden/make_loop_closing_reference.py writes it)."""
import functools
import os
import struct

import numpy as np

import covis_adapter_cases as A
import fuse_batch_adapter_cases as AC
import essential_graph_restatement as EG
import loop_correct_cases as LC
import loop_correct_restatement as LR
import map_graph_pin_cases as M
import map_graph_restatement as G
import mappoint_restatement as MR
import covis_restatement as R
import solver_pin_cases as S

F, D = np.float32, np.float64
SENTINEL = LC.SENTINEL
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loop_closing_reference.npz")
PROGRAM = "ref_loopclosing"
TH = 15                                                    # KeyFrame.cc:363


# =====================================================================================================================================
# loop scenes
# =====================================================================================================================================
def _spec(name):
    if name in ("only_current", "two_keyframes", "sixty_five_keyframes", "duplicate_slot", "skip", "null_slots",
                "outside_observers", "quaternion_branches", "scale_one", "scale_1_07", "identity_correction"):
        return LC._loop_scene(name)
    if name.startswith("three_holders_"):
        sp = LC.loop_spec(4, 5, n_points=10, slots=6)
        sp["addrs"] = sorted(sp["addrs"], reverse=name.endswith("descending"))
        order = LC._by_rank(sp)                              # connected keyframes in CorrectedSim3's order
        ranks = (0, 2, 3)
        p = LC._fresh_point(sp, [order[r] for r in ranks], order[ranks[1]])
        for r in (ranks[2], ranks[0], ranks[1]):
            sp["slot"][order[r]].append(p)
        # the first holder in pointer order shares the fewest points with the current keyframe: it is the last of the three in the vector
        sp["common"] = {order[0]: 0, order[2]: 2, order[3]: 2}
        sp["mark"], sp["holders"] = p, [order[r] for r in ranks]
        return sp
    if name == "reference_places":
        # the reference keyframe at, after and outside the owner.  BEFORE the owner cannot be: the reference keyframe observes the point
        # (MapPoint.cc:177-178 keeps it among the observers), so in a graph whose observations have their slots a corrected keyframe
        # before the owner holds the point and is the owner itself (loop_correct_cases keeps that case for the kernels)
        sp = LC.loop_spec(10, 5, n_out=2, n_points=8, slots=5)
        order = LC._by_rank(sp)
        owner = order[2]
        sp["marks"] = []
        for ref in (owner, order[4], 5):
            p = LC._fresh_point(sp, sorted({owner, ref}), ref)
            sp["slot"][owner].append(p)
            sp["marks"].append(p)
        return sp
    if name == "fusion":
        # :530-542: a matched point over a filled slot of the current keyframe (Replace) and over an empty one (AddMapPoint + AddObservation
        # + ComputeDistinctiveDescriptors); a matched point that IS the slot's point (Replace returns at once)
        sp = LC.loop_spec(50, 3, n_out=2, n_points=12, slots=8)
        sp["fusion"] = True
        return sp
    if name in ("fuse_repair", "fuse_enters_by_replace"):
        sp = LC.loop_spec(51 if name == "fuse_repair" else 52, 4, n_out=2, n_points=12, slots=8)
        sp["fuse"] = name
        return sp
    raise KeyError(name)


LOOP_SCENES = ("only_current", "two_keyframes", "sixty_five_keyframes", "three_holders_ascending", "three_holders_descending", "duplicate_slot",
               "skip", "null_slots", "reference_places", "outside_observers", "quaternion_branches", "scale_one", "scale_1_07",
               "identity_correction", "fusion", "fuse_repair", "fuse_enters_by_replace")
FUSE_SCENES = ("fusion", "fuse_repair", "fuse_enters_by_replace")


def consistent(sp):
    """The spec as a graph: dict(slots: per keyframe (all of them) the point per slot, obs: per point {keyframe: idx}, ref, level, bad,
    corrected, pos, desc: per keyframe (slots, 32) uint8, matched, loop_points, script, matched_kf)."""
    n_kf, n_all = sp["n_kf"], sp["n_kf"] + sp["n_out"]
    cur = n_kf - 1
    sp = dict(sp, pos=list(sp["pos"]), obs=[list(o) for o in sp["obs"]], ref=list(sp["ref"]), skip=list(sp["skip"]), level=list(sp["level"]))
    slots = [list(sp["slot"][k]) if k < n_kf else [] for k in range(n_all)]
    for p, o in enumerate(sp["obs"]):
        for k in o:
            if p in slots[k]:
                continue
            if k >= n_kf and p in slots[cur] and n_kf == 1:  # the only corrected keyframe shares nothing: nobody else may be connected
                continue
            slots[k].append(p)
    if n_kf > 1:                                             # the common points: 15 + (0, 1 or 2) with every keyframe meant to be corrected
        extra = sp.get("common", {})
        first = len(sp["pos"])
        for j in range(TH + 2):
            holders = [k for k in range(n_kf - 1) if j < TH + extra.get(k, k % 3)] + [cur]
            LC._fresh_point(sp, holders, cur)
        for k in range(n_kf):
            slots[k] += [first + j for j in range(TH + 2) if k == cur or j < TH + extra.get(k, k % 3)]
    P = len(sp["pos"])
    obs = [{k: slots[k].index(p) for k in range(n_all) if p in slots[k]} for p in range(P)]
    ref = [sp["ref"][p] if sp["ref"][p] in obs[p] else (min(obs[p]) if obs[p] else cur) for p in range(P)]
    g = {"slots": slots, "obs": obs, "ref": ref, "level": sp["level"], "pos": sp["pos"],
         "bad": [bool(sp["skip"][p] and p % 2) for p in range(P)], "corrected": [bool(sp["skip"][p] and not p % 2) for p in range(P)],
         "matched": [], "loop_points": [], "script": [], "matched_kf": n_all - 1, "spec": sp, "n_kf": n_kf, "n_all": n_all, "cur": cur}
    rng = np.random.default_rng(1000 + n_all * 31 + P)
    g["desc"] = [rng.integers(0, 256, (len(s), 32), dtype=np.uint8) for s in slots]
    if sp.get("fusion"):
        _script_fusion(g)
    if sp.get("fuse"):
        _script_fuse(g, sp["fuse"])
    return g


def _loop_side_point(g, kfs, pos=(0.0, 0.0, 12.0)):
    """A point of the loop's far side: held (in new slots) by the keyframes `kfs` outside the corrected set."""
    p = len(g["pos"])
    g["pos"].append(np.asarray(pos, F)); g["level"].append(2); g["bad"].append(False); g["corrected"].append(False)
    g["obs"].append({})
    for k in kfs:
        g["slots"][k].append(p)
        g["obs"][p][k] = len(g["slots"][k]) - 1
    g["ref"].append(kfs[0])
    rng = np.random.default_rng(77 + p)
    for k in kfs:
        g["desc"][k] = np.concatenate([g["desc"][k], rng.integers(0, 256, (1, 32), dtype=np.uint8)])
    return p


def _script_fusion(g):
    cur, out = g["cur"], list(range(g["n_kf"], g["n_all"]))
    row = g["slots"][cur]
    filled = [i for i, p in enumerate(row) if p >= 0 and not g["bad"][p]]
    empty = [i for i, p in enumerate(row) if p < 0]
    assert len(filled) >= 2 and empty
    a, b = _loop_side_point(g, out), _loop_side_point(g, out[:1])
    matched = [-1] * len(row)
    matched[filled[0]] = a                                   # Replace: the slot's point goes, `a` takes its observations
    matched[empty[0]] = b                                    # the empty slot takes `b`
    matched[filled[1]] = row[filled[1]]                      # the slot's own point: Replace returns at :226
    g["matched"] = matched
    g["marks"] = {"replaced": row[filled[0]], "by": a, "added": b, "slot": empty[0], "same": row[filled[1]]}


def _script_fuse(g, which):
    """SearchAndFuse (:609-635) with the scripted Fuse: (keyframe, index into mvpLoopMapPoints, slot) per landing; the keyframes are
    visited in CorrectedSim3's order, the replacements of one keyframe after its Fuse call."""
    n_kf, out = g["n_kf"], list(range(g["n_kf"], g["n_all"]))
    order = sorted(range(n_kf), key=lambda k: g["spec"]["addrs"][k])
    lp = [_loop_side_point(g, out), _loop_side_point(g, out[:1])]
    g["loop_points"] = lp

    def good_slot(k, away):
        return next(i for i, p in enumerate(g["slots"][k]) if p >= 0 and not g["bad"][p] and len(g["obs"][p]) >= 2 and away not in g["obs"][p]
                    and g["obs"][p].get(k) == i)
    first, second = order[0], order[1]
    if which == "fuse_repair":
        # the first keyframe's landing replaces a point that several keyframes observe: the survivor (loop point 0) takes their
        # observations and its descriptor is computed anew before the second keyframe's Fuse call meets it
        i = good_slot(first, second)
        g["script"] = [(first, 0, i)]
        j = next(s for s, p in enumerate(g["slots"][second]) if p >= 0 and not g["bad"][p] and p != g["slots"][first][i])
        g["script"] += [(second, 0, j), (second, 1, j)]      # two loop points on one slot: the second Replace meets a point already replaced
        g["marks"] = {"first": first, "second": second, "victim": g["slots"][first][i]}
    else:
        # the replaced point is held by the second keyframe too: through the first keyframe's Replace loop point 0 ENTERS the second
        # keyframe, whose Fuse call then passes it over as already found
        i = next(s for s, p in enumerate(g["slots"][first]) if p >= 0 and not g["bad"][p] and second in g["obs"][p] and g["obs"][p].get(first) == s)
        victim = g["slots"][first][i]
        g["script"] = [(first, 0, i), (second, 0, g["obs"][victim][second]), (second, 1, next(s for s, p in enumerate(g["slots"][second]) if p < 0))]
        g["marks"] = {"first": first, "second": second, "victim": victim}


@functools.lru_cache(maxsize=None)
def loop_graph(name):
    return consistent(_spec(name))


def scw_of(g):
    sp = g["spec"]
    if sp.get("scw") is not None:
        return np.asarray(sp["scw"], D).copy()
    scw = EG.mul(sp["pert"], EG.sim3_from_pose(sp["poses"][g["cur"]])).copy()
    scw[7] = sp["s"]
    return scw


def loop_blob(name):
    """What `ref_loopclosing loop` reads (oracle/ref_loopclosing_driver.cpp states it)."""
    g = loop_graph(name)
    sp, K, P = g["spec"], g["n_all"], len(g["pos"])
    off = np.zeros(K + 1, np.int64)
    np.cumsum([len(s) for s in g["slots"]], out=off[1:])
    flat = np.array([p for s in g["slots"] for p in s], np.int32)
    level = np.array([0 if p < 0 else g["level"][p] for p in flat], np.uint8)
    ooff = np.zeros(P + 1, np.int64)
    np.cumsum([len(o) for o in g["obs"]], out=ooff[1:])
    okf = np.array([k for o in g["obs"] for k in sorted(o)], np.int32)
    oidx = np.array([o[k] for o in g["obs"] for k in sorted(o)], np.int32)
    parts = [M.i32(K, P), np.array(sp["ids"], np.int64), np.zeros(K, np.uint8), np.full(K, 40, F), off, flat, level, np.full(len(flat), -1, F),
             np.ones(len(flat), F), np.array(g["bad"], np.uint8), np.ones(P, np.int32), np.ones(P, np.int32), np.zeros(P, np.int64),
             np.array([len(o) for o in g["obs"]], np.int32), ooff, okf, oidx,
             np.array(sp["addrs"], np.int64), LC.SF.astype(F), np.array(sp["poses"], F), np.concatenate(g["desc"]).astype(np.uint8),
             np.array(g["pos"], F).reshape(P, 3), np.array(g["ref"], np.int32), np.array(g["corrected"], np.uint8), M.i32(g["cur"], g["matched_kf"]),
             scw_of(g), M.i32(len(g["matched"])), np.array(g["matched"], np.int32), M.i32(len(g["loop_points"])), np.array(g["loop_points"], np.int32),
             M.i32(len(g["script"])), np.array(g["script"], np.int32).reshape(-1, 3)]
    return b"".join(p if isinstance(p, bytes) else np.ascontiguousarray(p).tobytes() for p in parts)


def table_of(g, connected):
    """The keyframe table of sivo_loop_correct as loop_correct_restatement.gather_loop orders it, in scene indices: the corrected
    keyframes in std::map order, then the others in address order."""
    addrs = g["spec"]["addrs"]
    cor = sorted(set(connected), key=lambda k: addrs[k])
    return cor + sorted((k for k in range(g["n_all"]) if k not in cor), key=lambda k: addrs[k])


def realise_loop(name, connected):
    """The restatement on the graph, with mvpCurrentConnectedKFs as given (scene indices, the current keyframe last): the dict of
    loop_correct_cases.realise_loop, so that the blobs of loop_correct_cases serve."""
    g = loop_graph(name)
    sp, n_all = g["spec"], g["n_all"]
    kfs = [LR.KeyFrame(sp["ids"][k], sp["addrs"][k], sp["poses"][k]) for k in range(n_all)]
    cur = kfs[g["cur"]]
    pts = []
    for p in range(len(g["pos"])):
        mp = LR.MapPoint(g["pos"][p], LC.SF[g["level"][p]], LC.SF[-1])
        for k, idx in g["obs"][p].items():
            mp.AddObservation(kfs[k], idx)
        mp.mpRefKF = kfs[g["ref"][p]]
        mp.mbBad = g["bad"][p]
        if g["corrected"][p]:
            mp.mnCorrectedByKF = cur.mnId
        pts.append(mp)
    for k in range(n_all):
        kfs[k].mvpMapPoints = [None if v < 0 else pts[v] for v in g["slots"][k]]
    conn = [kfs[k] for k in connected]
    others = [kfs[k] for k in range(n_all) if k not in connected]
    scw = scw_of(g)
    args, table = LR.gather_loop(cur, scw, conn, pts, others)
    assert [kfs.index(k) for k in table] == table_of(g, connected)
    cor, non = LR.correct_loop(cur, scw, conn)
    expect = LR.read_loop(args, table, pts, cur, cor, non, SENTINEL)
    spec = dict(sp, n_kf=len(conn), level=g["level"])
    return {"args": args, "expect": expect, "info": {"kfs": conn + others, "table": table, "points": pts, "cur": cur, "spec": spec}}


# ---- KeyFrame::UpdateConnections of the current keyframe on the graph (covis_restatement / map_graph_restatement) -------------------------
def covis_scene(g, slots=None, obs=None, bad=None):
    sp = g["spec"]
    sc = R.Scene(g["n_all"], addr=list(sp["addrs"]), ids=list(sp["ids"]))
    slots = g["slots"] if slots is None else slots
    obs = g["obs"] if obs is None else obs
    bad = g["bad"] if bad is None else bad
    sc.points = [R.MapPoint(p) for p in range(len(obs))]
    for k, kf in enumerate(sc.kfs):
        for v in slots[k]:
            kf.add_slot(None if v < 0 else sc.points[v], 0 if v < 0 else g["level"][v])
    for p, mp in enumerate(sc.points):
        for k in sorted(obs[p]):
            mp.AddObservation(sc.kfs[k], obs[p][k])
        mp.mbBad = bool(bad[p])
    return sc


def restated_connected(name):
    """mvpCurrentConnectedKFs (:432-437) from the restatement of KeyFrame::UpdateConnections."""
    g = loop_graph(name)
    sc = covis_scene(g)
    cur = sc.kfs[g["cur"]]
    counter = R.update_connections_counter(cur)
    G.UpdateConnections(cur)
    got = [sc.kfs.index(k) for k in G.graph_members(cur).mvpOrderedConnectedKeyFrames] + [g["cur"]]
    return got, {sc.kfs.index(k): n for k, n in counter.items()}


# ---- the loop fusion (:530-542), SearchAndFuse (:609-635) and LoopConnections (:553-579) restated on covis_restatement's objects -------------
def _compute_distinctive(mp, desc):                                 # MapPoint.cc:284-347
    if mp.mbBad:                                                    # :292
        return
    observations = mp.GetObservations()
    if not observations:                                            # :299
        return
    rows = [desc[kf][idx] for kf, idx in observations if not kf.isBad()]      # :305-310
    if not rows:
        return
    mp.mDescriptor = np.array(rows[MR.best_index_literal(np.array(rows))], np.uint8)


def _replace(this, pMP, desc):                                      # MapPoint.cc:225-261
    if pMP.mnId == this.mnId:                                       # :226
        return
    obs = this.GetObservations()                                    # :236-241
    this.mObservations = {}
    this.mbBad = True
    nvisible, nfound = this.mnVisible, this.mnFound
    this.mpReplaced = pMP
    for pKF, idx in obs:                                            # :244
        if pKF not in pMP.mObservations:                            # :248
            pKF.mvpMapPoints[idx] = pMP                             # ReplaceMapPointMatch
            pMP.AddObservation(pKF, idx)
        else:
            pKF.mvpMapPoints[idx] = None                            # :252
    pMP.mnFound += nfound                                           # :256-257
    pMP.mnVisible += nvisible
    _compute_distinctive(pMP, desc)                                 # :258


def restated_fusion(name, connected):
    """The graph from the loop fusion on: what the reference's snapshot shows of slots, observations, flags, replaced-by links, found /
    visible and descriptors, the matcher's calls as the script meets them, and LoopConnections.  The correction before it changes none
    of these but the covisibility graph, which UpdateConnections of every corrected keyframe (:525) rebuilds in CorrectedSim3's order."""
    g = loop_graph(name)
    sc = covis_scene(g)
    desc = {kf: g["desc"][k] for k, kf in enumerate(sc.kfs)}
    for mp in sc.points:                                            # (the driver: every point comes with the descriptor its observations give it)
        mp.mDescriptor, mp.mpReplaced, was_bad, mp.mbBad = None, None, mp.mbBad, False
        _compute_distinctive(mp, desc)
        mp.mbBad = was_bad
    cur = sc.kfs[g["cur"]]
    G.UpdateConnections(cur)                                        # :432
    order = sorted(set(connected), key=lambda k: g["spec"]["addrs"][k])
    for k in order:                                                 # :525, inside the correction's walk
        G.UpdateConnections(sc.kfs[k])
    for i, v in enumerate(g["matched"]):                            # :530
        if v < 0:
            continue
        pLoopMP, pCurMP = sc.points[v], cur.mvpMapPoints[i]
        if pCurMP is not None:
            _replace(pCurMP, pLoopMP, desc)                         # :535
        else:
            cur.mvpMapPoints[i] = pLoopMP                           # :537-539
            pLoopMP.AddObservation(cur, i)
            _compute_distinctive(pLoopMP, desc)
    loop_points = [sc.points[p] for p in g["loop_points"]]
    fuse_kf, actions, met = [], [], []
    for k in order:                                                 # :612, CorrectedSim3's order
        pKF = sc.kfs[k]
        fuse_kf.append(k)
        vpReplacePoints = [None] * len(loop_points)
        already = {id(p) for p in pKF.mvpMapPoints if p is not None and not p.isBad()}      # ORBmatcher.cc:951, KeyFrame::GetMapPoints
        for kf, lp, slot in g["script"]:
            if kf != k:
                continue
            pMP = loop_points[lp]
            met.append(np.zeros(32, np.uint8) if pMP.mDescriptor is None else pMP.mDescriptor)
            if pMP.isBad():
                actions.append(0)
            elif id(pMP) in already:
                actions.append(1)
            elif pKF.mvpMapPoints[slot] is not None:
                if not pKF.mvpMapPoints[slot].isBad():
                    vpReplacePoints[lp] = pKF.mvpMapPoints[slot]
                    actions.append(2)
                else:
                    actions.append(4)
            else:
                pMP.AddObservation(pKF, slot)
                pKF.mvpMapPoints[slot] = pMP
                actions.append(3)
        for i, pRep in enumerate(vpReplacePoints):                  # :628-633: after the keyframe's Fuse call, in list order
            if pRep is not None:
                _replace(pRep, loop_points[i], desc)
    conn = []
    vector = [sc.kfs[k] for k in connected]
    for pKFi in vector:                                             # :555-579
        previous = list(G.graph_members(pKFi).mvpOrderedConnectedKeyFrames)
        G.UpdateConnections(pKFi)
        left = set(pKFi.mConnectedKeyFrameWeights) - set(previous) - set(vector)
        conn.append((pKFi, left))
    words = []
    for pKFi, left in sorted(conn, key=lambda e: e[0].addr):       # std::map order, each std::set in pointer order
        words += [sc.kfs.index(pKFi), len(left)] + [sc.kfs.index(k) for k in sorted(left, key=lambda k: k.addr)]
    index = {id(p): i for i, p in enumerate(sc.points)}
    P = len(sc.points)
    return {"slots": [[-1 if p is None else index[id(p)] for p in kf.mvpMapPoints] for kf in sc.kfs],
            "obs": [[[sc.kfs.index(kf), idx] for kf, idx in mp.GetObservations()] for mp in sc.points],
            "n_obs": [mp.nObs for mp in sc.points],
            "bad": np.array([mp.mbBad for mp in sc.points], np.uint8),
            "replaced": np.array([-1 if mp.mpReplaced is None else index[id(mp.mpReplaced)] for mp in sc.points], np.int32),
            "found_visible": np.array([[mp.mnFound, mp.mnVisible] for mp in sc.points], np.int32).ravel(),
            "has_descriptor": np.array([mp.mDescriptor is not None for mp in sc.points], np.uint8),
            "descriptor": np.array([np.zeros(32, np.uint8) if mp.mDescriptor is None else mp.mDescriptor for mp in sc.points], np.uint8).reshape(P * 32),
            "fuse_kf": np.array(fuse_kf, np.int32), "fuse_action": np.array(actions, np.int32),
            "fuse_descriptor": np.array(met, np.uint8).reshape(-1), "loop_connections": np.array(words, np.int32)}


def parsed_dump(facts, name):
    g = loop_graph(name)
    kfs, pts, at = A.parse_graph(facts["dump"], g["n_all"], len(g["pos"]))
    assert at == len(facts["dump"])
    return kfs, pts


# =====================================================================================================================================
# the reference program, the facts
# =====================================================================================================================================
def records(raw):
    out, at = {}, 0
    while at < len(raw):
        n, = struct.unpack_from("<i", raw, at)
        name = raw[at + 4:at + 4 + n].decode()
        size, count = struct.unpack_from("<iq", raw, at + 4 + n)
        at += 16 + n
        out[name] = (size, raw[at:at + size * count])
        at += size * count
    return out


def _rec(recs, name, dt):
    size, b = recs[name]
    assert size == np.dtype(dt).itemsize, name
    return np.frombuffer(b, dt).copy()


def loop_facts_of(name, raw):
    """The reference's output in the terms of sivo_loop_correct (loop_correct_cases.LOOP_OUT, flat, sentinel-filled as
    loop_correct_restatement.read_loop fills them), from its bytes and the scene's inputs alone; and what the loop fusion and SearchAndFuse
    left."""
    g = loop_graph(name)
    sp, n_all, P = g["spec"], g["n_all"], len(g["pos"])
    r = records(raw)
    connected = _rec(r, "connected", np.int32)
    table = table_of(g, connected.tolist())
    K = len(set(connected.tolist()))
    assert _rec(r, "corrected_kf", np.int32).tolist() == table[:K] and _rec(r, "noncorrected_kf", np.int32).tolist() == table[:K]
    tcw, ow = _rec(r, "tcw", F).reshape(n_all, 16), _rec(r, "ow", F).reshape(n_all, 3)
    for k in table[K:]:                                     # a keyframe outside the corrected set keeps its pose
        assert tcw[k].tobytes() == np.asarray(sp["poses"][k], F).tobytes()
    by_id = {sp["ids"][k]: i for i, k in enumerate(table)}
    cur_id = sp["ids"][g["cur"]]
    by, refid = _rec(r, "corrected_by_id", np.int64), _rec(r, "corrected_reference_id", np.int64)
    pos, normal = _rec(r, "pos", F).reshape(P, 3), _rec(r, "normal", F).reshape(P, 3)
    dmin, dmax = _rec(r, "min_dist", F), _rec(r, "max_dist", F)
    out = {"connected": connected, "noncorrected_siw": _rec(r, "noncorrected_sim3", D), "corrected_siw": _rec(r, "corrected_sim3", D),
           "tiw_out": tcw[table[:K]].ravel(), "ow_out": ow[table[:K]].ravel(), "corrected_by": np.full(P, -1, np.int32),
           "pos_out": np.full((P, 3), SENTINEL, F), "normal": np.full((P, 3), SENTINEL, F), "max_dist": np.full(P, SENTINEL, F),
           "min_dist": np.full(P, SENTINEL, F), "flags": np.full(P, 255, np.uint8)}
    for p in range(P):
        if g["bad"][p] or g["corrected"][p] or by[p] != cur_id:
            assert pos[p].tobytes() == np.asarray(g["pos"][p], F).tobytes(), "a point the correction passed over has moved"
            continue
        out["corrected_by"][p] = by_id[int(refid[p])]
        out["pos_out"][p], out["normal"][p], out["max_dist"][p], out["min_dist"][p], out["flags"][p] = pos[p], normal[p], dmax[p], dmin[p], 0
    for k in ("pos_out", "normal"):
        out[k] = out[k].ravel()
    # the graph as correction, loop fusion and SearchAndFuse left it
    out.update(dump=_rec(r, "dump", np.int32), bad=_rec(r, "bad", np.uint8), replaced=_rec(r, "replaced", np.int32),
               found_visible=_rec(r, "found_visible", np.int32), has_descriptor=_rec(r, "has_descriptor", np.uint8),
               descriptor=_rec(r, "descriptor", np.uint8), loop_connections=_rec(r, "loop_connections", np.int32),
               fuse_kf=_rec(r, "fuse_kf", np.int32), fuse_scw=_rec(r, "fuse_scw", F), fuse_action=_rec(r, "fuse_action", np.int32),
               fuse_descriptor=_rec(r, "fuse_descriptor", np.uint8), loop_edges=_rec(r, "loop_edges", np.int32), after=_rec(r, "after", np.int32))
    return out


# ---- the trees ---------------------------------------------------------------------------------------------------------------------
TREE_SCENES = ("run_0", "run_1", "run_2", "run_40", "origin_outside", "unreached_reference", "two_origins", "bad_point", "points_0")
OTHER_BA = 3                                               # mnBAGlobalForKF of what the BA did not hold (loop_correct_cases.realise_tree)


def tree_blob(name):
    sp = LC.tree_scene(name)["info"]["spec"]
    K, P = len(sp["parent"]), len(sp["pos"])
    ba = lambda flags: np.where(np.array(flags, bool), LC.N_LOOP_KF, OTHER_BA).astype(np.int64)
    parts = [M.i32(K, P, len(sp["origins"])), np.array([LC.N_LOOP_KF], np.int64), np.array(sp["addrs"], np.int64), np.arange(K, dtype=np.int64),
             np.array(sp["poses"], F), np.array(sp["gba"], F), np.array(sp["bef"], F), ba(sp["in_gba"]), np.array(sp["parent"], np.int32),
             np.array(sp["origins"], np.int32), np.array(sp["pos"], F).reshape(P, 3), np.array(sp["pos_gba"], F).reshape(P, 3),
             ba(sp["point_in_gba"]), np.array(sp["point_bad"], np.uint8), np.array(sp["ref"], np.int32)]
    return b"".join(p if isinstance(p, bytes) else np.ascontiguousarray(p).tobytes() for p in parts)


def tree_facts_of(name, raw):
    """The reference's output in the terms of sivo_gba_propagate (loop_correct_cases.GBA_OUT, flat).  A keyframe the walk reached is one
    whose mTcwBefGBA now holds the pose it had (:715; the scenes' stale mTcwBefGBA is never that pose)."""
    sp = LC.tree_scene(name)["info"]["spec"]
    K, P = len(sp["parent"]), len(sp["pos"])
    r = records(raw)
    tcw, ow, gba, bef = (_rec(r, n, F).reshape(K, -1) for n in ("tcw", "ow", "tcw_gba", "tcw_bef"))
    in_gba = (_rec(r, "kf_ba", np.int64) == LC.N_LOOP_KF).astype(np.uint8)
    before = np.array(sp["poses"], F).reshape(K, 16)
    reached = np.array([bef[k].tobytes() == before[k].tobytes() for k in range(K)], np.uint8)
    for k in range(K):
        assert np.asarray(sp["bef"][k], F).tobytes() != before[k].tobytes()
        if not reached[k]:
            assert tcw[k].tobytes() == before[k].tobytes() and bef[k].tobytes() == np.asarray(sp["bef"][k], F).tobytes()
    pos = _rec(r, "pos", F).reshape(P, 3)
    status = np.zeros(P, np.uint8)
    pos_out = np.full((P, 3), SENTINEL, F)
    for p in range(P):
        if sp["point_bad"][p]:
            status[p] = LR.POINT_BAD
        elif sp["point_in_gba"][p]:
            status[p] = LR.POINT_FROM_BA
        else:
            status[p] = LR.POINT_CARRIED if in_gba[sp["ref"][p]] else LR.POINT_REF_OUTSIDE
        if status[p] in (LR.POINT_FROM_BA, LR.POINT_CARRIED):
            pos_out[p] = pos[p]
        else:
            assert pos[p].tobytes() == np.asarray(sp["pos"][p], F).tobytes(), "a point the update passed over has moved"
    return {"tcw_gba": gba.ravel(), "in_gba": in_gba, "tcw_bef": bef.ravel(), "tcw_out": np.where(reached[:, None] == 1, tcw, F(SENTINEL)).ravel(),
            "ow_out": np.where(reached[:, None] == 1, ow, F(SENTINEL)).ravel(), "kf_reached": reached, "pos_out": pos_out.ravel(),
            "point_status": status, "after": _rec(r, "after", np.int32)}


# ---- SearchAndFuse alone, on the loop scenes of tests/fuse_batch_adapter_cases.py ---------------------------------------------------------
# The matcher's script for each: (keyframe, index into the list, slot), written from the scene's own description of what lands where (the
# candidate choice is the part this build does not pin; the tests require that the adapter's event log shows the same landings).
ADAPTER_SCRIPTS = {
    # A on the key that holds C in target 0 (Replace), B on the empty key; in target 1 A is already found, B lands again
    "loop_same_point_two_keyframes": [(0, 0, 0), (0, 1, 1), (1, 0, 0), (1, 1, 1)],
    # A on C's key in target 0 (Replace: A's descriptor becomes DC0); with it A picks K_BETA in target 1; nothing in target 2
    "loop_descriptor_change": [(0, 0, 0), (1, 0, 1)],
}
ADAPTER_ACTIONS = {"loop_same_point_two_keyframes": [2, 3, 1, 3], "loop_descriptor_change": [2, 3]}


def adapter_blob(name):
    w = AC.scene(name)
    K, P = len(w.kfs), len(w.points)
    off = np.zeros(K + 1, np.int64)
    np.cumsum([len(f["keys"]) for f in w.kfs], out=off[1:])
    keys = [q for f in w.kfs for q in f["keys"]]
    script = ADAPTER_SCRIPTS[name]
    parts = [M.i32(K, P), off, np.array([q["slot"] for q in keys], np.int32), np.array([(q["xy"][0] - 10.0 if q["stereo"] else -1.0) for q in keys], F),
             np.array([q["desc"] for q in keys], np.uint8).reshape(len(keys), 32), np.array([p["bad"] for p in w.points], np.uint8),
             np.array([p["desc"] for p in w.points], np.uint8).reshape(P, 32), M.i32(len(w.list)), np.array(w.list, np.int32),
             M.i32(len(w.targets)), np.array(w.targets, np.int32), M.i32(len(script)), np.array(script, np.int32).reshape(-1, 3)]
    return b"".join(p if isinstance(p, bytes) else np.ascontiguousarray(p).tobytes() for p in parts)


def adapter_facts_of(name, raw):
    r = records(raw)
    return {"dump": _rec(r, "dump", np.int32), "bad": _rec(r, "bad", np.uint8), "replaced": _rec(r, "replaced", np.int32),
            "found_visible": _rec(r, "found_visible", np.int32), "descriptor": _rec(r, "descriptor", np.uint8),
            "fuse_kf": _rec(r, "fuse_kf", np.int32), "fuse_action": _rec(r, "fuse_action", np.int32)}


def adapter_graph_differs(dump, want, name):
    """One dump of tests/fuse_batch_adapter_prog.cpp (fuse_batch_adapter_cases.parse) against the reference's facts: the names that differ."""
    w = AC.scene(name)
    kfs, pts, at = A.parse_graph(want["dump"], len(w.kfs), len(w.points))
    assert at == len(want["dump"])
    fv = want["found_visible"].reshape(-1, 2)
    bad = []
    if dump["slots"] != [k["slots"] for k in kfs]:
        bad.append("slots")
    for i, p in enumerate(dump["points"]):
        ref = dict(bad=int(want["bad"][i]), n_obs=pts[i]["n_obs"], found=int(fv[i, 0]), visible=int(fv[i, 1]), replaced=int(want["replaced"][i]),
                   desc=want["descriptor"][32 * i:32 * i + 32].tobytes(), obs=[(AC.kf_id(k), idx) for k, idx in pts[i]["obs"]])
        bad += ["point %d %s" % (i, key) for key in ref if p[key] != ref[key]]
    return bad


def adapter_landings(dump, name):
    """What the event log of a dump says landed: the additions (keyframe, list index, slot) and the replacements (point -> point)."""
    w = AC.scene(name)
    adds = [(a - AC.kf_id(0), w.list.index(c), b) for kind, a, b, c in dump["events"] if kind == "add_map_point"]
    return adds, [(a, b) for kind, a, b, c in dump["events"] if kind == "replace"]


# ---- entries, the fixture ------------------------------------------------------------------------------------------------------------
ENTRIES = ["loop." + n for n in LOOP_SCENES] + ["gba." + n for n in TREE_SCENES] + ["fuse." + n for n in ADAPTER_SCRIPTS]
# kept whole in the fixture (the tests marked gpu read them); every other fact of more than map_graph_pin_cases.SHA_FROM bytes as its digest
WHOLE = ("inputs", "connected") + tuple(n for n, *_ in LC.LOOP_OUT) + tuple(n for n, *_ in LC.GBA_OUT)
FUSE_WHOLE = ("dump", "bad", "replaced", "descriptor", "has_descriptor")


def entry_blob(entry):
    mode, _, name = entry.partition(".")
    return mode, (loop_blob(name) if mode == "loop" else tree_blob(name) if mode == "gba" else adapter_blob(name))


def reference_program(name=PROGRAM):
    return M.reference_program(name)


def live_facts(entry, program=PROGRAM):
    mode, blob = entry_blob(entry)
    raw = M.run_reference(mode, blob, program)
    return loop_facts_of(entry[5:], raw) if mode == "loop" else tree_facts_of(entry[4:], raw) if mode == "gba" else adapter_facts_of(entry[5:], raw)


def inputs_digest(entry):
    return S.sha(np.frombuffer(entry_blob(entry)[1], np.uint8))


def reduce_facts(entry, facts):
    whole = WHOLE + (FUSE_WHOLE if entry[5:] in FUSE_SCENES or entry.startswith("fuse.") else ())
    out = {}
    for k, v in facts.items():
        v = np.ascontiguousarray(v)
        if k in whole or v.nbytes <= M.SHA_FROM:
            out[k] = v
        else:
            out[k + ".sha"] = S.sha(v)
    return out


@functools.lru_cache(maxsize=None)
def load_fixture():
    packed = {}
    with np.load(GOLDEN, allow_pickle=False) as z:
        for member in z.files:
            name, key = member.split("|")
            packed.setdefault(name, {})[key] = z[member]
    return {name: M.unpack_entry(p) for name, p in packed.items()}


@functools.lru_cache(maxsize=None)
def recorded_facts(entry):
    fx = load_fixture()[entry]
    assert fx["inputs"].tobytes() == inputs_digest(entry).tobytes(), "the scene generator drifted from the recorded fixture: " + entry
    return fx


@functools.lru_cache(maxsize=None)
def reference_facts(entry):
    """(facts, live) of one entry: from the reference program where it is, else the fixture."""
    if reference_program():
        return live_facts(entry), True
    return recorded_facts(entry), False


def differing(got, want, names):
    """The names whose bytes differ between got (flat arrays or arrays to flatten) and the reference's facts."""
    bad = []
    for n in names:
        v, w = np.ascontiguousarray(got[n]).ravel(), np.ascontiguousarray(want[n]).ravel()
        if v.dtype != w.dtype or v.shape != w.shape or v.tobytes() != w.tobytes():
            bad.append(n)
    return bad
