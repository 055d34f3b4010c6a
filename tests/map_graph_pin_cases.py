"""What tests/test_pin_map_graph.py runs: the scenes of the covisibility and local-map tests (and a few of its own) as blobs for
oracle/_ref/ref_mapgraph — the reference's own KeyFrame.cc, MapPoint.cc, Map.cc, LocalMapping.cc and Tracking.cc over real KeyFrame and
MapPoint objects —, the facts that program writes as dicts of integer arrays, and the fixture tests/golden/map_graph_reference.npz that
holds them where the reference is absent.  An entry is `<group>.<scene>`:

  conn.<scene>          KeyFrame::UpdateConnections for a list of keyframes in order: every keyframe and point afterwards (`dump`), and
                        read from it mConnectedKeyFrameWeights of the keyframe updated last, which is its KFcounter (`last_connected`)
  kfcull.<scene>.<mono> LocalMapping::KeyFrameCulling with the real KeyFrame::SetBadFlag: `dump`, the EraseKeyFrame calls in order
                        (`erased`), and read from the dump `decision` per local keyframe and `bad_after` per point
  mpcull.<scene>.<mono> LocalMapping::MapPointCulling: `dump`, the list afterwards (`list`), `trace` per listed point, `bad_after` per point
  localmap.<scene>      Tracking::UpdateLocalMap: both vectors, both reference keyframes, the frame's slots, every mnTrackReferenceForFrame
  bawin.<scene>         the graph Optimizer::LocalBundleAdjustment has built at its first initializeOptimization (oracle/_ref/ref_bawindow,
                        the reference's Optimizer.cc over the recording g2o stand-in): local and fixed keyframes and local points in
                        vertex order, per local point its edges as (pose vertex, idx), the three stamps of every object afterwards
  bawin_map.<scene>     the same on ba_window_cases.adapter_scene: a map whose observations name the slots that hold the points

All facts are integers; every comparison is an equality of bytes."""
import functools
import os
import subprocess
import tempfile

import numpy as np

import ba_window_cases as B
import ba_window_restatement as BW
import covis_adapter_cases as A
import covis_cases as C
import covis_restatement as R
import localmap_cases as L
import localmap_restatement as LR
import map_graph_restatement as G
import solver_pin_cases as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "map_graph_reference.npz")
WHOLE = ("last_connected", "decision", "trace", "list", "erased", "local_kf", "local_points", "reference", "frame_reference", "frame", "inputs",
         "fixed_kf", "local_point", "edge_off", "edge_pose", "edge_idx", "culled.erased", "culled.kf_bad", "culled.point_bad", "localmap.local_kf",
         "localmap.reference", "localmap.frame_reference", "window.local_kf", "window.fixed_kf")
SHA_FROM = 1024          # a fact of more bytes that no test marked gpu reads is kept as the SHA-256 of its bytes
ANCHOR_ID = 1 << 20      # the driver's extra keyframe: reference keyframe of every point, current keyframe, default parent


def i32(*v):
    return np.array(v, np.int32).tobytes()


# ---- the trailer every covisibility blob ends with ------------------------------------------------------------------------------------
def trailer(sc, links=False):
    out = [np.array([kf.addr for kf in sc.kfs], np.int64).tobytes(), np.array([kf.mbBad for kf in sc.kfs], np.uint8).tobytes(), i32(int(links))]
    if links:
        index = {kf: k for k, kf in enumerate(sc.kfs)}
        for kf in sc.kfs:
            G.graph_members(kf)
        w = [sorted(kf.mConnectedKeyFrameWeights.items(), key=lambda it: it[0].addr) for kf in sc.kfs]
        off, wk = C.csr([[index[o] for o, _ in x] for x in w], np.int32)
        _, wv = C.csr([[v for _, v in x] for x in w], np.int32)
        out += [np.array([-1 if kf.mpParent is None or kf.mpParent not in index else index[kf.mpParent] for kf in sc.kfs], np.int32).tobytes(),
                np.array([kf.mbFirstConnection for kf in sc.kfs], np.uint8).tobytes(), off.tobytes(), wk.tobytes(), wv.tobytes()]
    return b"".join(out)


def with_anchor(sc):
    """The driver's anchor on the Python side: behind every keyframe in address order, the parent of every keyframe that has none."""
    anchor = R.KeyFrame(ANCHOR_ID, max([kf.addr for kf in sc.kfs], default=0) + 1)
    G.graph_members(anchor)
    for kf in sc.kfs:
        if G.graph_members(kf).mpParent is None:
            G.ChangeParent(kf, anchor)
    return anchor


# =====================================================================================================================================
# UpdateConnections
# =====================================================================================================================================
def _shared(sc, a, b, n):
    for _ in range(n):
        sc.point([(a, 1), (b, 1)])


def conn_tied(descending):
    """Keyframe 0 shares 14 / 15 / 15 / 16 points with keyframes 1-4: 14 makes no connection, the two 15s are ordered by pointer (the
    larger pointer first after the push_front), ascending and descending addr."""
    def build():
        sc = R.Scene(5, addr=[500, 400, 300, 200, 100] if descending else None)
        for k, n in ((1, 14), (2, 15), (3, 15), (4, 16)):
            _shared(sc, 0, k, n)
        return sc, [0]
    return build


def conn_below_th(descending):
    """Nothing reaches 15; keyframes 1 and 3 tie at 7: the first maximum in pointer order is the one connection."""
    def build():
        sc = R.Scene(4, addr=[400, 300, 200, 100] if descending else None)
        for k, n in ((1, 7), (2, 3), (3, 7)):
            _shared(sc, 0, k, n)
        return sc, [0]
    return build


def conn_same_id():
    """Keyframe 2 carries keyframe 0's mnId and is another object: KeyFrame.cc:356 compares ids, so it is not counted from keyframe 0
    (nor keyframe 0 from it), while keyframe 1 counts both."""
    sc = R.Scene(3, ids=[4, 9, 4])
    _shared(sc, 0, 2, 20)
    _shared(sc, 0, 1, 16)
    _shared(sc, 1, 2, 17)
    return sc, [0, 2, 1]


def conn_bad_observer():
    """Keyframe 1 is bad and observes all the same: counted, connected and made the parent (isBad is not asked)."""
    sc = R.Scene(3)
    _shared(sc, 0, 1, 18)
    _shared(sc, 0, 2, 16)
    sc.kfs[1].mbBad = True
    return sc, [0]


def conn_id0():
    """The keyframe of mnId 0 gets its connections and no parent; it stays mbFirstConnection."""
    sc = R.Scene(3, ids=[0, 1, 2])
    _shared(sc, 0, 1, 15)
    _shared(sc, 0, 2, 4)
    return sc, [0, 1]


def conn_second_call():
    """Keyframe 0 has been connected before: mbFirstConnection is false and its parent is keyframe 1.  Its best covisible is keyframe 2
    now; the parent stays (:409), keyframe 2 gets no child.  Keyframe 1 is updated next and keyframe 0 once more."""
    sc = R.Scene(3)
    _shared(sc, 0, 1, 16)
    _shared(sc, 0, 2, 20)
    _shared(sc, 1, 2, 15)
    G.ChangeParent(sc.kfs[0], sc.kfs[1])
    sc.kfs[0].mbFirstConnection = False
    return sc, [0, 1, 0]


def conn_empty():
    """Null slots, a bad point, a point only the keyframe itself lists: the counter is empty and nothing changes (:363)."""
    sc = R.Scene(2)
    sc.kfs[0].add_slot(None, 0)
    sc.point([(0, 1), (1, 1)]).mbBad = True
    sc.point([(0, 1)])
    return sc, [0]


def _adapter_conn(order):
    return lambda: (A.connections_scene(), list(order))


CONN_CASES = {"adapter_" + k: _adapter_conn(v) for k, v in A.CONNECTION_ORDERS.items()}
CONN_CASES.update({"tied_15_ascending": conn_tied(False), "tied_15_descending": conn_tied(True), "below_th_tie_ascending": conn_below_th(False),
                   "below_th_tie_descending": conn_below_th(True), "same_id_other_object": conn_same_id, "bad_observer": conn_bad_observer,
                   "id0": conn_id0, "second_call": conn_second_call, "empty_counter": conn_empty})
CONN_LINKS = ("second_call",)                                       # scenes whose blob carries parents and first-connection flags
# what the adapter program can take: pointer order is index order there, and its blob has no bad keyframes and no links
CONN_INDEX_ORDER = [n for n in CONN_CASES if not n.endswith("descending") and n != "bad_observer" and n not in CONN_LINKS]


def conn_blob(name):
    sc, order = CONN_CASES[name]()
    return A.graph_blob(sc) + i32(len(order)) + np.array(order, np.int32).tobytes() + trailer(sc, links=name in CONN_LINKS)


def conn_derived(dump, sc, order):
    """mConnectedKeyFrameWeights of the keyframe updated last, as (keyframe, weight) pairs in pointer order: the KFcounter of that call
    (:404), which no later AddConnection has touched."""
    kfs, _, tail = parse_dump(dump, len(sc.kfs), len(sc.points))
    assert len(tail) == 0
    return {"dump": np.asarray(dump, np.int32), "last_connected": np.array(kfs[order[-1]]["connected"], np.int32).reshape(-1, 2)}


def conn_restated(name):
    sc, order = CONN_CASES[name]()
    for k in order:
        G.UpdateConnections(sc.kfs[k])
    return conn_derived(G.dump(sc.kfs, sc.points), sc, order)


def conn_counter(name):
    """covis_restatement.update_connections_counter of the keyframe updated last, as (keyframe, count) pairs in pointer order."""
    sc, order = CONN_CASES[name]()
    index = {kf: k for k, kf in enumerate(sc.kfs)}
    return [[index[o], n] for o, n in sorted(R.update_connections_counter(sc.kfs[order[-1]]).items(), key=lambda it: it[0].addr)]


def parse_dump(dump, n_kf, n_points):
    kfs, pts, at = A.parse_graph(np.asarray(dump, np.int32), n_kf, n_points)
    return kfs, pts, np.asarray(dump[at:], np.int32)


# =====================================================================================================================================
# KeyFrameCulling
# =====================================================================================================================================
def kf_surgery():
    """The tree surgery of KeyFrame.cc:503-561 feeding the next cull.  G = 0 is the grandparent, A = 1 its child, culled first.  A has two
    children: C1 = 2, covisible with G (weight 20), and C2 = 3, covisible with C1 alone: C1 goes to G, then C2 to C1, the new candidate.
    C1 comes later in the same list and is culled too: its children are C2 and D = 4 (D covisible with C2 alone), its parent is G by
    then — C2 falls to G by :554-558, D with it —, and G loses the child C1.  Keyframes 5-7 make A's and C1's points redundant."""
    sc = R.Scene(8)
    C._redundant(sc, 1, [5, 6, 7], 12)
    C._redundant(sc, 2, [5, 6, 7], 12)
    for kf in sc.kfs:
        G.graph_members(kf).mbFirstConnection = False
    for a, b, w in ((2, 0, 20), (3, 2, 17), (4, 3, 16), (1, 0, 30), (1, 2, 25), (1, 3, 18)):
        G.AddConnection(sc.kfs[a], sc.kfs[b], w)
        G.AddConnection(sc.kfs[b], sc.kfs[a], w)
    for child, parent in ((1, 0), (2, 1), (3, 1), (4, 2), (5, 0), (6, 0), (7, 0)):
        G.ChangeParent(sc.kfs[child], sc.kfs[parent])
    return sc, [1, 2]


KF_OWN = {"surgery": kf_surgery}
KF_RUNS = list(C.KF_RUNS) + [(n, 0) for n in KF_OWN]


def kf_scene(name):
    return (KF_OWN[name] if name in KF_OWN else C.KF_CASES[name])()


def kfcull_blob(name, mono):
    sc, local = kf_scene(name)
    return A.graph_blob(sc) + i32(int(mono), len(local)) + np.array(local, np.int32).tobytes() + trailer(sc, links=name in KF_OWN)


def kfcull_derived(dump, erased, sc, local):
    """decision per local keyframe and bad_after per point, read from the graph the call left."""
    kfs, pts, _ = parse_dump(dump, len(sc.kfs), len(sc.points))
    decision = [3 if sc.kfs[k].mnId == 0 else 1 if kfs[k]["bad"] else 2 if kfs[k]["to_be_erased"] else 0 for k in local]
    return {"dump": np.asarray(dump, np.int32), "erased": np.asarray(erased, np.int32), "decision": np.array(decision, np.uint8),
            "bad_after": np.array([p["bad"] for p in pts], np.uint8)}


def kfcull_restated(name, mono):
    sc, local = kf_scene(name)
    anchor = with_anchor(sc)
    erased = []
    out = G.keyframe_culling(sc.kfs, [sc.kfs[k] for k in local], bool(mono), erased)
    facts = kfcull_derived(G.dump(sc.kfs, sc.points, anchor), [sc.kfs.index(kf) for kf in erased], sc, local)
    assert facts["decision"].tolist() == [o[2] for o in out]      # the loop's own record and the graph it left say the same
    return facts


# =====================================================================================================================================
# MapPointCulling
# =====================================================================================================================================
MP_TWICE = 20            # the list of the `twice` entry: these points, then the first ten again
MP_RUNS = [(str(n), m) for n, m in C.MP_RUNS] + [("twice", 0), ("twice", 1)]


def mp_scene(name):
    if name == "twice":
        return A.mpcull_scene(MP_TWICE), list(range(MP_TWICE)) + list(range(10))
    return A.mpcull_scene(int(name)), list(range(int(name)))


def mpcull_blob(name, mono):
    sc, lst = mp_scene(name)
    return b"".join([A.graph_blob(sc), i32(int(mono)), np.array([C.MP_CURRENT], np.int64).tobytes(), i32(len(lst)), np.array(lst, np.int32).tobytes(),
                     trailer(sc)])


def mp_trace(lst, bad_before, bad_after, kept):
    """Per entry of the list as it stood: 0 it stays, 1 it was bad already, 2 it was set bad (statuses 2 and 3 of the restatement leave
    the same trace), 4 it left the list as it is.  A point named twice is told apart by position: the list afterwards is a subsequence."""
    trace, k = [], 0
    gone_bad = set()
    for p in lst:
        if k < len(kept) and kept[k] == p and not bad_after[p]:
            trace.append(0); k += 1
        elif bad_before[p] or p in gone_bad:
            trace.append(1)
        elif bad_after[p]:
            trace.append(2); gone_bad.add(p)
        else:
            trace.append(4)
    assert k == len(kept)
    return np.array(trace, np.uint8)


def mpcull_derived(dump, kept, n_kf, before, lst):
    """`before`: every point's bad flag before the call."""
    _, pts, _ = parse_dump(dump, n_kf, len(before))
    return {"dump": np.asarray(dump, np.int32), "list": np.asarray(kept, np.int32), "trace": mp_trace(lst, before, [p["bad"] for p in pts], list(kept)),
            "bad_after": np.array([p["bad"] for p in pts], np.uint8)}


def mpcull_restated(name, mono):
    sc, lst = mp_scene(name)
    before = [bool(p.mbBad) for p in sc.points]
    status, kept = R.map_point_culling([sc.points[p] for p in lst], C.MP_CURRENT, bool(mono))
    facts = mpcull_derived(G.dump(sc.kfs, sc.points), [p.mnId for p in kept], len(sc.kfs), before, lst)
    want = [{2: 2, 3: 2}.get(s, s) for s in status]
    assert facts["trace"].tolist() == want, (facts["trace"].tolist(), want)
    return facts, status


# =====================================================================================================================================
# UpdateLocalMap
# =====================================================================================================================================
LOCALMAP_KEYS = ("local_kf", "local_points", "reference", "frame_reference", "frame", "kf_marks", "point_marks")


def localmap_blob(name):
    sc = L.CASES[name]()
    tables, call = LR.export_tables(sc), LR.export_call(sc)
    ref = -1 if sc.reference is None else sc.kfs.index(sc.reference)
    return L.adapter_blob(tables, call, sc.frame.mnId, ref)


def localmap_as_facts(g):
    assert g["error"] is None and g["calls"] == 1
    return {"local_kf": np.array(g["local_kf"], np.int32), "local_points": np.array(g["local_points"], np.int32), "reference": np.array([g["reference"]], np.int32),
            "frame_reference": np.array([g["frame_reference"]], np.int32), "frame": np.array(g["frame"], np.int32),
            "kf_marks": np.array(g["kf_marks"], np.int64), "point_marks": np.array(g["point_marks"], np.int64)}


def localmap_restated(name):
    sc = L.CASES[name]()
    return localmap_as_facts(L.graph_after(sc, LR.run(sc)))


def localmap_outputs_differ(got, name, want):
    """The outputs of sivo_localmap_update (localmap_cases.OUTPUTS, from the host program or the device) against the reference's facts:
    the names of what differs.  The reference shows no `voted` and no counts; an empty vote is read from what it leaves: the caller's list
    and the caller's reference keyframe."""
    sc = L.CASES[name]()
    call = LR.export_call(sc)
    held = -1 if sc.reference is None else sc.kfs.index(sc.reference)
    bad = []
    n = got["n_local_points"]
    if np.asarray(got["local_point"][:n]).tolist() != want["local_points"].tolist():
        bad.append("local_point")
    if np.asarray(got["slot_cleared"]).astype(bool).tolist() != (call["frame_point"] != want["frame"]).tolist():
        bad.append("slot_cleared")
    if got["voted"]:
        if np.asarray(got["local_kf"][:got["n_local_kf"]]).tolist() != want["local_kf"].tolist():
            bad.append("local_kf")
    elif want["local_kf"].tolist() != call["prev_local_kf"].tolist():
        bad.append("voted")
    ref = got["ref_kf"] if got["ref_kf"] >= 0 else held
    if int(want["reference"][0]) != ref or int(want["frame_reference"][0]) != (got["ref_kf"] if got["ref_kf"] >= 0 else -1):
        bad.append("ref_kf")
    return bad


# =====================================================================================================================================
# the window of LocalBundleAdjustment
# =====================================================================================================================================
def bawin_scene(group, name):
    return B.CASES[name]() if group == "bawin" else B.adapter_scene(name)


def _stamps_of(sc):
    return (np.array([BW.stamps(kf).mnBALocalForKF for kf in sc.kfs], np.int64), np.array([BW.stamps(kf).mnBAFixedForKF for kf in sc.kfs], np.int64),
            np.array([BW.stamps(p).mnBALocalForKF for p in sc.points], np.int64))


def bawin_blob(group, name):
    sc = bawin_scene(group, name)
    tables, call = LR.export_tables(sc), BW.export_call(sc)
    obs_idx = [idx for p in sc.points for _, idx in p.GetObservations()]
    return (L.tables_blob(tables) + i32(sc.pkf) + L.arr(call["cand_kf"], np.int32) + L.arr(obs_idx, np.int32)
            + b"".join(L.arr(a, np.int64) for a in _stamps_of(sc)))


def bawin_facts(local_kf, fixed_kf, local_point, rows, stamps):
    """rows: per local point its edges as (pose vertex, idx)."""
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows], dtype=np.int64)]).astype(np.int32)
    flat = [e for r in rows for e in r]
    return {"local_kf": np.array(local_kf, np.int32), "fixed_kf": np.array(fixed_kf, np.int32), "local_point": np.array(local_point, np.int32),
            "edge_off": off, "edge_pose": np.array([e[0] for e in flat], np.int32), "edge_idx": np.array([e[1] for e in flat], np.int32),
            "kf_local_stamp": stamps[0], "kf_fixed_stamp": stamps[1], "point_local_stamp": stamps[2]}


def bawin_parse(raw, n_kf, n_points):
    w = np.frombuffer(raw, np.int64)
    n = int(w[0]); poses = w[1:1 + 2 * n].reshape(n, 2); at = 1 + 2 * n
    m = int(w[at]); points = w[at + 1:at + 1 + m]; at += 1 + m
    ne = int(w[at]); edges = w[at + 1:at + 1 + 3 * ne].reshape(ne, 3); at += 1 + 3 * ne
    stamps = (w[at:at + n_kf].copy(), w[at + n_kf:at + 2 * n_kf].copy(), w[at + 2 * n_kf:at + 2 * n_kf + n_points].copy())
    assert at + 2 * n_kf + n_points == len(w)
    fixed = poses[:, 1].astype(bool)
    n_local = int((~fixed).sum())
    assert not fixed[:n_local].any() and fixed[n_local:].all(), "a fixed vertex in front of a free one (no scene has a keyframe of id 0)"
    rows = [[] for _ in range(m)]
    last = 0
    for pt, pose, idx in edges.tolist():                            # the edges come grouped by point, in the points' order
        assert pt >= last
        last = pt
        rows[pt].append((pose, idx))
    return bawin_facts(poses[:n_local, 0], poses[n_local:, 0], points, rows, stamps)


def bawin_restated(group, name):
    sc = bawin_scene(group, name)
    index = {kf: k for k, kf in enumerate(sc.kfs)}
    w = BW.run(sc)
    pose = {id(kf): j for j, kf in enumerate(w.vertices)}
    at = {id(p): j for j, p in enumerate(w.lLocalMapPoints)}
    rows = []
    for pMP, row, stray in zip(w.lLocalMapPoints, w.edges, w.stray):        # one row per point, in the order of its observations
        both = {id(kf): (pose[id(kf)], idx) for kf, idx in row}
        both.update({id(kf): (-2 - at[id(v)], idx) for v, kf, idx in stray})
        rows.append([both[id(kf)] for kf, _ in pMP.GetObservations() if id(kf) in both])
    return bawin_facts([index[kf] for kf in w.lLocalKeyFrames], [index[kf] for kf in w.lFixedKFs], [p.mnId for p in w.lLocalMapPoints], rows, _stamps_of(sc))


def bawin_solvable(want):
    """The reference's window without the edges it ties to a point vertex (edge_pose < 0): what a solver can be handed."""
    keep = want["edge_pose"] >= 0
    per_point = np.add.reduceat(np.concatenate([keep, [False]]).astype(np.int64), want["edge_off"][:-1]) if len(want["edge_off"]) > 1 else np.zeros(0, np.int64)
    per_point[np.diff(want["edge_off"]) == 0] = 0
    return dict(want, edge_off=np.concatenate([[0], np.cumsum(per_point)]).astype(np.int32), edge_pose=want["edge_pose"][keep], edge_idx=want["edge_idx"][keep])


def bawin_outputs_differ(got, want, slots_agree):
    """The outputs of sivo_localmap_ba_window (ba_window_cases.OUTPUTS, from the host program or the device) against the reference's
    facts: the names of what differs.  slots_agree: the scene's observations name the slots that hold the points, so edge_slot is the
    reference's idx wherever it names a slot."""
    want = bawin_solvable(want)
    nl, npt, nf, ne = (int(v) for v in got["counts"])
    bad = []
    if [nl, npt, nf, ne] != [len(want["local_kf"]), len(want["local_point"]), len(want["fixed_kf"]), len(want["edge_pose"])]:
        return ["counts"]
    for k, n in (("local_kf", nl), ("fixed_kf", nf), ("local_point", npt), ("edge_off", npt + 1), ("edge_pose", ne)):
        if np.asarray(got[k][:n]).tolist() != want[k].tolist():
            bad.append(k)
    if slots_agree:
        slot = np.asarray(got["edge_slot"][:ne])
        if (slot[slot >= 0] != want["edge_idx"][slot >= 0]).any():
            bad.append("edge_slot")
    return bad


# =====================================================================================================================================
# the chains: nothing connected by hand
# =====================================================================================================================================
CHAIN_FRAME_ID = 9


def chain_scene(shuffled):
    """12 keyframes of mnId 0 .. 11 along a path and 400 points, nearly all of them seen by four to six consecutive keyframes at nearby levels, so that
    most keyframes are redundant while their neighbours stand.  A few points are bad (some with their lists left), keyframe 5 is bad.
    The frame sees every third point.  Returns (scene, frame slots)."""
    def build():
        rng = np.random.default_rng(41 if shuffled else 40)
        n_kf, n_points = 12, 400
        addr = [int(a) for a in rng.permutation(n_kf) + 700] if shuffled else None
        sc = R.Scene(n_kf, addr=addr, ids=list(range(n_kf)), th_depth=40.0)
        for j in range(n_points):
            span = int(rng.integers(4, 7)) if rng.random() < 0.96 else int(rng.integers(2, 4))
            first = min(j * n_kf // n_points, n_kf - span) if rng.random() < 0.8 else int(rng.integers(0, n_kf - span + 1))
            base = int(rng.integers(0, 4))
            sc.point([(k, base + int(rng.integers(0, 2)), rng.random() < 0.5, float(rng.uniform(1.0, 44.0))) for k in range(first, first + span)])
        for j in rng.choice(n_points, 6, replace=False):
            sc.points[int(j)].SetBadFlag()
        for j in rng.choice(n_points, 6, replace=False):
            sc.points[int(j)].mbBad = True
        for k in range(n_kf):
            sc.kfs[k].add_slot(None, 0)
        sc.kfs[5].mbBad = True
        sc.kfs[8].mbNotErase = True
        return sc, [j if j % 3 == 0 else -1 for j in range(n_points)]
    return build


CHAINS = {"ascending": chain_scene(False), "shuffled": chain_scene(True)}


def chain_blob(name):
    sc, frame = CHAINS[name]()
    return A.graph_blob(sc) + i32(0, CHAIN_FRAME_ID, len(frame)) + np.array(frame, np.int32).tobytes() + trailer(sc)


def chain_as_localmap_scene(sc, frame):
    """The covisibility scene as it stands, as a scene of tests/localmap_restatement.py with the same indices, ids and addresses."""
    out = LR.Scene(len(sc.kfs), addr=[kf.addr for kf in sc.kfs])
    out.points = [LR.MapPoint(i) for i in range(len(sc.points))]
    for kf, new in zip(sc.kfs, out.kfs):
        G.graph_members(kf)
        index = {k: i for i, k in enumerate(sc.kfs)}
        new.mnId, new.mbBad = kf.mnId, kf.mbBad
        new.mvpMapPoints = [None if p is None else out.points[p.mnId] for p in kf.mvpMapPoints]
        new.mvpOrderedConnectedKeyFrames = [out.kfs[index[o]] for o in kf.mvpOrderedConnectedKeyFrames]
        new.mspChildren = {out.kfs[index[c]] for c in kf.mspChildren}
        new.mpParent = None if kf.mpParent is None else out.kfs[index[kf.mpParent]]
    for p, new in zip(sc.points, out.points):
        new.mbBad = p.mbBad
        new.mObservations = {out.kfs[sc.kfs.index(kf)]: idx for kf, idx in p.mObservations.items()}
    out.set_frame([None if j < 0 else out.points[j] for j in frame], mnId=CHAIN_FRAME_ID)
    out.pkf = max(range(len(sc.kfs)), key=lambda k: sc.kfs[k].mnId)
    return out


def chain_window_blob(lsc):
    tables, call = LR.export_tables(lsc), BW.export_call(lsc)
    obs_idx = [idx for p in lsc.points for _, idx in p.GetObservations()]
    return (L.tables_blob(tables) + i32(lsc.pkf) + L.arr(call["cand_kf"], np.int32) + L.arr(obs_idx, np.int32)
            + b"".join(L.arr(a, np.int64) for a in _stamps_of(lsc)) + L.arr([kf.mnId for kf in lsc.kfs], np.int64))


def chain_restated(name):
    """The four steps on the restatements' own object graph; the facts after each, and the blob that asks the reference for the window
    of the last keyframe on the graph the first three steps left."""
    sc, frame = CHAINS[name]()
    for kf in sorted(sc.kfs, key=lambda kf: kf.mnId):
        G.UpdateConnections(kf)
    facts = {"connected.dump": G.dump(sc.kfs, sc.points)}
    current = max(sc.kfs, key=lambda kf: kf.mnId)
    erased = []
    G.keyframe_culling(sc.kfs, list(current.mvpOrderedConnectedKeyFrames), False, erased)
    facts["culled.dump"] = G.dump(sc.kfs, sc.points)
    facts["culled.erased"] = np.array([sc.kfs.index(kf) for kf in erased], np.int32)
    facts.update(chain_flags(facts["culled.dump"], len(sc.kfs), len(sc.points)))
    lsc = chain_as_localmap_scene(sc, frame)
    window_blob = chain_window_blob(lsc)
    t = LR.run(lsc)
    g = L.graph_after(lsc, t)
    facts.update({"localmap." + k: v.astype(np.int32) for k, v in localmap_as_facts(g).items()})
    index = {kf: k for k, kf in enumerate(lsc.kfs)}
    w = BW.run(lsc)
    pose = {id(kf): j for j, kf in enumerate(w.vertices)}
    assert not any(w.stray)
    rows = [[(pose[id(kf)], idx) for kf, idx in row] for row in w.edges]
    win = bawin_facts([index[kf] for kf in w.lLocalKeyFrames], [index[kf] for kf in w.lFixedKFs], [p.mnId for p in w.lLocalMapPoints], rows, _stamps_of(lsc))
    facts.update({"window." + k: v for k, v in win.items()})
    return facts, window_blob, lsc


def chain_flags(dump, n_kf, n_points):
    kfs, pts, _ = parse_dump(dump, n_kf, n_points)
    return {"culled.kf_bad": np.array([k["bad"] for k in kfs], np.uint8), "culled.point_bad": np.array([p["bad"] for p in pts], np.uint8)}


def chain_device_inputs(name):
    """What the device is handed for a chain, from the restatements' graph (which the CPU tests hold equal to the reference's after
    every step): the covisibility tables and the local list before the culling, the local-map tables before it, the row delta that
    carries the culling's changes, and the two calls on the graph after it."""
    import localmap_delta_cases as DC
    sc, frame = CHAINS[name]()
    for kf in sorted(sc.kfs, key=lambda kf: kf.mnId):
        G.UpdateConnections(kf)
    current = max(sc.kfs, key=lambda kf: kf.mnId)
    local = [sc.kfs.index(kf) for kf in current.mvpOrderedConnectedKeyFrames]
    covis = (R.export_table(sc), R.export_local(sc, local))
    before = DC.full(LR.export_tables(chain_as_localmap_scene(sc, frame)))
    G.keyframe_culling(sc.kfs, [sc.kfs[k] for k in local], False)
    lsc = chain_as_localmap_scene(sc, frame)
    after = DC.full(LR.export_tables(lsc))
    T = DC.Touched()
    for p in range(len(after["point_bad"])):
        row = lambda t: t["obs_kf"][t["obs_off"][p]:t["obs_off"][p + 1]].tolist()
        if row(before) != row(after) or before["point_bad"][p] != after["point_bad"][p]:
            T.points.add(p)
    for k in range(after["n_kf"]):
        same = before["kf_bad"][k] == after["kf_bad"][k] and before["parent"][k] == after["parent"][k]
        for off, val in (("slot_off", "slot_point"), ("covis_off", "covis_kf"), ("child_off", "child_kf")):
            same = same and before[val][before[off][k]:before[off][k + 1]].tolist() == after[val][after[off][k]:after[off][k + 1]].tolist()
        if not same:
            T.kfs.add(k)
    delta = DC.make_delta(before, after, T, False)
    update = LR.export_call(lsc)
    update["kf_capacity"], update["point_capacity"] = len(lsc.kfs) + 2, len(lsc.points) + 2
    window = BW.export_call(lsc)
    window.update(B.capacities(after))
    return dict(covis=covis, local=local, before=before, after=after, delta=delta, touched=T, update=update, window=window)


def chain_facts_of(name, raw, window_raw):
    sc, frame = CHAINS[name]()
    w = np.frombuffer(raw, np.int32)
    n = int(w[0]); facts = {"connected.dump": w[1:1 + n].copy()}; at = 1 + n
    n = int(w[at]); facts["culled.dump"] = w[at + 1:at + 1 + n].copy(); at += 1 + n
    n = int(w[at]); facts["culled.erased"] = w[at + 1:at + 1 + n].copy(); at += 1 + n
    facts.update(chain_flags(facts["culled.dump"], len(sc.kfs), len(sc.points)))
    n = int(w[at]); facts["localmap.local_kf"] = w[at + 1:at + 1 + n].copy(); at += 1 + n
    n = int(w[at]); facts["localmap.local_points"] = w[at + 1:at + 1 + n].copy(); at += 1 + n
    facts["localmap.reference"], facts["localmap.frame_reference"] = w[at:at + 1].copy(), w[at + 1:at + 2].copy(); at += 2
    facts["localmap.frame"] = w[at:at + len(frame)].copy(); at += len(frame)
    facts["localmap.kf_marks"] = w[at:at + len(sc.kfs)].copy(); at += len(sc.kfs)
    facts["localmap.point_marks"] = w[at:at + len(sc.points)].copy(); at += len(sc.points)
    assert at == len(w)
    facts.update({"window." + k: v for k, v in bawin_parse(window_raw, len(sc.kfs), len(sc.points)).items()})
    return facts


def chain_live(name, program="ref_mapgraph"):
    """The reference's facts of a chain.  The window is asked of ref_bawindow on the graph the first three steps left; that graph is
    the restatement's, which test_pin_map_graph.py has by then required to equal the reference's dump."""
    _, window_blob, _ = chain_restated(name)
    return chain_facts_of(name, run_reference("chain", chain_blob(name), program), run_reference("window", window_blob, "ref_bawindow"))


# =====================================================================================================================================
# the reference programs, the fixture
# =====================================================================================================================================
ENTRIES = (["conn." + n for n in CONN_CASES] + ["kfcull.%s.%d" % nm for nm in KF_RUNS] + ["mpcull.%s.%d" % nm for nm in MP_RUNS]
           + ["localmap." + n for n in L.CASES] + ["bawin." + n for n in B.CASES] + ["bawin_map." + n for n in B.ADAPTER_CASES]
           + ["chain." + n for n in CHAINS])


def entry_blob(entry):
    group, _, rest = entry.partition(".")
    if group == "conn":
        return "connections", conn_blob(rest)
    if group == "localmap":
        return "localmap", localmap_blob(rest)
    if group == "chain":
        return "chain", chain_blob(rest)
    if group in ("bawin", "bawin_map"):
        return "window", bawin_blob(group, rest)
    name, _, mono = rest.rpartition(".")
    return (group, kfcull_blob(name, int(mono))) if group == "kfcull" else (group, mpcull_blob(name, int(mono)))


@functools.lru_cache(maxsize=None)
def reference_program(name="ref_mapgraph"):
    """oracle/_ref/<name>, (re)built where the reference's sources are; None where neither they nor a built program are."""
    if S.reference_present():
        subprocess.run(["make", "-s", "-C", S.ORACLE, "liboracle.so", "_ref/" + name], check=True)
    exe = os.path.join(S.ORACLE, "_ref", name)
    return exe if os.path.exists(exe) else None


def run_reference(mode, blob, program="ref_mapgraph"):
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(blob)
        r = subprocess.run([reference_program(program), mode, fin, fout], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (mode, r.returncode, r.stderr[-3000:])
        with open(fout, "rb") as f:
            return f.read()


def facts_of(entry, raw):
    """The facts of an entry from the bytes the reference program wrote."""
    group, _, rest = entry.partition(".")
    if group == "localmap":
        sc = L.CASES[rest]()
        return localmap_as_facts(L.parse_adapter(raw, len(sc.frame.mvpMapPoints), len(sc.kfs), len(sc.points)))
    if group in ("bawin", "bawin_map"):
        sc = bawin_scene(group, rest)
        return bawin_parse(raw, len(sc.kfs), len(sc.points))
    w = np.frombuffer(raw, np.int32)
    if group == "conn":
        sc, order = CONN_CASES[rest]()
        return conn_derived(w.copy(), sc, order)
    name, _, mono = rest.rpartition(".")
    sc, what = kf_scene(name) if group == "kfcull" else mp_scene(name)
    _, _, tail = parse_dump(w, len(sc.kfs), len(sc.points))
    assert len(tail) == 1 + tail[0]
    dump = w[:len(w) - len(tail)]
    if group == "kfcull":
        return kfcull_derived(dump, tail[1:], sc, what)
    return mpcull_derived(dump, tail[1:], len(sc.kfs), [bool(p.mbBad) for p in sc.points], what)


def program_of(entry):
    return "ref_bawindow" if entry.startswith("bawin") else "ref_mapgraph"


def live_facts(entry, program=None):
    if entry.startswith("chain."):
        return chain_live(entry[6:], program or "ref_mapgraph")
    mode, blob = entry_blob(entry)
    return facts_of(entry, run_reference(mode, blob, program or program_of(entry)))


def inputs_digest(entry):
    if entry.startswith("chain."):
        return S.sha(np.frombuffer(chain_blob(entry[6:]), np.uint8))
    return S.sha(np.frombuffer(entry_blob(entry)[1], np.uint8))


def reduce_facts(facts):
    out = {}
    for k, v in facts.items():
        v = np.ascontiguousarray(v)
        if k in WHOLE or v.nbytes <= SHA_FROM:
            out[k] = v
        else:
            out[k + ".sha"] = S.sha(v)
    return out


def same_facts(want, got, what, keys=None):
    """want: the reference's facts (live: whole; fixture: reduced).  got: whole.  Byte for byte, the dtype included."""
    for k in (got if keys is None else keys):
        v = np.ascontiguousarray(got[k])
        if k in want:
            w = np.ascontiguousarray(want[k])
            assert v.dtype == w.dtype and v.shape == w.shape and v.tobytes() == w.tobytes(), (what, k, first_difference(v, w))
        else:
            assert S.sha(v).tobytes() == want[k + ".sha"].tobytes(), (what, k)


def first_difference(a, b):
    if a.shape != b.shape:
        return "shapes", a.shape, b.shape
    at = np.flatnonzero(a.ravel() != b.ravel())
    return None if not len(at) else (int(at[0]), a.ravel()[at[0]].item(), b.ravel()[at[0]].item())


def pack_entry(reduced):
    """The reduced facts of an entry as the two members the fixture keeps: `index` (text: key, dtype and shape per fact, in key order)
    and `bytes` (their bytes, one after the other).  Two members an entry keep the archive's own overhead small."""
    keys = sorted(reduced)
    index = ";".join("%s,%s,%s" % (k, reduced[k].dtype.str, "x".join(str(n) for n in reduced[k].shape)) for k in keys)
    return {"index": index, "bytes": np.frombuffer(b"".join(np.ascontiguousarray(reduced[k]).tobytes() for k in keys), np.uint8)}


def unpack_entry(packed):
    out, at, raw = {}, 0, packed["bytes"].tobytes()
    for item in bytes(packed["index"]).decode().split(";"):
        k, dt, shape = item.split(",")
        shape = tuple(int(n) for n in shape.split("x")) if shape else ()
        n = int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize
        out[k] = np.frombuffer(raw, dt, n // np.dtype(dt).itemsize, at).reshape(shape)
        at += n
    assert at == len(raw)
    return out


@functools.lru_cache(maxsize=None)
def load_fixture():
    packed = {}
    with np.load(GOLDEN, allow_pickle=False) as z:
        for member in z.files:
            name, key = member.split("|")
            packed.setdefault(name, {})[key] = z[member]
    return {name: unpack_entry(p) for name, p in packed.items()}


@functools.lru_cache(maxsize=None)
def reference_facts(entry):
    """(facts, live) of one entry: from the reference program where it is, else the fixture."""
    if reference_program(program_of(entry)):
        return live_facts(entry), True
    return recorded_facts(entry), False


@functools.lru_cache(maxsize=None)
def recorded_facts(entry):
    fx = load_fixture()[entry]
    assert fx["inputs"].tobytes() == inputs_digest(entry).tobytes(), "the scene generator drifted from the recorded fixture: " + entry
    return fx
