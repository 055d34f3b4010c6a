"""The scenes of the local-map tests, hand-made and small, and what runs them: the restatement (tests/localmap_restatement.py, the yardstick),
the host build of the kernels' arithmetic (tests/localmap_prog.cpp) and the blobs it reads.  A scene is built afresh for every run: the
restatement mutates its graph.  Every scene stays under a few thousand slots."""
import numpy as np

import host_prog
import localmap_restatement as R

LDS_KF = 8192                                                       # SIVO_COVIS_LDS_KF of include/sivo_hip.h
SENTINEL = R.SENTINEL
TABLES = ("obs_off", "obs_kf", "point_bad", "kf_bad", "slot_off", "slot_point", "covis_off", "covis_kf", "child_off", "child_kf", "parent", "kf_order")
OUTPUTS = ("voted", "n_local_kf", "ref_kf", "n_local_points", "slot_cleared", "local_kf", "local_point", "counts")


# ---- scenes --------------------------------------------------------------------------------------------------------------------------
def _vote(sc, counts):
    """Frame slots that give keyframe k counts[k] votes: that many new points observed (and held) by k alone."""
    slots = []
    for k, c in counts.items():
        slots += [sc.point([k]) for _ in range(c)]
    return slots


def three_kfs_all_voted():
    """Three keyframes, all voted, nothing else: the plain case, with a null frame slot."""
    sc = R.Scene(3)
    p = [sc.point([0, 1]), sc.point([1, 2]), sc.point([0, 1, 2]), sc.point([1])]
    sc.set_frame([p[0], p[1], None, p[2], p[3]])
    return sc


def bad_voted_highest():
    """The keyframe with the highest count is bad: skipped, and no part of the maximum."""
    sc = R.Scene(3)
    sc.set_frame(_vote(sc, {0: 2, 1: 5, 2: 3}))
    sc.kfs[1].mbBad = True
    return sc


def tie_order():
    """Two equal maxima; the walk is by address, 1, 3, 2, 0: keyframe 2 is met before keyframe 0."""
    sc = R.Scene(4, addr=[400, 100, 300, 200])
    sc.set_frame(_vote(sc, {0: 3, 2: 3, 1: 1, 3: 2}))
    return sc


def covis_eleventh():
    """Eleven covisibles, the first ten bad (1-5), voted (6, 7) or premarked (8-10); the eleventh is good and must not be taken."""
    sc = R.Scene(12)
    sc.set_frame(_vote(sc, {0: 3, 6: 1, 7: 1}))
    sc.connect(0, covisibles=range(1, 12))
    for k in range(1, 6):
        sc.kfs[k].mbBad = True
    sc.premark(kfs=[8, 9, 10])
    return sc


def bad_child_first():
    """Three children, the first of them bad: the second is taken, the third is not."""
    sc = R.Scene(4)
    sc.set_frame(_vote(sc, {0: 2}))
    sc.connect(0, children=[1, 2, 3])
    sc.kfs[1].mbBad = True
    return sc


def bad_parent_taken():
    """The parent is bad and is taken all the same: its isBad() is not asked; its point is listed too."""
    sc = R.Scene(3)
    sc.set_frame(_vote(sc, {0: 2}))
    sc.connect(0, parent=1)
    sc.kfs[1].mbBad = True
    sc.point([1])                                                   # the bad parent's point is listed too
    return sc


def parent_stops():
    """The parent is added at the second stage-1 keyframe: the third is not extended."""
    sc = R.Scene(8)
    sc.set_frame(_vote(sc, {0: 1, 1: 2, 2: 1}))
    sc.connect(0, covisibles=[3])
    sc.connect(1, covisibles=[5], parent=4)
    sc.connect(2, covisibles=[6], children=[7])
    return sc


def stage2_mark_seen():
    """What stage 2 adds is marked at once: keyframe 2, taken as keyframe 0's covisible, is not taken again as keyframe 1's covisible or
    child; 3 and 4 are."""
    sc = R.Scene(5)
    sc.set_frame(_vote(sc, {0: 1, 1: 1}))
    sc.connect(0, covisibles=[2])
    sc.connect(1, covisibles=[2, 3], children=[2, 4])
    return sc


def _stage1(n):
    sc = R.Scene(n + 5)
    sc.set_frame(_vote(sc, {k: 1 for k in range(n)}))
    return sc


def stage1_80():
    """Exactly 80: not more than 80, so the first keyframe still adds its covisible and its child (82); the second finds 82 > 80."""
    sc = _stage1(80)
    sc.connect(0, covisibles=[80], children=[81])
    sc.connect(1, covisibles=[82], children=[83])
    return sc


def stage1_81():
    """81 voted keyframes are more than 80: stage 2 adds nothing."""
    sc = _stage1(81)
    sc.connect(0, covisibles=[81], children=[82])
    return sc


def stage1_79():
    """79 -> 80 after the first keyframe, which is not more than 80: the second adds three, the parent among them (83)."""
    sc = _stage1(79)
    sc.connect(0, covisibles=[79])
    sc.connect(1, covisibles=[80], children=[81], parent=82)
    sc.connect(2, covisibles=[83])
    return sc


def children_70():
    """70 children, the first 64 bad: the first good one is the 65th, in the second chunk of 64 lanes."""
    sc = R.Scene(72)
    sc.set_frame(_vote(sc, {0: 1}))
    sc.connect(0, children=range(1, 71))
    for k in range(1, 65):
        sc.kfs[k].mbBad = True
    return sc


def empty_vote_prev():
    """Nobody votes: the list the caller holds stays, and the points are built from it."""
    sc = R.Scene(3)
    shared = sc.point([2, 0])
    sc.point([0]); sc.point([2]); sc.point([1])
    sc.kfs[2].add_slot(None)
    sc.kfs[2].add_slot(shared)
    sc.set_frame([None, None, None])
    sc.prev = [sc.kfs[2], sc.kfs[0]]
    sc.reference = sc.kfs[1]
    return sc


def empty_vote_bad_frame_point():
    """The only frame point is bad: cleared, nobody votes, the caller's list is walked; one of its points is premarked."""
    sc = R.Scene(2)
    bad = sc.point([0])
    bad.mbBad = True
    sc.point([0, 1]); sc.point([1])
    sc.set_frame([None, bad])
    sc.premark(points=[2])
    sc.prev = [sc.kfs[1], sc.kfs[0]]
    return sc


def all_voted_bad():
    """Every voted keyframe is bad: voted, an empty list, no reference keyframe, no points; the caller's list is not walked."""
    sc = R.Scene(3)
    sc.set_frame(_vote(sc, {0: 2, 1: 1}))
    sc.kfs[0].mbBad = sc.kfs[1].mbBad = True
    sc.point([2])
    sc.prev = [sc.kfs[2]]
    return sc


def frame_bad_point():
    """A bad point in a frame slot: cleared and not counted, so keyframe 1, which only it lists, gets no vote."""
    sc = R.Scene(2)
    good, bad = sc.point([0]), sc.point([0, 1])
    bad.mbBad = True
    sc.set_frame([bad, good, None, bad])
    return sc


def premarked():
    """Keyframe 1 is premarked: not taken as a covisible; keyframe 3 is premarked and voted: listed by stage 1 all the same.  Point 1 is
    premarked: not listed."""
    sc = R.Scene(5)
    a, b, c = sc.point([0]), sc.point([0, 3]), sc.point([0, 2])
    sc.point([1]); sc.point([2])
    sc.set_frame([a, b])
    sc.connect(0, covisibles=[1, 2])
    sc.premark(kfs=[1, 3], points=[1])
    return sc


def duplicate_points():
    """Points held by several keyframes, and twice by one: listed once, where they are first met."""
    sc = R.Scene(3, addr=[300, 200, 100])
    a = sc.point([2, 0, 1], slots=[0, 0, 1, 2])
    b = sc.point([1, 2])
    c = sc.point([0, 2], slots=[2, 0, 2])
    d = sc.point([1], slots=[1, 1])
    sc.set_frame([a, b, c, d])
    return sc


def _blocks(total):
    """Three voted keyframes whose slots number `total`; the very last slot holds a point met nowhere before, and the slots on both sides
    of every multiple of 256 hold one point (where the slot behind the boundary is the last one, it is the new point: at 257 and at
    3 x 256 + 1 a block of the point passes holds that slot alone; 258 has the pair across 256 and the new point behind it).  Null
    slots, bad points and earlier points again in between."""
    def build():
        sc = R.Scene(3)
        sizes = [total // 3, total // 3, total - 2 * (total // 3)]
        seq = []
        for g in range(total):
            fresh = g == total - 1 or (g + 1) % 256 == 0           # the last slot, and the first of a pair: new, not null, not bad
            if g % 256 == 0 and g and not fresh:
                seq.append(seq[-1])                                 # the pair across the boundary
            elif g % 11 == 3 and not fresh:
                seq.append(None)
            elif g % 7 == 5 and g > 20 and not fresh:
                seq.append(seq[g - 9] if seq[g - 9] is not None else seq[g - 8])   # an earlier point again
            else:
                p = R.MapPoint(len(sc.points))
                sc.points.append(p)
                p.mbBad = g % 13 == 6 and not fresh
                seq.append(p)
        at = 0
        for k, n in enumerate(sizes):
            for p in seq[at:at + n]:
                if p is not None:
                    p.mObservations.setdefault(sc.kfs[k], len(sc.kfs[k].mvpMapPoints))
                sc.kfs[k].add_slot(p)
            at += n
        first_good = lambda k: next(p for p in sc.kfs[k].mvpMapPoints if p is not None and not p.isBad())
        sc.set_frame([first_good(0), first_good(1), first_good(2)])
        return sc
    build.__doc__ = _blocks.__doc__
    return build


def zero_slot_keyframe():
    """Keyframe 1 is voted and holds no slot at all: the slot sequence steps over it."""
    sc = R.Scene(3)
    a = sc.point([0, 1], slots=[0])
    b = sc.point([1, 2], slots=[2])
    sc.point([2])
    sc.set_frame([a, b])
    return sc


def n_kf_1():
    """One keyframe, with a null slot and a point it holds twice."""
    sc = R.Scene(1)
    a, b = sc.point([0]), sc.point([0])
    sc.kfs[0].add_slot(None)
    sc.kfs[0].add_slot(a)
    sc.set_frame([b, None])
    return sc


def lds_plus_1():
    """SIVO_COVIS_LDS_KF + 1 keyframes, a handful of observations: the histogram and the marks leave LDS.  The last keyframe index is
    voted; 7000 is taken as a covisible, 8000 as a child — 7000, which stage 2 marked in global memory an iteration before, stands in front
    of it in the list — and 1 as a parent."""
    n = LDS_KF + 1
    addr = list(range(100, 100 + n))
    addr[5], addr[n - 1] = addr[n - 1], addr[5]                     # the walk meets the last keyframe before 4000
    sc = R.Scene(n, addr=addr)
    sc.set_frame(_vote(sc, {n - 1: 2, 5: 2, 4000: 1}))
    sc.connect(n - 1, covisibles=[5, 7000])
    sc.connect(5, children=[4000, 7000, 8000], parent=1)
    sc.point([7000]); sc.point([8000, 1])
    sc.premark(kfs=[8100])
    return sc


def random_graph(seed=3, n_kf=40, n_slots=60):
    def build():
        rng = np.random.default_rng(seed)
        sc = R.Scene(n_kf, addr=(100 + rng.permutation(n_kf)).tolist())
        for _ in range(n_kf * n_slots // 3):
            obs = rng.choice(n_kf, int(rng.integers(1, 6)), replace=False).tolist()
            p = sc.point(obs)
            p.mbBad = rng.random() < 0.08
        for kf in sc.kfs:                                           # null slots in between, and every keyframe at its size
            slots = kf.mvpMapPoints[:n_slots - 5]
            for _ in range(n_slots - len(slots)):
                slots.insert(int(rng.integers(0, len(slots) + 1)), None)
            kf.mvpMapPoints = slots
        for k in range(n_kf):
            cov = [int(c) for c in rng.permutation(n_kf)[:int(rng.integers(0, 13))] if c != k]
            sc.kfs[k].mvpOrderedConnectedKeyFrames = [sc.kfs[c] for c in cov]
            if k:
                par = int(rng.integers(0, k))
                sc.kfs[k].mpParent = sc.kfs[par]
                sc.kfs[par].mspChildren.add(sc.kfs[k])
            sc.kfs[k].mbBad = rng.random() < 0.15
        held = [p for kf in sc.kfs[:12] for p in kf.mvpMapPoints if p is not None]
        frame = [None if rng.random() < 0.2 else held[int(rng.integers(len(held)))] for _ in range(100)]
        sc.set_frame(frame)
        sc.premark(kfs=rng.choice(n_kf, 3, replace=False).tolist(), points=rng.choice(len(sc.points), 25, replace=False).tolist())
        sc.prev = [sc.kfs[1], sc.kfs[2]]
        return sc
    return build


CASES = {
    "three_kfs_all_voted": three_kfs_all_voted, "bad_voted_highest": bad_voted_highest, "tie_order": tie_order, "covis_eleventh": covis_eleventh,
    "bad_child_first": bad_child_first, "bad_parent_taken": bad_parent_taken, "parent_stops": parent_stops, "stage2_mark_seen": stage2_mark_seen, "stage1_80": stage1_80,
    "stage1_81": stage1_81, "stage1_79": stage1_79, "children_70": children_70, "empty_vote_prev": empty_vote_prev,
    "empty_vote_bad_frame_point": empty_vote_bad_frame_point, "all_voted_bad": all_voted_bad, "frame_bad_point": frame_bad_point,
    "premarked": premarked, "duplicate_points": duplicate_points, "blocks_255": _blocks(255), "blocks_256": _blocks(256),
    "blocks_257": _blocks(257), "blocks_258": _blocks(258), "blocks_769": _blocks(769), "zero_slot_keyframe": zero_slot_keyframe, "n_kf_1": n_kf_1,
    "lds_plus_1": lds_plus_1, "random_40x60": random_graph(),
}


def arrays(name, slack=2):
    """(tables, call, want, tracking) of a scene: the arrays before the call, and what the restatement leaves in sentinel-filled arrays
    `slack` entries longer than the map could fill."""
    sc = CASES[name]()
    tables, call = R.export_tables(sc), R.export_call(sc)
    t = R.run(sc)
    call["kf_capacity"], call["point_capacity"] = len(sc.kfs) + slack, len(sc.points) + slack
    want = R.export_result(sc, call, t, call["kf_capacity"], call["point_capacity"])
    return tables, call, want, t


# ---- blobs ---------------------------------------------------------------------------------------------------------------------------
def i32(*v):
    return np.array(v, np.int32).tobytes()


def arr(x, dt):
    """An array of the program's input: its length and its values; None stands for a NULL pointer."""
    if x is None:
        return np.array([-1], np.int64).tobytes()
    x = np.ascontiguousarray(x, dt).ravel()
    return np.array([len(x)], np.int64).tobytes() + x.tobytes()


_DT = dict(obs_off=np.int64, obs_kf=np.int32, point_bad=np.uint8, kf_bad=np.uint8, slot_off=np.int64, slot_point=np.int32, covis_off=np.int64,
           covis_kf=np.int32, child_off=np.int64, child_kf=np.int32, parent=np.int32, kf_order=np.int32)


def tables_blob(t, n_points=None):
    n_points = len(t["point_bad"]) if n_points is None else n_points
    return i32(t["n_kf"], n_points) + b"".join(arr(t[f], _DT[f]) for f in TABLES)


def op_create(t, **kw):
    return ("create", i32(1) + tables_blob(t, **kw), None)


def op_replace(t, **kw):
    return ("replace", i32(2) + tables_blob(t, **kw), None)


def op_set_bad(points=(), point_values=(), kfs=(), kf_values=(), n_points=None, n_kf=None):
    count = lambda x: 0 if x is None else len(x)
    return ("set_bad", i32(3, count(points) if n_points is None else n_points, count(kfs) if n_kf is None else n_kf) + arr(points, np.int32)
            + arr(point_values, np.uint8) + arr(kfs, np.int32) + arr(kf_values, np.uint8), None)


def op_update(call, n_kf, null_mask=0, **bent):
    """An update of the call's arguments; `bent` overrides a count (n_slots, n_kf_premarked, n_point_premarked, n_prev) or an argument."""
    c = dict(call, **{k: v for k, v in bent.items() if k in call})
    n = [bent.get("n_slots", len(c["frame_point"]) if c["frame_point"] is not None else 0),
         bent.get("n_kf_premarked", len(c["kf_premarked"]) if c["kf_premarked"] is not None else 0),
         bent.get("n_point_premarked", len(c["point_premarked"]) if c["point_premarked"] is not None else 0),
         bent.get("n_prev", len(c["prev_local_kf"]) if c["prev_local_kf"] is not None else 0)]
    blob = i32(4, *n, c["kf_capacity"], c["point_capacity"], null_mask) + b"".join(
        arr(c[k], np.int32) for k in ("frame_point", "kf_premarked", "point_premarked", "prev_local_kf"))
    return ("update", blob, (max(n[0], 0), max(c["kf_capacity"], 0), max(c["point_capacity"], 0), n_kf))


def run_ops(exe, tmp_path, ops):
    """The operations through the host program; one dict per operation: rc, message, and an update's outputs."""
    raw = host_prog.run(exe, tmp_path, "run", b"".join(o[1] for o in ops) + i32(0))
    at, out = 0, []
    for kind, _, sizes in ops:
        rc = int(np.frombuffer(raw, np.int32, 1, at)[0]); at += 4
        res = dict(rc=rc, message="")
        if rc:
            n = int(np.frombuffer(raw, np.int32, 1, at)[0]); at += 4
            res["message"] = raw[at:at + n].decode(); at += n
        if kind == "timed":
            res["median_us"] = float(np.frombuffer(raw, np.float64, 1, at)[0]); at += 8
            res["voted"], res["n_local_kf"], res["ref_kf"], res["n_local_points"] = (int(v) for v in np.frombuffer(raw, np.int32, 4, at)); at += 16
        if kind == "update":
            S, KC, PC, K = sizes
            res["voted"], res["n_local_kf"], res["ref_kf"], res["n_local_points"] = (int(v) for v in np.frombuffer(raw, np.int32, 4, at)); at += 16
            res["slot_cleared"] = np.frombuffer(raw, np.uint8, S, at); at += S
            for name, n in (("local_kf", KC), ("local_point", PC), ("counts", K)):
                res[name] = np.frombuffer(raw, np.int32, n, at); at += 4 * n
        out.append(res)
    assert at == len(raw), (at, len(raw))
    return out


def op_timed(call, n_kf, reps):
    kind, blob, sizes = op_update(call, n_kf)
    return ("timed", i32(5, reps) + blob[4:], None)


def host_update(exe, tmp_path, tables, call):
    return run_ops(exe, tmp_path, [op_create(tables), op_update(call, tables["n_kf"])])[1]


def same(got, want):
    """Every output of an update equals the wanted bytes (slot_cleared holds the program's 255 only where there is no slot)."""
    return [k for k in OUTPUTS if np.asarray(got[k]).tobytes() != np.asarray(want[k], np.asarray(got[k]).dtype).tobytes()]


# ---- the adapter program -------------------------------------------------------------------------------------------------------------
def adapter_blob(tables, call, frame_id, reference=-1, unknown_slot=-1, bad_kfs=(), bad_points=()):
    return tables_blob(tables) + i32(frame_id, reference, unknown_slot) + b"".join(
        arr(x, np.int32) for x in (call["frame_point"], call["kf_premarked"], call["point_premarked"], call["prev_local_kf"], bad_kfs, bad_points))


def parse_adapter(raw, n_slots, n_kf, n_points):
    """What tests/localmap_adapter_prog.cpp wrote: an error text, or the graph after the call."""
    status = int(np.frombuffer(raw, np.int32, 1)[0])
    if status:
        n = int(np.frombuffer(raw, np.int32, 1, 4)[0])
        return dict(error=raw[8:8 + n].decode())
    calls = int(np.frombuffer(raw, np.int64, 1, 4)[0])
    v = np.frombuffer(raw, np.int32, (len(raw) - 12 - 8 * (n_kf + n_points)) // 4, 12).tolist()
    nk = v[0]
    kfs, v = v[1:1 + nk], v[1 + nk:]
    npt = v[0]
    pts, v = v[1:1 + npt], v[1 + npt:]
    assert len(v) == 2 + n_slots
    marks = np.frombuffer(raw, np.int64, n_kf + n_points, len(raw) - 8 * (n_kf + n_points))
    return dict(error=None, calls=calls, local_kf=kfs, local_points=pts, reference=v[0], frame_reference=v[1], frame=v[2:],
                kf_marks=marks[:n_kf].tolist(), point_marks=marks[n_kf:].tolist())


def graph_after(scene, t):
    """The same fields from the restatement's graph after Tracking::UpdateLocalMap."""
    index = {kf: k for k, kf in enumerate(scene.kfs)}
    ref = lambda kf: -1 if kf is None else index[kf]
    return dict(error=None, calls=1, local_kf=[index[kf] for kf in t.mvpLocalKeyFrames], local_points=[p.mnId for p in t.mvpLocalMapPoints],
                reference=ref(t.mpReferenceKF), frame_reference=ref(scene.frame.mpReferenceKF),
                frame=[-1 if p is None else p.mnId for p in scene.frame.mvpMapPoints],
                kf_marks=[kf.mnTrackReferenceForFrame for kf in scene.kfs], point_marks=[p.mnTrackReferenceForFrame for p in scene.points])
