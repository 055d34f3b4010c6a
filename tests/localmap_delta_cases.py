"""The scenes of the local-map delta tests and what runs them.  A scene is an object graph (tests/localmap_restatement.py) that is exported
as tables, then EDITED as the local mapper edits a map — keyframes and points appended, observation lists, slots, covisibles, children,
parents and flags changed — with every edited object recorded, and exported again.  The delta holds the rows of the recorded objects, taken
from the second export.  Three yardsticks follow: the list-of-rows restatement of apply (tests/localmap_delta_restatement.py) must give the
second export; an update on the applied handle must equal an update on a handle created from those tables; both must equal
Tracking::UpdateLocalMap restated on the edited graph.  Everything is generated from fixed seeds and stays small: the shapes are the
smallest at which a pass can go wrong (tests/test_localmap_delta_host.py says which)."""
import numpy as np

import host_prog
import localmap_cases as P
import localmap_delta_restatement as D
import localmap_restatement as R

TABLES = P.TABLES
FRAME_ID = 9
POINT_ROWS = (("idx", np.int32), ("obs_off", np.int64), ("obs_kf", np.int32), ("bad", np.uint8))
KF_ROWS = (("idx", np.int32), ("bad", np.uint8), ("parent", np.int32), ("slot_off", np.int64), ("slot_point", np.int32), ("covis_off", np.int64),
           ("covis_kf", np.int32), ("child_off", np.int64), ("child_kf", np.int32))


class Touched:
    def __init__(self):
        self.points, self.kfs = set(), set()


# ---- the graph before the edits, and the edits --------------------------------------------------------------------------------------------
def base(rng, n_kf, n_points, perm=False):
    sc = R.Scene(n_kf, addr=(100 + rng.permutation(n_kf)).tolist() if perm else None)
    for _ in range(n_points):
        p = sc.point(sorted(rng.choice(n_kf, int(rng.integers(1, min(5, n_kf) + 1)), replace=False).tolist()))
        p.mbBad = rng.random() < 0.08
    for k, kf in enumerate(sc.kfs):
        for _ in range(3):
            kf.mvpMapPoints.insert(int(rng.integers(0, len(kf.mvpMapPoints) + 1)), None)
        kf.mvpOrderedConnectedKeyFrames = [sc.kfs[c] for c in rng.permutation(n_kf)[:int(rng.integers(0, 13))].tolist() if c != k]
        if k:
            par = int(rng.integers(0, k))
            kf.mpParent = sc.kfs[par]
            sc.kfs[par].mspChildren.add(kf)
        kf.mbBad = rng.random() < 0.1
    return sc


def add_kf(sc, T, rng, addr=None, sees=8):
    """A keyframe appended as ProcessNewKeyFrame leaves it: it observes `sees` old points (their lists grow), lists old covisibles, is the
    child of an old keyframe and the first covisible of one of its neighbours."""
    K = len(sc.kfs)
    kf = R.KeyFrame(K + 1, (max([k.addr for k in sc.kfs] + [99]) + 1) if addr is None else addr)
    sc.kfs.append(kf)
    T.kfs.add(K)
    for p in (rng.choice(len(sc.points), min(sees, len(sc.points)), replace=False).tolist() if sees and sc.points else []):
        sc.points[p].mObservations[kf] = kf.add_slot(sc.points[p])
        T.points.add(p)
    kf.add_slot(None)
    if K:
        cov = rng.choice(K, min(4, K), replace=False).tolist()
        kf.mvpOrderedConnectedKeyFrames = [sc.kfs[c] for c in cov]
        par = int(rng.integers(0, K))
        kf.mpParent = sc.kfs[par]
        sc.kfs[par].mspChildren.add(kf)
        sc.kfs[cov[0]].mvpOrderedConnectedKeyFrames.insert(0, kf)
        T.kfs.update([par, cov[0]])
    return K


def add_point(sc, T, observers, held=True):
    """A point appended as CreateNewMapPoints leaves it; held=False: observed, in no slot (no keyframe row changes)."""
    p = sc.point(sorted(observers), slots=None if held else [])
    T.points.add(p.mnId)
    if held:
        T.kfs.update(observers)
    return p


def set_observers(sc, T, p, observers):
    sc.points[p].mObservations = {sc.kfs[k]: 0 for k in observers}
    T.points.add(p)


def finish(sc, T, rng, n_old, stage2=True, n_frame=14):
    """The scene's frame: the newest points and some old ones, so that the vote runs across old and appended keyframes.  Where keyframe
    rows may change, the frame leaves out the points of one keyframe u, and the first keyframe stage 1 takes, v, gets u in front of its
    covisibility list — a replaced row through which stage 2 reaches a keyframe nobody voted for.  Returns (v, u) as indices, or None
    where the delta may hold no keyframe row."""
    pts = sc.points[-6:] + [sc.points[int(i)] for i in rng.choice(len(sc.points), min(n_frame, len(sc.points)), replace=False)] if sc.points else []
    walk = sorted(sc.kfs, key=lambda kf: kf.addr)
    link = None
    for u in (sorted(walk, key=lambda kf: (sc.kfs.index(kf) >= n_old, -kf.addr)) if stage2 else ()):     # an old keyframe where one will do
        if u.isBad():
            continue
        seen = [p for p in pts if u not in p.mObservations]
        voted = {kf for p in seen if not p.isBad() for kf in p.mObservations}
        v = next((kf for kf in walk if kf in voted and not kf.isBad()), None)
        if v is not None:
            pts = seen
            v.mvpOrderedConnectedKeyFrames = [u] + [c for c in v.mvpOrderedConnectedKeyFrames if c is not u]
            T.kfs.add(sc.kfs.index(v))
            link = (sc.kfs.index(v), sc.kfs.index(u))
            break
    assert link is not None or not stage2
    sc.set_frame([None] + pts + [None], mnId=FRAME_ID)
    return link


# ---- scenes: each returns (scene before the edits as tables, the edited scene, what was touched, whether the delta carries kf_order, meta) --
def _scene(seed, n_kf, n_points, edit, perm=False, give_order=False, stage2=True, prepare=None):
    def build():
        rng = np.random.default_rng(seed)
        sc = base(rng, n_kf, n_points, perm)
        if prepare:
            prepare(sc, rng)
        before = R.export_tables(sc)
        T = Touched()
        edit(sc, T, rng)
        link = finish(sc, T, rng, before["n_kf"], stage2)
        return before, sc, T, give_order, dict(stage2=link)
    build.__doc__ = edit.__doc__
    return build


def empty_delta(sc, T, rng):
    """Nothing changed: no rows, the same sizes, no order."""


def everything_appended(sc, T, rng):
    """A handle created with n_kf = n_points = 0; five keyframes and thirty points appended."""
    for _ in range(5):
        add_kf(sc, T, rng, sees=0)
    for _ in range(30):
        add_point(sc, T, rng.choice(5, int(rng.integers(1, 4)), replace=False).tolist())


def points_only(sc, T, rng):
    """Nine points appended that old keyframes observe and no slot holds: no keyframe row in the delta."""
    for _ in range(9):
        add_point(sc, T, rng.choice(len(sc.kfs), 3, replace=False).tolist(), held=False)


def kfs_only(sc, T, rng):
    """Three keyframes appended that observe nothing: no point row in the delta."""
    for _ in range(3):
        add_kf(sc, T, rng, sees=0)


def first_and_last(sc, T, rng):
    """The first and the last row of every table replaced: point 0 turns bad, the last point gets other observers, keyframe 0's
    covisibles are reversed, the last keyframe gets two more slots and a child."""
    K, Pn = len(sc.kfs), len(sc.points)
    sc.points[0].mbBad = not sc.points[0].mbBad
    T.points.add(0)
    set_observers(sc, T, Pn - 1, [0, K - 1, 2])
    sc.kfs[0].mvpOrderedConnectedKeyFrames.reverse()
    sc.kfs[K - 1].add_slot(sc.points[1]); sc.kfs[K - 1].add_slot(None)
    sc.kfs[K - 1].mspChildren.add(sc.kfs[3])
    T.kfs.update([0, K - 1])


def shrink_and_grow(sc, T, rng):
    """Rows shrunk to length 0 and rows grown, in every table: an observation list emptied and one grown to every keyframe, a keyframe
    without slots and one with twenty more, a covisibility list and a set of children emptied, a set of children grown."""
    set_observers(sc, T, 1, [])
    set_observers(sc, T, 2, range(len(sc.kfs)))
    sc.kfs[1].mvpMapPoints = []
    for i in range(20):
        sc.kfs[2].add_slot(sc.points[i] if i % 3 else None)
    sc.kfs[3].mvpOrderedConnectedKeyFrames = []
    sc.kfs[0].mspChildren = set()
    sc.kfs[4].mspChildren = set(sc.kfs[5:9])
    sc.kfs[5].mpParent = None
    T.kfs.update([0, 1, 2, 3, 4, 5])


def all_rows(sc, T, rng):
    """Every row of every table in the delta, one keyframe and four points appended."""
    k = add_kf(sc, T, rng)
    for _ in range(4):
        add_point(sc, T, [k, int(rng.integers(0, k))])
    for p in range(0, len(sc.points), 3):
        sc.points[p].mObservations.pop(next(iter(sc.points[p].mObservations)), None)
    for kf in sc.kfs[::2]:
        kf.mvpOrderedConnectedKeyFrames = kf.mvpOrderedConnectedKeyFrames[::-1]
    T.points.update(range(len(sc.points)))
    T.kfs.update(range(len(sc.kfs)))


def insertion(sc, T, rng):
    """A keyframe inserted with seven new points, ten old points touched: the point count after the edits is the scene's size (255, 256,
    257: around one block of the scan; 600: three blocks, so the sum of the blocks before one is taken)."""
    k = add_kf(sc, T, rng, sees=12)
    for _ in range(7):
        add_point(sc, T, [k] + rng.choice(k, 2, replace=False).tolist())
    for p in rng.choice(len(sc.points) - 7, 10, replace=False).tolist():
        set_observers(sc, T, p, rng.choice(len(sc.kfs), int(rng.integers(0, 6)), replace=False).tolist())
        sc.points[p].mbBad = rng.random() < 0.3


def long_rows(sc, T, rng):
    """Rows of 64, 65 and 130 entries, from the delta and from the old tables beside them: observation lists, slots and children."""
    add_kf(sc, T, rng, sees=20)
    sc.points[6].mObservations.pop(sc.kfs[-1], None)                # point 6, 70 observers long, stays as the old tables have it
    T.points.discard(6)
    for p, n in ((3, 64), (4, 65), (5, 130)):
        set_observers(sc, T, p, rng.choice(len(sc.kfs), n, replace=False).tolist())
    for k, n in ((1, 64), (2, 65), (6, 130)):
        sc.kfs[k].mvpMapPoints = [None if i % 7 == 3 else sc.points[int(rng.integers(len(sc.points)))] for i in range(n)]
        T.kfs.add(k)
    sc.kfs[7].mspChildren = set(sc.kfs[10:75])
    sc.kfs[8].mspChildren = set(sc.kfs[9:139])
    sc.kfs[12].mspChildren = set(sc.kfs[20:84])
    T.kfs.update([7, 8, 12])


def order_given(sc, T, rng):
    """kf_order given and not the identity: the appended keyframe's address lies in the middle of the old ones."""
    add_kf(sc, T, rng, addr=100 + len(sc.kfs) // 2 + 0.5)
    add_point(sc, T, [len(sc.kfs) - 1, 0])


def order_null_on_permuted(sc, T, rng):
    """kf_order NULL on a handle created with an order that is not the identity: the stored order, then the appended keyframes."""
    k = add_kf(sc, T, rng)
    add_kf(sc, T, rng)
    add_point(sc, T, [k, k + 1, 1])


def long_rows_before(sc, rng):
    """The old tables carry rows over 64 entries too, and the delta leaves them alone: they are copied from the old pool."""
    sc.kfs[9].mvpMapPoints = [None if i % 5 == 1 else sc.points[i % len(sc.points)] for i in range(100)]
    sc.points[6].mObservations = {sc.kfs[k]: 0 for k in range(20, 90)}
    sc.kfs[11].mspChildren = set(sc.kfs[30:96])


CASES = {
    "empty_delta": _scene(11, 8, 30, empty_delta, stage2=False),
    "everything_appended": _scene(12, 0, 0, everything_appended),
    "points_only": _scene(13, 8, 30, points_only, stage2=False),
    "kfs_only": _scene(14, 8, 30, kfs_only),
    "first_and_last": _scene(15, 10, 40, first_and_last),
    "shrink_and_grow": _scene(16, 10, 40, shrink_and_grow),
    "all_rows": _scene(17, 9, 35, all_rows),
    "points_255": _scene(18, 12, 248, insertion), "points_256": _scene(19, 12, 249, insertion), "points_257": _scene(20, 12, 250, insertion),
    "points_600": _scene(21, 14, 593, insertion),
    "long_rows": _scene(22, 140, 60, long_rows, prepare=long_rows_before),
    "order_given": _scene(23, 9, 30, order_given, perm=True, give_order=True),
    "order_null_on_permuted": _scene(24, 9, 30, order_null_on_permuted, perm=True),
}


def rows(off, val, idx, dt=np.int32):
    return R.csr([val[int(off[i]):int(off[i + 1])].tolist() for i in idx], dt)


def make_delta(before, after, T, give_order):
    """The rows of the touched and of the appended objects, out of the tables of the edited graph."""
    K0, P0, K1, P1 = before["n_kf"], len(before["point_bad"]), after["n_kf"], len(after["point_bad"])
    pi = sorted(set(T.points) | set(range(P0, P1)))
    ki = sorted(set(T.kfs) | set(range(K0, K1)))
    pr = dict(idx=np.array(pi, np.int32), bad=after["point_bad"][pi].astype(np.uint8))
    pr["obs_off"], pr["obs_kf"] = rows(after["obs_off"], after["obs_kf"], pi)
    kr = dict(idx=np.array(ki, np.int32), bad=after["kf_bad"][ki].astype(np.uint8), parent=after["parent"][ki].astype(np.int32))
    for name, inner in (("slot", "slot_point"), ("covis", "covis_kf"), ("child", "child_kf")):
        kr[name + "_off"], kr[inner] = rows(after[name + "_off"], after[inner], ki)
    return dict(n_kf=K1, n_points=P1, point_rows=pr, kf_rows=kr, kf_order=D.full_order(after) if give_order else None)


def full(t):
    return dict(t, kf_order=D.full_order(t))


_cache = {}


def arrays(name, slack=2):
    """(tables before, delta, tables after, call, want, meta) of a scene: `after` is the list-of-rows restatement's result, checked here
    against the export of the edited graph; `want` is Tracking::UpdateLocalMap restated on the edited graph.  Computed once per scene and
    shared: nobody changes the arrays."""
    if name not in _cache:
        before, sc, T, give_order, meta = CASES[name]()
        exported = full(R.export_tables(sc))
        delta = make_delta(before, exported, T, give_order)
        after = D.apply(before, delta)
        assert differing(after, exported) == [], (name, differing(after, exported))
        call = R.export_call(sc)
        t = R.run(sc)
        call["kf_capacity"], call["point_capacity"] = len(sc.kfs) + slack, len(sc.points) + slack
        want = R.export_result(sc, call, t, call["kf_capacity"], call["point_capacity"])
        _cache[name] = (before, delta, after, call, want, meta)
    return _cache[name]


def differing(a, b):
    """The tables of a and b that are not equal byte for byte (kf_order compared as stored)."""
    a, b = full(a), full(b)
    out = [] if a["n_kf"] == b["n_kf"] else ["n_kf"]
    return out + [f for f in TABLES if np.asarray(a[f], P._DT[f]).tobytes() != np.asarray(b[f], P._DT[f]).tobytes()]


# ---- blobs (tests/localmap_delta_prog.cpp) ---------------------------------------------------------------------------------------------------
def delta_blob(d, size=0, **counts):
    pr, kr = d["point_rows"], d["kf_rows"]
    n = lambda x: 0 if x is None else len(x)
    head = P.i32(6, size, counts.get("n_kf", d["n_kf"]), counts.get("n_points", d["n_points"]), counts.get("n_point_rows", n(pr["idx"])),
                 counts.get("n_kf_rows", n(kr["idx"])))
    return head + b"".join(P.arr(pr[f], dt) for f, dt in POINT_ROWS) + b"".join(P.arr(kr[f], dt) for f, dt in KF_ROWS) + P.arr(d["kf_order"], np.int32)


def op_apply(d, **kw):
    return ("apply", delta_blob(d, **kw), None)


def op_export():
    return ("export", P.i32(7), None)


def run_ops(exe, tmp_path, ops):
    """The operations through the host program; one dict per operation: rc, message, an update's outputs, an export's sizes and tables."""
    raw = host_prog.run(exe, tmp_path, "run", b"".join(o[1] for o in ops) + P.i32(0))
    at, out = 0, []

    def rc_and_message():
        nonlocal at
        rc = int(np.frombuffer(raw, np.int32, 1, at)[0]); at += 4
        msg = ""
        if rc:
            n = int(np.frombuffer(raw, np.int32, 1, at)[0]); at += 4
            msg = raw[at:at + n].decode(); at += n
        return rc, msg

    for kind, _, sizes in ops:
        rc, msg = rc_and_message()
        res = dict(rc=rc, message=msg)
        if kind == "update":
            S, KC, PC, K = sizes
            res["voted"], res["n_local_kf"], res["ref_kf"], res["n_local_points"] = (int(v) for v in np.frombuffer(raw, np.int32, 4, at)); at += 16
            res["slot_cleared"] = np.frombuffer(raw, np.uint8, S, at); at += S
            for name, n in (("local_kf", KC), ("local_point", PC), ("counts", K)):
                res[name] = np.frombuffer(raw, np.int32, n, at); at += 4 * n
        if kind == "export":
            n = np.frombuffer(raw, np.int64, 6, at).tolist(); at += 48
            res["sizes"] = tuple(n)
            rc2, msg2 = rc_and_message()
            res["rc"], res["message"] = rc or rc2, msg or msg2
            count = dict(obs_off=n[1] + 1, obs_kf=n[2], point_bad=n[1], kf_bad=n[0], slot_off=n[0] + 1, slot_point=n[3], covis_off=n[0] + 1,
                         covis_kf=n[4], child_off=n[0] + 1, child_kf=n[5], parent=n[0], kf_order=n[0])
            t = dict(n_kf=n[0])
            for f in TABLES:
                t[f] = np.frombuffer(raw, P._DT[f], count[f], at); at += t[f].nbytes
            res["tables"] = t
        out.append(res)
    assert at == len(raw), (at, len(raw))
    return out
