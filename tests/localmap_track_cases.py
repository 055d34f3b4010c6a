"""Scenes for sivo_localmap_search_local_points, shared by tests/test_localmap_track_host.py (the host build of the kernels' bodies) and
tests/test_gpu_localmap_track.py (the device): the 620-point local map and the 120-key frame of tests/search_local_cases.py hung on small
keyframe graphs of tests/localmap_restatement.py.  Point p of a graph has row p of the map as its attributes.  What a scene must give is
the COMPOSITION of the two yardsticks: Tracking::UpdateLocalMap restated on the object graph, then the sequential oracle of
SearchByProjection over the points the reference's recorded Frame::isInFrustum has in view and the walk of Tracking.cc:1033-1070 does not
skip.  Reads only tests/golden."""
import numpy as np

import frustum_pin_cases as P
import localmap_cases as LC
import localmap_restatement as R
import search_local_cases as S

F32 = np.float32
ATTRS = ("pos", "normal", "min_dist", "max_dist", "desc", "n_obs")
PER_POINT = ("status", "proj_x", "proj_y", "proj_xr", "view_cos", "level")
STATUS_SENTINEL, MATCH_SENTINEL = 255, -9
_MAP = []


def the_map():
    """search_local_cases.local_map(20, 5) and frame_keys(m, 120, 6), built once and left unchanged."""
    if not _MAP:
        m = S.local_map(20, 5)
        _MAP.append((m, S.frame_keys(m, 120, 6)))
    return _MAP[0]


def attrs(m, n_obs=None):
    return dict(pos=m["pos"], normal=m["normal"], min_dist=m["min_dist"], max_dist=m["max_dist"], desc=m["desc"],
                n_obs=np.asarray(m["obs"] if n_obs is None else n_obs, np.int32))


def _points(sc, n):
    for _ in range(n):
        sc.points.append(R.MapPoint(len(sc.points)))
    return sc.points


def _hold(sc, k, p):
    kf = sc.kfs[k]
    p.mObservations.setdefault(kf, len(kf.mvpMapPoints))
    kf.add_slot(p)


def full_scene(seed=11):
    """Six keyframes (pointer order 3, 0, 5, 1, 4, 2) over all 620 points: every point is held by one to three keyframes in shuffled slot
    order with null slots in between, so local_point is no identity and shared points are met where they come first; a twelfth of the
    points is bad, ten are premarked, keyframe 4 is bad.  The frame's 120 keys: 24 hold points — one of them bad (its slot is cleared), one
    with Observations() == 0 (it does not block its key), one held in two slots; 15 other points are in seen_point."""
    m, fk = the_map()
    rng = np.random.default_rng(seed)
    n = m["n"]
    sc = R.Scene(6, addr=[200, 400, 600, 100, 500, 300])
    pts = _points(sc, n)
    per_kf = [[] for _ in range(6)]
    for p in pts:
        for k in rng.choice(6, int(rng.integers(1, 4)), replace=False):
            per_kf[int(k)].append(p)
    for k, held in enumerate(per_kf):
        for i in rng.permutation(len(held)):
            if rng.random() < 0.05:
                sc.kfs[k].add_slot(None)
            _hold(sc, k, held[int(i)])
    bad = rng.random(n) < 1 / 12
    in_view = np.flatnonzero((P.recorded("probes")["in_view"][m["src"]] != 0) & ~bad)
    out_view = np.flatnonzero((P.recorded("probes")["in_view"][m["src"]] == 0) & ~bad)
    holders = np.concatenate([rng.choice(in_view, 18, replace=False), rng.choice(out_view, 4, replace=False)])
    bad_holder = int(rng.choice(np.flatnonzero(bad)))
    for p in np.flatnonzero(bad):
        pts[int(p)].mbBad = True
    n_obs = m["obs"].copy()
    n_obs[holders[:10]] = np.maximum(n_obs[holders[:10]], 1)
    n_obs[holders[10]] = 0                                          # held, and its key stays open to the search
    keys = rng.choice(120, 24, replace=False)
    slots = [None] * 120
    for key, p in zip(keys[:22], holders):
        slots[int(key)] = pts[int(p)]
    slots[int(keys[22])] = pts[bad_holder]
    slots[int(keys[23])] = pts[int(holders[0])]                     # one point in two slots
    sc.set_frame(slots)
    sc.connect(3, covisibles=[0, 1], children=[5])
    sc.connect(0, covisibles=[3, 2], parent=3)
    sc.connect(5, parent=3)
    sc.connect(1, covisibles=[4, 2])
    sc.kfs[4].mbBad = True
    free = np.setdiff1d(np.arange(n), np.concatenate([holders, [bad_holder]]))
    sc.premark(points=rng.choice(free, 10, replace=False).tolist())
    seen = np.sort(rng.choice(np.intersect1d(free, in_view), 12, replace=False)).astype(np.int32)
    seen = np.concatenate([seen, rng.choice(np.intersect1d(free, out_view), 3, replace=False).astype(np.int32)])
    return dict(sc=sc, n_points=n, n_obs=n_obs, seen=seen, th=3.0, nn_ratio=0.8)


def chain_scene(n_local, prev=False, vote=True):
    """The smallest shape with exactly n_local local points: one keyframe whose slots hold the first n_local points in view (none of them
    bad), a second keyframe with the rest of the map; the frame's key 0 holds the first keyframe's first point (vote) or nothing.  Without
    a vote the points come from prev_local_kf (prev) or there are none."""
    m, fk = the_map()
    iv = np.flatnonzero(P.recorded("probes")["in_view"][m["src"]] != 0)
    order = np.concatenate([iv, np.setdiff1d(np.arange(m["n"]), iv)])
    sc = R.Scene(2)
    pts = _points(sc, m["n"])
    for p in order[:n_local]:
        _hold(sc, 0, pts[int(p)])
    for p in order[n_local:]:
        _hold(sc, 1, pts[int(p)])
    slots = [None] * 120
    if vote and n_local:
        slots[0] = pts[int(order[0])]
    sc.set_frame(slots)
    if prev:
        sc.prev = [sc.kfs[0]]
    return dict(sc=sc, n_points=m["n"], n_obs=m["obs"].copy(), seen=np.zeros(0, np.int32), th=3.0, nn_ratio=0.8)


SCENES = {
    "full": full_scene,
    "one_point": lambda: chain_scene(1), "points_255": lambda: chain_scene(255), "points_256": lambda: chain_scene(256),
    "points_257": lambda: chain_scene(257), "points_600": lambda: chain_scene(600),
    "no_vote_no_prev": lambda: chain_scene(40, vote=False), "no_vote_prev": lambda: chain_scene(40, prev=True, vote=False),
    "no_points": lambda: chain_scene(0),
}


def expected(scene, slack=2):
    """(tables, call, want) of a scene: the tables and the call's arguments before the call, and every output of
    sivo_localmap_search_local_points in sentinel-filled arrays, from the restatement and the oracle.  want["status"] holds
    SIVO_FRUSTUM_SKIPPED, SIVO_FRUSTUM_IN_VIEW and, where the reference says "not in view", -1 (which `return false` it was is the host
    build's to say); the track fields are the REFERENCE's recorded ones for the points in view."""
    m, fk = the_map()
    sc = scene["sc"]
    ref = P.recorded("probes")
    tables, call = R.export_tables(sc), R.export_call(sc)
    fid = sc.frame.mnId
    t = R.run(sc)
    call["kf_capacity"], call["point_capacity"] = len(sc.kfs) + slack, len(sc.points) + slack
    want = R.export_result(sc, call, t, call["kf_capacity"], call["point_capacity"])
    # Tracking.cc:1035-1049: the frame's points that are left are stamped; :1057: and those stamped before the call
    last_seen = np.zeros(len(sc.points), np.int64)
    for p in sc.frame.mvpMapPoints:
        if p is not None:
            last_seen[p.mnId] = fid
    last_seen[scene["seen"]] = fid
    local = np.array([p.mnId for p in t.mvpLocalMapPoints], np.int32)
    skip = last_seen[local] == fid
    assert not any(sc.points[p].isBad() for p in local)
    in_view_all = np.zeros(m["n"], bool)
    in_view_all[local[~skip]] = ref["in_view"][m["src"][local[~skip]]] != 0
    frame_after = np.array([-1 if p is None else p.mnId for p in sc.frame.mvpMapPoints], np.int32)
    occ = np.where(frame_after >= 0, scene["n_obs"][np.maximum(frame_after, 0)], -1).astype(np.int32)
    mm = dict(m, obs=scene["n_obs"])
    nm, match, occ_out = S.oracle_search(fk, mm, in_view_all, scene["th"], scene["nn_ratio"], occ, order=local) if len(local) else (
        0, np.full(120, -1, np.int32), occ)
    pc = call["point_capacity"]
    status = np.full(pc, STATUS_SENTINEL, np.int16)
    status[:len(local)] = np.where(skip, 6, np.where(in_view_all[local], 0, -1))
    want.update(status=status, match=np.asarray(match, np.int32), n_matches=int(nm), n_to_match=int(in_view_all[local].sum()), skip=skip,
                local=local, occ=occ)
    iv = np.flatnonzero(status[:len(local)] == 0)
    src = m["src"][local[iv]]
    for j, k in enumerate(P.TRACK):
        want[k] = np.full(pc, P.SENTINEL, F32)
        want[k][iv] = ref["track"][src, j]
    want["level"] = np.full(pc, P.LEVEL_SENTINEL, np.int32)
    want["level"][iv] = ref["level"][src]
    return tables, call, want


def frustum_record():
    m, _ = the_map()
    return P.frustum_record(m["Tcw"])


def check_against_expected(got, want, what=""):
    """Every output of the call in sentinel-filled arrays against expected(): the update's byte for byte, status where the yardsticks
    decide it, the track fields of the points in view and the sentinels everywhere else, the matches and the counts."""
    bad = LC.same(got, want)
    assert not bad, (what, bad)
    st = np.asarray(got["status"]).astype(np.int16)
    decided = want["status"] >= 0
    assert np.array_equal(st[decided], want["status"][decided]), what
    assert not np.isin(st[~decided], (0, 6, STATUS_SENTINEL)).any(), what
    for k in P.TRACK + ("level",):
        assert np.asarray(got[k]).tobytes() == want[k].tobytes(), (what, k)
    assert np.array_equal(got["match"], want["match"]), what
    assert (int(got["n_to_match"]), int(got["n_matches"])) == (want["n_to_match"], want["n_matches"]), what


# ---- the host program (tests/localmap_track_prog.cpp) ----------------------------------------------------------------------------------
i32, arr = LC.i32, LC.arr
NULL = dict(voted=1, slot_cleared=2, local_kf=4, local_point=8, status=16, match=32, frustum=64, handle=128, frame=256)


def op_set_points(idx, at, n_rows=None, **bent):
    """set_points of the rows `idx` of the attribute arrays `at`; `bent` replaces an array (None: a NULL pointer)."""
    idx = None if idx is None else np.asarray(idx, np.int32)
    rows = {k: None if idx is None else np.ascontiguousarray(at[k][idx]) for k in ATTRS}
    rows.update(bent)
    n = (0 if idx is None else len(idx)) if n_rows is None else n_rows
    return ("set_points", i32(6, n) + arr(idx, np.int32) + b"".join(arr(rows[k], np.uint8 if k == "desc" else np.int32 if k == "n_obs" else F32)
                                                                    for k in ATTRS), None)


def op_get_points(idx, n_rows=None, null_out=False):
    n = (0 if idx is None else len(idx)) if n_rows is None else n_rows
    return ("get_points", i32(7, n, int(null_out)) + arr(idx, np.int32), max(n, 0))


def op_append(n_new):
    return ("append", i32(8, n_new), None)


def op_frame(fk, levels=None):
    levels = len(fk["scale"]) if levels is None else levels
    return ("frame", i32(9) + np.array(P.BOUNDS, F32).tobytes() + np.array([len(fk["keys"])], np.int64).tobytes() + fk["keys"].tobytes()
            + np.ascontiguousarray(fk["u_right"], F32).tobytes() + np.ascontiguousarray(fk["desc"], np.uint8).tobytes() + i32(levels)
            + np.ascontiguousarray(fk["scale"][:levels], F32).tobytes(), None)


def op_device(d):
    return ("device", i32(11, d), None)


def op_search(call, scene, n_kf, n_keys=120, composed=False, null=(), frustum=None, **bent):
    """The call on the scene's arguments; `bent` overrides a count (n_slots, n_seen, ...) or an argument (frame_point, seen_point, ...)."""
    c = dict(call, seen_point=scene["seen"])
    c.update({k: v for k, v in bent.items() if k in c})
    count = lambda k, a: bent.get(k, 0 if c[a] is None else len(c[a]))
    n = [count("n_slots", "frame_point"), count("n_kf_premarked", "kf_premarked"), count("n_point_premarked", "point_premarked"),
         count("n_prev", "prev_local_kf"), count("n_seen", "seen_point")]
    fr = frustum_record() if frustum is None else frustum
    blob = (i32(10) + fr.tobytes() + np.array([bent.get("th", scene["th"]), bent.get("nn_ratio", scene["nn_ratio"])], F32).tobytes()
            + i32(int(composed), *n, c["kf_capacity"], c["point_capacity"], sum(NULL[k] for k in null))
            + b"".join(arr(c[k], np.int32) for k in ("frame_point", "kf_premarked", "point_premarked", "prev_local_kf", "seen_point")))
    return ("search", blob, (max(n[0], 0), max(c["kf_capacity"], 0), max(c["point_capacity"], 0), n_kf, n_keys))


def run_ops(exe, tmp_path, ops):
    """The operations through the host program; one dict per operation that answers: rc, message, and the outputs."""
    import host_prog
    raw = host_prog.run(exe, tmp_path, "run", b"".join(o[1] for o in ops) + i32(0))
    at, out = 0, []

    def take(dt, n):
        nonlocal at
        v = np.frombuffer(raw, dt, n, at)
        at += v.nbytes
        return v

    for kind, _, sizes in ops:
        if kind in ("frame", "device"):
            out.append({})
            continue
        rc = int(take(np.int32, 1)[0])
        res = dict(rc=rc, message="")
        if rc:
            res["message"] = bytes(take(np.uint8, int(take(np.int32, 1)[0]))).decode()
        if kind == "get_points":
            n = sizes
            res.update(pos=take(F32, 3 * n).reshape(n, 3), normal=take(F32, 3 * n).reshape(n, 3), min_dist=take(F32, n), max_dist=take(F32, n),
                       desc=take(np.uint8, 32 * n).reshape(n, 32), n_obs=take(np.int32, n), is_set=take(np.uint8, n))
        if kind == "search":
            S, KC, PC, K, NK = sizes
            for k, v in zip(("voted", "n_local_kf", "ref_kf", "n_local_points", "n_to_match", "n_matches"), take(np.int32, 6)):
                res[k] = int(v)
            res["slot_cleared"] = take(np.uint8, S)
            for name, n in (("local_kf", KC), ("local_point", PC), ("counts", K)):
                res[name] = take(np.int32, n)
            res["status"] = take(np.uint8, PC)
            for k in P.TRACK:
                res[k] = take(F32, PC)
            res["level"], res["match"] = take(np.int32, PC), take(np.int32, NK)
        out.append(res)
    assert at == len(raw), (at, len(raw))
    return out


SEARCH_OUT = ("voted", "n_local_kf", "ref_kf", "n_local_points", "n_to_match", "n_matches", "slot_cleared", "local_kf", "local_point", "counts",
              "status", "level", "match") + P.TRACK


def same_bytes(a, b, what=""):
    for k in SEARCH_OUT:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k)


# ---- the adapter program (tests/localmap_track_adapter_prog.cpp) -----------------------------------------------------------------------
def adapter_script(scene, want):
    """Three frames on the full scene.  The first is the scene's own.  The second carries the points the first ended with in its even
    keys, holds two fresh points and nothing else in the odd ones, finds four more points already seen, two points bad and three points
    in view moved behind the camera.  The third carries everything over and finds one of the moved points back in place."""
    m, _ = the_map()
    local = want["local"]
    in_view = local[want["status"][:len(local)] == 0]
    matched = local[want["match"][want["match"] >= 0]]
    rest = np.setdiff1d(in_view, matched)
    moved = np.array([matched[1], matched[5], rest[0]], np.int32)
    behind = m["pos"][moved].copy()
    behind[:, 2] = -np.abs(behind[:, 2]) - 5
    slots2 = np.where(np.arange(120) % 2 == 0, -2, -1).astype(np.int32)
    slots2[[11, 35]] = rest[[3, 4]]
    return [dict(id=7, slot=want_frame(scene), seen=scene["seen"], bad=[], moved=[], to=np.zeros((0, 3), F32)),
            dict(id=8, slot=slots2, seen=rest[5:9], bad=[matched[2], rest[9]], moved=moved, to=behind),
            dict(id=9, slot=np.full(120, -2, np.int32), seen=[], bad=[], moved=moved[:1], to=m["pos"][moved[:1]])]


def want_frame(scene):
    return np.array([-1 if p is None else p.mnId for p in scene["sc"].frame.mvpMapPoints], np.int32)


def adapter_blob(tables, call, scene, script, touch_geometry=True):
    m, fk = the_map()
    at = attrs(m, scene["n_obs"])
    blob = [i32(int(touch_geometry)), LC.tables_blob(tables)]
    blob += [np.ascontiguousarray(at[k]).tobytes() for k in ("pos", "normal", "min_dist", "max_dist", "n_obs", "desc")]
    blob += [frustum_record().tobytes(), np.array([scene["th"], scene["nn_ratio"]], F32).tobytes(), np.array([len(fk["keys"])], np.int64).tobytes(),
             fk["keys"].tobytes(), np.ascontiguousarray(fk["u_right"], F32).tobytes(), np.ascontiguousarray(fk["desc"], np.uint8).tobytes(), np.array([script[0]["id"]], np.int64).tobytes(),
             arr(call["kf_premarked"], np.int32), arr(call["point_premarked"], np.int32), i32(len(script))]
    for st in script:
        blob += [np.array([st["id"]], np.int64).tobytes()] + [arr(np.asarray(st[k], np.int32), np.int32) for k in ("slot", "seen", "bad", "moved")]
        blob += [np.ascontiguousarray(st["to"], F32).tobytes()]
    return b"".join(blob)


POINT_DUMP = np.dtype([("visible", np.int32), ("last_seen", np.int64), ("track_ref", np.int64), ("in_view", np.int32), ("track", F32, 4),
                       ("level", np.int32)], align=False)


def parse_adapter(raw, steps, n_kf, n_points, n_keys=120):
    """Per step a pair (A, B) of dicts: the counters, and `state`, the bytes of everything else the copy holds."""
    at, out = 0, []
    for _ in range(steps):
        pair = []
        for _ in range(2):
            start = at
            head = np.frombuffer(raw, np.int32, 6, at); at += 24
            slots = np.frombuffer(raw, np.int32, n_keys, at); at += 4 * n_keys
            nk = int(np.frombuffer(raw, np.int32, 1, at)[0]); at += 4
            local_kf = np.frombuffer(raw, np.int32, nk, at); at += 4 * nk
            npt = int(np.frombuffer(raw, np.int32, 1, at)[0]); at += 4
            local_points = np.frombuffer(raw, np.int32, npt, at); at += 4 * npt
            kf_marks = np.frombuffer(raw, np.int64, n_kf, at); at += 8 * n_kf
            points = np.frombuffer(raw, POINT_DUMP, n_points, at); at += POINT_DUMP.itemsize * n_points
            pair.append(dict(ret=int(head[0]), n_to_match=int(head[1]), updates=int(head[2]), searches=int(head[3]), reference=int(head[4]),
                             frame_reference=int(head[5]), slots=slots, local_kf=local_kf, local_points=local_points, kf_marks=kf_marks,
                             points=points, state=raw[start:start + 8] + raw[start + 16:at]))
        out.append(pair)
    assert at == len(raw), (at, len(raw))
    return out
