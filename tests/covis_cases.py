"""The scenes of the covisibility tests, hand-made and seeded, and what runs them: the restatement (tests/covis_restatement.py, the
yardstick), the host build of the kernels' arithmetic (tests/covis_prog.cpp) and the blobs both programs read.  A scene is built afresh
for every run: the restatement mutates its graph."""
import functools

import numpy as np

import covis_restatement as R
import host_prog

LDS_KF = 8192                                                       # SIVO_COVIS_LDS_KF of include/sivo_hip.h
SENTINEL = R.SENTINEL
run_prog = host_prog.run                                            # (the tests' assertions call it by this name)


# ---- blobs ---------------------------------------------------------------------------------------------------------------------------
def i32(*v):
    return np.array(v, np.int32).tobytes()


def table_blob(t):
    return b"".join([i32(t["n_kf"], len(t["point_bad"])), np.array([len(t["obs_kf"])], np.int64).tobytes(), t["obs_off"].tobytes(),
                     t["obs_kf"].tobytes(), t["obs_level"].tobytes(), t["obs_stereo"].tobytes(), t["point_bad"].tobytes()])


def csr(lists, dt):
    off = np.zeros(len(lists) + 1, np.int64)
    if len(lists):
        off[1:] = np.cumsum([len(s) for s in lists])
    flat = np.concatenate([np.asarray(s, dt) for s in lists]).astype(dt) if len(lists) else np.zeros(0, dt)
    return off, flat


def count_blob(t, sets, selfs):
    off, pts = csr(sets, np.int32)
    return table_blob(t) + i32(len(sets)) + off.tobytes() + pts.tobytes() + np.asarray(selfs, np.int32).tobytes()


def kfcull_blob(t, local, monocular):
    off, pts = csr([k["point"] for k in local], np.int32)
    _, lvl = csr([k["level"] for k in local], np.uint8)
    _, dep = csr([k["depth"] for k in local], np.float32)
    return b"".join([table_blob(t), i32(len(local), int(monocular)), np.array([k["kf"] for k in local], np.int32).tobytes(),
                     np.array([k["is_id0"] for k in local], np.uint8).tobytes(), np.array([k["erasable"] for k in local], np.uint8).tobytes(),
                     np.array([k["th_depth"] for k in local], np.float32).tobytes(), off.tobytes(), pts.tobytes(), lvl.tobytes(), dep.tobytes()])


def mpcull_blob(a, current, monocular):
    return b"".join([i32(len(a["found"]), int(monocular)), np.array([current], np.int64).tobytes(), a["found"].tobytes(), a["visible"].tobytes(),
                     a["first_kf_id"].tobytes(), a["n_obs"].tobytes(), a["bad"].tobytes()])


# ---- host build ----------------------------------------------------------------------------------------------------------------------
def host_count(exe, tmp_path, t, sets, selfs):
    raw = host_prog.run(exe, tmp_path, "count", count_blob(t, sets, selfs))
    rc = int(np.frombuffer(raw, np.int32, 1)[0])
    return rc, np.frombuffer(raw, np.int32, len(sets) * t["n_kf"], 4).reshape(len(sets), t["n_kf"])


def host_kfcull(exe, tmp_path, t, local, monocular):
    raw = host_prog.run(exe, tmp_path, "kfcull", kfcull_blob(t, local, monocular))
    K, P = len(local), len(t["point_bad"])
    assert len(raw) == 4 + 9 * K + P
    return dict(rc=int(np.frombuffer(raw, np.int32, 1)[0]), n_mps=np.frombuffer(raw, np.int32, K, 4), n_redundant=np.frombuffer(raw, np.int32, K, 4 + 4 * K),
                decision=np.frombuffer(raw, np.uint8, K, 4 + 8 * K), bad_after=np.frombuffer(raw, np.uint8, P, 4 + 9 * K))


def host_mpcull(exe, tmp_path, a, current, monocular):
    raw = host_prog.run(exe, tmp_path, "mpcull", mpcull_blob(a, current, monocular))
    return int(np.frombuffer(raw, np.int32, 1)[0]), np.frombuffer(raw, np.uint8, len(a["found"]), 4)


# =====================================================================================================================================
# Counts: a case is (scene, sets); a set is ("kf", index) — KeyFrame::UpdateConnections of that keyframe — or ("frame", Frame) — the vote
# =====================================================================================================================================
def _fill_keyframe(sc, rng, k, n_slots, n_kf, pool):
    """n_slots slots for keyframe k: new points it observes with a few other keyframes, null slots, points that do not list k (self absent
    from the list), bad points, and earlier points again in a second slot."""
    kf = sc.kfs[k]
    mine = []
    while len(kf.mvpMapPoints) < n_slots:
        r = rng.random()
        if r < 0.1:
            kf.add_slot(None, 0)
        elif r < 0.2 and mine:
            kf.add_slot(mine[rng.integers(len(mine))], int(rng.integers(0, 8)))                      # a point in two slots
        elif r < 0.3 and n_kf > 1:
            others = [int(o) for o in rng.choice(pool, min(len(pool), 3), replace=False) if o != k]
            p = sc.point([(o, int(rng.integers(0, 8))) for o in others])
            kf.add_slot(p, int(rng.integers(0, 8)))                                                  # k holds it, the point does not list k
        else:
            others = [int(o) for o in rng.choice(pool, min(len(pool), int(rng.integers(1, 7))), replace=False) if o != k]
            idx = kf.add_slot(None, int(rng.integers(0, 8)), 5.0 if rng.random() < 0.5 else -1.0)
            p = sc.point([(o, int(rng.integers(0, 8))) for o in others])
            kf.mvpMapPoints[idx] = p
            p.AddObservation(kf, idx)
            mine.append(p)
            if rng.random() < 0.1:
                p.mbBad = True                                                                        # bad, its list still in the table
            elif rng.random() < 0.05:
                p.SetBadFlag()


def _frame(sc, rng, n_slots):
    slots = []
    for _ in range(n_slots):
        r = rng.random()
        if r < 0.15 or not sc.points:
            slots.append(None)
        elif r < 0.2:
            sc.points.append(R.MapPoint(len(sc.points)))                                              # a point without observations
            slots.append(sc.points[-1])
        else:
            slots.append(sc.points[rng.integers(len(sc.points))])
    return R.Frame(slots)


def _count_random(n_kf, set_sizes, frame_sizes, seed, exact=False):
    """exact: the other observers come from the keyframes that are no set themselves, so every set has exactly the size asked for"""
    def build():
        pool = np.arange(len(set_sizes) if exact else 0, n_kf)
        rng = np.random.default_rng(seed)
        sc = R.Scene(n_kf, addr=[int(a) for a in rng.permutation(n_kf) + 1000])
        for k, n in enumerate(set_sizes):
            _fill_keyframe(sc, rng, k, n, n_kf, pool)
        return sc, [("kf", k) for k in range(len(set_sizes))] + [("frame", _frame(sc, rng, n)) for n in frame_sizes]
    return build


def _count_one_counter():
    """Every slot of a 2049-slot set is observed by keyframe 1: one counter takes them all."""
    sc = R.Scene(2)
    for _ in range(2049):
        sc.point([(0, 0), (1, 0)])
    return sc, [("kf", 0), ("frame", R.Frame(list(sc.points)))]


def _count_bound(n_kf):
    def build():
        sc = R.Scene(n_kf)
        for i in range(6):
            sc.point([(0, 0), (n_kf - 1, 1), (n_kf - 2 - i, 2), (1 + i, 3)])
        sc.points[2].SetBadFlag()
        return sc, [("kf", 0), ("kf", n_kf - 1), ("frame", R.Frame(list(sc.points) + [None, sc.points[0]]))]
    return build


COUNT_CASES = {}
for _n in (1, 2, 63, 64, 65, 1025):
    COUNT_CASES["n_kf_%d" % _n] = _count_random(_n, [40], [30], 10 + _n)
for _n in (LDS_KF - 1, LDS_KF, LDS_KF + 1):
    COUNT_CASES["lds_bound_%d" % _n] = _count_bound(_n)
COUNT_CASES["set_sizes"] = _count_random(20, [0, 1, 63, 64, 65, 2049], [0, 1, 65], 5, exact=True)
COUNT_CASES["three_sets"] = _count_random(12, [7, 300, 41], [], 6, exact=True)
COUNT_CASES["one_counter"] = _count_one_counter


def count_arrays(name):
    """table, sets (point indices), selfs of a case, and the restatement's counts as a dense (n_sets, n_kf) array."""
    sc, sets = COUNT_CASES[name]()
    t = R.export_table(sc)
    index = {kf: k for k, kf in enumerate(sc.kfs)}
    slots, selfs, want = [], [], np.zeros((len(sets), len(sc.kfs)), np.int32)
    for s, (kind, what) in enumerate(sets):
        holder = sc.kfs[what] if kind == "kf" else what
        slots.append(R.export_slots(sc, holder.mvpMapPoints))
        selfs.append(what if kind == "kf" else -1)
        counter = R.update_connections_counter(holder) if kind == "kf" else R.vote_local_keyframes(holder)
        for kf, c in counter.items():
            want[s, index[kf]] = c
    return t, slots, np.array(selfs, np.int32), want


# =====================================================================================================================================
# Keyframe culling: a case builds (scene, local keyframe indices); KF_MONO says which run monocular as well
# =====================================================================================================================================
def _redundant(sc, k, helpers, n, level=1, stereo=False, depth=1.0):
    """n points that keyframe k observes together with three helper keyframes at its own level: redundant for k"""
    return [sc.point([(k, level, stereo, depth)] + [(h, level) for h in helpers]) for _ in range(n)]


def kf_nothing_culled():
    sc = R.Scene(4)
    for i in range(12):
        sc.point([(i % 4, 1), ((i + 1) % 4, 1)])
    return sc, [0, 1, 2, 3]


def kf_edge(n_redundant, n_plain):
    def build():
        sc = R.Scene(4)
        _redundant(sc, 0, [1, 2, 3], n_redundant)
        for _ in range(n_plain):
            sc.point([(0, 1), (1, 1)])
        sc.kfs[0].add_slot(None, 0)
        return sc, [0]
    return build


def kf_two_stereo():
    sc = R.Scene(2)
    sc.point([(0, 1, True), (1, 1, True)])
    return sc, [0]


def kf_level_edge():
    sc = R.Scene(4)
    sc.point([(0, 2), (1, 3), (2, 3), (3, 3)])                      # level + 1 three times: redundant
    sc.point([(0, 2), (1, 3), (2, 3), (3, 4)])                      # level + 2 does not count: two observers, not redundant
    return sc, [0]


def kf_chain(not_erasable=False, id0_at=None):
    """Ten points seen by A = 0, B = 1 and two helpers, one observation each: nObs 4, three other observers — redundant for A and for B.
    Culling A leaves them nObs 3: no longer above thObs, B keeps them all."""
    def build():
        n_kf = 5
        ids = [1, 2, 3, 4, 0]
        sc = R.Scene(n_kf, ids=ids)
        for _ in range(10):
            sc.point([(0, 1), (1, 1), (2, 1), (3, 1)])
        _redundant(sc, 4, [0, 2, 3], 5)                            # the keyframe of id 0 would be culled were it not skipped
        sc.kfs[0].mbNotErase = not_erasable
        local = [0, 1]
        if id0_at is not None:
            local.insert(id0_at, 4)
        return sc, local
    return build


def kf_bad_chain():
    """A = 0: 28 redundant points and 3 it shares with B = 1 alone (nObs 2).  B: those 3 and 19 redundant ones: 19 of 22, kept.  Culling A
    leaves the 3 with nObs 1: bad, B is 19 of 19 and goes too."""
    sc = R.Scene(5)
    _redundant(sc, 0, [2, 3, 4], 28)
    for _ in range(3):
        sc.point([(0, 1), (1, 1)])
    _redundant(sc, 1, [2, 3, 4], 19)
    return sc, [0, 1]


def kf_depth():
    """Keyframe 0, th_depth 40: redundant points at depth 41 (left out), 40 (counted), -1 (left out), NaN (counted), 39.5 (counted) and two
    plain points that are not redundant: 3 of 5 with the rule, 5 of 7 monocular."""
    sc = R.Scene(4, th_depth=40.0)
    for d in (41.0, 40.0, -1.0, float("nan"), 39.5):
        _redundant(sc, 0, [1, 2, 3], 1, depth=d)
    for _ in range(2):
        sc.point([(0, 1, False, 10.0), (1, 1)])
    return sc, [0]


def kf_not_listed():
    """Keyframe 0 holds a point in a slot that the point's observations do not name: every observer is another keyframe."""
    sc = R.Scene(5)
    p = sc.point([(1, 1), (2, 1), (3, 1), (4, 1)])
    sc.kfs[0].add_slot(p, 1)
    _redundant(sc, 0, [1, 2, 3], 9)
    return sc, [0, 1]


def kf_slot_counts():
    def build():
        rng = np.random.default_rng(77)
        sizes = [0, 1, 1023, 1024, 1025, 2500]
        sc = R.Scene(len(sizes) + 6)
        for k, n in enumerate(sizes):
            while len(sc.kfs[k].mvpMapPoints) < n:
                if rng.random() < 0.1:
                    sc.kfs[k].add_slot(None, 0)
                else:
                    others = rng.choice(np.arange(len(sizes), len(sizes) + 6), int(rng.integers(1, 6)), replace=False)
                    sc.point([(k, int(rng.integers(0, 4)), rng.random() < 0.5)] + [(int(o), int(rng.integers(0, 5)), rng.random() < 0.5) for o in others])
        return sc, list(range(len(sizes)))
    return build


def kf_culled_2500():
    """A culled keyframe of 2500 slots: 2400 redundant points and, every 25th slot, one it shares with keyframe 1 alone (stereo here, nObs
    3): culling leaves those with nObs 1, bad, in slots of every round of the kernel's 1024 threads over the keyframe."""
    sc = R.Scene(5)
    for i in range(2500):
        if i % 25 == 24:
            sc.point([(0, 1, True), (1, 1)])
        else:
            _redundant(sc, 0, [2, 3, 4], 1)
    _redundant(sc, 1, [2, 3, 4], 30)
    return sc, [0, 1]


def kf_empty_list():
    sc = R.Scene(3)
    _redundant(sc, 0, [1, 2], 4)
    sc.points[1].mbBad = True
    return sc, []


def kf_family(seed, n_kf=40, n_points=3000):
    """Clusters of three to seven keyframes that see nearly the same points at nearly the same levels: every keyframe of a cluster is
    redundant while the others stand, and each one culled leaves the rest less so.  The local list is a shuffle of all keyframes."""
    def build():
        rng = np.random.default_rng(seed)
        sc = R.Scene(n_kf, addr=[int(a) for a in rng.permutation(n_kf) + 500], ids=list(range(n_kf)), th_depth=35.0)      # keyframe 0 has id 0
        clusters, k = [], 0
        while k < n_kf:
            size = min(n_kf - k, int(rng.integers(3, 8)))
            clusters.append(list(range(k, k + size)))
            k += size
        for _ in range(n_points):
            members = clusters[int(rng.integers(len(clusters)))]
            base = int(rng.integers(1, 5))
            seen = [m for m in members if rng.random() < 0.95] or members[:1]
            sc.point([(m, base + int(rng.choice([-1, 0, 0, 0, 0, 1])), rng.random() < 0.4, float(rng.uniform(1.0, 36.0))) for m in seen])
        for k in rng.choice(n_kf, 4, replace=False):
            sc.kfs[int(k)].mbNotErase = True
        for k in range(n_kf):                                       # a null slot and a slot whose point may not list the keyframe
            sc.kfs[k].add_slot(None, 0)
            sc.kfs[k].add_slot(sc.points[int(rng.integers(n_points))], 2, -1.0, 3.0)
        for i in rng.choice(n_points, 30, replace=False):
            sc.points[int(i)].SetBadFlag()
        return sc, [int(k) for k in rng.permutation(n_kf)]
    return build


FAMILY_SEEDS = (1, 2, 3)
KF_CASES = {
    "nothing_culled": kf_nothing_culled,
    "edge_9_of_10": kf_edge(9, 1),
    "edge_10_of_10": kf_edge(10, 0),
    "edge_0_of_0": kf_edge(0, 0),
    "two_stereo": kf_two_stereo,
    "level_edge": kf_level_edge,
    "chain": kf_chain(),
    "bad_chain": kf_bad_chain,
    "id0_first": kf_chain(id0_at=0),
    "id0_middle": kf_chain(id0_at=1),
    "not_erasable": kf_chain(not_erasable=True),
    "depth": kf_depth,
    "not_listed": kf_not_listed,
    "slot_counts": kf_slot_counts(),
    "empty_list": kf_empty_list,
    "culled_2500": kf_culled_2500,
}
for _s in FAMILY_SEEDS:
    KF_CASES["family_%d" % _s] = kf_family(_s)
KF_MONO = ("depth", "slot_counts", "family_1")                      # run with monocular = 1 as well
KF_RUNS = [(n, 0) for n in KF_CASES] + [(n, 1) for n in KF_MONO]


def kf_arrays(name):
    sc, local = KF_CASES[name]()
    return R.export_table(sc), R.export_local(sc, local)


@functools.lru_cache(maxsize=None)
def kf_restatement(name, monocular, removals=True):
    """What the restatement leaves: n_mps, n_redundant, decision per local keyframe, bad_after per point, and the graph for a closer look."""
    sc, local = KF_CASES[name]()
    out = R.keyframe_culling([sc.kfs[k] for k in local], bool(monocular), removals)
    cols = list(zip(*out)) if out else [(), (), ()]
    return dict(n_mps=np.array(cols[0], np.int32), n_redundant=np.array(cols[1], np.int32), decision=np.array(cols[2], np.uint8),
                bad_after=np.array([p.isBad() for p in sc.points], np.uint8), scene=sc, local=local)


# =====================================================================================================================================
# Map-point culling
# =====================================================================================================================================
MP_CURRENT = 10
BIG = 1 << 32                                                       # ids beyond int: both are cast before the subtraction


def mp_points():
    """Every edge once: (found, visible, first_kf_id, n_obs, bad)."""
    rows = [(1, 4, 10, 9, 0),              # ratio exactly 0.25: not below, young: stays
            (249, 1000, 10, 9, 0),         # 0.249: SetBadFlag by ratio
            (0, 0, 10, 9, 0),              # NaN: not below
            (1, 0, 10, 9, 0),              # inf: not below
            (0, 5, 10, 9, 1),              # already bad comes first
            (5, 5, 10, 9, 1)]
    for diff in (1, 2, 3):
        for n_obs in (2, 3, 4):
            rows.append((5, 5, MP_CURRENT - diff, n_obs, 0))
    rows += [(5, 5, MP_CURRENT + 1, 1, 0),                          # a negative difference
             (5, 5, MP_CURRENT - 2 + BIG, 3, 0),                    # the difference is 2 only after the casts
             (5, 5, MP_CURRENT - 3 + BIG, 9, 0)]
    rng = np.random.default_rng(3)
    while len(rows) < 65:
        rows.append((int(rng.integers(0, 8)), int(rng.integers(0, 12)), int(MP_CURRENT - rng.integers(0, 5)), int(rng.integers(0, 6)), int(rng.random() < 0.2)))
    return rows


def mp_objects(n):
    pts = []
    for i, (found, visible, first, n_obs, bad) in enumerate(mp_points()[:n]):
        p = R.MapPoint(i, first_kf_id=first, found=found, visible=visible)
        p.nObs, p.mbBad = n_obs, bool(bad)
        pts.append(p)
    return pts


MP_RUNS = [(n, m) for n in (0, 1, 64, 65) for m in (0, 1)]


def mp_restatement(n, monocular):
    pts = mp_objects(n)
    status, kept = R.map_point_culling(pts, MP_CURRENT, bool(monocular))
    return np.array(status, np.uint8), [p.mnId for p in kept], np.array([p.isBad() for p in pts], np.uint8)
