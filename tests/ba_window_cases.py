"""The scenes of the bundle-adjustment window tests, hand-made and as small as the pass they aim at allows, and what runs them: the
restatement (tests/ba_window_restatement.py, the yardstick), the host build of the kernels' arithmetic (tests/ba_window_prog.cpp) and the
blobs it reads.  A scene is built afresh for every run: the restatement stamps its graph.  scene.pkf is the index of pKF."""
import numpy as np

import ba_window_restatement as W
import host_prog
import localmap_cases as LC
import localmap_restatement as R

LDS_KF = LC.LDS_KF
SENTINEL = W.SENTINEL
OUTPUTS = W.OUTPUTS
i32, arr = LC.i32, LC.arr


def _scene(n_kf, pkf=0, covisibles=(), addr=None):
    sc = R.Scene(n_kf, addr=addr)
    sc.pkf = pkf
    sc.connect(pkf, covisibles=covisibles)
    return sc


def _stamp(sc, local=(), fixed=(), points=()):
    """mnBALocalForKF / mnBAFixedForKF of the listed objects already equal pKF's id."""
    ident = sc.kfs[sc.pkf].mnId
    for k in local:
        W.stamps(sc.kfs[k]).mnBALocalForKF = ident
    for k in fixed:
        W.stamps(sc.kfs[k]).mnBAFixedForKF = ident
    for p in points:
        W.stamps(sc.points[p]).mnBALocalForKF = ident


# ---- scenes --------------------------------------------------------------------------------------------------------------------------
def bad_covisible():
    """Covisible 1 is bad: marked local, not listed, never fixed although a local point sees it, its edges gone; keyframe 3, seen only
    through the bad keyframe's own slots, is not reached."""
    sc = _scene(4, covisibles=[1, 2])
    sc.point([0, 1]); sc.point([1, 3]); sc.point([0, 2, 1])
    sc.kfs[1].mbBad = True
    return sc


def bad_observer():
    """Keyframe 2 observes a local point, is not local and is bad: stamped fixed, not listed, no vertex, no edge; 3 is fixed."""
    sc = _scene(4, covisibles=[1])
    sc.point([0, 2, 3]); sc.point([1, 2])
    sc.kfs[2].mbBad = True
    return sc


def bad_pkf():
    """pKF itself is bad: listed all the same (:499 asks nothing) and a vertex, but no edge goes to it (:670)."""
    sc = _scene(3, covisibles=[1])
    sc.point([0, 1]); sc.point([0, 2])
    sc.kfs[0].mbBad = True
    return sc


def bad_point_null_slots():
    """Null slots and a bad point between the good ones; the bad point's observer 2 is not reached."""
    sc = _scene(3, covisibles=[1])
    sc.kfs[0].add_slot(None)
    bad = sc.point([0, 2])
    bad.mbBad = True
    sc.kfs[0].add_slot(None)
    sc.point([0, 1])
    sc.kfs[1].add_slot(None)
    sc.point([1])
    return sc


def point_in_two_local():
    """Points held by both local keyframes, and twice by one: listed once, where first met; one edge per observation."""
    sc = _scene(3, covisibles=[1])
    sc.point([0, 1]); sc.point([1, 0, 2], slots=[1, 0, 2, 1]); sc.point([1])
    return sc


def fixed_order():
    """Fixed keyframes in the order the observations meet them: the rows walk by address (5, 3, then 4), and 3 is met again through
    the second point."""
    sc = _scene(6, covisibles=[1], addr=[100, 101, 102, 140, 150, 130])
    sc.point([0, 3, 5]); sc.point([0, 4, 3]); sc.point([1, 5, 2])
    return sc


def premarked_local_observer():
    """Keyframe 2 is not bad and carries pKF's id in mnBALocalForKF without being a candidate: neither local nor fixed, so it has no
    vertex and its edge is dropped."""
    sc = _scene(4, covisibles=[1])
    sc.point([0, 2, 3]); sc.point([1, 2])
    _stamp(sc, local=[2])
    return sc


def premarked_fixed():
    """Keyframe 2 already carries the id in mnBAFixedForKF: not listed, no vertex, no edge; candidate 1 carries it too and is local
    all the same."""
    sc = _scene(4, covisibles=[1])
    sc.point([0, 2, 3]); sc.point([1, 3])
    _stamp(sc, fixed=[2, 1])
    return sc


def premarked_point():
    """Point 0 already carries the id: not listed, so keyframe 2, which only it leads to, is not fixed."""
    sc = _scene(4, covisibles=[1])
    sc.point([0, 2]); sc.point([0, 1, 3])
    _stamp(sc, points=[0])
    return sc


def premarked_candidate_local():
    """A candidate that is premarked local is a candidate like any other."""
    sc = _scene(3, covisibles=[1])
    sc.point([0, 1, 2])
    _stamp(sc, local=[1, 0])
    return sc


def pkf_alone():
    """pKF without covisibles and without a slot: one vertex, nothing else."""
    return _scene(1)


def pkf_alone_among_others():
    """pKF without covisibles or points in a map that has both."""
    sc = _scene(3, pkf=2)
    sc.point([0, 1])
    return sc


def _slot_blocks(total):
    """The three keyframes of tests/localmap_cases.py whose slots number `total` (a pair of equal points across every multiple of 256,
    a new point in the very last slot, null slots, bad points and repeats in between) as pKF and its two covisibles."""
    def build():
        sc = LC.CASES["blocks_%d" % total]()
        sc.pkf = 0
        sc.connect(0, covisibles=[1, 2])
        return sc
    build.__doc__ = _slot_blocks.__doc__
    return build


def obs_blocks():
    """401 observations in rows of two (one of three), the fixed keyframe in front of pKF (its address is the highest): keyframes 10, 11 and 13 are
    first met at h = 254, 256 and 258 — 11 opens the second block of 256 —, 13 is bad, 14 is met at 255 and again, 12 in the last row."""
    n = 16
    sc = _scene(n, addr=[900] + list(range(101, 100 + n)))
    other = {127: 10, 128: 11, 129: 13, 199: 12}
    for j in range(200):
        sc.point([0, other.get(j, 1 + j % 7)], slots=[0])
    sc.points[127].mObservations[sc.kfs[14]] = 0                    # row 127: 10 (h = 254), 14 (h = 255), pKF (h = 256) ...
    del sc.points[127].mObservations[sc.kfs[0]]                     # ... without pKF, so that row 128 starts at 256
    sc.points[130].mObservations[sc.kfs[14]] = 0
    sc.kfs[13].mbBad = True
    for k in range(1, n):                                           # the observers hold their points, so that every edge has its slot
        for p in sc.points:
            if sc.kfs[k] in p.mObservations:
                p.mObservations[sc.kfs[k]] = sc.kfs[k].add_slot(p)
    return sc


SLOT_ROWS = [(L, hit) for L in (63, 64, 65, 129) for hit in (0, 63, 64, L - 1) if hit < L]


def slot_rows():
    """Observers whose slot rows are 63, 64, 65 and 129 long, the point at 0, 63, 64 and in the last slot; then two hits in one chunk
    of 64, two hits in different chunks, a third chunk's only hit, and no hit at all (a stale observation)."""
    rows = sorted(set(SLOT_ROWS))
    extra = [(130, (3, 9)), (130, (5, 70)), (200, (191,)), (70, ())]
    sc = _scene(1 + len(rows) + len(extra))
    for j, (L, hits) in enumerate([(L, (hit,)) for L, hit in rows] + extra):
        kf = sc.kfs[1 + j]
        p = sc.point([0], slots=[0])
        p.mObservations[kf] = hits[0] if hits else 7
        kf.mvpMapPoints = [p if s in hits else None for s in range(L)]
    return sc


def lds_plus_1():
    """SIVO_COVIS_LDS_KF + 1 keyframes, otherwise tiny: pKF is the last index, a covisible and a bad covisible, a fixed keyframe and a
    premarked one far apart."""
    n = LDS_KF + 1
    sc = _scene(n, pkf=n - 1, covisibles=[5, 8100, 4000])
    sc.kfs[8100].mbBad = True
    sc.point([n - 1, 5, 7000]); sc.point([5, 8000, 1]); sc.point([4000, 8191]); sc.point([8100, 2])
    _stamp(sc, fixed=[8000], local=[8191])
    return sc


def random_graph(seed, pkf):
    def build():
        sc = LC.random_graph(seed)()
        rng = np.random.default_rng(seed + 100)
        sc.pkf = pkf
        sc.kfs[pkf].mvpOrderedConnectedKeyFrames = [sc.kfs[int(c)] for c in rng.permutation(40)[:14] if c != pkf]     # more than the ten the map stores
        ident = sc.kfs[pkf].mnId
        for kf in sc.kfs:                                           # arbitrary stamps: other keyframes' ids, and now and then this one's
            W.stamps(kf).mnBALocalForKF = ident if rng.random() < 0.08 else int(rng.integers(0, 60))
            kf.mnBAFixedForKF = ident if rng.random() < 0.08 else int(rng.integers(0, 60))
        for p in sc.points:
            W.stamps(p).mnBALocalForKF = ident if rng.random() < 0.05 else int(rng.integers(0, 60))
        for p in sc.points[::17]:                                   # some stale observations, and a point in two slots of a keyframe
            kf = next(iter(p.mObservations))
            kf.mvpMapPoints = [None if q is p else q for q in kf.mvpMapPoints]
        for p in sc.points[5::23]:
            next(iter(p.mObservations)).mvpMapPoints[1] = p
        return sc
    return build


CASES = {
    "bad_covisible": bad_covisible, "bad_observer": bad_observer, "bad_pkf": bad_pkf, "bad_point_null_slots": bad_point_null_slots,
    "point_in_two_local": point_in_two_local, "fixed_order": fixed_order, "premarked_local_observer": premarked_local_observer,
    "premarked_fixed": premarked_fixed, "premarked_point": premarked_point, "premarked_candidate_local": premarked_candidate_local,
    "pkf_alone": pkf_alone, "pkf_alone_among_others": pkf_alone_among_others, "slots_255": _slot_blocks(255), "slots_256": _slot_blocks(256),
    "slots_257": _slot_blocks(257), "obs_blocks": obs_blocks, "slot_rows": slot_rows, "lds_plus_1": lds_plus_1,
    "random_a": random_graph(3, 4), "random_b": random_graph(11, 17),
}


def capacities(tables, slack=2):
    """What no result can exceed, and `slack` entries more: the sentinels behind the counts show what the call left alone."""
    n_slot, n_obs, P = int(tables["slot_off"][-1]), int(tables["obs_off"][-1]) if len(tables["obs_off"]) else 0, len(tables["point_bad"])
    return dict(kf_capacity=tables["n_kf"] + slack, point_capacity=min(P, n_slot) + slack, edge_capacity=n_obs + slack)


_cache = {}


def arrays(name):
    """(tables, call, want) of a scene: the arrays before the call and what the restatement leaves in sentinel-filled arrays.  Computed
    once per process and shared: nobody writes into them."""
    if name not in _cache:
        sc = CASES[name]()
        tables, call = R.export_tables(sc), W.export_call(sc)
        call.update(capacities(tables))
        w = W.run(sc)
        want = W.export_result(sc, w, call["kf_capacity"], call["point_capacity"], call["edge_capacity"])
        for a in (*tables.values(), *call.values(), *want.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[name] = (tables, call, want)
    return _cache[name]


def same(got, want):
    """The outputs that differ from the wanted bytes."""
    return [k for k in OUTPUTS if np.asarray(got[k]).tobytes() != np.asarray(want[k], np.asarray(got[k]).dtype).tobytes()]


INTR = (500.0, 500.0, 320.0, 240.0, 40.0)                           # fx, fy, cx, cy, bf


def solver_arrays(res):
    """(poses, fixed, points, edges, intr) for sivo_amd.optimizer.local_ba, made from a window (the outputs of the call or of the
    restatement): poses and points are functions of the indices alone, one monocular observation per edge — the projection, moved by
    what the edge's slot says."""
    from sivo_amd.optimizer import EDGE_DTYPE
    nl, npt, nf, ne = (int(v) for v in res["counts"])
    kfs = np.concatenate([res["local_kf"][:nl], res["fixed_kf"][:nf]]).astype(np.int64)
    pts = np.asarray(res["local_point"][:npt], np.int64)
    poses = np.zeros((len(kfs), 12))
    poses[:, [0, 4, 8]] = 1.0
    poses[:, 9] = 0.05 * (kfs % 11) - 0.25
    poses[:, 10] = 0.03 * (kfs % 7) - 0.1
    fixed = np.concatenate([np.zeros(nl, np.uint8), np.ones(nf, np.uint8)])
    xyz = np.stack([0.4 * (pts % 13) - 2.4, 0.3 * (pts % 9) - 1.2, 6.0 + 0.5 * (pts % 5)], 1).astype(np.float64)
    edges = np.zeros(ne, EDGE_DTYPE)
    edges["pose"] = res["edge_pose"][:ne]
    edges["point"] = np.repeat(np.arange(npt), np.diff(res["edge_off"][:npt + 1]))
    slot = np.asarray(res["edge_slot"][:ne], np.int64)
    cam = xyz[edges["point"]] + poses[edges["pose"], 9:12]
    edges["obs"][:, 0] = INTR[0] * cam[:, 0] / cam[:, 2] + INTR[2] + 0.25 * (slot % 5 - 2)
    edges["obs"][:, 1] = INTR[1] * cam[:, 1] / cam[:, 2] + INTR[3] + 0.25 * (slot % 3 - 1)
    edges["inv_sigma2"] = 1.0
    return poses, fixed, xyz, edges, INTR


# ---- blobs (the formats of tests/ba_window_prog.cpp; create and set_bad are those of tests/localmap_prog.cpp) --------------------------
op_create, op_set_bad = LC.op_create, LC.op_set_bad
NULLABLE = ("local_kf", "fixed_kf", "local_point", "edge_off", "edge_pose", "edge_slot", "counts")      # bit i of null_mask


def op_window(call, null=(), **bent):
    """A window call of the call's arguments; `bent` overrides a count (n_cand, n_kf_local_pre, n_kf_fixed_pre, n_point_pre), a capacity
    or a list; `null` names the outputs passed as NULL."""
    c = dict(call, **{k: v for k, v in bent.items() if k in call})
    lists = ("cand_kf", "kf_local_pre", "kf_fixed_pre", "point_pre")
    n = [bent.get(k, 0 if c[f] is None else len(c[f])) for k, f in zip(("n_cand", "n_kf_local_pre", "n_kf_fixed_pre", "n_point_pre"), lists)]
    mask = sum(1 << NULLABLE.index(x) for x in null)
    blob = (i32(6, *n, c["kf_capacity"], c["point_capacity"]) + np.array([c["edge_capacity"]], np.int64).tobytes() + i32(mask)
            + b"".join(arr(c[f], np.int32) for f in lists))
    return ("window", blob, (max(c["kf_capacity"], 0), max(c["point_capacity"], 0), max(c["edge_capacity"], 0)))


def run_ops(exe, tmp_path, ops):
    """The operations through the host program; one dict per operation: rc, message, and a window's outputs."""
    raw = host_prog.run(exe, tmp_path, "run", b"".join(o[1] for o in ops) + i32(0))
    at, out = 0, []
    for kind, _, sizes in ops:
        rc = int(np.frombuffer(raw, np.int32, 1, at)[0]); at += 4
        res = dict(rc=rc, message="")
        if rc:
            n = int(np.frombuffer(raw, np.int32, 1, at)[0]); at += 4
            res["message"] = raw[at:at + n].decode(); at += n
        if kind == "window":
            KC, PC, EC = sizes
            res["counts"] = np.frombuffer(raw, np.int64, 4, at); at += 32
            for name, n, dt in (("local_kf", KC, np.int32), ("fixed_kf", KC, np.int32), ("local_point", PC, np.int32), ("edge_off", PC + 1, np.int64),
                                ("edge_pose", EC, np.int32), ("edge_slot", EC, np.int32)):
                res[name] = np.frombuffer(raw, dt, n, at); at += n * np.dtype(dt).itemsize
        out.append(res)
    assert at == len(raw), (at, len(raw))
    return out


def host_window(exe, tmp_path, tables, call):
    return run_ops(exe, tmp_path, [op_create(tables), op_window(call)])[1]


# ---- the adapter program (tests/ba_window_adapter_prog.cpp) ----------------------------------------------------------------------------
ADAPTER_CASES = ("bad_covisible", "bad_observer", "bad_pkf", "bad_point_null_slots", "point_in_two_local", "fixed_order", "pkf_alone",
                 "slots_257", "obs_blocks", "slot_rows", "random_a", "random_b")        # the scenes without premarks: the adapter passes none


def adapter_scene(name):
    """The scene as a map the SLAM system could hold: no stamp carries pKF's id, and mObservations' idx names the slot that holds the
    point — the LAST of them where a keyframe holds it twice, so that the lowest slot is the wrong answer — and stays what it was
    (folded into the keyframe's keys) where no slot does."""
    sc = CASES[name]()
    for obj in list(sc.kfs) + list(sc.points):
        for f in ("mnBALocalForKF", "mnBAFixedForKF"):
            if hasattr(obj, f):
                setattr(obj, f, 0)
    for p in sc.points:
        for kf in p.mObservations:
            held = [s for s, q in enumerate(kf.mvpMapPoints) if q is p]
            p.mObservations[kf] = held[-1] if held else p.mObservations[kf] % max(1, len(kf.mvpMapPoints))
    return sc


def adapter_blob(sc, mode=0):
    tables, call = R.export_tables(sc), W.export_call(sc)
    obs_idx = [idx for p in sc.points for _, idx in p.GetObservations()]
    return LC.tables_blob(tables) + i32(sc.pkf, mode) + arr(call["cand_kf"], np.int32) + arr(obs_idx, np.int32)


def parse_adapter(raw, n_kf, n_points):
    """What the program wrote: an error text, or the number of window calls and (problem bytes, stamps) of the walk and of the device
    gather."""
    status = int(np.frombuffer(raw, np.int32, 1)[0])
    if status:
        n = int(np.frombuffer(raw, np.int32, 1, 4)[0])
        return dict(error=raw[8:8 + n].decode())
    out, at = dict(error=None, calls=int(np.frombuffer(raw, np.int64, 1, 4)[0])), 12
    for who in ("walk", "device"):
        n = int(np.frombuffer(raw, np.int64, 1, at)[0]); at += 8
        out[who] = raw[at:at + n]; at += n
        s = np.frombuffer(raw, np.int64, 2 * n_kf + n_points, at); at += 8 * len(s)
        out[who + "_local"], out[who + "_fixed"] = s[:n_kf + n_points], s[n_kf + n_points:]
    assert at == len(raw)
    return out


def problem_edges(blob):
    """(n_local_kf, n_local_points, the edges as (keyframe, point, pose, point index), SivoEdge records) of a problem the program wrote."""
    from sivo_amd.optimizer import EDGE_DTYPE
    v = lambda at, n=1: np.frombuffer(blob, np.int32, n, at)
    nl = int(v(0)[0]); at = 4 + 4 * nl
    npt = int(v(at)[0]); at += 4 + 4 * npt
    nv = int(v(at)[0]); at += 4 + 8 * nv
    at += 8 * 12 * nv + nv + 8 * 3 * npt
    ne = int(np.frombuffer(blob, np.int64, 1, at)[0]); at += 8
    edges = np.frombuffer(blob, EDGE_DTYPE, ne, at); at += EDGE_DTYPE.itemsize * ne
    ekf = v(at + 4, ne); at += 4 + 4 * ne
    emp = v(at + 4, ne); at += 4 + 4 * ne
    assert at == len(blob)
    return nl, npt, nv, edges, ekf, emp
