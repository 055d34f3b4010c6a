"""The scenes of the loop-correction tests, one per quirk of LoopClosing::CorrectLoop (reference src/orbslam/LoopClosing.cc:436-526) and
of the map update behind the global bundle adjustment (:694-753): each is an object graph of loop_correct_restatement, flattened into the
arguments of sivo_loop_correct / sivo_gba_propagate before the restatement walks it and read off in the calls' terms afterwards.  Also
the blobs tests/loop_correct_prog.cpp reads and writes.  Every scene is built once per process."""
import functools
import itertools
import struct

import numpy as np

import essential_graph_restatement as EG
import loop_correct_restatement as LR
import sim3_restatement as S3

F, D = np.float32, np.float64
SENTINEL = -7.0
SF = F(1.2) ** np.arange(8, dtype=F)                       # mvScaleFactors of every keyframe


def _rot(axis, angle):
    a = np.asarray(axis, D) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _pose(Rwc, c):
    T = np.eye(4)
    T[:3, :3] = Rwc.T
    T[:3, 3] = -Rwc.T @ c
    return T.astype(F)


def random_pose(rng, k, turn=None):
    yaw = 0.07 * k + rng.normal() * 0.02
    Rwc = _rot([0, 1, 0], yaw) @ np.asarray(S3.random_rotation(rng, 0.05), D)
    if turn is not None:                                   # the camera-from-world rotation itself close to a half turn about one axis
        Rwc = (_rot(np.eye(3)[turn], np.pi - 0.02 - 0.01 * rng.random()) @ np.asarray(S3.random_rotation(rng, 0.01), D)).T
    c = np.array([12 * np.sin(0.07 * k), 0.1 * rng.normal(), 12 * np.cos(0.07 * k)]) + rng.normal(size=3) * 0.05
    return _pose(Rwc, c)


def quat_branch(T):
    """Which branch Quaterniond(R) takes for the rotation of a pose: 3 = positive trace, else the index of the largest diagonal entry
    as Eigen picks it."""
    R = np.asarray(T, D)[:3, :3]
    if R[0, 0] + R[1, 1] + R[2, 2] > 0.0:
        return 3
    i = 0
    if R[1, 1] > R[0, 0]:
        i = 1
    if R[2, 2] > R[i, i]:
        i = 2
    return i


# ---- loop correction -----------------------------------------------------------------------------------------------
def loop_spec(seed, n_kf, n_out=2, n_points=40, slots=12, s=1.0, turns=()):
    """A random scene as plain lists, to be edited before realise_loop: keyframes 0 .. n_kf - 1 are mvpCurrentConnectedKFs (the current
    one last, :437), n_kf .. n_kf + n_out - 1 the keyframes outside the corrected set.  slots: per connected keyframe, or one number."""
    rng = np.random.default_rng(seed)
    n_all = n_kf + n_out
    poses = [random_pose(rng, k, turns[k] if k < len(turns) else None) for k in range(n_all)]
    counts = [slots] * n_kf if np.isscalar(slots) else list(slots)
    slot = []
    for k in range(n_kf):
        row = rng.integers(0, max(n_points, 1), counts[k]) if n_points else np.full(counts[k], -1)
        row = np.where(rng.random(counts[k]) < 0.15, -1, row)
        slot.append([int(v) for v in row])
    obs = []
    for p in range(n_points):
        holders = [k for k in range(n_kf) if p in slot[k]]
        extra = [int(k) for k in rng.integers(0, n_all, 2) if rng.random() < 0.5]
        o = sorted(set(holders + extra))
        obs.append(o if o else [int(rng.integers(0, n_all))])
    ref = [int(o[rng.integers(0, len(o))]) for o in obs]
    pos = [(np.array([12 * np.sin(0.07 * rng.integers(0, n_all)), 0, 12 * np.cos(0.07 * rng.integers(0, n_all))]) + rng.normal(size=3) * 6).astype(F)
           for _ in range(n_points)]
    skip = [bool(rng.random() < 0.1) for _ in range(n_points)]
    level = [int(rng.integers(0, 8)) for _ in range(n_points)]
    pert = EG.exp([0.01 * rng.normal(), 0.02 * rng.normal(), 0.01 * rng.normal(), 0.3 * rng.normal(), 0.05 * rng.normal(), 0.3 * rng.normal(), 0.0])
    return {"rng": rng, "n_kf": n_kf, "n_out": n_out, "poses": poses, "ids": [int(v) for v in rng.permutation(3 * n_all)[:n_all] + 1],
            "addrs": [int(v) for v in rng.permutation(10 * n_all)[:n_all] * 16 + 4096], "slot": slot, "obs": obs, "ref": ref, "pos": pos,
            "skip": skip, "level": level, "pert": pert, "s": s}


def realise_loop(spec):
    """Objects from the lists, the arguments gathered, the restatement run, its results read: dict(args, expect, info)."""
    n_kf, n_all = spec["n_kf"], spec["n_kf"] + spec["n_out"]
    kfs = [LR.KeyFrame(spec["ids"][k], spec["addrs"][k], spec["poses"][k]) for k in range(n_all)]
    cur = kfs[n_kf - 1]
    pts = []
    for p in range(len(spec["pos"])):
        mp = LR.MapPoint(spec["pos"][p], SF[spec["level"][p]], SF[-1])
        for k in spec["obs"][p]:
            mp.AddObservation(kfs[k], 0)
        mp.mpRefKF = None if spec["ref"][p] is None else kfs[spec["ref"][p]]
        if spec["skip"][p]:
            if p % 2:
                mp.mbBad = True
            else:
                mp.mnCorrectedByKF = cur.mnId
        pts.append(mp)
    for k in range(n_kf):
        kfs[k].mvpMapPoints = [None if v < 0 else pts[v] for v in spec["slot"][k]]
    scw = EG.mul(spec["pert"], EG.sim3_from_pose(cur.GetPose())) if spec.get("scw") is None else np.asarray(spec["scw"], D)
    scw = scw.copy()
    if spec.get("scw") is None:
        scw[7] = spec["s"]
    connected = kfs[:n_kf]
    args, table = LR.gather_loop(cur, scw, connected, pts, kfs[n_kf:])
    old_centres = {k: k.GetCameraCenter() for k in kfs}
    cor, non = LR.correct_loop(cur, scw, connected)
    expect = LR.read_loop(args, table, pts, cur, cor, non, SENTINEL)
    return {"args": args, "expect": expect, "info": {"kfs": kfs, "table": table, "points": pts, "cur": cur, "old_centres": old_centres, "spec": spec}}


def _fresh_point(spec, holders, ref, pos=None):
    """A new point held by nobody yet, observed by `holders`; returns its index."""
    rng = spec["rng"]
    p = len(spec["pos"])
    spec["pos"].append((np.array([0.0, 0.0, 12.0]) + rng.normal(size=3) * 4).astype(F) if pos is None else np.asarray(pos, F))
    spec["obs"].append(list(holders))
    spec["ref"].append(ref)
    spec["skip"].append(False)
    spec["level"].append(3)
    return p


def _by_rank(spec):
    """Connected keyframes (vector indices) in CorrectedSim3's order."""
    n_kf = spec["n_kf"]
    return sorted(range(n_kf), key=lambda k: spec["addrs"][k])


def _loop_scene(name):
    if name == "only_current":
        return loop_spec(1, 1, n_out=2, n_points=20, slots=15)
    if name == "two_keyframes":
        return loop_spec(2, 2, n_out=1, n_points=25, slots=14)
    if name == "sixty_five_keyframes":
        return loop_spec(3, 65, n_out=3, n_points=300, slots=20, s=1.07)
    if name == "three_holders":
        sp = loop_spec(4, 5, n_points=10, slots=6)
        order = _by_rank(sp)
        # three holders whose first in CorrectedSim3's order is not their first in mvpCurrentConnectedKFs
        ranks = next(t for t in itertools.combinations(range(5), 3) if order[t[0]] != min(order[r] for r in t))
        p = _fresh_point(sp, [order[r] for r in ranks], order[ranks[1]])
        for r in (ranks[2], ranks[0], ranks[1]):
            sp["slot"][order[r]].append(p)
        sp["mark"], sp["holders"] = p, list(ranks)
        return sp
    if name == "duplicate_slot":
        sp = loop_spec(5, 3, n_points=10, slots=6)
        k = _by_rank(sp)[1]
        p = _fresh_point(sp, [k], k)
        sp["slot"][k] = [p] + sp["slot"][k] + [p]
        sp["mark"] = p
        return sp
    if name == "skip":
        sp = loop_spec(6, 3, n_points=12, slots=8)
        k = _by_rank(sp)[0]
        for j in range(2):                                   # one bad, one already corrected by this loop (odd / even index)
            while len(sp["pos"]) % 2 != j:
                _fresh_point(sp, [k], k)
            p = _fresh_point(sp, [k], k)
            sp["skip"][p] = True
            sp["slot"][k].append(p)
            sp.setdefault("marks", []).append(p)
        return sp
    if name == "null_slots":
        sp = loop_spec(7, 3, n_points=12, slots=8)
        sp["slot"][0] = [-1, -1] + sp["slot"][0] + [-1]
        sp["slot"][1] = [-1] * 5
        return sp
    if name == "empty_keyframe":
        sp = loop_spec(8, 4, n_points=12, slots=8)
        sp["slot"][_by_rank(sp)[1]] = []
        return sp
    if name == "observer_lengths":
        sp = loop_spec(9, 3, n_out=66, n_points=6, slots=4)
        k = _by_rank(sp)[1]
        sp["marks"] = []
        for n in (0, 1, 63, 64, 65):
            obs = ([k] + list(range(3, 3 + n - 1))) if n else []
            p = _fresh_point(sp, obs, k)
            sp["slot"][k].append(p)
            sp["marks"].append(p)
        return sp
    if name == "reference_places":
        sp = loop_spec(10, 5, n_out=2, n_points=8, slots=5)
        order = _by_rank(sp)
        owner = order[2]
        sp["marks"] = []
        for ref in (order[0], owner, order[4], 5):         # before the owner, the owner, after it, outside the corrected set
            p = _fresh_point(sp, sorted({owner, ref}), ref)
            sp["slot"][owner].append(p)
            sp["marks"].append(p)
        return sp
    if name == "outside_observers":
        sp = loop_spec(11, 3, n_out=4, n_points=8, slots=5)
        k = _by_rank(sp)[2]
        p = _fresh_point(sp, [k, 3, 4, 5, 6], 4)
        sp["slot"][k].append(p)
        sp["mark"] = p
        return sp
    if name.startswith("slots_"):
        total = int(name[6:])
        sp = loop_spec(12 + total, 3, n_points=60, slots=[total // 3, 0, total - total // 3 - 1])
        order = _by_rank(sp)
        counts = [total // 3, 0, total - total // 3 - 1]
        rng = sp["rng"]
        for r, k in enumerate(order):                       # the counts follow CorrectedSim3's order: the last slot is the last keyframe's
            row = np.where(rng.random(counts[r]) < 0.1, -1, rng.integers(0, 60, counts[r]))
            sp["slot"][k] = [int(v) for v in row]
        for p in range(60):
            sp["obs"][p] = sorted(set([k for k in range(3) if p in sp["slot"][k]] + [int(rng.integers(0, 5))]))
            sp["ref"][p] = sp["obs"][p][0]
        p = _fresh_point(sp, [order[2]], order[2])
        sp["slot"][order[2]].append(p)
        sp["mark"] = p
        return sp
    if name == "quaternion_branches":
        return loop_spec(20, 5, n_out=1, n_points=30, slots=10, turns=(0, 1, 2, None, None))
    if name == "scale_one":
        return loop_spec(21, 4, n_points=20, slots=10, s=1.0)
    if name == "scale_1_07":
        return loop_spec(21, 4, n_points=20, slots=10, s=1.07)
    if name == "identity_correction":                       # mg2oScw = the current keyframe's own uncorrected Sim3: nothing should move
        sp = loop_spec(22, 6, n_points=40, slots=14)
        sp["scw"] = EG.sim3_from_pose(sp["poses"][5])
        return sp
    raise KeyError(name)


LOOP_SCENES = ("only_current", "two_keyframes", "sixty_five_keyframes", "three_holders", "duplicate_slot", "skip", "null_slots",
               "empty_keyframe", "observer_lengths", "reference_places", "outside_observers", "slots_255", "slots_256", "slots_257",
               "slots_769", "quaternion_branches", "scale_one", "scale_1_07", "identity_correction")


@functools.lru_cache(maxsize=None)
def loop_scene(name):
    return realise_loop(_loop_scene(name))


# ---- the map update behind the global BA ---------------------------------------------------------------------------
N_LOOP_KF = 77


def tree_spec(seed, parent, in_gba, origins, n_points, bad=0.05, from_ba=0.5):
    rng = np.random.default_rng(seed)
    n = len(parent)
    poses = [random_pose(rng, k) for k in range(n)]
    gba = [(random_pose(rng, k) if in_gba[k] else random_pose(rng, k + 50)) for k in range(n)]     # outside the BA: stale
    bef = [random_pose(rng, k + 90) for k in range(n)]                                               # stale
    return {"rng": rng, "parent": list(parent), "in_gba": list(in_gba), "origins": list(origins), "poses": poses, "gba": gba, "bef": bef,
            "addrs": [int(v) for v in rng.permutation(10 * n)[:n] * 16 + 4096],
            "pos": [(rng.normal(size=3) * 8).astype(F) for _ in range(n_points)], "pos_gba": [(rng.normal(size=3) * 8).astype(F) for _ in range(n_points)],
            "point_in_gba": [bool(rng.random() < from_ba) for _ in range(n_points)], "point_bad": [bool(rng.random() < bad) for _ in range(n_points)],
            "ref": [int(rng.integers(0, n)) for _ in range(n_points)]}


def realise_tree(spec):
    n = len(spec["parent"])
    kfs = [LR.KeyFrame(k, spec["addrs"][k], spec["poses"][k]) for k in range(n)]
    for k in range(n):
        kfs[k].mTcwGBA = np.array(spec["gba"][k], F)
        kfs[k].mTcwBefGBA = np.array(spec["bef"][k], F)
        kfs[k].mnBAGlobalForKF = N_LOOP_KF if spec["in_gba"][k] else 3
        if spec["parent"][k] >= 0:
            kfs[spec["parent"][k]].AddChild(kfs[k])
    pts = []
    for p in range(len(spec["pos"])):
        mp = LR.MapPoint(spec["pos"][p])
        mp.mPosGBA = np.array(spec["pos_gba"][p], F)
        mp.mnBAGlobalForKF = N_LOOP_KF if spec["point_in_gba"][p] else 3
        mp.mbBad = spec["point_bad"][p]
        mp.mpRefKF = kfs[spec["ref"][p]]
        pts.append(mp)
    origins = [kfs[k] for k in spec["origins"]]
    args = LR.gather_gba(kfs, origins, pts, N_LOOP_KF)
    walked, status = LR.propagate_global_ba(origins, pts, N_LOOP_KF)
    expect = LR.read_gba(kfs, pts, walked, status, N_LOOP_KF, SENTINEL)
    return {"args": args, "expect": expect, "info": {"kfs": kfs, "points": pts, "walked": walked, "spec": spec}}


def _chain_tree(run):
    """Origin 0 with three children inside the BA; below child 1 a chain of `run` keyframes outside the BA, each with a sibling inside
    the BA, and one keyframe inside the BA below the chain's end."""
    parent, in_gba = [-1, 0, 0, 0], [1, 1, 1, 1]
    tip = 1
    for _ in range(run):
        parent += [tip, tip]
        in_gba += [0, 1]
        tip = len(parent) - 2
    parent.append(tip)
    in_gba.append(1)
    return parent, in_gba


def _tree_scene(name):
    if name.startswith("run_"):
        run = int(name[4:])
        parent, in_gba = _chain_tree(run)
        return tree_spec(30 + run, parent, in_gba, [0], 30)
    if name == "origin_outside":
        parent, in_gba = _chain_tree(2)
        in_gba[0] = 0
        return tree_spec(40, parent, in_gba, [0], 30)
    if name == "unreached_reference":
        parent, in_gba = _chain_tree(1)
        first = len(parent)
        parent += [-1, first, first]                         # a second tree whose root is no origin
        in_gba += [1, 0, 1]
        sp = tree_spec(41, parent, in_gba, [0], 30)
        for j, k in enumerate((first, first + 1, first + 2)):
            sp["ref"][j], sp["point_in_gba"][j], sp["point_bad"][j] = k, False, False
        sp["marks"] = [first, first + 1, first + 2]
        return sp
    if name == "two_origins":
        parent, in_gba = _chain_tree(2)
        first = len(parent)
        parent += [-1, first, first + 1]
        in_gba += [1, 0, 0]
        return tree_spec(42, parent, in_gba, [first, 0], 30)
    if name == "bad_point":
        parent, in_gba = _chain_tree(1)
        sp = tree_spec(43, parent, in_gba, [0], 12, bad=0.0)
        sp["point_bad"][3] = True
        sp["point_bad"][4], sp["point_in_gba"][4] = True, True
        return sp
    if name.startswith("points_"):
        parent, in_gba = _chain_tree(3)
        return tree_spec(44, parent, in_gba, [0], int(name[7:]))
    raise KeyError(name)


TREE_SCENES = ("run_0", "run_1", "run_2", "run_40", "origin_outside", "unreached_reference", "two_origins", "bad_point", "points_0",
               "points_255", "points_256", "points_257")


@functools.lru_cache(maxsize=None)
def tree_scene(name):
    return realise_tree(_tree_scene(name))


def run_lengths(spec):
    """The lengths of the maximal chains of keyframes outside the BA below a keyframe that is inside it or an origin, per chain end."""
    parent, in_gba = spec["parent"], spec["in_gba"]
    out = []
    for k in range(len(parent)):
        if in_gba[k] or k in spec["origins"]:
            continue
        if any(parent[c] == k and not in_gba[c] for c in range(len(parent))):
            continue
        n, d = k, 0
        while not in_gba[n] and n not in spec["origins"]:
            n, d = parent[n], d + 1
        out.append(d)
    return out


# ---- the blobs of tests/loop_correct_prog.cpp ----------------------------------------------------------------------
LOOP_IN = (("tiw", F), ("twc_cur", F), ("scw", D), ("ow", F), ("slot_off", np.int64), ("slot_point", np.int32), ("pos", F), ("skip", np.uint8),
           ("obs_off", np.int64), ("obs_kf", np.int32), ("ref_kf", np.int32), ("level_scale", F), ("last_scale", F))
LOOP_OUT = (("noncorrected_siw", D, 8, "k"), ("corrected_siw", D, 8, "k"), ("tiw_out", F, 16, "k"), ("ow_out", F, 3, "k"),
            ("corrected_by", np.int32, 1, "p"), ("pos_out", F, 3, "p"), ("normal", F, 3, "p"), ("max_dist", F, 1, "p"), ("min_dist", F, 1, "p"),
            ("flags", np.uint8, 1, "p"))
GBA_IN = (("origin", np.int32), ("child_off", np.int64), ("child_kf", np.int32), ("tcw", F), ("tcw_gba", F), ("in_gba", np.uint8), ("tcw_bef", F),
          ("pos", F), ("pos_gba", F), ("point_in_gba", np.uint8), ("point_bad", np.uint8), ("ref_kf", np.int32))
GBA_OUT = (("tcw_gba", F, 16, "k"), ("in_gba", np.uint8, 1, "k"), ("tcw_bef", F, 16, "k"), ("tcw_out", F, 16, "k"), ("ow_out", F, 3, "k"),
           ("kf_reached", np.uint8, 1, "k"), ("pos_out", F, 3, "p"), ("point_status", np.uint8, 1, "p"))
LOOP_POINTERS = [n for n, _ in LOOP_IN] + [n for n, *_ in LOOP_OUT]                   # the struct's pointers in declaration order
GBA_POINTERS = [n for n, _ in GBA_IN] + ["tcw_out", "ow_out", "kf_reached", "pos_out", "point_status"]
NULL_PROBLEM = 1 << 31


def _arrays(a, fields):
    out = b""
    for name, dt in fields:
        v = np.ascontiguousarray(a[name], dt).ravel()
        out += struct.pack("<q", v.size) + v.tobytes()
    return out


def loop_blob(a, null=(), k_out=None, p_out=None, null_problem=False):
    mask = sum(1 << LOOP_POINTERS.index(n) for n in null) | (NULL_PROBLEM if null_problem else 0)
    k_out = max(a["n_kf"], 0) if k_out is None else k_out
    p_out = max(a["n_points"], 0) if p_out is None else p_out
    return struct.pack("<iiiiIqq", a["n_kf"], a["cur"], a["n_all"], a["n_points"], mask, k_out, p_out) + _arrays(a, LOOP_IN)


def gba_blob(a, null=(), k_out=None, p_out=None, null_problem=False):
    mask = sum(1 << GBA_POINTERS.index(n) for n in null) | (NULL_PROBLEM if null_problem else 0)
    k_out = max(a["n_kf"], 0) if k_out is None else k_out
    p_out = max(a["n_points"], 0) if p_out is None else p_out
    return struct.pack("<iiiIqq", a["n_kf"], a["n_origins"], a["n_points"], mask, k_out, p_out) + _arrays(a, GBA_IN)


def loop_adapter_blob(sc):
    """The scene for tests/loop_correct_adapter_prog.cpp: the arrays, and what the object graph needs beside them."""
    a, info = sc["args"], sc["info"]
    table, spec = info["table"], info["spec"]
    by_addr = sorted(table, key=lambda k: k.addr)
    extra = {"rank": [by_addr.index(k) for k in table], "ids": [k.mnId for k in table],
             "connected": [table.index(k) for k in info["kfs"][:spec["n_kf"]]], "bad": [p.mbBad for p in info["points"]], "level": spec["level"], "sf": SF}
    return loop_blob(a) + _arrays(extra, (("rank", np.int32), ("ids", np.int64), ("connected", np.int32), ("bad", np.uint8), ("level", np.int32), ("sf", F)))


def gba_adapter_blob(sc):
    kfs = sc["info"]["kfs"]
    by_addr = sorted(kfs, key=lambda k: k.addr)
    return gba_blob(sc["args"]) + _arrays({"rank": [by_addr.index(k) for k in kfs]}, (("rank", np.int32),))


CALLS = (("calls", np.int32, 1, "1"),)


def parse(blob, fields, k, p):
    """-> rc, error text, {name: flat array}."""
    rc, n = struct.unpack_from("<ii", blob, 0)
    at = 8
    text = blob[at:at + n].decode()
    at += n
    out = {}
    for name, dt, per, which in fields:
        count = per * {"k": k, "p": p, "1": 1}[which]
        out[name] = np.frombuffer(blob, dt, count, at).copy()
        at += count * np.dtype(dt).itemsize
    assert at == len(blob), (at, len(blob))
    return rc, text, out


def same_bytes(got, expect):
    """The names whose bytes differ (floats and doubles compared as bits)."""
    bad = []
    for name, v in got.items():
        e = np.ascontiguousarray(expect[name], v.dtype).ravel()
        if v.shape != e.shape or v.tobytes() != e.tobytes():
            bad.append(name)
    return bad
