"""The inputs of tests/covis_adapter_prog.cpp: scenes of tests/covis_cases.py and a few of their own as whole object graphs (every
keyframe's slots, every point's observations with their slot index), and the reader of what the program writes."""
import numpy as np

import covis_cases as P
import covis_restatement as R


def graph_blob(sc):
    """The graph as it stands; nObs travels as it is (a bad point keeps its last value, map-point culling sets it by hand)."""
    index = {kf: k for k, kf in enumerate(sc.kfs)}
    off, pts = P.csr([R.export_slots(sc, kf.mvpMapPoints) for kf in sc.kfs], np.int32)
    _, lvl = P.csr([kf.octave for kf in sc.kfs], np.uint8)
    _, right = P.csr([kf.mvRight for kf in sc.kfs], np.float32)
    _, depth = P.csr([kf.mvDepth for kf in sc.kfs], np.float32)
    obs = [p.GetObservations() for p in sc.points]
    ooff, okf = P.csr([[index[kf] for kf, _ in o] for o in obs], np.int32)
    _, oidx = P.csr([[idx for _, idx in o] for o in obs], np.int32)
    a = R.export_recent(sc.points)
    return b"".join([P.i32(len(sc.kfs), len(sc.points)), np.array([kf.mnId for kf in sc.kfs], np.int64).tobytes(),
                     np.array([kf.mbNotErase for kf in sc.kfs], np.uint8).tobytes(), np.array([kf.mThDepth for kf in sc.kfs], np.float32).tobytes(),
                     off.tobytes(), pts.tobytes(), lvl.tobytes(), right.tobytes(), depth.tobytes(), a["bad"].tobytes(), a["found"].tobytes(),
                     a["visible"].tobytes(), a["first_kf_id"].tobytes(), a["n_obs"].tobytes(), ooff.tobytes(), okf.tobytes(), oidx.tobytes()])


def copies(raw, n_copies):
    """The int32 streams the program wrote: the first is the reference's way, each later one SIVO's with the number of C ABI calls."""
    w = np.frombuffer(raw, np.int32)
    out, calls, at = [], [], 0
    for c in range(n_copies):
        n = int(w[at]); out.append(w[at + 1:at + 1 + n]); at += 1 + n
        if c:
            calls.append(int(w[at])); at += 1
    assert at == len(w)
    return out, calls


def parse_graph(w, n_kf, n_points):
    """The stream Graph::dump writes, as dicts; returns (keyframes, points, words read)."""
    at, kfs, pts = 0, [], []

    def take(width=1):
        nonlocal at
        n = int(w[at]); v = w[at + 1:at + 1 + n * width]; at += 1 + n * width
        return v.tolist() if width == 1 else v.reshape(-1, width).tolist()

    for _ in range(n_kf):
        kf = dict(bad=int(w[at]), to_be_erased=int(w[at + 1]), first_connection=int(w[at + 2]), parent=int(w[at + 3]))
        at += 4
        kf.update(ordered=take(), weights=take(), connected=take(2), children=take(), slots=take())
        kfs.append(kf)
    for _ in range(n_points):
        pt = dict(bad=int(w[at]), n_obs=int(w[at + 1]))
        at += 2
        pt["obs"] = take(2)
        pts.append(pt)
    return kfs, pts, at


# ---- UpdateConnections ---------------------------------------------------------------------------------------------------------------
def connections_scene():
    """Keyframe 0 shares 20 points with keyframe 1 and 20 with keyframe 2 (a tie, resolved by pointer), 16 with keyframe 3, 3 with keyframe 4
    (below th: no connection).  Keyframe 5 shares 4 points with keyframe 4 and 4 with keyframe 3: nothing reaches th, the first maximum
    in pointer order is the fallback.  Keyframe 6 has id 0 (no parent), keyframe 7 sees nothing.  Some points are bad, some slots null."""
    sc = R.Scene(8, ids=[5, 3, 9, 1, 7, 2, 0, 4])
    for a, b, n in ((0, 1, 20), (0, 2, 20), (0, 3, 16), (0, 4, 3), (5, 4, 4), (5, 3, 4), (6, 1, 17), (6, 0, 15), (1, 2, 14)):
        for _ in range(n):
            sc.point([(a, 1), (b, 1, True)])
    for _ in range(3):                                              # bad points do not count: 0 - 3 stays at 16
        sc.point([(0, 1), (3, 1)]).mbBad = True
    sc.kfs[0].add_slot(None, 0)
    sc.kfs[0].add_slot(sc.points[40], 2)                            # a point in two slots counts twice: 0 - 3 is 17 seen from 0
    return sc


CONNECTION_ORDERS = {"all": [0, 1, 2, 3, 4, 5, 6, 7], "shuffled": [5, 2, 7, 0, 6, 3, 1, 4], "one": [0], "twice": [0, 5, 0]}


def connections_blob(order):
    return graph_blob(connections_scene()) + P.i32(len(order)) + np.array(order, np.int32).tobytes()


# ---- KeyFrameCulling -----------------------------------------------------------------------------------------------------------------
KF_NAMES = ("chain", "bad_chain", "not_erasable", "id0_middle", "depth", "not_listed", "empty_list", "family_1")


def kfcull_blob(name, mono):
    sc, local = P.KF_CASES[name]()
    return graph_blob(sc) + P.i32(int(mono), len(local)) + np.array(local, np.int32).tobytes()


# ---- MapPointCulling -----------------------------------------------------------------------------------------------------------------
def mpcull_scene(n):
    """The points of covis_cases.mp_points; the first 20 sit in slots of keyframe 0 and list it, so that SetBadFlag has a slot to clear."""
    sc = R.Scene(2)
    sc.points = P.mp_objects(n)
    for p in sc.points[:20]:
        n_obs, bad = p.nObs, p.mbBad
        idx = sc.kfs[0].add_slot(p, 1)
        p.AddObservation(sc.kfs[0], idx)
        p.nObs = n_obs
        if bad:                                                     # a bad point has left its keyframes
            p.mObservations = {}
            sc.kfs[0].mvpMapPoints[idx] = None
    return sc


def mpcull_blob(n, mono):
    sc = mpcull_scene(n)
    return b"".join([graph_blob(sc), P.i32(int(mono)), np.array([P.MP_CURRENT], np.int64).tobytes(), P.i32(n),
                     np.arange(n, dtype=np.int32).tobytes()])


# ---- the vote ------------------------------------------------------------------------------------------------------------------------
def vote_scene():
    sc, sets = P.COUNT_CASES["n_kf_65"]()
    return sc, sets[1][1]


def vote_blob():
    sc, frame = vote_scene()
    slots = R.export_slots(sc, frame.mvpMapPoints)
    return graph_blob(sc) + P.i32(len(slots)) + slots.tobytes()


def walk_blob(reps):
    """The timing mode tools/covis_probe.py uses, on the chain scene: its two local keyframes, a frame over all points, every point as a
    recent one."""
    sc, local = P.KF_CASES["chain"]()
    n = len(sc.points)
    slots = np.arange(n, dtype=np.int32)
    return b"".join([graph_blob(sc), P.i32(0, len(local)), np.array(local, np.int32).tobytes(), P.i32(n), slots.tobytes(),
                     np.array([P.MP_CURRENT], np.int64).tobytes(), P.i32(n), slots.tobytes(), P.i32(reps)])


def all_blobs():
    out = [("connections", connections_blob(o)) for o in CONNECTION_ORDERS.values()]
    out += [("kfcull", kfcull_blob(n, m)) for n in KF_NAMES for m in ((0, 1) if n in P.KF_MONO else (0,))]
    out += [("mpcull", mpcull_blob(n, m)) for n, m in P.MP_RUNS]
    return out + [("vote", vote_blob())]
