"""The yardstick of the bundle-adjustment window tests: the head of Optimizer::LocalBundleAdjustment of the reference
(src/orbslam/Optimizer.cc:496-559: lLocalKeyFrames, lLocalMapPoints, lFixedKFs; :585-622: the vertices; :651-670: one edge per observation)
restated line by line on the OBJECT GRAPH of tests/localmap_restatement.py — KeyFrame and MapPoint objects with mnBALocalForKF and
mnBAFixedForKF stamps — deliberately not in the array form the library computes on.  The line numbers stand beside the statements.
std::map<KeyFrame *, size_t> iterates in pointer order: GetObservations() of the graph sorts by `addr`.

It produces what the function has built when the optimisation starts (Window) and exports a scene as the arrays of
sivo_localmap_ba_window (export_call, export_result)."""
import numpy as np

import localmap_restatement as R

SENTINEL = R.SENTINEL
SLOT_NONE, SLOT_AMBIGUOUS = -1, -2                                  # SIVO_BAWIN_SLOT_*
OUTPUTS = ("counts", "local_kf", "fixed_kf", "local_point", "edge_off", "edge_pose", "edge_slot")


def stamps(obj):
    """mnBALocalForKF (KeyFrame.cc:39, MapPoint.cc:37, :69) and mnBAFixedForKF (KeyFrame.cc:39) start at 0."""
    if not hasattr(obj, "mnBALocalForKF"):
        obj.mnBALocalForKF = 0
        obj.mnBAFixedForKF = 0
    return obj


def GetVectorCovisibleKeyFrames(pKF):                                # KeyFrame.cc:217-220, a copy
    return list(pKF.mvpOrderedConnectedKeyFrames)


class Window:
    """lLocalKeyFrames, lLocalMapPoints, lFixedKFs, the pose vertices in the order they are added, and per local point its edges as
    (pKFi, idx) in the order they are added.  `stray` holds, per local point, the edges the reference ties to a POINT vertex: (the local
    point whose vertex the id lookup found, pKFi, idx) — see LocalBundleAdjustment; they are no part of `edges`."""

    def __init__(self):
        self.lLocalKeyFrames, self.lLocalMapPoints, self.lFixedKFs, self.vertices, self.edges, self.stray = [], [], [], [], [], []


def LocalBundleAdjustment(pKF):
    w = Window()
    stamps(pKF)
    w.lLocalKeyFrames.append(pKF)                                   # :499
    pKF.mnBALocalForKF = pKF.mnId                                   # :500

    vCovisibleKFs = GetVectorCovisibleKeyFrames(pKF)                # :503-504
    for pKFi in vCovisibleKFs:                                      # :506-507
        stamps(pKFi).mnBALocalForKF = pKF.mnId                      # :508
        if not pKFi.isBad():                                        # :510
            w.lLocalKeyFrames.append(pKFi)                          # :511

    for lit in w.lLocalKeyFrames:                                   # :517-519
        vpMPs = lit.GetMapPointMatches()                            # :521
        for pMP in vpMPs:                                           # :522-523
            if pMP is not None:                                     # :524
                if not pMP.isBad():                                 # :525
                    if stamps(pMP).mnBALocalForKF != pKF.mnId:      # :526
                        w.lLocalMapPoints.append(pMP)               # :527
                        pMP.mnBALocalForKF = pKF.mnId               # :528

    for lit in w.lLocalMapPoints:                                   # :538-540
        observations = lit.GetObservations()                        # :542
        for pKFi, _ in observations:                                # :546-549
            stamps(pKFi)
            if pKFi.mnBALocalForKF != pKF.mnId and pKFi.mnBAFixedForKF != pKF.mnId:     # :551-552
                pKFi.mnBAFixedForKF = pKF.mnId                      # :553
                if not pKFi.isBad():                                # :554
                    w.lFixedKFs.append(pKFi)                        # :555

    for pKFi in w.lLocalKeyFrames:                                  # :585-587
        w.vertices.append(pKFi)                                     # :594-600
    for pKFi in w.lFixedKFs:                                        # :608-609
        w.vertices.append(pKFi)                                     # :612-618

    maxKFid = max([0] + [v.mnId for v in w.vertices])               # :577, :602-604, :619-621
    by_id = {v.mnId: v for v in w.vertices}                         # optimizer.vertex(id) looks an id up among ALL vertices
    for pMP in w.lLocalMapPoints:                                   # :651-653
        by_id.setdefault(pMP.mnId + maxKFid + 1, pMP)               # :657-660 (addVertex refuses an id that is taken)
        observations = pMP.GetObservations()                        # :662-663
        row, stray = [], []
        for pKFi, idx in observations:                              # :666-668
            if not pKFi.isBad():                                    # :670
                v = by_id.get(pKFi.mnId)                            # :687, :726: by the keyframe's id, not by the keyframe
                if v is pKFi:
                    row.append((pKFi, idx))
                elif v is not None:                                 # a keyframe without a pose vertex whose id a point vertex carries: the
                    stray.append((v, pKFi, idx))                    # reference adds an edge between two point vertices, which no solve survives
        w.edges.append(row)                                         # (optimizer.vertex() is null otherwise: addEdge refuses the edge)
        w.stray.append(stray)
    return w


def export_call(scene):
    """The arguments of sivo_localmap_ba_window for scene.kfs[scene.pkf], before the call."""
    index = {kf: k for k, kf in enumerate(scene.kfs)}
    pKF = scene.kfs[scene.pkf]
    return dict(cand_kf=np.array([scene.pkf] + [index[c] for c in GetVectorCovisibleKeyFrames(pKF)], np.int32),
                kf_local_pre=np.array([k for k, kf in enumerate(scene.kfs) if stamps(kf).mnBALocalForKF == pKF.mnId], np.int32),
                kf_fixed_pre=np.array([k for k, kf in enumerate(scene.kfs) if stamps(kf).mnBAFixedForKF == pKF.mnId], np.int32),
                point_pre=np.array([p.mnId for p in scene.points if stamps(p).mnBALocalForKF == pKF.mnId], np.int32))


def slot_code(pKFi, pMP):
    held = [s for s, q in enumerate(pKFi.mvpMapPoints) if q is pMP]
    return held[0] if len(held) == 1 else SLOT_NONE if not held else SLOT_AMBIGUOUS


def export_result(scene, w, kf_capacity, point_capacity, edge_capacity):
    """What sivo_localmap_ba_window leaves in sentinel-filled arrays of the given capacities, from the restatement's window."""
    index = {kf: k for k, kf in enumerate(scene.kfs)}
    pose = {id(kf): j for j, kf in enumerate(w.vertices)}
    n_edges = sum(len(row) for row in w.edges)
    out = dict(counts=np.array([len(w.lLocalKeyFrames), len(w.lLocalMapPoints), len(w.lFixedKFs), n_edges], np.int64),
               local_kf=np.full(kf_capacity, SENTINEL, np.int32), fixed_kf=np.full(kf_capacity, SENTINEL, np.int32),
               local_point=np.full(point_capacity, SENTINEL, np.int32), edge_off=np.full(point_capacity + 1, SENTINEL, np.int64),
               edge_pose=np.full(edge_capacity, SENTINEL, np.int32), edge_slot=np.full(edge_capacity, SENTINEL, np.int32))
    out["local_kf"][:len(w.lLocalKeyFrames)] = [index[kf] for kf in w.lLocalKeyFrames]
    out["fixed_kf"][:len(w.lFixedKFs)] = [index[kf] for kf in w.lFixedKFs]
    out["local_point"][:len(w.lLocalMapPoints)] = [p.mnId for p in w.lLocalMapPoints]
    out["edge_off"][:len(w.edges) + 1] = np.concatenate([[0], np.cumsum([len(row) for row in w.edges], dtype=np.int64)])
    flat = [(pMP, pKFi) for pMP, row in zip(w.lLocalMapPoints, w.edges) for pKFi, _ in row]
    out["edge_pose"][:n_edges] = [pose[id(pKFi)] for _, pKFi in flat]
    out["edge_slot"][:n_edges] = [slot_code(pKFi, pMP) for pMP, pKFi in flat]
    return out


def run(scene):
    """The restatement on the scene (which it mutates); the Window."""
    return LocalBundleAdjustment(scene.kfs[scene.pkf])
