"""A line-by-line walk of the two map corrections of the loop closer on an object graph: LoopClosing::CorrectLoop's pose propagation and
point correction (reference src/orbslam/LoopClosing.cc:436-526) and the map update behind RunGlobalBundleAdjustment (:694-753), with
KeyFrame / MapPoint classes that carry what those passages touch (SetPose, GetCameraCenter, UpdateNormalAndDepth, the pointer-ordered
std::map and std::set, the std::list of the breadth-first walk).  cv::Mat arithmetic is numpy float32 under the rounding rules of
sivo_amd/api/compat/cv_min.hpp, g2o::Sim3 arithmetic float64 through the routines of essential_graph_restatement, the normal and the
distances through mappoint_restatement.  Also: the flattening of such a graph into the arrays of sivo_loop_correct / sivo_gba_propagate
(include/sivo_hip.h) and the reading of the graph after the walk in the same terms — what the C++ adapter does with the SLAM types.
The checker of sivo_amd/csrc/loopcorrect_math.hpp; test infrastructure, not the product."""
import collections

import numpy as np

import essential_graph_restatement as EG
import mappoint_restatement as MR

F, D = np.float32, np.float64
NO_OBSERVATION = MR.NO_OBSERVATION
POINT_BAD, POINT_FROM_BA, POINT_CARRIED, POINT_REF_OUTSIDE = 0, 1, 2, 3


# ---- cv::Mat, CV_32F (cv_min.hpp) ----------------------------------------------------------------------------------
def gemm(A, B, alpha=1.0, C=None, beta=1.0):
    """alpha * A * B + beta * C with no transposed operand and an inner dimension of 2..4: gemm's small-matrix path — every dot product
    accumulated left to right in float, then (float)(t * alpha + c * beta) in double."""
    A, B = np.asarray(A, F), np.asarray(B, F)
    B2 = B.reshape(B.shape[0], -1)
    M, K, N = A.shape[0], A.shape[1], B2.shape[1]
    assert 2 <= K <= 4 and (K == N or K == M) and B2.shape[0] == K
    out = np.zeros((M, N), F)
    C2 = None if C is None else np.asarray(C, F).reshape(M, N)
    with np.errstate(all="ignore"):
        for i in range(M):
            for j in range(N):
                t = F(A[i, 0] * B2[0, j])
                for k in range(1, K):
                    t = F(t + F(A[i, k] * B2[k, j]))
                c = D(0.0) if C2 is None else D(C2[i, j]) * D(beta)
                out[i, j] = F(D(t) * D(alpha) + c)
    return out.reshape(M) if B.ndim == 1 else out


class PtrMap:
    """std::map<KeyFrame *, T> / std::set<KeyFrame *>: iteration by pointer value (the object's `addr`)."""

    def __init__(self):
        self._d = {}

    def __setitem__(self, k, v):
        self._d[k] = v

    def __getitem__(self, k):
        return self._d[k]

    def __contains__(self, k):
        return k in self._d

    def __len__(self):
        return len(self._d)

    def items(self):
        return sorted(self._d.items(), key=lambda kv: kv[0].addr)

    def keys(self):
        return [k for k, _ in self.items()]


class KeyFrame:
    def __init__(self, mnId, addr, Tcw):
        self.mnId, self.addr = mnId, addr
        self.mvpMapPoints = []                 # GetMapPointMatches(): MapPoint or None per slot
        self.mspChildrens = PtrMap()           # std::set<KeyFrame *>
        self.mTcwGBA = np.eye(4, dtype=F)
        self.mTcwBefGBA = np.eye(4, dtype=F)
        self.mnBAGlobalForKF = 0
        self.set_pose_calls = 0
        self.SetPose(Tcw)
        self.set_pose_calls = 0

    def SetPose(self, Tcw):
        """KeyFrame.cc:116-129 (without the stereo centre)."""
        self.mTcw = np.array(Tcw, F)
        Rcw = self.mTcw[0:3, 0:3]
        tcw = self.mTcw[0:3, 3]
        Rwc = Rcw.T.copy()                                     # cv::Mat Rwc = Rcw.t(): materialised
        self.mOw = gemm(Rwc, tcw, alpha=-1.0)                  # mOw = -Rwc * tcw
        self.mTwc = np.eye(4, dtype=F)
        self.mTwc[0:3, 0:3] = Rwc
        self.mTwc[0:3, 3] = self.mOw
        self.set_pose_calls += 1

    def GetPose(self):
        return self.mTcw.copy()

    def GetPoseInverse(self):
        return self.mTwc.copy()

    def GetCameraCenter(self):
        return self.mOw.copy()

    def GetMapPointMatches(self):
        return list(self.mvpMapPoints)

    def GetChildren(self):
        return self.mspChildrens.keys()

    def AddChild(self, kf):
        self.mspChildrens[kf] = True


class MapPoint:
    def __init__(self, pos, level_scale=1.0, last_scale=1.0):
        self.mWorldPos = np.array(pos, F)
        self.mbBad = False
        self.mnCorrectedByKF = 0
        self.mnCorrectedReference = 0
        self.mObservations = PtrMap()          # std::map<KeyFrame *, size_t>
        self.mpRefKF = None
        self.level_scale, self.last_scale = F(level_scale), F(last_scale)     # mvScaleFactors[level], mvScaleFactors[nLevels - 1]
        self.mNormalVector = np.full(3, -7.0, F)
        self.mfMaxDistance = F(-7.0)
        self.mfMinDistance = F(-7.0)
        self.mnBAGlobalForKF = 0
        self.mPosGBA = np.zeros(3, F)
        self.updates = 0                       # how often UpdateNormalAndDepth wrote
        self.centres_seen = None               # the camera centres the last UpdateNormalAndDepth read, reference keyframe last

    def isBad(self):
        return self.mbBad

    def GetWorldPos(self):
        return self.mWorldPos.copy()

    def SetWorldPos(self, P):
        self.mWorldPos = np.array(P, F).reshape(3)

    def GetReferenceKeyFrame(self):
        return self.mpRefKF

    def AddObservation(self, kf, idx=0):
        self.mObservations[kf] = idx

    def UpdateNormalAndDepth(self):
        """MapPoint.cc:368-411; the sums and norms are mappoint_restatement's."""
        if self.mbBad:
            return
        observations = self.mObservations.keys()
        if len(observations) == 0:
            return
        ow = np.stack([kf.GetCameraCenter() for kf in observations])
        ref_ow = self.mpRefKF.GetCameraCenter()
        r = MR.refresh([0, 0], np.zeros((0, 32), np.uint8), [0, len(observations)], ow, self.mWorldPos[None], ref_ow[None],
                       [self.level_scale], [self.last_scale])
        self.mfMaxDistance, self.mfMinDistance, self.mNormalVector = r["max_dist"][0], r["min_dist"][0], r["normal"][0].copy()
        self.updates += 1
        self.centres_seen = np.concatenate([ow, ref_ow[None]])


# ---- LoopClosing::CorrectLoop, :436-526 ----------------------------------------------------------------------------
def correct_loop(mpCurrentKF, mg2oScw, mvpCurrentConnectedKFs):
    """mvpCurrentConnectedKFs: GetVectorCovisibleKeyFrames() with mpCurrentKF pushed back (:436-437).  Returns CorrectedSim3,
    NonCorrectedSim3 (PtrMaps of (8,) float64: qx qy qz qw tx ty tz s)."""
    mg2oScw = np.asarray(mg2oScw, D)
    CorrectedSim3, NonCorrectedSim3 = PtrMap(), PtrMap()
    CorrectedSim3[mpCurrentKF] = mg2oScw.copy()                                     # :440
    Twc = mpCurrentKF.GetPoseInverse()                                              # :441
    for pKFi in mvpCurrentConnectedKFs:                                             # :447
        Tiw = pKFi.GetPose()
        if pKFi is not mpCurrentKF:                                                 # :455
            Tic = gemm(Tiw, Twc)
            g2oSic = EG.sim3_from_pose(Tic)                                         # Sim3(Ric, tic, 1.0)
            CorrectedSim3[pKFi] = EG.mul(g2oSic, mg2oScw)                           # :461-463
        NonCorrectedSim3[pKFi] = EG.sim3_from_pose(Tiw)                             # :466-471
    for pKFi, g2oCorrectedSiw in CorrectedSim3.items():                             # :476
        g2oCorrectedSwi = EG.inv(g2oCorrectedSiw)
        g2oSiw = NonCorrectedSim3[pKFi]
        for pMPi in pKFi.GetMapPointMatches():                                      # :486-487
            if pMPi is None:
                continue
            if pMPi.isBad():
                continue
            if pMPi.mnCorrectedByKF == mpCurrentKF.mnId:
                continue
            eigP3Dw = pMPi.GetWorldPos().astype(D)                                  # :498-500
            eigCorrectedP3Dw = EG.sim3_map(g2oCorrectedSwi, EG.sim3_map(g2oSiw, eigP3Dw))
            pMPi.SetWorldPos(np.asarray(eigCorrectedP3Dw, D).astype(F))             # :504-505
            pMPi.mnCorrectedByKF = mpCurrentKF.mnId
            pMPi.mnCorrectedReference = pKFi.mnId
            pMPi.UpdateNormalAndDepth()                                             # :508
        pKFi.SetPose(EG.pose_from_sim3(g2oCorrectedSiw))                            # :513-522
    return CorrectedSim3, NonCorrectedSim3


# ---- RunGlobalBundleAdjustment, :694-753 ---------------------------------------------------------------------------
def propagate_global_ba(mvpKeyFrameOrigins, vpMPs, nLoopKF):
    """Returns the keyframes the walk came by, in its order."""
    lpKFtoCheck = collections.deque(mvpKeyFrameOrigins)                             # :695
    walked = []
    while lpKFtoCheck:
        pKF = lpKFtoCheck[0]
        sChilds = pKF.GetChildren()
        Twc = pKF.GetPoseInverse()
        for pChild in sChilds:                                                      # :702
            if pChild.mnBAGlobalForKF != nLoopKF:
                Tchildc = gemm(pChild.GetPose(), Twc)                               # :707
                pChild.mTcwGBA = gemm(Tchildc, pKF.mTcwGBA)                         # :708-709
                pChild.mnBAGlobalForKF = nLoopKF
            lpKFtoCheck.append(pChild)
        pKF.mTcwBefGBA = pKF.GetPose()                                              # :715
        pKF.SetPose(pKF.mTcwGBA)
        walked.append(pKF)
        lpKFtoCheck.popleft()
    status = []
    for pMP in vpMPs:                                                               # :723
        if pMP.isBad():
            status.append(POINT_BAD)
            continue
        if pMP.mnBAGlobalForKF == nLoopKF:
            pMP.SetWorldPos(pMP.mPosGBA)                                            # :731
            status.append(POINT_FROM_BA)
        else:
            pRefKF = pMP.GetReferenceKeyFrame()
            if pRefKF.mnBAGlobalForKF != nLoopKF:                                   # :737
                status.append(POINT_REF_OUTSIDE)
                continue
            Rcw = pRefKF.mTcwBefGBA[0:3, 0:3]
            tcw = pRefKF.mTcwBefGBA[0:3, 3]
            Xc = gemm(Rcw, pMP.GetWorldPos(), C=tcw)                                # :744
            Twc = pRefKF.GetPoseInverse()
            pMP.SetWorldPos(gemm(Twc[0:3, 0:3], Xc, C=Twc[0:3, 3]))                 # :747-751
            status.append(POINT_CARRIED)
    return walked, status


# ---- the graph as the arrays of include/sivo_hip.h -----------------------------------------------------------------
def csr(lists, dt):
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(s) for s in lists], out=off[1:])
    flat = np.concatenate([np.asarray(s, dt).ravel() for s in lists]) if len(lists) else np.zeros(0, dt)
    return off, np.ascontiguousarray(flat, dt)


def gather_loop(cur, scw, connected, points, others=()):
    """The arguments of sivo_loop_correct for the graph BEFORE correct_loop runs.  points: every MapPoint of the scene (their order is the
    point index); others: keyframes outside the corrected set that observe or are reference keyframes.  Returns (args, kfs): kfs the
    keyframe table, the corrected ones first in std::map order."""
    corrected = sorted(set(connected), key=lambda k: k.addr)
    kfs = corrected + sorted((k for k in others if k not in corrected), key=lambda k: k.addr)
    kidx = {k: i for i, k in enumerate(kfs)}
    pidx = {id(p): i for i, p in enumerate(points)}
    slot_off, slot_point = csr([[-1 if m is None else pidx[id(m)] for m in k.mvpMapPoints] for k in corrected], np.int32)
    obs_off, obs_kf = csr([[kidx[k] for k in p.mObservations.keys()] for p in points], np.int32)
    n = len(points)
    a = {
        "n_kf": len(corrected), "cur": kidx[cur], "n_all": len(kfs), "n_points": n,
        "tiw": np.stack([k.GetPose() for k in corrected]).astype(F), "twc_cur": cur.GetPoseInverse(), "scw": np.asarray(scw, D).copy(),
        "ow": np.stack([k.GetCameraCenter() for k in kfs]).astype(F), "slot_off": slot_off, "slot_point": slot_point,
        "pos": np.array([p.mWorldPos for p in points], F).reshape(n, 3),
        "skip": np.array([p.isBad() or p.mnCorrectedByKF == cur.mnId for p in points], np.uint8),
        "obs_off": obs_off, "obs_kf": obs_kf, "ref_kf": np.array([-1 if p.mpRefKF is None else kidx[p.mpRefKF] for p in points], np.int32),
        "level_scale": np.array([p.level_scale for p in points], F), "last_scale": np.array([p.last_scale for p in points], F),
    }
    return a, kfs


def read_loop(a, kfs, points, cur, corrected_sim3, noncorrected_sim3, sentinel=-7.0):
    """The outputs of sivo_loop_correct read off the graph AFTER correct_loop ran on it (a: what gather_loop returned before)."""
    K, n = a["n_kf"], a["n_points"]
    by_id = {k.mnId: i for i, k in enumerate(kfs)}
    out = {
        "noncorrected_siw": np.stack([noncorrected_sim3[k] for k in kfs[:K]]), "corrected_siw": np.stack([corrected_sim3[k] for k in kfs[:K]]),
        "tiw_out": np.stack([k.GetPose() for k in kfs[:K]]), "ow_out": np.stack([k.GetCameraCenter() for k in kfs[:K]]),
        "corrected_by": np.full(n, -1, np.int32), "pos_out": np.full((n, 3), sentinel, F), "normal": np.full((n, 3), sentinel, F),
        "max_dist": np.full(n, sentinel, F), "min_dist": np.full(n, sentinel, F), "flags": np.full(n, 255, np.uint8),
    }
    for i, p in enumerate(points):
        if a["skip"][i] or p.mnCorrectedByKF != cur.mnId:
            continue
        out["corrected_by"][i] = by_id[p.mnCorrectedReference]
        out["pos_out"][i] = p.mWorldPos
        if len(p.mObservations) == 0:
            out["flags"][i] = NO_OBSERVATION
            continue
        out["flags"][i] = 0
        out["normal"][i], out["max_dist"][i], out["min_dist"][i] = p.mNormalVector, p.mfMaxDistance, p.mfMinDistance
    return out


def gather_gba(kfs, origins, points, nLoopKF):
    """The arguments of sivo_gba_propagate for the graph BEFORE propagate_global_ba runs; kfs: every keyframe (their order is the index)."""
    kidx = {k: i for i, k in enumerate(kfs)}
    child_off, child_kf = csr([[kidx[c] for c in k.GetChildren()] for k in kfs], np.int32)
    n, K = len(points), len(kfs)
    return {
        "n_kf": K, "n_origins": len(origins), "n_points": n, "origin": np.array([kidx[k] for k in origins], np.int32),
        "child_off": child_off, "child_kf": child_kf, "tcw": np.array([k.GetPose() for k in kfs], F).reshape(K, 4, 4),
        "tcw_gba": np.array([k.mTcwGBA for k in kfs], F).reshape(K, 4, 4),
        "in_gba": np.array([k.mnBAGlobalForKF == nLoopKF for k in kfs], np.uint8),
        "tcw_bef": np.array([k.mTcwBefGBA for k in kfs], F).reshape(K, 4, 4), "pos": np.array([p.mWorldPos for p in points], F).reshape(n, 3),
        "pos_gba": np.array([p.mPosGBA for p in points], F).reshape(n, 3),
        "point_in_gba": np.array([p.mnBAGlobalForKF == nLoopKF for p in points], np.uint8),
        "point_bad": np.array([p.isBad() for p in points], np.uint8),
        "ref_kf": np.array([-1 if p.mpRefKF is None else kidx[p.mpRefKF] for p in points], np.int32),
    }


def read_gba(kfs, points, walked, status, nLoopKF, sentinel=-7.0):
    K, n = len(kfs), len(points)
    reached = np.array([k in walked for k in kfs], np.uint8)
    out = {
        "tcw_gba": np.array([k.mTcwGBA for k in kfs], F).reshape(K, 4, 4), "in_gba": np.array([k.mnBAGlobalForKF == nLoopKF for k in kfs], np.uint8),
        "tcw_bef": np.array([k.mTcwBefGBA for k in kfs], F).reshape(K, 4, 4), "tcw_out": np.full((K, 4, 4), sentinel, F),
        "ow_out": np.full((K, 3), sentinel, F), "kf_reached": reached, "pos_out": np.full((n, 3), sentinel, F),
        "point_status": np.array(status, np.uint8).reshape(n),
    }
    for i, k in enumerate(kfs):
        if reached[i]:
            out["tcw_out"][i], out["ow_out"][i] = k.GetPose(), k.GetCameraCenter()
    for i, p in enumerate(points):
        if status[i] in (POINT_FROM_BA, POINT_CARRIED):
            out["pos_out"][i] = p.mWorldPos
    return out
