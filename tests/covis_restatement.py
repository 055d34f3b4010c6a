"""The yardstick of the covisibility tests: the reference's bookkeeping restated line by line on an OBJECT GRAPH — KeyFrame and MapPoint
objects that mutate each other through AddObservation / EraseObservation / SetBadFlag / EraseMapPointMatch, as the reference's do —
deliberately not in the array form the library computes on.  Transcribed from the reference's src/orbslam sources; the line numbers
stand beside the statements.  std::map<KeyFrame *, ...> iterates in pointer order: a KeyFrame carries `addr`, its stand-in for the
pointer value, and every walk over a map sorts by it.

It produces the results of the four functions (update_connections_counter, vote_local_keyframes, keyframe_culling, map_point_culling)
and exports any scene as the arrays of include/sivo_hip.h (export_table, export_local, export_recent)."""
import numpy as np

SENTINEL = -7                                                       # n_mps / n_redundant of a keyframe the loop skips as id 0


class MapPoint:
    def __init__(self, mnId, first_kf_id=0, found=1, visible=1):
        self.mnId = mnId
        self.mObservations = {}                                     # KeyFrame -> idx
        self.nObs = 0
        self.mbBad = False
        self.mnFirstKFid, self.mnFound, self.mnVisible = first_kf_id, found, visible

    def AddObservation(self, pKF, idx):                              # MapPoint.cc:149-162
        if pKF in self.mObservations:                               # :151
            return
        self.mObservations[pKF] = idx                               # :155
        if pKF.mvRight[idx] >= 0:                                   # :157
            self.nObs += 2
        else:
            self.nObs += 1

    def EraseObservation(self, pKF):                                 # MapPoint.cc:164-189
        bBad = False
        if pKF in self.mObservations:                               # :168
            idx = self.mObservations[pKF]
            if pKF.mvRight[idx] >= 0:                               # :170
                self.nObs -= 2
            else:
                self.nObs -= 1
            del self.mObservations[pKF]                             # :175
            if self.nObs <= 2:                                      # :181
                bBad = True
        if bBad:
            self.SetBadFlag()                                       # :187

    def GetObservations(self):                                       # :191-194, a copy, in std::map order
        return sorted(self.mObservations.items(), key=lambda it: it[0].addr)

    def Observations(self):                                          # :196-199
        return self.nObs

    def SetBadFlag(self):                                            # MapPoint.cc:201-217
        self.mbBad = True                                           # :206
        obs = self.GetObservations()                                # :207
        self.mObservations = {}                                     # :208
        for pKF, idx in obs:                                        # :211-214
            pKF.EraseMapPointMatch(idx)

    def isBad(self):
        return self.mbBad

    def GetFoundRatio(self):                                         # MapPoint.cc:279-282: static_cast<float>(mnFound) / mnVisible
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.float32(self.mnFound) / np.float32(self.mnVisible)


class KeyFrame:
    def __init__(self, mnId, addr, th_depth=40.0):
        self.mnId, self.addr = mnId, addr
        self.mvpMapPoints, self.octave, self.mvRight, self.mvDepth = [], [], [], []
        self.mThDepth = np.float32(th_depth)
        self.mbNotErase = self.mbToBeErased = self.mbBad = False

    def add_slot(self, pMP, octave, right=-1.0, depth=1.0):
        self.mvpMapPoints.append(pMP); self.octave.append(int(octave)); self.mvRight.append(float(right)); self.mvDepth.append(np.float32(depth))
        return len(self.mvpMapPoints) - 1

    def EraseMapPointMatch(self, idx):                               # KeyFrame.cc:265-268 (the size_t overload)
        self.mvpMapPoints[idx] = None

    def SetBadFlag(self):                                            # KeyFrame.cc:477-568 without the graph and tree surgery
        if self.mnId == 0:                                          # :480
            return
        elif self.mbNotErase:                                       # :482
            self.mbToBeErased = True
            return
        for i in range(len(self.mvpMapPoints)):                     # :493-495
            if self.mvpMapPoints[i] is not None:
                self.mvpMapPoints[i].EraseObservation(self)
        self.mbBad = True                                           # :563

    def isBad(self):
        return self.mbBad


class Frame:
    def __init__(self, slots):
        self.mvpMapPoints = list(slots)


class Scene:
    """Keyframes (their table index is their position in `kfs`), points (likewise), and what a case wants to run on them."""

    def __init__(self, n_kf, addr=None, ids=None, th_depth=40.0):
        addr = list(range(100, 100 + n_kf)) if addr is None else addr
        ids = list(range(1, n_kf + 1)) if ids is None else ids
        self.kfs = [KeyFrame(ids[k], addr[k], th_depth) for k in range(n_kf)]
        self.points = []

    def point(self, observers, **kw):
        """A new point observed by (kf index, octave[, stereo[, depth]]) ...: a slot in each keyframe and the observation."""
        pMP = MapPoint(len(self.points), **kw)
        self.points.append(pMP)
        for ob in observers:
            k, octave = ob[0], ob[1]
            stereo = bool(ob[2]) if len(ob) > 2 else False
            depth = ob[3] if len(ob) > 3 else 1.0
            idx = self.kfs[k].add_slot(pMP, octave, 5.0 if stereo else -1.0, depth)
            pMP.AddObservation(self.kfs[k], idx)
        return pMP


# ------------------------------------------------------------------------------------------------------------------------------------
def update_connections_counter(pKF):
    """KFcounter of KeyFrame::UpdateConnections (KeyFrame.cc:328-360)."""
    KFcounter = {}
    vpMP = list(pKF.mvpMapPoints)                                   # :334
    for pMP in vpMP:                                                # :340
        if pMP is None:                                             # :346
            continue
        if pMP.isBad():                                             # :349
            continue
        for pKFi, _ in pMP.GetObservations():                       # :352-354
            if pKFi.mnId == pKF.mnId:                               # :356
                continue
            KFcounter[pKFi] = KFcounter.get(pKFi, 0) + 1            # :358
    return KFcounter


def vote_local_keyframes(frame):
    """keyframeCounter of Tracking::UpdateLocalKeyFrames (Tracking.cc:1128-1142); bad points leave the frame."""
    keyframeCounter = {}
    for i in range(len(frame.mvpMapPoints)):                        # :1129
        if frame.mvpMapPoints[i] is not None:                       # :1130
            pMP = frame.mvpMapPoints[i]
            if not pMP.isBad():                                     # :1132
                for pKF, _ in pMP.GetObservations():                # :1133-1137
                    keyframeCounter[pKF] = keyframeCounter.get(pKF, 0) + 1
            else:
                frame.mvpMapPoints[i] = None                        # :1139
    return keyframeCounter


def keyframe_culling(vpLocalKeyFrames, mbMonocular, removals=True):
    """LocalMapping::KeyFrameCulling (LocalMapping.cc:732-791).  Returns per keyframe (nMPs, nRedundantObservations, decision);
    removals=False records the decision without calling SetBadFlag — what a loop that is not sequential would compute."""
    out = []
    for pKF in vpLocalKeyFrames:                                    # :732
        if pKF.mnId == 0:                                           # :735
            out.append((SENTINEL, SENTINEL, 3))
            continue
        vpMapPoints = list(pKF.mvpMapPoints)                        # :739
        thObs = 3                                                   # :741-742
        nRedundantObservations = 0
        nMPs = 0
        for i in range(len(vpMapPoints)):                           # :745
            pMP = vpMapPoints[i]
            if pMP is not None:                                     # :747
                if not pMP.isBad():                                 # :748
                    if not mbMonocular:                             # :749
                        if pKF.mvDepth[i] > pKF.mThDepth or pKF.mvDepth[i] < 0:     # :750-751 (float comparisons)
                            continue
                    nMPs += 1                                       # :756
                    if pMP.Observations() > thObs:                  # :757
                        scaleLevel = pKF.octave[i]                  # :758
                        nObs = 0
                        for pKFi, idx in pMP.GetObservations():     # :759-765
                            if pKFi is pKF:                         # :767
                                continue
                            scaleLeveli = pKFi.octave[idx]          # :771-772
                            if scaleLeveli <= scaleLevel + 1:       # :774
                                nObs += 1
                                if nObs >= thObs:                   # :776
                                    break
                        if nObs >= thObs:                           # :781
                            nRedundantObservations += 1
        decision = 0
        if nRedundantObservations > 0.9 * nMPs:                     # :789
            decision = 2 if pKF.mbNotErase else 1
            if removals:
                pKF.SetBadFlag()                                    # :790
        out.append((nMPs, nRedundantObservations, decision))
    return out


def map_point_culling(mlpRecentAddedMapPoints, nCurrentKFid, mbMonocular):
    """LocalMapping::MapPointCulling (LocalMapping.cc:165-196).  Returns the status of every point of the list as it stood (the branch it
    took) and the list afterwards."""
    def to_int(x):                                                  # (int) of an unsigned long
        x &= 0xFFFFFFFF
        return x - (1 << 32) if x >= (1 << 31) else x

    def int_sub(a, b):
        return to_int((a - b) & 0xFFFFFFFF)

    cnThObs = 2 if mbMonocular else 3                               # :170-177
    status, kept = [], []
    for pMP in list(mlpRecentAddedMapPoints):                       # :179
        age = int_sub(to_int(nCurrentKFid), to_int(pMP.mnFirstKFid))
        if pMP.isBad():                                             # :181
            status.append(1)
        elif pMP.GetFoundRatio() < np.float32(0.25):                # :183
            pMP.SetBadFlag()
            status.append(2)
        elif age >= 2 and pMP.Observations() <= cnThObs:            # :186-187
            pMP.SetBadFlag()
            status.append(3)
        elif age >= 3:                                              # :190
            status.append(4)
        else:
            status.append(0)
            kept.append(pMP)
    return status, kept


# ------------------------------------------------------------------------------------------------------------------------------------
def export_table(scene):
    """The SivoObsTable of the scene as it stands now."""
    index = {kf: k for k, kf in enumerate(scene.kfs)}
    off, kf, level, stereo = [0], [], [], []
    for pMP in scene.points:
        for pKF, idx in pMP.GetObservations():
            kf.append(index[pKF]); level.append(pKF.octave[idx]); stereo.append(1 if pKF.mvRight[idx] >= 0 else 0)
        off.append(len(kf))
    return dict(n_kf=len(scene.kfs), obs_off=np.array(off, np.int64), obs_kf=np.array(kf, np.int32), obs_level=np.array(level, np.uint8),
                obs_stereo=np.array(stereo, np.uint8), point_bad=np.array([p.isBad() for p in scene.points], np.uint8))


def export_slots(scene, slots):
    return np.array([-1 if p is None else p.mnId for p in slots], np.int32)


def export_local(scene, local):
    """The per-keyframe input of sivo_keyframe_culling for the keyframes `local` (table indices), as sivo_amd.covisibility takes it."""
    out = []
    for k in local:
        pKF = scene.kfs[k]
        out.append(dict(kf=k, is_id0=pKF.mnId == 0, erasable=not pKF.mbNotErase, th_depth=pKF.mThDepth, point=export_slots(scene, pKF.mvpMapPoints),
                        level=np.array(pKF.octave, np.uint8), depth=np.array(pKF.mvDepth, np.float32)))
    return out


def export_recent(points):
    return dict(found=np.array([p.mnFound for p in points], np.int32), visible=np.array([p.mnVisible for p in points], np.int32),
                first_kf_id=np.array([p.mnFirstKFid for p in points], np.int64), n_obs=np.array([p.Observations() for p in points], np.int32),
                bad=np.array([p.isBad() for p in points], np.uint8))
