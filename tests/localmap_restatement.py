"""The yardstick of the local-map tests: Tracking::UpdateLocalMap of the reference (src/orbslam/Tracking.cc:1087-1235) restated line by
line on an OBJECT GRAPH — KeyFrame, MapPoint and Frame objects with mnTrackReferenceForFrame, ordered connections, children and a parent —
deliberately not in the array form the library computes on.  The line numbers stand beside the statements.  std::map<KeyFrame *, ...> and
std::set<KeyFrame *> iterate in pointer order: a KeyFrame carries `addr`, its stand-in for the pointer value, and every walk over a map or
a set sorts by it.

It produces what the function leaves (Tracking.UpdateLocalMap) and exports a scene as the arrays of include/sivo_hip.h (export_tables,
export_call, export_result)."""
import numpy as np

SENTINEL = -7                                                       # what an output entry holds that the call does not own


class MapPoint:
    def __init__(self, mnId):
        self.mnId = mnId
        self.mObservations = {}                                     # KeyFrame -> idx
        self.mbBad = False
        self.mnTrackReferenceForFrame = 0                           # MapPoint.cc:36, :68

    def GetObservations(self):                                       # MapPoint.cc:191-194, a copy, in std::map order
        return sorted(self.mObservations.items(), key=lambda it: it[0].addr)

    def isBad(self):
        return self.mbBad


class KeyFrame:
    def __init__(self, mnId, addr):
        self.mnId, self.addr = mnId, addr
        self.mvpMapPoints = []
        self.mvpOrderedConnectedKeyFrames = []
        self.mspChildren = set()
        self.mpParent = None
        self.mbBad = False
        self.mnTrackReferenceForFrame = 0                           # KeyFrame.cc:38

    def add_slot(self, pMP):
        self.mvpMapPoints.append(pMP)
        return len(self.mvpMapPoints) - 1

    def GetMapPointMatches(self):                                    # KeyFrame.cc:317-320, a copy
        return list(self.mvpMapPoints)

    def GetBestCovisibilityKeyFrames(self, N):                       # KeyFrame.cc:222-230
        if len(self.mvpOrderedConnectedKeyFrames) < N:              # :224
            return list(self.mvpOrderedConnectedKeyFrames)
        else:
            return list(self.mvpOrderedConnectedKeyFrames[:N])      # :228

    def GetChildren(self):                                           # KeyFrame.cc:433-436, a copy of the std::set
        return sorted(self.mspChildren, key=lambda kf: kf.addr)

    def GetParent(self):                                             # KeyFrame.cc:438-441
        return self.mpParent

    def isBad(self):
        return self.mbBad


class Frame:
    def __init__(self, mnId, slots):
        self.mnId = mnId
        self.mvpMapPoints = list(slots)
        self.numSemanticKeys = len(self.mvpMapPoints)
        self.mpReferenceKF = None


class Tracking:
    def __init__(self, frame, local_kfs=(), reference_kf=None):
        self.mCurrentFrame = frame
        self.mvpLocalKeyFrames = list(local_kfs)
        self.mvpLocalMapPoints = []
        self.mpReferenceKF = reference_kf
        self.keyframeCounter = None                                 # kept for the tests: the vote, and whether it was empty
        self.pKFmax = None

    def UpdateLocalMap(self):                                        # :1087-1094 (without the viewer's :1089)
        self.UpdateLocalKeyFrames()                                 # :1092
        self.UpdateLocalPoints()                                    # :1093

    def UpdateLocalPoints(self):                                     # :1096-1124
        self.mvpLocalMapPoints = []                                 # :1097
        for pKF in self.mvpLocalKeyFrames:                          # :1099-1103
            vpMPs = pKF.GetMapPointMatches()                        # :1105
            for pMP in vpMPs:                                       # :1107
                if pMP is None:                                     # :1110
                    continue
                if pMP.mnTrackReferenceForFrame == self.mCurrentFrame.mnId:     # :1114
                    continue
                if not pMP.isBad():                                 # :1118
                    self.mvpLocalMapPoints.append(pMP)              # :1119
                    pMP.mnTrackReferenceForFrame = self.mCurrentFrame.mnId      # :1120

    def UpdateLocalKeyFrames(self):                                  # :1126-1235
        F = self.mCurrentFrame
        keyframeCounter = {}                                        # :1128
        for i in range(F.numSemanticKeys):                          # :1129
            if F.mvpMapPoints[i] is not None:                       # :1130
                pMP = F.mvpMapPoints[i]
                if not pMP.isBad():                                 # :1132
                    for pKF, _ in pMP.GetObservations():            # :1133-1137
                        keyframeCounter[pKF] = keyframeCounter.get(pKF, 0) + 1
                else:
                    F.mvpMapPoints[i] = None                        # :1139
        self.keyframeCounter = keyframeCounter
        self.pKFmax = None
        if not keyframeCounter:                                     # :1144
            return

        max_ = 0                                                    # :1147
        pKFmax = None                                               # :1148
        self.mvpLocalKeyFrames = []                                 # :1150

        for pKF, count in sorted(keyframeCounter.items(), key=lambda it: it[0].addr):      # :1156-1159, std::map order
            if pKF.isBad():                                         # :1162
                continue
            if count > max_:                                        # :1165
                max_ = count
                pKFmax = pKF
            self.mvpLocalKeyFrames.append(pKF)                      # :1170
            pKF.mnTrackReferenceForFrame = F.mnId                   # :1171

        itEndKF = len(self.mvpLocalKeyFrames)                       # :1179: the end iterator is taken before the loop
        for it in range(itEndKF):                                   # :1177-1181
            if len(self.mvpLocalKeyFrames) > 80:                    # :1183
                break
            pKF = self.mvpLocalKeyFrames[it]                        # :1186
            vNeighs = pKF.GetBestCovisibilityKeyFrames(10)          # :1188-1189
            for pNeighKF in vNeighs:                                # :1191-1195
                if not pNeighKF.isBad():                            # :1197
                    if pNeighKF.mnTrackReferenceForFrame != F.mnId:                 # :1198
                        self.mvpLocalKeyFrames.append(pNeighKF)     # :1199
                        pNeighKF.mnTrackReferenceForFrame = F.mnId  # :1200
                        break                                       # :1201
            spChilds = pKF.GetChildren()                            # :1206
            for pChildKF in spChilds:                               # :1207-1210
                if not pChildKF.isBad():                            # :1212
                    if pChildKF.mnTrackReferenceForFrame != F.mnId:                 # :1213
                        self.mvpLocalKeyFrames.append(pChildKF)     # :1214
                        pChildKF.mnTrackReferenceForFrame = F.mnId  # :1215
                        break                                       # :1216
            pParent = pKF.GetParent()                               # :1221
            if pParent is not None:                                 # :1222
                if pParent.mnTrackReferenceForFrame != F.mnId:      # :1223
                    self.mvpLocalKeyFrames.append(pParent)          # :1224
                    pParent.mnTrackReferenceForFrame = F.mnId       # :1225
                    break                                           # :1226: the innermost loop is the one over the keyframes

        self.pKFmax = pKFmax
        if pKFmax is not None:                                      # :1231
            self.mpReferenceKF = pKFmax                             # :1232
            F.mpReferenceKF = self.mpReferenceKF                    # :1233


class Scene:
    """Keyframes (their table index is their position in `kfs`) and points (likewise), and the call a case makes on them: the frame, the
    local keyframes the caller holds, the reference keyframe it holds."""

    def __init__(self, n_kf, addr=None):
        addr = list(range(100, 100 + n_kf)) if addr is None else list(addr)
        assert len(set(addr)) == n_kf
        self.kfs = [KeyFrame(k + 1, addr[k]) for k in range(n_kf)]
        self.points = []
        self.frame = Frame(7, [])
        self.prev = []
        self.reference = None

    def point(self, observers, slots=None):
        """A new point observed by the keyframes `observers` (table indices), held in a slot of each (or of `slots` where given)."""
        pMP = MapPoint(len(self.points))
        self.points.append(pMP)
        for k in observers:
            pMP.mObservations[self.kfs[k]] = len(self.kfs[k].mvpMapPoints)
        for k in (observers if slots is None else slots):
            self.kfs[k].add_slot(pMP)
        return pMP

    def connect(self, k, covisibles=(), children=(), parent=None):
        kf = self.kfs[k]
        kf.mvpOrderedConnectedKeyFrames = [self.kfs[c] for c in covisibles]
        kf.mspChildren = {self.kfs[c] for c in children}
        kf.mpParent = None if parent is None else self.kfs[parent]

    def set_frame(self, slots, mnId=7):
        self.frame = Frame(mnId, slots)

    def premark(self, kfs=(), points=()):
        for k in kfs:
            self.kfs[k].mnTrackReferenceForFrame = self.frame.mnId
        for p in points:
            self.points[p].mnTrackReferenceForFrame = self.frame.mnId


def csr(lists, dt):
    off = np.zeros(len(lists) + 1, np.int64)
    if len(lists):
        off[1:] = np.cumsum([len(s) for s in lists])
    flat = np.array([v for s in lists for v in s], dt)
    return off, flat


def export_tables(scene):
    """SivoLocalMapTables of the scene as it stands now (n_kf and the twelve arrays)."""
    index = {kf: k for k, kf in enumerate(scene.kfs)}
    obs_off, obs_kf = csr([[index[kf] for kf, _ in p.GetObservations()] for p in scene.points], np.int32)
    slot_off, slot_point = csr([[-1 if p is None else p.mnId for p in kf.mvpMapPoints] for kf in scene.kfs], np.int32)
    covis_off, covis_kf = csr([[index[c] for c in kf.mvpOrderedConnectedKeyFrames] for kf in scene.kfs], np.int32)
    child_off, child_kf = csr([[index[c] for c in kf.GetChildren()] for kf in scene.kfs], np.int32)
    order = np.array(sorted(range(len(scene.kfs)), key=lambda k: scene.kfs[k].addr), np.int32)
    return dict(n_kf=len(scene.kfs), obs_off=obs_off, obs_kf=obs_kf, point_bad=np.array([p.isBad() for p in scene.points], np.uint8),
                kf_bad=np.array([kf.isBad() for kf in scene.kfs], np.uint8), slot_off=slot_off, slot_point=slot_point, covis_off=covis_off,
                covis_kf=covis_kf, child_off=child_off, child_kf=child_kf,
                parent=np.array([-1 if kf.mpParent is None else index[kf.mpParent] for kf in scene.kfs], np.int32),
                kf_order=None if order.tolist() == list(range(len(order))) else order)


def export_call(scene):
    """The arguments of sivo_localmap_update for the scene's frame, before the call."""
    index = {kf: k for k, kf in enumerate(scene.kfs)}
    F = scene.frame
    return dict(frame_point=np.array([-1 if p is None else p.mnId for p in F.mvpMapPoints], np.int32),
                kf_premarked=np.array([k for k, kf in enumerate(scene.kfs) if kf.mnTrackReferenceForFrame == F.mnId], np.int32),
                point_premarked=np.array([p.mnId for p in scene.points if p.mnTrackReferenceForFrame == F.mnId], np.int32),
                prev_local_kf=np.array([index[kf] for kf in scene.prev], np.int32))


def run(scene):
    """Tracking::UpdateLocalMap on the scene (which it mutates); the Tracking object afterwards."""
    t = Tracking(scene.frame, scene.prev, scene.reference)
    t.UpdateLocalMap()
    return t


def export_result(scene, before, t, kf_capacity, point_capacity):
    """What sivo_localmap_update leaves in sentinel-filled arrays of the given capacities, from the restatement's graph after the call;
    `before` = export_call(scene) taken before it."""
    index = {kf: k for k, kf in enumerate(scene.kfs)}
    voted = bool(t.keyframeCounter)
    after = np.array([-1 if p is None else p.mnId for p in scene.frame.mvpMapPoints], np.int32)
    local_kf = np.full(kf_capacity, SENTINEL, np.int32)
    if voted:
        local_kf[:len(t.mvpLocalKeyFrames)] = [index[kf] for kf in t.mvpLocalKeyFrames]
    local_point = np.full(point_capacity, SENTINEL, np.int32)
    local_point[:len(t.mvpLocalMapPoints)] = [p.mnId for p in t.mvpLocalMapPoints]
    counts = np.zeros(len(scene.kfs), np.int32)
    for kf, c in t.keyframeCounter.items():
        counts[index[kf]] = c
    return dict(voted=int(voted), n_local_kf=len(t.mvpLocalKeyFrames) if voted else SENTINEL,
                ref_kf=-1 if t.pKFmax is None else index[t.pKFmax], n_local_points=len(t.mvpLocalMapPoints),
                slot_cleared=(before["frame_point"] != after).astype(np.uint8), local_kf=local_kf, local_point=local_point, counts=counts)
