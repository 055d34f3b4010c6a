"""The part of the reference's map graph that tests/covis_restatement.py leaves out, restated line by line on its object graph: the
covisibility graph and the spanning tree of src/orbslam/KeyFrame.cc — AddConnection / UpdateBestCovisibles (:171-205), the second half of
UpdateConnections (:362-414), EraseConnection (:575-587), ChangeParent (:427-431) and SetBadFlag with its tree surgery (:477-568).  The
line numbers stand beside the statements.  A keyframe of covis_restatement gets the members on first use (`graph_members`);
std::map<KeyFrame *, ...> and std::set<KeyFrame *> iterate in pointer order, which is the order of `addr`.

`dump` writes a scene as the int32 stream tests/covis_adapter_prog.cpp and oracle/ref_mapgraph_driver.cpp write."""
import numpy as np

import covis_restatement as R


def graph_members(pKF):
    if not hasattr(pKF, "mConnectedKeyFrameWeights"):
        pKF.mConnectedKeyFrameWeights = {}                         # KeyFrame -> weight
        pKF.mvpOrderedConnectedKeyFrames, pKF.mvOrderedWeights = [], []
        pKF.mbFirstConnection = True                                # KeyFrame.cc:84
        pKF.mpParent = None                                         # :85
        pKF.mspChildren = set()
    return pKF


def _by_addr(kfs):
    return sorted(kfs, key=lambda kf: kf.addr)


def ordered_pairs(pairs):
    """std::sort on (weight, pointer) pairs, then each pushed to the FRONT of a list (:194-200, :392-398)."""
    vPairs = sorted(pairs, key=lambda wk: (wk[0], wk[1].addr))
    lKFs, lWs = [], []
    for w, kf in vPairs:
        lKFs.insert(0, kf)
        lWs.insert(0, w)
    return lKFs, lWs


def UpdateBestCovisibles(pKF):                                       # KeyFrame.cc:185-205
    graph_members(pKF)
    vPairs = [(w, kf) for kf, w in pKF.mConnectedKeyFrameWeights.items()]      # :189-192
    pKF.mvpOrderedConnectedKeyFrames, pKF.mvOrderedWeights = ordered_pairs(vPairs)


def AddConnection(pKF, other, weight):                               # KeyFrame.cc:171-183
    graph_members(pKF)
    if other not in pKF.mConnectedKeyFrameWeights:                  # :174
        pKF.mConnectedKeyFrameWeights[other] = weight
    elif pKF.mConnectedKeyFrameWeights[other] != weight:            # :176
        pKF.mConnectedKeyFrameWeights[other] = weight
    else:
        return                                                      # :179
    UpdateBestCovisibles(pKF)                                       # :182


def EraseConnection(pKF, other):                                     # KeyFrame.cc:575-587
    graph_members(pKF)
    if other in pKF.mConnectedKeyFrameWeights:                      # :579
        del pKF.mConnectedKeyFrameWeights[other]
        UpdateBestCovisibles(pKF)                                   # :586


def AddChild(pKF, child):                                            # :417-420
    graph_members(pKF).mspChildren.add(child)


def EraseChild(pKF, child):                                          # :422-425
    graph_members(pKF).mspChildren.discard(child)


def ChangeParent(pKF, parent):                                       # KeyFrame.cc:427-431
    graph_members(pKF).mpParent = parent
    AddChild(parent, pKF)


def GetWeight(pKF, other):                                           # :252-258
    return graph_members(pKF).mConnectedKeyFrameWeights.get(other, 0)


def UpdateConnections(pKF):                                          # KeyFrame.cc:327-415
    graph_members(pKF)
    KFcounter = R.update_connections_counter(pKF)                   # :328-360
    if not KFcounter:                                               # :363
        return
    nmax, pKFmax, th = 0, None, 15                                  # :370-372
    vPairs = []
    for other in _by_addr(KFcounter):                               # :376, std::map order
        n = KFcounter[other]
        if n > nmax:                                                # :377
            nmax, pKFmax = n, other
        if n >= th:                                                 # :381
            vPairs.append((n, other))
            AddConnection(other, pKF, n)                            # :383
    if not vPairs:                                                  # :387
        vPairs.append((nmax, pKFmax))
        AddConnection(pKFmax, pKF, nmax)                            # :389
    lKFs, lWs = ordered_pairs(vPairs)                               # :392-398
    pKF.mConnectedKeyFrameWeights = dict(KFcounter)                 # :404
    pKF.mvpOrderedConnectedKeyFrames, pKF.mvOrderedWeights = lKFs, lWs        # :405-407
    if pKF.mbFirstConnection and pKF.mnId != 0:                     # :409
        pKF.mpParent = pKF.mvpOrderedConnectedKeyFrames[0]          # :410
        AddChild(pKF.mpParent, pKF)                                 # :411
        pKF.mbFirstConnection = False                               # :412


def SetBadFlag(pKF, erased=None):
    """KeyFrame::SetBadFlag (KeyFrame.cc:477-568) whole; `erased` collects the keyframes handed to Map::EraseKeyFrame (:566)."""
    graph_members(pKF)
    if pKF.mnId == 0:                                               # :480
        return
    elif pKF.mbNotErase:                                            # :482
        pKF.mbToBeErased = True
        return
    for other in _by_addr(pKF.mConnectedKeyFrameWeights):           # :488-491
        EraseConnection(other, pKF)
    for i in range(len(pKF.mvpMapPoints)):                          # :493-495
        if pKF.mvpMapPoints[i] is not None:
            pKF.mvpMapPoints[i].EraseObservation(pKF)
    pKF.mConnectedKeyFrameWeights = {}                              # :500
    pKF.mvpOrderedConnectedKeyFrames = []                           # :501 (mvOrderedWeights stays as it was)
    sParentCandidates = {pKF.mpParent}                              # :504-505
    while pKF.mspChildren:                                          # :510
        bContinue = False
        max_ = -1                                                   # :513
        pC = pP = None
        for child in _by_addr(pKF.mspChildren):                     # :517, std::set order
            if child.isBad():                                       # :520
                continue
            vpConnected = list(graph_members(child).mvpOrderedConnectedKeyFrames)     # :524-525
            for connected in vpConnected:                           # :526
                for cand in _by_addr(sParentCandidates):            # :527
                    if connected.mnId == cand.mnId:                 # :530: ids, not pointers
                        w = GetWeight(child, connected)             # :531
                        if w > max_:                                # :532
                            pC, pP, max_ = child, connected, w
                            bContinue = True
        if bContinue:                                               # :543
            ChangeParent(pC, pP)                                    # :544
            sParentCandidates.add(pC)                               # :545
            pKF.mspChildren.discard(pC)                             # :546
        else:
            break                                                   # :548
    if pKF.mspChildren:                                             # :554
        for child in _by_addr(pKF.mspChildren):                     # :555-558
            ChangeParent(child, pKF.mpParent)
    EraseChild(pKF.mpParent, pKF)                                   # :561
    pKF.mbBad = True                                                # :563
    if erased is not None:
        erased.append(pKF)                                          # :566-567


def keyframe_culling(kfs, vpLocalKeyFrames, mbMonocular, erased=None):
    """LocalMapping::KeyFrameCulling as covis_restatement.keyframe_culling states it, every keyframe of `kfs` with the whole SetBadFlag
    above in place of the one without the tree surgery."""
    for pKF in kfs:
        pKF.SetBadFlag = (lambda kf: lambda: SetBadFlag(kf, erased))(pKF)
    return R.keyframe_culling(vpLocalKeyFrames, mbMonocular)


def dump(kfs, points, anchor=None):
    """The int32 stream of Graph::dump (tests/covis_adapter_prog.cpp); `anchor` is written as len(kfs)."""
    index = {kf: k for k, kf in enumerate(kfs)}
    if anchor is not None:
        index[anchor] = len(kfs)
    pidx = {p: i for i, p in enumerate(points)}
    w = []
    for kf in kfs:
        graph_members(kf)
        w += [int(kf.mbBad), int(kf.mbToBeErased), int(kf.mbFirstConnection), -1 if kf.mpParent is None else index[kf.mpParent]]
        w += [len(kf.mvpOrderedConnectedKeyFrames)] + [index[o] for o in kf.mvpOrderedConnectedKeyFrames]
        w += [len(kf.mvOrderedWeights)] + list(kf.mvOrderedWeights)
        w.append(len(kf.mConnectedKeyFrameWeights))
        for o in _by_addr(kf.mConnectedKeyFrameWeights):
            w += [index[o], kf.mConnectedKeyFrameWeights[o]]
        w += [len(kf.mspChildren)] + [index[c] for c in _by_addr(kf.mspChildren)]
        w += [len(kf.mvpMapPoints)] + [-1 if p is None else pidx[p] for p in kf.mvpMapPoints]
    for p in points:
        obs = p.GetObservations()
        w += [int(p.mbBad), int(p.nObs), len(obs)]
        for kf, idx in obs:
            w += [index[kf], idx]
    return np.array(w, np.int32)
