"""The two map corrections of the loop closer on arrays: LoopClosing::CorrectLoop's pose propagation and point correction (reference
src/orbslam/LoopClosing.cc:436-526) and the map update behind the global bundle adjustment (LoopClosing.cc:694-753).  Host numpy arrays
in and out; the work runs on the GPU (sivo_amd/csrc/loopcorrect.hip) and equals the reference's loops bit for bit."""
import ctypes as C

import numpy as np

from ._lib import check, lib

POINT_STATUS = ("bad", "from_ba", "carried", "reference_outside")          # SIVO_GBA_POINT_*
NO_OBSERVATION = 1                                                         # SIVO_MP_NO_OBSERVATION

_VP = C.c_void_p


class LoopCorrect(C.Structure):  # == SivoLoopCorrect
    _fields_ = [("n_kf", C.c_int32), ("cur", C.c_int32), ("n_all", C.c_int32), ("n_points", C.c_int32)] + [(n, _VP) for n in (
        "tiw", "twc_cur", "scw", "ow", "slot_off", "slot_point", "pos", "skip", "obs_off", "obs_kf", "ref_kf", "level_scale", "last_scale",
        "noncorrected_siw", "corrected_siw", "tiw_out", "ow_out", "corrected_by", "pos_out", "normal", "max_dist", "min_dist", "flags")]


class GbaPropagate(C.Structure):  # == SivoGbaPropagate
    _fields_ = [("n_kf", C.c_int32), ("n_origins", C.c_int32), ("n_points", C.c_int32)] + [(n, _VP) for n in (
        "origin", "child_off", "child_kf", "tcw", "tcw_gba", "in_gba", "tcw_bef", "pos", "pos_gba", "point_in_gba", "point_bad", "ref_kf",
        "tcw_out", "ow_out", "kf_reached", "pos_out", "point_status")]


def _a(x, dt, count=None, what=""):
    v = np.ascontiguousarray(x, dt).ravel()
    if count is not None and v.size != count:
        raise ValueError(f"{what} holds {v.size} numbers where {count} are expected")
    return v


def _p(x):
    return x.ctypes.data if x is not None and x.size else None


def _out(out, name, shape, dt, fill):
    """The caller's array for an output (entries the call does not write keep what it holds), or a fresh one."""
    if out is not None and name in out:
        v = out[name]
        if not isinstance(v, np.ndarray) or v.dtype != dt or v.shape != shape or not v.flags.c_contiguous:
            raise ValueError(f"out[{name!r}] must be a contiguous {np.dtype(dt).name} array of shape {shape}")
        return v
    return np.full(shape, fill, dt)


def correct_loop(tiw, cur, twc_cur, scw, ow, slot_off, slot_point, pos, skip, obs_off, obs_kf, ref_kf, level_scale, last_scale, out=None):
    """LoopClosing.cc:447-526 for the n_kf keyframes of CorrectedSim3 in the order that std::map iterates (tiw: their poses, (n_kf, 4, 4)),
    `cur` the index of the current keyframe, twc_cur its inverse pose, scw = mg2oScw (qx qy qz qw tx ty tz s).  ow (n_all, 3): the camera
    centres of the keyframe table, whose first n_kf entries are the corrected keyframes.  slot_off / slot_point: GetMapPointMatches() of
    each corrected keyframe (-1: null slot).  Per point: pos, skip (isBad() or already corrected by this loop), obs_off / obs_kf (its
    observers in the table, in the order of mObservations), ref_kf, level_scale, last_scale (as mappoint refresh).
    Returns a dict: noncorrected_siw, corrected_siw (n_kf, 8) float64; tiw_out (n_kf, 4, 4), ow_out (n_kf, 3); per point corrected_by
    (the keyframe that moved it, -1: untouched), pos_out, normal, max_dist, min_dist, flags.  The entries of untouched points, and normal
    and the distances of a moved point without observations (flags == NO_OBSERVATION), keep what `out` held (0 without `out`)."""
    tiw = _a(tiw, np.float32)
    K = tiw.size // 16
    ow = _a(ow, np.float32)
    A = ow.size // 3
    pos = _a(pos, np.float32)
    P = pos.size // 3
    if tiw.size != 16 * K or ow.size != 3 * A or pos.size != 3 * P:
        raise ValueError("tiw, ow and pos must hold whole 4 x 4 poses and 3-vectors")
    slot_off, slot_point = _a(slot_off, np.int64, K + 1, "slot_off"), _a(slot_point, np.int32)
    if slot_point.size < (int(slot_off[-1]) if K >= 0 and slot_off.size else 0):
        raise ValueError("slot_point is shorter than slot_off says")
    obs_off, obs_kf = _a(obs_off, np.int64, P + 1, "obs_off"), _a(obs_kf, np.int32)
    if obs_kf.size < int(obs_off[-1]):
        raise ValueError("obs_kf is shorter than obs_off says")
    twc_cur, scw = _a(twc_cur, np.float32, 16, "twc_cur"), _a(scw, np.float64, 8, "scw")
    skip, ref_kf = _a(skip, np.uint8, P, "skip"), _a(ref_kf, np.int32, P, "ref_kf")
    level_scale, last_scale = _a(level_scale, np.float32, P, "level_scale"), _a(last_scale, np.float32, P, "last_scale")
    res = {"noncorrected_siw": np.zeros((K, 8), np.float64), "corrected_siw": np.zeros((K, 8), np.float64),
           "tiw_out": np.zeros((K, 4, 4), np.float32), "ow_out": np.zeros((K, 3), np.float32), "corrected_by": np.full(P, -1, np.int32)}
    for name, shape, dt in (("pos_out", (P, 3), np.float32), ("normal", (P, 3), np.float32), ("max_dist", (P,), np.float32),
                            ("min_dist", (P,), np.float32), ("flags", (P,), np.uint8)):
        res[name] = _out(out, name, shape, dt, 0)
    keep = (tiw, twc_cur, scw, ow, slot_off, slot_point, pos, skip, obs_off, obs_kf, ref_kf, level_scale, last_scale)
    s = LoopCorrect(K, int(cur), A, P, *[_p(v) for v in keep], *[_p(res[n]) for n in (
        "noncorrected_siw", "corrected_siw", "tiw_out", "ow_out", "corrected_by", "pos_out", "normal", "max_dist", "min_dist", "flags")])
    check(lib().sivo_loop_correct(C.byref(s)))
    return res


def propagate_global_ba(origins, child_off, child_kf, tcw, tcw_gba, in_gba, tcw_bef, pos, pos_gba, point_in_gba, point_bad, ref_kf, out=None):
    """LoopClosing.cc:695-753: the walk from the origins through the children (child_off / child_kf: GetChildren() as a CSR) and the
    map points.  tcw = GetPose(), tcw_gba = mTcwGBA, in_gba = (mnBAGlobalForKF == nLoopKF), tcw_bef = mTcwBefGBA per keyframe; pos, pos_gba
    = mPosGBA, point_in_gba, point_bad, ref_kf per point.  The inputs are not modified.
    Returns a dict: tcw_gba, in_gba, tcw_bef after the walk; tcw_out, ow_out (the pose SetPose receives and its camera centre; the rows
    of unreached keyframes keep what `out` held, 0 without `out`), kf_reached; pos_out (written where point_status is from_ba or carried)
    and point_status (indices into POINT_STATUS)."""
    tcw = _a(tcw, np.float32)
    K = tcw.size // 16
    pos = _a(pos, np.float32)
    P = pos.size // 3
    if tcw.size != 16 * K or pos.size != 3 * P:
        raise ValueError("tcw and pos must hold whole 4 x 4 poses and 3-vectors")
    origins = _a(origins, np.int32)
    child_off, child_kf = _a(child_off, np.int64, K + 1, "child_off"), _a(child_kf, np.int32)
    if child_kf.size < int(child_off[-1]):
        raise ValueError("child_kf is shorter than child_off says")
    res = {"tcw_gba": _a(tcw_gba, np.float32, 16 * K, "tcw_gba").copy().reshape(K, 4, 4), "in_gba": _a(in_gba, np.uint8, K, "in_gba").copy(),
           "tcw_bef": _a(tcw_bef, np.float32, 16 * K, "tcw_bef").copy().reshape(K, 4, 4),
           "tcw_out": _out(out, "tcw_out", (K, 4, 4), np.float32, 0), "ow_out": _out(out, "ow_out", (K, 3), np.float32, 0),
           "kf_reached": np.zeros(K, np.uint8), "pos_out": _out(out, "pos_out", (P, 3), np.float32, 0), "point_status": np.zeros(P, np.uint8)}
    pos_gba = _a(pos_gba, np.float32, 3 * P, "pos_gba")
    point_in_gba, point_bad = _a(point_in_gba, np.uint8, P, "point_in_gba"), _a(point_bad, np.uint8, P, "point_bad")
    ref_kf = _a(ref_kf, np.int32, P, "ref_kf")
    s = GbaPropagate(K, origins.size, P, _p(origins), _p(child_off), _p(child_kf), _p(tcw), _p(res["tcw_gba"]), _p(res["in_gba"]),
                     _p(res["tcw_bef"]), _p(pos), _p(pos_gba), _p(point_in_gba), _p(point_bad), _p(ref_kf), _p(res["tcw_out"]), _p(res["ow_out"]),
                     _p(res["kf_reached"]), _p(res["pos_out"]), _p(res["point_status"]))
    check(lib().sivo_gba_propagate(C.byref(s)))
    return res
