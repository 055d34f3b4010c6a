"""The covisibility bookkeeping of the three SLAM threads on arrays: the counting loop of KeyFrame::UpdateConnections (reference
src/orbslam/KeyFrame.cc:327-415) and of Tracking::UpdateLocalKeyFrames (Tracking.cc:1126-1142), LocalMapping::KeyFrameCulling
(LocalMapping.cc:727-792) and LocalMapping::MapPointCulling (LocalMapping.cc:165-196).  Host numpy arrays in and out; the work runs on
the GPU (sivo_amd/csrc/covis.hip).  Integer results: exact."""
import ctypes as C

import numpy as np

from ._lib import check, lib

DECISION = ("kept", "culled", "to_be_erased", "id0")                                       # SIVO_KFCULL_*
STATUS = ("stays", "already_bad", "found_ratio", "observations", "aged_out")               # SIVO_MPCULL_*
LDS_KF = 8192                                                                              # SIVO_COVIS_LDS_KF


class _Table(C.Structure):  # == SivoObsTable
    _fields_ = [("n_kf", C.c_int32), ("n_points", C.c_int32), ("obs_off", C.c_void_p), ("obs_kf", C.c_void_p), ("obs_level", C.c_void_p),
                ("obs_stereo", C.c_void_p), ("point_bad", C.c_void_p)]


def _a(x, dt):
    return np.ascontiguousarray(x, dt).ravel()


def _p(x):
    return x.ctypes.data if x is not None and x.size else None


class ObservationTable:
    """mObservations of n_points map points as a CSR over dense keyframe indices 0 .. n_kf - 1: obs_off (n_points + 1), and per
    observation obs_kf, obs_level (mvKeysSemantic[idx].octave) and obs_stereo (mvRight[idx] >= 0); point_bad (n_points) = isBad()."""

    def __init__(self, n_kf, obs_off, obs_kf, obs_level, obs_stereo, point_bad):
        self.n_kf = int(n_kf)
        self.obs_off = _a(obs_off, np.int64)
        self.obs_kf, self.obs_level, self.obs_stereo = _a(obs_kf, np.int32), _a(obs_level, np.uint8), _a(obs_stereo, np.uint8)
        self.point_bad = _a(point_bad, np.uint8)
        self.n_points = len(self.point_bad)
        if len(self.obs_off) != self.n_points + 1:
            raise ValueError("obs_off must hold n_points + 1 offsets")
        n = int(self.obs_off[-1])
        if not (len(self.obs_kf) == len(self.obs_level) == len(self.obs_stereo)) or len(self.obs_kf) < n:
            raise ValueError("the observation arrays are shorter than obs_off says")

    def struct(self):
        return _Table(self.n_kf, self.n_points, _p(self.obs_off), _p(self.obs_kf), _p(self.obs_level), _p(self.obs_stereo), _p(self.point_bad))


def _csr(lists, dt):
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(s) for s in lists], out=off[1:])
    flat = np.concatenate([_a(s, dt) for s in lists]) if len(lists) else np.zeros(0, dt)
    return off, _a(flat, dt)


def shared_counts(table, sets, selfs, out=None):
    """counts[s, k] = the number of slots of sets[s] (map-point indices, -1 for a null slot) whose point is not bad and is observed by
    keyframe k, observations by k == selfs[s] skipped (-1 skips none).  Every set in one launch.  Returns (len(sets), n_kf) int32."""
    off, pts = _csr(sets, np.int32)
    selfs = _a(selfs, np.int32)
    if len(selfs) != len(sets):
        raise ValueError("one self index per set")
    counts = np.zeros((len(sets), table.n_kf), np.int32) if out is None else out
    if counts.shape != (len(sets), table.n_kf) or counts.dtype != np.int32 or not counts.flags.c_contiguous:
        raise ValueError("out must be a contiguous (n_sets, n_kf) int32 array")
    t = table.struct()
    check(lib().sivo_covis_count(C.byref(t), len(sets), _p(off), _p(pts), _p(selfs), _p(counts)))
    return counts


def keyframe_culling(table, local, monocular=False, out=None):
    """LocalMapping::KeyFrameCulling over the keyframes of `local`, in order.  Each is a dict: kf (table index), is_id0, erasable,
    th_depth, and per slot point (-1: null), level, depth.  Returns n_mps, n_redundant, decision (indices into DECISION) and bad_after
    (per point of the table).  `out` pre-fills n_mps / n_redundant: a keyframe skipped as id 0 leaves its entries as they were."""
    K = len(local)
    kf = _a([k["kf"] for k in local], np.int32)
    id0 = _a([bool(k["is_id0"]) for k in local], np.uint8)
    erasable = _a([bool(k["erasable"]) for k in local], np.uint8)
    th = _a([k["th_depth"] for k in local], np.float32)
    off, pts = _csr([k["point"] for k in local], np.int32)
    _, lvl = _csr([k["level"] for k in local], np.uint8)
    _, dep = _csr([k["depth"] for k in local], np.float32)
    if not (len(pts) == len(lvl) == len(dep)):
        raise ValueError("point, level and depth of a keyframe differ in length")
    res = {}
    for name in ("n_mps", "n_redundant"):
        res[name] = np.zeros(K, np.int32) if out is None or name not in out else _a(out[name], np.int32).copy()
        if len(res[name]) != K:
            raise ValueError(name + " differs in length from the keyframes")
    decision, bad_after = np.zeros(K, np.uint8), np.zeros(table.n_points, np.uint8)
    t = table.struct()
    check(lib().sivo_keyframe_culling(C.byref(t), K, _p(kf), _p(id0), _p(erasable), _p(th), _p(off), _p(pts), _p(lvl), _p(dep), int(bool(monocular)),
                                      _p(res["n_mps"]), _p(res["n_redundant"]), _p(decision), _p(bad_after)))
    res.update(decision=decision, bad_after=bad_after)
    return res


def map_point_culling(found, visible, first_kf_id, n_obs, bad, current_kf_id, monocular=False):
    """The branch of LocalMapping::MapPointCulling each recently added point takes: indices into STATUS."""
    found, visible, n_obs = _a(found, np.int32), _a(visible, np.int32), _a(n_obs, np.int32)
    first, bad = _a(first_kf_id, np.int64), _a(bad, np.uint8)
    n = len(found)
    if not (len(visible) == len(n_obs) == len(first) == len(bad) == n):
        raise ValueError("the point arrays differ in length")
    status = np.zeros(n, np.uint8)
    check(lib().sivo_mappoint_culling(n, _p(found), _p(visible), _p(first), _p(n_obs), _p(bad), int(current_kf_id), int(bool(monocular)), _p(status)))
    return status
