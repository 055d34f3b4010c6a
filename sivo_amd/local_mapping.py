"""Python mirror of the computation of LocalMapping::Run between SearchForTriangulation and LocalBundleAdjustment (reference
src/orbslam/LocalMapping.cc:198-472, src/orbslam/MapPoint.cc:284-347, :368-411) over the C ABI: sivo_triangulate /
sivo_triangulate_batch run the loop over the matches of a keyframe pair (parallax, triangulation or unprojection, the depth,
reprojection and scale tests, both CheckSemantics calls), sivo_mappoint_refresh runs ComputeDistinctiveDescriptors and
UpdateNormalAndDepth for a batch of map points."""
import ctypes as C

import numpy as np

from ._lib import TriKeyFrame, TriMatch, TriProblem, check, lib

KEYFRAME_DTYPE = np.dtype([("Rcw", np.float32, 9), ("tcw", np.float32, 3), ("Ow", np.float32, 3), ("Twc", np.float32, 12),
                           ("fx", np.float32), ("fy", np.float32), ("cx", np.float32), ("cy", np.float32), ("invfx", np.float32),
                           ("invfy", np.float32), ("mb", np.float32), ("mbf", np.float32), ("nlevels", np.int32),
                           ("scale_factors", np.float32, 16), ("level_sigma2", np.float32, 16)])
MATCH_DTYPE = np.dtype([("x1", np.float32), ("y1", np.float32), ("octave1", np.int32), ("r1", np.float32), ("depth1", np.float32),
                        ("x2", np.float32), ("y2", np.float32), ("octave2", np.int32), ("r2", np.float32), ("depth2", np.float32),
                        ("entropy1", np.float64), ("confidence1", np.float64), ("class1", np.uint8), ("class2", np.uint8),
                        ("pad_", np.uint8, 6)])
assert KEYFRAME_DTYPE.itemsize == C.sizeof(TriKeyFrame) == 272
assert MATCH_DTYPE.itemsize == C.sizeof(TriMatch) == 64

# SIVO_TRI_*: the `continue` of LocalMapping.cc:277-470 that rejected the match, in reference order
STATUS = ("accepted", "low_parallax", "w_zero", "z1", "z2", "reproj1", "reproj2", "zero_dist", "scale", "semantics")
VOID = 255
NO_OBSERVATION, NO_DESCRIPTOR = 1, 2


def keyframe(Rcw, tcw, fx, fy, cx, cy, mb, mbf, scale_factors, level_sigma2):
    """One KEYFRAME_DTYPE record from the pose and the intrinsics: Ow = -Rcw' tcw, Twc = [Rcw' | Ow], invfx = 1 / fx in float."""
    k = np.zeros((), KEYFRAME_DTYPE)
    R = np.asarray(Rcw, np.float32).reshape(3, 3)
    t = np.asarray(tcw, np.float32).reshape(3)
    Ow = (-(R.T.astype(np.float64) @ t.astype(np.float64))).astype(np.float32)
    k["Rcw"], k["tcw"], k["Ow"] = R.reshape(-1), t, Ow
    k["Twc"] = np.concatenate([R.T, Ow[:, None]], axis=1).reshape(-1)
    k["fx"], k["fy"], k["cx"], k["cy"], k["mb"], k["mbf"] = fx, fy, cx, cy, mb, mbf
    k["invfx"], k["invfy"] = np.float32(1.0) / np.float32(fx), np.float32(1.0) / np.float32(fy)
    sf = np.asarray(scale_factors, np.float32).reshape(-1)
    k["nlevels"] = sf.shape[0]
    k["scale_factors"][:sf.shape[0]] = sf
    k["level_sigma2"][:sf.shape[0]] = np.asarray(level_sigma2, np.float32).reshape(-1)
    return k


def _fill(P, p):
    m = np.ascontiguousarray(p["matches"], MATCH_DTYPE).reshape(-1)
    n = m.shape[0]
    for name in ("kf1", "kf2"):
        k = np.ascontiguousarray(p[name], KEYFRAME_DTYPE).reshape(())
        C.memmove(C.addressof(getattr(P, name)), k.ctypes.data, KEYFRAME_DTYPE.itemsize)
    P.ratio_factor = float(np.float32(p["ratio_factor"]))
    cov = np.ascontiguousarray(p["state_cov"], np.float64).reshape(36)
    P.state_cov[:] = cov.tolist()
    P.th_confidence, P.th_entropy = float(p["th_confidence"]), float(p["th_entropy"])
    out = {"status": np.zeros(n, np.uint8), "wP": np.zeros((n, 3), np.float32), "detected_class": np.full(n, VOID, np.uint8)}
    P.matches = m.ctypes.data if n else None
    P.n = n
    for k, a in out.items():
        setattr(P, k, a.ctypes.data if n else None)
    return m, out


def triangulate_batch(problems):
    """k keyframe pairs in one launch.  Each is a dict: kf1, kf2 (KEYFRAME_DTYPE: the current keyframe and the neighbour), matches
    (MATCH_DTYPE), ratio_factor (1.5f * mfScaleFactor) and, of keyframe 1, state_cov (6 x 6), th_confidence, th_entropy.  Returns one
    dict per problem: status (n,) uint8 (an index into STATUS), wP (n, 3) float32, detected_class (n,) uint8.  Each is bit-identical to
    triangulate on that problem."""
    P = (TriProblem * max(len(problems), 1))()
    keep, outs = [], []
    for i, p in enumerate(problems):
        k, o = _fill(P[i], p)
        keep.append(k); outs.append(o)
    check(lib().sivo_triangulate_batch(C.cast(P, C.c_void_p), len(problems)))
    return outs


def triangulate(kf1, kf2, matches, ratio_factor, state_cov, th_confidence, th_entropy):
    """One keyframe pair (sivo_triangulate): see triangulate_batch."""
    P = TriProblem()
    keep, out = _fill(P, {"kf1": kf1, "kf2": kf2, "matches": matches, "ratio_factor": ratio_factor, "state_cov": state_cov,
                          "th_confidence": th_confidence, "th_entropy": th_entropy})
    check(lib().sivo_triangulate(C.byref(P)))
    return out


def refresh_map_points(desc_off, desc, obs_off, obs_ow, pos, ref_ow, level_scale, last_scale, out=None):
    """ComputeDistinctiveDescriptors + UpdateNormalAndDepth of np map points (sivo_mappoint_refresh).  Point p owns the descriptors
    desc[desc_off[p]:desc_off[p + 1]] ((nd, 32) uint8, bad keyframes left out) and the camera centres obs_ow[obs_off[p]:obs_off[p + 1]]
    of all its observations; pos / ref_ow (np, 3), level_scale / last_scale (np,).  Returns a dict: best_idx (np,) int32, max_dist,
    min_dist (np,), normal (np, 3) float32, flags (np,) uint8 (NO_OBSERVATION: the point's entries are left as `out` had them, or 0;
    NO_DESCRIPTOR: best_idx likewise)."""
    desc_off = np.ascontiguousarray(desc_off, np.int64).reshape(-1)
    obs_off = np.ascontiguousarray(obs_off, np.int64).reshape(-1)
    n = desc_off.shape[0] - 1
    if obs_off.shape[0] != n + 1:
        raise ValueError("desc_off and obs_off differ in length")
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    obs_ow = np.ascontiguousarray(obs_ow, np.float32).reshape(-1, 3)
    if n > 0 and (desc.shape[0] < desc_off[-1] or obs_ow.shape[0] < obs_off[-1]):
        raise ValueError("an offset array points past its data")
    per = [np.ascontiguousarray(a, np.float32).reshape(s) for a, s in ((pos, (n, 3)), (ref_ow, (n, 3)), (level_scale, (n,)), (last_scale, (n,)))]
    if out is None:
        out = {"best_idx": np.zeros(n, np.int32), "max_dist": np.zeros(n, np.float32), "min_dist": np.zeros(n, np.float32),
               "normal": np.zeros((n, 3), np.float32)}
    out["flags"] = np.zeros(n, np.uint8)
    ptr = lambda a: a.ctypes.data if a.size else None
    check(lib().sivo_mappoint_refresh(n, ptr(desc_off), ptr(desc), ptr(obs_off), ptr(obs_ow), *[ptr(a) for a in per],
                                      ptr(out["best_idx"]), ptr(out["max_dist"]), ptr(out["min_dist"]), ptr(out["normal"]),
                                      ptr(out["flags"])))
    return out
