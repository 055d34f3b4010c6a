"""The per-frame step of the tracking thread between its two pose optimisations, on arrays: Tracking::SearchLocalPoints (reference
src/orbslam/Tracking.cc:1033-1085) — Frame::isInFrustum (Frame.cc:267-324) over the local map, then
ORBmatcher::SearchByProjection(Frame &, const vector<MapPoint *> &, th).  Host numpy arrays in and out; the work runs on the GPU
(sivo_amd/csrc/frustum.hip, search.hip)."""
import ctypes as C
import ctypes.util

import numpy as np

from ._lib import Frustum, check, lib

IN_VIEW, BEHIND, U_OUTSIDE, V_OUTSIDE, DISTANCE, ANGLE, SKIPPED = range(7)      # SIVO_FRUSTUM_*


def log_scale_factor(scale_factor):
    """mfLogScaleFactor = log(mfScaleFactor) on a float (Frame.cc:118): libm's logf, the function the reference calls — numpy's float32
    log is another implementation and differs from it in the last bit at 1.2f."""
    m = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.logf.restype, m.logf.argtypes = C.c_float, [C.c_float]
    return float(m.logf(float(np.float32(scale_factor))))


def _a(x, dt):
    return np.ascontiguousarray(x, dt)


def _p(x):
    return x.ctypes.data_as(C.c_void_p) if x is not None else None


def frustum(Tcw, fx, fy, cx, cy, bf, bounds, scale_factor, nlevels, cos_limit=0.5):
    """A SivoFrustum: Tcw 4 x 4 (or 3 x 4), bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY), scale_factor = mfScaleFactor."""
    T = np.asarray(Tcw, np.float32)
    fr = Frustum()
    for i, x in enumerate(T[:3, :3].ravel()):
        fr.Rcw[i] = float(x)
    for i, x in enumerate(T[:3, 3]):
        fr.tcw[i] = float(x)
    fr.fx, fr.fy, fr.cx, fr.cy, fr.bf = (float(np.float32(v)) for v in (fx, fy, cx, cy, bf))
    fr.min_x, fr.max_x, fr.min_y, fr.max_y = (float(np.float32(v)) for v in bounds)
    fr.log_scale_factor = log_scale_factor(scale_factor)
    fr.nlevels = int(nlevels)
    fr.cos_limit = float(np.float32(cos_limit))
    return fr


def _points(pos, normal, min_dist, max_dist, skip):
    pos = _a(pos, np.float32).reshape(-1, 3); n = len(pos)
    normal = _a(normal, np.float32).reshape(-1, 3)
    min_dist, max_dist = _a(min_dist, np.float32).ravel(), _a(max_dist, np.float32).ravel()
    skip = None if skip is None else _a(skip, np.uint8).ravel()
    if len(normal) != n or len(min_dist) != n or len(max_dist) != n or (skip is not None and len(skip) != n):
        raise ValueError("the point arrays differ in length")
    return n, pos, normal, min_dist, max_dist, skip


def _track(n, out):
    """The outputs of a cull; `out` pre-fills them (the entries of a point that is not in view stay as they were)."""
    names = (("proj_x", np.float32), ("proj_y", np.float32), ("proj_xr", np.float32), ("view_cos", np.float32), ("level", np.int32))
    res = {}
    for k, dt in names:
        res[k] = np.zeros(n, dt) if out is None or k not in out else _a(out[k], dt).copy()
        if len(res[k]) != n:
            raise ValueError(k + " differs in length from the points")
    return res


def frustum_cull(fr, pos, normal, min_dist, max_dist, skip=None, out=None):
    """Frame::isInFrustum for every point.  Returns status (SIVO_FRUSTUM_*), in_view, proj_x, proj_y, proj_xr, view_cos, level and
    n_in_view; the track fields are written for the points in view only."""
    n, pos, normal, min_dist, max_dist, skip = _points(pos, normal, min_dist, max_dist, skip)
    res = _track(n, out)
    status = np.zeros(n, np.uint8); count = C.c_int32(0)
    check(lib().sivo_frustum_cull(C.byref(fr), n, _p(pos), _p(normal), _p(min_dist), _p(max_dist), _p(skip), _p(status), _p(res["proj_x"]),
                                  _p(res["proj_y"]), _p(res["proj_xr"]), _p(res["view_cos"]), _p(res["level"]), C.byref(count)))
    res.update(status=status, in_view=status == IN_VIEW, n_in_view=count.value)
    return res


def frustum_cull_dev(fr, pos, normal, min_dist, max_dist, skip, status, proj_x, proj_y, proj_xr, view_cos, level, n_in_view=None):
    """frustum_cull on torch tensors of one GPU, on torch's current stream, with no synchronisation (sivo_frustum_cull_dev).  pos, normal
    (n, 3) float32; min_dist, max_dist, proj_*, view_cos (n) float32; skip (n) uint8 or None; status (n) uint8; level (n) int32;
    n_in_view: a one-element int32 tensor that receives the count, or None.  The outputs are written in place, those of a point that
    is not in view are left alone."""
    import torch
    n = int(pos.shape[0])
    f32 = (pos, normal, min_dist, max_dist, proj_x, proj_y, proj_xr, view_cos)
    for t, dt, size in [(t, torch.float32, 3 * n if t is pos or t is normal else n) for t in f32] + \
                       [(status, torch.uint8, n), (level, torch.int32, n)] + ([] if skip is None else [(skip, torch.uint8, n)]) + \
                       ([] if n_in_view is None else [(n_in_view, torch.int32, 1)]):
        if not (t.is_cuda and t.device == pos.device and t.dtype == dt and t.is_contiguous() and t.numel() == size):
            raise ValueError("frustum_cull_dev takes contiguous tensors of one GPU in the documented types and lengths")
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    with torch.cuda.device(pos.device):
        check(lib().sivo_frustum_cull_dev(C.byref(fr), n, ptr(pos), ptr(normal), ptr(min_dist), ptr(max_dist), ptr(skip), ptr(status), ptr(proj_x),
                                          ptr(proj_y), ptr(proj_xr), ptr(view_cos), ptr(level), ptr(n_in_view),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))


def search_local_points(F, fr, pos, normal, min_dist, max_dist, skip, mp_desc, mp_obs, th, nn_ratio, occ_obs, out=None):
    """The cull and SearchByProjection in one call (sivo_search_local_points); F: a matcher.MatchFrame.  Returns what frustum_cull
    returns (n_in_view is nToMatch) and n_matches, match, occ_obs as matcher.search_by_projection_mappoints."""
    n, pos, normal, min_dist, max_dist, skip = _points(pos, normal, min_dist, max_dist, skip)
    res = _track(n, out)
    mp_desc = _a(mp_desc, np.uint8).reshape(-1, 32); mp_obs = _a(mp_obs, np.int32).ravel()
    if len(mp_desc) != n or len(mp_obs) != n:
        raise ValueError("the point arrays differ in length")
    occ = _a(occ_obs, np.int32).copy()
    if len(occ) != F.n:
        raise ValueError("occ_obs differs in length from the frame's keys")
    status = np.zeros(n, np.uint8); match = np.empty(F.n, np.int32); nt, nm = C.c_int32(0), C.c_int32(0)
    check(F._L.sivo_search_local_points(F._h, C.byref(fr), n, _p(pos), _p(normal), _p(min_dist), _p(max_dist), _p(skip), _p(mp_desc),
                                         _p(mp_obs), th, nn_ratio, _p(occ), _p(match), _p(status), _p(res["proj_x"]), _p(res["proj_y"]),
                                         _p(res["proj_xr"]), _p(res["view_cos"]), _p(res["level"]), C.byref(nt), C.byref(nm)))
    res.update(status=status, in_view=status == IN_VIEW, n_in_view=nt.value, n_matches=nm.value, match=match, occ_obs=occ)
    return res
