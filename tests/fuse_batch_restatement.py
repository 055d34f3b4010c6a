"""ORBmatcher::Fuse for every (keyframe, map point) pair up to the choice of the keypoint (reference src/orbslam/ORBmatcher.cc:805-912 with a
keyframe's pose, :958-1039 with a Sim3), restated in numpy scalars: every float operation one rounded float32 operation in the order the
cv::Mat expressions evaluate (rows of R * X summed left to right, then + t; cv::norm and Mat::dot summed in float64), PredictScale through
libm's logf (MapPoint.cc:423-437), Frame::GetFeaturesInArea over the 64 x 48 grid (Frame.cc:326-390) and the sequential first-minimum
scan.  What sivo_fuse_batch must return, pair by pair."""
import ctypes
import ctypes.util

import numpy as np

F32, F64 = np.float32, np.float64
GRID_COLS, GRID_ROWS, TH_LOW, INT_MAX = 64, 48, 50, 2 ** 31 - 1
MATCHED, SKIPPED, BEHIND, IMAGE, DISTANCE, ANGLE, NO_CANDIDATE, TOO_FAR = range(8)
CAMERA_DTYPE = np.dtype([("Rcw", F32, 9), ("tcw", F32, 3), ("Ow", F32, 3), ("fx", F32), ("fy", F32), ("cx", F32), ("cy", F32), ("bf", F32),
                         ("min_x", F32), ("max_x", F32), ("min_y", F32), ("max_y", F32), ("log_scale_factor", F32), ("nlevels", np.int32),
                         ("scw_variant", np.int32)])
U_SENTINEL, LEVEL_SENTINEL = F32(-12345.0), -77

_m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_m.logf.restype, _m.logf.argtypes = ctypes.c_float, [ctypes.c_float]


def logf(x):
    return F32(_m.logf(float(F32(x))))


def predict_scale(max_dist, dist, log_scale_factor, nlevels):
    """MapPoint::PredictScale: ceil(log(ratio) / mfLogScaleFactor) on floats, clamped (a NaN ends at 0)."""
    with np.errstate(all="ignore"):
        ratio = F32(max_dist) / F32(dist)
        c = np.ceil(logf(ratio) / F32(log_scale_factor))
    if c != c or c < 0:
        return 0
    return nlevels - 1 if c >= nlevels else int(c)


def _round_half_away(x):
    x = float(x)
    return int(np.sign(x) * np.floor(abs(x) + 0.5))


class Frame:
    """What the matcher reads of a keyframe: keys (x, y, octave), mvRight or None, descriptors, image bounds, mvScaleFactors,
    mvInvLevelSigma2, and the grid of Frame::AssignFeaturesToGrid (Frame.cc:205-221, PosInGrid :392-404)."""

    def __init__(self, x, y, octave, u_right, desc, bounds, scale, inv_sigma2):
        self.x, self.y, self.octave = np.asarray(x, F32), np.asarray(y, F32), np.asarray(octave, np.int32)
        self.n = len(self.x)
        self.u_right = None if u_right is None else np.asarray(u_right, F32)
        self.desc = np.asarray(desc, np.uint8).reshape(self.n, 32)
        self.bounds = tuple(F32(b) for b in bounds)
        self.scale, self.inv_sigma2 = np.asarray(scale, F32), np.asarray(inv_sigma2, F32)
        self.inv_w = F32(GRID_COLS) / (self.bounds[1] - self.bounds[0])
        self.inv_h = F32(GRID_ROWS) / (self.bounds[3] - self.bounds[2])
        self.grid = [[[] for _ in range(GRID_ROWS)] for _ in range(GRID_COLS)]
        for i in range(self.n):
            px = _round_half_away((self.x[i] - self.bounds[0]) * self.inv_w)
            py = _round_half_away((self.y[i] - self.bounds[2]) * self.inv_h)
            if 0 <= px < GRID_COLS and 0 <= py < GRID_ROWS:
                self.grid[px][py].append(i)

    def features_in_area(self, x, y, r):
        """GetFeaturesInArea(x, y, r) without level arguments: the cells column by column, the keys of a cell in index order."""
        x, y, r = F32(x), F32(y), F32(r)
        out = []
        with np.errstate(all="ignore"):
            c0 = max(0, int(np.floor((x - self.bounds[0] - r) * self.inv_w)))
            if c0 >= GRID_COLS:
                return out
            c1 = min(GRID_COLS - 1, int(np.ceil((x - self.bounds[0] + r) * self.inv_w)))
            if c1 < 0:
                return out
            r0 = max(0, int(np.floor((y - self.bounds[2] - r) * self.inv_h)))
            if r0 >= GRID_ROWS:
                return out
            r1 = min(GRID_ROWS - 1, int(np.ceil((y - self.bounds[2] + r) * self.inv_h)))
            if r1 < 0:
                return out
        for ix in range(c0, c1 + 1):
            for iy in range(r0, r1 + 1):
                for i in self.grid[ix][iy]:
                    if abs(self.x[i] - x) < r and abs(self.y[i] - y) < r:
                        out.append(i)
        return out


def project(cam, X, Pn, min_dist, max_dist):
    """The per-point tests (:814-849 / :966-1003): (status, u, v, ur, level); status None when the pair goes on to the window query."""
    R, t, Ow = cam["Rcw"].reshape(3, 3), cam["tcw"], cam["Ow"]
    X, Pn = np.asarray(X, F32), np.asarray(Pn, F32)
    with np.errstate(all="ignore"):
        pc = []
        for r in range(3):
            s = R[r, 0] * X[0]
            s = s + R[r, 1] * X[1]
            s = s + R[r, 2] * X[2]
            pc.append(F32(s + t[r]))
        if pc[2] < F32(0.0):
            return BEHIND, None, None, None, None
        invz = F32(1.0) / pc[2]
        x, y = pc[0] * invz, pc[1] * invz
        u = cam["fx"] * x + cam["cx"]
        v = cam["fy"] * y + cam["cy"]
        if not (u >= cam["min_x"] and u < cam["max_x"] and v >= cam["min_y"] and v < cam["max_y"]):
            return IMAGE, None, None, None, None
        ur = u - cam["bf"] * invz
        PO = [F32(X[i] - Ow[i]) for i in range(3)]
        s2 = F64(PO[0]) * F64(PO[0])
        s2 = s2 + F64(PO[1]) * F64(PO[1])
        s2 = s2 + F64(PO[2]) * F64(PO[2])
        dist = F32(np.sqrt(s2))
        if dist < F32(0.8) * F32(min_dist) or dist > F32(1.2) * F32(max_dist):
            return DISTANCE, None, None, None, None
        dot = F64(PO[0]) * F64(Pn[0])
        dot = dot + F64(PO[1]) * F64(Pn[1])
        dot = dot + F64(PO[2]) * F64(Pn[2])
        if dot < F64(0.5) * F64(dist):
            return ANGLE, None, None, None, None
        level = predict_scale(max_dist, dist, cam["log_scale_factor"], int(cam["nlevels"]))
    return None, F32(u), F32(v), F32(ur), level


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def scan(frame, u, v, ur, level, desc, th, scw_variant):
    """The window query and the candidate loop (:852-912 / :1006-1039): (status, best_idx, best_dist)."""
    radius = F32(th) * frame.scale[level]
    idxs = frame.features_in_area(u, v, radius)
    best_dist, best = (INT_MAX if scw_variant else 256), -1
    if not idxs:
        return NO_CANDIDATE, -1, best_dist
    for i in idxs:
        lvl = int(frame.octave[i])
        if lvl < level - 1 or lvl > level:
            continue
        if not scw_variant:
            ex, ey = u - frame.x[i], v - frame.y[i]
            kur = F32(-1.0) if frame.u_right is None else frame.u_right[i]
            if kur >= 0:
                er = ur - kur
                e2 = ex * ex + ey * ey + er * er
                if F64(F32(e2 * frame.inv_sigma2[lvl])) > 7.8:
                    continue
            else:
                e2 = ex * ex + ey * ey
                if F64(F32(e2 * frame.inv_sigma2[lvl])) > 5.99:
                    continue
        d = hamming(desc, frame.desc[i])
        if d < best_dist:
            best_dist, best = d, i
    if best_dist <= TH_LOW:
        return MATCHED, best, best_dist
    # (from INT_MAX a distance of 256 is taken and then fails TH_LOW; sivo_fuse reports that as no comparison, and so does the batch)
    return TOO_FAR, -1, (INT_MAX if scw_variant and best_dist == 256 else best_dist)


def fuse_batch(frames, cams, pos, normal, min_dist, max_dist, mp_desc, th, skip_point=None, skip_pair=None):
    """Every pair: dict of (n_kf, n_mp) arrays best_idx, best_dist, status, u, v, ur, level (the last four at their sentinels where the
    pair did not reach the window query)."""
    K, N = len(frames), len(pos)
    cams = np.asarray(cams, CAMERA_DTYPE)
    mp_desc = np.asarray(mp_desc, np.uint8).reshape(N, 32)
    out = dict(best_idx=np.full((K, N), -1, np.int32), best_dist=np.zeros((K, N), np.int32), status=np.zeros((K, N), np.uint8),
               u=np.full((K, N), U_SENTINEL, F32), v=np.full((K, N), U_SENTINEL, F32), ur=np.full((K, N), U_SENTINEL, F32),
               level=np.full((K, N), LEVEL_SENTINEL, np.int32))
    for k in range(K):
        cam = cams[k]
        none = INT_MAX if cam["scw_variant"] else 256
        for i in range(N):
            out["best_dist"][k, i] = none
            if (skip_point is not None and skip_point[i]) or (skip_pair is not None and np.asarray(skip_pair).reshape(K, N)[k, i]):
                out["status"][k, i] = SKIPPED
                continue
            st, u, v, ur, level = project(cam, pos[i], normal[i], min_dist[i], max_dist[i])
            if st is not None:
                out["status"][k, i] = st
                continue
            st, best, dist = scan(frames[k], u, v, ur, level, mp_desc[i], th, int(cam["scw_variant"]))
            out["status"][k, i], out["best_idx"][k, i], out["best_dist"][k, i] = st, best, dist
            out["u"][k, i], out["v"][k, i], out["ur"][k, i], out["level"][k, i] = u, v, ur, level
    return out
