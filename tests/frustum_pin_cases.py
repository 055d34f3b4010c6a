"""Inputs of the frustum-cull pin (tests/test_pin_frustum.py, tests/test_gpu_frustum.py, tests/golden/make_frustum_reference.py), built
without reading the reference, and the binding of the host program tests/frustum_prog.cpp.

Three groups of map points:
  probes   the 600 points of pin_frame_common.probes(352, 1024, 5) under that function's pose: every exit of Frame::isInFrustum and
           every predicted level;
  sweep    30 visible points, three for each k = -1 .. nlevels, each with max_dist stepped through 48 consecutive floats from 24 ulps
           below dist * 1.2^k to 23 above (1440 points): the level changes from k to k + 1 inside the 21 rows of k = 0 .. nlevels - 2, the
           other 9 rows are clamped, and the k = -1 rows straddle the `dist > 1.2f * maxDist` gate.  Normals along PO, min_dist =
           max_dist / 100, the probes' pose;
  hand     a few points under a pose of its own (R = I, t = -0): PcZ exactly +0 and -0, u exactly mnMinX and mnMaxX, v exactly mnMinY and
           mnMaxY (in view: the comparisons are strict), viewCos on either side of the limit, two visible points the caller skips.
The expected values are the reference's own Frame::isInFrustum (oracle/_ref/libref_frame.so through pin_frame_common.reference_frame),
recorded in tests/golden/frustum_reference.npz."""
import functools
import os

import numpy as np

import host_prog
import pin_frame_common as FC

ROOT = FC.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "frustum_reference.npz")
ROWS, COLS = 352, 1024
BOUNDS = (0.0, float(COLS), 0.0, float(ROWS))          # mnMinX, mnMaxX, mnMinY, mnMaxY without distortion (Frame.cc:436-440)
SCALE_FACTOR, NLEVELS, COS_LIMIT = 1.2, 8, 0.5
SCENE = "kitti-crop-d12|2000/8"
GROUPS = ("probes", "sweep", "hand")
F32 = np.float32
FRUSTUM_DTYPE = np.dtype([("Rcw", F32, 9), ("tcw", F32, 3), ("fx", F32), ("fy", F32), ("cx", F32), ("cy", F32), ("bf", F32), ("min_x", F32),
                          ("max_x", F32), ("min_y", F32), ("max_y", F32), ("log_scale_factor", F32), ("nlevels", np.int32), ("cos_limit", F32)])
SENTINEL, LEVEL_SENTINEL = F32(-12345.0), -77
TRACK = ("proj_x", "proj_y", "proj_xr", "view_cos")


def scale_factors():
    """mvScaleFactors as ORBextractor builds them: a running float product."""
    s = np.ones(NLEVELS, F32)
    for i in range(1, NLEVELS):
        s[i] = s[i - 1] * F32(SCALE_FACTOR)
    return s


def log_scale_factor():
    from sivo_amd import tracking
    return tracking.log_scale_factor(SCALE_FACTOR)


def frustum_record(Tcw, cos_limit=COS_LIMIT, nlevels=NLEVELS):
    r = np.zeros((), FRUSTUM_DTYPE)
    T = np.asarray(Tcw, F32)
    r["Rcw"] = T[:3, :3].ravel(); r["tcw"] = T[:3, 3]
    r["fx"], r["fy"], r["cx"], r["cy"], r["bf"] = FC.FX, FC.FY, FC.CX, FC.CY, FC.BF
    r["min_x"], r["max_x"], r["min_y"], r["max_y"] = BOUNDS
    r["log_scale_factor"] = log_scale_factor(); r["nlevels"] = nlevels; r["cos_limit"] = cos_limit
    return r


# ---------------------------------------------------------------------------------------------------------------------
# the arithmetic of the projection in numpy float32, only to PLACE the hand-made points (every step one rounded float operation)
# ---------------------------------------------------------------------------------------------------------------------
def _camera(T, X):
    T = np.asarray(T, F32); X = np.asarray(X, F32)
    out = []
    for r in range(3):
        s = T[r, 0] * X[0]
        s = s + T[r, 1] * X[1]
        s = s + T[r, 2] * X[2]
        out.append(s + T[r, 3])
    return out


def _project(T, X):
    pc = _camera(T, X)
    with np.errstate(all="ignore"):
        invz = F32(1.0) / pc[2]
        return F32(FC.FX) * pc[0] * invz + F32(FC.CX), F32(FC.FY) * pc[1] * invz + F32(FC.CY)


def _centre(T):
    T = np.asarray(T, F32)
    return np.array([F32(-sum(np.float64(T[r, c]) * np.float64(T[r, 3]) for r in range(3))) for c in range(3)], F32)


def _scan(make, value, target, what):
    """The float nearest `value` (within 64 ulps) for which make(x) == target exactly, or None."""
    x0 = F32(value)
    for step in range(64):
        for x in ((x0,) if step == 0 else (_ulps(x0, step), _ulps(x0, -step))):
            if make(x) == F32(target):
                return F32(x)
    return None


def _on_bound(axis, target, what):
    """A point in front of the camera whose projection along `axis` is exactly `target`.  The product fx * X moves by 0.7 or by 1.4 of its
    ulps per ulp of X, depending on the two mantissas: depths are tried until every float of the product is reached."""
    f, c, other = (FC.FX, FC.CX, 0.5 * ROWS) if axis == 0 else (FC.FY, FC.CY, 0.5 * COLS)
    for z in (8.0, 6.0, 7.0, 5.0, 3.0, 12.0, 10.0, 9.0, 11.0):
        z = F32(z)
        fixed = F32((other - (FC.CY if axis == 0 else FC.CX)) * float(z) / (FC.FY if axis == 0 else FC.FX))
        point = (lambda x: (x, fixed, z)) if axis == 0 else (lambda y: (fixed, y, z))
        x = _scan(lambda x: _project(HAND_POSE, point(x))[axis], (target - c) * float(z) / f, target, what)
        if x is not None:
            return np.array(point(x), F32)
    raise AssertionError("no float gives " + what)


def _ulps(x, k):
    x = np.asarray(x, F32)
    i = x.view(np.int32).astype(np.int64)
    i = np.where(i < 0, -(i & 0x7FFFFFFF), i) + k                  # sign-magnitude -> a line
    return np.where(i < 0, (-i) | 0x80000000, i).astype(np.uint32).view(F32)


HAND_POSE = np.eye(4, dtype=F32)
HAND_POSE[:3, 3] = F32(-0.0)
HAND_NAMES = ("z_plus_zero", "z_minus_zero", "u_min", "u_max", "v_min", "v_max", "u_below_min", "u_above_max", "v_below_min", "v_above_max",
              "cos_above", "cos_below", "skipped_0", "skipped_1", "plain")


def _hand():
    T = HAND_POSE
    z = F32(8.0)
    mid_x, mid_y = F32((0.5 * COLS - FC.CX) * 8.0 / FC.FX), F32((0.5 * ROWS - FC.CY) * 8.0 / FC.FY)
    u_of = lambda p: _project(T, p)[0]
    v_of = lambda p: _project(T, p)[1]
    pts = {"z_plus_zero": (0.5, 0.25, 0.0), "z_minus_zero": (-0.5, -0.25, -0.0), "plain": (mid_x, mid_y, z),
           "u_min": _on_bound(0, BOUNDS[0], "u_min"), "u_max": _on_bound(0, BOUNDS[1], "u_max"),
           "v_min": _on_bound(1, BOUNDS[2], "v_min"), "v_max": _on_bound(1, BOUNDS[3], "v_max"),
           "cos_above": (0.0, 0.0, 10.0), "cos_below": (0.0, 0.0, 10.0), "skipped_0": (mid_x, mid_y, z), "skipped_1": (0.1, 0.1, 5.0)}
    for name, axis, k in (("u_below_min", 0, -2), ("u_above_max", 0, 2), ("v_below_min", 1, -2), ("v_above_max", 1, 2)):
        q = np.array(pts[{"u_below_min": "u_min", "u_above_max": "u_max", "v_below_min": "v_min", "v_above_max": "v_max"}[name]], F32)
        q[axis] = _ulps(q[axis], k)                                    # 2 ulps of the coordinate outside
        pts[name] = q
    pos = np.array([pts[k] for k in HAND_NAMES], F32)
    assert np.signbit(pos[1, 2]) and not np.signbit(pos[0, 2])
    # the boundary points stand exactly on the bounds, their neighbours 2 ulps of the coordinate outside
    assert u_of(pos[2]) == BOUNDS[0] and u_of(pos[3]) == BOUNDS[1] and v_of(pos[4]) == BOUNDS[2] and v_of(pos[5]) == BOUNDS[3]
    assert u_of(pos[6]) < BOUNDS[0] and u_of(pos[7]) > BOUNDS[1] and v_of(pos[8]) < BOUNDS[2] and v_of(pos[9]) > BOUNDS[3]
    PO = pos - _centre(T)
    dist = np.linalg.norm(PO.astype(np.float64), axis=1)
    normal = (PO / np.maximum(dist, 1e-6)[:, None]).astype(F32)
    for name, c in (("cos_above", 0.501), ("cos_below", 0.499)):       # on the optical axis viewCos is the normal's z
        normal[HAND_NAMES.index(name)] = (np.sqrt(1 - c * c), 0.0, c)
    max_dist = (dist * 2.0).astype(F32); max_dist[:2] = 1.0
    skip = np.array([k.startswith("skipped") for k in HAND_NAMES], np.uint8)
    return dict(Tcw=T.copy(), pos=pos, normal=normal, min_dist=(max_dist / F32(3.58)).astype(F32), max_dist=max_dist, skip=skip)


SWEEP_KS = tuple(range(-1, NLEVELS + 1))
SWEEP_STEPS = np.arange(-24, 24)


def _sweep(Tcw):
    rng = np.random.default_rng(11)
    rows = 3 * len(SWEEP_KS)
    z = rng.uniform(4, 40, rows); u = rng.uniform(40, COLS - 40, rows); v = rng.uniform(40, ROWS - 40, rows)
    cam = np.stack([(u - FC.CX) * z / FC.FX, (v - FC.CY) * z / FC.FY, z], 1)
    T = np.asarray(Tcw, np.float64)
    base = ((cam - T[:3, 3]) @ T[:3, :3]).astype(F32)                   # world = R^T (cam - t): visible by construction
    PO = base.astype(np.float64) - _centre(Tcw).astype(np.float64)
    dist = np.sqrt((PO * PO).sum(1)).astype(F32)                        # cv::norm: the sum in double, rounded once
    k = np.repeat(SWEEP_KS, 3)
    centre = (dist.astype(np.float64) * 1.2 ** k).astype(F32)
    max_dist = _ulps(centre[:, None], SWEEP_STEPS[None, :]).astype(F32)          # rows x 48
    n = rows * len(SWEEP_STEPS)
    pos = np.repeat(base, len(SWEEP_STEPS), axis=0)
    normal = np.repeat((PO / np.sqrt((PO * PO).sum(1))[:, None]).astype(F32), len(SWEEP_STEPS), axis=0)
    max_dist = max_dist.reshape(n)
    return dict(Tcw=np.asarray(Tcw, F32).copy(), pos=pos, normal=normal, min_dist=(max_dist / F32(100)).astype(F32), max_dist=max_dist,
                skip=np.zeros(n, np.uint8), k=np.repeat(k, len(SWEEP_STEPS)))


_INPUTS = {}


def inputs(group):
    if not _INPUTS:
        pr = FC.probes(ROWS, COLS, 5)
        assert pr["cos_limit"] == COS_LIMIT
        _INPUTS["probes"] = dict(Tcw=pr["Tcw"], pos=pr["pos"], normal=pr["normal"], min_dist=pr["min_dist"], max_dist=pr["max_dist"],
                                 skip=np.zeros(len(pr["pos"]), np.uint8))
        _INPUTS["sweep"] = _sweep(pr["Tcw"])
        _INPUTS["hand"] = _hand()
        for g in _INPUTS.values():
            for key in ("pos", "normal", "min_dist", "max_dist"):
                g[key] = np.ascontiguousarray(g[key], F32)
                g[key].setflags(write=False)
    return _INPUTS[group]


# ---------------------------------------------------------------------------------------------------------------------
# the reference: live, and as recorded
# ---------------------------------------------------------------------------------------------------------------------
def reference_present():
    return os.path.exists(FC.REF_LIB)


_SCENE = []


def reference(group, cos_limit=COS_LIMIT, relax_distance=False):
    """Frame::isInFrustum of the reference library on a group's points (skip is the caller's business and not applied)."""
    if not _SCENE:
        _SCENE.append(FC.scenes()[SCENE])
    g = inputs(group)
    pr = FC.probes(ROWS, COLS, 5)
    n = len(g["pos"])
    pr.update(Tcw=g["Tcw"], pos=g["pos"], normal=g["normal"], cos_limit=cos_limit,
              min_dist=np.zeros(n, F32) if relax_distance else g["min_dist"], max_dist=np.full(n, np.inf, F32) if relax_distance else g["max_dist"])
    pr["qx"], pr["qy"], pr["qr"], pr["qmin"], pr["qmax"] = (pr[k][:1].copy() for k in ("qx", "qy", "qr", "qmin", "qmax"))
    left, right, classes, cfg = _SCENE[0]
    assert cfg[1] == SCALE_FACTOR and cfg[2] == NLEVELS and left.shape == (ROWS, COLS)
    r = FC.reference_frame(left, right, classes, cfg, pr)
    assert tuple(float(b) for b in r["bounds"]) == BOUNDS
    return {"in_view": r["in_view"].copy(), "track": r["track"].copy(), "level": r["level"].copy()}


_FIXTURE = {}


def recorded(group):
    if not _FIXTURE:
        with np.load(GOLDEN) as z:
            _FIXTURE.update({k: z[k] for k in z.files})
    return {k: _FIXTURE[group + "." + k] for k in ("in_view", "track", "level")}


def expected_status_in_view(group, want):
    """in view as the caller sees it: the reference's answer, except where the caller skipped the point."""
    return (want["in_view"] != 0) & (inputs(group)["skip"] == 0)


def same_as_reference(group, got, want, what):
    """status 0 exactly where the reference says in view; the four track floats and the level bit for bit on those; the sentinels
    everywhere else.  No tolerance, no case left out."""
    inv = expected_status_in_view(group, want)
    assert np.array_equal(got["status"] == 0, inv), (what, group, np.flatnonzero((got["status"] == 0) != inv)[:10])
    assert np.array_equal(got["status"] == 6, inputs(group)["skip"] != 0), (what, group)
    for c, k in enumerate(TRACK):
        a, b = np.ascontiguousarray(got[k], F32).view(np.uint32), np.ascontiguousarray(want["track"][:, c], F32).view(np.uint32)
        assert np.array_equal(a[inv], b[inv]), (what, group, k, np.flatnonzero(inv & (a != b))[:10])
        assert (got[k][~inv].view(np.uint32) == SENTINEL.view(np.uint32)).all(), (what, group, k, "an entry of a point out of view was written")
    assert np.array_equal(got["level"][inv], want["level"][inv]), (what, group, "level", np.flatnonzero(inv & (got["level"] != want["level"]))[:10])
    assert (got["level"][~inv] == LEVEL_SENTINEL).all(), (what, group, "level of a point out of view was written")
    assert int(got["n_in_view"]) == int(inv.sum())


# ---------------------------------------------------------------------------------------------------------------------
# the host program
# ---------------------------------------------------------------------------------------------------------------------
run_prog = functools.partial(host_prog.run, timeout=120)              # (the tests' assertions call it by this name)


def points_blob(g, n=None):
    n = len(g["pos"]) if n is None else n
    return b"".join([np.array([n], np.int64).tobytes(), g["pos"][:n].tobytes(), g["normal"][:n].tobytes(), g["min_dist"][:n].tobytes(),
                     g["max_dist"][:n].tobytes()])


def host_cull(exe, tmp_path, group, mode="cull", n=None, nlevels=NLEVELS):
    g = inputs(group)
    n = len(g["pos"]) if n is None else n
    raw = run_prog(exe, tmp_path, mode, frustum_record(g["Tcw"], nlevels=nlevels).tobytes() + points_blob(g, n) + g["skip"][:n].tobytes())
    assert len(raw) == 21 * n + (4 if mode == "cull" else 0)
    res = {"status": np.frombuffer(raw, np.uint8, n), "level": np.frombuffer(raw, np.int32, n, 17 * n)}
    for c, k in enumerate(TRACK):
        res[k] = np.frombuffer(raw, F32, n, n + 4 * n * c)
    if mode == "cull":
        res["n_in_view"] = int(np.frombuffer(raw, np.int32, 1, 21 * n)[0])
    else:                                                                # mbTrackInView -> the status the comparison reads
        res["status"] = np.where(res["status"] != 0, 0, np.where(g["skip"][:n] != 0, 6, 1)).astype(np.uint8)
        res["n_in_view"] = int((res["status"] == 0).sum())
    return res
