"""Python mirror of the per-edge linearisation behind SIVO::Optimizer (reference
src/orbslam/Optimizer.cc:318-409, 651-755) over the C ABI."""
import ctypes as C
import math

import numpy as np
import torch

from ._lib import BaOptions, Edge, Sim3Edge, Sim3Match, Sim3Problem, check, lib

EDGE_DTYPE = np.dtype([("pose", np.int32), ("point", np.int32), ("stereo", np.int32), ("pad_", np.int32),
                       ("obs", np.float64, 3), ("inv_sigma2", np.float64)])
assert EDGE_DTYPE.itemsize == C.sizeof(Edge) == 48
SIM3_MATCH_DTYPE = np.dtype([("obs1", np.float64, 2), ("inv_sigma2_1", np.float64), ("obs2", np.float64, 2),
                             ("inv_sigma2_2", np.float64), ("x1c", np.float64, 3), ("x2c", np.float64, 3)])
assert SIM3_MATCH_DTYPE.itemsize == C.sizeof(Sim3Match) == 96
SIM3_EDGE_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("meas", np.float64, 8)])
assert SIM3_EDGE_DTYPE.itemsize == C.sizeof(Sim3Edge) == 72
TH_HUBER_MONO = math.sqrt(5.991)     # Optimizer.cc:647
TH_HUBER_STEREO = math.sqrt(7.815)   # Optimizer.cc:648


def linearize(poses, points, edges, intr, delta_mono=TH_HUBER_MONO, delta_stereo=TH_HUBER_STEREO):
    """Host arrays in/out (numpy)."""
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    edges = np.ascontiguousarray(edges, EDGE_DTYPE)
    intr = (C.c_double * 5)(*[float(v) for v in intr])
    nE = edges.shape[0]
    out = {"err": np.empty((nE, 3)), "Jx": np.empty((nE, 3, 3)), "Jp": np.empty((nE, 3, 6)), "chi2": np.empty(nE),
           "rho": np.empty(nE), "w": np.empty(nE), "depth_ok": np.empty(nE, np.uint8)}
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    check(lib().sivo_ba_linearize(p(poses), poses.shape[0], p(points), points.shape[0], p(edges), nE, intr,
                                  delta_mono, delta_stereo, p(out["err"]), p(out["Jx"]), p(out["Jp"]), p(out["chi2"]),
                                  p(out["rho"]), p(out["w"]), p(out["depth_ok"])))
    return out


def linearize_dev(d_poses, d_points, d_edges_u8, n_edges, intr, out, delta_mono=TH_HUBER_MONO,
                  delta_stereo=TH_HUBER_STEREO):
    """Device-resident: d_edges_u8 is a cuda uint8 tensor holding n_edges SivoEdge records; `out` a dict of
    preallocated cuda tensors (err, Jx, Jp, chi2, rho, w, depth_ok)."""
    intr = (C.c_double * 5)(*[float(v) for v in intr])
    g = lambda k: out[k].data_ptr() if out.get(k) is not None else None
    check(lib().sivo_ba_linearize_dev(d_poses.data_ptr(), d_points.data_ptr(), d_edges_u8.data_ptr(), n_edges, intr,
                                      delta_mono, delta_stereo, g("err"), g("Jx"), g("Jp"), g("chi2"), g("rho"), g("w"),
                                      g("depth_ok"), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def _intr(intr):
    return (C.c_double * 5)(*[float(v) for v in intr])


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


BA_SOLVERS = {"auto": 0, "dense": 1, "sparse": 2}      # SIVO_BA_SOLVER_*


def _ba_options(solver):
    """The SivoBaOptions of a solver name; None for "auto" (the plain entry points)."""
    if solver not in BA_SOLVERS:
        raise ValueError(f"solver must be one of {sorted(BA_SOLVERS)}, not {solver!r}")
    return None if solver == "auto" else BaOptions(C.sizeof(BaOptions), BA_SOLVERS[solver])


def ba_optimize(poses, fixed, points, edges, intr, iterations, level=None, robust=None,
                delta_mono=float(np.sqrt(np.float32(5.991))), delta_stereo=float(np.sqrt(np.float32(7.815))), stop=None, solver="auto"):
    """One g2o optimize(iterations) call (Optimizer::BundleAdjustment, reference Optimizer.cc:49-271) on arrays.  solver: how the
    reduced camera system is solved, "dense", "sparse" or "auto" (sparse from 64 free keyframes on, or when the dense edge table would
    be refused)."""
    poses = np.array(poses, np.float64).reshape(-1, 12).copy(); points = np.array(points, np.float64).reshape(-1, 3).copy()
    fixed = np.ascontiguousarray(fixed, np.uint8); edges = np.ascontiguousarray(edges, EDGE_DTYPE)
    nE = edges.shape[0]
    level = None if level is None else np.ascontiguousarray(level, np.uint8)
    robust = None if robust is None else np.ascontiguousarray(robust, np.uint8)
    err = np.zeros((nE, 3)); hpp = np.zeros((int((fixed == 0).sum()), 6, 6)); n = C.c_int(0); tr = C.c_int(0)
    args = (_vp(poses), _vp(fixed), poses.shape[0], _vp(points), points.shape[0], _vp(edges), nE, _intr(intr), delta_mono, delta_stereo,
            _vp(level), _vp(robust), iterations, C.addressof(stop) if stop is not None else None, _vp(err), _vp(hpp), C.byref(n), C.byref(tr))
    opts = _ba_options(solver)
    check(lib().sivo_ba_optimize(*args) if opts is None else lib().sivo_ba_optimize_opts(*args, C.addressof(opts)))
    return {"poses": poses, "points": points, "err": err, "hpp": hpp, "iterations": n.value, "trials": tr.value}


def local_ba(poses, fixed, points, edges, intr, cov_pose=-1, stop=None, solver="auto"):
    """Optimizer::LocalBundleAdjustment (reference Optimizer.cc:757-926) on arrays; `stop` is a ctypes c_uint8 (the reference's bool *pbStopFlag) or None;
    solver as in ba_optimize."""
    poses = np.array(poses, np.float64).reshape(-1, 12).copy(); points = np.array(points, np.float64).reshape(-1, 3).copy()
    fixed = np.ascontiguousarray(fixed, np.uint8); edges = np.ascontiguousarray(edges, EDGE_DTYPE)
    nE = edges.shape[0]
    outlier = np.zeros(nE, np.uint8); cov = np.zeros((6, 6)); ok = C.c_int(0); n = C.c_int(0); tr = C.c_int(0)
    args = (_vp(poses), _vp(fixed), poses.shape[0], _vp(points), points.shape[0], _vp(edges), nE, _intr(intr),
            C.addressof(stop) if stop is not None else None, _vp(outlier), cov_pose, _vp(cov), C.byref(ok), C.byref(n), C.byref(tr))
    opts = _ba_options(solver)
    check(lib().sivo_local_ba(*args) if opts is None else lib().sivo_local_ba_opts(*args, C.addressof(opts)))
    return {"poses": poses, "points": points, "outlier": outlier, "cov": cov, "cov_ok": bool(ok.value),
            "iterations": n.value, "trials": tr.value}


def ba_analyze(fixed, n_points, edges, solver="auto"):
    """What the sparse path of the bundle adjustment plans for a problem, host only: free poses, blocks of S below the diagonal,
    off-diagonal blocks of L, nnz(L) (scalars, lower triangle), flops of one numeric factorisation, elimination-tree levels,
    contribution pairs, and the path `solver` takes (1 dense, 2 sparse)."""
    fixed = np.ascontiguousarray(fixed, np.uint8); edges = np.ascontiguousarray(edges, EDGE_DTYPE)
    out = np.zeros(8, np.int64)
    opts = _ba_options(solver)
    check(lib().sivo_ba_analyze(_vp(fixed), fixed.shape[0], int(n_points), _vp(edges), edges.shape[0],
                                None if opts is None else C.addressof(opts), _vp(out)))
    return dict(zip(("free_poses", "s_blocks", "l_blocks", "nnz_l", "flops", "levels", "pairs", "path"), (int(v) for v in out)))


def pose_optimize(pose0, points, edges, intr):
    """Optimizer::PoseOptimization (reference Optimizer.cc:273-491) on arrays."""
    pose0 = np.ascontiguousarray(pose0, np.float64).reshape(12); points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    edges = np.ascontiguousarray(edges, EDGE_DTYPE)
    nE = edges.shape[0]
    outlier = np.zeros(nE, np.uint8); pose = np.empty(12); cov = np.zeros((6, 6)); chi2 = np.zeros(nE)
    ok = C.c_int(0); inl = C.c_int(0); n = C.c_int(0); tr = C.c_int(0)
    check(lib().sivo_pose_optimize(_vp(pose0), _vp(points), points.shape[0], _vp(edges), nE, _intr(intr), _vp(outlier),
                                   _vp(pose), _vp(cov), C.byref(ok), _vp(chi2), C.byref(inl), C.byref(n), C.byref(tr)))
    return {"pose": pose, "outlier": outlier, "cov": cov, "cov_ok": bool(ok.value), "chi2": chi2, "inliers": inl.value,
            "iterations": n.value, "trials": tr.value}


def _sim3_args(s12, k1, k2, matches):
    s12 = np.array(s12, np.float64).reshape(8).copy()
    k1 = (C.c_double * 4)(*[float(v) for v in k1]); k2 = (C.c_double * 4)(*[float(v) for v in k2])
    return s12, k1, k2, np.ascontiguousarray(matches, SIM3_MATCH_DTYPE)


def sim3_optimize(s12, k1, k2, matches, th2=10.0, fix_scale=True):
    """Optimizer::OptimizeSim3 (reference Optimizer.cc:1236-1449) from the built graph on: s12 = qx qy qz qw tx ty tz s (g2o::Sim3),
    k1 / k2 = fx fy cx cy, matches = SIM3_MATCH_DTYPE records.  Returns the optimised s12 (the input when fewer than 10 pairs survive),
    the outlier flags (the vpMatches1 entries the reference nulls), the inlier count (its return value), the chi2 values the last
    test read and the iteration / trial counts of both optimize() calls."""
    s12, k1, k2, m = _sim3_args(s12, k1, k2, matches)
    n = m.shape[0]
    outlier = np.zeros(n, np.uint8); c12 = np.zeros(n); c21 = np.zeros(n)
    inl = C.c_int(0); it = C.c_int(0); tr = C.c_int(0)
    check(lib().sivo_sim3_optimize(_vp(s12), k1, k2, _vp(m), n, float(th2), int(bool(fix_scale)), _vp(outlier), C.byref(inl),
                                   _vp(c12), _vp(c21), C.byref(it), C.byref(tr)))
    return {"s12": s12, "outlier": outlier, "inliers": inl.value, "chi2_12": c12, "chi2_21": c21, "iterations": it.value,
            "trials": tr.value}


def sim3_optimize_batch(problems):
    """k independent OptimizeSim3 problems in one launch (one workgroup each): `problems` is a list of dicts with the arguments of
    sim3_optimize (s12, k1, k2, matches, optional th2 / fix_scale).  Returns a list of the dicts sim3_optimize returns; each is
    bit-identical to the single call on the same problem."""
    P = (Sim3Problem * max(len(problems), 1))()
    keep, out = [], []
    for i, p in enumerate(problems):
        s12, k1, k2, m = _sim3_args(p["s12"], p["k1"], p["k2"], p["matches"])
        n = m.shape[0]
        r = {"s12": s12, "outlier": np.zeros(n, np.uint8), "chi2_12": np.zeros(n), "chi2_21": np.zeros(n)}
        P[i].s12[:] = list(s12); P[i].k1[:] = list(k1); P[i].k2[:] = list(k2)
        P[i].matches = m.ctypes.data if n else None; P[i].n = n
        P[i].th2 = float(p.get("th2", 10.0)); P[i].fix_scale = int(bool(p.get("fix_scale", True)))
        P[i].outlier = r["outlier"].ctypes.data if n else None
        P[i].chi2_12 = r["chi2_12"].ctypes.data if n else None; P[i].chi2_21 = r["chi2_21"].ctypes.data if n else None
        keep.append(m); out.append(r)
    check(lib().sivo_sim3_optimize_batch(C.cast(P, C.c_void_p), len(problems)))
    for i, r in enumerate(out):
        r["s12"] = np.array(P[i].s12[:], np.float64)
        r["inliers"] = P[i].n_inliers; r["iterations"] = P[i].iterations; r["trials"] = P[i].trials
    return out


def _graph_args(siw, fixed, edges):
    siw = np.array(siw, np.float64).reshape(-1, 8).copy()
    n = siw.shape[0]
    fixed = np.ascontiguousarray(np.asarray(fixed, bool).reshape(n), np.uint8)
    return siw, fixed, np.ascontiguousarray(edges, SIM3_EDGE_DTYPE)


def essential_graph_optimize(siw, fixed, edges, fix_scale=True, iterations=20):
    """Optimizer::OptimizeEssentialGraph (reference Optimizer.cc:928-1180) from the built graph on: siw (n, 8) = qx qy qz qw tx ty tz s
    of every vertex (g2o::Sim3), fixed (n,) bool, edges = SIM3_EDGE_DTYPE records (i = vertex 0, j = vertex 1, meas = Sji).  Returns
    the optimised siw (a new array), the chi2 (sum of e'e) at the start and at the end, and the LM iteration / trial counts."""
    siw, fixed, e = _graph_args(siw, fixed, edges)
    chi2 = np.zeros(2)
    it = C.c_int(0); tr = C.c_int(0)
    check(lib().sivo_essential_graph_optimize(_vp(siw), _vp(fixed), siw.shape[0], _vp(e), e.shape[0], int(bool(fix_scale)),
                                              int(iterations), _vp(chi2), C.byref(it), C.byref(tr)))
    return {"siw": siw, "chi2_start": float(chi2[0]), "chi2": float(chi2[1]), "iterations": it.value, "trials": tr.value}


def essential_graph_analyze(fixed, edges):
    """The ordering and symbolic factorisation essential_graph_optimize uses, host only: variables, off-diagonal blocks of L,
    nnz(L) (scalars, lower triangle), flops of one numeric factorisation, elimination-tree levels, off-diagonal blocks of H."""
    fixed = np.ascontiguousarray(np.asarray(fixed, bool), np.uint8)
    e = np.ascontiguousarray(edges, SIM3_EDGE_DTYPE)
    out = np.zeros(6, np.int64)
    check(lib().sivo_essential_graph_analyze(_vp(fixed), fixed.shape[0], _vp(e), e.shape[0], _vp(out)))
    return dict(zip(("variables", "l_blocks", "nnz_l", "flops", "levels", "h_blocks"), (int(v) for v in out)))


def sim3_correct_points(xyz, ref, siw_before, siw_after):
    """The map-point correction of OptimizeEssentialGraph (Optimizer.cc:1205-1233): for point k with r = ref[k] >= 0,
    (float) siw_after[r]^-1 . map(siw_before[r] . map((double) xyz[k])); ref[k] = -1 leaves the point as it is."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    ref = np.ascontiguousarray(ref, np.int32).reshape(-1)
    before = np.ascontiguousarray(siw_before, np.float64).reshape(-1, 8)
    after = np.ascontiguousarray(siw_after, np.float64).reshape(-1, 8)
    if ref.shape[0] != xyz.shape[0] or before.shape != after.shape:
        raise ValueError("xyz / ref or siw_before / siw_after differ in length")
    out = np.empty_like(xyz)
    check(lib().sivo_sim3_correct_points(_vp(xyz), _vp(ref), xyz.shape[0], _vp(before), _vp(after), before.shape[0], _vp(out)))
    return out
