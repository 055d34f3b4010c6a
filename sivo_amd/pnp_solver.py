"""Python mirror of SIVO::PnPsolver (reference src/orbslam/PnPsolver.cc) over the C ABI: sivo_pnp_ransac / sivo_pnp_ransac_batch
evaluate every EPnP RANSAC hypothesis of every relocalisation candidate in one launch and refine every running best in a second
one; the PnPsolver class replays the results with the reference's sequential semantics (iterate / find / SetRansacParameters)."""
import ctypes as C
import math
import random

import numpy as np

from ._lib import PnpPoint, PnpRansacProblem, check, lib

PNP_POINT_DTYPE = np.dtype([("xw", np.float32, 3), ("u", np.float32), ("v", np.float32), ("max_err", np.float32)])
assert PNP_POINT_DTYPE.itemsize == C.sizeof(PnpPoint) == 24


def _fill(P, p):
    """One SivoPnpRansacProblem from a dict (points, K, samples, optional min_inliers / best_in); returns the arrays it points to
    (inputs to keep alive, outputs to hand back)."""
    pts = np.ascontiguousarray(p["points"], PNP_POINT_DTYPE).reshape(-1)
    smp = np.ascontiguousarray(p["samples"], np.int32).reshape(-1, 4)
    n, nh = pts.shape[0], smp.shape[0]
    words = (n + 63) // 64
    out = {"count": np.zeros(nh, np.int32), "T": np.zeros((nh, 12), np.float32), "inlier_bits": np.zeros((nh, words), np.uint64),
           "refined": np.full(nh, -1, np.int32), "refined_T": np.zeros((nh, 12), np.float32),
           "refined_bits": np.zeros((nh, words), np.uint64)}
    P.points = pts.ctypes.data if n else None
    P.n = n
    P.K[:] = [float(v) for v in p["K"]]
    P.min_inliers = int(p.get("min_inliers", 8))
    P.best_in = int(p.get("best_in", 0))
    P.samples = smp.ctypes.data if nh else None
    P.n_hyp = nh
    for k, a in out.items():
        setattr(P, k, a.ctypes.data if nh and a.size else None)
    return (pts, smp), out


def pnp_ransac_batch(problems):
    """k problems (every relocalisation candidate) in one call.  Each is a dict: points (PNP_POINT_DTYPE), K = fx fy cx cy, samples
    (n_hyp, 4) indices into points, optional min_inliers (8) and best_in (0).  Returns one dict per problem: count (n_hyp,), T
    (n_hyp, 12: Rcw row-major, tcw), inlier_bits (n_hyp, ceil(n / 64)) uint64, refined (n_hyp,: -1 where the hypothesis is no
    record), refined_T, refined_bits (rows of the records), n_records.  Each is bit-identical to pnp_ransac on that problem."""
    P = (PnpRansacProblem * max(len(problems), 1))()
    keep, outs = [], []
    for i, p in enumerate(problems):
        k, o = _fill(P[i], p)
        keep.append(k); outs.append(o)
    check(lib().sivo_pnp_ransac_batch(C.cast(P, C.c_void_p), len(problems)))
    for i, o in enumerate(outs):
        o["n_records"] = P[i].n_records
    return outs


def pnp_ransac(points, K, samples, min_inliers=8, best_in=0):
    """One problem (sivo_pnp_ransac): see pnp_ransac_batch."""
    P = PnpRansacProblem()
    keep, out = _fill(P, {"points": points, "K": K, "samples": samples, "min_inliers": min_inliers, "best_in": best_in})
    check(lib().sivo_pnp_ransac(C.byref(P)))
    out["n_records"] = P.n_records
    return out


def unpack_bits(words, n):
    """mvbInliersi of one hypothesis from its inlier words."""
    b = np.unpackbits(np.ascontiguousarray(words, "<u8").view(np.uint8), bitorder="little")
    return b[:n].astype(bool)


def _to_int(x):
    """A double converted to int as the reference's build does (cvttsd2si): out of range or not finite gives INT_MIN."""
    if not math.isfinite(x) or not (-2.0 ** 31 <= x < 2.0 ** 31):
        return -2 ** 31
    return int(x)


def _mat(T):
    M = np.eye(4, dtype=np.float32)
    M[:3, :3] = np.asarray(T[:9], np.float32).reshape(3, 3)
    M[:3, 3] = T[9:12]
    return M


_KEYS = ("count", "T", "inlier_bits", "refined", "refined_T", "refined_bits")


class PnPsolver:
    """PnPsolver over gathered arrays: xw (N, 3) = mvP3Dw, uv (N, 2) = mvP2D, sigma2 (N,) = mvSigma2, K = fx fy cx cy, indices[i] =
    mvKeyPointIndices[i] (the entry of vpMapPointMatches point i came from; default: i) and n_matches =
    mvpMapPointMatches.size() (default: N).  `randint(lo, hi)` draws the samples (default: random.randint).  All mRansacMaxIts
    samples are drawn when the solver is first evaluated (solve_all: several solvers in one call); iterate replays the results as
    PnPsolver.cc:180-269 does.  `.result` holds what has been evaluated (the _KEYS arrays, one row per hypothesis ever drawn);
    `evaluate(problem) -> result` replaces the device call (tests)."""

    def __init__(self, xw, uv, sigma2, K, indices=None, n_matches=None, randint=None, evaluate=None):
        self.points = np.zeros(len(xw), PNP_POINT_DTYPE)
        self.points["xw"] = np.asarray(xw, np.float32).reshape(-1, 3)
        uv = np.asarray(uv, np.float32).reshape(-1, 2)
        self.points["u"], self.points["v"] = uv[:, 0], uv[:, 1]
        self.sigma2 = np.asarray(sigma2, np.float32).reshape(-1)
        self.K = tuple(K)
        self.N = self.points.shape[0]
        self.indices = np.arange(self.N) if indices is None else np.asarray(indices, np.int64)
        self.n_matches = self.N if n_matches is None else int(n_matches)
        self.randint = randint or random.randint
        self.evaluate = evaluate
        self.iterations = 0
        self.best_inliers = 0
        self.best = None                    # (Tcw 4 x 4, inliers) of the running best
        self.refined = None                 # (count, Tcw 4 x 4, inliers): Refine of the running best
        self.result = None
        self.samples = np.zeros((0, 4), np.int32)
        self.set_ransac_parameters()

    def set_ransac_parameters(self, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4, th2=5.991):
        if min_set != 4:
            raise ValueError("the device evaluates samples of 4 correspondences (min_set == 4)")
        f32 = np.float32
        N = self.N
        eps = f32(epsilon)
        with np.errstate(all="ignore"):
            n_min = max(_to_int(float(f32(N) * eps)), int(min_inliers), min_set)
            ratio = f32(n_min) / f32(N)
            if eps < ratio:
                eps = ratio
            if n_min == N:
                n_it = 1
            else:
                n_it = _to_int(float(np.ceil(np.log(1 - np.float64(probability)) / np.log(1 - np.float64(eps) ** 3))))
        self.prob, self.min_inliers, self.epsilon = probability, n_min, eps
        self.max_its = max(1, min(n_it, int(max_iterations)))
        self.points["max_err"] = self.sigma2 * f32(th2)
        if self.iterations == 0:            # (what is held was evaluated against the former thresholds)
            self.result = None
            self.samples = np.zeros((0, 4), np.int32)

    def draw_samples(self, n_hyp):
        S = np.zeros((n_hyp, 4), np.int32)
        for h in range(n_hyp):
            avail = list(range(self.N))
            for i in range(4):
                r = self.randint(0, len(avail) - 1)
                S[h, i] = avail[r]
                avail[r] = avail[-1]
                avail.pop()
        return S

    def _can_run(self):
        return self.N >= self.min_inliers and self.N >= 4

    def _problem(self, n_hyp, best_in):
        S = self.draw_samples(n_hyp)
        self.samples = np.concatenate([self.samples, S])
        return {"points": self.points, "K": self.K, "samples": S, "min_inliers": self.min_inliers, "best_in": best_in}

    def _append(self, r):
        self.result = {k: np.asarray(r[k]) for k in _KEYS} if self.result is None else \
            {k: np.concatenate([self.result[k], np.asarray(r[k])]) for k in _KEYS}

    @staticmethod
    def solve_all(solvers):
        """Evaluates every solver not yet evaluated (None entries skipped) in ONE call."""
        todo = []
        for s in solvers:
            if s is not None and s.result is None and s._can_run() and s not in todo:
                todo.append(s)
        dev = [s for s in todo if s.evaluate is None]
        probs = {id(s): s._problem(s.max_its, 0) for s in todo}
        if dev:
            for s, r in zip(dev, pnp_ransac_batch([probs[id(s)] for s in dev])):
                s._append(r)
        for s in todo:
            if s.evaluate is not None:
                s._append(s.evaluate(probs[id(s)]))

    def _spread(self, bits):
        v = np.zeros(self.n_matches, bool)
        v[self.indices[bits]] = True
        return v

    def iterate(self, n_iterations):
        """-> (Tcw (4 x 4 float32) or None, bNoMore, vbInliers, nInliers); vbInliers is empty where the reference leaves it so."""
        none = np.zeros(0, bool)
        if not self._can_run():
            return None, True, none, 0
        PnPsolver.solve_all([self])
        cur = 0
        while self.iterations < self.max_its or cur < n_iterations:
            if self.iterations == len(self.result["count"]):
                # past the samples held: what is left of this call, in one further call
                p = self._problem(n_iterations - cur, self.best_inliers)
                self._append(self.evaluate(p) if self.evaluate is not None else pnp_ransac_batch([p])[0])
            r = self.result
            cur += 1
            h = self.iterations
            self.iterations += 1
            c = int(r["count"][h])
            if c >= self.min_inliers:
                if c > self.best_inliers:
                    self.best_inliers = c
                    self.best = (_mat(r["T"][h]), unpack_bits(r["inlier_bits"][h], self.N))
                    self.refined = (int(r["refined"][h]), _mat(r["refined_T"][h]), unpack_bits(r["refined_bits"][h], self.N))
                if self.refined[0] > self.min_inliers:
                    return self.refined[1].copy(), False, self._spread(self.refined[2]), self.refined[0]
        if self.iterations >= self.max_its:
            if self.best_inliers >= self.min_inliers:
                return self.best[0].copy(), True, self._spread(self.best[1]), self.best_inliers
            return None, True, none, 0
        return None, False, none, 0

    def find(self):
        T, _, inl, n = self.iterate(self.max_its)
        return T, inl, n
