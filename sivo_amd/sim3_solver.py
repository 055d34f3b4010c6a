"""Python mirror of SIVO::Sim3Solver (reference src/orbslam/Sim3Solver.cc) over the C ABI: sivo_sim3_ransac /
sivo_sim3_ransac_batch evaluate every RANSAC hypothesis of every loop candidate in one launch; the Sim3Solver class replays
the counts with the reference's sequential semantics (iterate / find / SetRansacParameters)."""
import ctypes as C
import math
import random

import numpy as np

from ._lib import Sim3Pair, Sim3RansacProblem, check, lib

SIM3_PAIR_DTYPE = np.dtype([("x1c", np.float32, 3), ("x2c", np.float32, 3), ("max_err1", np.float32), ("max_err2", np.float32)])
assert SIM3_PAIR_DTYPE.itemsize == C.sizeof(Sim3Pair) == 32


def _fill(P, p):
    """One SivoSim3RansacProblem from a dict (pairs, k1, k2, triples, optional min_inliers / fix_scale); returns the arrays it
    points to (inputs to keep alive, outputs to hand back)."""
    pairs = np.ascontiguousarray(p["pairs"], SIM3_PAIR_DTYPE).reshape(-1)
    tri = np.ascontiguousarray(p["triples"], np.int32).reshape(-1, 3)
    n, nh = pairs.shape[0], tri.shape[0]
    words = (n + 63) // 64
    out = {"count": np.zeros(nh, np.int32), "T": np.zeros((nh, 13), np.float32), "inlier_bits": np.zeros((nh, words), np.uint64)}
    P.pairs = pairs.ctypes.data if n else None
    P.n = n
    P.k1[:] = [float(v) for v in p["k1"]]
    P.k2[:] = [float(v) for v in p["k2"]]
    P.triples = tri.ctypes.data if nh else None
    P.n_hyp = nh
    P.min_inliers = int(p.get("min_inliers", 20))
    P.fix_scale = int(bool(p.get("fix_scale", True)))
    P.count = out["count"].ctypes.data if nh else None
    P.T = out["T"].ctypes.data if nh else None
    P.inlier_bits = out["inlier_bits"].ctypes.data if nh and words else None
    return (pairs, tri), out


def sim3_ransac_batch(problems):
    """k problems (every loop candidate) in one launch.  Each is a dict: pairs (SIM3_PAIR_DTYPE), k1 / k2 = fx fy cx cy, triples
    (n_hyp, 3) indices into pairs, optional min_inliers (20) and fix_scale (True).  Returns one dict per problem: count (n_hyp,),
    T (n_hyp, 13: R12 row-major, t12, s12), inlier_bits (n_hyp, ceil(n / 64)) uint64, first_accept, best.  Each is bit-identical
    to sim3_ransac on that problem."""
    P = (Sim3RansacProblem * max(len(problems), 1))()
    keep, outs = [], []
    for i, p in enumerate(problems):
        k, o = _fill(P[i], p)
        keep.append(k); outs.append(o)
    check(lib().sivo_sim3_ransac_batch(C.cast(P, C.c_void_p), len(problems)))
    for i, o in enumerate(outs):
        o["first_accept"] = P[i].first_accept; o["best"] = P[i].best
    return outs


def sim3_ransac(pairs, k1, k2, triples, min_inliers=20, fix_scale=True):
    """One problem (sivo_sim3_ransac): see sim3_ransac_batch."""
    P = Sim3RansacProblem()
    keep, out = _fill(P, {"pairs": pairs, "k1": k1, "k2": k2, "triples": triples, "min_inliers": min_inliers, "fix_scale": fix_scale})
    check(lib().sivo_sim3_ransac(C.byref(P)))
    out["first_accept"] = P.first_accept; out["best"] = P.best
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


class Sim3Solver:
    """Sim3Solver over gathered arrays: pairs (SIM3_PAIR_DTYPE), k1 / k2, indices1[i] = mvnIndices1[i] (the entry of vpMatched12
    pair i came from; default: i) and n_matches = mN1 (default: the number of pairs).  `randint(lo, hi)` draws the samples
    (default: random.randint).  All mRansacMaxIts triples are drawn at the first iterate / find and evaluated in one launch
    (solve_all: several solvers in one launch); iterate replays the counts as Sim3Solver.cc:143-208 does."""

    def __init__(self, pairs, k1, k2, fix_scale=True, indices1=None, n_matches=None, randint=None):
        self.pairs = np.ascontiguousarray(pairs, SIM3_PAIR_DTYPE).reshape(-1)
        self.k1, self.k2, self.fix_scale = k1, k2, bool(fix_scale)
        self.N = self.pairs.shape[0]
        self.indices1 = np.arange(self.N) if indices1 is None else np.asarray(indices1, np.int64)
        self.mN1 = self.N if n_matches is None else int(n_matches)
        self.randint = randint or random.randint
        self.iterations = 0
        self.best_inliers = 0
        self.best = None                    # (T12 4 x 4, R, t, s, inliers) of the running best
        self.result = None
        self.set_ransac_parameters()

    def set_ransac_parameters(self, probability=0.99, min_inliers=6, max_iterations=300):
        self.prob, self.min_inliers = probability, int(min_inliers)
        N = self.N
        if self.min_inliers == N:
            n_it = 1
        else:
            with np.errstate(all="ignore"):
                eps = np.float32(self.min_inliers) / np.float32(N)
                n_it = _to_int(float(np.ceil(np.log(1 - np.float64(probability)) / np.log(1 - np.float64(eps) ** 3))))
        self.max_its = max(1, min(n_it, int(max_iterations)))
        self.iterations = 0
        self.result = None                  # (the samples are drawn for max_its: drawn again at the next iterate)

    def draw_triples(self):
        tri = np.zeros((self.max_its, 3), np.int32)
        for h in range(self.max_its):
            avail = list(range(self.N))
            for i in range(3):
                r = self.randint(0, len(avail) - 1)
                tri[h, i] = avail[r]
                avail[r] = avail[-1]
                avail.pop()
        return tri

    def _can_run(self):
        return self.N >= self.min_inliers and self.N >= 3

    def _problem(self):
        self.triples = self.draw_triples()
        return {"pairs": self.pairs, "k1": self.k1, "k2": self.k2, "triples": self.triples, "min_inliers": self.min_inliers,
                "fix_scale": self.fix_scale}

    @staticmethod
    def solve_all(solvers):
        """Evaluates every solver not yet evaluated (None entries skipped) in ONE launch."""
        todo = [s for s in solvers if s is not None and s.result is None and s._can_run()]
        if todo:
            for s, r in zip(todo, sim3_ransac_batch([s._problem() for s in todo])):
                s.result = r

    def iterate(self, n_iterations):
        """-> (T12 (4 x 4 float32) or None, bNoMore, vbInliers (mN1 bools), nInliers)."""
        inliers = np.zeros(self.mN1, bool)
        if not self._can_run():             # (N < 3 cannot be sampled: the reference would index an empty vector)
            return None, True, inliers, 0
        Sim3Solver.solve_all([self])
        r = self.result
        cur = 0
        while self.iterations < self.max_its and cur < n_iterations:
            cur += 1
            h = self.iterations
            self.iterations += 1
            c = int(r["count"][h])
            if c >= self.best_inliers:
                T = r["T"][h]
                R, t, s = T[:9].reshape(3, 3).copy(), T[9:12].copy(), np.float32(T[12])
                T12 = np.eye(4, dtype=np.float32)
                with np.errstate(all="ignore"):
                    T12[:3, :3] = R * s
                T12[:3, 3] = t
                bits = unpack_bits(r["inlier_bits"][h], self.N)
                self.best_inliers = c
                self.best = (T12, R, t, s, bits)
                if c > self.min_inliers:
                    inliers[self.indices1[bits]] = True
                    return T12, False, inliers, c
        return None, self.iterations >= self.max_its, inliers, 0

    def find(self):
        T, _, inl, n = self.iterate(self.max_its)
        return T, inl, n

    def estimated_rotation(self):
        return self.best[1].copy()

    def estimated_translation(self):
        return self.best[2].copy()

    def estimated_scale(self):
        return self.best[3]
