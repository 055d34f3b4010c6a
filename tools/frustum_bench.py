"""Times the per-frame local-map step of the tracking thread (Tracking::SearchLocalPoints) two ways, at 2000 and 4000 local map points
against a 1500-key frame:
  (a) a host cull (numpy, float32: Frame::isInFrustum vectorised) followed by sivo_search_by_projection_mappoints — the path before
      sivo_search_local_points existed, and the comparison;
  (b) sivo_search_local_points: the points go up in the engine's one upload, the cull and the queries are made on the device.
Both end in a device synchronise inside the library, so a host clock around the call is the call's time.  The two are alternated call by
call after a warm-up; the medians and the quartiles of each are printed as one JSON line per size, with whether both found the same
matches.
    python tools/frustum_bench.py [--repeats 2000] [--warmup 30]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sivo_amd import matcher as M, tracking as T  # noqa: E402

F32 = np.float32
FX, FY, CX, CY, BF = 718.856, 718.856, 607.1928, 185.2157, 386.1448
ROWS, COLS, NLEVELS, SCALE = 376, 1241, 8, 1.2


def scene(n_points, n_keys, seed):
    rng = np.random.default_rng(seed)
    a = np.deg2rad(2.0)
    Tcw = np.eye(4, dtype=F32)
    Tcw[0, 0] = Tcw[2, 2] = np.cos(a); Tcw[0, 2] = np.sin(a); Tcw[2, 0] = -np.sin(a); Tcw[:3, 3] = (0.2, -0.05, 0.4)
    # a local map: two thirds of it projects into the image, the rest lies around it or behind the camera
    z = rng.uniform(-3, 60, n_points); u = rng.uniform(-250, COLS + 250, n_points); v = rng.uniform(-60, ROWS + 60, n_points)
    pos = np.stack([(u - CX) * z / FX, (v - CY) * z / FY, z], 1).astype(F32)
    dist = np.linalg.norm(pos, axis=1)
    normal = (pos / np.maximum(dist, 1e-6)[:, None] + rng.normal(0, 0.2, pos.shape)).astype(F32)
    max_dist = (dist * rng.uniform(0.9, 4.0, n_points)).astype(F32)
    min_dist = (max_dist / F32(3.58)).astype(F32)
    desc = rng.integers(0, 256, (n_points, 32), dtype=np.uint8)
    obs = rng.integers(1, 8, n_points).astype(np.int32)
    scale = np.ones(NLEVELS, F32)
    for i in range(1, NLEVELS):
        scale[i] = scale[i - 1] * F32(SCALE)
    fr = T.frustum(Tcw, FX, FY, CX, CY, BF, (0, COLS, 0, ROWS), SCALE, NLEVELS)
    cull = host_cull(fr, Tcw, pos, normal, min_dist, max_dist)
    iv = np.flatnonzero(cull[0])
    of = rng.choice(iv, n_keys)
    keys = np.zeros(n_keys, M.KP_DTYPE)
    keys["x"] = cull[1][of] + rng.uniform(-2, 2, n_keys).astype(F32); keys["y"] = cull[2][of] + rng.uniform(-2, 2, n_keys).astype(F32)
    keys["octave"] = np.maximum(cull[4][of] - rng.integers(0, 2, n_keys), 0); keys["size"] = 31; keys["class_id"] = -1
    kd = np.unpackbits(desc[of], axis=1)
    kd ^= (rng.random(kd.shape) < 0.06).astype(np.uint8)
    F = M.MatchFrame(keys, (cull[3][of] + rng.uniform(-1, 1, n_keys)).astype(F32), np.packbits(kd, axis=1), (0, COLS, 0, ROWS), scale,
                     (scale * scale).astype(F32), (F32(1) / (scale * scale)).astype(F32))
    occ = np.where(rng.random(n_keys) < 0.1, 3, -1).astype(np.int32)
    return dict(F=F, fr=fr, Tcw=Tcw, pos=pos, normal=normal, min_dist=min_dist, max_dist=max_dist, desc=desc, obs=obs, occ=occ)


def host_cull(fr, Tcw, pos, normal, min_dist, max_dist):
    """Frame::isInFrustum over arrays in numpy float32 (the order of operations of the reference; the level through numpy's log)."""
    R, t = Tcw[:3, :3], Tcw[:3, 3]
    with np.errstate(all="ignore"):
        pc = [((R[r, 0] * pos[:, 0] + R[r, 1] * pos[:, 1]) + R[r, 2] * pos[:, 2]) + t[r] for r in range(3)]
        invz = F32(1) / pc[2]
        u = F32(FX) * pc[0] * invz + F32(CX); v = F32(FY) * pc[1] * invz + F32(CY)
        ow = (-(R.astype(np.float64).T @ t.astype(np.float64))).astype(F32)
        po = pos - ow
        dist = np.sqrt((po.astype(np.float64) ** 2).sum(1)).astype(F32)
        cos = ((po.astype(np.float64) * normal).sum(1) / dist).astype(F32)
        ok = ~(pc[2] < 0) & ~((u < fr.min_x) | (u > fr.max_x)) & ~((v < fr.min_y) | (v > fr.max_y))
        ok &= ~((dist < F32(0.8) * min_dist) | (dist > F32(1.2) * max_dist)) & ~(cos < F32(fr.cos_limit))
        level = np.clip(np.nan_to_num(np.ceil(np.log(max_dist / dist) / F32(fr.log_scale_factor))), 0, NLEVELS - 1).astype(np.int32)
    return ok, u, v, u - F32(BF) * invz, np.where(ok, level, 0), cos


def path_a(s, th):
    ok, u, v, ur, level, cos = host_cull(s["fr"], s["Tcw"], s["pos"], s["normal"], s["min_dist"], s["max_dist"])
    return M.search_by_projection_mappoints(s["F"], ok, u, v, ur, level, cos, s["desc"], s["obs"], th, 0.8, s["occ"])


def path_b(s, th):
    r = T.search_local_points(s["F"], s["fr"], s["pos"], s["normal"], s["min_dist"], s["max_dist"], None, s["desc"], s["obs"], th, 0.8, s["occ"])
    return r["n_matches"], r["match"], r["occ_obs"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--keys", type=int, default=1500)
    args = ap.parse_args()
    for n_points in (2000, 4000):
        s = scene(n_points, args.keys, n_points)
        ra, rb = path_a(s, 1.0), path_b(s, 1.0)
        times = {"a": [], "b": []}
        for i in range(args.warmup + args.repeats):
            for name, fn in (("a", path_a), ("b", path_b)) if i % 2 == 0 else (("b", path_b), ("a", path_a)):
                t0 = time.perf_counter()
                fn(s, 1.0)
                dt = time.perf_counter() - t0
                if i >= args.warmup:
                    times[name].append(dt * 1e3)
        q = {k: np.percentile(v, [25, 50, 75]) for k, v in times.items()}
        print(json.dumps({"points": n_points, "keys": args.keys, "repeats": args.repeats, "n_matches": int(rb[0]),
                          "same_matches": bool(ra[0] == rb[0] and np.array_equal(ra[1], rb[1])),
                          "a_host_cull_then_search_ms": {"p25": round(q["a"][0], 4), "median": round(q["a"][1], 4), "p75": round(q["a"][2], 4)},
                          "b_search_local_points_ms": {"p25": round(q["b"][0], 4), "median": round(q["b"][1], 4), "p75": round(q["b"][2], 4)}}))


if __name__ == "__main__":
    main()
