"""Times Tracking::TrackLocalMap's device part on the resident map, at maps of 300, 1000 and 3000 keyframes (200 new points per keyframe,
each observed by the five keyframes around it; about a thousand filled slots of 1400 per keyframe; covisibility lists of 20; a chain of
parents and children) and a frame of 1500 keys that looks at the newest sixty keyframes, which gives a local map of some sixty
keyframes and 12 000 points at every map size.  Three measurements per map size, in ONE run, interleaved call by call so that a drift
of the machine meets all three alike:
  (a) fused     LocalMap.search_local_points: sivo_localmap_search_local_points
  (b) pair      LocalMap.update, a numpy gather of the attribute arrays by local_point, tracking.search_local_points
  (c) gather    the numpy gather of (b) alone: seven fancy-index reads, the skip flags and the occupancy
(c) is a LOWER BOUND on what the C++ adapter pays between the two calls of (b): SIVO::SearchLocalPoints walks the MapPoint objects and
takes a mutex and clones a cv::Mat per getter (GetWorldPos, GetNormal, GetDescriptor ...), which contiguous numpy arrays do not.

The time of each call by a host clock around it, the arrays ready, every library call synchronising inside.  Medians and quartiles over
--repeats calls after --warmup, one JSON line; `within` says whether (a) is not slower than (b) by more than (b)'s own interquartile
range.  The results of (a) and (b) are compared byte for byte before anything is timed.
    python tools/track_local_map_probe.py [--repeats 300] [--warmup 30] [--sizes 300,1000,3000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sivo_amd import _lib, local_map, matcher, tracking  # noqa: E402

PPK, SPAN, SLOTS, N_KEYS, NEWEST, NLEVELS, SCALE = 200, 2, 1400, 1500, 60, 8, 1.2
FX, FY, CX, CY, BF, BOUNDS = 718.856, 718.856, 607.19, 185.22, 386.1448, (0.0, 1241.0, 0.0, 376.0)
ATTRS = ("pos", "normal", "min_dist", "max_dist", "desc", "n_obs")
F32 = np.float32


def csr(rows):
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    return off, (np.concatenate(rows) if len(rows) else np.zeros(0)).astype(np.int32)


def scene(n_kf, seed=1):
    rng = np.random.default_rng(seed)
    P = n_kf * PPK
    centre = np.arange(P) // PPK
    lo, hi = np.maximum(centre - SPAN, 0), np.minimum(centre + SPAN + 1, n_kf)
    cnt = hi - lo
    obs_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    obs_kf = (np.repeat(lo, cnt) + np.arange(obs_off[-1]) - np.repeat(obs_off[:-1], cnt)).astype(np.int32)
    slots = []
    for k in range(n_kf):                                           # the points of the keyframes around k, scattered over its slots
        mine = np.arange(max(k - SPAN, 0) * PPK, min(k + SPAN + 1, n_kf) * PPK, dtype=np.int32)
        s = np.full(SLOTS, -1, np.int32)
        s[np.sort(rng.choice(SLOTS, len(mine), replace=False))] = rng.permutation(mine)
        slots.append(s)
    slot_off, slot_point = csr(slots)
    covis_off, covis_kf = csr([np.array([c for d in range(1, 11) for c in (k - d, k + d) if 0 <= c < n_kf], np.int32) for k in range(n_kf)])
    child_off, child_kf = csr([np.array([k + 1] if k + 1 < n_kf else [], np.int32) for k in range(n_kf)])
    tables = dict(obs_off=obs_off, obs_kf=obs_kf, point_bad=(rng.random(P) < 0.01).astype(np.uint8), kf_bad=(rng.random(n_kf) < 0.02).astype(np.uint8),
                  slot_off=slot_off, slot_point=slot_point, covis_off=covis_off, covis_kf=covis_kf, child_off=child_off, child_kf=child_kf,
                  parent=np.arange(-1, n_kf - 1, dtype=np.int32), kf_order=rng.permutation(n_kf).astype(np.int32))
    # the points in front of an identity camera, most of them inside the image; the normal looks back at the camera
    z = rng.uniform(5, 60, P)
    u, v = rng.uniform(-150, BOUNDS[1] + 150, P), rng.uniform(-60, BOUNDS[3] + 60, P)
    pos = np.stack([(u - CX) * z / FX, (v - CY) * z / FY, z], 1).astype(F32)
    dist = np.linalg.norm(pos, axis=1)
    at = dict(pos=pos, normal=(pos / dist[:, None]).astype(F32), min_dist=(dist * rng.uniform(0.3, 0.9, P)).astype(F32),
              max_dist=(dist * rng.uniform(1.1, 4.0, P)).astype(F32), desc=rng.integers(0, 256, (P, 32), dtype=np.uint8),
              n_obs=cnt.astype(np.int32))
    keys = np.zeros(N_KEYS, matcher.KP_DTYPE)
    keys["x"], keys["y"] = rng.uniform(0, BOUNDS[1], N_KEYS), rng.uniform(0, BOUNDS[3], N_KEYS)
    keys["octave"], keys["size"], keys["angle"], keys["class_id"] = rng.integers(0, NLEVELS, N_KEYS), 31, rng.uniform(0, 360, N_KEYS), -1
    s = (F32(SCALE) ** np.arange(NLEVELS)).astype(F32)
    frame = matcher.MatchFrame(keys, np.where(rng.random(N_KEYS) < 0.2, -1, keys["x"] - 5).astype(F32), rng.integers(0, 256, (N_KEYS, 32), dtype=np.uint8),
                               BOUNDS, s, s * s, (F32(1) / (s * s)).astype(F32))
    newest = np.arange((n_kf - NEWEST) * PPK, P)
    fp = np.where(rng.random(N_KEYS) < 0.4, rng.choice(newest, N_KEYS), -1).astype(np.int32)
    seen = np.sort(rng.choice(newest, 100, replace=False)).astype(np.int32)
    T = np.eye(4, dtype=F32)
    fr = tracking.frustum(T, FX, FY, CX, CY, BF, BOUNDS, SCALE, NLEVELS)
    return tables, at, frame, fr, fp, seen, np.arange(n_kf - 80, n_kf, dtype=np.int32)


def quartiles(t):
    q = np.percentile(np.array(t) * 1e3, [25, 50, 75])
    return dict(median_ms=round(float(q[1]), 4), q25_ms=round(float(q[0]), 4), q75_ms=round(float(q[2]), 4), iqr_ms=round(float(q[2] - q[0]), 4))


def measure(n_kf, repeats, warmup):
    tables, at, frame, fr, fp, seen, prev = scene(n_kf)
    P = len(at["n_obs"])
    cap = min(P, 1 << 15)                                           # what a tracker would bound its local map by
    with local_map.LocalMap(n_kf, **tables) as h:
        h.set_points(np.arange(P), *(at[k] for k in ATTRS))
        out = dict(slot_cleared=np.zeros(N_KEYS, np.uint8), local_kf=np.zeros(n_kf, np.int32), local_point=np.zeros(cap, np.int32),
                   counts=np.zeros(n_kf, np.int32))
        search_out = dict(out, status=np.zeros(cap, np.uint8), proj_x=np.zeros(cap, F32), proj_y=np.zeros(cap, F32), proj_xr=np.zeros(cap, F32),
                          view_cos=np.zeros(cap, F32), level=np.zeros(cap, np.int32), match=np.zeros(N_KEYS, np.int32))
        kept = {}

        def fused():
            kept["a"] = h.search_local_points(frame, fr, fp, None, None, prev, seen, 3.0, 0.8, kf_capacity=n_kf, point_capacity=cap, out=search_out)

        def update():
            kept["u"] = h.update(fp, None, None, prev, kf_capacity=n_kf, point_capacity=cap, out=out)

        def gather():
            u = kept["u"]
            local = u.local_points
            held = (fp >= 0) & (u.slot_cleared == 0)
            skip = np.isin(local, np.concatenate([fp[held], seen])).astype(np.uint8)
            kept["g"] = ([at[k][local] for k in ATTRS], skip, np.where(held, at["n_obs"][np.maximum(fp, 0)], -1).astype(np.int32))

        def search():
            (pos, normal, lo, hi, desc, n_obs), skip, occ = kept["g"]
            kept["b"] = tracking.search_local_points(frame, fr, pos, normal, lo, hi, skip, desc, n_obs, 3.0, 0.8, occ)

        def pair():
            update(); gather(); search()

        fused(); pair()
        a, b, u = kept["a"], kept["b"], kept["u"]
        n = len(u.local_points)
        assert a.local_points.tobytes() == u.local_points.tobytes() and a.local_kf.tobytes() == u.local_kf.tobytes() and a.ref_kf == u.ref_kf
        assert a.status.tobytes() == b["status"].tobytes() and a.match.tobytes() == b["match"].tobytes()
        assert (a.n_to_match, a.n_matches) == (b["n_in_view"], b["n_matches"])
        iv = b["in_view"]
        for k in ("proj_x", "proj_y", "proj_xr", "view_cos", "level"):
            assert getattr(a, k)[iv].tobytes() == b[k][iv].tobytes(), k
        for _ in range(warmup):
            fused(); pair()
        t = dict(fused=[], pair=[], gather=[])
        for _ in range(repeats):                                    # interleaved: one call of each per round
            t0 = time.perf_counter(); fused(); t1 = time.perf_counter()
            update(); t2 = time.perf_counter(); gather(); t3 = time.perf_counter(); search(); t4 = time.perf_counter()
            t["fused"].append(t1 - t0); t["pair"].append(t4 - t1); t["gather"].append(t3 - t2)
        res = {k: quartiles(v) for k, v in t.items()}
        res["shape"] = dict(n_kf=n_kf, n_points=P, total_slots=int(tables["slot_off"][-1]), frame_keys=N_KEYS, n_local_kf=int(len(u.local_kf)),
                            n_local_points=n, n_to_match=int(a.n_to_match), n_matches=int(a.n_matches))
        res["within"] = bool(res["fused"]["median_ms"] <= res["pair"]["median_ms"] + res["pair"]["iqr_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--sizes", default="300,1000,3000")
    a = ap.parse_args()
    if a.repeats < 200:
        raise SystemExit("at least 200 repeats: the medians and quartiles are what the probe is for")
    _lib.require_gpu()
    print(json.dumps({str(n): measure(n, a.repeats, a.warmup) for n in (int(s) for s in a.sizes.split(","))}))


if __name__ == "__main__":
    main()
