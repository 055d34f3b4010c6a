"""Times sivo_loop_correct and sivo_gba_propagate, the loop closer's two map corrections, at two sizes: a KITTI-sized loop
closure (60 corrected keyframes beside 20 others, 20 000 map points) and a whole large map (2 000 keyframes, 200 000 map points).  Points
are held and observed by 3 to 8 neighbouring keyframes; the spanning tree is the chain a forward drive leaves, with side branches, its last
30 keyframes outside the BA (created while it ran).  Beside each device call the host build of the same per-item bodies
(tests/loop_correct_host_capi.hpp: sequential loops, one thread) on the same inputs on the same box, and a byte comparison of the two.

Device side: the time of the C ABI call with the arrays ready (the argument checks, one upload, the launches, one download, one
synchronise inside the library), by a host clock around the call.  Medians and quartiles, one JSON line.  No pass mark.
    python tools/loop_correct_probe.py [--repeats 100] [--warmup 10] [--host-repeats 9]"""
import argparse
import ctypes as C
import json
import os
import pathlib
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import host_prog  # noqa: E402
import loop_correct_cases as LC  # noqa: E402
from sivo_amd import _lib, loop_closing  # noqa: E402

F = np.float32
SIZES = ((60, 20, 20000), (2000, 0, 200000))


def poses(rng, n):
    T = np.tile(np.eye(4, dtype=F), (n, 1, 1))
    for k in range(n):
        T[k] = LC.random_pose(rng, k % 90)
    return T


def centres(T):
    return np.stack([-(t[:3, :3].T.astype(np.float64) @ t[:3, 3].astype(np.float64)) for t in T]).astype(F)


def loop_args(n_kf, n_out, n_points, seed=1):
    rng = np.random.default_rng(seed)
    n_all = n_kf + n_out
    T = poses(rng, n_all)
    centre = rng.integers(0, n_all, n_points)
    held = [[] for _ in range(n_kf)]
    obs = []
    for p in range(n_points):
        lo, hi = max(0, centre[p] - 6), min(n_all, centre[p] + 7)
        mine = np.sort(rng.choice(np.arange(lo, hi), min(int(rng.integers(3, 9)), hi - lo), replace=False))
        obs.append(mine.astype(np.int32))
        for k in mine:
            if k < n_kf:
                held[k].append(p)
    slot_off, slot_point = LC.LR.csr([np.where(rng.random(len(h)) < 0.05, -1, np.array(h, np.int32)) for h in held], np.int32)
    obs_off, obs_kf = LC.LR.csr(obs, np.int32)
    cur = n_kf - 1
    from essential_graph_restatement import exp, mul, sim3_from_pose
    scw = mul(exp([0.01, 0.02, -0.01, 0.4, 0.02, -0.3, 0.0]), sim3_from_pose(T[cur]))
    twc = np.eye(4, dtype=F)
    twc[:3, :3], twc[:3, 3] = T[cur][:3, :3].T, centres(T[cur:cur + 1])[0]
    return {"n_kf": n_kf, "cur": cur, "n_all": n_all, "n_points": n_points, "tiw": T[:n_kf], "twc_cur": twc, "scw": scw, "ow": centres(T),
            "slot_off": slot_off, "slot_point": slot_point, "pos": (rng.normal(size=(n_points, 3)) * 10).astype(F),
            "skip": (rng.random(n_points) < 0.03).astype(np.uint8), "obs_off": obs_off, "obs_kf": obs_kf,
            "ref_kf": np.array([o[0] for o in obs], np.int32), "level_scale": LC.SF[rng.integers(0, 8, n_points)], "last_scale": np.full(n_points, LC.SF[-1], F)}


def gba_args(n_kf, n_points, seed=2):
    rng = np.random.default_rng(seed)
    parent = np.arange(-1, n_kf - 1)
    side = rng.random(n_kf) < 0.1                           # one keyframe in ten hangs off an older one
    parent[side] = np.maximum(np.arange(n_kf)[side] - rng.integers(2, 6, side.sum()), 0)
    parent[0] = -1
    children = [[] for _ in range(n_kf)]
    for k in range(1, n_kf):
        children[parent[k]].append(k)
    child_off, child_kf = LC.LR.csr(children, np.int32)
    in_gba = np.ones(n_kf, np.uint8)
    in_gba[n_kf - 30:] = 0
    T = poses(rng, n_kf)
    return {"n_kf": n_kf, "n_origins": 1, "n_points": n_points, "origin": np.zeros(1, np.int32), "child_off": child_off, "child_kf": child_kf,
            "tcw": T, "tcw_gba": poses(rng, n_kf), "in_gba": in_gba, "tcw_bef": np.zeros((n_kf, 4, 4), F),
            "pos": (rng.normal(size=(n_points, 3)) * 10).astype(F), "pos_gba": (rng.normal(size=(n_points, 3)) * 10).astype(F),
            "point_in_gba": (rng.random(n_points) < 0.9).astype(np.uint8), "point_bad": (rng.random(n_points) < 0.02).astype(np.uint8),
            "ref_kf": rng.integers(0, n_kf, n_points).astype(np.int32)}


def quartiles(t):
    q = np.percentile(np.array(t) * 1e3, [25, 50, 75])
    return dict(median_ms=round(float(q[1]), 4), q25_ms=round(float(q[0]), 4), q75_ms=round(float(q[2]), 4))


def timed(call, repeats, warmup):
    for _ in range(warmup):
        call()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        t.append(time.perf_counter() - t0)
    return quartiles(t)


def device_loop(a, repeats, warmup):
    keep = [np.ascontiguousarray(a[n], dt).ravel() for n, dt in LC.LOOP_IN]
    out = {n: np.zeros(per * (a["n_kf"] if which == "k" else a["n_points"]), dt) for n, dt, per, which in LC.LOOP_OUT}
    s = loop_closing.LoopCorrect(a["n_kf"], a["cur"], a["n_all"], a["n_points"], *[v.ctypes.data for v in keep], *[out[n].ctypes.data for n, *_ in LC.LOOP_OUT])
    L = _lib.lib()

    def call():
        _lib.check(L.sivo_loop_correct(C.byref(s)))
    return timed(call, repeats, warmup), out


def device_gba(a, repeats, warmup):
    fresh = {n: np.ascontiguousarray(a[n], dt).ravel() for n, dt in LC.GBA_IN}
    keep = {n: v.copy() for n, v in fresh.items()}
    K, P = a["n_kf"], a["n_points"]
    out = {"tcw_out": np.zeros(16 * K, F), "ow_out": np.zeros(3 * K, F), "kf_reached": np.zeros(K, np.uint8), "pos_out": np.zeros(3 * P, F),
           "point_status": np.zeros(P, np.uint8)}
    s = loop_closing.GbaPropagate(K, a["n_origins"], P, *[keep[n].ctypes.data for n, _ in LC.GBA_IN], *[out[n].ctypes.data for n in out])
    L = _lib.lib()

    def call():
        for n in ("tcw_gba", "in_gba", "tcw_bef"):          # the in/out arrays as they were (a copy of 130 KB at most)
            keep[n][:] = fresh[n]
        _lib.check(L.sivo_gba_propagate(C.byref(s)))
    t = timed(call, repeats, warmup)
    out.update({n: keep[n] for n in ("tcw_gba", "in_gba", "tcw_bef")})
    return t, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-repeats", type=int, default=9)
    a = ap.parse_args()
    _lib.require_gpu()
    rows = []
    with tempfile.TemporaryDirectory() as d:
        d = pathlib.Path(d)
        exe = host_prog.build("loop_correct_prog", d)
        for n_kf, n_out, n_points in SIZES:
            la, ga = loop_args(n_kf, n_out, n_points), gba_args(n_kf, n_points)
            dev_loop, out_loop = device_loop(la, a.repeats, a.warmup)
            dev_gba, out_gba = device_gba(ga, a.repeats, a.warmup)
            raw = host_prog.run(exe, d, "loop_timed", LC.loop_blob(la), extra_args=(a.host_repeats,), timeout=900)
            rc, _, host = LC.parse(raw[:-8], LC.LOOP_OUT, n_kf, n_points)
            moved = host["corrected_by"] >= 0
            same_loop = rc == 0 and all(out_loop[n].tobytes() == host[n].tobytes() for n in ("noncorrected_siw", "corrected_siw", "tiw_out", "ow_out", "corrected_by"))
            same_loop = same_loop and out_loop["pos_out"].reshape(-1, 3)[moved].tobytes() == host["pos_out"].reshape(-1, 3)[moved].tobytes()
            same_loop = same_loop and out_loop["normal"].reshape(-1, 3)[moved].tobytes() == host["normal"].reshape(-1, 3)[moved].tobytes()
            host_loop_ms = float(np.frombuffer(raw[-8:], np.float64)[0]) / 1e3
            raw = host_prog.run(exe, d, "gba_timed", LC.gba_blob(ga), extra_args=(a.host_repeats,), timeout=900)
            rc, _, host = LC.parse(raw[:-8], LC.GBA_OUT, n_kf, n_points)
            written = np.isin(host["point_status"], (1, 2))
            same_gba = rc == 0 and all(out_gba[n].tobytes() == host[n].tobytes() for n in ("tcw_gba", "in_gba", "tcw_bef", "tcw_out", "ow_out", "kf_reached", "point_status"))
            same_gba = same_gba and out_gba["pos_out"].reshape(-1, 3)[written].tobytes() == host["pos_out"].reshape(-1, 3)[written].tobytes()
            host_gba_ms = float(np.frombuffer(raw[-8:], np.float64)[0]) / 1e3
            rows.append(dict(shape=dict(n_kf=n_kf, n_outside=n_out, n_points=n_points, slots=int(la["slot_off"][-1]), observations=int(la["obs_off"][-1]),
                                        points_moved=int(moved.sum()), points_carried=int((host["point_status"] == 2).sum())),
                             loop_correct=dict(device_ms=dev_loop, host_build_median_ms=round(host_loop_ms, 4), same_bytes=bool(same_loop)),
                             gba_propagate=dict(device_ms=dev_gba, host_build_median_ms=round(host_gba_ms, 4), same_bytes=bool(same_gba))))
    print(json.dumps(rows))
    assert all(r["loop_correct"]["same_bytes"] and r["gba_propagate"]["same_bytes"] for r in rows), "the device and the host build differ"


if __name__ == "__main__":
    main()
