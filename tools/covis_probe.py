"""Times the three covisibility entry points (sivo_covis_count, sivo_keyframe_culling, sivo_mappoint_culling) at the local mapper's own
shape — 80 local keyframes of 2000 slots, about 12 000 distinct map points with observation lists of 3 to 40, a 1500-point frame for the
vote, a few hundred recently added points — against the walk the reference does on the host: the stand-in object graph of
tests/covis_standins.hpp (std::map copies per point, one thread), compiled into tests/covis_adapter_prog.cpp and timed on the same box.

Device side: the time of the C ABI call with the arrays ready (one staged upload, one launch, one download, one synchronise inside the
library), by a host clock around the call; the gather from an object graph into those arrays, which an adapter pays on top, is not in
either figure.  Host side: the walk alone on a freshly built graph.  Medians and quartiles, one JSON line.  No pass mark.
    python tools/covis_probe.py [--repeats 200] [--warmup 20] [--walk-repeats 15]"""
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
import covis_cases as P  # noqa: E402
import host_prog  # noqa: E402
from sivo_amd import _lib, covisibility as cov  # noqa: E402

N_KF, N_LOCAL, SLOTS, N_POINTS, N_FRAME, N_RECENT, CURRENT_ID = 100, 80, 2000, 12000, 1500, 400, 500


def scene(seed=1):
    """Arrays of a whole object graph: per keyframe its slots (point, level, right, depth), per point its observations (keyframe, slot)."""
    rng = np.random.default_rng(seed)
    slots = [[] for _ in range(N_KF)]                               # (point, level, right, depth)
    obs = []
    for p in range(N_POINTS):
        room = [k for k in range(N_KF) if len(slots[k]) < SLOTS - 40]
        if len(room) < 3:
            break
        length = int(np.clip(rng.geometric(0.085) + 2, 3, min(40, len(room))))
        base = int(rng.integers(0, 6))
        mine = []
        for k in rng.choice(room, length, replace=False):
            k = int(k)
            mine.append((k, len(slots[k])))
            slots[k].append((p, max(0, base + int(rng.integers(-1, 2))), 5.0 if rng.random() < 0.5 else -1.0, float(rng.uniform(1.0, 45.0))))
        obs.append(mine)
    for k in range(N_KF):                                           # null slots up to the keyframe's 2000
        while len(slots[k]) < SLOTS:
            slots[k].append((-1, 0, -1.0, -1.0))
    n = len(obs)
    bad = (rng.random(n) < 0.01).astype(np.uint8)
    local = [int(k) for k in rng.permutation(N_LOCAL)]
    frame = np.where(rng.random(N_FRAME) < 0.1, -1, rng.integers(0, n, N_FRAME)).astype(np.int32)
    recent = rng.choice(n, N_RECENT, replace=False).astype(np.int32)
    return dict(slots=slots, obs=obs, bad=bad, local=local, frame=frame, recent=recent, n_points=n,
                found=rng.integers(0, 20, n).astype(np.int32), visible=rng.integers(1, 20, n).astype(np.int32),
                first=(CURRENT_ID - rng.integers(0, 5, n)).astype(np.int64))


def arrays(sc):
    n = sc["n_points"]
    level = [[s[1] for s in sl] for sl in sc["slots"]]
    right = [[s[2] for s in sl] for sl in sc["slots"]]
    obs_off, obs_kf = P.csr([[k for k, _ in o] for o in sc["obs"]], np.int32)
    _, obs_idx = P.csr([[i for _, i in o] for o in sc["obs"]], np.int32)
    obs_level = np.array([level[k][i] for o in sc["obs"] for k, i in o], np.uint8)
    obs_stereo = np.array([right[k][i] >= 0 for o in sc["obs"] for k, i in o], np.uint8)
    n_obs = np.array([sum(2 if right[k][i] >= 0 else 1 for k, i in o) for o in sc["obs"]], np.int32)
    table = cov.ObservationTable(N_KF, obs_off, obs_kf, obs_level, obs_stereo, sc["bad"])
    soff, spt = P.csr([[s[0] for s in sl] for sl in sc["slots"]], np.int32)
    _, slv = P.csr(level, np.uint8)
    _, srt = P.csr(right, np.float32)
    _, sdp = P.csr([[s[3] for s in sl] for sl in sc["slots"]], np.float32)
    graph = b"".join([P.i32(N_KF, n), np.arange(1, N_KF + 1, dtype=np.int64).tobytes(), np.zeros(N_KF, np.uint8).tobytes(),
                      np.full(N_KF, 40, np.float32).tobytes(), soff.tobytes(), spt.tobytes(), slv.tobytes(), srt.tobytes(), sdp.tobytes(),
                      sc["bad"].tobytes(), sc["found"].tobytes(), sc["visible"].tobytes(), sc["first"].tobytes(), n_obs.tobytes(),
                      obs_off.tobytes(), obs_kf.tobytes(), obs_idx.tobytes()])
    return table, dict(soff=soff, spt=spt, slv=slv, sdp=sdp, n_obs=n_obs), graph


def quartiles(t):
    q = np.percentile(np.array(t) * 1e3, [25, 50, 75])
    return dict(median_ms=round(float(q[1]), 4), q25_ms=round(float(q[0]), 4), q75_ms=round(float(q[2]), 4))


def timed(call, repeats, warmup):
    for _ in range(warmup):
        assert call() == 0
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        t.append(time.perf_counter() - t0)
    return quartiles(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--walk-repeats", type=int, default=15)
    a = ap.parse_args()
    _lib.require_gpu()
    sc = scene()
    table, s, graph = arrays(sc)
    L, st, p = _lib.lib(), table.struct(), (lambda x: x.ctypes.data)
    local = np.array(sc["local"], np.int32)
    # keyframe culling: the local keyframes' slots
    koff, kpt = P.csr([s["spt"][s["soff"][k]:s["soff"][k + 1]] for k in local], np.int32)
    _, klv = P.csr([s["slv"][s["soff"][k]:s["soff"][k + 1]] for k in local], np.uint8)
    _, kdp = P.csr([s["sdp"][s["soff"][k]:s["soff"][k + 1]] for k in local], np.float32)
    K = len(local)
    id0, erasable, th = np.zeros(K, np.uint8), np.ones(K, np.uint8), np.full(K, 40, np.float32)
    n_mps, n_red, dec, bad_after = np.zeros(K, np.int32), np.zeros(K, np.int32), np.zeros(K, np.uint8), np.zeros(table.n_points, np.uint8)
    kfcull = lambda: L.sivo_keyframe_culling(C.byref(st), K, p(local), p(id0), p(erasable), p(th), p(koff), p(kpt), p(klv), p(kdp), 0, p(n_mps),
                                             p(n_red), p(dec), p(bad_after))
    # the vote: one 1500-slot frame; UpdateConnections: the first local keyframe's own 2000 slots
    foff, fself, fcounts = np.array([0, N_FRAME], np.int64), np.array([-1], np.int32), np.zeros(N_KF, np.int32)
    vote = lambda: L.sivo_covis_count(C.byref(st), 1, p(foff), p(sc["frame"]), p(fself), p(fcounts))
    k0 = int(local[0])
    uslots = np.ascontiguousarray(s["spt"][s["soff"][k0]:s["soff"][k0 + 1]])
    uoff, uself, ucounts = np.array([0, len(uslots)], np.int64), np.array([k0], np.int32), np.zeros(N_KF, np.int32)
    update = lambda: L.sivo_covis_count(C.byref(st), 1, p(uoff), p(uslots), p(uself), p(ucounts))
    # all 80 local keyframes in one launch (the vector form of the adapter)
    aself, acounts = local.copy(), np.zeros((K, N_KF), np.int32)
    update_all = lambda: L.sivo_covis_count(C.byref(st), K, p(koff), p(kpt), p(aself), p(acounts))
    r = sc["recent"]
    found, visible, first = (np.ascontiguousarray(sc[k][r]) for k in ("found", "visible", "first"))
    nobs, rbad, status = np.ascontiguousarray(s["n_obs"][r]), np.ascontiguousarray(sc["bad"][r]), np.zeros(len(r), np.uint8)
    mpcull = lambda: L.sivo_mappoint_culling(len(r), p(found), p(visible), p(first), p(nobs), p(rbad), CURRENT_ID, 0, p(status))
    device = {name: timed(call, a.repeats, a.warmup) for name, call in (("keyframe_culling", kfcull), ("vote", vote), ("update_connections", update),
                                                                       ("update_connections_80", update_all), ("map_point_culling", mpcull))}
    # the same on the host: the reference's walk over the stand-in object graph
    with tempfile.TemporaryDirectory() as d:
        d = pathlib.Path(d)
        exe = host_prog.build("covis_adapter_prog", d)
        blob = b"".join([graph, P.i32(0, K), local.tobytes(), P.i32(N_FRAME), sc["frame"].tobytes(), np.array([CURRENT_ID], np.int64).tobytes(),
                         P.i32(len(r)), r.tobytes(), P.i32(a.walk_repeats)])
        walk = np.frombuffer(host_prog.run(exe, d, "walk", blob), np.float64)[:4] / 1e3
    host = dict(zip(("keyframe_culling", "vote", "update_connections", "map_point_culling"), (round(float(x), 4) for x in walk)))
    print(json.dumps(dict(shape=dict(n_kf=N_KF, n_local=K, slots_per_keyframe=SLOTS, n_points=int(table.n_points), n_observations=int(len(table.obs_kf)),
                                     frame_slots=N_FRAME, recent_points=int(len(r))),
                          culled=int((dec == 1).sum()), bad_after=int(bad_after.sum()), status=np.bincount(status, minlength=5).tolist(),
                          device_ms=device, host_walk_median_ms=host)))


if __name__ == "__main__":
    main()
