"""Times sivo_localmap_update, the tracking thread's Tracking::UpdateLocalMap on the resident map, at a tracking-sized map: 300 keyframes
of 2000 slots (about 60 % filled), 60 000 map points observed by 3 to 20 neighbouring keyframes each, ordered covisibility lists of 20, a
chain of parents and children, and a frame of 1500 slots that looks at the newest part of the map — which gives a local map of about 60
keyframes and some 14 000 points.  Beside it the host build of the same routine (tests/localmap_host_capi.hpp:
the same per-item bodies in sequential loops, one thread) on the same box, and what a rebuild (sivo_localmap_replace) and a
sivo_localmap_set_bad of ten flags cost.

Device side: the time of the C ABI call with the arrays ready (one upload, the launches, one download, one synchronise inside the
library), by a host clock around the call.  Medians and quartiles, one JSON line.  No pass mark.
    python tools/localmap_probe.py [--repeats 200] [--warmup 20] [--host-repeats 15]"""
import argparse
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
import localmap_cases as P  # noqa: E402
from sivo_amd import _lib, local_map  # noqa: E402

N_KF, SLOTS, N_POINTS, N_FRAME, WINDOW = 300, 2000, 60000, 1500, 15


def scene(seed=1):
    rng = np.random.default_rng(seed)
    centre = np.sort(rng.integers(0, N_KF, N_POINTS))
    held = [[] for _ in range(N_KF)]
    obs = []
    for p in range(N_POINTS):
        lo, hi = max(0, centre[p] - WINDOW), min(N_KF, centre[p] + WINDOW + 1)
        mine = np.sort(rng.choice(np.arange(lo, hi), min(int(rng.integers(3, 21)), hi - lo), replace=False))
        mine = [int(k) for k in mine if len(held[k]) < SLOTS * 6 // 10]
        for k in mine:
            held[k].append(p)
        obs.append(mine)
    slots = []
    for k in range(N_KF):                                           # the keyframe's points scattered over its 2000 slots, the rest null
        s = np.full(SLOTS, -1, np.int32)
        s[np.sort(rng.choice(SLOTS, len(held[k]), replace=False))] = held[k]
        slots.append(s)
    covis = [[c for d in range(1, 11) for c in (k - d, k + d) if 0 <= c < N_KF] for k in range(N_KF)]
    obs_off, obs_kf = P.R.csr(obs, np.int32)
    slot_off, slot_point = P.R.csr(slots, np.int32)
    covis_off, covis_kf = P.R.csr(covis, np.int32)
    child_off, child_kf = P.R.csr([[k + 1] if k + 1 < N_KF else [] for k in range(N_KF)], np.int32)
    tables = dict(n_kf=N_KF, obs_off=obs_off, obs_kf=obs_kf, point_bad=(rng.random(N_POINTS) < 0.01).astype(np.uint8),
                  kf_bad=(rng.random(N_KF) < 0.02).astype(np.uint8), slot_off=slot_off, slot_point=slot_point, covis_off=covis_off, covis_kf=covis_kf,
                  child_off=child_off, child_kf=child_kf, parent=np.arange(-1, N_KF - 1, dtype=np.int32), kf_order=rng.permutation(N_KF).astype(np.int32))
    newest = np.flatnonzero(centre >= N_KF - 60)
    frame = np.where(rng.random(N_FRAME) < 0.1, -1, rng.choice(newest, N_FRAME)).astype(np.int32)
    call = dict(frame_point=frame, kf_premarked=np.zeros(0, np.int32), point_premarked=np.zeros(0, np.int32),
                prev_local_kf=np.arange(N_KF - 80, N_KF, dtype=np.int32), kf_capacity=N_KF, point_capacity=N_POINTS)
    return tables, call


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=15)
    a = ap.parse_args()
    _lib.require_gpu()
    tables, call = scene()
    only = {k: v for k, v in tables.items() if k != "n_kf"}
    with local_map.LocalMap(N_KF, **only) as h:
        out = dict(slot_cleared=np.zeros(N_FRAME, np.uint8), local_kf=np.zeros(N_KF, np.int32), local_point=np.zeros(N_POINTS, np.int32),
                   counts=np.zeros(N_KF, np.int32))
        update = lambda: h.update(call["frame_point"], None, None, call["prev_local_kf"], kf_capacity=N_KF, point_capacity=N_POINTS, out=out)
        r = update()
        device = dict(update=timed(update, a.repeats, a.warmup))
        device["replace"] = timed(lambda: h.replace(N_KF, **only), max(a.repeats // 10, 3), 2)
        ten = np.arange(10, dtype=np.int32)
        device["set_bad_10"] = timed(lambda: h.set_bad(ten, tables["point_bad"][:10], ten[:2], tables["kf_bad"][:2]), a.repeats, a.warmup)
        again = update()
        assert again.local_points.tobytes() == r.local_points.tobytes() and again.local_kf.tobytes() == r.local_kf.tobytes()
    with tempfile.TemporaryDirectory() as d:
        d = pathlib.Path(d)
        exe = host_prog.build("localmap_prog", d)
        host = P.run_ops(exe, d, [P.op_create(tables), P.op_timed(call, N_KF, a.host_repeats)])[1]
    assert host["rc"] == 0 and (host["n_local_kf"], host["ref_kf"], host["n_local_points"]) == (len(r.local_kf), r.ref_kf, len(r.local_points))
    print(json.dumps(dict(shape=dict(n_kf=N_KF, slots_per_keyframe=SLOTS, total_slots=int(tables["slot_off"][-1]), n_points=N_POINTS,
                                     n_observations=int(len(tables["obs_kf"])), frame_slots=N_FRAME),
                          result=dict(voted=bool(r.voted), n_local_kf=int(len(r.local_kf)), ref_kf=r.ref_kf, n_local_points=int(len(r.local_points))),
                          device_ms=device, host_build_update_median_ms=round(host["median_us"] / 1e3, 4))))


if __name__ == "__main__":
    main()
