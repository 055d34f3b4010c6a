"""Times sivo_localmap_ba_window, the window of Optimizer::LocalBundleAdjustment on the resident map, beside the host walk it replaces, at
maps of 300, 1000 and 3000 keyframes shaped as tools/localmap_probe.py makes them (2000 slots a keyframe, about 60 % filled, 200 points a
keyframe observed by 3 to 20 neighbours each).  pKF is the newest keyframe, its covisibles the 20 before it.

Per map: the median of 15 calls of the C entry point with its arrays ready (a host clock around the call: one upload, the launches, two downloads, two
synchronisations inside the library); the median of 15 runs of the host walk — optimizer_detail::gather_local_ba(pKF) of
sivo_amd/api/orbslam/OptimizerAdapter.h over the stand-in object graph of tests/ba_window_adapter_prog.cpp, one thread, this box — and of
what the adapter does around the device call (the arrays filled by index); and one sivo_local_ba of the window, for the call's share of it.
One JSON line per map.  No pass mark; needs nothing outside the repository.
    python tools/ba_window_probe.py [--sizes 300 1000 3000] [--repeats 15]"""
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
import ba_window_cases as P  # noqa: E402
import host_prog  # noqa: E402
import localmap_cases as LC  # noqa: E402
from sivo_amd import _lib, local_map, optimizer  # noqa: E402

SLOTS, POINTS_PER_KF, WINDOW, COVISIBLES = 2000, 200, 15, 20


def scene(n_kf, seed=1):
    """The tables, the candidates and mObservations' idx of every observation."""
    rng = np.random.default_rng(seed)
    n_points = POINTS_PER_KF * n_kf
    centre = np.sort(rng.integers(0, n_kf, n_points))
    held = [[] for _ in range(n_kf)]
    obs = []
    for p in range(n_points):
        lo, hi = max(0, centre[p] - WINDOW), min(n_kf, centre[p] + WINDOW + 1)
        mine = np.sort(rng.choice(np.arange(lo, hi), min(int(rng.integers(3, 21)), hi - lo), replace=False))
        mine = [int(k) for k in mine if len(held[k]) < SLOTS * 6 // 10]
        for k in mine:
            held[k].append(p)
        obs.append(mine)
    slots, where = [], {}
    for k in range(n_kf):                                           # the keyframe's points scattered over its 2000 slots, the rest null
        s = np.full(SLOTS, -1, np.int32)
        at = np.sort(rng.choice(SLOTS, len(held[k]), replace=False))
        s[at] = held[k]
        slots.append(s)
        where[k] = dict(zip(held[k], at.tolist()))
    covis = [[c for d in range(1, 11) for c in (k - d, k + d) if 0 <= c < n_kf] for k in range(n_kf)]
    obs_off, obs_kf = LC.R.csr(obs, np.int32)
    slot_off, slot_point = LC.R.csr(slots, np.int32)
    covis_off, covis_kf = LC.R.csr(covis, np.int32)
    child_off, child_kf = LC.R.csr([[k + 1] if k + 1 < n_kf else [] for k in range(n_kf)], np.int32)
    kf_bad = (rng.random(n_kf) < 0.02).astype(np.uint8)
    kf_bad[n_kf - 1] = 0
    tables = dict(n_kf=n_kf, obs_off=obs_off, obs_kf=obs_kf, point_bad=(rng.random(n_points) < 0.01).astype(np.uint8), kf_bad=kf_bad,
                  slot_off=slot_off, slot_point=slot_point, covis_off=covis_off, covis_kf=covis_kf, child_off=child_off, child_kf=child_kf,
                  parent=np.arange(-1, n_kf - 1, dtype=np.int32), kf_order=None)
    cand = np.arange(n_kf - 1, n_kf - 2 - COVISIBLES, -1, dtype=np.int32)
    obs_idx = np.array([where[k][p] for p, row in enumerate(obs) for k in row], np.int32)
    return tables, cand, obs_idx


def median_ms(call, repeats):
    call()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        t.append(time.perf_counter() - t0)
    return round(float(np.median(t)) * 1e3, 4)


def raw_call(h, cand):
    """The C ABI call with every array ready, sized by what no result can exceed."""
    K, Pn, n_obs, n_slot = h.sizes()[:4]
    kf, pt, off = np.zeros((2, K), np.int32), np.zeros(min(Pn, n_slot), np.int32), np.zeros(min(Pn, n_slot) + 1, np.int64)
    edge, counts = np.zeros((2, n_obs), np.int32), np.zeros(4, np.int64)
    edge[:] = 0                                                     # (touched once: no page of it is first mapped inside a timed call)
    f = _lib.lib().sivo_localmap_ba_window

    def call():
        _lib.check(f(h._h, len(cand), cand.ctypes.data, 0, None, 0, None, 0, None, K, kf[0].ctypes.data, kf[1].ctypes.data, len(pt), pt.ctypes.data,
                     off.ctypes.data, n_obs, edge[0].ctypes.data, edge[1].ctypes.data, counts.ctypes.data))
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[300, 1000, 3000])
    ap.add_argument("--repeats", type=int, default=15)
    a = ap.parse_args()
    _lib.require_gpu()
    with tempfile.TemporaryDirectory() as d:
        d = pathlib.Path(d)
        exe = host_prog.build("ba_window_adapter_prog", d)
        for n_kf in a.sizes:
            tables, cand, obs_idx = scene(n_kf)
            only = {k: v for k, v in tables.items() if k != "n_kf"}
            with local_map.LocalMap(n_kf, **only) as h:
                first = h.ba_window(cand)
                device_ms = median_ms(raw_call(h, cand), a.repeats)
                again = h.ba_window(cand)
            assert [x.tobytes() for x in first] == [x.tobytes() for x in again]
            blob = LC.tables_blob(tables) + P.i32(n_kf - 1, 0) + P.arr(cand, np.int32) + P.arr(obs_idx, np.int32)
            raw = host_prog.run(exe, d, "time", blob, extra_args=[a.repeats], timeout=1200)
            walk_us, _, around_us = np.frombuffer(raw, np.float64, 3)
            sizes = np.frombuffer(raw, np.int64, 4, 24).tolist()
            local_kf, fixed_kf, local_points, edge_off, edge_pose, edge_slot = first
            assert sizes == [len(local_kf), len(local_points), len(fixed_kf), len(edge_pose)] and (edge_slot >= 0).all()
            res = dict(counts=np.array([len(local_kf), len(local_points), len(fixed_kf), len(edge_pose)]), local_kf=local_kf, fixed_kf=fixed_kf,
                       local_point=local_points, edge_off=edge_off, edge_pose=edge_pose, edge_slot=edge_slot)
            solver = P.solver_arrays(res)
            local_ba_ms = median_ms(lambda: optimizer.local_ba(*solver), 5)
            print(json.dumps(dict(shape=dict(n_kf=n_kf, total_slots=int(tables["slot_off"][-1]), n_points=len(tables["point_bad"]),
                                             n_observations=len(tables["obs_kf"]), candidates=len(cand)),
                                  window=dict(local_kf=sizes[0], local_points=sizes[1], fixed_kf=sizes[2], edges=sizes[3]),
                                  device_call_median_ms=device_ms, adapter_around_the_call_median_ms=round(float(around_us) / 1e3, 4),
                                  host_walk_median_ms=round(float(walk_us) / 1e3, 4), local_ba_median_ms=local_ba_ms,
                                  device_call_share_of_local_ba=round(device_ms / local_ba_ms, 4))), flush=True)


if __name__ == "__main__":
    main()
