"""Times what keeps the resident local map current after one keyframe insertion, at the C ABI: sivo_localmap_replace with the full new
tables against sivo_localmap_apply with the delta, on the same box and in the same process.  Synthetic maps of 200 / 1000 / 3000 keyframes
of 2000 slots (200 points per keyframe, 3 to 9 neighbouring observers each, covisibility lists of 10, a chain of parents and children, a
kf_order that is not the identity); the delta is one insertion: 1 new keyframe, 30 neighbour keyframes whose rows are replaced, 1500 old
points that gain an observer and 300 new points.  The new tables `replace` sends are the export of the handle after `apply`.

Each figure is a host clock around the C call with the structs ready (the call ends in the library's synchronise).  Before every timed
apply the handle is put back to the old tables by an untimed replace.  Warm-up first, then medians and quartiles over the repeats, the two
calls alternating; one JSON line.  The host-side gather of the rows from an object graph is in neither figure.  No pass mark.
    python tools/localmap_delta_probe.py [--repeats 30] [--warmup 5] [--rungs 200,1000,3000]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sivo_amd import _lib, local_map  # noqa: E402

SLOTS, PER_KF, NEIGHBOURS, TOUCHED, NEW_POINTS = 2000, 200, 30, 1500, 300


def csr_of(lengths):
    off = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=off[1:])
    return off


def scene(K, seed=1):
    rng = np.random.default_rng(seed)
    Pn = K * PER_KF
    centre = np.sort(rng.integers(0, K, Pn))
    n_obs = rng.integers(3, 10, Pn)
    start = np.clip(centre - n_obs // 2, 0, K - n_obs)
    obs_off = csr_of(n_obs)
    row = np.repeat(np.arange(Pn), n_obs)
    obs_kf = (np.repeat(start, n_obs) + np.arange(obs_off[-1]) - obs_off[row]).astype(np.int32)
    order = np.argsort(obs_kf, kind="stable")                       # every keyframe's points, in point order, into its first slots
    kf_sorted, pt_sorted = obs_kf[order], row[order]
    pos = np.arange(len(order)) - np.searchsorted(kf_sorted, kf_sorted, side="left")
    keep = pos < SLOTS - 400                                        # room for the insertion's new points
    slot_point = np.full(K * SLOTS, -1, np.int32)
    slot_point[kf_sorted[keep].astype(np.int64) * SLOTS + pos[keep]] = pt_sorted[keep]
    steps = np.array([d for i in range(1, 6) for d in (-i, i)])
    covis_kf = ((np.arange(K)[:, None] + steps[None, :]) % K).astype(np.int32).ravel()
    tables = dict(obs_off=obs_off, obs_kf=obs_kf, point_bad=(rng.random(Pn) < 0.01).astype(np.uint8), kf_bad=(rng.random(K) < 0.02).astype(np.uint8),
                  slot_off=np.arange(K + 1, dtype=np.int64) * SLOTS, slot_point=slot_point, covis_off=np.arange(K + 1, dtype=np.int64) * 10,
                  covis_kf=covis_kf, child_off=np.minimum(np.arange(K + 1, dtype=np.int64), K - 1), child_kf=np.arange(1, K, dtype=np.int32),
                  parent=np.arange(-1, K - 1, dtype=np.int32), kf_order=rng.permutation(K).astype(np.int32))
    # the insertion: keyframe K, observed with the newest TOUCHED points, NEW_POINTS new points shared with two neighbours each
    touched = np.sort(rng.choice(np.arange(Pn - 4 * TOUCHED, Pn), TOUCHED, replace=False))
    new = np.arange(Pn, Pn + NEW_POINTS)
    t_len = n_obs[touched] + 1
    pr_off = csr_of(np.concatenate([t_len, np.full(NEW_POINTS, 3)]))
    pr_kf = np.empty(pr_off[-1], np.int32)
    for j, p in enumerate(touched):                                 # the old observers, then the new keyframe (the highest pointer)
        pr_kf[pr_off[j]:pr_off[j + 1] - 1] = obs_kf[obs_off[p]:obs_off[p + 1]]
        pr_kf[pr_off[j + 1] - 1] = K
    partner = rng.integers(K - NEIGHBOURS, K - 1, NEW_POINTS)
    pr_kf[pr_off[TOUCHED]:] = np.stack([partner, partner + 1, np.full(NEW_POINTS, K)], 1).ravel()
    point_rows = dict(idx=np.concatenate([touched, new]).astype(np.int32), obs_off=pr_off, obs_kf=pr_kf,
                      bad=np.zeros(TOUCHED + NEW_POINTS, np.uint8))
    kf_idx = np.arange(K - NEIGHBOURS, K + 1)
    slots = [slot_point[k * SLOTS:(k + 1) * SLOTS].copy() for k in kf_idx[:-1]]
    for p, a in zip(new, partner):                                  # a new point takes the last free slot of both partners
        for k in (a, a + 1):
            s = slots[k - (K - NEIGHBOURS)]
            s[np.flatnonzero(s < 0)[-1]] = p
    mine = np.full(SLOTS, -1, np.int32)
    mine[:TOUCHED + NEW_POINTS] = np.concatenate([touched, new])
    slots.append(mine)
    covis = [np.concatenate([[K], covis_kf[k * 10:k * 10 + 9]]) for k in kf_idx[:-1]] + [np.arange(K - 10, K)]
    child = [np.array([k + 1]) for k in kf_idx[:-1]] + [np.zeros(0, np.int32)]
    kf_rows = dict(idx=kf_idx.astype(np.int32), bad=np.zeros(NEIGHBOURS + 1, np.uint8), parent=(kf_idx - 1).astype(np.int32),
                   slot_off=csr_of([len(s) for s in slots]), slot_point=np.concatenate(slots).astype(np.int32),
                   covis_off=csr_of([len(c) for c in covis]), covis_kf=np.concatenate(covis).astype(np.int32),
                   child_off=csr_of([len(c) for c in child]), child_kf=np.concatenate(child).astype(np.int32))
    return tables, dict(n_kf=K + 1, n_points=Pn + NEW_POINTS, point_rows=point_rows, kf_rows=kf_rows)


def tables_struct(n_kf, t):
    return local_map._Tables(n_kf, len(t["point_bad"]), *[t[f].ctypes.data if t[f].size else None for f in local_map.TABLE_FIELDS])


def delta_struct(d):
    pr, kr = d["point_rows"], d["kf_rows"]
    p = lambda x: x.ctypes.data if x.size else None
    return local_map._Delta(C.sizeof(local_map._Delta), d["n_kf"], d["n_points"], len(pr["idx"]), p(pr["idx"]), p(pr["obs_off"]), p(pr["obs_kf"]),
                            p(pr["bad"]), len(kr["idx"]), p(kr["idx"]), p(kr["bad"]), p(kr["parent"]), p(kr["slot_off"]), p(kr["slot_point"]),
                            p(kr["covis_off"]), p(kr["covis_kf"]), p(kr["child_off"]), p(kr["child_kf"]), None)


def quartiles(t):
    q = np.percentile(np.array(t) * 1e3, [25, 50, 75])
    return dict(median_ms=round(float(q[1]), 4), q25_ms=round(float(q[0]), 4), q75_ms=round(float(q[2]), 4))


def rung(K, repeats, warmup):
    L = _lib.lib()
    old, delta = scene(K)
    with local_map.LocalMap(K, **old) as h:
        h.apply(delta["n_kf"], delta["n_points"], point_rows=delta["point_rows"], kf_rows=delta["kf_rows"])
        new = {f: v for f, v in h.export().items() if f != "n_kf"}
        st_old, st_new, st_delta = tables_struct(K, old), tables_struct(K + 1, new), delta_struct(delta)
        t_apply, t_replace = [], []
        for i in range(warmup + repeats):
            _lib.check(L.sivo_localmap_replace(h._h, C.byref(st_old)))                  # back to the old map: not timed
            t0 = time.perf_counter()
            rc = L.sivo_localmap_apply(h._h, C.byref(st_delta))
            t1 = time.perf_counter()
            _lib.check(rc)
            t2 = time.perf_counter()
            rc = L.sivo_localmap_replace(h._h, C.byref(st_new))
            t3 = time.perf_counter()
            _lib.check(rc)
            if i >= warmup:
                t_apply.append(t1 - t0); t_replace.append(t3 - t2)
        h.n_kf, h.n_points = K + 1, delta["n_points"]
        again = h.export()
        assert all(again[f].tobytes() == new[f].tobytes() for f in new)
    mb = lambda arrays: round(sum(a.nbytes for a in arrays) / 1e6, 3)
    return dict(n_kf=K, n_points=len(old["point_bad"]), observations=int(old["obs_off"][-1]), slots=K * SLOTS,
                delta_rows=dict(points=len(delta["point_rows"]["idx"]), keyframes=len(delta["kf_rows"]["idx"])),
                upload_mb=dict(replace=mb(new.values()), apply=mb(list(delta["point_rows"].values()) + list(delta["kf_rows"].values()))),
                replace=quartiles(t_replace), apply=quartiles(t_apply))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rungs", default="200,1000,3000")
    a = ap.parse_args()
    _lib.require_gpu()
    print(json.dumps(dict(probe="localmap_delta", repeats=a.repeats, warmup=a.warmup,
                          rungs=[rung(int(k), a.repeats, a.warmup) for k in a.rungs.split(",")])))


if __name__ == "__main__":
    main()
