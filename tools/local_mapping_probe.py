"""Wall time per call (staging, one launch, one synchronisation; median of --reps after warm-up) of
    sivo_triangulate        at 100, 500 and 2000 matches of one keyframe pair                      (cases tri:N)
    sivo_mappoint_refresh   at (points, observations per point) = (500, 10), (3000, 10), (3000, 30) (cases refresh:PxN)
and, as the yardstick, of the call that precedes triangulation in LocalMapping::CreateNewMapPoints:
    sivo_search_for_triangulation between two keyframes of 1000 keys each                           (case search:1000)
Each case runs in a child process of its own under `timeout -k 10`; the children run one after another and the first failure ends the
probe (nothing is started on the GPU after a fault).  Prints one JSON line per case.  The kernel time comes from a run of its own:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/local_mapping_probe.py --one tri:500 --reps 20

    python tools/local_mapping_probe.py [--cases tri:100,...] [--reps 20]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = "tri:100,tri:500,tri:2000,refresh:500x10,refresh:3000x10,refresh:3000x30,search:1000"


def timed(call, reps):
    import numpy as np
    for _ in range(3):
        res = call()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); call(); t.append(time.perf_counter() - t0)
    return res, {"ms_median": 1e3 * float(np.median(t)), "ms_min": 1e3 * min(t)}


def one(case, reps):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    from sivo_amd import local_mapping as LM
    kind, size = case.split(":")
    if kind == "tri":
        import triangulate_restatement as TR
        p = TR.make_problem(200, int(size), min_margin=0)
        res, t = timed(lambda: LM.triangulate(p["kf1"], p["kf2"], p["matches"], p["ratio_factor"], p["state_cov"], p["th_confidence"],
                                              p["th_entropy"]), reps)
        out = {"matches": int(size), "accepted": int((res["status"] == 0).sum())}
    elif kind == "refresh":
        import mappoint_restatement as MR
        npts, nobs = (int(v) for v in size.split("x"))
        s = MR.make_points(201, [nobs] * npts)
        res, t = timed(lambda: LM.refresh_map_points(**s), reps)
        out = {"points": npts, "observations": nobs, "flagged": int((res["flags"] != 0).sum())}
    else:
        from sivo_amd import matcher as M
        from search_scene import node_lists
        n = int(size)
        rng = np.random.default_rng(202)
        keys = []
        for _ in range(2):
            k = np.zeros(n, M.KP_DTYPE)
            k["x"], k["y"], k["octave"], k["angle"], k["size"] = rng.uniform(20, 1220, n), rng.uniform(20, 350, n), rng.integers(0, 8, n), rng.uniform(0, 360, n), 31
            keys.append(k)
        keys[1]["x"], keys[1]["y"] = keys[0]["x"] + 6, keys[0]["y"] + 2               # image 2 = image 1 translated by (6, 2)
        d1 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        d2 = d1 ^ (rng.random((n, 32, 8)) < 0.05).dot(1 << np.arange(8)).astype(np.uint8)
        ur = [np.where(rng.random(n) < 0.7, k["x"] - rng.uniform(3, 60, n), -1).astype(np.float32) for k in keys]
        scale = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
        F2 = M.MatchFrame(keys[1], ur[1], d2, (0, 1241, 0, 376), scale, scale * scale, 1 / (scale * scale))
        off1, idx1, off2, idx2 = node_lists(n, n, rng, n_nodes=40)
        has = np.zeros(n, np.uint8)
        F12 = np.array([[0, 0, 2.0], [0, 0, -6.0], [-2.0, 6.0, 0]], np.float32).T.copy()
        res, t = timed(lambda: M.search_for_triangulation(off1, idx1, off2, idx2, keys[0], ur[0], has, d1, F2, has, F12, 2000.0, 170.0, False, True), reps)
        out = {"keys": n, "matches": int(res[0])}
    print(json.dumps({"case": case, **out, **t}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=CASES)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--one", default="")
    a = ap.parse_args()
    if a.one:
        one(a.one, a.reps)
        return 0
    for case in a.cases.split(","):
        rc = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--one", case,
                             "--reps", str(a.reps)]).returncode
        if rc != 0:
            print(json.dumps({"case": case, "error": f"exit status {rc}: probe stopped"}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
