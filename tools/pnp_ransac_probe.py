"""Wall time of sivo_pnp_ransac_batch (one call: staging, the hypothesis launch, the scan, the refine launch, two synchronisations)
at 300 hypotheses per candidate for (candidates, correspondences) = (5, 100), (5, 500), (5, 2000), (1, 100), 30 % gross outliers,
0.5 px noise, the Tracking parameters (minInliers = max(10, N / 2)).  Each case runs in a child process of its own
under `timeout -k 10`; the children run one after another and the first failure ends the probe (nothing is started on the GPU
after a fault).  Prints one JSON line per case.

    python tools/pnp_ransac_probe.py [--cases 5x100,5x500,5x2000,1x100] [--reps 20]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(case, reps):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import pnp_ransac_restatement as R
    from sivo_amd import pnp_solver
    k, n = (int(v) for v in case.split("x"))
    probs = []
    for i in range(k):
        sc = R.make_scene(100 + i, n, noise=0.5, outliers=0.3)
        S = R.draw_samples(np.random.RandomState(i), n, 300)
        probs.append({"points": sc["pts"], "K": sc["K"], "samples": S, "min_inliers": max(10, n // 2)})
    for _ in range(3):
        res = pnp_solver.pnp_ransac_batch(probs)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); pnp_solver.pnp_ransac_batch(probs); t.append(time.perf_counter() - t0)
    none = [dict(p, best_in=n) for p in probs]             # no record: the hypothesis launch alone
    t1 = []
    for _ in range(reps):
        t0 = time.perf_counter(); pnp_solver.pnp_ransac_batch(none); t1.append(time.perf_counter() - t0)
    print(json.dumps({"candidates": k, "points": n, "hypotheses": 300, "ms_median": 1e3 * float(np.median(t)), "ms_min": 1e3 * min(t),
                      "ms_median_hypotheses_only": 1e3 * float(np.median(t1)), "records": [int(r["n_records"]) for r in res],
                      "record_counts": [r["count"][r["refined"] >= 0].tolist() for r in res],
                      "best_refined": [int(r["refined"].max()) for r in res]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="5x100,5x500,5x2000,1x100")
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
