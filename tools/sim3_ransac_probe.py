"""Wall time of sivo_sim3_ransac_batch (one call: staging, one launch, one synchronisation) at 300 hypotheses per candidate for
(candidates, pairs) = (1, 100), (8, 100), (8, 500), (1, 2000), 30 % gross outliers.  Each case runs in a child process of its own
under `timeout -k 10`; the children run one after another and the first failure ends the probe (nothing is started on the GPU
after a fault).  Prints one JSON line per case.

    python tools/sim3_ransac_probe.py [--cases 1x100,8x100,8x500,1x2000] [--reps 20]"""
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
    import sim3_ransac_restatement as R
    from sivo_amd import sim3_solver
    k, n = (int(v) for v in case.split("x"))
    probs = []
    for i in range(k):
        sc = R.make_scene(n, 100 + i, outliers=0.3, n_hyp=300)
        probs.append({"pairs": sc["pairs"], "k1": sc["k1"], "k2": sc["k2"], "triples": sc["triples"], "min_inliers": 20, "fix_scale": True})
    for _ in range(3):
        res = sim3_solver.sim3_ransac_batch(probs)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); sim3_solver.sim3_ransac_batch(probs); t.append(time.perf_counter() - t0)
    print(json.dumps({"candidates": k, "pairs": n, "hypotheses": 300, "ms_median": 1e3 * float(np.median(t)), "ms_min": 1e3 * min(t),
                      "first_accept": [r["first_accept"] for r in res], "best_count": [int(r["count"][r["best"]]) for r in res]}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1x100,8x100,8x500,1x2000")
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
