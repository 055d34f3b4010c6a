"""Wall time of sivo_sim3_optimize (one call: staging, one launch, one synchronisation) and of sivo_sim3_optimize_batch (8 problems,
one launch) for n = 100 / 500 / 2000 pairs (20 % gross outliers: both optimize() calls run).  Each size runs in a child process of
its own under `timeout -k 10`; the children run one after another and the first failure ends the probe (nothing is started on the
GPU after a fault).  Prints one JSON line per size.

    python tools/sim3_probe.py [--sizes 100,500,2000] [--reps 20]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(n, reps):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import sim3_restatement as R
    from sivo_amd import optimizer
    # the scene: the generator's geometry without running the restatement (make_scene's near-threshold check is for the tests)
    sc = R.make_scene(n, 1, outliers=0.2, tries=1, margin=-1.0) if n <= 500 else None
    if sc is None:
        base = R.make_scene(500, 1, outliers=0.2, tries=1, margin=-1.0)
        m = np.concatenate([base["matches"]] * (n // 500 + 1))[:n]
        sc = dict(base, matches=m)
    args = (sc["s12"], sc["k1"], sc["k2"], sc["matches"], 10.0, True)
    for _ in range(3):
        optimizer.sim3_optimize(*args)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); r = optimizer.sim3_optimize(*args); t.append(time.perf_counter() - t0)
    probs = [{"s12": sc["s12"], "k1": sc["k1"], "k2": sc["k2"], "matches": sc["matches"]}] * 8
    optimizer.sim3_optimize_batch(probs)
    tb = []
    for _ in range(reps):
        t0 = time.perf_counter(); optimizer.sim3_optimize_batch(probs); tb.append(time.perf_counter() - t0)
    print(json.dumps({"n": n, "single_ms_median": 1e3 * float(np.median(t)), "single_ms_min": 1e3 * min(t),
                      "batch8_ms_median": 1e3 * float(np.median(tb)), "iterations": r["iterations"], "trials": r["trials"],
                      "inliers": r["inliers"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,500,2000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--one", type=int, default=0)
    a = ap.parse_args()
    if a.one:
        one(a.one, a.reps)
        return 0
    for n in [int(v) for v in a.sizes.split(",")]:
        rc = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--one", str(n),
                             "--reps", str(a.reps)]).returncode
        if rc != 0:
            print(json.dumps({"n": n, "error": f"exit status {rc}: probe stopped"}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
