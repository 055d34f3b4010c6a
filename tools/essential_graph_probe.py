"""Wall time of sivo_essential_graph_optimize (one call: ordering and symbolic factorisation on the host, staging, the LM steps,
the read-back) on synthetic maps of N = 300 / 1000 / 2000 keyframes (tests/essential_graph_restatement.make_map: about 6 edges per
keyframe, 3 older loop closures, the current loop's LoopConnections).  Prints per size: ms per call (median of --reps), trials,
iterations, nnz(L), the flops of one numeric factorisation, elimination-tree levels.  Each size runs in a child process of its own
under `timeout -k 10`; the first failure ends the probe (nothing is started on the GPU after a fault).  For the per-kernel split run
one size under `rocprofv3 --kernel-trace --stats -- python tools/essential_graph_probe.py --child N`.

    python tools/essential_graph_probe.py [--sizes 300,1000,2000] [--reps 10]"""
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
    import essential_graph_restatement as E
    from sivo_amd import optimizer
    m = E.make_map(n, 21, n_loops=3, covis=8, falloff=25, fix_scale=True)
    siw, fixed, vertex, e = E.gather(m)
    a = optimizer.essential_graph_analyze(fixed, e)
    r = optimizer.essential_graph_optimize(siw, fixed, e)          # (warm-up: buffers, code objects)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = optimizer.essential_graph_optimize(siw, fixed, e)
        ts.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    for _ in range(20):
        optimizer.essential_graph_analyze(fixed, e)
    host_ms = (time.perf_counter() - t0) * 1e3 / 20
    print(json.dumps({"keyframes": n, "edges": int(len(e)), "edges_per_kf": round(len(e) / n, 2), "ms": round(float(np.median(ts)), 3),
                      "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3), "host_symbolic_ms": round(host_ms, 3),
                      "iterations": r["iterations"], "trials": r["trials"], "chi2_start": r["chi2_start"], "chi2": r["chi2"], **a}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="300,1000,2000")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--child", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        one(args.child, args.reps)
        return
    for n in (int(v) for v in args.sizes.split(",")):
        rc = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", str(n), "--reps",
                             str(args.reps)]).returncode
        if rc != 0:
            print(json.dumps({"keyframes": n, "failed": rc}), flush=True)
            sys.exit(1)


if __name__ == "__main__":
    main()
