#!/usr/bin/env python3
"""The two paths of the bundle adjustment's reduced camera system on tests/ba_sparse_cases.windowed_scene, rung by rung: 32 .. 512 free
keyframes dense and sparse, 1024 and 2048 sparse only.

    ba_sparse_probe.py                 the whole ba_optimize(..., 1) call (host plan, upload, one LM trial, download) per rung and path,
                                       one warm-up and the median of 5 calls; the host plan alone (sivo_ba_analyze) beside it
    ba_sparse_probe.py --kernels DIR   additionally one child process per rung under `rocprofv3 --kernel-trace --stats`: the mean time
                                       per launch of the Schur kernel and of the factor + solve kernel of each path
    ba_sparse_probe.py --rungs 64,128  a subset of the rungs

The crossover N of AUTO (BA_SPARSE_MIN_FREE in sivo_amd/csrc/ba_sparse_plan.hpp) is the smallest rung from 64 up at which
the whole sparse call is faster than the dense one."""
import argparse
import csv
import glob
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RUNGS = (32, 64, 128, 256, 512, 1024, 2048)
DENSE_MAX = 512
SCHUR = {"dense": ("ba_schur_kernel",), "sparse": ("ba_sparse_schur_kernel",)}
SOLVE = {"dense": ("ba_dense_solve_kernel", "ba_dense_solve_lds_kernel"), "sparse": ("ba_sparse_solve_kernel",)}


def problem(n_free):
    import ba_sparse_cases as S
    poses, pts, edges, intr = S.windowed_scene(21, n_free + 2)
    rng = np.random.default_rng(3)
    fixed = np.zeros(len(poses), np.uint8); fixed[:2] = 1
    P0 = poses.copy(); P0[2:, 9:] += rng.normal(0, 0.02, (n_free, 3))
    return P0, fixed, pts + rng.normal(0, 0.05, pts.shape), edges, intr


def calls(n_free, solvers, runs=5):
    """{solver: median ms of the whole call}, the host plan's ms, the problem's sizes"""
    from sivo_amd import optimizer
    P0, fixed, X0, edges, intr = problem(n_free)
    out = {}
    for solver in solvers:
        optimizer.ba_optimize(P0, fixed, X0, edges, intr, 1, solver=solver)
        ts = []
        for _ in range(runs):
            t0 = time.perf_counter(); g = optimizer.ba_optimize(P0, fixed, X0, edges, intr, 1, solver=solver); ts.append(1e3 * (time.perf_counter() - t0))
        out[solver] = (float(np.median(ts)), g["trials"])
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter(); a = optimizer.ba_analyze(fixed, len(X0), edges, solver="sparse"); ts.append(1e3 * (time.perf_counter() - t0))
    return out, float(np.median(ts)), a, len(X0), len(edges)


def kernel_means(stats_csv):
    """kernel name (without arguments and namespace) -> (launches, mean us) from a rocprofv3 kernel_stats file"""
    res = {}
    with open(stats_csv, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "").split("(")[0].split("::")[-1].strip()
            n = int(float(row.get("Calls", 0)))
            total = float(row.get("TotalDurationNs", 0.0))
            if n:
                res[name] = (n, total / n / 1e3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", metavar="DIR", help="per-kernel times: one child per rung under rocprofv3, its output below DIR")
    ap.add_argument("--rungs", default=",".join(map(str, RUNGS)))
    ap.add_argument("--worker", type=int, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        calls(a.worker, ("dense", "sparse") if a.worker <= DENSE_MAX else ("sparse",))
        return
    rungs = [int(v) for v in a.rungs.split(",")]
    print("free kf | points | edges | S blocks | L blocks | levels | dense call ms | sparse call ms | host plan ms (share of the sparse call)"
          + (" | dense schur / solve us | sparse schur / solve us" if a.kernels else ""))
    for n in rungs:
        solvers = ("dense", "sparse") if n <= DENSE_MAX else ("sparse",)
        t, plan, an, nx, ne = calls(n, solvers)
        line = (f"{n:7d} | {nx:6d} | {ne:6d} | {an['s_blocks']:6d} | {an['l_blocks']:6d} | {an['levels']:5d} | "
                + (f"{t['dense'][0]:10.3f}" if "dense" in t else "         -") + f" | {t['sparse'][0]:10.3f} | {plan:8.3f} ({plan / t['sparse'][0]:.2f})")
        if a.kernels:
            out = os.path.join(a.kernels, f"rung_{n}")
            os.makedirs(out, exist_ok=True)
            # (a fresh child: the profiled program goes behind `--`)
            r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable,
                                os.path.abspath(__file__), "--worker", str(n)], capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.exit(f"rocprofv3 failed at rung {n}: {r.stderr[-2000:]}")
            found = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
            if not found:
                sys.exit(f"no kernel_stats file below {out}")
            k = kernel_means(found[0])
            for path in ("dense", "sparse"):
                if path in solvers:
                    sch = sum(k[name][1] for name in SCHUR[path] if name in k)
                    sol = sum(k[name][1] for name in SOLVE[path] if name in k)
                    line += f" | {sch:9.1f} / {sol:9.1f}"
                else:
                    line += " |         - /         -"
        print(line, flush=True)


if __name__ == "__main__":
    main()
