"""Writes tests/golden/pnp_solver_reference.npz and sim3_solver_reference.npz: what the reference's own PnPsolver.cc and
Sim3Solver.cc (oracle/_ref/ref_pnp, oracle/_ref/ref_sim3, built by `make -C oracle ref` where the reference's sources are) compute
on the problems of tests/solver_pin_cases.py -- per scene the counts, poses and inlier words (or their digest) of compute_pose /
ComputeSim3 + CheckInliers with a digest of the scene's inputs, the `run` transcripts, the constructors' gather, SetRansacParameters
over a grid.  Recorded results only.  tests/test_pin_solvers.py reads them where the reference is absent and, where it is present,
requires that this script writes the same bytes again.

    python tests/golden/make_solver_reference.py [output directory]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import solver_pin_cases as C  # noqa: E402


def write(out_dir):
    assert C.reference_program("ref_pnp") and C.reference_program("ref_sim3"), "oracle/_ref/ref_pnp and ref_sim3 are needed: make -C oracle ref"
    paths = {}
    for which in ("pnp", "sim3"):
        paths[which] = os.path.join(out_dir, os.path.basename(C.GOLDEN[which]))
        C.write_fixture(paths[which], C.fixture_entries(which))
    return paths


if __name__ == "__main__":
    for p in write(sys.argv[1] if len(sys.argv) > 1 else HERE).values():
        print(p, os.path.getsize(p), "bytes")
