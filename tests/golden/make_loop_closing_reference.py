"""Writes tests/golden/loop_closing_reference.npz: what the reference's own LoopClosing.cc, KeyFrame.cc, MapPoint.cc, Map.cc and Converter.cc
(oracle/_ref/ref_loopclosing, built by `make -C oracle ref` where the reference's sources are) leave on the scenes of
tests/loop_closing_pin_cases.py -- per loop scene what LoopClosing::CorrectLoop has made of the map when it calls
Optimizer::OptimizeEssentialGraph, in the terms of sivo_loop_correct, and what the loop fusion and SearchAndFuse left of slots, observations,
flags and descriptors; per tree what LoopClosing::RunGlobalBundleAdjustment leaves, in the terms of sivo_gba_propagate.  A fact of more than
map_graph_pin_cases.SHA_FROM bytes that no test marked gpu reads is kept as the SHA-256 of its bytes; with every entry a digest of its
inputs.  Recorded results only.  tests/test_pin_loop_closing.py reads the file where the reference is absent and, where it is present,
requires that this script writes the same bytes again.

    python tests/golden/make_loop_closing_reference.py [output directory]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import loop_closing_pin_cases as P  # noqa: E402
import map_graph_pin_cases as M  # noqa: E402
import solver_pin_cases as S  # noqa: E402


def write(out_dir):
    assert P.reference_program(), "oracle/_ref/ref_loopclosing is needed: make -C oracle ref"
    path = os.path.join(out_dir, os.path.basename(P.GOLDEN))
    entries = {}
    for e in P.ENTRIES:
        entries[e] = M.pack_entry(dict(P.reduce_facts(e, P.live_facts(e)), inputs=P.inputs_digest(e)))
    S.write_fixture(path, entries)
    assert os.path.getsize(path) < 256 * 1024
    return path


if __name__ == "__main__":
    p = write(sys.argv[1] if len(sys.argv) > 1 else HERE)
    print(p, os.path.getsize(p), "bytes")
