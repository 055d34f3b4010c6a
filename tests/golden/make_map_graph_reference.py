"""Writes tests/golden/map_graph_reference.npz: what the reference's own KeyFrame.cc, MapPoint.cc, Map.cc, LocalMapping.cc and Tracking.cc
(oracle/_ref/ref_mapgraph) and its Optimizer.cc (oracle/_ref/ref_bawindow), built by `make -C oracle ref` where the reference's sources
are, leave on the scenes of tests/map_graph_pin_cases.py -- per entry the graph after KeyFrame::UpdateConnections,
LocalMapping::KeyFrameCulling and LocalMapping::MapPointCulling, what Tracking::UpdateLocalMap leaves, and the window
Optimizer::LocalBundleAdjustment has built when it starts to optimise; a fact of more than map_graph_pin_cases.SHA_FROM bytes that no test
marked gpu reads is kept as the SHA-256 of its bytes; with every entry a digest of its inputs.  Recorded results only.
tests/test_pin_map_graph.py reads the file where the reference is absent and, where it is present, requires that this script writes the
same bytes again.

    python tests/golden/make_map_graph_reference.py [output directory]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import map_graph_pin_cases as M  # noqa: E402
import solver_pin_cases as S  # noqa: E402


def write(out_dir):
    assert M.reference_program() and M.reference_program("ref_bawindow"), "oracle/_ref/ref_mapgraph and ref_bawindow are needed: make -C oracle ref"
    path = os.path.join(out_dir, os.path.basename(M.GOLDEN))
    entries = {}
    for e in M.ENTRIES:
        entries[e] = M.pack_entry(dict(M.reduce_facts(M.live_facts(e)), inputs=M.inputs_digest(e)))
    S.write_fixture(path, entries)
    assert os.path.getsize(path) < 256 * 1024
    return path


if __name__ == "__main__":
    p = write(sys.argv[1] if len(sys.argv) > 1 else HERE)
    print(p, os.path.getsize(p), "bytes")
