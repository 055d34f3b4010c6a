"""Writes tests/golden/bowdb_reference.npz: what the reference's own KeyFrameDatabase.cc over DBoW2's real vocabulary
(oracle/_ref/ref_kfdb, built by `make -C oracle ref` where the reference's sources are) leaves behind on the scripts of
tests/bowdb_pin_cases.py -- per script every returned candidate vector in its order, every change of the six query members of every
keyframe from one operation to the next, and a digest of the script's inputs.  Recorded results only.  tests/test_pin_bow_database.py reads
the file where the reference is absent and, where it is present, requires that this script writes the same bytes again.

    python tests/golden/make_bowdb_reference.py [output directory]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import bowdb_pin_cases as P  # noqa: E402
import solver_pin_cases as S  # noqa: E402


def write(out_dir):
    assert P.reference_program(), "oracle/_ref/ref_kfdb is needed: make -C oracle ref"
    path = os.path.join(out_dir, os.path.basename(P.GOLDEN))
    S.write_fixture(path, P.fixture_entries())
    assert os.path.getsize(path) < 256 * 1024
    return path


if __name__ == "__main__":
    p = write(sys.argv[1] if len(sys.argv) > 1 else HERE)
    print(p, os.path.getsize(p), "bytes")
