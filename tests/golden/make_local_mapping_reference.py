"""Writes tests/golden/local_mapping_reference.npz: what the reference's own LocalMapping.cc and MapPoint.cc (oracle/_ref/ref_localmapping,
built by `make -C oracle ref` where the reference's sources are) compute on the scenes of tests/local_mapping_pin_cases.py -- per
triangulation scene which matches became map points, their positions, descriptors, normals and distance ranges, both CheckSemantics results
and the F12 handed to the matcher; per refresh scene which points were touched and what they hold afterwards; the cosine of
LocalMapping.cc:308 over 75 000 depths (as a digest and its first rows) with the size of the type g++ gives that expression; with every
scene a digest of its inputs.  Recorded results only.  tests/test_pin_local_mapping.py reads the file where the reference is absent and,
where it is present, requires that this script writes the same bytes again.

    python tests/golden/make_local_mapping_reference.py [output directory]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import local_mapping_pin_cases as P  # noqa: E402
import solver_pin_cases as S  # noqa: E402


def write(out_dir):
    assert P.reference_program(), "oracle/_ref/ref_localmapping is needed: make -C oracle ref"
    path = os.path.join(out_dir, os.path.basename(P.GOLDEN))
    entries = {}
    for name, e in P.live_entries().items():
        entries[name] = P.reduce_facts({k: v for k, v in e.items() if k != "inputs"})
        if "inputs" in e:
            entries[name]["inputs"] = e["inputs"]
    # the libm values themselves are kept as a digest; their largest distance from the float64 cosine is recorded beside it
    entries["cos"]["libm_worst_ulps"] = P.np.array([P.cosine_worst_ulps(P.live_entries()["cos"]["cos"][:, 0])])
    S.write_fixture(path, entries)
    assert os.path.getsize(path) < 256 * 1024
    return path


if __name__ == "__main__":
    p = write(sys.argv[1] if len(sys.argv) > 1 else HERE)
    print(p, os.path.getsize(p), "bytes")
