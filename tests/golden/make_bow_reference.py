"""Writes tests/golden/bow_reference.npz: what the reference's own DBoW2 computes on the test vocabularies of tests/bow_restatement.py.
Compiles tests/bow_reference_driver.cpp against the reference's TemplatedVocabulary.h, FORB.cpp, BowVector.cpp, FeatureVector.cpp and
ScoringObject.cpp (over the cv::Mat / cv::FileStorage stand-in under tests/bow_reference_shim) in a temporary directory, runs it, and
records inputs and results: data only.  The inputs avoid the two places where the reference itself is indeterminate: the vocabulary files
have no final newline, and only those levelsup are recorded at which no leaf lies above level L - levelsup.

    python tests/golden/make_bow_reference.py <reference checkout> [output directory]"""
import io
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
import bow_restatement as BR  # noqa: E402

N_FEATURES = 200


def levels_without_a_leaf_above(v):
    return [lv for lv in BR.levels(v) if not ((v.level[1:] < v.L - lv) & (v.is_leaf > 0)).any()]


def write(reference, out_dir):
    dbow = os.path.join(reference, "dependencies", "DBoW2")
    entries = {"names": np.array(list(BR.VOCS))}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "driver")
        srcs = [os.path.join(dbow, "DBoW2", f) for f in ("FORB.cpp", "BowVector.cpp", "FeatureVector.cpp", "ScoringObject.cpp")]
        srcs += [os.path.join(dbow, "DUtils", f) for f in ("Random.cpp", "Timestamp.cpp")]
        subprocess.run(["g++", "-std=c++14", "-O2", "-w", "-ffp-contract=off", "-I" + os.path.join(TESTS, "bow_reference_shim"), "-I" + os.path.join(dbow, "DBoW2"),
                        os.path.join(TESTS, "bow_reference_driver.cpp"), *srcs, "-o", exe], check=True)
        for i, name in enumerate(BR.VOCS):
            v = BR.voc(name)
            levels = levels_without_a_leaf_above(v)
            f1, f2 = BR.features(300 + i, N_FEATURES, v), BR.features(400 + i, N_FEATURES, v)
            fvoc, fin, fout = (os.path.join(tmp, x) for x in ("voc.txt", "in.bin", "out.bin"))
            with open(fvoc, "w") as f:
                f.write(v.text(final_newline=False))
            with open(fin, "wb") as f:
                f.write(np.array([len(levels)] + levels, np.int64).tobytes())
                for s in (f1, f2):
                    f.write(np.array([len(s)], np.int64).tobytes() + s.tobytes())
            subprocess.run([exe, fvoc, fin, fout], check=True)
            raw, at = open(fout, "rb").read(), 0
            entries.update({f"{i}_desc": v.desc, f"{i}_weight": v.weight, f"{i}_levelsup": np.array(levels, np.int64), f"{i}_features": f1, f"{i}_features2": f2})
            for lv in levels:
                n, nw, nf, m = np.frombuffer(raw, np.int64, 4, at)
                at += 32
                for key, cnt, dt in (("word", n, np.int32), ("node", n, np.int32), ("words", nw, np.int32), ("fv_nodes", nf, np.int32),
                                     ("fv_offsets", nf + 1, np.int32), ("fv_features", m, np.int32), ("values", nw, np.float64)):
                    entries[f"{i}_{lv}_{key}"] = np.frombuffer(raw, dt, int(cnt), at).copy()
                    at += int(cnt) * np.dtype(dt).itemsize
            entries[f"{i}_scores"] = np.frombuffer(raw, np.float64, 2, at).copy()
            assert at + 16 == len(raw)
    path = os.path.join(out_dir, "bow_reference.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:          # fixed dates, no compression: the same bytes for the same results
        for key in sorted(entries):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(entries[key]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    return path


if __name__ == "__main__":
    p = write(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else HERE)
    print(p, os.path.getsize(p), "bytes")
