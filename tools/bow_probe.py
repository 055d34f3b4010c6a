"""Times the place-recognition entry points on the device beside the host build of the same arithmetic: sivo_bow_transform
for 2000 features on a synthetic vocabulary of ORBvoc.txt's shape (k = 10, L = 6, 1 111 110 nodes, random descriptors), a batch of 32 such
sets, and sivo_bowdb_query against 300 / 1000 / 2000 stored vectors of 1000 words.  Each call ends in a stream synchronise inside the
library, so the host clock around it is the call's time; warm-up, then many repetitions, the median with p10 / p90 beside it.  The share of
the ordered L1-norm sum comes from the per-set kernel's own device-clock stamps, which only the diagnostic build takes
(libsivo_hip_diag.so, sivo_diag_bow_profile_read): a pass of its own after the product library has been timed.  Host figures: tests/bow_prog.cpp
built at -O2 here, `bench` mode, the same shapes.  One JSON line per figure.

    python tools/bow_probe.py [--out FILE] [--reps 200]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import host_prog  # noqa: E402


def full_voc(k, L, seed=1):
    rng = np.random.default_rng(seed)
    counts = [k ** l for l in range(1, L + 1)]
    first = np.cumsum([1] + counts)                       # id of the first node of each level (breadth first)
    parent = np.concatenate([np.repeat(np.arange(first[l] - (counts[l - 1] if l else 1), first[l]), k) for l in range(L)]).astype(np.int32)
    n = parent.shape[0]
    leaf = np.zeros(n, np.uint8)
    leaf[n - counts[-1]:] = 1
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    weight = np.where(leaf > 0, rng.uniform(0.5, 4.5, n), 0.0)
    return parent, leaf, desc, weight


def timed(fn, reps, warm=20):
    for _ in range(warm):
        fn()
    us = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        us.append(1e6 * (time.perf_counter() - t0))
    us = np.sort(us)
    return {"median_us": round(float(np.median(us)), 1), "p10_us": round(float(us[len(us) // 10]), 1), "p90_us": round(float(us[len(us) * 9 // 10]), 1), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    import torch
    from sivo_amd import _lib, bow
    _lib.require_gpu()
    lines = []

    def emit(what, **kw):
        rec = dict(what=what, measured_on=torch.cuda.get_device_name(0), **kw)
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    k, L, n = 10, 6, 2000
    voc = bow.Vocabulary.from_arrays(k, L, *full_voc(k, L))
    rng = np.random.default_rng(2)
    sets = [rng.integers(0, 256, (n, 32), dtype=np.uint8) for _ in range(32)]
    emit("vocabulary", k=k, L=L, nodes=voc.n_nodes, words=voc.n_words)
    r = timed(lambda: voc.transform(sets[0], 4), a.reps)
    words = len(voc.transform(sets[0], 4)["words"])
    with _lib.use("diag") as D:                                     # the same call in the diagnostic build, for the kernel's own stamps
        dvoc = bow.Vocabulary.from_arrays(k, L, *full_voc(k, L))
        D.sivo_diag_bow_profile_read.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double)]
        set_us, norm_us = [], []
        su, nu = C.c_double(), C.c_double()
        for i in range(20 + a.reps // 2):
            dvoc.transform(sets[0], 4)
            D.sivo_diag_bow_profile_read(C.byref(su), C.byref(nu))
            if i >= 20:
                set_us.append(su.value)
                norm_us.append(nu.value)
        del dvoc
    emit("sivo_bow_transform", n=n, levelsup=4, bow_words=words, diag_set_kernel_median_us=round(float(np.median(set_us)), 2),
         diag_norm_sum_median_us=round(float(np.median(norm_us)), 2), **r)
    emit("sivo_bow_transform_batch", sets=32, n=n, levelsup=4, **timed(lambda: voc.transform_batch(sets, 4), max(a.reps // 4, 20), warm=5))
    for stored in (300, 1000, 2000):
        db = bow.BowDatabase(voc)
        vecs = []
        for _ in range(stored + 1):
            w = np.sort(rng.choice(voc.n_words, 1000, replace=False)).astype(np.int32)
            w[::3] = np.arange(0, 1000, 3) * 7                              # a third of the words shared by every vector
            w = np.unique(w)
            vecs.append((w, np.full(len(w), 1.0 / len(w))))
        for w, v in vecs[:-1]:
            db.add(w, v)
        q = vecs[-1]
        shared = int(np.median(db.query(*q)["common"]))
        emit("sivo_bowdb_query", stored=stored, words_per_vector=1000, median_shared_words=shared, **timed(lambda: db.query(*q), a.reps))
    # the host build of the same arithmetic, the same shapes
    with tempfile.TemporaryDirectory() as tmp:
        exe = host_prog.build("bow_prog", tmp)
        for stored in (300, 1000, 2000):
            out = subprocess.run([exe, "bench", str(k), str(L), str(n), str(stored), "1000"], check=True, capture_output=True, text=True, timeout=600).stdout
            for ln in out.splitlines():
                rec = json.loads(ln)
                if rec["what"] == "host_transform" and stored != 300:
                    continue
                emit(rec.pop("what"), stored=stored if "query" in ln else None, **rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
