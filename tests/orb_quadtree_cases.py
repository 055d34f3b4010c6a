"""Scenes of the quadtree keypoint distribution (DistributeOctTree), each named for the branch it exists for; shared by the host tests
(tests/test_orb_quadtree_host.py) and the GPU tests (tests/test_gpu_orb_quadtree.py).  A scene is (keys, min_x, max_x, min_y, max_y,
n_features); keys are what FAST produces: integer x in [0, max_x - min_x), integer y, integer response in [0, 256); class_id numbers
the keys, so a kept key that was not copied whole from its input key shows."""
import struct

import numpy as np

import host_prog
from sivo_amd.orb import KP_DTYPE

MIN_B = 16                                      # the extractor's minBorder: regions start there, keys are relative to it
THREADS = 1024                                  # the kernel's workgroup
MAX_CELLS = 2048                                # its cell table
LDS_CANDIDATES = 4096                           # sets up to this size keep their candidates in LDS, larger ones in device scratch


def keys_of(x, y, response):
    k = np.zeros(len(x), KP_DTYPE)
    k["x"], k["y"], k["response"] = x, y, response
    k["size"], k["angle"], k["class_id"] = 7, -1, np.arange(len(x))
    return k


def uniform(seed, n, w, h, response_below=256):
    rng = np.random.default_rng(seed)
    return keys_of(rng.integers(0, w, n), rng.integers(0, h, n), rng.integers(0, response_below, n))


def clustered(seed, n_clusters, per, spread, w, h):
    rng = np.random.default_rng(seed)
    n = n_clusters * per
    cx, cy = rng.integers(spread, w - spread, n_clusters), rng.integers(spread, h - spread, n_clusters)
    x = np.repeat(cx, per) + rng.integers(-spread, spread + 1, n)
    y = np.repeat(cy, per) + rng.integers(-spread, spread + 1, n)
    return keys_of(x, y, rng.integers(0, 256, n))


def distinct(seed, n, w, h):
    """n keys on n different pixels."""
    rng = np.random.default_rng(seed)
    at = rng.choice(w * h, n, replace=False)
    return keys_of(at % w, at // w, rng.integers(0, 256, n))


def scene(keys, w, h, n_features):
    return keys, MIN_B, MIN_B + w, MIN_B, MIN_B + h, n_features


def _build():
    s = {}
    s["empty"] = scene(keys_of([], [], []), 200, 64, 40)
    s["one"] = scene(keys_of([17], [5], [80]), 200, 64, 40)
    s["coincident_two"] = scene(keys_of([44, 44], [9, 9], [10, 200]), 200, 64, 40)            # never separate: count == before
    s["one_root"] = scene(uniform(3, 80, 90, 100), 300, 100, 30)                              # three roots, all keys in the first
    s["n_ini_2p5"] = scene(uniform(4, 150, 250, 100), 250, 100, 60)                           # round(2.5) = 3 roots
    s["n_ini_under_1p5"] = scene(uniform(5, 150, 149, 100), 149, 100, 60)                     # round(1.49) = 1 root
    quirk_x = [327, 328, 329, 656, 657, 658]
    s["root_box_quirk"] = scene(keys_of(quirk_x * 2 + [5, 500, 900, 985], [3] * 6 + [300] * 6 + [100, 20, 250, 328],
                                        [50, 60, 70, 80, 90, 100] * 2 + [1, 2, 3, 4]), 986, 329, 12)
    for t in (1, 2, 3, 4):
        s["first_round_target_%d" % t] = scene(uniform(6, 50, 100, 100), 100, 100, t)
    lat_x, lat_y = np.meshgrid(8 + 16 * np.arange(8), 8 + 16 * np.arange(4))                  # a lattice every split divides evenly
    s["target_above_count"] = scene(keys_of(lat_x.ravel(), lat_y.ravel(), (np.arange(32) * 11) % 256), 128, 64, 500)    # every key its own leaf
    s["close_phase_mid_pass"] = scene(uniform(0, 120, 200, 64), 200, 64, 40)                  # stops at place 9 of 12
    s["close_phase_tie"] = s["close_phase_mid_pass"]                                          # equal sizes in grown, the rule matters
    s["close_phase_three_passes"] = scene(clustered(0, 10, 12, 2, 400, 130), 400, 130, 45)
    dense_x, dense_y = np.meshgrid(np.arange(33), np.arange(37))                              # every pixel of the region, every third twice
    dx, dy = np.concatenate([dense_x.ravel(), dense_x.ravel()[::3]]), np.concatenate([dense_y.ravel(), dense_y.ravel()[::3]])
    s["odd_extents_one_pixel_cells"] = scene(keys_of(dx, dy, (np.arange(len(dx)) * 37) % 256), 33, 37, 2000)
    s["response_ties"] = scene(uniform(8, 200, 160, 64, response_below=2), 160, 64, 12)       # the smallest index wins
    for n in (63, 64, 65, 255, 256, 257):
        s["count_%d" % n] = scene(uniform(100 + n, n, 300, 100), 300, 100, max(n // 3, 8))
    for n in (LDS_CANDIDATES, LDS_CANDIDATES + 1):                                            # the last set whose candidates stay in LDS, the first in scratch
        s["count_%d" % n] = scene(uniform(100 + n, n, 1000, 320), 1000, 320, 434)
    s["larger_than_workgroup"] = scene(uniform(9, 6000, 1000, 320), 1000, 320, 434)
    s["many_cells"] = scene(distinct(10, 3000, 1000, 320), 1000, 320, MAX_CELLS - 3)          # the table filled to its last cells
    return s


SCENES = _build()
BATCH = ["count_65", "close_phase_three_passes", "one", "larger_than_workgroup", "empty", "root_box_quirk", "count_257", "coincident_two"]
assert len(BATCH) == 8 and BATCH[4] == "empty"


def words_of(keys):
    return (keys["x"].astype(np.uint32) | (keys["y"].astype(np.uint32) << 12) | (keys["response"].astype(np.uint32) << 24)).astype("<u4")


def blob_of(names):
    parts = [struct.pack("<i", len(names))]
    for name in names:
        keys, x0, x1, y0, y1, target = SCENES[name]
        parts += [struct.pack("<iiii", len(keys), x1 - x0, y1 - y0, target), words_of(keys).tobytes()]
    return b"".join(parts)


def run_prog(exe, tmp_path, names):
    """The stand-alone walk over the named scenes: per scene (status, kept keys, rounds, passes, stop)."""
    raw = host_prog.run(exe, tmp_path, "run", blob_of(names))
    out, at = [], 0
    for name in names:
        status, count, rounds, passes, stop = struct.unpack_from("<5i", raw, at); at += 20
        words = np.frombuffer(raw, "<u4", count, at); at += 4 * count
        index = np.frombuffer(raw, "<i4", count, at); at += 4 * count
        keys = SCENES[name][0]
        assert np.array_equal(words, words_of(keys)[index])
        out.append((status, keys[index].copy(), rounds, passes, stop))
    assert at == len(raw)
    return out
