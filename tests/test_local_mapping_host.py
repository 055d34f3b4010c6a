"""Triangulation and map-point refresh without a device: the kernels' arithmetic (triangulate_math.hpp, mappoint_math.hpp) compiled for
the host against the numpy restatements, bit for bit; the two unpinned pieces of the triangulation against a float64 evaluation; the
descriptor rule against a literal transcription; header, exports, ctypes layout and argument checks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import host_prog
import mappoint_restatement as MR
import triangulate_restatement as TR

ROOT = host_prog.ROOT
API = os.path.join(ROOT, "sivo_amd", "api")
F, D = np.float32, np.float64


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic, compiled for the host
# ---------------------------------------------------------------------------------------------------------------------
def run_tri(exe, tmp_path, p):
    m = np.ascontiguousarray(p["matches"], TR.MATCH_DTYPE)
    blob = b"".join([np.asarray(p["kf1"], TR.KEYFRAME_DTYPE).tobytes(), np.asarray(p["kf2"], TR.KEYFRAME_DTYPE).tobytes(),
                     np.array([p["ratio_factor"], 0], F).tobytes(), np.asarray(p["state_cov"], D).tobytes(),
                     np.array([p["th_confidence"], p["th_entropy"]], D).tobytes(), np.array([m.shape[0]], np.int64).tobytes(), m.tobytes()])
    raw, n = host_prog.run(exe, tmp_path, "tri", blob, timeout=120), m.shape[0]
    assert len(raw) == 14 * n
    return {"status": np.frombuffer(raw, np.uint8, n), "detected_class": np.frombuffer(raw, np.uint8, n, n),
            "wP": np.frombuffer(raw, F, 3 * n, 2 * n).reshape(n, 3)}


def run_refresh(exe, tmp_path, s):
    n = len(s["pos"])
    rec = np.concatenate([s["pos"], s["ref_ow"], s["level_scale"][:, None], s["last_scale"][:, None]], axis=1).astype(F)
    blob = b"".join([np.array([n], np.int64).tobytes(), np.asarray(s["desc_off"], np.int64).tobytes(), np.asarray(s["obs_off"], np.int64).tobytes(),
                     np.ascontiguousarray(s["desc"], np.uint8).tobytes(), np.ascontiguousarray(s["obs_ow"], F).tobytes(), rec.tobytes()])
    raw = host_prog.run(exe, tmp_path, "refresh", blob, timeout=120)
    assert len(raw) == 25 * n
    geom = np.frombuffer(raw, F, 5 * n, 4 * n).reshape(n, 5)
    best = np.frombuffer(raw, np.int32, n).copy()
    best[best < 0] = 0
    return {"best_idx": best, "max_dist": geom[:, 0], "min_dist": geom[:, 1], "normal": geom[:, 2:], "flags": np.frombuffer(raw, np.uint8, n, 24 * n)}


def nan_problem():
    """Keyframe 2's translation holds a NaN: every triangulated point is NaN and falls through every `>` test."""
    p = TR.make_problem(21, 40, min_margin=0, stereo=(0.0, 0.0))
    k2 = np.array(p["kf2"])
    k2["tcw"][0] = np.nan
    p["kf2"] = k2
    return p


def tri_problems():
    return [TR.make_problem(1, 300, min_margin=0), TR.all_status_problem(), nan_problem(),
            TR.make_problem(2, 120, min_margin=0, stereo=(1.0, 1.0), mbf2=300.0), TR.make_problem(3, 120, min_margin=0, stereo=(0.0, 1.0)),
            TR.make_problem(4, 64, min_margin=0, stereo=(0.0, 0.0), nlevels=3)]


REFRESH_SIZES = [1, 2, 63, 64, 65, 0, 200, 3, 7, 30]


def refresh_sets():
    return [MR.make_points(1, REFRESH_SIZES, bad=0.15), MR.make_points(2, [5, 9, 12, 2, 31] * 4, ties=True),
            MR.make_points(3, [4, 17, 1], identical=True), MR.make_points(4, [3, 3], bad=1.0)]


def check_host(exe, tmp_path):
    seen, nans = set(), 0
    for p in tri_problems():
        got, want = run_tri(exe, tmp_path, p), TR.triangulate(p)
        for k in ("status", "detected_class", "wP"):
            assert got[k].tobytes() == want[k].tobytes(), k
        seen |= set(want["status"].tolist())
        nans += int(np.isnan(want["wP"]).any(axis=1).sum())
        assert (want["wP"].view(np.uint32)[np.isnan(want["wP"])] == 0x7FC00000).all()
    assert seen == set(range(10)) and nans > 0
    flags = 0
    for s in refresh_sets():
        got, want = run_refresh(exe, tmp_path, s), MR.refresh(**s)
        for k in ("best_idx", "max_dist", "min_dist", "normal", "flags"):
            assert got[k].tobytes() == want[k].tobytes(), k
        flags |= int(np.bitwise_or.reduce(want["flags"]))
    assert flags == 3                 # a point without observations and one with observations of bad keyframes only


def test_host_build_of_the_kernel_arithmetic_equals_the_restatement(tmp_path):
    check_host(host_prog.build("local_mapping_prog", tmp_path), tmp_path)


def test_host_build_under_address_and_undefined_sanitizers(tmp_path):
    """The same stand-alone program built with -fsanitize=address,undefined and run directly: no finding, the same bytes."""
    if not host_prog.sanitizer_runtime_present(tmp_path):
        pytest.skip("the sanitizer runtime (libasan / libubsan) is not installed: a trivial main does not link with -fsanitize")
    check_host(host_prog.build("local_mapping_prog", tmp_path, sanitize=True), tmp_path)


def test_the_sweep_count_is_read_from_the_source():
    assert TR.sweeps() >= 4
    p = TR.make_problem(5, 60, min_margin=0, stereo=(0.0, 0.0))
    A = TR.matrix_A(p["kf1"], p["kf2"], p["matches"])
    assert TR.null_vector(A).tobytes() == TR.null_vector(A, TR.sweeps() + 2).tobytes()      # converged: two more sweeps change no bit
    assert TR.null_vector(A).tobytes() != TR.null_vector(A, 1).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# the unpinned pieces against float64
# ---------------------------------------------------------------------------------------------------------------------
def test_the_cosine_is_within_one_ulp_of_the_float64_value():
    """(d^2 - a^2) / (d^2 + a^2) in double, rounded to float, against the float rounding of np.cos(2 * np.arctan2(a, d)): both are
    roundings of reals that agree to double precision, so they differ by one float ulp at the most."""
    rng = np.random.default_rng(0)
    depth = np.concatenate([rng.uniform(0.05, 200, 20000), 10.0 ** rng.uniform(-3, 4, 5000)]).astype(F)
    worst = 0.0
    for mb in (0.1, 0.5371, 1.0):
        got = TR._cos_stereo(F(mb), depth)
        want = np.cos(2 * np.arctan2(D(F(mb)) / 2, depth.astype(D))).astype(F)
        ulp = np.spacing(np.abs(want)).astype(D)
        worst = max(worst, float((np.abs(got.astype(D) - want.astype(D)) / ulp).max()))
    print("cosine: worst difference in float ulps", worst)
    assert worst <= 1.0


SCENES_64 = [dict(seed=31, n=150), dict(seed=32, n=150, stereo=(0.0, 0.0)), dict(seed=33, n=150, stereo=(1.0, 0.3), mbf2=300.0),
             dict(seed=34, n=150, stereo=(0.0, 1.0), noise=1.0)]


@pytest.fixture(scope="module")
def scenes64():
    out = []
    for kw in SCENES_64:
        p = TR.make_problem(**kw)
        out.append((p, TR.pipeline64(p), TR.triangulate(p), TR.triangulate(p, null=lambda A: TR.null_svd(A, F).astype(F))))
    return out


def test_null_vector_error_against_float64_is_at_the_level_of_a_float32_svd(scenes64):
    """Relative wP error of the restated null vector (Jacobi on A'A in double, rounded to float) and of numpy's float32 SVD (the nearest
    stand-in here for OpenCV's float Jacobi) against the float64 SVD of the same float A, over the triangulated matches."""
    worst = {"restatement": 0.0, "float32_svd": 0.0}
    count = 0
    for p, ref, ours, f32 in scenes64:
        A = TR.matrix_A(p["kf1"], p["kf2"], p["matches"])
        e64 = TR.null_svd(A, D)
        tri = ours["triangulated"]
        w64 = e64[tri, :3] / e64[tri, 3:4]
        for name, e in (("restatement", TR.null_vector(A)), ("float32_svd", TR.null_svd(A, F))):
            e = e.astype(F)
            w = (e[tri, :3] * (1.0 / e[tri, 3:4].astype(D)).astype(F)).astype(D)
            worst[name] = max(worst[name], float((np.linalg.norm(w - w64, axis=1) / np.linalg.norm(w64, axis=1)).max()))
        count += int(tri.sum())
    print("null vector: max relative wP error against float64 over", count, "points:", worst)
    # (numpy.linalg computes a float32 SVD in double and rounds: DESIGN 3.6e sets a decomposition that runs in single precision beside it)
    assert count > 100
    assert worst["restatement"] <= 2 * worst["float32_svd"]


def test_statuses_agree_with_the_float64_pipeline(scenes64):
    """No match of these scenes lies within a relative 1e-3 of a threshold in float64 (such draws were replaced): the restatement, and
    the float32-SVD stand-in, take every decision as the float64 pipeline does."""
    seen = set()
    for p, ref, ours, f32 in scenes64:
        assert ref["margin"].min() >= 1e-3
        assert np.array_equal(ours["status"], ref["status"])
        assert np.array_equal(f32["status"], ref["status"])
        seen |= set(ref["status"].tolist())
    assert {TR.ACCEPTED, TR.Z1, TR.REPROJ1, TR.REPROJ2, TR.SCALE, TR.SEMANTICS} <= seen


# ---------------------------------------------------------------------------------------------------------------------
# the descriptor rule
# ---------------------------------------------------------------------------------------------------------------------
def test_rank_selection_equals_the_sort_and_index_rule():
    rng = np.random.default_rng(9)
    tied = 0
    for trial in range(120):
        N = int(rng.integers(1, 40))
        s = MR.make_points(100 + trial, [N], ties=trial % 2 == 0, identical=trial % 17 == 0)
        d = s["desc"]
        assert MR.best_index(d) == MR.best_index_literal(d)
        med = MR.row_medians(d)
        assert med.tolist() == [sorted(r)[int(0.5 * (N - 1))] for r in MR.hamming_matrix(d).tolist()]
        tied += int((med == med.min()).sum() > 1)
    assert tied > 20                                        # planted ties between the medians


def test_one_and_two_descriptors_choose_the_first():
    for N in (1, 2):
        d = np.random.default_rng(N).integers(0, 256, (N, 32), dtype=np.uint8)
        assert MR.best_index(d) == MR.best_index_literal(d) == 0           # N = 2: both medians are element 0 of the sorted row, 0


# ---------------------------------------------------------------------------------------------------------------------
# header, exports, argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    h = open(os.path.join(ROOT, "include", "sivo_hip.h")).read()
    assert "int sivo_triangulate(SivoTriProblem *problem);" in h
    assert "int sivo_triangulate_batch(SivoTriProblem *problems, int n_problems);" in h
    assert "int sivo_mappoint_refresh(int np, const int64_t *desc_off," in h
    assert "LocalMapping.cc:277-470" in h and "MapPoint.cc:284-347" in h         # every entry point cites the lines it replaces
    from sivo_amd import _lib, local_mapping
    L = _lib.lib()
    assert all(hasattr(L, n) for n in ("sivo_triangulate", "sivo_triangulate_batch", "sivo_mappoint_refresh"))
    assert local_mapping.MATCH_DTYPE.itemsize == C.sizeof(_lib.TriMatch) == 64
    assert local_mapping.KEYFRAME_DTYPE.itemsize == C.sizeof(_lib.TriKeyFrame) == 272
    assert len(local_mapping.STATUS) == 10


def test_ctypes_structs_and_dtypes_match_the_header(tmp_path):
    from sivo_amd import _lib, local_mapping
    for c, t in (("SivoTriKeyFrame", _lib.TriKeyFrame), ("SivoTriMatch", _lib.TriMatch), ("SivoTriProblem", _lib.TriProblem)):
        host_prog.c_layout(tmp_path, c, t)
    for dt, t in ((local_mapping.KEYFRAME_DTYPE, _lib.TriKeyFrame), (local_mapping.MATCH_DTYPE, _lib.TriMatch)):
        assert [dt.fields[f[0]][1] for f in t._fields_] == [getattr(t, f[0]).offset for f in t._fields_]


def test_entry_points_check_arguments_and_fail_loudly_without_a_device():
    from sivo_amd import _lib, local_mapping as LM
    p = TR.make_problem(6, 20, min_margin=0, nlevels=5)
    args = lambda q: (q["kf1"], q["kf2"], q["matches"], q["ratio_factor"], q["state_cov"], q["th_confidence"], q["th_entropy"])
    # invalid arguments are reported as such before any device is needed
    for field, value in (("octave1", 5), ("octave2", 5), ("octave1", -1), ("octave2", 16)):          # an octave >= nlevels, or negative
        m = p["matches"].copy()
        m[field][7] = value
        with pytest.raises(_lib.SivoInvalidArgument):
            LM.triangulate(*args(dict(p, matches=m)))
        with pytest.raises(_lib.SivoInvalidArgument):
            LM.triangulate_batch([p, dict(p, matches=m)])
    for nl in (0, 17):
        k = np.array(p["kf2"])
        k["nlevels"] = nl
        with pytest.raises(_lib.SivoInvalidArgument):
            LM.triangulate(*args(dict(p, kf2=k)))
    P = _lib.TriProblem()
    P.kf1.nlevels = P.kf2.nlevels = 8
    P.n = -1                                                                                     # n < 0
    assert _lib.lib().sivo_triangulate(C.byref(P)) == _lib.ERR_INVALID_ARGUMENT
    P.n = 5                                                                                      # a NULL array with n > 0
    assert _lib.lib().sivo_triangulate(C.byref(P)) == _lib.ERR_INVALID_ARGUMENT
    assert _lib.lib().sivo_triangulate(None) == _lib.ERR_INVALID_ARGUMENT
    assert _lib.lib().sivo_triangulate_batch(None, 2) == _lib.ERR_INVALID_ARGUMENT
    assert _lib.lib().sivo_triangulate_batch(None, -1) == _lib.ERR_INVALID_ARGUMENT
    s = MR.make_points(1, [3, 4, 2])
    for key in ("desc_off", "obs_off"):
        bad = dict(s)
        bad[key] = np.array([0, 3, 2, 9])                                                        # a CSR offset that decreases
        with pytest.raises(_lib.SivoInvalidArgument):
            LM.refresh_map_points(**bad)
        bad[key] = np.array([1, 3, 7, 9])                                                        # ... that does not start at 0
        with pytest.raises(_lib.SivoInvalidArgument):
            LM.refresh_map_points(**bad)
    L = _lib.lib()
    z = np.zeros(16, np.int64)
    assert L.sivo_mappoint_refresh(-1, *([None] * 13)) == _lib.ERR_INVALID_ARGUMENT               # np < 0
    assert L.sivo_mappoint_refresh(2, *([None] * 13)) == _lib.ERR_INVALID_ARGUMENT                # NULL arrays with np > 0
    off = np.array([0, 1, 2], np.int64)
    f = np.zeros(8, F)
    assert L.sivo_mappoint_refresh(2, off.ctypes.data, None, off.ctypes.data, f.ctypes.data, f.ctypes.data, f.ctypes.data, f.ctypes.data,
                                   f.ctypes.data, z.ctypes.data, f.ctypes.data, f.ctypes.data, f.ctypes.data, z.ctypes.data) == _lib.ERR_INVALID_ARGUMENT
    # nothing to do: no launch, no device needed
    assert LM.triangulate_batch([]) == []
    empty = LM.triangulate(*args(dict(p, matches=p["matches"][:0])))
    assert len(empty["status"]) == 0
    assert len(LM.refresh_map_points([0], np.zeros((0, 32), np.uint8), [0], np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), [], [])["flags"]) == 0
    if _lib.lib().sivo_device_count() >= 1:            # (a device is visible: the calls run; tests/test_gpu_local_mapping.py checks what they compute)
        assert len(LM.triangulate(*args(p))["status"]) == 20
        return
    for call in (lambda: LM.triangulate(*args(p)), lambda: LM.triangulate_batch([p, p]), lambda: LM.refresh_map_points(**s)):
        with pytest.raises(_lib.SivoError) as e:
            call()
        assert e.value.code == _lib.ERR_RUNTIME


# ---------------------------------------------------------------------------------------------------------------------
# SIVO::CreateNewMapPoints / TriangulateMatches / RefreshMapPoints
# ---------------------------------------------------------------------------------------------------------------------
SNIPPETS = {
    # LocalMapping.cc:198-472 as LocalMapping::Run calls it (:71-72)
    "create_new_map_points": r'''int f(LKeyFrame *mpCurrentKeyFrame, std::vector<LKeyFrame *> vpNeighKFs, LMap *mpMap, std::list<LMapPoint *> &mlpRecentAddedMapPoints, bool mbMonocular) {
    return SIVO::CreateNewMapPoints(mpCurrentKeyFrame, vpNeighKFs, mpMap, mbMonocular, mlpRecentAddedMapPoints, [] { return false; });
}
''',
    # the loops of :116-123 and :624-633
    "refresh_map_points": r'''void g(LKeyFrame *mpCurrentKeyFrame) {
    std::vector<LMapPoint *> vpMapPointMatches = mpCurrentKeyFrame->mvpMapPoints;
    SIVO::RefreshMapPoints(vpMapPointMatches);
}
''',
}


@pytest.mark.parametrize("snippet", list(SNIPPETS))
def test_adapter_instantiates_over_stand_in_types(tmp_path, snippet):
    tu = tmp_path / "use.cpp"
    tu.write_text('#include "local_mapping_standins.hpp"\n' + SNIPPETS[snippet])
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-I" + API, "-I" + os.path.join(ROOT, "tests"), str(tu)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


def adapter_prog(out_dir, defines=()):
    return host_prog.build("local_mapping_adapter_prog", out_dir, link_lib=("sivo_api", "sivo_hip"), defines=defines)


def tri_blob(p):
    m = np.ascontiguousarray(p["matches"], TR.MATCH_DTYPE)
    return b"".join([np.asarray(p["kf1"], TR.KEYFRAME_DTYPE).tobytes(), np.asarray(p["kf2"], TR.KEYFRAME_DTYPE).tobytes(),
                     np.array([p["ratio_factor"], 0], F).tobytes(), np.asarray(p["state_cov"], D).tobytes(),
                     np.array([p["th_confidence"], p["th_entropy"]], D).tobytes(), np.array([m.shape[0]], np.int64).tobytes(), m.tobytes()])


def adapter_problem(seed=81, n=200):
    """A problem whose keypoints truncate to distinct pixels in each keyframe (the stand-in semantic maps hold one value per pixel)."""
    p = TR.make_problem(seed, n, min_margin=0, stereo=(0.9, 0.5))
    m = p["matches"]
    _, i1 = np.unique(np.stack([m["y1"].astype(int), m["x1"].astype(int)]), axis=1, return_index=True)
    _, i2 = np.unique(np.stack([m["y2"].astype(int), m["x2"].astype(int)]), axis=1, return_index=True)
    p["matches"] = m[np.intersect1d(i1, i2)]
    assert len(p["matches"]) > n // 2
    return p


def test_adapter_gathers_the_records_of_the_reference_walk(tmp_path):
    """gather_matches over stand-in keyframes whose keys are the scene's keypoints (keyframe 2's in reverse order): the staged problem is
    the scene, byte for byte — keypoints, octaves, mvRight, mvDepth and the four semantic lookups at the truncated positions."""
    p = adapter_problem()
    exe = adapter_prog(tmp_path)
    fout = tmp_path / "gather.out"
    host_prog.run(exe, tmp_path, "gather", tri_blob(p), timeout=60)                 # (writes fout)
    assert fout.read_bytes() == tri_blob(p)


# ---------------------------------------------------------------------------------------------------------------------
# the loop over the neighbours (LocalMapping.cc:230-259): a stand-in map with a skipped neighbour and two dependent ones
# ---------------------------------------------------------------------------------------------------------------------
KEY_DTYPE = np.dtype([("x", F), ("y", F), ("octave", np.int32), ("r", F), ("depth", F), ("cls", np.int32), ("entropy", D), ("confidence", D),
                      ("node", np.int32), ("pad", np.int32)])


def map_scene(seed=91, n=240):
    """The current keyframe and three neighbours.  Neighbour 0 stands where the current keyframe stands (baseline < mb: skipped, :243-244);
    neighbours 1 and 2 see the same points as the current keyframe (key i of the current keyframe matches key n - 1 - i of either, with a
    descriptor three bits away, in the same vocabulary node), so whatever neighbour 1 makes a point of is a slot neighbour 2's search must
    find occupied."""
    rng = np.random.default_rng(seed)
    k1, k2 = TR.make_keyframes(rng)
    _, k3 = TR.make_keyframes(np.random.default_rng(seed + 1))
    k3 = np.array(k3)
    k0 = np.array(k1)
    k0["fx"] = k1["fx"] * F(1.01)                     # (a neighbour of its own, at the current keyframe's pose)
    k0["invfx"] = F(1) / k0["fx"]
    m2 = TR.draw_matches(np.random.default_rng(seed + 2), k1, k2, n, stereo=(0.9, 0.5), outliers=0.1)
    m3 = TR.draw_matches(np.random.default_rng(seed + 2), k1, k3, n, stereo=(0.9, 0.5), outliers=0.1)
    for f in ("x1", "y1", "octave1", "r1", "depth1", "class1", "entropy1", "confidence1"):
        assert np.array_equal(m2[f], m3[f])            # one set of keys in the current keyframe
    d1 = rng.integers(0, 256, (n, 32), dtype=np.uint8)

    def keys(x, y, o, r, depth, cls, ent, conf, order):
        k = np.zeros(n, KEY_DTYPE)
        k["x"], k["y"], k["octave"], k["r"], k["depth"], k["cls"], k["entropy"], k["confidence"] = x, y, o, r, depth, cls, ent, conf
        k["node"] = np.arange(n) % 17
        return k[order]

    fwd, rev = np.arange(n), np.arange(n)[::-1]
    cur = keys(m2["x1"], m2["y1"], m2["octave1"], m2["r1"], m2["depth1"], m2["class1"], m2["entropy1"], m2["confidence1"], fwd)
    frames = [(np.array(k1), cur, d1)]
    for kf, m, salt in ((k0, m2, 5), (np.array(k2), m2, 6), (k3, m3, 7)):
        flips = np.zeros((n, 32), np.uint8)
        flips[np.arange(n), (np.arange(n) * salt) % 32] = 0x0b
        # (neighbour 1 sees another class at every second point: those stay free for neighbour 2)
        cls = np.where((np.arange(n) % 2 == 0) & (salt == 6), (m["class1"].astype(int) + 1) % 9, m["class2"])
        frames.append((kf, keys(m["x2"], m["y2"], m["octave2"], m["r2"], m["depth2"], cls, 0.0, 0.0, rev), (d1 ^ flips)[rev]))
    # one value per pixel in the stand-in semantic maps: keys that share a truncated position share their values
    for _, k, _ in frames:
        seen = {}
        for i in range(n):
            px = (int(k["y"][i]), int(k["x"][i]))
            j = seen.setdefault(px, i)
            for f in ("cls", "entropy", "confidence"):
                k[f][i] = k[f][j]
    cov = rng.normal(size=(6, 6)) * 0.1
    sc = {"frames": frames, "state_cov": 1e-4 * (np.eye(6) + cov @ cov.T), "th_confidence": 0.6, "th_entropy": 0.0}
    p = {"kf1": k1, "kf2": k2, "matches": m2, "ratio_factor": F(1.5) * F(1.2), "state_cov": sc["state_cov"], "th_confidence": 0.6, "th_entropy": 0.0}
    r = TR.triangulate(p)
    mis = r["mi"][r["reached"] & np.isfinite(r["mi"])]
    sc["th_entropy"] = float(np.median(mis)) - 0.8
    return sc


def map_blob(sc, checks):
    out = [np.array([len(sc["frames"]) - 1, checks], np.int64).tobytes(), np.asarray(sc["state_cov"], D).tobytes(),
           np.array([sc["th_confidence"], sc["th_entropy"]], D).tobytes()]
    for kf, keys, desc in sc["frames"]:
        out += [np.asarray(kf, TR.KEYFRAME_DTYPE).tobytes(), np.array([len(keys)], np.int64).tobytes(), keys.tobytes(), np.ascontiguousarray(desc).tobytes()]
    return b"".join(out)


def _gemm(A, B, alpha=1.0, C=None, tA=False, tB=False):
    """cv::gemm on CV_32F as api/compat/cv_min.hpp states it."""
    A, B = np.asarray(A, F), np.asarray(B, F)
    a, b = (A.T if tA else A), (B.T if tB else B)
    M, K, N = a.shape[0], a.shape[1], b.shape[1]
    small = not tA and not tB and 2 <= K <= 4 and (K == N or K == M)
    out = np.zeros((M, N), F)
    for i in range(M):
        for j in range(N):
            c = 0.0 if C is None else float(D(C[i, j]) * 1.0)
            if small:
                t = a[i, 0] * b[0, j]
                for k in range(1, K):
                    t = t + a[i, k] * b[k, j]
                out[i, j] = F(D(t) * alpha + c)
            else:
                s = D(0)
                for k in range(K):
                    s = s + D(a[i, k]) * D(b[k, j])
                out[i, j] = F(alpha * s + c)
    return out


def _inv3(S):
    """cv::invert of a 3 x 3 CV_32F matrix: determinant and cofactors in double, times 1 / det, stored as float."""
    s = np.asarray(S, F).astype(D)
    d = s[0, 0] * (s[1, 1] * s[2, 2] - s[1, 2] * s[2, 1]) - s[0, 1] * (s[1, 0] * s[2, 2] - s[1, 2] * s[2, 0]) + s[0, 2] * (s[1, 0] * s[2, 1] - s[1, 1] * s[2, 0])
    d = 1.0 / d
    return np.array([[(s[1, 1] * s[2, 2] - s[1, 2] * s[2, 1]) * d, (s[0, 2] * s[2, 1] - s[0, 1] * s[2, 2]) * d, (s[0, 1] * s[1, 2] - s[0, 2] * s[1, 1]) * d],
                     [(s[1, 2] * s[2, 0] - s[1, 0] * s[2, 2]) * d, (s[0, 0] * s[2, 2] - s[0, 2] * s[2, 0]) * d, (s[0, 2] * s[1, 0] - s[0, 0] * s[1, 2]) * d],
                     [(s[1, 0] * s[2, 1] - s[1, 1] * s[2, 0]) * d, (s[0, 1] * s[2, 0] - s[0, 0] * s[2, 1]) * d, (s[0, 0] * s[1, 1] - s[0, 1] * s[1, 0]) * d]]).astype(F)


def compute_f12(k1, k2):
    """LocalMapping::ComputeF12 (LocalMapping.cc:639-654), every product one cv::gemm."""
    K = lambda k: np.array([[k["fx"], 0, k["cx"]], [0, k["fy"], k["cy"]], [0, 0, 1]], F)
    R1, t1 = np.asarray(k1["Rcw"], F).reshape(3, 3), np.asarray(k1["tcw"], F).reshape(3, 1)
    R2, t2 = np.asarray(k2["Rcw"], F).reshape(3, 3), np.asarray(k2["tcw"], F).reshape(3, 1)
    R12 = _gemm(R1, R2, tB=True)
    t12 = _gemm(_gemm(R1, R2, alpha=-1.0, tB=True), t2, C=t1)[:, 0]
    t12x = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]], F)
    return _gemm(_gemm(_gemm(_inv3(K(k1).T.copy()), t12x), R12), _inv3(K(k2)))


def skipped(k1, k2):
    """:238-244: baseline < pKF2->mb."""
    v = np.asarray(k2["Ow"], F) - np.asarray(k1["Ow"], F)
    s = D(0)
    for i in range(3):
        s = s + D(v[i]) * D(v[i])
    return F(np.sqrt(s)) < F(k2["mb"])


@pytest.mark.parametrize("checks", [5, 1])
def test_adapter_walks_the_neighbours_as_the_reference_does(tmp_path, checks):
    """walk_neighbours (the loop CreateNewMapPoints runs) with a stand-in search and a stand-in triangulation, against a line-by-line walk
    of :230-259, :471 in Python: neighbour 0 is skipped for its baseline, the pairs neighbour 2's search is given depend on the points
    neighbour 1 made, checkNewKeyFrames() ends the loop (checks = 1: before the last neighbour), and F12 is ComputeF12's, bit for bit."""
    sc = map_scene()
    exe = adapter_prog(tmp_path)
    fout = tmp_path / "walk.out"
    host_prog.run(exe, tmp_path, "walk", map_blob(sc, checks), timeout=60)          # (writes fout)
    # the literal walk
    frames = sc["frames"]
    n = len(frames[0][1])
    occ = [np.zeros(len(f[1]), bool) for f in frames]
    want, calls, searched = [], 0, []
    for i in range(3):
        if i > 0:
            calls += 1
            if calls > checks:
                break
        if skipped(frames[0][0], frames[i + 1][0]):
            continue
        pairs = [j for j in range(n) if not occ[0][j] and not occ[i + 1][j] and j % (i + 2) == 0]
        new = [j for j in pairs if j % 3 == 0]
        occ[0][new] = True
        occ[i + 1][new] = True
        searched.append(i)
        want.append(np.array([i], np.int64).tobytes() + compute_f12(frames[0][0], frames[i + 1][0]).tobytes() + np.array([len(pairs)], np.int64).tobytes()
                    + np.array([[j, j] for j in pairs], np.int64).tobytes() + np.array([len(new)], np.int64).tobytes())
    assert searched == ([1, 2] if checks == 5 else [1])
    assert fout.read_bytes() == b"".join(want)
    if checks == 5:                   # the dependence: without neighbour 1's points, neighbour 2 would have been given more pairs
        assert len([j for j in range(n) if j % 4 == 0]) > np.frombuffer(want[1], np.int64, 1, 8 + 36)[0] > 0
