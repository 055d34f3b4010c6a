"""Triangulation of new map points and the map-point refresh pinned against the reference's OWN src/orbslam/LocalMapping.cc and MapPoint.cc.

oracle/Makefile compiles the two sources untouched, with their own headers and the reference's sivo_helpers, over data holders for the
rest of the SLAM graph (oracle/ref_shims_localmapping) and links them with oracle/ref_localmapping_driver.cpp into
oracle/_ref/ref_localmapping.  The kernels (triangulate_math.hpp, mappoint_math.hpp), their host build, the numpy restatements and the C++
adapter were written from one reading of those sources and are tested against each other bit for bit; this file holds each of them
against what the sources themselves compute, byte for byte:
  * CreateNewMapPoints() over one scripted neighbour: which matches become map points, mWorldPos, and mDescriptor / mNormalVector /
    mfMinDistance / mfMaxDistance after the two refresh calls the reference makes; CheckSemantics called directly on both keyframes;
    the F12 handed to SearchForTriangulation.  A rejected match's reason is not observable in an untouched source: the accepted set on
    all_status (with one twin per `continue`, moved just across that threshold) and on the min_margin = 0 scenes stands for it;
  * ComputeDistinctiveDescriptors() and UpdateNormalAndDepth() on points built from the CSR scenes, also with the keyframes allocated in
    descending address order (std::map<KeyFrame *, size_t> then walks the observations backwards) and with bad points;
  * CreateNewMapPoints() over the three-neighbour map of tests/test_local_mapping_host.py: which neighbours are searched, F12 per
    neighbour, the pairs handed over and the points made, also monocular and with a keyframe arriving in the queue;
  * SearchInNeighbors() on a small stand-in graph: the target list, the fuse candidates, the points refreshed afterwards;
  * cos(2 * atan2(mb / 2, depth)) of LocalMapping.cc:308 through the overload g++ picks and glibc's libm, against the rational form.
Still substitutions: cv::SVD::compute and cv::Mat::inv (oracle/cv_primitives.cpp, compared here with the restatements'
routines byte for byte), KeyFrame::UnprojectStereo, the scripted SearchForTriangulation.
Where the reference is absent the same assertions read tests/golden/local_mapping_reference.npz; the tests marked gpu read only that file."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import host_prog as hp                   # (host_prog is a fixture's name below)
import local_mapping_pin_cases as P
import mappoint_restatement as MR
import solver_pin_cases as S
import test_gpu_local_mapping as G
import test_local_mapping_host as H
import triangulate_restatement as TR

F, D = np.float32, np.float64
ENTRIES = ["tri." + n for n in P.TRI_NAMES] + ["refresh." + n for n in P.REFRESH_NAMES] + ["walk." + n for n in P.WALK_NAMES] + ["neighbors." + n for n in P.NEIGHBOR_NAMES] + ["cos"]


def test_with_the_reference_present_the_live_comparison_runs():
    _, live = P.reference_facts("tri.one")
    assert live or not S.reference_present(), "the reference is here: the live comparison must run"
    assert sorted(P.load_fixture()) == sorted(ENTRIES)


def test_fixture_is_what_the_reference_computes(tmp_path):
    """The committed fixture, byte for byte, from a fresh run of the reference program; its size; the digests of the scenes' inputs."""
    assert os.path.getsize(P.GOLDEN) < 256 * 1024
    for e in ENTRIES:
        P.recorded_facts(e)                                             # (asserts the digest of the scene's inputs)
    if P.reference_program():
        import importlib.util
        spec = importlib.util.spec_from_file_location("make_local_mapping_reference", os.path.join(ROOT, "tests", "golden", "make_local_mapping_reference.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        assert open(mod.write(str(tmp_path)), "rb").read() == open(P.GOLDEN, "rb").read()


# ---------------------------------------------------------------------------------------------------------------------
# the restatements
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", P.TRI_NAMES)
def test_triangulation_restatement_equals_the_reference(name):
    want, _ = P.reference_facts("tri." + name)
    r = P.tri_restated(name)
    P.same_facts(want, P.tri_as_facts(r), name)
    P.check_detected_class(want, r["status"], r["detected_class"], name)       # tr_match's own class, not only the copy of its rule in P
    if name == "mbf_differs":
        assert int(r["accepted"].sum()) > 5 and P.tri_scene(name)["kf1"]["mbf"] != P.tri_scene(name)["kf2"]["mbf"]
    if name == "stereo_2_only":                                          # the `else if` of :310 is taken by every match
        m = P.tri_scene(name)["matches"]
        assert (m["r1"] < 0).all() and (m["r2"] >= 0).all()


def test_the_reference_accepts_exactly_the_twins_of_all_status():
    """all_status holds every `continue` of the loop; behind it one twin per `continue`: a match with that status moved across the
    threshold.  The reference makes a point of every twin, and of those of the originals the restatement accepts, and of nothing else."""
    p, n0, of = P.all_status_with_twins()
    assert sorted(of) == list(range(1, 10))
    want, _ = P.reference_facts("tri.all_status")
    st = P.tri_restated("all_status")["status"]
    assert set(st[:n0].tolist()) == set(range(10))
    assert want["accepted"][n0:].tolist() == [1] * len(of)
    assert want["accepted"][:n0].tolist() == (st[:n0] == TR.ACCEPTED).astype(int).tolist()


@pytest.mark.parametrize("name", P.REFRESH_NAMES)
def test_refresh_restatement_equals_the_reference(name):
    want, _ = P.reference_facts("refresh." + name)
    got = P.refresh_expected(name, MR.refresh(**P.walked(name)))
    P.same_facts(want, got, name)
    t = got["touched"]
    if name == "mixed_with_empty":
        assert t[5].tolist() == [0, 0] and t[4].tolist() == [1, 1]      # a point nobody observes stays as it was
    if name == "bad_keyframes_only":
        assert t.tolist() == [[0, 1], [0, 1]]                           # no descriptor to choose from; normal and range all the same
    if name == "mixed_with_empty_bad_points":
        assert not t[::3].any() and t[1].all()
    if name == "mixed_with_empty_reversed":                             # the walk order matters: the forward scene gives other bytes
        fwd = P.refresh_expected("mixed_with_empty", MR.refresh(**P.walked("mixed_with_empty")))
        assert fwd["desc"].tobytes() != got["desc"].tobytes() and fwd["geom"].tobytes() != got["geom"].tobytes()
    if name == "even_sizes":                                            # the median index: element N / 2 would choose another descriptor
        w, other = P.walked(name), 0
        for a, b in zip(w["desc_off"][:-1], w["desc_off"][1:]):
            rows = np.sort(MR.hamming_matrix(w["desc"][a:b]), axis=1)
            other += int(np.argmin(rows[:, (b - a) // 2]) != np.argmin(rows[:, int(0.5 * (b - a - 1))]))
        assert other > 10
    if name == "strided":
        assert int(np.diff(P.walked(name)["desc_off"]).max()) == 200     # the largest N: float Distances[N][N] is on the reference's stack


@pytest.mark.parametrize("name", P.WALK_NAMES)
def test_walk_over_the_neighbours_equals_the_reference(name):
    """CreateNewMapPoints() over the three-neighbour map: which neighbours are searched (the baseline skip, the monocular skip through
    ComputeSceneMedianDepth, CheckNewKeyFrames() turning true after a search), the F12 each search is handed, the pairs (which depend on
    the slots earlier neighbours' points took) and the points made, against the line-by-line walk with tr_match's restatement."""
    want, _ = P.reference_facts("walk." + name)
    got = P.walk_as_facts(P.walk_restated(name))
    P.same_facts(want, got, name)
    assert got["neighbours"].tolist() == {"all": [1, 2], "keyframe_arrives": [1], "monocular": [2]}[name]
    assert (got["point_counts"] > 3).all()
    if name == "all":
        assert P.walk_blocked("all") > 0 and P.walk_blocked("monocular") == 0      # neighbour 2's search lost slots to neighbour 1's points


@pytest.mark.parametrize("name", P.NEIGHBOR_NAMES)
def test_search_in_neighbors_equals_the_line_by_line_walk(name):
    """SearchInNeighbors() on a small graph: the target list (bad and already marked keyframes skipped, five second neighbours each, a
    second neighbour is NOT marked and so can enter twice; 10 first neighbours, 20 when monocular), the fuse candidates, and the points of
    the current keyframe refreshed afterwards (null and bad ones skipped, as SIVO::RefreshMapPoints skips them)."""
    want, _ = P.reference_facts("neighbors." + name)
    got = P.neighbors_restated(name)
    P.same_facts(want, got, name)
    t = got["targets"].tolist()
    assert t[:7] == [1, 6, 7, 4, 6, 8, 5] and 2 not in t and 3 not in t and 0 not in t and (t[-1] == 8) == (name == "monocular")
    assert got["candidates"].tolist() == [3, 0, 5, 7, 2] and got["refreshed"].tolist() == [0, 2]


# ---------------------------------------------------------------------------------------------------------------------
# the host build of the kernels' arithmetic
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_prog(tmp_path_factory):
    return hp.build("local_mapping_prog", tmp_path_factory.mktemp("local_mapping_prog"))


def test_host_build_equals_the_reference(host_prog, tmp_path):
    reached = 0
    for name in P.TRI_NAMES:
        got = H.run_tri(host_prog, tmp_path, P.tri_scene(name))
        P.same_facts(P.reference_facts("tri." + name)[0], P.tri_from(name, got["status"], got["wP"], lambda **s: H.run_refresh(host_prog, tmp_path, s)), name)
        reached += P.check_detected_class(P.reference_facts("tri." + name)[0], got["status"], got["detected_class"], name)
    assert reached > 500
    for name in P.REFRESH_NAMES:
        got = P.refresh_expected(name, H.run_refresh(host_prog, tmp_path, P.walked(name)))
        P.same_facts(P.reference_facts("refresh." + name)[0], got, name)


# ---------------------------------------------------------------------------------------------------------------------
# the two primitives under LocalMapping.cc
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prim():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "libcvprim.so"], check=True)
    return C.CDLL(os.path.join(ROOT, "oracle", "libcvprim.so"))


def test_null_vector_primitive_equals_the_restatements_routine(prim):
    assert prim.cvp_sweeps_tri() == TR.sweeps()
    fp = C.POINTER(C.c_float)
    count = 0
    for name in ("stereo_none", "all_status", "nan", "batch_2"):
        p = P.tri_scene(name)
        A = np.ascontiguousarray(TR.matrix_A(p["kf1"], p["kf2"], p["matches"]), F)
        with np.errstate(all="ignore"):
            want = TR.null_vector(A).astype(F)
        for i in range(len(A)):
            e = np.zeros(4, F)
            prim.cvp_null4(A[i].ctypes.data_as(fp), e.ctypes.data_as(fp))
            assert P.canon(e).tobytes() == P.canon(want[i]).tobytes(), (name, i)
            count += 1
    assert count > 500


def test_inverse_primitive_equals_the_restatements_routine(prim):
    fp = C.POINTER(C.c_float)
    rng = np.random.default_rng(5)
    mats = [rng.normal(size=(3, 3)).astype(F) for _ in range(50)]
    for name in ("one", "batch_2"):
        k = P.tri_scene(name)["kf1"]
        K = np.array([[k["fx"], 0, k["cx"]], [0, k["fy"], k["cy"]], [0, 0, 1]], F)
        mats += [K, K.T.copy()]
    for S3 in mats:
        got = np.zeros((3, 3), F)
        prim.cvp_inv3f(np.ascontiguousarray(S3).ctypes.data_as(fp), got.ctypes.data_as(fp))
        assert got.tobytes() == H._inv3(S3).tobytes()
    got = np.ones((3, 3), F)
    prim.cvp_inv3f(np.zeros((3, 3), F).ctypes.data_as(fp), got.ctypes.data_as(fp))
    assert not got.any()                                                  # a zero determinant: the zero matrix


# ---------------------------------------------------------------------------------------------------------------------
# cos(2 * atan2(mb / 2, depth))
# ---------------------------------------------------------------------------------------------------------------------
def test_the_cosine_of_the_reference_line_and_the_rational_form():
    """LocalMapping.cc:308 under g++ here: cos(2 * atan2(float, float)) takes the float overloads (sizeof 4: cosf(2 * atan2f(a, d))).  Over
    the 75 000 depths of tests/test_local_mapping_host.py the rational form of the restatement is never further from the float64 value
    than that libm path, and stays within one float ulp; that no DECISION of any scene differs is what the byte-for-byte tests above show
    (every scene's accepted set is the reference's, which went through libm)."""
    want, _ = P.reference_facts("cos")
    assert want["sizeof"].tolist() == [4]
    v = P.cosine_inputs()
    ours = TR._cos_stereo(v[:, 0], v[:, 1])
    worst_ours = P.cosine_worst_ulps(ours)
    if "cos" in want:                                                   # live: the libm values themselves
        worst_libm = P.cosine_worst_ulps(want["cos"][:, 0])
        print("values that differ between the two paths:", int((want["cos"][:, 0] != ours).sum()), "of", len(ours))
    else:                                                               # the fixture holds them as a digest, and their largest error beside it
        worst_libm = float(want["libm_worst_ulps"][0])
    print("cosine, float ulps from the float64 value: rational form", worst_ours, ", libm path", worst_libm)
    assert worst_ours <= 1.0 and worst_ours <= worst_libm


# ---------------------------------------------------------------------------------------------------------------------
# the reference driver under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_driver_under_address_and_undefined_sanitizers():
    """oracle/_ref/ref_localmapping_san: the same stand-alone program built with -fsanitize=address,undefined, on every scene.
    LIVE ONLY: where neither the reference's sources nor a built oracle/_ref are at hand there is nothing to run and the test passes
    without having checked anything."""
    if not P.reference_program():
        return
    assert P.reference_program("ref_localmapping_san")
    for name in P.TRI_NAMES:
        P.same_facts(P.reference_facts("tri." + name)[0], P.tri_facts(name, "ref_localmapping_san"), name)
    for name in P.REFRESH_NAMES:
        P.same_facts(P.reference_facts("refresh." + name)[0], P.refresh_facts(name, "ref_localmapping_san"), name)
    for name in P.WALK_NAMES:
        P.same_facts(P.reference_facts("walk." + name)[0], P.walk_facts(name, "ref_localmapping_san"), name)
    for name in P.NEIGHBOR_NAMES:
        P.same_facts(P.reference_facts("neighbors." + name)[0], P.neighbors_facts(name, "ref_localmapping_san"), name)


# ---------------------------------------------------------------------------------------------------------------------
# the device: reads only tests/golden
# ---------------------------------------------------------------------------------------------------------------------
def device_tri(name, res, want):
    from sivo_amd import local_mapping as LM
    P.check_detected_class(want, res["status"], res["detected_class"], name)
    return P.tri_from(name, res["status"], res["wP"], lambda **s: LM.refresh_map_points(**s))


@pytest.mark.gpu
def test_device_triangulate_equals_the_recorded_reference():
    for name in P.TRI_NAMES:
        want = P.recorded_facts("tri." + name)
        P.same_facts(want, device_tri(name, G.run(P.tri_scene(name)), want), name)


@pytest.mark.gpu
def test_device_triangulate_batch_equals_the_recorded_reference():
    from sivo_amd import local_mapping as LM
    for name, res in zip(P.TRI_NAMES, LM.triangulate_batch([P.tri_scene(n) for n in P.TRI_NAMES])):
        want = P.recorded_facts("tri." + name)
        P.same_facts(want, device_tri(name, res, want), name)


@pytest.mark.gpu
def test_device_mappoint_refresh_equals_the_recorded_reference():
    from sivo_amd import local_mapping as LM
    for name in P.REFRESH_NAMES:
        P.same_facts(P.recorded_facts("refresh." + name), P.refresh_expected(name, LM.refresh_map_points(**P.walked(name))), name)


# ---------------------------------------------------------------------------------------------------------------------
# the C++ adapter (sivo_amd/api/orbslam/LocalMappingAdapter.h) through tests/local_mapping_adapter_prog.cpp: over the host build of the
# kernels' arithmetic (tests/local_mapping_host_capi.hpp) against the live or recorded reference, and on the device against the recorded one
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def adapter_prog(tmp_path_factory):
    return H.adapter_prog(tmp_path_factory.mktemp("local_mapping_adapter_prog"))


@pytest.fixture(scope="module")
def adapter_prog_host(tmp_path_factory):
    return H.adapter_prog(tmp_path_factory.mktemp("local_mapping_adapter_prog_host"), defines=("SIVO_LM_ON_HOST",))


run_adapter = functools.partial(hp.run, timeout=120)


def check_cpp_walk(exe, tmp_path, name, want):
    """SIVO::local_mapping_detail::walk_neighbours -- the loop SIVO::CreateNewMapPoints runs -- with the reference driver's scripted search
    and SIVO::TriangulateMatches: which neighbours are searched (baseline skip, the monocular skip through ComputeSceneMedianDepth,
    checkNewKeyFrames()), F12, the slots occupied at each search, the pairs, the points and their positions."""
    got = P.walk_as_facts(P.parse_walk(run_adapter(exe, tmp_path, "pinwalk", P.walk_blob(name))))
    P.same_facts(want, got, name)
    assert got["neighbours"].tolist() == {"all": [1, 2], "keyframe_arrives": [1], "monocular": [2]}[name]


def check_cpp_triangulate_matches(exe, tmp_path, name, want):
    """SIVO::TriangulateMatches (the loop of CreateNewMapPoints over ONE neighbour's matches) over stand-in SLAM types."""
    p = P.tri_scene(name)
    n = len(p["matches"])
    raw = run_adapter(exe, tmp_path, "triangulate", H.tri_blob(p))
    k = int(np.frombuffer(raw, np.int64, 1)[0])
    rec = np.dtype([("idx", np.int64, 2), ("pos", np.float32, 3), ("geom", np.float32, 5), ("desc", np.uint8, 32)])
    got = np.frombuffer(raw, rec, k, 8)
    accepted = np.frombuffer(raw, np.uint8, n, 8 + k * rec.itemsize)
    assert got["idx"].tolist() == [[int(i), int(n - 1 - i)] for i in np.flatnonzero(accepted)]
    geom = got["geom"][:, [2, 3, 4, 1, 0]]                               # (max, min, normal) -> (normal, min, max)
    P.same_facts(want, {"accepted": accepted, "wP": P.canon(got["pos"]), "geom": P.canon(geom), "desc": got["desc"]}, name)


def check_cpp_refresh(exe, tmp_path, name, want):
    """SIVO::RefreshMapPoints over stand-in map points whose observation maps walk the scene in the order of P.walked.  The program has no
    per-point bad flag (RefreshMapPoints' skip of bad points is the `if (!pMP || pMP->isBad()) continue` the null entry the program plants
    also takes), so the `_bad_points` scene is not fed to it; which points the reference touched is READ from the reference's facts here
    (to know where the stand-in point's zeros stand for `untouched`) and is not itself compared."""
    s, kf_bad, _, rev = P.refresh_scene(name)
    w = P.walked(name)
    if rev:
        kf_bad = np.concatenate([kf_bad[a:b][::-1] for a, b in zip(s["obs_off"][:-1], s["obs_off"][1:])])
    n = len(w["pos"])
    rec = np.concatenate([w["pos"], w["ref_ow"], w["level_scale"][:, None], w["last_scale"][:, None]], axis=1).astype(F)
    blob = b"".join([np.array([n], np.int64).tobytes(), w["desc_off"].astype(np.int64).tobytes(), w["obs_off"].astype(np.int64).tobytes(),
                     w["desc"].tobytes(), w["obs_ow"].tobytes(), rec.tobytes(), kf_bad.astype(np.uint8).tobytes()])
    got = np.frombuffer(run_adapter(exe, tmp_path, "refresh", blob), np.dtype([("geom", np.float32, 5), ("desc", np.uint8, 32)]), n)
    touched = want["touched"]
    geom = got["geom"][:, [2, 3, 4, 1, 0]].copy()
    assert not got["geom"][touched[:, 1] == 0].any() and not got["desc"][touched[:, 0] == 0].any()      # untouched: the stand-in point's zeros
    geom[touched[:, 1] == 0] = [0, 0, 0, -1, -1]                         # (the reference's points start from the driver's sentinels)
    P.same_facts(want, {"desc": got["desc"], "geom": P.canon(geom)}, name)


ADAPTER_REFRESH_NAMES = [n for n in P.REFRESH_NAMES if not n.endswith("_bad_points")]


@pytest.mark.parametrize("name", P.WALK_NAMES)
def test_cpp_walk_on_the_host_build_equals_the_reference(adapter_prog_host, tmp_path, name):
    check_cpp_walk(adapter_prog_host, tmp_path, name, P.reference_facts("walk." + name)[0])


def test_cpp_triangulate_matches_and_refresh_on_the_host_build_equal_the_reference(adapter_prog_host, tmp_path):
    for name in P.TRI_NAMES:
        check_cpp_triangulate_matches(adapter_prog_host, tmp_path, name, P.reference_facts("tri." + name)[0])
    for name in ADAPTER_REFRESH_NAMES:
        check_cpp_refresh(adapter_prog_host, tmp_path, name, P.reference_facts("refresh." + name)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", P.WALK_NAMES)
def test_cpp_create_new_map_points_walk_equals_the_recorded_reference(adapter_prog, tmp_path, name):
    check_cpp_walk(adapter_prog, tmp_path, name, P.recorded_facts("walk." + name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", P.TRI_NAMES)
def test_cpp_triangulate_matches_equals_the_recorded_reference(adapter_prog, tmp_path, name):
    check_cpp_triangulate_matches(adapter_prog, tmp_path, name, P.recorded_facts("tri." + name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ADAPTER_REFRESH_NAMES)
def test_cpp_refresh_map_points_equals_the_recorded_reference(adapter_prog, tmp_path, name):
    check_cpp_refresh(adapter_prog, tmp_path, name, P.recorded_facts("refresh." + name))
