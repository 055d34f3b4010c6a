"""The frustum cull (sivo_amd/csrc/frustum_math.hpp) and its C++ adapter (sivo_amd/api/orbslam/TrackingAdapter.h) pinned against the
reference's OWN Frame::isInFrustum (src/orbslam/Frame.cc:267-324, compiled untouched into oracle/_ref/libref_frame.so), without a device:
the arithmetic is compiled for the host into the stand-alone tests/frustum_prog.cpp (tests/frustum_host_capi.hpp stands in front of the
library's C ABI).  Which points are in view, and mTrackProjX / mTrackProjY / mTrackProjXR / mTrackViewCos / mnTrackScaleLevel of those,
are compared bit for bit with tests/golden/frustum_reference.npz and, where the reference library is built, with a fresh run of it.
Inputs: tests/frustum_pin_cases.py."""
import os

import numpy as np
import pytest

import frustum_pin_cases as P
import host_prog

F32 = np.float32


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return host_prog.build("frustum_prog", tmp_path_factory.mktemp("frustum_prog"))


def sources():
    """The recorded reference always; the live one where it is built."""
    out = [("recorded", P.recorded)]
    if P.reference_present():
        out.append(("live", P.reference))
    return out


def test_fixture_is_what_the_reference_computes():
    assert os.path.getsize(P.GOLDEN) < 128 * 1024
    for g in P.GROUPS:
        want = P.recorded(g)
        n = len(P.inputs(g)["pos"])
        assert want["in_view"].shape == (n,) and want["track"].shape == (n, 4) and want["level"].shape == (n,)
        if P.reference_present():
            live = P.reference(g)
            inv = live["in_view"] != 0
            assert np.array_equal(live["in_view"], want["in_view"])
            assert live["track"][inv].tobytes() == want["track"][inv].tobytes() and np.array_equal(live["level"][inv], want["level"][inv])
    assert [len(P.inputs(g)["pos"]) for g in P.GROUPS] == [600, 1440, len(P.HAND_NAMES)]


@pytest.mark.parametrize("group", P.GROUPS)
def test_host_build_equals_the_reference(prog, tmp_path, group):
    got = P.host_cull(prog, tmp_path, group)
    for name, src in sources():
        P.same_as_reference(group, got, src(group), "host build / " + name)


def test_every_exit_and_every_level_is_reached(prog, tmp_path):
    """What the cases were built for, read from the host build's status byte: every `return false` of the function at least 10 times on
    the probes (the generator of the fixture shows the same of the reference alone), every level, and the hand-made points' exits."""
    st = P.host_cull(prog, tmp_path, "probes")
    assert np.bincount(st["status"], minlength=7).tolist() == [206, 13, 159, 153, 22, 47, 0]
    assert np.bincount(st["level"][st["status"] == 0], minlength=P.NLEVELS).min() >= 10
    hand = dict(zip(P.HAND_NAMES, P.host_cull(prog, tmp_path, "hand")["status"].tolist()))
    assert hand == {"z_plus_zero": 2, "z_minus_zero": 2, "u_min": 0, "u_max": 0, "v_min": 0, "v_max": 0, "u_below_min": 2, "u_above_max": 2,
                    "v_below_min": 3, "v_above_max": 3, "cos_above": 0, "cos_below": 5, "skipped_0": 6, "skipped_1": 6, "plain": 0}
    sw = P.host_cull(prog, tmp_path, "sweep")
    k = P.inputs("sweep")["k"]
    assert set(sw["status"][k >= 0].tolist()) == {0} and set(sw["status"][k == -1].tolist()) == {0, 4}


@pytest.mark.parametrize("group", P.GROUPS)
def test_adapter_is_in_frustum_equals_the_reference(prog, tmp_path, group):
    """SIVO::isInFrustum over stand-in Frame / MapPoint types: mbTrackInView and the mTrack* members."""
    got = P.host_cull(prog, tmp_path, group, mode="isinfrustum")
    for name, src in sources():
        P.same_as_reference(group, got, src(group), "SIVO::isInFrustum / " + name)


def test_level_table_brackets_every_level(prog, tmp_path):
    """T[k] is the last float of level k: by the direct expression ceil(logf(x) / logScaleFactor), T[k] has level k and the next float
    above it level k + 1; and the count of thresholds below a ratio is the direct level on a sweep around every threshold."""
    lsf = F32(P.log_scale_factor())
    for nlevels in (1, 2, 8, 16):
        raw = P.run_prog(prog, tmp_path, "table", lsf.tobytes() + np.array([nlevels], np.int32).tobytes())
        T = np.frombuffer(raw, F32, 15)
        lv = np.frombuffer(raw, np.int32, 2 * (nlevels - 1), 60).reshape(-1, 2)
        assert lv.tolist() == [[k, k + 1] for k in range(nlevels - 1)], nlevels
        assert (np.diff(T[:nlevels - 1]) > 0).all() and not T[nlevels - 1:].any()
        assert np.allclose(T[:nlevels - 1], 1.2 ** np.arange(nlevels - 1), rtol=1e-5)


def test_sanitizer_build_of_the_program_agrees(prog, tmp_path, tmp_path_factory):
    """The stand-alone program built a second time with -fsanitize=address,undefined and run directly (it has its own main: nothing is
    preloaded), every mode: the same bytes as the plain build, and no report."""
    san_dir = tmp_path_factory.mktemp("frustum_prog_san")
    if not host_prog.sanitizer_runtime_present(san_dir):
        pytest.skip("the sanitizer runtime (libasan / libubsan) is not installed: a trivial main does not link with -fsanitize")
    san = host_prog.build("frustum_prog", san_dir, sanitize=True)
    for group in P.GROUPS:
        for mode in ("cull", "isinfrustum"):
            a, b = P.host_cull(prog, tmp_path, group, mode=mode), P.host_cull(san, tmp_path, group, mode=mode)
            assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a), (group, mode)
    blob = F32(P.log_scale_factor()).tobytes() + np.array([8], np.int32).tobytes()
    assert P.run_prog(prog, tmp_path, "table", blob) == P.run_prog(san, tmp_path, "table", blob)
    scene = bookkeeping_scene()
    assert P.run_prog(prog, tmp_path, "searchlocal", scene["blob"]) == P.run_prog(san, tmp_path, "searchlocal", scene["blob"])


# ---------------------------------------------------------------------------------------------------------------------
# SIVO::SearchLocalPoints: the bookkeeping of Tracking.cc:1033-1085 on a hand-made map
# ---------------------------------------------------------------------------------------------------------------------
FRAME_ID = 41


def bookkeeping_scene():
    """The probes as the map.  The frame holds 120 keys at the projections of points in view (noisy copies of their descriptors); 30 of its
    slots already hold a map point — every third of those bad, some with no observation — whose mnLastFrameSeen is an older frame.  The
    local map lists every point once, in a shuffled order; some of its points are bad, some were already seen in this frame."""
    import search_local_cases as S
    return S.bookkeeping_scene(FRAME_ID)


def test_search_local_points_bookkeeping_is_the_references(prog, tmp_path):
    import search_local_cases as S
    sc = bookkeeping_scene()
    raw = P.run_prog(prog, tmp_path, "searchlocal", sc["blob"])
    n, nk = sc["n"], sc["nk"]
    ret, n_to_match = np.frombuffer(raw, np.int32, 2)
    rec = np.frombuffer(raw, S.POINT_OUT, n, 8)
    slots = np.frombuffer(raw, np.int32, nk, 8 + n * S.POINT_OUT.itemsize)
    want = S.walk_search_local_points(sc, P.recorded("probes"))
    # the first loop: bad points leave their slot, the others are counted visible and stamped
    assert np.array_equal(rec["visible"], want["visible"]) and np.array_equal(rec["last_seen"], want["last_seen"])
    held = np.zeros(n, bool)
    held[sc["slot"][sc["slot"] >= 0]] = True
    assert (want["visible"][held & ~sc["bad"]] == 1).all() and (want["last_seen"][held & ~sc["bad"]] == FRAME_ID).all()
    assert (want["visible"][held & sc["bad"]] == 0).all() and (held & sc["bad"]).sum() >= 10
    # the cull: mbTrackInView and the mTrack* members of the points in view are the reference's, every other point keeps what it had
    assert np.array_equal(rec["in_view"] != 0, want["in_view"])
    inv = want["in_view"]
    src = sc["m"]["src"]
    ref = {k: v[src] for k, v in P.recorded("probes").items()}
    assert rec["track"][inv].tobytes() == ref["track"][inv].tobytes() and np.array_equal(rec["level"][inv], ref["level"][inv])
    assert (rec["track"][~inv].view(np.uint32) == P.SENTINEL.view(np.uint32)).all() and (rec["level"][~inv] == P.LEVEL_SENTINEL).all()
    assert int(n_to_match) == int(inv.sum()) and 30 < int(n_to_match) < int((ref["in_view"] != 0).sum())
    skipped_in_view = sc["ref_in_view"] & ~inv                          # in the frustum, but bad or already seen: not projected
    assert skipped_in_view.sum() >= 10 and (rec["visible"][skipped_in_view & ~held] == 0).all()
    # the search: the slots after the call and the count, against the sequential oracle fed with the reference's track fields
    assert np.array_equal(slots, want["slots"]) and int(ret) == want["n_matches"] and want["n_matches"] > 30
    freed = sc["slot_bad"]                                              # a bad point's slot is free again: empty, or taken by a match
    assert freed.sum() >= 10 and (slots[freed] != sc["slot"][freed]).all() and (slots[freed] == -1).any() and (slots[freed] >= 0).any()
