"""The batched fusion search without a device: the host build of the kernel's per-pair arithmetic (sivo_amd/csrc/fuse_math.hpp through
tests/fuse_batch_prog.cpp) against the numpy restatement of ORBmatcher::Fuse (tests/fuse_batch_restatement.py), bit for bit on every scene
of tests/fuse_batch_cases.py; the C++ adapters (sivo_amd/api/orbslam/FusionAdapter.h) against the loop of single-keyframe Fuse calls on
copies of one object graph (tests/fuse_batch_adapter_prog.cpp); the scenes themselves; every argument rule with its message; the
sanitizer builds of both programs; the ABI's declarations."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fuse_batch_adapter_cases as AC
import fuse_batch_cases as FC
import fuse_batch_restatement as R
import host_prog

ROOT = host_prog.ROOT
ALL_SCENES = FC.HAND_SCENES + ("random",)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return host_prog.build("fuse_batch_prog", tmp_path_factory.mktemp("fuse_batch_prog"))


@pytest.fixture(scope="module")
def adapter_prog(tmp_path_factory):
    return host_prog.build("fuse_batch_adapter_prog", tmp_path_factory.mktemp("fuse_batch_adapter_prog"))


def run_batch(exe, tmp_path, sc, **kw):
    K, N = len(sc["frames"]), len(sc["pos"])
    pairs = kw.get("pairs_out", K * N)
    return FC.parse(host_prog.run(exe, tmp_path, "batch", FC.blob(sc, **kw)), pairs, (K, N) if pairs == K * N else None)


def run_adapter(exe, tmp_path, name, repair=True):
    w = AC.scene(name)
    return AC.parse(host_prog.run(exe, tmp_path, AC.mode(name), AC.blob(w, repair=repair)), w)


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------
def test_scenes_show_what_they_are_named_for(adapter_prog, tmp_path):
    """Each scene reaches its branch in the restatement's own answer (resp. in the event log of the loop of single calls): a scene that
    stopped doing so would leave its test green and empty."""
    def of(name):
        sc = FC.scene(name)
        return sc, sc["expect"], {n: i for i, n in enumerate(sc["names"])}

    sc, e, at = of("depth_and_image")
    st = e["status"][0]
    assert sc["pos"][at["z_zero"], 2] == 0 and not np.signbit(sc["pos"][at["z_zero"], 2]) and np.signbit(sc["pos"][at["z_minus_zero"], 2])
    assert [st[at[n]] for n in ("z_zero", "z_zero_axis", "z_minus_zero", "z_just_behind")] == [R.IMAGE, R.IMAGE, R.IMAGE, R.BEHIND]
    assert [st[at[n]] for n in ("u_min", "u_max", "v_min", "v_max")] == [R.NO_CANDIDATE, R.IMAGE, R.NO_CANDIDATE, R.IMAGE]
    assert e["u"][0, at["u_min"]] == 0.0 and e["v"][0, at["v_min"]] == 0.0 and st[at["u_below_min"]] == R.IMAGE and st[at["u_below_max"]] == R.NO_CANDIDATE
    assert 639.99 < e["u"][0, at["u_below_max"]] < 640.0
    sc, e, at = of("distance_and_angle")
    st = e["status"][0]
    assert np.float32(0.8) * sc["min_dist"][at["at_min"]] == 4.0 and np.float32(1.2) * sc["max_dist"][at["at_max"]] == 4.0
    assert [st[at[n]] for n in ("at_min", "below_min", "at_max", "above_max")] == [R.NO_CANDIDATE, R.DISTANCE, R.NO_CANDIDATE, R.DISTANCE]
    assert sc["normal"][at["cos_at_half"], 2] == 0.5 and sc["normal"][at["cos_below_half"], 2] < 0.5
    assert [st[at[n]] for n in ("cos_at_half", "cos_below_half", "cos_negative")] == [R.NO_CANDIDATE, R.ANGLE, R.ANGLE]
    sc, e, at = of("levels")
    assert np.all(e["status"] == R.NO_CANDIDATE)
    lv = e["level"][0, :len(FC.LEVEL_KS) * len(FC.LEVEL_STEPS)].reshape(len(FC.LEVEL_KS), len(FC.LEVEL_STEPS))
    changes = [k for k in range(len(FC.LEVEL_KS)) if lv[k, 0] != lv[k, -1]]
    assert changes == list(range(FC.NLEVELS - 1)) and np.all(np.diff(lv, axis=1) >= 0)          # the table decides inside every sweep below the clamp
    assert np.all(lv[FC.NLEVELS - 1:] == FC.NLEVELS - 1)
    assert [e["level"][0, at[n]] for n in ("ratio_below_one", "ratio_huge", "ratio_inf")] == [0, FC.NLEVELS - 1, FC.NLEVELS - 1]
    assert e["level"][1].max() == 2 and np.array_equal(e["level"][1], np.minimum(e["level"][0], 2))     # a camera of three levels clamps at 2
    sc, e, at = of("windows")
    assert e["status"][:, 0].tolist() == [R.NO_CANDIDATE, R.TOO_FAR, R.MATCHED, R.NO_CANDIDATE] and e["level"][0, 0] == 2
    assert sorted(sc["frames"][1].octave.tolist()) == [0, 3] and e["best_idx"][2, 0] == 1 and e["best_dist"][2, 0] == 20
    sc, e, at = of("gates")
    assert e["status"][:6, 0].tolist() == [R.MATCHED, R.TOO_FAR, R.MATCHED, R.TOO_FAR, R.MATCHED, R.TOO_FAR]       # around 7.8, around 5.99, mvRight alone
    assert np.all(e["status"][6:, 0] == R.MATCHED) and np.all(sc["cams"]["scw_variant"][6:] == 1)               # no gate in the Scw form
    assert sc["frames"][4].u_right is None and sc["frames"][2].u_right[0] < 0 and sc["frames"][0].u_right[0] >= 0
    sc, e, at = of("ties_and_threshold")
    assert e["best_idx"][:4, 0].tolist() == [1, 0, 1, 0] and e["best_dist"][:6, 0].tolist() == [20, 20, 19, 50, 51, R.INT_MAX]
    assert e["status"][3:6, 0].tolist() == [R.MATCHED, R.TOO_FAR, R.TOO_FAR] and e["best_dist"][11, 0] == 256
    f = sc["frames"][0]
    assert f.features_in_area(320.0, 240.0, 5.18) == [1, 0]                                         # grid order, not index order
    sc, e, at = of("masks")
    assert (e["status"] == R.SKIPPED).sum() == 4 and (e["status"] == R.MATCHED).sum() == 4
    sc, e, at = of("posed")
    assert set(np.unique(e["status"])) >= {R.MATCHED, R.BEHIND, R.IMAGE, R.DISTANCE, R.ANGLE} or set(np.unique(e["status"])) >= {R.BEHIND, R.IMAGE, R.DISTANCE, R.ANGLE}
    sc, e, at = of("random")
    assert [f.n for f in sc["frames"]] == list(FC.RANDOM_KEYS) and e["status"].shape == (5, 203)
    crowd = sc["frames"][4]
    assert max(len(c) for col in crowd.grid for c in col) > 64
    reached = np.isin(e["status"][4], (R.MATCHED, R.NO_CANDIDATE, R.TOO_FAR))
    windows = [len(crowd.features_in_area(e["u"][4, i], e["v"][4, i], np.float32(sc["th"]) * crowd.scale[e["level"][4, i]])) for i in np.flatnonzero(reached)]
    assert max(windows) > 64                                                                        # more candidates than lanes
    assert (e["status"] == R.MATCHED).sum() > 40 and (e["status"] == R.TOO_FAR).sum() > 40 and set(sc["cams"]["scw_variant"]) == {0, 1}
    assert sc["frames"][2].u_right is None and any(f.u_right is not None and (f.u_right < 0).any() and (f.u_right >= 0).any() for f in sc["frames"])

    # the object graphs, read off the loop of single-keyframe calls
    def events(name, **kw):
        a, b, counters = run_adapter(adapter_prog, tmp_path, name, **kw)
        return AC.scene(name), a, b, counters

    w, a, b, c = events("replaced_later_entry")
    A, B = w.names["A"], w.names["B"]
    assert ("replace", B, A, 0) in b["events"] and b["points"][B]["bad"] and w.list.index(B) > w.list.index(A)
    assert not any(ev[0] == "add_observation" and ev[1] == B for ev in b["events"]) and b["n_fused"] == [1, 1]
    w, a, b, c = events("descriptor_change")
    A = w.names["A"]
    assert b["points"][A]["desc"] == AC.DC0.tobytes() and ("descriptor", A, AC.kf_id(0), 0) in b["events"]
    assert ("add_observation", A, AC.kf_id(1), 1) in b["events"] and b["n_fused"] == [1, 1, 0] and c["repairs"] == 1 and c["batch"] == 2
    w, a_off, b_off, c_off = events("descriptor_change", repair=False)
    assert b_off == b and a_off["events"] != b["events"] and c_off["repairs"] == 0 and c_off["batch"] == 1
    assert ("add_observation", A, AC.kf_id(1), 0) in a_off["events"] and ("add_observation", A, AC.kf_id(2), 0) in a_off["events"]
    w, a, b, c = events("enters_by_replace")
    A, Cp = w.names["A"], w.names["C"]
    assert ("replace", Cp, A, 0) in b["events"] and ("replace_match", AC.kf_id(2), 0, A) in b["events"] and b["n_fused"] == [0, 1, 0]
    assert b["slots"][2] == [A, -1] and c["batch"] == 1
    w, a, b, c = events("observation_ties")
    assert ("replace", w.names["C"], w.names["A"], 0) in b["events"] and ("replace", w.names["B"], w.names["D"], 0) in b["events"]
    w, a, b, c = events("null_and_bad")
    assert w.list[0] == -1 and w.points[w.list[1]]["bad"] and b["n_fused"] == [1, 1] and len([ev for ev in b["events"] if ev[0] == "add_map_point"]) == 2
    w, a, b, c = events("loop_same_point_two_keyframes")
    A, Cp = w.names["A"], w.names["C"]
    assert [ev for ev in b["events"] if ev[0] == "replace"] == [("replace", Cp, A, 0)] and b["n_fused"] == [2, 1] and b["slots"][1][0] == A
    w, a, b, c = events("loop_descriptor_change")
    assert b["points"][w.names["A"]]["desc"] == AC.DC0.tobytes() and ("add_observation", w.names["A"], AC.kf_id(1), 1) in b["events"] and c["repairs"] == 1
    w, a_off, b_off, c_off = events("loop_descriptor_change", repair=False)
    assert a_off["events"] != b["events"]


# ---- the host build against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_SCENES)
def test_host_build_equals_the_restatement(prog, tmp_path, name):
    sc = FC.scene(name)
    rc, text, got = run_batch(prog, tmp_path, sc)
    assert rc == 0 and text == "" and FC.differences(got, sc["expect"]) == []


def test_optional_outputs_and_masks_may_be_null(prog, tmp_path):
    sc = FC.scene("random")
    rc, text, got = run_batch(prog, tmp_path, sc, null=("u", "ur"))
    e = dict(sc["expect"])
    e["u"] = np.full_like(e["u"], R.U_SENTINEL); e["ur"] = np.full_like(e["ur"], R.U_SENTINEL)
    assert rc == 0 and FC.differences(got, e) == []
    m = FC.scene("masks")
    rc, text, got = run_batch(prog, tmp_path, m, null=("skip_point", "skip_pair"))
    assert rc == 0 and np.all(got["status"] == R.MATCHED)


# ---- the adapters against the loop of single calls ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(AC.SCENES))
def test_adapter_equals_the_loop_of_single_keyframe_calls(adapter_prog, tmp_path, name):
    """Event logs, slots, observation maps, bad flags, descriptors, found / visible counters, what vpReplacePoints caused, and the
    per-keyframe nFused: identical.  The batch needs one device call, and one more per keyframe in front of which a descriptor changed."""
    a, b, counters = run_adapter(adapter_prog, tmp_path, name)
    assert a == b
    assert counters["batch"] == 1 + counters["repairs"] and counters["single"] == 0          # (the adapter's run: no single-keyframe call)


# ---- the argument rules --------------------------------------------------------------------------------------------------------------------
def invalid_blobs():
    """(message, blob, pairs) for every rule."""
    sc = FC.scene("masks")
    K, N = 2, 4
    out = [("negative count", FC.blob(sc, n_kf=-1), K * N), ("negative count", FC.blob(sc, n_mp=-1), K * N)]
    out += [("null frame array", FC.blob(sc, null=("kfs",)), K * N), ("null camera array", FC.blob(sc, null=("cams",)), K * N)]
    out += [("null point array", FC.blob(sc, null=(n,)), K * N) for n in ("pos", "normal", "min_dist", "max_dist", "mp_desc")]
    out += [("null output", FC.blob(sc, null=(n,)), K * N) for n in ("best_idx", "best_dist", "status")]
    out += [("null frame", FC.blob(sc, null_frames=(1,)), K * N), ("frames on different devices", FC.blob(sc, devices=(0, 1)), K * N)]
    for what, change in (("nlevels outside 1 .. 16", dict(nlevels=0)), ("nlevels outside 1 .. 16", dict(nlevels=17)),
                         ("nlevels above the frame's", dict(nlevels=9)), ("log_scale_factor is not positive", dict(log_scale_factor=0.0)),
                         ("log_scale_factor is not positive", dict(log_scale_factor=-0.1)), ("log_scale_factor is not positive", dict(log_scale_factor=np.nan))):
        cams = sc["cams"].copy()
        for k, v in change.items():
            cams[k][1] = v
        out.append((what, FC.blob(dict(sc, cams=cams)), K * N))
    # null arrays with a zero count are nobody's business
    return out


def test_every_argument_rule_has_its_message_and_writes_nothing(prog, tmp_path):
    seen = set()
    for what, blob, pairs in invalid_blobs():
        rc, text, got = FC.parse(host_prog.run(prog, tmp_path, "batch", blob), pairs)
        assert rc == 1 and text == "sivo_fuse_batch: " + what, (what, text)
        assert np.all(got["best_idx"] == -7) and np.all(got["best_dist"] == -7) and np.all(got["status"] == 255), what
        assert np.all(got["u"] == R.U_SENTINEL) and np.all(got["v"] == R.U_SENTINEL) and np.all(got["ur"] == R.U_SENTINEL) and np.all(got["level"] == R.LEVEL_SENTINEL), what
        seen.add(what)
    assert len(seen) == 10
    # no keyframe or no point: success, nothing launched, nothing written
    sc = FC.scene("masks")
    for kw in (dict(n_kf=0, null=("kfs", "cams", "best_idx", "best_dist", "status")), dict(n_mp=0, null=("pos", "normal", "min_dist", "max_dist", "mp_desc", "status"))):
        rc, text, got = FC.parse(host_prog.run(prog, tmp_path, "batch", FC.blob(sc, **kw)), 8)
        assert rc == 0 and text == "" and np.all(got["status"] == 255) and np.all(got["best_idx"] == -7)


def test_sanitizer_builds_of_both_programs_agree(prog, adapter_prog, tmp_path, tmp_path_factory):
    """Both stand-alone programs built a second time with -fsanitize=address,undefined and run directly (each has its own main: nothing is
    preloaded) on every scene and every argument rule: the same bytes as the plain build, and no report."""
    san_dir = tmp_path_factory.mktemp("fuse_batch_prog_san")
    if not host_prog.sanitizer_runtime_present(san_dir):
        pytest.skip("the sanitizer runtime (libasan / libubsan) is not installed: a trivial main does not link with -fsanitize")
    san = host_prog.build("fuse_batch_prog", san_dir, sanitize=True)
    asan = host_prog.build("fuse_batch_adapter_prog", san_dir, sanitize=True)
    for name in ALL_SCENES:
        blob = FC.blob(FC.scene(name))
        assert host_prog.run(prog, tmp_path, "batch", blob) == host_prog.run(san, tmp_path, "batch", blob), name
    for what, blob, pairs in invalid_blobs():
        assert host_prog.run(prog, tmp_path, "batch", blob) == host_prog.run(san, tmp_path, "batch", blob), what
    for name in AC.SCENES:
        for repair in (True, False):
            blob = AC.blob(AC.scene(name), repair=repair)
            assert host_prog.run(adapter_prog, tmp_path, AC.mode(name), blob) == host_prog.run(asan, tmp_path, AC.mode(name), blob), name


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------
def test_struct_prototype_and_signature(tmp_path):
    from sivo_amd import _lib, matcher
    header = open(os.path.join(ROOT, "include", "sivo_hip.h")).read()
    assert re.search(r"int sivo_fuse_batch\(const sivo_mframe_t \*kfs, const SivoFuseCamera \*cams, int n_kf, int n_mp,", header)
    assert re.search(r"enum \{ SIVO_FUSE_MATCHED = 0, SIVO_FUSE_SKIPPED, SIVO_FUSE_BEHIND, SIVO_FUSE_IMAGE, SIVO_FUSE_DISTANCE,\s+SIVO_FUSE_ANGLE, "
                     r"SIVO_FUSE_NO_CANDIDATE, SIVO_FUSE_TOO_FAR \};", header)
    host_prog.c_layout(tmp_path, "SivoFuseCamera", _lib.FuseCamera)
    assert C.sizeof(_lib.FuseCamera) == matcher.FUSE_CAMERA_DTYPE.itemsize == R.CAMERA_DTYPE.itemsize == 108
    assert [f[0] for f in _lib.FuseCamera._fields_] == list(matcher.FUSE_CAMERA_DTYPE.names) == list(R.CAMERA_DTYPE.names)
    for n in matcher.FUSE_CAMERA_DTYPE.names:
        assert matcher.FUSE_CAMERA_DTYPE.fields[n][1] == getattr(_lib.FuseCamera, n).offset == R.CAMERA_DTYPE.fields[n][1], n
    vp = C.c_void_p
    assert _lib.SIGNATURES["sivo_fuse_batch"] == [vp, vp, C.c_int, C.c_int] + [vp] * 7 + [C.c_float] + [vp] * 7
    assert matcher.FUSE_STATUS == ("matched", "skipped", "behind", "image", "distance", "angle", "no_candidate", "too_far")
    assert (R.MATCHED, R.SKIPPED, R.BEHIND, R.IMAGE, R.DISTANCE, R.ANGLE, R.NO_CANDIDATE, R.TOO_FAR) == tuple(range(8))
    makefile = open(os.path.join(ROOT, "sivo_amd", "csrc", "Makefile")).read()
    assert " fuse_batch.hip " in makefile


def test_library_checks_arguments_first_and_fails_loudly_without_a_device():
    """The library refuses bad arguments before it touches a device — this test runs where there is none — and n_kf == 0 or n_mp == 0
    succeeds without one."""
    from sivo_amd import _lib
    L = _lib.lib()
    one = (C.c_void_p * 1)(None)
    cam = FC.camera()
    buf = np.zeros(64, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda kfs, cams, n_kf, n_mp, pts=buf, out=buf: L.sivo_fuse_batch(kfs, cams, n_kf, n_mp, p(pts) if pts is not None else None, p(buf), p(buf), p(buf),
                                                                             p(buf), None, None, 3.0, p(out) if out is not None else None, p(buf), p(buf),
                                                                             None, None, None, None)
    for what, args in ((b"negative count", (one, p(cam), -1, 1)), (b"negative count", (one, p(cam), 1, -1)), (b"null frame array", (None, p(cam), 1, 1)),
                       (b"null camera array", (one, None, 1, 1)), (b"null point array", (one, p(cam), 1, 1, None)), (b"null output", (one, p(cam), 1, 1, buf, None)),
                       (b"null frame", (one, p(cam), 1, 1))):
        assert call(*args) == _lib.ERR_INVALID_ARGUMENT and L.sivo_last_error() == b"sivo_fuse_batch: " + what, what
    assert call(None, None, 0, 5) == 0 and call(one, p(cam), 0, 0) == 0
    assert np.all(buf == 0)
