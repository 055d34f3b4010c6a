"""The loop closer's two map corrections without a device: the host build of the kernels' per-item bodies (sivo_amd/csrc/loopcorrect_math.hpp
through tests/loop_correct_prog.cpp) and the C++ adapter over stand-in SLAM types (tests/loop_correct_adapter_prog.cpp) against the
object-graph restatement of the reference (tests/loop_correct_restatement.py), byte for byte on every scene of tests/loop_correct_cases.py;
the scenes themselves; the restatement against a plain float64 pipeline; every argument rule with its message; the ABI's declarations."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import host_prog
import loop_correct_cases as LC
import loop_correct_float64 as F64
import loop_correct_restatement as LR

ROOT = host_prog.ROOT
S = LC.SENTINEL


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return host_prog.build("loop_correct_prog", tmp_path_factory.mktemp("loop_correct_prog"))


@pytest.fixture(scope="module")
def adapter_prog(tmp_path_factory):
    return host_prog.build("loop_correct_adapter_prog", tmp_path_factory.mktemp("loop_correct_adapter_prog"))


def run_loop(exe, tmp_path, a, **kw):
    k = kw.get("k_out", max(a["n_kf"], 0))
    p = kw.get("p_out", max(a["n_points"], 0))
    return LC.parse(host_prog.run(exe, tmp_path, "loop", LC.loop_blob(a, **kw)), LC.LOOP_OUT, k, p)


def run_gba(exe, tmp_path, a, **kw):
    k = kw.get("k_out", max(a["n_kf"], 0))
    p = kw.get("p_out", max(a["n_points"], 0))
    return LC.parse(host_prog.run(exe, tmp_path, "gba", LC.gba_blob(a, **kw)), LC.GBA_OUT, k, p)


# ---- the scenes --------------------------------------------------------------------------------------------------------------------
def test_scenes_show_what_they_are_named_for():
    """Each scene exercises its quirk in the restatement's own output: a scene that stopped doing so would leave its test green and
    empty."""
    def loop(name):
        sc = LC.loop_scene(name)
        return sc["args"], sc["expect"], sc["info"], sc["info"]["spec"]

    a, e, info, sp = loop("only_current")
    assert a["n_kf"] == 1 and a["cur"] == 0 and e["corrected_siw"][0].tobytes() == a["scw"].tobytes() and (e["corrected_by"] == 0).sum() > 3
    a, e, info, sp = loop("two_keyframes")
    assert a["n_kf"] == 2 and set(e["corrected_by"]) == {-1, 0, 1}
    a, e, info, sp = loop("sixty_five_keyframes")
    assert a["n_kf"] == 65 and a["scw"][7] == 1.07 and len(set(e["corrected_by"])) > 40
    assert e["corrected_siw"][a["cur"]].tobytes() == a["scw"].tobytes() and np.all(e["corrected_siw"][:, 7] == 1.07)
    a, e, info, sp = loop("three_holders")
    holders = [i for i in range(a["n_kf"]) if sp["mark"] in a["slot_point"][a["slot_off"][i]:a["slot_off"][i + 1]]]
    assert holders == sp["holders"] and len(holders) == 3 and e["corrected_by"][sp["mark"]] == holders[0] and info["points"][sp["mark"]].updates == 1
    assert info["kfs"].index(info["table"][holders[0]]) != min(info["kfs"].index(info["table"][h]) for h in holders)     # not the first of the vector
    a, e, info, sp = loop("duplicate_slot")
    row = a["slot_point"][a["slot_off"][1]:a["slot_off"][2]]
    assert (row == sp["mark"]).sum() == 2 and e["corrected_by"][sp["mark"]] == 1 and info["points"][sp["mark"]].updates == 1
    a, e, info, sp = loop("skip")
    done, bad = sp["marks"]
    assert info["points"][bad].mbBad and not info["points"][done].mbBad and info["points"][done].mnCorrectedReference == 0
    for p in sp["marks"]:
        assert a["skip"][p] and p in a["slot_point"][a["slot_off"][0]:a["slot_off"][1]] and e["corrected_by"][p] == -1 and np.all(e["pos_out"][p] == S)
    a, e, info, sp = loop("null_slots")
    rows = [a["slot_point"][a["slot_off"][i]:a["slot_off"][i + 1]] for i in range(a["n_kf"])]
    assert any(len(r) and np.all(r == -1) for r in rows) and any(r[0] == -1 and r[-1] == -1 and np.any(r >= 0) for r in rows if len(r))
    a, e, info, sp = loop("empty_keyframe")
    assert a["slot_off"][2] == a["slot_off"][1] and a["cur"] != 1 and np.all(e["tiw_out"][1] != S) and 1 not in e["corrected_by"]
    a, e, info, sp = loop("observer_lengths")
    assert [int(a["obs_off"][p + 1] - a["obs_off"][p]) for p in sp["marks"]] == [0, 1, 63, 64, 65]
    assert np.all(e["corrected_by"][sp["marks"]] == 1) and e["flags"][sp["marks"]].tolist() == [LR.NO_OBSERVATION, 0, 0, 0, 0]
    assert np.all(e["normal"][sp["marks"][0]] == S) and np.all(e["pos_out"][sp["marks"][0]] != S) and np.all(e["normal"][sp["marks"][1:]] != S)
    a, e, info, sp = loop("reference_places")
    refs = [int(a["ref_kf"][p]) for p in sp["marks"]]
    assert np.all(e["corrected_by"][sp["marks"]] == 2) and refs[0] < 2 and refs[1] == 2 and 2 < refs[2] < a["n_kf"] and refs[3] >= a["n_kf"]
    for j, p in enumerate(sp["marks"]):                      # only a reference keyframe the walk had left behind shows its new centre
        seen, kf = info["points"][p].centres_seen[-1], info["table"][refs[j]]
        old, new = info["old_centres"][kf], kf.GetCameraCenter()
        assert not np.array_equal(old, new) or refs[j] >= a["n_kf"]
        assert np.array_equal(seen, new if j == 0 else old)
    a, e, info, sp = loop("outside_observers")
    obs = a["obs_kf"][a["obs_off"][sp["mark"]]:a["obs_off"][sp["mark"] + 1]]
    assert (obs >= a["n_kf"]).sum() == 4 and e["corrected_by"][sp["mark"]] == 2 and e["flags"][sp["mark"]] == 0
    for total in (255, 256, 257, 769):
        a, e, info, sp = loop("slots_%d" % total)
        assert a["slot_off"][-1] == total and a["slot_point"][-1] == sp["mark"] and (a["slot_point"] == sp["mark"]).sum() == 1
        assert e["corrected_by"][sp["mark"]] == 2
    a, e, info, sp = loop("quaternion_branches")
    assert {LC.quat_branch(T) for T in a["tiw"]} == {0, 1, 2, 3}
    assert loop("scale_one")[0]["scw"][7] == 1.0 and loop("scale_1_07")[0]["scw"][7] == 1.07
    assert np.any(loop("scale_one")[1]["tiw_out"] != loop("scale_1_07")[1]["tiw_out"])

    def tree(name):
        sc = LC.tree_scene(name)
        return sc["args"], sc["expect"], sc["info"]["spec"]

    for run in (0, 1, 2, 40):
        a, e, sp = tree("run_%d" % run)
        assert max(LC.run_lengths(sp), default=0) == run and int(e["in_gba"].sum() - a["in_gba"].sum()) == run and np.all(e["kf_reached"] == 1)
    a, e, sp = tree("origin_outside")
    assert a["in_gba"][0] == 0 and e["in_gba"][0] == 0 and e["kf_reached"][0] == 1 and e["tcw_out"][0].tobytes() == a["tcw_gba"][0].tobytes()
    assert (e["point_status"] == LR.POINT_REF_OUTSIDE).sum() > 0
    a, e, sp = tree("unreached_reference")
    assert np.all(e["kf_reached"][sp["marks"]] == 0) and np.all(e["tcw_out"][sp["marks"]] == S)
    assert e["tcw_bef"][sp["marks"]].tobytes() == a["tcw_bef"][sp["marks"]].tobytes()
    assert e["point_status"][:3].tolist() == [LR.POINT_CARRIED, LR.POINT_REF_OUTSIDE, LR.POINT_CARRIED] and a["ref_kf"][:3].tolist() == sp["marks"]
    a, e, sp = tree("two_origins")
    assert a["n_origins"] == 2 and np.all(e["kf_reached"] == 1) and (a["in_gba"] == 0).sum() == 4
    a, e, sp = tree("bad_point")
    assert e["point_status"][3] == LR.POINT_BAD and e["point_status"][4] == LR.POINT_BAD and a["point_in_gba"][4] and np.all(e["pos_out"][3:5] == S)
    assert tree("points_0")[0]["n_points"] == 0
    for n in (255, 256, 257):
        a, e, sp = tree("points_%d" % n)
        assert a["n_points"] == n and set(e["point_status"]) >= {0, 1, 2}
    assert sum(int(LC.loop_scene(n)["args"]["slot_off"][-1]) for n in LC.LOOP_SCENES) < 5000


# ---- the host build and the adapter against the restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", LC.LOOP_SCENES)
def test_loop_scene_host_build_and_adapter_match_the_restatement(prog, adapter_prog, tmp_path, name):
    sc = LC.loop_scene(name)
    a = sc["args"]
    rc, text, got = run_loop(prog, tmp_path, a)
    assert rc == 0 and text == "" and LC.same_bytes(got, sc["expect"]) == []
    raw = host_prog.run(adapter_prog, tmp_path, "loop", LC.loop_adapter_blob(sc))
    rc, text, got = LC.parse(raw, LC.LOOP_OUT + LC.CALLS, a["n_kf"], a["n_points"])
    assert rc == 0 and got.pop("calls").tolist() == [1] and LC.same_bytes(got, sc["expect"]) == []


@pytest.mark.parametrize("name", LC.TREE_SCENES)
def test_tree_scene_host_build_and_adapter_match_the_restatement(prog, adapter_prog, tmp_path, name):
    sc = LC.tree_scene(name)
    a = sc["args"]
    rc, text, got = run_gba(prog, tmp_path, a)
    assert rc == 0 and text == "" and LC.same_bytes(got, sc["expect"]) == []
    raw = host_prog.run(adapter_prog, tmp_path, "gba", LC.gba_adapter_blob(sc))
    rc, text, got = LC.parse(raw, LC.GBA_OUT + LC.CALLS, a["n_kf"], a["n_points"])
    assert rc == 0 and got.pop("calls").tolist() == [1] and LC.same_bytes(got, sc["expect"]) == []


def test_sanitizer_builds_of_both_programs_agree(prog, adapter_prog, tmp_path, tmp_path_factory):
    """Both stand-alone programs built a second time with -fsanitize=address,undefined and run directly (each has its own main: nothing is
    preloaded) on every scene, and the argument rules on the first: the same bytes as the plain build, and no report."""
    san_dir = tmp_path_factory.mktemp("loop_correct_prog_san")
    if not host_prog.sanitizer_runtime_present(san_dir):
        pytest.skip("the sanitizer runtime (libasan / libubsan) is not installed: a trivial main does not link with -fsanitize")
    san = host_prog.build("loop_correct_prog", san_dir, sanitize=True)
    asan = host_prog.build("loop_correct_adapter_prog", san_dir, sanitize=True)
    for name in LC.LOOP_SCENES:
        sc = LC.loop_scene(name)
        blob, ablob = LC.loop_blob(sc["args"]), LC.loop_adapter_blob(sc)
        assert host_prog.run(prog, tmp_path, "loop", blob) == host_prog.run(san, tmp_path, "loop", blob), name
        assert host_prog.run(adapter_prog, tmp_path, "loop", ablob) == host_prog.run(asan, tmp_path, "loop", ablob), name
    for name in LC.TREE_SCENES:
        sc = LC.tree_scene(name)
        blob, ablob = LC.gba_blob(sc["args"]), LC.gba_adapter_blob(sc)
        assert host_prog.run(prog, tmp_path, "gba", blob) == host_prog.run(san, tmp_path, "gba", blob), name
        assert host_prog.run(adapter_prog, tmp_path, "gba", ablob) == host_prog.run(asan, tmp_path, "gba", ablob), name
    for what, mode, blob, k, p in invalid_blobs():
        assert host_prog.run(prog, tmp_path, mode, blob) == host_prog.run(san, tmp_path, mode, blob), what


# ---- the restatement against a plain float64 pipeline --------------------------------------------------------------------------------
# The largest difference between the restatement and tests/loop_correct_float64.py over all scenes, measured on the CPU (poses and
# normals absolutely, positions and distances relative to the largest coordinate): float32 rounding of the poses and points, a few ulps
# of the scene's extent.  The bound is the measured value times 4, which absorbs scene edits; a mistake in the order of operations, in
# which keyframe owns a point or in which camera centre a point sees shows up at 1e-2 .. 1.
MEASURED_LOOP = {"tiw_out": 2.79e-6, "ow_out": 2.13e-7, "pos_out": 1.47e-7, "normal": 4.19e-7, "max_dist": 1.04e-7, "min_dist": 1.10e-7}
MEASURED_TREE = {"tcw_out": 4.01e-6, "pos_out": 2.71e-7}
LOOP_KINDS = (("tiw_out", "pose"), ("ow_out", "point"), ("pos_out", "point"), ("normal", "pose"), ("max_dist", "point"), ("min_dist", "point"))


def test_restatement_agrees_with_a_float64_pipeline(capsys):
    worst = {}
    for name in LC.LOOP_SCENES:
        sc = LC.loop_scene(name)
        a, e = sc["args"], sc["expect"]
        o = F64.correct_loop(a)
        assert np.array_equal(o["corrected_by"], e["corrected_by"]), name
        moved = e["corrected_by"] >= 0
        geo = moved & (e["flags"] == 0)
        assert np.array_equal(~np.isnan(o["normal"][:, 0]), geo), name
        for k, v in F64.differences(LOOP_KINDS, e, o, {"pos_out": moved, "normal": geo, "max_dist": geo, "min_dist": geo}).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("loop correction, restatement vs float64:", {k: "%.3g" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= 4 * MEASURED_LOOP[k], (k, v)
    worst = {}
    for name in LC.TREE_SCENES:
        sc = LC.tree_scene(name)
        a, e = sc["args"], sc["expect"]
        o = F64.propagate_global_ba(a)
        reached, written = e["kf_reached"].astype(bool), np.isin(e["point_status"], (LR.POINT_FROM_BA, LR.POINT_CARRIED))
        assert np.array_equal(o["kf_reached"], reached) and np.array_equal(~np.isnan(o["pos_out"][:, 0]), written), name
        for k, v in F64.differences((("tcw_out", "pose"), ("pos_out", "point")), e, o, {"tcw_out": reached, "pos_out": written}).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("global BA propagation, restatement vs float64:", {k: "%.3g" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= 4 * MEASURED_TREE[k], (k, v)


def test_identity_correction_returns_every_pose_and_point():
    """mg2oScw = the current keyframe's own uncorrected Sim3: every corrected Sim3 is the uncorrected one up to rounding, so every pose,
    camera centre and moved point comes back within the bound of the float64 comparison."""
    sc = LC.loop_scene("identity_correction")
    a, e = sc["args"], sc["expect"]
    moved = e["corrected_by"] >= 0
    assert moved.sum() > 20
    d = F64.differences((("tiw_out", "pose"), ("ow_out", "point"), ("pos_out", "point")), e,
                        {"tiw_out": a["tiw"], "ow_out": a["ow"][:a["n_kf"]], "pos_out": a["pos"]}, {"pos_out": moved})
    for k, v in d.items():
        assert v <= 4 * MEASURED_LOOP[k], (k, v)
    assert np.any(e["pos_out"][moved] != a["pos"][moved]) or np.any(e["tiw_out"] != a["tiw"])       # through the arithmetic, not around it


# ---- the argument rules ----------------------------------------------------------------------------------------------------------------
def bent(v, i, x):
    w = np.array(v).copy()
    w.ravel()[i] = x
    return w


def invalid_blobs():
    """(message, mode, blob, k_out, p_out) for every rule of the two calls."""
    out = []
    a = LC.loop_scene("two_keyframes")["args"]
    K, P = a["n_kf"], a["n_points"]
    held = int(np.flatnonzero((a["slot_point"] >= 0) & (a["skip"][np.maximum(a["slot_point"], 0)] == 0))[0])
    moved_point = int(a["slot_point"][held])
    cases = [
        ("negative count", dict(n_kf=-1)), ("negative count", dict(n_all=-1)), ("negative count", dict(n_points=-1)),
        ("n_kf must be at least 1", dict(n_kf=0)), ("n_all is smaller than n_kf", dict(n_all=K - 1)),
        ("cur outside 0 .. n_kf - 1", dict(cur=-1)), ("cur outside 0 .. n_kf - 1", dict(cur=K)),
        ("scw scale is not positive", dict(scw=bent(a["scw"], 7, 0.0))), ("scw scale is not positive", dict(scw=bent(a["scw"], 7, -1.0))),
        ("scw scale is not positive", dict(scw=bent(a["scw"], 7, np.nan))),
        ("slot_off does not start at 0", dict(slot_off=a["slot_off"] + 1)), ("slot_off decreases", dict(slot_off=bent(a["slot_off"], 1, a["slot_off"][2] + 1))),
        ("slot_point outside -1 .. n_points - 1", dict(slot_point=bent(a["slot_point"], 3, P))),
        ("slot_point outside -1 .. n_points - 1", dict(slot_point=bent(a["slot_point"], 3, -2))),
        ("obs_off does not start at 0", dict(obs_off=a["obs_off"] + 1)), ("obs_off decreases", dict(obs_off=bent(a["obs_off"], 2, a["obs_off"][3] + 1))),
        ("obs_kf outside 0 .. n_all - 1", dict(obs_kf=bent(a["obs_kf"], 1, a["n_all"]))), ("obs_kf outside 0 .. n_all - 1", dict(obs_kf=bent(a["obs_kf"], 1, -1))),
        ("ref_kf outside -1 .. n_all - 1", dict(ref_kf=bent(a["ref_kf"], 0, a["n_all"]))), ("ref_kf outside -1 .. n_all - 1", dict(ref_kf=bent(a["ref_kf"], 0, -2))),
        ("a point that would be moved has no reference keyframe", dict(ref_kf=bent(a["ref_kf"], moved_point, -1))),
    ]
    for what, change in cases:
        out.append((what, "loop", LC.loop_blob(dict(a, **change), k_out=K, p_out=P), K, P))
    nulls = [("null keyframe array", n) for n in ("tiw", "twc_cur", "scw", "ow")]
    nulls += [("null keyframe output", n) for n in ("noncorrected_siw", "corrected_siw", "tiw_out", "ow_out")]
    nulls += [("null slot_off", "slot_off"), ("null slot_point", "slot_point"), ("null obs_off", "obs_off"), ("null obs_kf", "obs_kf")]
    nulls += [("null point array", n) for n in ("pos", "skip", "ref_kf", "level_scale", "last_scale")]
    nulls += [("null point output", n) for n in ("corrected_by", "pos_out", "normal", "max_dist", "min_dist", "flags")]
    for what, name in nulls:
        out.append((what, "loop", LC.loop_blob(a, null=(name,)), K, P))
    out.append(("null problem", "loop", LC.loop_blob(a, null_problem=True), K, P))

    t = LC.tree_scene("run_2")["args"]
    K, P = t["n_kf"], t["n_points"]
    carried = int(np.flatnonzero((t["point_bad"] == 0) & (t["point_in_gba"] == 0))[0])

    def children(lists):
        off = np.zeros(len(lists) + 1, np.int64)
        np.cumsum([len(c) for c in lists], out=off[1:])
        return dict(child_off=off, child_kf=np.array([c for row in lists for c in row], np.int32))

    lists = [list(t["child_kf"][t["child_off"][k]:t["child_off"][k + 1]]) for k in range(K)]

    def with_child(parent, child):
        rows = [list(r) for r in lists]
        rows[parent].append(child)
        return children(rows)

    leaf = next(k for k in range(K) if not lists[k])
    first_child = lists[0][0]
    cases = [
        ("negative count", dict(n_kf=-1)), ("negative count", dict(n_origins=-1)), ("negative count", dict(n_points=-1)),
        ("origin outside 0 .. n_kf - 1", dict(origin=np.array([K], np.int32))), ("origin outside 0 .. n_kf - 1", dict(origin=np.array([-1], np.int32))),
        ("child_off does not start at 0", dict(child_off=t["child_off"] + 1)), ("child_off decreases", dict(child_off=bent(t["child_off"], 1, t["child_off"][2] + 1))),
        ("child_kf outside 0 .. n_kf - 1", dict(child_kf=bent(t["child_kf"], 0, K))), ("child_kf outside 0 .. n_kf - 1", dict(child_kf=bent(t["child_kf"], 0, -1))),
        ("a keyframe is listed as a child more than once", with_child(leaf, first_child)),
        ("a keyframe is listed as a child more than once", with_child(0, first_child)),
        ("an origin is somebody's child", with_child(leaf, 0)),
        ("an origin is listed more than once", dict(n_origins=2, origin=np.array([0, 0], np.int32))),
        ("ref_kf outside -1 .. n_kf - 1", dict(ref_kf=bent(t["ref_kf"], 0, K))), ("ref_kf outside -1 .. n_kf - 1", dict(ref_kf=bent(t["ref_kf"], 0, -2))),
        ("a point that would be carried has no reference keyframe", dict(ref_kf=bent(t["ref_kf"], carried, -1))),
    ]
    # cycles, none of them reachable from an origin: two keyframes that list each other, a ring of three, a keyframe that lists itself
    for ring in ((K, K + 1), (K, K + 1, K + 2), (K,)):
        n = K + len(ring)
        rows = [list(r) for r in lists] + [[ring[(j + 1) % len(ring)]] for j in range(len(ring))]
        grown = {k: np.concatenate([t[k], np.repeat(t[k][:1], len(ring), axis=0)]) for k in ("tcw", "tcw_gba", "tcw_bef", "in_gba")}
        cases.append(("the children form a cycle", dict(n_kf=n, **grown, **children(rows))))
    for what, change in cases:
        k = max(dict(t, **change)["n_kf"], K)
        out.append((what, "gba", LC.gba_blob(dict(t, **change), k_out=k, p_out=P), k, P))
    nulls = [("null origin", "origin"), ("null child_off", "child_off"), ("null child_kf", "child_kf")]
    nulls += [("null keyframe array", n) for n in ("tcw", "tcw_gba", "in_gba", "tcw_bef")] + [("null keyframe output", n) for n in ("tcw_out", "ow_out", "kf_reached")]
    nulls += [("null point array", n) for n in ("pos", "pos_gba", "point_in_gba", "point_bad", "ref_kf")] + [("null point output", n) for n in ("pos_out", "point_status")]
    for what, name in nulls:
        out.append((what, "gba", LC.gba_blob(t, null=(name,)), K, P))
    out.append(("null problem", "gba", LC.gba_blob(t, null_problem=True), K, P))
    return out


def test_every_argument_rule_has_its_message_and_writes_nothing(prog, tmp_path):
    seen = set()
    for what, mode, blob, k, p in invalid_blobs():
        fields = LC.LOOP_OUT if mode == "loop" else LC.GBA_OUT
        rc, text, got = LC.parse(host_prog.run(prog, tmp_path, mode, blob), fields, k, p)
        assert rc == 1 and text == ("sivo_loop_correct: " if mode == "loop" else "sivo_gba_propagate: ") + what, (what, text)
        for name, *_ in fields:
            if name in ("tcw_gba", "in_gba", "tcw_bef"):
                continue
            assert np.all(got[name] == (255 if got[name].dtype == np.uint8 else -7)), (what, name)
        seen.add((mode, what))
    assert len(seen) >= 40
    # what the rules leave alone: ref_kf = -1 for a point no slot would move, for a bad point and for a point the BA holds
    a = LC.loop_scene("two_keyframes")["args"]
    unheld = [p for p in range(a["n_points"]) if p not in a["slot_point"] or a["skip"][p]]
    assert len(unheld) >= 2
    rc, text, got = run_loop(prog, tmp_path, dict(a, ref_kf=bent(bent(a["ref_kf"], unheld[0], -1), unheld[1], -1)))
    assert rc == 0 and LC.same_bytes(got, LC.loop_scene("two_keyframes")["expect"]) == []
    t = LC.tree_scene("bad_point")
    free = np.flatnonzero((t["args"]["point_bad"] == 1) | (t["args"]["point_in_gba"] == 1))
    ref = t["args"]["ref_kf"].copy()
    ref[free] = -1
    rc, text, got = run_gba(prog, tmp_path, dict(t["args"], ref_kf=ref))
    assert rc == 0 and LC.same_bytes(got, t["expect"]) == []
    # no keyframe and no point: nothing to do
    empty = {n: np.zeros(0, dt) for n, dt in LC.GBA_IN}
    rc, text, got = run_gba(prog, tmp_path, dict(empty, n_kf=0, n_origins=0, n_points=0, child_off=np.zeros(1, np.int64)))
    assert rc == 0


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_structs_prototypes_and_signatures(tmp_path):
    from sivo_amd import _lib, loop_closing
    header = open(os.path.join(ROOT, "include", "sivo_hip.h")).read()
    assert re.search(r"int sivo_loop_correct\(const SivoLoopCorrect \*problem\);", header)
    assert re.search(r"int sivo_gba_propagate\(const SivoGbaPropagate \*problem\);", header)
    for name in ("SIVO_GBA_POINT_BAD = 0", "SIVO_GBA_POINT_FROM_BA = 1", "SIVO_GBA_POINT_CARRIED = 2", "SIVO_GBA_POINT_REF_OUTSIDE = 3"):
        assert name in header
    host_prog.c_layout(tmp_path, "SivoLoopCorrect", loop_closing.LoopCorrect)
    host_prog.c_layout(tmp_path, "SivoGbaPropagate", loop_closing.GbaPropagate)
    assert [f[0] for f in loop_closing.LoopCorrect._fields_][4:] == LC.LOOP_POINTERS
    assert [f[0] for f in loop_closing.GbaPropagate._fields_][3:] == LC.GBA_POINTERS
    assert _lib.SIGNATURES["sivo_loop_correct"] == [C.c_void_p] and _lib.SIGNATURES["sivo_gba_propagate"] == [C.c_void_p]
    assert loop_closing.POINT_STATUS == ("bad", "from_ba", "carried", "reference_outside") and loop_closing.NO_OBSERVATION == LR.NO_OBSERVATION
    makefile = open(os.path.join(ROOT, "sivo_amd", "csrc", "Makefile")).read()
    assert " loopcorrect.hip " in makefile


def test_library_checks_arguments_first_and_fails_loudly_without_a_device():
    """The library runs the same checks before it touches a device — this test runs where there is none — and real work without a
    device is SIVO_ERR_RUNTIME, never a silent fallback."""
    from sivo_amd import _lib, loop_closing as lc
    L = _lib.lib()
    a = LC.loop_scene("two_keyframes")["args"]
    call = lambda **kw: lc.correct_loop(*[dict(a, **kw)[n] for n in ("tiw", "cur", "twc_cur", "scw", "ow", "slot_off", "slot_point", "pos", "skip",
                                                                      "obs_off", "obs_kf", "ref_kf", "level_scale", "last_scale")])
    for what, kw in (("cur outside", dict(cur=2)), ("scw scale is not positive", dict(scw=bent(a["scw"], 7, 0.0))),
                     ("slot_off decreases", dict(slot_off=bent(a["slot_off"], 1, a["slot_off"][2] + 1))),
                     ("obs_kf outside", dict(obs_kf=bent(a["obs_kf"], 0, a["n_all"]))), ("slot_point outside", dict(slot_point=bent(a["slot_point"], 0, -2)))):
        with pytest.raises(ValueError, match=what):
            call(**kw)
    t = LC.tree_scene("run_2")["args"]
    names = ("origin", "child_off", "child_kf", "tcw", "tcw_gba", "in_gba", "tcw_bef", "pos", "pos_gba", "point_in_gba", "point_bad", "ref_kf")
    tcall = lambda **kw: lc.propagate_global_ba(*[dict(t, **kw)[n] for n in names])
    ring = bent(t["child_kf"], 0, 0)                        # the origin as its own child: an origin that is somebody's child
    for what, kw in (("an origin is somebody's child", dict(child_kf=ring)), ("origin outside", dict(origin=[t["n_kf"]])),
                     ("an origin is listed more than once", dict(origin=[0, 0])), ("ref_kf outside", dict(ref_kf=bent(t["ref_kf"], 0, t["n_kf"])))):
        with pytest.raises(ValueError, match=what):
            tcall(**kw)
    assert L.sivo_loop_correct(None) == _lib.ERR_INVALID_ARGUMENT and b"null problem" in L.sivo_last_error()
    assert L.sivo_gba_propagate(None) == _lib.ERR_INVALID_ARGUMENT and b"null problem" in L.sivo_last_error()
    empty = lc.GbaPropagate()
    assert L.sivo_gba_propagate(C.byref(empty)) == 0        # no keyframe and no point: no device needed
    if L.sivo_device_count() < 1:
        with pytest.raises(RuntimeError, match="no HIP device"):
            call()
        with pytest.raises(RuntimeError, match="no HIP device"):
            tcall()
        keep = [np.ascontiguousarray(a[n], dt).ravel() for n, dt in LC.LOOP_IN]
        outs = [np.zeros(per * (a["n_kf"] if which == "k" else a["n_points"]), dt) for _, dt, per, which in LC.LOOP_OUT]
        s = lc.LoopCorrect(a["n_kf"], a["cur"], a["n_all"], a["n_points"], *[v.ctypes.data for v in keep], *[v.ctypes.data for v in outs])
        assert L.sivo_loop_correct(C.byref(s)) == _lib.ERR_RUNTIME
