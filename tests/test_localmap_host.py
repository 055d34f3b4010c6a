"""The tracking thread's local map (sivo_amd/csrc/localmap_math.hpp, the sivo_localmap_* C ABI of include/sivo_hip.h and
sivo_amd/api/orbslam/LocalMapAdapter.h) against a line-by-line restatement of the reference on an object graph
(tests/localmap_restatement.py), without a device: the per-item bodies the kernels run are compiled for the host into two stand-alone
programs (tests/localmap_prog.cpp for the C ABI, tests/localmap_adapter_prog.cpp for the adapter over stand-in SLAM types), plain and with
-fsanitize=address,undefined.  Every output is an integer and must be equal.  Scenes: tests/localmap_cases.py."""
import ctypes as C
import os

import numpy as np
import pytest

import host_prog
import localmap_cases as P
import localmap_restatement as R

ROOT = host_prog.ROOT
INVALID, CAPACITY = 1, 5                                            # SIVO_ERR_INVALID_ARGUMENT, SIVO_ERR_CAPACITY


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return host_prog.build("localmap_prog", tmp_path_factory.mktemp("localmap_prog"))


@pytest.fixture(scope="module")
def adapter_prog(tmp_path_factory):
    return host_prog.build("localmap_adapter_prog", tmp_path_factory.mktemp("localmap_adapter_prog"))


# ---- the C ABI on the host build ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.CASES))
def test_host_build_equals_the_restatement(prog, tmp_path, name):
    """Every output, in sentinel-filled arrays: local_kf keeps the sentinel where nobody voted, and everything past the counts does."""
    tables, call, want, _ = P.arrays(name)
    got = P.host_update(prog, tmp_path, tables, call)
    assert got["rc"] == 0 and P.same(got, want) == []
    assert (want["local_point"][want["n_local_points"]:] == P.SENTINEL).all() and len(want["local_point"]) >= want["n_local_points"] + 2
    if not want["voted"]:
        assert (got["local_kf"] == P.SENTINEL).all() and got["n_local_kf"] == P.SENTINEL and got["ref_kf"] == -1


def test_scenes_show_what_they_are_named_for():
    w = lambda name: P.arrays(name)[2]
    kfs = lambda name: w(name)["local_kf"][:w(name)["n_local_kf"]].tolist()
    pts = lambda name: w(name)["local_point"][:w(name)["n_local_points"]].tolist()
    assert kfs("three_kfs_all_voted") == [0, 1, 2] and w("three_kfs_all_voted")["ref_kf"] == 1
    assert kfs("bad_voted_highest") == [0, 2] and w("bad_voted_highest")["ref_kf"] == 2 and w("bad_voted_highest")["counts"].tolist() == [2, 5, 3]
    assert kfs("tie_order") == [1, 3, 2, 0] and w("tie_order")["ref_kf"] == 2 and w("tie_order")["counts"].tolist() == [3, 1, 3, 2]
    assert kfs("covis_eleventh") == [0, 6, 7]                       # 11 is not taken
    assert kfs("bad_child_first") == [0, 2] and kfs("bad_parent_taken") == [0, 1] and 2 in pts("bad_parent_taken")
    assert kfs("parent_stops") == [0, 1, 2, 3, 5, 4]                # nothing of keyframe 2
    assert kfs("stage2_mark_seen") == [0, 1, 2, 3, 4]
    assert kfs("stage1_80") == list(range(80)) + [80, 81] and kfs("stage1_81") == list(range(81))
    assert kfs("stage1_79") == list(range(79)) + [79, 80, 81, 82]
    assert kfs("children_70") == [0, 65]
    e = w("empty_vote_prev")
    assert (e["voted"], e["ref_kf"]) == (0, -1) and pts("empty_vote_prev") == [0, 2, 1]             # keyframe 2's slots, then keyframe 0's
    b = w("empty_vote_bad_frame_point")
    assert b["voted"] == 0 and b["slot_cleared"].tolist() == [0, 1] and pts("empty_vote_bad_frame_point") == [1]
    a = w("all_voted_bad")
    assert (a["voted"], a["n_local_kf"], a["ref_kf"], a["n_local_points"]) == (1, 0, -1, 0)
    f = w("frame_bad_point")
    assert f["slot_cleared"].tolist() == [1, 0, 0, 1] and f["counts"].tolist() == [1, 0] and kfs("frame_bad_point") == [0]
    assert kfs("premarked") == [0, 3, 2] and 1 not in pts("premarked")
    assert kfs("duplicate_points") == [2, 1, 0] and pts("duplicate_points") == [0, 1, 2, 3]
    for total in (255, 256, 257, 258, 769):
        t, _, want, _ = P.arrays("blocks_%d" % total)
        assert int(t["slot_off"][-1]) == total
        seq = t["slot_point"]
        for edge in range(256, total - 1, 256):                     # the pair across every boundary that has a slot behind it
            assert seq[edge - 1] == seq[edge] >= 0 and not t["point_bad"][seq[edge]]
        last = int(seq[-1])
        assert last >= 0 and (seq[:-1] != last).all() and pts("blocks_%d" % total)[-1] == last      # first met in the very last slot
        assert (seq == -1).any() and t["point_bad"].any() and len(np.unique(seq[seq >= 0])) < (seq >= 0).sum()
    z = P.arrays("zero_slot_keyframe")
    assert np.diff(z[0]["slot_off"]).tolist() == [1, 0, 2] and kfs("zero_slot_keyframe") == [0, 1, 2]
    assert P.arrays("n_kf_1")[0]["n_kf"] == 1 and kfs("n_kf_1") == [0]
    big = P.arrays("lds_plus_1")
    assert big[0]["n_kf"] == P.LDS_KF + 1 and kfs("lds_plus_1") == [P.LDS_KF, 4000, 5, 7000, 8000, 1] and big[2]["ref_kf"] == P.LDS_KF
    r = P.arrays("random_40x60")
    assert r[0]["n_kf"] == 40 and int(r[0]["slot_off"][-1]) == 2400 and r[0]["kf_order"] is not None and r[2]["slot_cleared"].any()
    assert max(int(P.arrays(n)[0]["slot_off"][-1]) for n in P.CASES) < 4000


def bent(x, i, v):
    y = np.array(x).copy(); y[i] = v
    return y


def invalid_tables():
    """(the message, the tables bent once, n_points where it is not the length of point_bad): one per rule of the header."""
    t = P.arrays("random_40x60")[0]
    K, Pn = t["n_kf"], len(t["point_bad"])
    out = []
    for f, inner, lo in (("obs", "obs_kf", 0), ("slot", "slot_point", -1), ("covis", "covis_kf", 0), ("child", "child_kf", 0)):
        off = t[f + "_off"]
        out += [("%s_off does not start at 0" % f, dict(t, **{f + "_off": bent(off, 0, 1)}), None),
                ("%s_off decreases" % f, dict(t, **{f + "_off": bent(off, 3, int(off[4]) + 1)}), None),
                ("null %s_off" % f, dict(t, **{f + "_off": None}), Pn),
                ("null " + inner, dict(t, **{inner: None}), None),
                (inner + " outside", dict(t, **{inner: bent(t[inner], 5, Pn if inner == "slot_point" else K)}), None),
                (inner + " outside", dict(t, **{inner: bent(t[inner], 5, lo - 1)}), None)]
    out += [("parent outside", dict(t, parent=bent(t["parent"], 2, K)), None), ("parent outside", dict(t, parent=bent(t["parent"], 2, -2)), None),
            ("null parent", dict(t, parent=None), None), ("null kf_bad", dict(t, kf_bad=None), None), ("null point_bad", dict(t, point_bad=None), Pn),
            ("kf_order is not a permutation", dict(t, kf_order=bent(t["kf_order"], 1, int(t["kf_order"][0]))), None),
            ("kf_order is not a permutation", dict(t, kf_order=bent(t["kf_order"], 1, K)), None),
            ("kf_order is not a permutation", dict(t, kf_order=bent(t["kf_order"], 1, -1)), None),
            ("negative count", dict(t, n_kf=-1), None), ("negative count", t, -1)]
    return out


def test_host_build_reports_every_invalid_argument(prog, tmp_path):
    tables, call, want, _ = P.arrays("random_40x60")
    K, Pn = tables["n_kf"], len(tables["point_bad"])
    for what, t, n_points in invalid_tables():
        for op in (P.op_create, P.op_replace):
            res = P.run_ops(prog, tmp_path, [P.op_create(tables), op(t, n_points=n_points)])[1]
            assert res["rc"] == INVALID and what in res["message"], (what, res)
    upd = lambda **kw: P.run_ops(prog, tmp_path, [P.op_create(tables), P.op_update(call, K, **kw)])[1]
    fp, kp, pp, prev = call["frame_point"], call["kf_premarked"], call["point_premarked"], call["prev_local_kf"]
    for what, kw in [("frame_point outside", dict(frame_point=bent(fp, 0, Pn))), ("frame_point outside", dict(frame_point=bent(fp, 0, -2))),
                     ("kf_premarked outside", dict(kf_premarked=bent(kp, 0, K))), ("kf_premarked outside", dict(kf_premarked=bent(kp, 0, -1))),
                     ("point_premarked outside", dict(point_premarked=bent(pp, 0, Pn))), ("point_premarked outside", dict(point_premarked=bent(pp, 0, -1))),
                     ("prev_local_kf outside", dict(prev_local_kf=bent(prev, 1, K))), ("prev_local_kf outside", dict(prev_local_kf=bent(prev, 1, -1))),
                     ("null frame_point", dict(frame_point=None, n_slots=len(fp))), ("null kf_premarked", dict(kf_premarked=None, n_kf_premarked=1)),
                     ("null point_premarked", dict(point_premarked=None, n_point_premarked=1)), ("null prev_local_kf", dict(prev_local_kf=None, n_prev=2)),
                     ("negative count", dict(n_slots=-1)), ("negative count", dict(n_kf_premarked=-1)), ("negative count", dict(n_point_premarked=-1)),
                     ("negative count", dict(n_prev=-1)), ("negative count", dict(kf_capacity=-1)), ("negative count", dict(point_capacity=-1)),
                     ("null result", dict(null_mask=1)), ("null slot_cleared", dict(null_mask=2)), ("null local_kf", dict(null_mask=4)),
                     ("null local_point", dict(null_mask=8))]:
        res = upd(**kw)
        assert res["rc"] == INVALID and what in res["message"] and res["message"].startswith("sivo_localmap_update: "), (what, res)
        assert res["voted"] == res["n_local_points"] == P.SENTINEL and (res["local_point"] == P.SENTINEL).all()
    sb = lambda **kw: P.run_ops(prog, tmp_path, [P.op_create(tables), P.op_set_bad(**kw)])[1]
    for what, kw in [("point_idx outside", dict(points=[Pn], point_values=[1])), ("point_idx outside", dict(points=[-1], point_values=[1])),
                     ("kf_idx outside", dict(kfs=[K], kf_values=[1])), ("kf_idx outside", dict(kfs=[-1], kf_values=[1])),
                     ("null point_idx", dict(points=None, point_values=[1], n_points=1)), ("null point_val", dict(points=[0], point_values=None)),
                     ("null kf_idx", dict(kfs=None, kf_values=[1], n_kf=1)), ("null kf_val", dict(kfs=[0], kf_values=None)),
                     ("negative count", dict(n_points=-1)), ("negative count", dict(n_kf=-1))]:
        res = sb(**kw)
        assert res["rc"] == INVALID and what in res["message"], (what, res)
    # a handle that was never made
    res = P.run_ops(prog, tmp_path, [P.op_replace(tables), P.op_set_bad(points=[0], point_values=[1]), P.op_update(call, 0)])
    assert [r["rc"] for r in res] == [INVALID] * 3 and all("null handle" in r["message"] for r in res)
    # one too small a capacity: SIVO_ERR_CAPACITY and nothing written; exactly enough is enough
    for kw, text in [(dict(kf_capacity=want["n_local_kf"] - 1), "%d local keyframes, capacity %d" % (want["n_local_kf"], want["n_local_kf"] - 1)),
                     (dict(point_capacity=want["n_local_points"] - 1), "%d local map points, capacity %d" % (want["n_local_points"], want["n_local_points"] - 1))]:
        res = upd(**kw)
        assert res["rc"] == CAPACITY and text in res["message"]
        assert res["voted"] == res["ref_kf"] == P.SENTINEL and (res["slot_cleared"] == 255).all()
        assert all((res[k] == P.SENTINEL).all() for k in ("local_kf", "local_point", "counts"))
    res = upd(kf_capacity=want["n_local_kf"], point_capacity=want["n_local_points"])
    assert res["rc"] == 0 and res["local_kf"].tobytes() == want["local_kf"][:want["n_local_kf"]].tobytes()
    assert res["local_point"].tobytes() == want["local_point"][:want["n_local_points"]].tobytes()


def test_host_handle_replace_set_bad_and_repeated_updates(prog, tmp_path):
    """What the GPU file asks of the resident handle, on the host build: replace gives the new tables' results, set_bad equals tables made
    with those flags (of an index listed twice the later entry holds), and an update leaves nothing behind for the next."""
    ta, ca, wa, _ = P.arrays("random_40x60")
    tb, cb, wb, _ = P.arrays("premarked")
    flagged = dict(ta, point_bad=ta["point_bad"].copy(), kf_bad=ta["kf_bad"].copy())
    flagged["point_bad"][[40, 3]] = [1, 0]
    flagged["kf_bad"][[16, 31]] = 1
    res = P.run_ops(prog, tmp_path, [P.op_create(ta), P.op_update(ca, ta["n_kf"]), P.op_update(ca, ta["n_kf"]), P.op_replace(tb), P.op_update(cb, tb["n_kf"]),
                                     P.op_replace(ta), P.op_set_bad([3, 40, 3], [1, 1, 0], [16, 31], [1, 1]), P.op_update(ca, ta["n_kf"])])
    assert [r["rc"] for r in res] == [0] * 8
    assert P.same(res[1], wa) == [] and P.same(res[2], wa) == [] and P.same(res[4], wb) == []
    assert P.same(res[7], P.host_update(prog, tmp_path, flagged, ca)) == [] and P.same(res[7], wa) != []


# ---- the library itself, where there may be no device ----------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    h = open(os.path.join(ROOT, "include", "sivo_hip.h")).read()
    names = ("sivo_localmap_create", "sivo_localmap_replace", "sivo_localmap_set_bad", "sivo_localmap_destroy", "sivo_localmap_update")
    for n in names:
        assert "int %s(" % n in h
    for cite in ("Tracking.cc:1087-1235", "Tracking.cc:1092-1093", "KeyFrame.cc:222-230", ":1156-1172", ":1222-1228", ":1138-1140"):
        assert cite in h, cite
    from sivo_amd import _lib, local_map
    L = _lib.lib()
    assert all(hasattr(L, n) for n in names) and set(names) <= set(_lib.SIGNATURES) and local_map.LDS_KF == P.LDS_KF
    mk = open(os.path.join(ROOT, "sivo_amd", "csrc", "Makefile")).read()
    assert " localmap.hip " in mk.split("SRCS =")[1].splitlines()[0]


def test_ctypes_tables_match_the_header(tmp_path):
    from sivo_amd import local_map
    host_prog.c_layout(tmp_path, "SivoLocalMapTables", local_map._Tables)
    assert tuple(f for f, _ in local_map._Tables._fields_[2:]) == P.TABLES == local_map.TABLE_FIELDS


def test_library_checks_arguments_before_it_needs_a_device():
    """The library's own create reports every invalid table as such — a ValueError here — where there is no device; valid tables without
    a device are an error, never a silent fallback; a null handle is an invalid argument everywhere."""
    from sivo_amd import _lib, local_map
    tables = P.arrays("random_40x60")[0]
    for what, t, n_points in invalid_tables():
        if n_points is not None or t["n_kf"] < 0:
            continue                                                # (the Python layer takes n_points from point_bad; raw calls below)
        with pytest.raises(ValueError, match=what):
            local_map.LocalMap(t["n_kf"], **{k: v for k, v in t.items() if k != "n_kf"})
    L = _lib.lib()
    st = local_map._Tables(-1, 0)
    h = C.c_void_p()
    assert L.sivo_localmap_create(C.byref(st), C.byref(h)) == _lib.ERR_INVALID_ARGUMENT and b"negative count" in L.sivo_last_error() and not h
    st = local_map._Tables(0, 3)
    assert L.sivo_localmap_create(C.byref(st), C.byref(h)) == _lib.ERR_INVALID_ARGUMENT and b"null obs_off" in L.sivo_last_error()
    assert L.sivo_localmap_create(None, C.byref(h)) == _lib.ERR_INVALID_ARGUMENT and b"null tables" in L.sivo_last_error()
    assert L.sivo_localmap_create(C.byref(st), None) == _lib.ERR_INVALID_ARGUMENT and b"null handle pointer" in L.sivo_last_error()
    v = C.c_int32()
    assert L.sivo_localmap_update(None, 0, None, 0, None, 0, None, 0, None, C.byref(v), None, 0, None, C.byref(v), C.byref(v), 0, None, C.byref(v),
                                  None) == _lib.ERR_INVALID_ARGUMENT and b"null handle" in L.sivo_last_error()
    assert L.sivo_localmap_replace(None, C.byref(st)) == _lib.ERR_INVALID_ARGUMENT and L.sivo_localmap_set_bad(None, 0, None, None, 0, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert L.sivo_localmap_destroy(None) == 0
    if L.sivo_device_count() < 1:
        with pytest.raises(RuntimeError, match="no HIP device"):
            local_map.LocalMap(tables["n_kf"], **{k: v for k, v in tables.items() if k != "n_kf"})


# ---- the adapter ---------------------------------------------------------------------------------------------------------------------
def run_adapter(exe, tmp_path, name, unknown_slot=-1, bad_kfs=(), bad_points=()):
    """The adapter program on a scene, and the restatement's graph after the same call (with the late flags set from the start)."""
    sc = P.CASES[name]()
    tables, call = R.export_tables(sc), R.export_call(sc)
    ref = -1 if sc.reference is None else sc.kfs.index(sc.reference)
    raw = host_prog.run(exe, tmp_path, "update", P.adapter_blob(tables, call, sc.frame.mnId, ref, unknown_slot, bad_kfs, bad_points))
    for k in bad_kfs:
        sc.kfs[k].mbBad = True
    for p in bad_points:
        sc.points[p].mbBad = True
    t = R.run(sc)
    return P.parse_adapter(raw, len(call["frame_point"]), tables["n_kf"], len(tables["point_bad"])), P.graph_after(sc, t)


@pytest.mark.parametrize("name", list(P.CASES))
def test_adapter_leaves_the_reference_graph(adapter_prog, tmp_path, name):
    """Both vectors, every mnTrackReferenceForFrame, the reference keyframe of the tracker and of the frame, the frame's slots — from
    ONE call of sivo_localmap_update."""
    got, want = run_adapter(adapter_prog, tmp_path, name)
    assert got == want


def test_adapter_mark_bad_then_update(adapter_prog, tmp_path):
    plain, _ = run_adapter(adapter_prog, tmp_path, "random_40x60")
    got, want = run_adapter(adapter_prog, tmp_path, "random_40x60", bad_kfs=[16, 31], bad_points=[40])
    assert got == want and got["local_kf"] != plain["local_kf"] and 40 not in got["local_points"]


def test_adapter_refuses_a_point_made_after_rebuild(adapter_prog, tmp_path):
    got, _ = run_adapter(adapter_prog, tmp_path, "three_kfs_all_voted", unknown_slot=2)
    assert got["error"] is not None and "frame slot 2" in got["error"] and "created after the last Rebuild" in got["error"]


# ---- the sanitizer build ----------------------------------------------------------------------------------------------------------------
def test_sanitizer_builds_of_both_programs_agree(prog, adapter_prog, tmp_path, tmp_path_factory):
    """Both stand-alone programs built a second time with -fsanitize=address,undefined and run directly (each has its own main: nothing
    is preloaded) over all scenes: the same bytes as the plain build, and no report."""
    san_dir = tmp_path_factory.mktemp("localmap_prog_san")
    if not host_prog.sanitizer_runtime_present(san_dir):
        pytest.skip("the sanitizer runtime (libasan / libubsan) is not installed: a trivial main does not link with -fsanitize")
    san = host_prog.build("localmap_prog", san_dir, sanitize=True)
    asan = host_prog.build("localmap_adapter_prog", san_dir, sanitize=True)
    for name in P.CASES:
        sc = P.CASES[name]()
        tables, call = R.export_tables(sc), R.export_call(sc)
        call["kf_capacity"], call["point_capacity"] = tables["n_kf"] + 2, len(tables["point_bad"]) + 2
        blob = b"".join(o[1] for o in (P.op_create(tables), P.op_update(call, tables["n_kf"]), P.op_set_bad([0], [1], [0], [1]),
                                       P.op_update(call, tables["n_kf"]), P.op_replace(tables), P.op_update(call, tables["n_kf"]))) + P.i32(0)
        assert host_prog.run(prog, tmp_path, "run", blob) == host_prog.run(san, tmp_path, "run", blob), name
        ref = -1 if sc.reference is None else sc.kfs.index(sc.reference)
        blob = P.adapter_blob(tables, call, sc.frame.mnId, ref)
        assert host_prog.run(adapter_prog, tmp_path, "update", blob) == host_prog.run(asan, tmp_path, "update", blob), name
    tables, call = (lambda sc: (R.export_tables(sc), R.export_call(sc)))(P.CASES["three_kfs_all_voted"]())
    blob = P.adapter_blob(tables, call, 7, -1, 2)                   # the refused call unwinds cleanly too
    assert host_prog.run(adapter_prog, tmp_path, "update", blob) == host_prog.run(asan, tmp_path, "update", blob)
