"""sivo_localmap_apply / _sizes / _export (sivo_amd/csrc/localmap_delta_math.hpp, include/sivo_hip.h) and LocalMapDevice::Touch / Sync
(sivo_amd/api/orbslam/LocalMapAdapter.h) without a device: the per-item bodies the kernels run are compiled for the host into two
stand-alone programs (tests/localmap_delta_prog.cpp for the C ABI, tests/localmap_delta_adapter_prog.cpp for the adapter over stand-in SLAM
types), plain and with -fsanitize=address,undefined.  The yardsticks are the list-of-rows restatement of apply
(tests/localmap_delta_restatement.py) and Tracking::UpdateLocalMap restated on the edited object graph (tests/localmap_restatement.py).
Every comparison is an equality of bytes.  Scenes: tests/localmap_delta_cases.py."""
import ctypes as C
import os

import numpy as np
import pytest

import host_prog
import localmap_cases as P
import localmap_delta_cases as Q
import localmap_delta_restatement as D

ROOT = host_prog.ROOT
INVALID = 1                                                         # SIVO_ERR_INVALID_ARGUMENT
NAMES = ("sivo_localmap_apply", "sivo_localmap_sizes", "sivo_localmap_export")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return host_prog.build("localmap_delta_prog", tmp_path_factory.mktemp("localmap_delta_prog"))


@pytest.fixture(scope="module")
def adapter_prog(tmp_path_factory):
    return host_prog.build("localmap_delta_adapter_prog", tmp_path_factory.mktemp("localmap_delta_adapter_prog"))


def scene_ops(name):
    """create(before), apply(delta), export, update — then the same update on a handle created from the restatement's tables."""
    before, delta, after, call, want, _ = Q.arrays(name)
    return [P.op_create(before), Q.op_apply(delta), Q.op_export(), P.op_update(call, after["n_kf"]), P.op_create(after), Q.op_export(),
            P.op_update(call, after["n_kf"])]


# ---- the C ABI on the host build ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Q.CASES))
def test_host_build_equals_the_restatements(prog, tmp_path, name):
    """The export after apply is the list-of-rows restatement byte for byte (and what a handle created from those tables exports); an
    update on the applied handle equals one on the created handle, and both equal the reference restated on the edited graph."""
    before, delta, after, call, want, _ = Q.arrays(name)
    res = Q.run_ops(prog, tmp_path, scene_ops(name))
    assert [r["rc"] for r in res] == [0] * 7, [r["message"] for r in res]
    sizes = (after["n_kf"], len(after["point_bad"]), len(after["obs_kf"]), len(after["slot_point"]), len(after["covis_kf"]), len(after["child_kf"]))
    assert res[2]["sizes"] == sizes == res[5]["sizes"]
    assert Q.differing(res[2]["tables"], after) == [] and Q.differing(res[5]["tables"], after) == []
    assert P.same(res[3], res[6]) == [] and P.same(res[3], want) == []


def test_scenes_show_what_they_are_named_for():
    A = {n: Q.arrays(n) for n in Q.CASES}
    rows = lambda n: (len(A[n][1]["point_rows"]["idx"]), len(A[n][1]["kf_rows"]["idx"]))
    grew = lambda n: (A[n][1]["n_kf"] - A[n][0]["n_kf"], A[n][1]["n_points"] - len(A[n][0]["point_bad"]))
    d = A["empty_delta"][1]
    assert rows("empty_delta") == (0, 0) == grew("empty_delta") and d["kf_order"] is None
    assert A["everything_appended"][0]["n_kf"] == 0 == len(A["everything_appended"][0]["point_bad"]) and grew("everything_appended") == (5, 30)
    assert rows("points_only") == (9, 0) and grew("points_only") == (0, 9)
    assert rows("kfs_only")[0] == 0 and grew("kfs_only") == (3, 0)
    for n in ("first_and_last", "shrink_and_grow"):
        assert grew(n) == (0, 0)
    b, d, a = A["first_and_last"][:3]
    assert {0, len(a["point_bad"]) - 1} == set(d["point_rows"]["idx"].tolist()) and {0, a["n_kf"] - 1} <= set(d["kf_rows"]["idx"].tolist())
    b, d, a = A["shrink_and_grow"][:3]
    for f in ("obs", "slot", "covis", "child"):
        change = np.diff(a[f + "_off"]) - np.diff(b[f + "_off"])
        assert (change < 0).any() and (change > 0).any() and ((np.diff(a[f + "_off"]) == 0) & (change < 0)).any(), f
    assert rows("all_rows") == (A["all_rows"][1]["n_points"], A["all_rows"][1]["n_kf"])
    for n in (255, 256, 257, 600):
        assert A["points_%d" % n][1]["n_points"] == n and grew("points_%d" % n) == (1, 7)
    b, d, a = A["long_rows"][:3]
    touched_p, touched_k = set(d["point_rows"]["idx"].tolist()), set(d["kf_rows"]["idx"].tolist())
    for f, touched in (("obs", touched_p), ("slot", touched_k), ("child", touched_k)):
        new_len, old_len = np.diff(a[f + "_off"]), np.diff(b[f + "_off"])
        assert {64, 65, 130} <= {int(new_len[i]) for i in touched if i < len(new_len)}, f                  # from the delta's pool
        assert any(old_len[i] > 64 for i in range(len(old_len)) if i not in touched), f                     # and from the old pool
    assert A["order_given"][1]["kf_order"] is not None and A["order_given"][2]["kf_order"].tolist() != list(range(A["order_given"][2]["n_kf"]))
    b, d, a = A["order_null_on_permuted"][:3]
    assert d["kf_order"] is None and b["kf_order"] is not None and a["kf_order"].tolist() == b["kf_order"].tolist() + [9, 10]
    for n, (before, delta, after, call, want, meta) in A.items():
        K0 = before["n_kf"]
        kfs = want["local_kf"][:want["n_local_kf"]].tolist()
        assert want["voted"] == 1 and want["n_local_points"] > 0
        if len(delta["kf_rows"]["idx"]):                            # stage 2 through a replaced covisibility row, to a keyframe without votes
            v, u = meta["stage2"]
            assert v in delta["kf_rows"]["idx"] and u in kfs and want["counts"][u] == 0 and after["covis_kf"][after["covis_off"][v]] == u
        if n not in ("empty_delta", "points_only", "kfs_only", "first_and_last", "shrink_and_grow"):       # the vote spans old and new
            assert (want["counts"][K0:] > 0).any() and (K0 == 0 or (want["counts"][:K0] > 0).any()), n
    assert max(len(A[n][2]["slot_point"]) for n in A) < 4000


def bent(x, i, v):
    y = np.array(x).copy(); y[i] = v
    return y


def refusals():
    """(the message, the delta bent once, counts passed beside it): one per rule of the header."""
    before, d, after = Q.arrays("points_257")[:3]
    K0, P0, K1, P1 = before["n_kf"], len(before["point_bad"]), d["n_kf"], d["n_points"]
    pr, kr = d["point_rows"], d["kf_rows"]
    pset = lambda **kw: dict(d, point_rows=dict(pr, **kw))
    kset = lambda **kw: dict(d, kf_rows=dict(kr, **kw))
    at = len(pr["idx"]) - (P1 - P0)                                 # the first appended point's place in the list
    unlisted = int(pr["idx"][at - 1]) + 1                           # an old index instead: the list stays strictly increasing
    assert unlisted < P0
    out = [("size is not sizeof(SivoLocalMapDelta)", d, dict(size=8)), ("size is not sizeof(SivoLocalMapDelta)", d, dict(size=1000)),
           ("n_kf is smaller than the handle's", d, dict(n_kf=K0 - 1)), ("n_points is smaller than the handle's", d, dict(n_points=P0 - 1)),
           ("negative count", d, dict(n_point_rows=-1)), ("negative count", d, dict(n_kf_rows=-1)),
           ("point_idx is not strictly increasing", pset(idx=bent(pr["idx"], 1, int(pr["idx"][0]))), {}),
           ("point_idx is not strictly increasing", pset(idx=bent(pr["idx"], 0, int(pr["idx"][1]) + 1)), {}),
           ("point_idx outside", pset(idx=bent(pr["idx"], -1, P1)), {}), ("point_idx outside", pset(idx=bent(pr["idx"], 0, -1)), {}),
           ("kf_idx is not strictly increasing", kset(idx=bent(kr["idx"], 1, int(kr["idx"][0]))), {}),
           ("kf_idx outside", kset(idx=bent(kr["idx"], -1, K1)), {}), ("kf_idx outside", kset(idx=bent(kr["idx"], 0, -1)), {}),
           # an appended row that is not listed: the first appended point replaced by an old index, one more point than listed, one more keyframe
           ("point_idx does not list every appended point", pset(idx=bent(pr["idx"], at, unlisted)), {}),
           ("point_idx does not list every appended point", d, dict(n_points=P1 + 1)),
           ("kf_idx does not list every appended keyframe", d, dict(n_kf=K1 + 1)),
           ("kf_order is not a permutation", dict(d, kf_order=bent(np.arange(K1), 1, 0)), {}),
           ("kf_order is not a permutation", dict(d, kf_order=bent(np.arange(K1), 1, K1)), {}),
           ("kf_order is not a permutation", dict(d, kf_order=bent(np.arange(K1), 1, -1)), {}),
           ("null point_idx", pset(idx=None), dict(n_point_rows=len(pr["idx"]))), ("null kf_idx", kset(idx=None), dict(n_kf_rows=len(kr["idx"]))),
           ("null point_bad", pset(bad=None), {}), ("null kf_bad", kset(bad=None), {}), ("null kf_parent", kset(parent=None), {}),
           ("kf_parent outside", kset(parent=bent(kr["parent"], 0, K1)), {}), ("kf_parent outside", kset(parent=bent(kr["parent"], 0, -2)), {})]
    for rows, setter, f, inner, lo, hi in ((pr, pset, "obs_off", "obs_kf", 0, K1), (kr, kset, "slot_off", "slot_point", -1, P1),
                                           (kr, kset, "covis_off", "covis_kf", 0, K1), (kr, kset, "child_off", "child_kf", 0, K1)):
        prefix = "point_" if rows is pr else "kf_"
        off = rows[f]
        out += [("%s%s does not start at 0" % (prefix, f), setter(**{f: bent(off, 0, 1)}), {}),
                ("%s%s decreases" % (prefix, f), setter(**{f: bent(off, 3, int(off[4]) + 1)}), {}),
                ("null %s%s" % (prefix, f), setter(**{f: None}), {}), ("null %s%s" % (prefix, inner), setter(**{inner: None}), {}),
                ("%s%s outside" % (prefix, inner), setter(**{inner: bent(rows[inner], 2, hi)}), {}),
                ("%s%s outside" % (prefix, inner), setter(**{inner: bent(rows[inner], 2, lo - 1)}), {})]
    return out


def test_host_build_refuses_every_invalid_delta_and_keeps_the_handle(prog, tmp_path):
    """Each refusal of the header gives SIVO_ERR_INVALID_ARGUMENT with a message that names the field, and the export before and after the
    refused delta is equal; a payload index may lie in the NEW ranges."""
    before, d, after, call, want, _ = Q.arrays("points_257")
    cases = refusals()
    ops = [P.op_create(before), Q.op_export()]
    for _, bad, counts in cases:
        ops += [Q.op_apply(bad, **counts), Q.op_export()]
    ops += [Q.op_apply(d), Q.op_export()]
    res = Q.run_ops(prog, tmp_path, ops)
    first = res[1]
    assert first["rc"] == 0 and Q.differing(first["tables"], before) == []
    for i, (what, _, _) in enumerate(cases):
        r, e = res[2 + 2 * i], res[3 + 2 * i]
        assert r["rc"] == INVALID and what in r["message"] and r["message"].startswith("sivo_localmap_apply: "), (what, r)
        assert e["rc"] == 0 and e["sizes"] == first["sizes"] and Q.differing(e["tables"], first["tables"]) == [], what
    assert res[-2]["rc"] == 0 and Q.differing(res[-1]["tables"], after) == []
    K0, K1 = before["n_kf"], d["n_kf"]
    assert (d["point_rows"]["obs_kf"] >= K0).any() and (d["kf_rows"]["slot_point"] >= len(before["point_bad"])).any()      # new indices in the payload
    # a handle that was never made, and an export into tables of other sizes
    res = Q.run_ops(prog, tmp_path, [Q.op_apply(d), Q.op_export()])
    assert res[0]["rc"] == INVALID and "null handle" in res[0]["message"] and res[1]["rc"] == INVALID and "null handle" in res[1]["message"]


def test_host_handle_chain_set_bad_and_replace(prog, tmp_path):
    """What the GPU file asks of the resident handle, on the host build: A -> apply B -> apply C equals a fresh handle on C; apply then
    set_bad equals tables with those flags; replace after apply gives the replaced tables; the empty delta leaves everything."""
    a, d1, b = Q.arrays("points_600")[:3]
    d2 = second_delta(b)
    c = D.apply(b, d2)
    flagged = dict(c, point_bad=c["point_bad"].copy(), kf_bad=c["kf_bad"].copy())
    flagged["point_bad"][[5, 599, 603]] = [1, 1, 1]
    flagged["kf_bad"][[2, 15]] = 1
    call = Q.arrays("points_600")[3]
    other = Q.arrays("order_given")[2]
    empty = Q.arrays("empty_delta")[1]
    ops = [P.op_create(a), Q.op_apply(d1), Q.op_apply(d2), Q.op_export(), P.op_update(call, c["n_kf"]),
           P.op_set_bad([5, 599, 603], [1, 1, 1], [2, 15], [1, 1]), Q.op_export(), P.op_update(call, c["n_kf"]),
           P.op_create(flagged), P.op_update(call, c["n_kf"]), P.op_create(c), P.op_update(call, c["n_kf"]),
           P.op_replace(other), Q.op_export(), Q.op_apply(dict(empty, n_kf=other["n_kf"], n_points=len(other["point_bad"]))), Q.op_export()]
    res = Q.run_ops(prog, tmp_path, ops)
    assert [r["rc"] for r in res] == [0] * len(ops), [r["message"] for r in res]
    assert Q.differing(res[3]["tables"], c) == [] and P.same(res[4], res[11]) == []
    assert Q.differing(res[6]["tables"], flagged) == [] and P.same(res[7], res[9]) == []
    assert Q.differing(res[13]["tables"], other) == [] and Q.differing(res[15]["tables"], other) == []


def second_delta(b):
    """A second keyframe insertion on the tables b: one keyframe, four points, two old rows of each kind replaced."""
    K, Pn = b["n_kf"], len(b["point_bad"])
    pr = dict(idx=np.array([1, 7] + list(range(Pn, Pn + 4)), np.int32), bad=np.array([1, 0, 0, 0, 1, 0], np.uint8))
    pr["obs_off"], pr["obs_kf"] = P.R.csr([[0, K], [], [K], [K, 3], [2, K], [K, 1, 0]], np.int32)
    kr = dict(idx=np.array([0, 4, K], np.int32), bad=np.array([0, 1, 0], np.uint8), parent=np.array([-1, K, 4], np.int32))
    kr["slot_off"], kr["slot_point"] = P.R.csr([[Pn, -1, 3], [], [Pn, Pn + 1, Pn + 2, Pn + 3, -1, 7]], np.int32)
    kr["covis_off"], kr["covis_kf"] = P.R.csr([[K, 1], [K], [0, 4, 2]], np.int32)
    kr["child_off"], kr["child_kf"] = P.R.csr([[1], [K, 5], []], np.int32)
    return dict(n_kf=K + 1, n_points=Pn + 4, point_rows=pr, kf_rows=kr, kf_order=None)


# ---- the library itself, where there may be no device ----------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    h = open(os.path.join(ROOT, "include", "sivo_hip.h")).read()
    for n in NAMES:
        assert "int %s(" % n in h
    assert "} SivoLocalMapDelta;" in h
    from sivo_amd import _lib, local_map
    L = _lib.lib()
    assert all(hasattr(L, n) for n in NAMES) and set(NAMES) <= set(_lib.SIGNATURES)
    assert all(hasattr(local_map.LocalMap, m) for m in ("apply", "sizes", "export"))


def test_ctypes_delta_matches_the_header(tmp_path):
    from sivo_amd import local_map
    host_prog.c_layout(tmp_path, "SivoLocalMapDelta", local_map._Delta)
    names = [f for f, _ in local_map._Delta._fields_]
    assert names[:4] == ["size", "n_kf", "n_points", "n_point_rows"] and names[-1] == "kf_order" and len(names) == 19


def test_library_refuses_before_it_needs_a_device():
    """A null handle is an invalid argument for the three entry points of the library itself, with or without a device."""
    from sivo_amd import _lib, local_map
    L = _lib.lib()
    d = local_map._Delta(C.sizeof(local_map._Delta), 0, 0, 0)
    out = (C.c_int64 * 6)()
    t = local_map._Tables(0, 0)
    assert L.sivo_localmap_apply(None, C.byref(d)) == _lib.ERR_INVALID_ARGUMENT and b"sivo_localmap_apply: null handle" in L.sivo_last_error()
    assert L.sivo_localmap_sizes(None, out) == _lib.ERR_INVALID_ARGUMENT and b"sivo_localmap_sizes: null handle" in L.sivo_last_error()
    assert L.sivo_localmap_export(None, C.byref(t)) == _lib.ERR_INVALID_ARGUMENT and b"sivo_localmap_export: null handle" in L.sivo_last_error()


# ---- the adapter ---------------------------------------------------------------------------------------------------------------------
STEPS = ("insert_keyframe", "fuse_point", "cull_keyframe", "erase_observation", "reorder_covisibles")


def parse_adapter(raw):
    status = int(np.frombuffer(raw, np.int32, 1)[0])
    if status:
        n = int(np.frombuffer(raw, np.int32, 1, 4)[0])
        return dict(error=raw[8:8 + n].decode())
    v = np.frombuffer(raw, np.int64, (len(raw) - 4) // 8, 4).tolist()
    out = dict(error=None, late_threw=v[0], late_message_ok=v[1], empty_sync_applies=v[2], steps=[])
    for i in range(len(STEPS)):
        s = v[3 + 6 * i:9 + 6 * i]
        out["steps"].append(dict(equal=s[0], applies=s[1], n_local_kf=s[2], n_local_points=s[3], n_kf=s[4], n_points=s[5]))
    return out


def adapter_blob(name="order_null_on_permuted"):
    before = Q.arrays(name)[0]
    return P.tables_blob(before)


def test_adapter_sync_equals_a_fresh_rebuild_after_every_edit(adapter_prog, tmp_path):
    """The script of graph edits (tests/localmap_delta_adapter_prog.cpp) with the right Touch calls and one Sync per step: after each,
    UpdateLocalMap through the synced device leaves what it leaves through a second device freshly Rebuilt over the same graph — compared
    on pointers inside the program; exactly one apply per non-empty Sync and none for an empty one; the frame that holds a just-created
    point throws before Sync and works after."""
    got = parse_adapter(host_prog.run(adapter_prog, tmp_path, "script", adapter_blob()))
    assert got["error"] is None, got["error"]
    assert got["late_threw"] == 1 and got["late_message_ok"] == 1 and got["empty_sync_applies"] == 0
    for i, s in enumerate(got["steps"]):
        assert s["equal"] == 1 and s["applies"] == i + 1 and s["n_local_kf"] > 1 and s["n_local_points"] > 0, (STEPS[i], s)
    # one keyframe and four points appended by the first step; the fused point and the culled keyframe keep their rows
    assert all((s["n_kf"], s["n_points"]) == (10, 34) for s in got["steps"])


# ---- the sanitizer build ----------------------------------------------------------------------------------------------------------------
def test_sanitizer_builds_of_both_programs_agree(prog, adapter_prog, tmp_path, tmp_path_factory):
    """Both stand-alone programs built a second time with -fsanitize=address,undefined and run directly (each has its own main: nothing
    is preloaded) over all scenes, the refusals and the script: the same bytes as the plain build, and no report."""
    san_dir = tmp_path_factory.mktemp("localmap_delta_prog_san")
    if not host_prog.sanitizer_runtime_present(san_dir):
        pytest.skip("the sanitizer runtime (libasan / libubsan) is not installed: a trivial main does not link with -fsanitize")
    san = host_prog.build("localmap_delta_prog", san_dir, sanitize=True)
    asan = host_prog.build("localmap_delta_adapter_prog", san_dir, sanitize=True)
    blobs = [b"".join(o[1] for o in scene_ops(name)) + P.i32(0) for name in Q.CASES]
    before = Q.arrays("points_257")[0]
    blobs.append(P.op_create(before)[1] + b"".join(Q.op_apply(bad, **counts)[1] + Q.op_export()[1] for _, bad, counts in refusals()) + P.i32(0))
    for blob in blobs:
        assert host_prog.run(prog, tmp_path, "run", blob) == host_prog.run(san, tmp_path, "run", blob)
    # the adapter: the appended keyframe lives on the heap, so where it stands in pointer order — and with it the lists' lengths — may
    # differ between two builds; the verdicts, the call counts and the sizes may not
    blob = adapter_blob()
    plain, checked = (parse_adapter(host_prog.run(exe, tmp_path, "script", blob)) for exe in (adapter_prog, asan))
    stable = lambda g: [g[k] for k in ("error", "late_threw", "late_message_ok", "empty_sync_applies")] + [
        (s["equal"], s["applies"], s["n_kf"], s["n_points"]) for s in g["steps"]]
    assert stable(plain) == stable(checked) and all(s["equal"] == 1 for s in checked["steps"])
