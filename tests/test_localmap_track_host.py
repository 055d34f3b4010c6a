"""The resident attribute store and sivo_localmap_search_local_points on the HOST build of the kernels' per-item bodies
(sivo_amd/csrc/localmap_track_math.hpp through tests/localmap_track_host_capi.hpp and tests/localmap_track_prog.cpp): against the
restatement of Tracking::UpdateLocalMap composed with the sequential oracle of SearchByProjection and the reference's recorded track fields
(tests/localmap_track_cases.py), against the pair of entry points the call is defined by, and against a dict-of-rows restatement of the
store.  No GPU; the program also runs under the sanitizers.  Reads only tests/golden."""
import os
import re
import subprocess

import numpy as np
import pytest

import frustum_pin_cases as P
import host_prog
import localmap_cases as LC
import localmap_track_cases as TC

F32 = np.float32
INVALID, CAPACITY = -1, None


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return host_prog.build("localmap_track_prog", tmp_path_factory.mktemp("localmap_track_prog"))


@pytest.fixture(scope="module")
def prog_san(tmp_path_factory):
    d = tmp_path_factory.mktemp("localmap_track_prog_san")
    if not host_prog.sanitizer_runtime_present(d):
        pytest.skip("g++ cannot link with -fsanitize=address,undefined here")
    return host_prog.build("localmap_track_prog", d, sanitize=True)


def codes():
    hdr = open(os.path.join(host_prog.ROOT, "include", "sivo_hip.h")).read()
    return {k: int(re.search(r"#define\s+%s\s+\(?(-?\d+)\)?" % k, hdr).group(1)) for k in ("SIVO_ERR_INVALID_ARGUMENT", "SIVO_ERR_CAPACITY")}


def setup_ops(scene, tables):
    m, fk = TC.the_map()
    at = TC.attrs(m, scene["n_obs"])
    return at, [LC.op_create(tables), TC.op_set_points(np.arange(scene["n_points"]), at), TC.op_frame(fk)]


def run_scene(exe, tmp_path, name):
    scene = TC.SCENES[name]()
    tables, call, want = TC.expected(scene)
    at, ops = setup_ops(scene, tables)
    ops += [TC.op_search(call, scene, tables["n_kf"]), TC.op_search(call, scene, tables["n_kf"], composed=True),
            TC.op_search(call, scene, tables["n_kf"])]
    res = TC.run_ops(exe, tmp_path, ops)
    assert all(r.get("rc", 0) == 0 for r in res), [r.get("message") for r in res]
    return want, res[3], res[4], res[5]


@pytest.mark.parametrize("name", sorted(TC.SCENES))
def test_scene_equals_the_yardsticks_and_the_composed_pair(prog, tmp_path, name):
    """Every output of the call: the restatement composed with the oracle over the expected skip set, the reference's recorded track
    fields for the points in view, and byte for byte the pair sivo_localmap_update + sivo_search_local_points on gathered rows; a second
    call on the handle gives the first one's bytes (no mark of a call outlives it)."""
    want, got, pair, again = run_scene(prog, tmp_path, name)
    TC.check_against_expected(got, want, name)
    TC.same_bytes(got, pair, name)
    TC.same_bytes(got, again, name)


def test_full_scene_has_what_it_is_meant_to_have():
    scene = TC.SCENES["full"]()
    tables, call, want = TC.expected(scene)
    m, _ = TC.the_map()
    local = want["local"]
    assert not np.array_equal(local, np.sort(local)) and len(local) > 2 * 256                   # no identity; several blocks of the passes
    assert tables["point_bad"].sum() > 20 and len(call["point_premarked"]) == 10 and not np.isin(call["point_premarked"], local).any()
    assert want["slot_cleared"].sum() == 1 and (call["frame_point"] >= 0).sum() == 24
    held = call["frame_point"][(call["frame_point"] >= 0) & (want["slot_cleared"] == 0)]
    assert (scene["n_obs"][held] == 0).any() and (scene["n_obs"][held] > 0).any()
    assert len(scene["seen"]) == 15 and np.isin(scene["seen"], local).sum() >= 10 and not np.isin(scene["seen"], held).any()
    assert want["skip"].sum() == np.isin(local, np.concatenate([held, scene["seen"]])).sum()
    assert np.isin(np.arange(600, 620), local).sum() >= 10 and want["n_matches"] > 50             # the twins are in the list
    shared = np.diff(tables["obs_off"]) > 1
    assert shared[local].sum() > 100


def test_sanitized_program_on_the_full_scene(prog_san, tmp_path):
    want, got, pair, again = run_scene(prog_san, tmp_path, "full")
    TC.check_against_expected(got, want, "sanitized")
    TC.same_bytes(got, pair, "sanitized")


def test_store_follows_a_dict_of_rows(prog, tmp_path):
    """set_points (twice over some rows: the later row holds), apply (the appended rows unset, then set), replace (all unset), get_points —
    against a dict of rows."""
    scene = TC.SCENES["one_point"]()
    tables, call, want = TC.expected(scene)
    m, fk = TC.the_map()
    at = TC.attrs(m, scene["n_obs"])
    n = scene["n_points"]
    rng = np.random.default_rng(2)
    other = {k: np.ascontiguousarray(at[k][::-1]) for k in TC.ATTRS}                            # other rows under the same indices
    big = {k: np.concatenate([at[k], at[k][:5]]) for k in TC.ATTRS}
    first = np.sort(rng.choice(n, 300, replace=False))
    second = np.sort(rng.choice(n, 200, replace=False))
    everything = np.arange(n)
    ops = [LC.op_create(tables), TC.op_get_points(everything), TC.op_set_points(first, at), TC.op_set_points(second, other),
           TC.op_get_points(everything), TC.op_append(5), TC.op_get_points(np.arange(n + 5)), TC.op_set_points([n + 1, n + 4], big),
           TC.op_get_points(np.arange(n + 5)), TC.op_get_points([7]), LC.op_replace(tables), TC.op_get_points(everything)]
    res = TC.run_ops(prog, tmp_path, ops)
    assert all(r["rc"] == 0 for r in res), [r["message"] for r in res]
    rows = {}

    def check(r, idx):
        for j, p in enumerate(idx):
            assert r["is_set"][j] == (p in rows), p
            for k in TC.ATTRS:
                wanted = rows[p][k] if p in rows else np.zeros_like(np.asarray(at[k][0]))
                assert np.asarray(r[k][j]).tobytes() == np.asarray(wanted).tobytes(), (p, k)

    check(res[1], everything)
    rows.update({int(p): {k: at[k][p] for k in TC.ATTRS} for p in first})
    rows.update({int(p): {k: other[k][p] for k in TC.ATTRS} for p in second})
    check(res[4], everything)
    check(res[6], np.arange(n + 5))
    rows.update({p: {k: big[k][p] for k in TC.ATTRS} for p in (n + 1, n + 4)})
    check(res[8], np.arange(n + 5))
    check(res[9], [7])
    rows.clear()
    check(res[11], everything)


def test_refusals_leave_the_handle_and_the_outputs_alone(prog, tmp_path):
    c = codes()
    scene = TC.SCENES["points_257"]()
    tables, call, want = TC.expected(scene)
    at, ops = setup_ops(scene, tables)
    n, K = scene["n_points"], tables["n_kf"]
    search = lambda **kw: TC.op_search(call, scene, K, **kw)
    fr17, fr0, frlog = TC.frustum_record().copy(), TC.frustum_record().copy(), TC.frustum_record().copy()
    fr17["nlevels"], fr0["nlevels"], frlog["log_scale_factor"] = 17, 0, 0.0
    _, fk = TC.the_map()
    bad = [
        (TC.op_set_points([3, 3], at), "sivo_localmap_set_points: point_idx is not strictly increasing"),
        (TC.op_set_points([5, 4], at), "sivo_localmap_set_points: point_idx is not strictly increasing"),
        (TC.op_set_points([0, n], dict(at, **{k: np.concatenate([at[k], at[k][:1]]) for k in TC.ATTRS})), "sivo_localmap_set_points: point_idx outside 0 .. n_points - 1"),
        (TC.op_set_points([-1], at), "sivo_localmap_set_points: point_idx outside 0 .. n_points - 1"),
        (TC.op_set_points([1, 2], at, n_rows=-1), "sivo_localmap_set_points: negative count"),
        (TC.op_set_points(None, at, n_rows=2), "sivo_localmap_set_points: null point_idx"),
        (TC.op_set_points([1, 2], at, desc=None), "sivo_localmap_set_points: null attribute array"),
        (TC.op_set_points([1, 2], at, pos=None), "sivo_localmap_set_points: null attribute array"),
        (TC.op_get_points([2, 1]), "sivo_localmap_get_points: point_idx is not strictly increasing"),
        (TC.op_get_points([n]), "sivo_localmap_get_points: point_idx outside 0 .. n_points - 1"),
        (TC.op_get_points([1], n_rows=-3), "sivo_localmap_get_points: negative count"),
        (TC.op_get_points(None, n_rows=1), "sivo_localmap_get_points: null point_idx"),
        (TC.op_get_points([1], null_out=True), "sivo_localmap_get_points: null output array"),
        (search(null=("handle",)), "sivo_localmap_search_local_points: null handle"),
        (search(null=("frame",)), "sivo_localmap_search_local_points: null frame"),
        (search(null=("frustum",)), "sivo_localmap_search_local_points: null frustum"),
        (search(null=("status",)), "sivo_localmap_search_local_points: null status"),
        (search(null=("match",)), "sivo_localmap_search_local_points: null match"),
        (search(null=("voted",)), "sivo_localmap_search_local_points: null result"),
        (search(n_seen=-1), "sivo_localmap_search_local_points: negative count"),
        (search(seen_point=None, n_seen=2), "sivo_localmap_search_local_points: null seen_point"),
        (search(seen_point=np.array([0, n], np.int32)), "sivo_localmap_search_local_points: seen_point outside 0 .. n_points - 1"),
        (search(seen_point=np.array([-1], np.int32)), "sivo_localmap_search_local_points: seen_point outside 0 .. n_points - 1"),
        (search(frame_point=call["frame_point"][:119]), "sivo_localmap_search_local_points: n_slots is 119 and the frame has 120 keypoints"),
        (search(frame_point=np.full(120, n, np.int32)), "sivo_localmap_search_local_points: frame_point outside -1 .. n_points - 1"),
        (search(frustum=fr17), "sivo_localmap_search_local_points: nlevels outside 1 .. 16"),
        (search(frustum=fr0), "sivo_localmap_search_local_points: nlevels outside 1 .. 16"),
        (search(frustum=frlog), "sivo_localmap_search_local_points: log_scale_factor must be positive"),
    ]
    ops += [TC.op_search(call, scene, K)]
    for op, _ in bad:
        ops += [op]
    ops += [TC.op_device(1), search(), TC.op_device(0), TC.op_frame(fk, levels=4), search(), TC.op_frame(fk),
            TC.op_search(dict(call, point_capacity=256), scene, K), TC.op_search(dict(call, kf_capacity=0), scene, K),
            TC.op_search(call, scene, K), TC.op_get_points(np.arange(n)),
            TC.op_append(2), search(), LC.op_replace(tables), search()]
    res = TC.run_ops(prog, tmp_path, ops)
    base = res[3]
    assert base["rc"] == 0
    TC.check_against_expected(base, want, "before")
    untouched = dict(voted=-7, n_local_kf=-7, ref_kf=-7, n_local_points=-7, n_to_match=-7, n_matches=-7)

    def refused(r, code, text):
        assert (r["rc"], r["message"]) == (code, text)
        if "status" not in r:
            return
        assert all(r[k] == v for k, v in untouched.items())
        assert (r["slot_cleared"] == 255).all() and (r["status"] == 255).all() and (r["match"] == -9).all() and (r["level"] == -77).all()
        assert all((r[k] == -7).all() for k in ("local_kf", "local_point", "counts"))
        assert all((r[k].view(np.uint32) == P.SENTINEL.view(np.uint32)).all() for k in P.TRACK)

    for r, (_, text) in zip(res[4:], bad):
        refused(r, c["SIVO_ERR_INVALID_ARGUMENT"], text)
    tail = res[4 + len(bad):]
    refused(tail[1], c["SIVO_ERR_INVALID_ARGUMENT"], "sivo_localmap_search_local_points: the map is on device 1 and the frame on device 0")
    refused(tail[4], c["SIVO_ERR_INVALID_ARGUMENT"], "sivo_localmap_search_local_points: the frustum has more levels than the frame's scale tables")
    refused(tail[6], c["SIVO_ERR_CAPACITY"], "sivo_localmap_search_local_points: 257 local map points, capacity 256")
    refused(tail[7], c["SIVO_ERR_CAPACITY"], "sivo_localmap_search_local_points: 1 local keyframes, capacity 0")
    # the handle after all of it: the same call gives the same bytes, and every stored row is what was set
    assert tail[8]["rc"] == 0
    TC.same_bytes(tail[8], base, "after")
    rows = tail[9]
    assert rows["rc"] == 0 and rows["is_set"].all()
    for k in TC.ATTRS:
        assert rows[k].tobytes() == np.ascontiguousarray(at[k]).tobytes(), k
    # unset rows: their count and the first of them
    refused(tail[11], c["SIVO_ERR_INVALID_ARGUMENT"],
            "sivo_localmap_search_local_points: 2 of the handle's %d points have no attributes, the first is point %d" % (n + 2, n))
    refused(tail[13], c["SIVO_ERR_INVALID_ARGUMENT"],
            "sivo_localmap_search_local_points: %d of the handle's %d points have no attributes, the first is point 0" % (n, n))


def test_header_declarations_are_exported():
    """Every sivo_* function the public header declares is a dynamic symbol of the library: what the new entry points add is built and
    linked, not only declared."""
    lib = os.path.join(host_prog.PKG, "libsivo_hip.so")
    if not os.path.exists(lib):
        pytest.fail("sivo_amd/libsivo_hip.so is not built")
    hdr = open(os.path.join(host_prog.ROOT, "include", "sivo_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(sivo_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    exported = {line.split()[-1] for line in out.stdout.splitlines() if line.strip()}
    assert {"sivo_localmap_set_points", "sivo_localmap_get_points", "sivo_localmap_search_local_points"} <= declared
    assert not declared - exported, sorted(declared - exported)


# ---- the adapter: SIVO::TrackLocalMapSearch against SIVO::UpdateLocalMap + SIVO::SearchLocalPoints ---------------------------------------
def run_adapter(exe, tmp_path, touch_geometry):
    scene = TC.SCENES["full"]()
    tables, call, want = TC.expected(scene)
    script = TC.adapter_script(scene, want)
    raw = host_prog.run(exe, tmp_path, "run", TC.adapter_blob(tables, call, scene, script, touch_geometry))
    return want, script, TC.parse_adapter(raw, len(script), tables["n_kf"], scene["n_points"])


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_adapter_leaves_what_the_pair_leaves(tmp_path_factory, tmp_path, sanitize):
    """Every field of the frame, of every keyframe and of every point after each of three frames that hand their points on: the copy
    that ran TrackLocalMapSearch equals the copy that ran UpdateLocalMap + SearchLocalPoints, byte for byte; the new call made one
    library call per frame, and the first frame's result is the scene's expected one."""
    d = tmp_path_factory.mktemp("localmap_track_adapter")
    if sanitize and not host_prog.sanitizer_runtime_present(d):
        pytest.skip("g++ cannot link with -fsanitize=address,undefined here")
    exe = host_prog.build("localmap_track_adapter_prog", d, sanitize=sanitize)
    want, script, steps = run_adapter(exe, tmp_path, True)
    for s, (a, b) in enumerate(steps):
        assert a["state"] == b["state"], s
        assert (b["searches"] - a["searches"], b["updates"] - a["updates"]) == (1, 1), s      # (the host build's search runs the host update)
    a, b = steps[0]
    local = want["local"]
    assert np.array_equal(b["local_points"], local) and b["ret"] == want["n_matches"] and b["n_to_match"] == want["n_to_match"]
    hit = want["match"] >= 0
    assert np.array_equal(b["slots"][hit], local[want["match"][hit]])
    assert np.array_equal(np.flatnonzero(b["points"]["in_view"]), np.sort(local[want["status"][:len(local)] == 0]))
    moved = script[1]["moved"]
    assert not steps[1][1]["points"]["in_view"][moved].any() and steps[2][1]["points"]["in_view"][moved[0]]
    assert steps[1][1]["ret"] > 0 and steps[2][1]["ret"] >= 0 and (steps[2][1]["slots"] >= 0).sum() > (steps[0][1]["slots"] >= 0).sum()


def test_adapter_without_touch_geometry_is_stale(tmp_path_factory, tmp_path):
    """The same script with the moved points not reported: the device map still has them where they were, and the copies differ — in
    the second frame, at the moved points."""
    exe = host_prog.build("localmap_track_adapter_prog", tmp_path_factory.mktemp("localmap_track_adapter_stale"))
    want, script, steps = run_adapter(exe, tmp_path, False)
    assert steps[0][0]["state"] == steps[0][1]["state"]
    a, b = steps[1]
    assert a["state"] != b["state"]
    moved = script[1]["moved"]
    assert not a["points"]["in_view"][moved].any() and b["points"]["in_view"][moved].any()
