"""sivo_localmap_search_local_points and the resident attribute store on the device (sivo_amd/csrc/localmap_track.hip through
sivo_amd/local_map.py) against the pair it replaces — sivo_localmap_update, a gather by index on the host, sivo_search_local_points —
byte for byte in every output, and against the two yardsticks composed (tests/localmap_track_cases.py).  All comparisons are exact: the
arithmetic is frustum_math.hpp's and the search engine's.  Reads only tests/golden."""
import numpy as np
import pytest

import frustum_pin_cases as P
import localmap_track_cases as TC

pytestmark = pytest.mark.gpu
F32 = np.float32
UPDATE = ("slot_cleared", "local_kf", "local_point", "counts")


def frustum_of(nlevels=P.NLEVELS):
    from sivo_amd import tracking as T
    m, _ = TC.the_map()
    return T.frustum(m["Tcw"], *(getattr(P.FC, k) for k in ("FX", "FY", "CX", "CY", "BF")), P.BOUNDS, P.SCALE_FACTOR, nlevels, P.COS_LIMIT)


@pytest.fixture(scope="module")
def frame():
    from sivo_amd import matcher as M
    _, fk = TC.the_map()
    return M.MatchFrame(fk["keys"], fk["u_right"], fk["desc"], P.BOUNDS, fk["scale"], fk["sigma2"], fk["inv_sigma2"])


def make_map(tables, at):
    from sivo_amd import local_map as LM
    lm = LM.LocalMap(tables["n_kf"], **{k: v for k, v in tables.items() if k != "n_kf"})
    lm.set_points(np.arange(len(at["n_obs"])), *(at[k] for k in TC.ATTRS))
    return lm


def sentinels(call, n_kf, n_keys):
    kc, pc = call["kf_capacity"], call["point_capacity"]
    out = dict(slot_cleared=np.full(n_keys, 255, np.uint8), local_kf=np.full(kc, TC.R.SENTINEL, np.int32),
               local_point=np.full(pc, TC.R.SENTINEL, np.int32), counts=np.full(n_kf, TC.R.SENTINEL, np.int32),
               status=np.full(pc, TC.STATUS_SENTINEL, np.uint8), level=np.full(pc, P.LEVEL_SENTINEL, np.int32),
               match=np.full(n_keys, TC.MATCH_SENTINEL, np.int32))
    out.update({k: np.full(pc, P.SENTINEL, F32) for k in P.TRACK})
    return out


def as_dict(res, out):
    """A TrackResult / Result and the arrays the call wrote into, in the form of the host program's outputs."""
    d = dict(out, voted=int(res.voted), n_local_kf=TC.R.SENTINEL if res.local_kf is None else len(res.local_kf), ref_kf=res.ref_kf,
             n_local_points=len(res.local_points))
    for k in ("n_to_match", "n_matches"):
        if hasattr(res, k):
            d[k] = getattr(res, k)
    return d


def fused(lm, F, call, seen, th, nn_ratio, fr=None):
    out = sentinels(call, lm.n_kf, F.n)
    res = lm.search_local_points(F, fr or frustum_of(), call["frame_point"], call["kf_premarked"], call["point_premarked"], call["prev_local_kf"],
                                 seen, th, nn_ratio, kf_capacity=call["kf_capacity"], point_capacity=call["point_capacity"], out=out)
    return as_dict(res, out)


def composed(lm, F, call, seen, th, nn_ratio, at, fr=None):
    """sivo_localmap_update, the gather by index, sivo_search_local_points: the pair the issue defines the new call by."""
    from sivo_amd import tracking as T
    out = sentinels(call, lm.n_kf, F.n)
    upd = lm.update(call["frame_point"], call["kf_premarked"], call["point_premarked"], call["prev_local_kf"], kf_capacity=call["kf_capacity"],
                    point_capacity=call["point_capacity"], out={k: out[k] for k in UPDATE})
    local, fp = upd.local_points, call["frame_point"]
    held = fp[(fp >= 0) & (upd.slot_cleared == 0)]
    skip = np.isin(local, np.concatenate([held, np.asarray(seen, np.int32)])).astype(np.uint8)
    occ = np.where((fp >= 0) & (upd.slot_cleared == 0), at["n_obs"][np.maximum(fp, 0)], -1).astype(np.int32)
    n = len(local)
    pre = {k: out[k][:n] for k in P.TRACK + ("level",)}
    res = T.search_local_points(F, fr or frustum_of(), at["pos"][local], at["normal"][local], at["min_dist"][local], at["max_dist"][local], skip,
                                at["desc"][local], at["n_obs"][local], th, nn_ratio, occ, out=pre)
    for k in P.TRACK + ("level", "status"):
        out[k][:n] = res[k]
    out["match"] = res["match"]
    d = as_dict(upd, out)
    d.update(n_to_match=res["n_in_view"], n_matches=res["n_matches"])
    return d


def same(a, b, what):
    for k in sorted(a):
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k)


def run_scene(name):
    scene = TC.SCENES[name]()
    tables, call, want = TC.expected(scene)
    m, _ = TC.the_map()
    at = TC.attrs(m, scene["n_obs"])
    return scene, tables, call, want, at


@pytest.mark.parametrize("name", sorted(TC.SCENES))
def test_equals_update_then_search_and_the_yardsticks(frame, name):
    """Every output, byte for byte, of the composed pair on the device — the 620-point scene (a non-identity local_point over several
    blocks of the point passes, bad, premarked, seen and held points, a cleared slot, a held point without observations, twins that
    force repair rounds) and the smallest shapes: 0, 1, 255, 256, 257 and 600 local points, nobody voting with and without
    prev_local_kf — and the restatement composed with the sequential oracle on the reference's recorded track fields."""
    scene, tables, call, want, at = run_scene(name)
    with make_map(tables, at) as lm:
        got = fused(lm, frame, call, scene["seen"], scene["th"], scene["nn_ratio"])
        same(got, composed(lm, frame, call, scene["seen"], scene["th"], scene["nn_ratio"], at), name)
    TC.check_against_expected(got, want, name)
    if name == "full":
        assert want["n_matches"] > 20 and want["skip"].sum() >= 30 and want["slot_cleared"].sum() == 1
        assert not np.array_equal(want["local"], np.sort(want["local"]))


def test_full_scene_needs_repair_rounds(frame):
    """The twins of the scene choose one keypoint: the generic engine on the queries of the composed pair runs more than the two rounds
    of a collision-free call, so the new call's producer fed an engine that had to repair."""
    from sivo_amd import matcher as M, tracking as T
    scene, tables, call, want, at = run_scene("full")
    _, fk = TC.the_map()
    local = want["local"]
    cull = T.frustum_cull(frustum_of(), at["pos"][local], at["normal"][local], at["min_dist"][local], at["max_dist"][local], want["skip"].astype(np.uint8))
    q = np.zeros(len(local), M.QUERY_DTYPE)
    iv = cull["in_view"]
    r = np.where(cull["view_cos"] > 0.998, F32(2.5), F32(4.0)) * F32(scene["th"]) * fk["scale"][np.where(iv, cull["level"], 0)]
    q["u"], q["v"], q["ur"], q["radius"], q["gate"] = cull["proj_x"], cull["proj_y"], cull["proj_xr"], r, r
    q["lvl_lo"], q["lvl_hi"] = cull["level"] - 1, cull["level"]
    q["flags"] = np.where(iv, M.Q_VALID | np.where(at["n_obs"][local] > 0, M.Q_BLOCKS, 0), 0)
    res = M.search(frame, q, at["desc"][local], dict(th_dist=M.TH_HIGH, gate_mode=1, ratio_mode=1, nn_ratio=0.8, dynamic=1), blocked=want["occ"] > 0)
    assert res["rounds"] > 2


def test_nothing_in_view(frame):
    """Every stored position behind the camera: no match, every status BEHIND or SKIPPED, the track outputs untouched."""
    scene, tables, call, want, at = run_scene("full")
    at = dict(at, pos=at["pos"].copy())
    at["pos"][:, 2] = -np.abs(at["pos"][:, 2]) - 5
    with make_map(tables, at) as lm:
        got = fused(lm, frame, call, scene["seen"], 3.0, 0.8)
        same(got, composed(lm, frame, call, scene["seen"], 3.0, 0.8, at), "behind")
    n = got["n_local_points"]
    assert got["n_to_match"] == 0 and got["n_matches"] == 0 and (got["match"] == -1).all() and n == want["n_local_points"]
    assert np.isin(got["status"][:n], (1, 6)).all() and (got["level"] == P.LEVEL_SENTINEL).all()
    assert (got["proj_x"].view(np.uint32) == P.SENTINEL.view(np.uint32)).all()


def test_capacity_error_writes_no_search_output(frame):
    from sivo_amd._lib import ERR_CAPACITY, SivoError
    scene, tables, call, want, at = run_scene("full")
    small = dict(call, point_capacity=want["n_local_points"] - 1)
    with make_map(tables, at) as lm:
        out = sentinels(small, lm.n_kf, frame.n)
        before = {k: v.copy() for k, v in out.items()}
        with pytest.raises(SivoError, match="local map points, capacity") as e:
            lm.search_local_points(frame, frustum_of(), call["frame_point"], call["kf_premarked"], call["point_premarked"], call["prev_local_kf"],
                                   scene["seen"], 3.0, 0.8, kf_capacity=small["kf_capacity"], point_capacity=small["point_capacity"], out=out)
        assert e.value.code == ERR_CAPACITY
        same(out, before, "capacity")
        got = fused(lm, frame, call, scene["seen"], scene["th"], scene["nn_ratio"])       # the handle serves the next call
    TC.check_against_expected(got, want, "after the capacity error")


def test_calls_on_one_handle_do_not_see_each_other(frame):
    """Three calls on one handle: the scene's, one with another seen_point and th (the skip marks of the first are gone), the first again:
    run-to-run identity, and each equal to the composed pair."""
    scene, tables, call, want, at = run_scene("full")
    other_seen = want["local"][want["status"][:len(want["local"])] == 0][::3]
    with make_map(tables, at) as lm:
        first = fused(lm, frame, call, scene["seen"], 3.0, 0.8)
        second = fused(lm, frame, call, other_seen, 1.0, 0.8)
        same(second, composed(lm, frame, call, other_seen, 1.0, 0.8, at), "second")
        third = fused(lm, frame, call, scene["seen"], 3.0, 0.8)
    same(first, third, "run to run")
    TC.check_against_expected(first, want, "first")
    assert (second["status"][:len(want["local"])][np.isin(want["local"], other_seen)] == 6).all() and second["n_to_match"] < first["n_to_match"]


def test_set_points_of_one_row_changes_that_point_alone(frame):
    scene, tables, call, want, at = run_scene("full")
    matched = want["match"][want["match"] >= 0]
    i = int(matched[len(matched) // 2])                                 # a local point in view that won a keypoint
    p = int(want["local"][i])
    moved = {k: at[k].copy() for k in TC.ATTRS}
    moved["pos"][p, 2] = -abs(moved["pos"][p, 2]) - 5
    with make_map(tables, at) as lm:
        base = fused(lm, frame, call, scene["seen"], 3.0, 0.8)
        lm.set_points([p], *(moved[k][p:p + 1] for k in TC.ATTRS))
        row = lm.get_points([p])
        assert row["is_set"].all() and all(row[k].tobytes() == np.asarray(moved[k][p:p + 1]).tobytes() for k in TC.ATTRS)
        got = fused(lm, frame, call, scene["seen"], 3.0, 0.8)
        same(got, composed(lm, frame, call, scene["seen"], 3.0, 0.8, moved), "moved")
    others = np.arange(len(got["status"])) != i
    assert base["status"][i] == 0 and got["status"][i] == 1 and got["n_to_match"] == base["n_to_match"] - 1
    for k in ("status", "level") + P.TRACK:
        assert got[k][others].tobytes() == base[k][others].tobytes(), k
    assert (got["match"] != i).all()


def test_attributes_over_apply_replace_and_a_second_handle(frame):
    """apply onto a larger map keeps the stored rows and leaves the appended points unset (the search is refused with their count and
    the first index until a set_points names them); replace unsets everything; a second handle with other attributes is not touched."""
    from sivo_amd._lib import SivoError
    scene, tables, call, want, at = run_scene("full")
    n = scene["n_points"]
    behind = dict(at, pos=at["pos"].copy())
    behind["pos"][:, 2] = -np.abs(behind["pos"][:, 2]) - 5
    args = (frame, frustum_of(), call["frame_point"], call["kf_premarked"], call["point_premarked"], call["prev_local_kf"], scene["seen"], 3.0, 0.8)
    with make_map(tables, at) as lm, make_map(tables, behind) as lm2:
        base = fused(lm, frame, call, scene["seen"], 3.0, 0.8)
        lm.apply(lm.n_kf, n + 3, point_rows=dict(idx=[n, n + 1, n + 2], obs_off=[0, 0, 0, 0], obs_kf=[], bad=[0, 0, 0]))
        rows = lm.get_points(np.arange(n + 3))
        assert rows["is_set"][:n].all() and not rows["is_set"][n:].any() and not rows["desc"][n:].any()
        for k in TC.ATTRS:
            assert rows[k][:n].tobytes() == np.ascontiguousarray(at[k]).tobytes(), k
        with pytest.raises(SivoError, match="3 of the handle's %d points have no attributes, the first is point %d" % (n + 3, n)):
            lm.search_local_points(*args)
        lm.set_points([n, n + 1, n + 2], *(at[k][:3] for k in TC.ATTRS))
        same(fused(lm, frame, call, scene["seen"], 3.0, 0.8), base, "after apply")
        other = fused(lm2, frame, call, scene["seen"], 3.0, 0.8)
        assert other["n_to_match"] == 0 and base["n_to_match"] > 0
        same(fused(lm, frame, call, scene["seen"], 3.0, 0.8), base, "beside a second handle")
        lm.replace(tables["n_kf"], **{k: v for k, v in tables.items() if k != "n_kf"})
        assert not lm.get_points(np.arange(n))["is_set"].any()
        with pytest.raises(SivoError, match="%d of the handle's %d points have no attributes, the first is point 0" % (n, n)):
            lm.search_local_points(*args)
    TC.check_against_expected(base, want, "base")


def test_refusals(frame):
    from sivo_amd import matcher as M
    from sivo_amd._lib import SivoError
    scene, tables, call, want, at = run_scene("one_point")
    _, fk = TC.the_map()
    rest = (call["kf_premarked"], call["point_premarked"], call["prev_local_kf"])
    with make_map(tables, at) as lm:
        with pytest.raises(SivoError, match="n_slots is 119 and the frame has 120 keypoints"):
            lm.search_local_points(frame, frustum_of(), call["frame_point"][:119], *rest)
        with pytest.raises(SivoError, match="seen_point outside"):
            lm.search_local_points(frame, frustum_of(), call["frame_point"], *rest, seen_point=[scene["n_points"]])
        for nlevels in (0, 17):
            with pytest.raises(SivoError, match="nlevels outside 1 .. 16"):
                lm.search_local_points(frame, frustum_of(nlevels), call["frame_point"], *rest)
        keys = fk["keys"].copy()
        keys["octave"] = np.minimum(keys["octave"], 3)
        few = M.MatchFrame(keys, fk["u_right"], fk["desc"], P.BOUNDS, fk["scale"][:4], fk["sigma2"][:4], fk["inv_sigma2"][:4])
        with pytest.raises(SivoError, match="more levels than the frame"):
            lm.search_local_points(few, frustum_of(), np.minimum(call["frame_point"], -1), *rest)
        for idx, text in (([3, 3], "not strictly increasing"), ([5, 4], "not strictly increasing"), ([scene["n_points"]], "point_idx outside"), ([-1], "point_idx outside")):
            with pytest.raises(SivoError, match=text):
                lm.set_points(idx, *(at[k][:len(idx)] for k in TC.ATTRS))
            with pytest.raises(SivoError, match=text):
                lm.get_points(idx)
        got = fused(lm, frame, call, scene["seen"], 3.0, 0.8)                              # the handle is as it was
    TC.check_against_expected(got, want, "after the refusals")
