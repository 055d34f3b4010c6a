"""The loop closer's two map corrections on the device (sivo_amd/csrc/loopcorrect.hip): every scene of tests/loop_correct_cases.py byte for
byte against the object-graph restatement of the reference (tests/loop_correct_restatement.py), through the C ABI and through
sivo_amd/loop_closing.py; what the calls leave untouched, repeated and interleaved calls, and the chain correct_loop -> shared_counts ->
essential_graph_optimize -> sim3_correct_points against the restatements chained the same way.  Reads only tests/."""
import ctypes as C

import numpy as np
import pytest

import essential_graph_restatement as EG
import loop_correct_cases as LC

pytestmark = pytest.mark.gpu

S = LC.SENTINEL
LOOP_OUT_NAMES = [n for n, *_ in LC.LOOP_OUT]
GBA_OUT_NAMES = [n for n, *_ in LC.GBA_OUT]


@pytest.fixture(scope="module")
def lc():
    from sivo_amd import loop_closing
    return loop_closing


def _ptr(v):
    return v.ctypes.data if v.size else None


def loop_sentinels(a):
    K, P = a["n_kf"], a["n_points"]
    return {"noncorrected_siw": np.full((K, 8), S, np.float64), "corrected_siw": np.full((K, 8), S, np.float64),
            "tiw_out": np.full((K, 4, 4), S, np.float32), "ow_out": np.full((K, 3), S, np.float32), "corrected_by": np.full(P, -7, np.int32),
            "pos_out": np.full((P, 3), S, np.float32), "normal": np.full((P, 3), S, np.float32), "max_dist": np.full(P, S, np.float32),
            "min_dist": np.full(P, S, np.float32), "flags": np.full(P, 255, np.uint8)}


def loop_abi(lc, a):
    """sivo_loop_correct itself, every output pre-filled with the sentinels."""
    from sivo_amd import _lib
    keep = [np.ascontiguousarray(a[n], dt).ravel() for n, dt in LC.LOOP_IN]
    out = loop_sentinels(a)
    s = lc.LoopCorrect(a["n_kf"], a["cur"], a["n_all"], a["n_points"], *[_ptr(v) for v in keep], *[_ptr(out[n]) for n in LOOP_OUT_NAMES])
    assert _lib.lib().sivo_loop_correct(C.byref(s)) == 0, _lib.lib().sivo_last_error()
    return out


def loop_wrapper(lc, a):
    o = loop_sentinels(a)
    return lc.correct_loop(a["tiw"], a["cur"], a["twc_cur"], a["scw"], a["ow"], a["slot_off"], a["slot_point"], a["pos"], a["skip"], a["obs_off"],
                           a["obs_kf"], a["ref_kf"], a["level_scale"], a["last_scale"],
                           out={k: o[k] for k in ("pos_out", "normal", "max_dist", "min_dist", "flags")})


def gba_abi(lc, a):
    from sivo_amd import _lib
    K, P = a["n_kf"], a["n_points"]
    keep = {n: np.ascontiguousarray(a[n], dt).ravel().copy() for n, dt in LC.GBA_IN}
    out = {"tcw_out": np.full((K, 4, 4), S, np.float32), "ow_out": np.full((K, 3), S, np.float32), "kf_reached": np.full(K, 255, np.uint8),
           "pos_out": np.full((P, 3), S, np.float32), "point_status": np.full(P, 255, np.uint8)}
    s = lc.GbaPropagate(K, a["n_origins"], P, *[_ptr(keep[n]) for n, _ in LC.GBA_IN],
                        *[_ptr(out[n]) for n in ("tcw_out", "ow_out", "kf_reached", "pos_out", "point_status")])
    assert _lib.lib().sivo_gba_propagate(C.byref(s)) == 0, _lib.lib().sivo_last_error()
    out.update(tcw_gba=keep["tcw_gba"], in_gba=keep["in_gba"], tcw_bef=keep["tcw_bef"])
    return out


def gba_wrapper(lc, a):
    K, P = a["n_kf"], a["n_points"]
    out = {"tcw_out": np.full((K, 4, 4), S, np.float32), "ow_out": np.full((K, 3), S, np.float32), "pos_out": np.full((P, 3), S, np.float32)}
    return lc.propagate_global_ba(a["origin"], a["child_off"], a["child_kf"], a["tcw"], a["tcw_gba"], a["in_gba"], a["tcw_bef"], a["pos"],
                                  a["pos_gba"], a["point_in_gba"], a["point_bad"], a["ref_kf"], out=out)


def flat(d, names):
    return {n: np.ascontiguousarray(d[n]).ravel() for n in names}


@pytest.mark.parametrize("name", LC.LOOP_SCENES)
def test_loop_scene_matches_the_restatement_byte_for_byte(lc, name):
    sc = LC.loop_scene(name)
    a, want = sc["args"], sc["expect"]
    got = loop_abi(lc, a)
    assert LC.same_bytes(flat(got, LOOP_OUT_NAMES), want) == []
    # untouched points hold the caller's sentinels in every per-point output but corrected_by
    still = got["corrected_by"] < 0
    assert still.sum() == (want["corrected_by"] < 0).sum()
    assert np.all(got["pos_out"][still] == S) and np.all(got["normal"][still] == S) and np.all(got["flags"][still] == 255)
    w = loop_wrapper(lc, a)
    names = [n for n in LOOP_OUT_NAMES if n != "corrected_by"]
    assert LC.same_bytes(flat(w, names), want) == [] and np.array_equal(w["corrected_by"], want["corrected_by"])


@pytest.mark.parametrize("name", LC.TREE_SCENES)
def test_tree_scene_matches_the_restatement_byte_for_byte(lc, name):
    sc = LC.tree_scene(name)
    a, want = sc["args"], sc["expect"]
    got = gba_abi(lc, a)
    assert LC.same_bytes(flat(got, GBA_OUT_NAMES), want) == []
    away = got["kf_reached"] == 0
    assert np.all(got["tcw_out"][away] == S) and np.all(got["ow_out"][away] == S)
    assert got["tcw_gba"].reshape(-1, 16)[away].tobytes() == np.asarray(a["tcw_gba"], np.float32).reshape(-1, 16)[away].tobytes()
    kept = ~np.isin(got["point_status"], (1, 2))
    assert np.all(got["pos_out"][kept] == S)
    held = {n: np.array(a[n]).tobytes() for n in ("tcw_gba", "in_gba", "tcw_bef")}
    w = gba_wrapper(lc, a)
    assert LC.same_bytes(flat(w, GBA_OUT_NAMES), want) == []
    assert all(np.asarray(a[n]).tobytes() == held[n] for n in held)                 # the wrapper works on copies


def test_repeated_and_interleaved_calls_give_identical_bytes(lc):
    """Nothing of one call reaches the next: the ownership words, the scratch and the staging buffers, which grow for the larger scene
    and are reused, larger than needed, for the smaller one after it."""
    small, large = LC.loop_scene("two_keyframes"), LC.loop_scene("sixty_five_keyframes")
    tsmall, tlarge = LC.tree_scene("run_1"), LC.tree_scene("run_40")
    first = {}
    for rnd in range(2):
        for key, sc, call, names in (("s", small, loop_abi, LOOP_OUT_NAMES), ("ts", tsmall, gba_abi, GBA_OUT_NAMES), ("l", large, loop_abi, LOOP_OUT_NAMES),
                                     ("tl", tlarge, gba_abi, GBA_OUT_NAMES), ("s2", small, loop_abi, LOOP_OUT_NAMES), ("s3", small, loop_abi, LOOP_OUT_NAMES),
                                     ("ts2", tsmall, gba_abi, GBA_OUT_NAMES)):
            got = flat(call(lc, sc["args"]), names)
            assert LC.same_bytes(got, sc["expect"]) == [], (rnd, key)
            if rnd == 0:
                first[key] = got
            else:
                assert all(got[n].tobytes() == first[key][n].tobytes() for n in names), (rnd, key)


def test_buffers_grow_and_shrink(lc):
    """A problem larger than the staging buffers' first size (4 MiB), between two small ones."""
    rng = np.random.default_rng(5)
    sc = LC.tree_scene("run_2")
    a = dict(sc["args"])
    P = 300000                                              # 300 000 points: 3.6 MB per position array, over 10 MB staged
    a.update(n_points=P, pos=(rng.normal(size=(P, 3)) * 8).astype(np.float32), pos_gba=(rng.normal(size=(P, 3)) * 8).astype(np.float32),
             point_in_gba=(rng.random(P) < 0.5).astype(np.uint8), point_bad=(rng.random(P) < 0.05).astype(np.uint8),
             ref_kf=rng.integers(0, a["n_kf"], P).astype(np.int32))
    before = flat(gba_abi(lc, sc["args"]), GBA_OUT_NAMES)
    big = gba_abi(lc, a)
    after = flat(gba_abi(lc, sc["args"]), GBA_OUT_NAMES)
    assert LC.same_bytes(before, sc["expect"]) == [] and LC.same_bytes(after, sc["expect"]) == []
    # the keyframes of the large call are the small call's; its points follow their three rules
    assert big["tcw_out"].tobytes() == np.asarray(sc["expect"]["tcw_out"]).tobytes()
    st = big["point_status"]
    assert np.array_equal(st == 0, a["point_bad"] == 1) and np.array_equal(st == 1, (a["point_bad"] == 0) & (a["point_in_gba"] == 1))
    assert big["pos_out"][st == 1].tobytes() == a["pos_gba"][st == 1].tobytes() and np.all(np.isin(st, (0, 1, 2)))
    carried = np.flatnonzero(st == 2)[:50]                  # a cut of the carried ones against the restatement's gemm
    import loop_correct_restatement as LR
    for p in carried:
        r = a["ref_kf"][p]
        bef, twc = np.asarray(sc["expect"]["tcw_bef"]).reshape(-1, 4, 4)[r], sc["info"]["kfs"][r].GetPoseInverse()
        Xc = LR.gemm(bef[:3, :3], a["pos"][p], C=bef[:3, 3])
        assert big["pos_out"][p].tobytes() == LR.gemm(twc[:3, :3], Xc, C=twc[:3, 3]).tobytes()


def _counts(a, bad):
    """The counting loop of KeyFrame::UpdateConnections over the scene's arrays: per corrected keyframe, how many of its slots hold a
    point that is not bad and is observed by keyframe k (k itself skipped)."""
    out = np.zeros((a["n_kf"], a["n_all"]), np.int32)
    for i in range(a["n_kf"]):
        for p in a["slot_point"][a["slot_off"][i]:a["slot_off"][i + 1]]:
            if p < 0 or bad[p]:
                continue
            for k in a["obs_kf"][a["obs_off"][p]:a["obs_off"][p + 1]]:
                if k != i:
                    out[i, k] += 1
    return out


def _graph(a, spec_poses, table_index, loop, counts):
    """The essential graph the loop closer hands on: the corrected Sim3 for the corrected keyframes and Sim3(pose) for the others as
    estimates, an edge between every two keyframes that share a point, measured from the uncorrected poses, the outside keyframe fixed."""
    K, A = a["n_kf"], a["n_all"]
    before = np.stack([loop["noncorrected_siw"].reshape(K, 8)[i] if i < K else EG.sim3_from_pose(spec_poses[table_index[i]]) for i in range(A)])
    siw = before.copy()
    siw[:K] = loop["corrected_siw"].reshape(K, 8)
    from sivo_amd.optimizer import SIM3_EDGE_DTYPE
    edges = [(i, j, EG.mul(before[j], EG.inv(before[i]))) for i in range(K) for j in range(A) if j != i and counts[i, j] > 0 and (j >= K or j < i)]
    fixed = np.zeros(A, bool)
    fixed[K + int(np.flatnonzero(counts[:, K:].sum(0) > 0)[0])] = True               # pLoopKF: an outside keyframe the graph reaches
    return siw, fixed, np.array(edges, SIM3_EDGE_DTYPE)


def test_chained_with_the_rest_of_the_loop_closer(lc):
    """correct_loop -> covisibility.shared_counts -> essential_graph_optimize -> sim3_correct_points on the device, and the restatements
    chained the same way.  The first two links and the last are exact; the optimiser agrees with its restatement to the bound of
    tests/test_gpu_essential_graph.py (2e-6 in the quaternion and the scale, 2e-6 of the extent in the translation), which
    the point correction passes on: a point X in the reference keyframe's frame moves by at most 2 |X| dq + |X| ds + dt, below
    8 * 2e-6 * extent with |X| and |t| inside the extent."""
    from sivo_amd import covisibility as cov, optimizer as opt
    sc = LC.loop_scene("reference_places")
    a, want, info = sc["args"], sc["expect"], sc["info"]
    got = loop_abi(lc, a)
    assert LC.same_bytes(flat(got, LOOP_OUT_NAMES), want) == []
    bad = np.array([p.mbBad for p in info["points"]], np.uint8)
    no = int(a["obs_off"][-1])
    table = cov.ObservationTable(a["n_all"], a["obs_off"], a["obs_kf"], np.zeros(no, np.uint8), np.zeros(no, np.uint8), bad)
    sets = [a["slot_point"][a["slot_off"][i]:a["slot_off"][i + 1]] for i in range(a["n_kf"])]
    counts = cov.shared_counts(table, sets, np.arange(a["n_kf"]))
    want_counts = _counts(a, bad)
    assert np.array_equal(counts, want_counts) and counts.sum() > 0
    spec, kfs = info["spec"], info["kfs"]
    table_index = [kfs.index(k) for k in info["table"]]
    g_siw, fixed, g_edges = _graph(a, spec["poses"], table_index, got, counts)
    w_siw, _, w_edges = _graph(a, spec["poses"], table_index, want, want_counts)
    assert g_siw.tobytes() == w_siw.tobytes() and g_edges.tobytes() == w_edges.tobytes() and len(g_edges) >= a["n_kf"]
    g_opt = opt.essential_graph_optimize(g_siw, fixed, g_edges, fix_scale=False)
    w_opt = EG.optimize(w_siw, fixed, w_edges, False)
    tol = 2e-6
    extent = max(1.0, float(np.max(np.abs(g_siw[:, 4:7]))), float(np.max(np.abs(a["pos"]))))
    sign = np.where(np.sum(g_opt["siw"][:, :4] * w_opt["siw"][:, :4], 1) < 0, -1.0, 1.0)[:, None]
    assert np.max(np.abs(g_opt["siw"][:, :4] - sign * w_opt["siw"][:, :4])) < tol and np.max(np.abs(g_opt["siw"][:, 7] - w_opt["siw"][:, 7])) < tol
    assert np.max(np.abs(g_opt["siw"][:, 4:7] - w_opt["siw"][:, 4:7])) < tol * extent
    moved = got["corrected_by"] >= 0
    xyz = np.where(moved[:, None], got["pos_out"], a["pos"]).astype(np.float32)
    ref = np.where(moved, got["corrected_by"], a["ref_kf"]).astype(np.int32)           # (Optimizer.cc:1213-1221)
    g_pts = opt.sim3_correct_points(xyz, ref, g_siw, g_opt["siw"])
    assert g_pts.tobytes() == EG.correct_points(xyz, ref, g_siw, g_opt["siw"]).tobytes()
    w_pts = EG.correct_points(xyz, ref, w_siw, w_opt["siw"])
    assert np.max(np.abs(g_pts.astype(np.float64) - w_pts.astype(np.float64))) < 8 * tol * extent
