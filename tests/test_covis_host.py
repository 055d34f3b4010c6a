"""The covisibility bookkeeping (sivo_amd/csrc/covis_math.hpp, the C ABI of include/sivo_hip.h and sivo_amd/api/orbslam/CovisibilityAdapter.h)
against a line-by-line restatement of the reference on an object graph (tests/covis_restatement.py), without a device: the per-slot
bodies the kernels run are compiled for the host into two stand-alone programs (tests/covis_prog.cpp for the C ABI, tests/covis_adapter_prog.cpp
for the adapter over stand-in SLAM types), plain and with -fsanitize=address,undefined.  Every output is an integer and must be equal.
Scenes: tests/covis_cases.py."""
import ctypes as C
import os

import numpy as np
import pytest

import covis_adapter_cases as A
import covis_cases as P
import covis_restatement as R
import host_prog

ROOT = host_prog.ROOT


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return host_prog.build("covis_prog", tmp_path_factory.mktemp("covis_prog"))


@pytest.fixture(scope="module")
def adapter_prog(tmp_path_factory):
    return host_prog.build("covis_adapter_prog", tmp_path_factory.mktemp("covis_adapter_prog"))


# ---- counts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.COUNT_CASES))
def test_counts_equal_the_restatement(prog, tmp_path, name):
    t, sets, selfs, want = P.count_arrays(name)
    rc, got = P.host_count(prog, tmp_path, t, sets, selfs)
    assert rc == 0 and np.array_equal(got, want)
    for s, me in enumerate(selfs):                                  # the keyframe itself is never counted
        if me >= 0:
            assert want[s, me] == 0


def test_count_scenes_hold_what_they_are_named_for():
    assert [P.count_arrays("n_kf_%d" % n)[0]["n_kf"] for n in (1, 2, 63, 64, 65, 1025)] == [1, 2, 63, 64, 65, 1025]
    assert [P.count_arrays("lds_bound_%d" % n)[0]["n_kf"] for n in (P.LDS_KF - 1, P.LDS_KF, P.LDS_KF + 1)] == [8191, 8192, 8193]
    for n in (P.LDS_KF - 1, P.LDS_KF, P.LDS_KF + 1):                # the last keyframe index is counted, and a bad point is not
        t, sets, selfs, want = P.count_arrays("lds_bound_%d" % n)
        assert want[0, n - 1] == 5 and want[1, 0] == 5 and want[2, n - 1] == 6 and t["point_bad"].sum() == 1
    t, sets, selfs, want = P.count_arrays("set_sizes")
    assert [len(s) for s in sets] == [0, 1, 63, 64, 65, 2049, 0, 1, 65] and selfs.tolist() == [0, 1, 2, 3, 4, 5, -1, -1, -1]
    big = sets[5]
    held = big[big >= 0]
    assert (big == -1).sum() > 50 and t["point_bad"][held].sum() > 50                                  # null slots and bad points
    assert len(np.unique(held)) < len(held)                                                            # a point in two slots
    lists = [set(t["obs_kf"][t["obs_off"][p]:t["obs_off"][p + 1]].tolist()) for p in held]
    assert sum(5 in l for l in lists) > 100 and sum(5 not in l and len(l) > 0 for l in lists) > 50     # self present and absent
    fr = sets[8]
    assert any(t["obs_off"][p] == t["obs_off"][p + 1] and not t["point_bad"][p] for p in fr[fr >= 0])  # a point without observations
    t, sets, selfs, want = P.count_arrays("one_counter")
    assert want.tolist() == [[0, 2049], [2049, 2049]]
    # a point in two slots counts twice: the same set without the second slot counts one less for each of the point's observers
    t, sets, selfs, want = P.count_arrays("three_sets")
    s = sets[1]
    vals, cnt = np.unique(s[s >= 0], return_counts=True)
    dup = [v for v, c in zip(vals, cnt) if c == 2 and not t["point_bad"][v]]
    assert dup


def test_three_sets_in_one_call_equal_the_single_calls(prog, tmp_path):
    t, sets, selfs, want = P.count_arrays("three_sets")
    assert len({len(s) for s in sets}) == 3
    for s in range(3):
        rc, got = P.host_count(prog, tmp_path, t, sets[s:s + 1], selfs[s:s + 1])
        assert rc == 0 and np.array_equal(got[0], want[s])
    # and a second slot of a point adds one for each of its observers
    one = sets[1]
    vals, cnt = np.unique(one[one >= 0], return_counts=True)
    p = next(int(v) for v, c in zip(vals, cnt) if c == 2 and not t["point_bad"][v])
    less = np.delete(one, np.flatnonzero(one == p)[1])
    rc, got = P.host_count(prog, tmp_path, t, [less], selfs[1:2])
    obs = t["obs_kf"][t["obs_off"][p]:t["obs_off"][p + 1]]
    delta = np.bincount(obs[obs != selfs[1]], minlength=t["n_kf"])
    assert delta.sum() > 0 and np.array_equal(want[1] - got[0], delta)


# ---- keyframe culling --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mono", P.KF_RUNS)
def test_keyframe_culling_equals_the_restatement(prog, tmp_path, name, mono):
    t, local = P.kf_arrays(name)
    want = P.kf_restatement(name, mono)
    got = P.host_kfcull(prog, tmp_path, t, local, mono)
    assert got["rc"] == 0
    for k in ("decision", "n_mps", "n_redundant", "bad_after"):     # (a keyframe skipped as id 0 keeps the caller's -7 in both)
        assert np.array_equal(got[k], want[k]), k


def test_keyframe_scenes_show_what_they_are_named_for():
    r = lambda name, mono=0, removals=True: P.kf_restatement(name, mono, removals)
    assert r("nothing_culled")["decision"].tolist() == [0, 0, 0, 0] and r("nothing_culled")["n_mps"].min() > 0
    assert (r("edge_9_of_10")["n_mps"][0], r("edge_9_of_10")["n_redundant"][0], r("edge_9_of_10")["decision"][0]) == (10, 9, 0)
    assert (r("edge_10_of_10")["n_mps"][0], r("edge_10_of_10")["n_redundant"][0], r("edge_10_of_10")["decision"][0]) == (10, 10, 1)
    assert (r("edge_0_of_0")["n_mps"][0], r("edge_0_of_0")["n_redundant"][0], r("edge_0_of_0")["decision"][0]) == (0, 0, 0)
    two = r("two_stereo")
    assert two["scene"].points[0].Observations() == 4 and len(two["scene"].points[0].mObservations) == 2
    assert (two["n_mps"][0], two["n_redundant"][0]) == (1, 0)
    assert (r("level_edge")["n_mps"][0], r("level_edge")["n_redundant"][0]) == (2, 1)
    # the chain: a loop without the removals culls both, the reference's only the first
    assert r("chain")["decision"].tolist() == [1, 0] and r("chain", removals=False)["decision"].tolist() == [1, 1]
    assert r("chain")["bad_after"].sum() == 0 and r("chain")["n_redundant"].tolist() == [15, 0]
    # the bad-point chain: the points A leaves with nObs 1 go bad, B's nMPs shrinks from 22 to 19 and B is culled
    bc, bc_off = r("bad_chain"), r("bad_chain", removals=False)
    assert bc["decision"].tolist() == [1, 1] and bc_off["decision"].tolist() == [1, 0]
    assert bc["n_mps"].tolist() == [31, 19] and bc_off["n_mps"].tolist() == [31, 22] and bc["bad_after"].sum() == 3 and bc_off["bad_after"].sum() == 0
    nothing = r("nothing_culled")                                   # nObs 2 and nothing lost: not bad
    assert all(p.Observations() == 2 for p in nothing["scene"].points) and nothing["bad_after"].sum() == 0
    assert r("id0_first")["decision"].tolist() == [3, 1, 0] and r("id0_middle")["decision"].tolist() == [1, 3, 0]
    assert r("id0_first")["n_mps"].tolist() == [P.SENTINEL, 15, 10]
    ne = r("not_erasable")                                          # to be erased later: the keyframe behind it sees no removal
    assert ne["decision"].tolist() == [2, 1] and ne["n_redundant"].tolist() == [15, 10] and ne["scene"].kfs[0].mbToBeErased and not ne["scene"].kfs[0].isBad()
    assert (r("depth")["n_mps"][0], r("depth")["n_redundant"][0]) == (5, 3) and (r("depth", 1)["n_mps"][0], r("depth", 1)["n_redundant"][0]) == (7, 5)
    nl = r("not_listed")
    assert nl["decision"].tolist() == [1, 0] and nl["n_redundant"].tolist() == [10, 1] and nl["bad_after"].sum() == 0
    assert [len(k["point"]) for k in P.kf_arrays("slot_counts")[1]] == [0, 1, 1023, 1024, 1025, 2500]
    big = r("culled_2500")                                          # 100 points turn bad, in each of the three rounds of 1024 threads
    assert big["decision"].tolist() == [1, 1] and big["n_mps"].tolist() == [2500, 30] and big["bad_after"].sum() == 100
    assert big["bad_after"][2048:].sum() == len(range(2049, 2500, 25)) == 19 and r("culled_2500", removals=False)["n_mps"].tolist() == [2500, 130]
    assert len(r("empty_list")["decision"]) == 0 and r("empty_list")["bad_after"].tolist() == [0, 1, 0, 0]


@pytest.mark.parametrize("seed", P.FAMILY_SEEDS)
def test_the_seeded_family_is_sequential(seed):
    on, off = P.kf_restatement("family_%d" % seed, 0), P.kf_restatement("family_%d" % seed, 0, False)
    n = len(on["decision"])
    culled = int((on["decision"] == 1).sum())
    assert n == 40 and 2 <= culled <= n - 2
    assert (on["decision"] != off["decision"]).any()
    assert 2900 < len(on["bad_after"]) <= 3000 and on["bad_after"].sum() > off["bad_after"].sum() >= 30
    assert set(on["decision"].tolist()) >= {0, 1, 3}


# ---- map-point culling -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,mono", P.MP_RUNS)
def test_map_point_culling_equals_the_restatement(prog, tmp_path, n, mono):
    want, _, _ = P.mp_restatement(n, mono)
    rc, got = P.host_mpcull(prog, tmp_path, R.export_recent(P.mp_objects(n)), P.MP_CURRENT, mono)
    assert rc == 0 and np.array_equal(got, want)


def test_map_point_edges_take_the_branch_they_are_named_for():
    st = {m: P.mp_restatement(65, m)[0] for m in (0, 1)}
    assert st[0][:6].tolist() == [0, 2, 0, 0, 1, 1] and st[1][:6].tolist() == [0, 2, 0, 0, 1, 1]
    # id differences 1, 2, 3 x n_obs 2, 3, 4: threshold 3 (stereo), 2 (monocular)
    assert st[0][6:15].tolist() == [0, 0, 0, 3, 3, 0, 3, 3, 4] and st[1][6:15].tolist() == [0, 0, 0, 3, 0, 0, 3, 4, 4]
    assert st[0][15:18].tolist() == [0, 3, 4]                       # a negative difference; 2 and 3 only after the casts to int
    assert set(st[0].tolist()) == {0, 1, 2, 3, 4}


# ---- the adapter --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", list(A.CONNECTION_ORDERS))
def test_adapter_update_connections_equals_the_reference_style(adapter_prog, tmp_path, order):
    """Ordered connection vectors, weights, parent, children and the AddConnection side effects on the other keyframes: the graph after
    SIVO::UpdateConnections, one keyframe at a time and in the vector form (one C ABI call), is the graph after the stand-ins' own."""
    seq = A.CONNECTION_ORDERS[order]
    (ref, single, vector), calls = A.copies(P.run_prog(adapter_prog, tmp_path, "connections", A.connections_blob(seq)), 3)
    assert ref.tobytes() == single.tobytes() == vector.tobytes()
    assert calls == [len(seq), 1]
    sc = A.connections_scene()
    kfs, pts, used = A.parse_graph(ref, len(sc.kfs), len(sc.points))
    assert used == len(ref)
    # the scene holds a weight tie (resolved by falling pointer) and a keyframe that reaches th with nobody (the fallback)
    index = {kf: k for k, kf in enumerate(sc.kfs)}
    c0 = {index[k]: v for k, v in R.update_connections_counter(sc.kfs[0]).items()}
    c5 = {index[k]: v for k, v in R.update_connections_counter(sc.kfs[5]).items()}
    assert c0 == {1: 20, 2: 20, 3: 17, 4: 3, 6: 15} and c5 == {3: 4, 4: 4}
    if order == "one":
        assert kfs[0]["ordered"] == [2, 1, 3, 6] and kfs[0]["weights"] == [20, 20, 17, 15] and kfs[0]["parent"] == 2 and kfs[0]["first_connection"] == 0
        assert sorted(map(tuple, kfs[0]["connected"])) == sorted(c0.items())
        assert kfs[2]["children"] == [0] and kfs[1]["connected"] == [[0, 20]] and kfs[4]["connected"] == [] and kfs[4]["first_connection"] == 1
    if order == "all":
        assert kfs[5]["ordered"] == [3] and kfs[5]["weights"] == [4] and kfs[5]["parent"] == 3 and [5, 4] in kfs[3]["connected"]
        assert kfs[6]["parent"] == -1 and kfs[6]["first_connection"] == 1 and kfs[6]["ordered"] == [1, 0]      # id 0 takes no parent
        assert kfs[7]["ordered"] == [] and kfs[7]["first_connection"] == 1


@pytest.mark.parametrize("name,mono", [(n, m) for n in A.KF_NAMES for m in ((0, 1) if n in P.KF_MONO else (0,))])
def test_adapter_keyframe_culling_leaves_the_reference_graph(adapter_prog, tmp_path, name, mono):
    (ref, sivo), calls = A.copies(P.run_prog(adapter_prog, tmp_path, "kfcull", A.kfcull_blob(name, mono)), 2)
    assert ref.tobytes() == sivo.tobytes()
    want = P.kf_restatement(name, mono)
    assert calls == [1 if len(want["local"]) else 0]
    kfs, pts, used = A.parse_graph(ref, len(want["scene"].kfs), len(want["scene"].points))
    assert used == len(ref)
    # and that graph is the restatement's: bad keyframes, marked keyframes, bad points, the observation maps, the slots
    sc = want["scene"]
    index = {kf: k for k, kf in enumerate(sc.kfs)}
    assert [k["bad"] for k in kfs] == [int(kf.isBad()) for kf in sc.kfs] and [k["to_be_erased"] for k in kfs] == [int(kf.mbToBeErased) for kf in sc.kfs]
    assert [p["bad"] for p in pts] == want["bad_after"].tolist() and [p["n_obs"] for p in pts] == [p.Observations() for p in sc.points]
    assert [sorted(map(tuple, p["obs"])) for p in pts] == [sorted((index[kf], idx) for kf, idx in p.mObservations.items()) for p in sc.points]
    assert [k["slots"] for k in kfs] == [R.export_slots(sc, kf.mvpMapPoints).tolist() for kf in sc.kfs]


@pytest.mark.parametrize("n,mono", P.MP_RUNS)
def test_adapter_map_point_culling_leaves_the_reference_list(adapter_prog, tmp_path, n, mono):
    (ref, sivo), calls = A.copies(P.run_prog(adapter_prog, tmp_path, "mpcull", A.mpcull_blob(n, mono)), 2)
    assert ref.tobytes() == sivo.tobytes() and calls == [1 if n else 0]
    sc = A.mpcull_scene(n)
    status, kept = R.map_point_culling(sc.points, P.MP_CURRENT, bool(mono))
    kfs, pts, used = A.parse_graph(ref, 2, n)
    assert ref[used] == len(kept) and ref[used + 1:].tolist() == [p.mnId for p in kept]
    assert [p["bad"] for p in pts] == [int(p.isBad()) for p in sc.points]
    assert kfs[0]["slots"] == R.export_slots(sc, sc.kfs[0].mvpMapPoints).tolist()
    if n >= 64:
        assert -1 in kfs[0]["slots"] and set(status) == {0, 1, 2, 3, 4}


def test_adapter_vote_equals_the_reference_style(adapter_prog, tmp_path):
    (ref, sivo), calls = A.copies(P.run_prog(adapter_prog, tmp_path, "vote", A.vote_blob()), 2)
    assert ref.tobytes() == sivo.tobytes() and calls == [1]
    sc, frame = A.vote_scene()
    before = R.export_slots(sc, frame.mvpMapPoints)
    index = {kf: k for k, kf in enumerate(sc.kfs)}
    counter = sorted((index[kf], c) for kf, c in R.vote_local_keyframes(frame).items())
    n = int(ref[0])
    assert n == len(counter) > 5 and ref[1:1 + 2 * n].reshape(-1, 2).tolist() == [list(c) for c in counter]
    after = R.export_slots(sc, frame.mvpMapPoints)
    assert ref[1 + 2 * n:].tolist() == after.tolist() and (before != after).any()        # bad points left the frame


def test_walk_mode_of_the_probe_runs(adapter_prog, tmp_path):
    """The timing mode tools/covis_probe.py drives: four medians in microseconds and a checksum of what the walks left, which does not
    depend on the clock (3 runs x (0 + 4 voted keyframes + 0 + 10 points left in the list + keyframe 0 culled in every run's graphs))."""
    a = np.frombuffer(P.run_prog(adapter_prog, tmp_path, "walk", A.walk_blob(3)), np.float64)
    b = np.frombuffer(P.run_prog(adapter_prog, tmp_path, "walk", A.walk_blob(3)), np.float64)
    assert a.shape == (5,) and np.isfinite(a).all() and (a[:4] >= 0).all() and a[4] == b[4] > 0


# ---- header, exports, ctypes, invalid arguments ------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    h = open(os.path.join(ROOT, "include", "sivo_hip.h")).read()
    assert "int sivo_covis_count(const SivoObsTable *t, int n_sets, const int64_t *set_off, const int32_t *set_point," in h
    assert "int sivo_keyframe_culling(const SivoObsTable *t, int n_local, const int32_t *local_kf, const uint8_t *is_id0," in h
    assert "int sivo_mappoint_culling(int n, const int32_t *found, const int32_t *visible, const int64_t *first_kf_id," in h
    for cite in ("KeyFrame.cc:327-415", "Tracking.cc:1126-1142", "LocalMapping.cc:727-792", "LocalMapping.cc:165-196", "KeyFrame.cc:340-360",
                 "LocalMapping.cc:732-791", "LocalMapping.cc:181-194"):
        assert cite in h, cite                                      # every entry point cites the lines it replaces
    assert "#define SIVO_COVIS_LDS_KF %d" % P.LDS_KF in h
    from sivo_amd import _lib, covisibility
    L = _lib.lib()
    assert all(hasattr(L, n) for n in ("sivo_covis_count", "sivo_keyframe_culling", "sivo_mappoint_culling"))
    assert covisibility.LDS_KF == P.LDS_KF and len(covisibility.DECISION) == 4 and len(covisibility.STATUS) == 5
    assert {"sivo_covis_count", "sivo_keyframe_culling", "sivo_mappoint_culling"} <= set(_lib.SIGNATURES)
    mk = open(os.path.join(ROOT, "sivo_amd", "csrc", "Makefile")).read()
    assert " covis.hip " in mk.split("SRCS =")[1].splitlines()[0]


def test_ctypes_table_matches_the_header(tmp_path):
    from sivo_amd import covisibility
    host_prog.c_layout(tmp_path, "SivoObsTable", covisibility._Table)


def invalid_calls(cov):
    """(what is wrong, a call that must report it): every check of the three entry points, on a small valid scene bent once."""
    t, sets, selfs, _ = P.count_arrays("three_sets")
    kt, local = P.kf_arrays("chain")

    def make(d, **kw):
        d = dict(d, **kw)
        T = cov.ObservationTable.__new__(cov.ObservationTable)
        T.n_kf, T.n_points = int(d["n_kf"]), int(d.get("n_points", len(d["point_bad"])))
        for k in ("obs_off", "obs_kf", "obs_level", "obs_stereo", "point_bad"):
            setattr(T, k, d[k])
        return T

    def bent(x, i, v):
        y = x.copy(); y[i] = v
        return y

    count = lambda T=None, s=sets, me=selfs: cov.shared_counts(T or make(t), s, me)
    cull = lambda T=None, loc=local: cov.keyframe_culling(T or make(kt), loc)
    out = [
        ("obs_off does not start at 0", lambda: count(make(t, obs_off=bent(t["obs_off"], 0, 1)))),
        ("obs_off decreases", lambda: count(make(t, obs_off=bent(t["obs_off"], 3, int(t["obs_off"][4]) + 1)))),
        ("obs_kf outside", lambda: count(make(t, obs_kf=bent(t["obs_kf"], 5, t["n_kf"])))),
        ("obs_kf outside", lambda: count(make(t, obs_kf=bent(t["obs_kf"], 5, -1)))),
        ("null observation array", lambda: count(make(t, obs_level=np.zeros(0, np.uint8)))),
        ("null point_bad", lambda: count(make(t, point_bad=np.zeros(0, np.uint8), n_points=len(t["point_bad"])))),
        ("null obs_off", lambda: count(make(t, obs_off=np.zeros(0, np.int64), n_points=len(t["point_bad"])))),
        ("set_point outside", lambda: count(s=[bent(sets[0], 0, len(t["point_bad"]))] + sets[1:])),
        ("set_point outside", lambda: count(s=[bent(sets[0], 0, -2)] + sets[1:])),
        ("set_self outside", lambda: count(me=bent(selfs, 1, t["n_kf"]))),
        ("set_self outside", lambda: count(me=bent(selfs, 1, -2))),
        ("local_kf outside", lambda: cull(loc=[dict(local[0], kf=kt["n_kf"])] + local[1:])),
        ("local_kf outside", lambda: cull(loc=[dict(local[0], kf=-1)] + local[1:])),
        ("slot_point outside", lambda: cull(loc=[dict(local[0], point=bent(local[0]["point"], 2, len(kt["point_bad"])))] + local[1:])),
        ("slot_point outside", lambda: cull(loc=[dict(local[0], point=bent(local[0]["point"], 2, -2))] + local[1:])),
        ("obs_off decreases", lambda: cull(make(kt, obs_off=bent(kt["obs_off"], 2, 0)))),
        ("obs_kf outside", lambda: cull(make(kt, obs_kf=bent(kt["obs_kf"], 0, kt["n_kf"])))),
    ]
    return out


def test_entry_points_check_arguments_and_fail_loudly_without_a_device():
    """Every invalid argument is reported as such — SIVO_ERR_INVALID_ARGUMENT, a ValueError here — before any device is needed: this
    test runs where there is none.  Raw calls cover what the Python layer cannot express (offsets of a set list, negative counts)."""
    from sivo_amd import _lib, covisibility as cov
    for what, call in invalid_calls(cov):
        with pytest.raises(ValueError, match=what):
            call()
    L = _lib.lib()
    t, sets, selfs, _ = P.count_arrays("three_sets")
    T = cov.ObservationTable(t["n_kf"], t["obs_off"], t["obs_kf"], t["obs_level"], t["obs_stereo"], t["point_bad"])
    st = T.struct()
    neg_kf, neg_points = T.struct(), T.struct()
    neg_kf.n_kf, neg_points.n_points = -1, -1
    off, pts = P.csr(sets, np.int32)
    counts = np.zeros((3, t["n_kf"]), np.int32)
    p = lambda x: x.ctypes.data
    off1, off_dec, soff_dec = off + 1, np.array([0, 9, 5, 10], np.int64), np.array([0, 12, 3], np.int64)      # (kept alive over the calls)
    bad_calls = {
        "set_off does not start at 0": lambda: L.sivo_covis_count(C.byref(st), 3, p(off1), p(pts), p(selfs), p(counts)),
        "set_off decreases": lambda: L.sivo_covis_count(C.byref(st), 3, p(off_dec), p(pts), p(selfs), p(counts)),
        "negative count": lambda: L.sivo_covis_count(C.byref(st), -1, p(off), p(pts), p(selfs), p(counts)),
        "null set_off": lambda: L.sivo_covis_count(C.byref(st), 3, None, p(pts), p(selfs), p(counts)),
        "null set_point": lambda: L.sivo_covis_count(C.byref(st), 3, p(off), None, p(selfs), p(counts)),
        "null set_self": lambda: L.sivo_covis_count(C.byref(st), 3, p(off), p(pts), None, p(counts)),
        "null counts": lambda: L.sivo_covis_count(C.byref(st), 3, p(off), p(pts), p(selfs), None),
        "negative count   ": lambda: L.sivo_covis_count(C.byref(neg_kf), 3, p(off), p(pts), p(selfs), p(counts)),
        "negative count    ": lambda: L.sivo_covis_count(C.byref(neg_points), 3, p(off), p(pts), p(selfs), p(counts)),
        "null table": lambda: L.sivo_covis_count(None, 3, p(off), p(pts), p(selfs), p(counts)),
    }
    kt, local = P.kf_arrays("chain")
    KT = cov.ObservationTable(kt["n_kf"], kt["obs_off"], kt["obs_kf"], kt["obs_level"], kt["obs_stereo"], kt["point_bad"])
    kst = KT.struct()
    K = len(local)
    kf = np.array([k["kf"] for k in local], np.int32); flags = np.ones(K, np.uint8); th = np.full(K, 40, np.float32)
    soff, spt = P.csr([k["point"] for k in local], np.int32)
    _, slv = P.csr([k["level"] for k in local], np.uint8)
    _, sdp = P.csr([k["depth"] for k in local], np.float32)
    soff1 = soff + 1
    o32, o8, bad = np.zeros(K, np.int32), np.zeros(K, np.uint8), np.zeros(KT.n_points, np.uint8)
    kc = lambda n=K, kf_=p(kf), off_=p(soff), pt_=p(spt), lv_=p(slv), out_=p(o32), bad_=p(bad): L.sivo_keyframe_culling(
        C.byref(kst), n, kf_, p(flags), p(flags), p(th), off_, pt_, lv_, p(sdp), 0, out_, p(o32), p(o8), bad_)
    bad_calls.update({
        "negative count ": lambda: kc(n=-1),
        "slot_off does not start at 0": lambda: kc(off_=p(soff1)),
        "slot_off decreases": lambda: kc(off_=p(soff_dec)),
        "null local_kf": lambda: kc(kf_=None),
        "null slot_off": lambda: kc(off_=None),
        "null slot_point": lambda: kc(pt_=None),
        "null slot array": lambda: kc(lv_=None),
        "null keyframe array": lambda: kc(out_=None),
        "null bad_after": lambda: kc(bad_=None),
    })
    a = R.export_recent(P.mp_objects(5))
    status = np.zeros(5, np.uint8)
    mc = lambda n=5, f=p(a["found"]), s=p(status): L.sivo_mappoint_culling(n, f, p(a["visible"]), p(a["first_kf_id"]), p(a["n_obs"]), p(a["bad"]), 10, 0, s)
    bad_calls.update({"negative count  ": lambda: mc(n=-1), "null array": lambda: mc(f=None), "null array ": lambda: mc(s=None)})
    for what, call in bad_calls.items():
        assert call() == _lib.ERR_INVALID_ARGUMENT, what
        assert what.strip() in L.sivo_last_error().decode(), (what, L.sivo_last_error())
    # zero work needs no device either, and writes what the ABI says
    assert L.sivo_covis_count(C.byref(st), 0, None, None, None, None) == 0
    assert L.sivo_mappoint_culling(0, None, None, None, None, None, 10, 0, None) == 0
    bad[:] = 9
    assert L.sivo_keyframe_culling(C.byref(kst), 0, None, None, None, None, None, None, None, None, 0, None, None, None, p(bad)) == 0
    assert np.array_equal(bad, kt["point_bad"])
    no_slots = np.zeros(4, np.int64)
    counts[:] = 9
    assert L.sivo_covis_count(C.byref(st), 3, p(no_slots), None, p(selfs), p(counts)) == 0 and not counts.any()
    # real work without a device is an error, never a silent fallback
    if L.sivo_device_count() < 1:
        with pytest.raises(RuntimeError, match="no HIP device"):
            cov.shared_counts(T, sets, selfs)
        with pytest.raises(RuntimeError, match="no HIP device"):
            cov.keyframe_culling(KT, local)
        with pytest.raises(RuntimeError, match="no HIP device"):
            cov.map_point_culling(a["found"], a["visible"], a["first_kf_id"], a["n_obs"], a["bad"], 10)


# ---- the sanitizer build -----------------------------------------------------------------------------------------------------------
def test_sanitizer_builds_of_both_programs_agree(prog, adapter_prog, tmp_path, tmp_path_factory):
    """Both stand-alone programs built a second time with -fsanitize=address,undefined and run directly (each has its own main: nothing
    is preloaded) on a cut of the scenes: the same bytes as the plain build, and no report."""
    san_dir = tmp_path_factory.mktemp("covis_prog_san")
    if not host_prog.sanitizer_runtime_present(san_dir):
        pytest.skip("the sanitizer runtime (libasan / libubsan) is not installed: a trivial main does not link with -fsanitize")
    san = host_prog.build("covis_prog", san_dir, sanitize=True)
    for name in ("n_kf_1", "n_kf_65", "lds_bound_%d" % (P.LDS_KF + 1), "set_sizes", "one_counter"):
        t, sets, selfs, _ = P.count_arrays(name)
        blob = P.count_blob(t, sets, selfs)
        assert P.run_prog(prog, tmp_path, "count", blob) == P.run_prog(san, tmp_path, "count", blob), name
    for name, mono in P.KF_RUNS:
        t, local = P.kf_arrays(name)
        blob = P.kfcull_blob(t, local, mono)
        assert P.run_prog(prog, tmp_path, "kfcull", blob) == P.run_prog(san, tmp_path, "kfcull", blob), name
    for n, mono in P.MP_RUNS:
        blob = P.mpcull_blob(R.export_recent(P.mp_objects(n)), P.MP_CURRENT, mono)
        assert P.run_prog(prog, tmp_path, "mpcull", blob) == P.run_prog(san, tmp_path, "mpcull", blob)
    asan = host_prog.build("covis_adapter_prog", san_dir, sanitize=True)
    for mode, blob in A.all_blobs():
        assert P.run_prog(adapter_prog, tmp_path, mode, blob) == P.run_prog(asan, tmp_path, mode, blob), mode
    walk = [np.frombuffer(P.run_prog(e, tmp_path, "walk", A.walk_blob(2)), np.float64) for e in (adapter_prog, asan)]
    assert walk[0][4] == walk[1][4]                                 # (the times differ; what the walks left does not)
