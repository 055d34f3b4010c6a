"""sivo_localmap_ba_window (sivo_amd/csrc/ba_window.hip) through sivo_amd/local_map.py on the device: every scene of
tests/ba_window_cases.py byte for byte against the line-by-line restatement of Optimizer.cc:496-559 and :651-670
(tests/ba_window_restatement.py), what stays on the handle between the calls, the capacity refusal, and a window handed to sivo_local_ba.
Every comparison is an equality.  Reads only tests/."""
import numpy as np
import pytest

import ba_window_cases as P
import localmap_delta_restatement as D
import localmap_restatement as R
from test_gpu_localmap import tables_of

pytestmark = pytest.mark.gpu
S = P.SENTINEL
CAPACITY = 5                                                        # SIVO_ERR_CAPACITY


@pytest.fixture(scope="module")
def lm():
    from sivo_amd import local_map
    return local_map


def device_window(handle, call, **caps):
    """One call of the C entry point into sentinel-filled arrays: rc and the outputs in the form of ba_window_cases.OUTPUTS."""
    from sivo_amd import _lib
    kc, pc, ec = (caps.get(k, call[k]) for k in ("kf_capacity", "point_capacity", "edge_capacity"))
    out = dict(counts=np.full(4, S, np.int64), local_kf=np.full(kc, S, np.int32), fixed_kf=np.full(kc, S, np.int32), local_point=np.full(pc, S, np.int32),
               edge_off=np.full(pc + 1, S, np.int64), edge_pose=np.full(ec, S, np.int32), edge_slot=np.full(ec, S, np.int32))
    lists = [np.ascontiguousarray(call[k], np.int32) for k in ("cand_kf", "kf_local_pre", "kf_fixed_pre", "point_pre")]
    p = lambda a: a.ctypes.data if a.size else None
    rc = _lib.lib().sivo_localmap_ba_window(handle._h, len(lists[0]), p(lists[0]), len(lists[1]), p(lists[1]), len(lists[2]), p(lists[2]), len(lists[3]),
                                            p(lists[3]), kc, p(out["local_kf"]), p(out["fixed_kf"]), pc, p(out["local_point"]), out["edge_off"].ctypes.data,
                                            ec, p(out["edge_pose"]), p(out["edge_slot"]), out["counts"].ctypes.data)
    return dict(out, rc=rc, message=_lib.lib().sivo_last_error().decode() if rc else "")


@pytest.mark.parametrize("name", list(P.CASES))
def test_scene(lm, name):
    """Every output in sentinel-filled arrays, twice on one handle: the second call sees nothing of the first; and the Python method
    returns the same lists cut at the counts."""
    tables, call, want = P.arrays(name)
    with lm.LocalMap(tables["n_kf"], **tables_of(tables)) as h:
        first, second = device_window(h, call), device_window(h, call)
        lists = h.ba_window(call["cand_kf"], call["kf_local_pre"], call["kf_fixed_pre"], call["point_pre"])
    assert first["rc"] == 0 and P.same(first, want) == []
    assert second["rc"] == 0 and P.same(second, first) == []
    nl, npt, nf, ne = (int(v) for v in want["counts"])
    cut = (want["local_kf"][:nl], want["fixed_kf"][:nf], want["local_point"][:npt], want["edge_off"][:npt + 1], want["edge_pose"][:ne], want["edge_slot"][:ne])
    assert [a.tobytes() for a in lists] == [a.tobytes() for a in cut] and [a.dtype for a in lists] == [a.dtype for a in cut]


def appended_pkf(before):
    """A delta that appends keyframe K — it holds three old points and a new one, which keyframe 7 observes too — and the call that makes
    it pKF."""
    K, Pn = before["n_kf"], len(before["point_bad"])
    old = [3, 10, 25]
    rows = [before["obs_kf"][before["obs_off"][p]:before["obs_off"][p + 1]].tolist() + [K] for p in old] + [[7, K]]
    obs_off, obs_kf = R.csr(rows, np.int32)
    pr = dict(idx=np.array(old + [Pn], np.int32), bad=np.zeros(4, np.uint8), obs_off=obs_off, obs_kf=obs_kf)
    kr = dict(idx=np.array([K], np.int32), bad=np.zeros(1, np.uint8), parent=np.array([-1], np.int32), slot_off=np.array([0, 5], np.int64),
              slot_point=np.array([3, -1, 10, Pn, 25], np.int32), covis_off=np.array([0, 3], np.int64), covis_kf=np.array([4, 9, 2], np.int32),
              child_off=np.zeros(2, np.int64), child_kf=np.zeros(0, np.int32))
    delta = dict(n_kf=K + 1, n_points=Pn + 1, point_rows=pr, kf_rows=kr, kf_order=None)
    empty = np.zeros(0, np.int32)
    call = dict(cand_kf=np.array([K, 4, 9, 2], np.int32), kf_local_pre=empty, kf_fixed_pre=empty, point_pre=empty)
    return delta, call


def test_set_bad_and_apply_equal_a_fresh_handle(lm):
    """After set_bad, and after apply of a delta whose appended keyframe becomes pKF, the resident handle answers as a handle created
    from the edited tables."""
    tables, call, want = P.arrays("random_a")
    flagged = dict(tables, point_bad=tables["point_bad"].copy(), kf_bad=tables["kf_bad"].copy())
    kfs, pts = [int(want["local_kf"][1]), int(want["fixed_kf"][0])], [int(want["local_point"][0]), int(want["local_point"][5])]
    flagged["kf_bad"][kfs] = 1
    flagged["point_bad"][pts] = 1
    delta, call2 = appended_pkf(flagged)
    after = D.apply(flagged, delta)
    call2.update(P.capacities(after))
    with lm.LocalMap(tables["n_kf"], **tables_of(tables)) as h, lm.LocalMap(tables["n_kf"], **tables_of(flagged)) as fresh, \
            lm.LocalMap(after["n_kf"], **tables_of(after)) as fresh2:
        plain = device_window(h, call)
        h.set_bad(pts, [1, 1], kfs, [1, 1])
        got, ref = device_window(h, call), device_window(fresh, call)
        assert got["rc"] == ref["rc"] == 0 and P.same(got, ref) == [] and P.same(got, plain) != [] and P.same(plain, want) == []
        h.apply(delta["n_kf"], delta["n_points"], point_rows=delta["point_rows"], kf_rows=delta["kf_rows"], kf_order=delta["kf_order"])
        got2, ref2 = device_window(h, call2), device_window(fresh2, call2)
        assert got2["rc"] == ref2["rc"] == 0 and P.same(got2, ref2) == []
        assert got2["local_kf"][0] == tables["n_kf"] and got2["counts"][1] > 4 and len(tables["point_bad"]) in got2["local_point"]


def test_capacity_refusal_and_retry(lm):
    """One entry too few in each capacity: SIVO_ERR_CAPACITY, the four counts and nothing else; the Python method raises with the
    counts, and a second call sized by them succeeds."""
    tables, call, want = P.arrays("random_b")
    nl, npt, nf, ne = (int(v) for v in want["counts"])
    assert nf > nl                                                  # (the keyframe capacity serves both lists)
    with lm.LocalMap(tables["n_kf"], **tables_of(tables)) as h:
        for caps in (dict(kf_capacity=nf - 1), dict(point_capacity=npt - 1), dict(edge_capacity=ne - 1)):
            res = device_window(h, call, **caps)
            assert res["rc"] == CAPACITY and "capacity %d" % list(caps.values())[0] in res["message"]
            assert res["counts"].tolist() == [nl, npt, nf, ne]
            assert all((res[k] == S).all() for k in P.OUTPUTS if k != "counts")
            with pytest.raises(lm.WindowCapacity) as err:
                h.ba_window(call["cand_kf"], call["kf_local_pre"], call["kf_fixed_pre"], call["point_pre"], **caps)
            assert err.value.counts == (nl, npt, nf, ne)
        res = device_window(h, call, kf_capacity=nf, point_capacity=npt, edge_capacity=ne)
        assert res["rc"] == 0
        for k in P.OUTPUTS:
            assert res[k].tobytes() == want[k][:len(res[k])].tobytes(), k
        lists = h.ba_window(call["cand_kf"], call["kf_local_pre"], call["kf_fixed_pre"], call["point_pre"], kf_capacity=nf, point_capacity=npt,
                            edge_capacity=ne)
        assert [len(a) for a in lists] == [nl, nf, npt, npt + 1, ne, ne]


def test_refusals_on_a_live_handle(lm):
    """The argument check of a handle that exists: the message, SIVO_ERR_INVALID_ARGUMENT as a ValueError, and nothing written."""
    tables, call, _ = P.arrays("random_a")
    K, Pn = tables["n_kf"], len(tables["point_bad"])
    cand = call["cand_kf"]
    with lm.LocalMap(K, **tables_of(tables)) as h:
        for what, args in [("cand_kf lists a keyframe twice", (np.append(cand, cand[1]),)), ("cand_kf outside", (np.append(cand, K),)),
                           ("n_cand < 1", ([],)), ("kf_local_pre outside", (cand, [K])), ("kf_fixed_pre outside", (cand, [], [-1])),
                           ("point_pre outside", (cand, [], [], [Pn])), ("negative count", (cand, [], [], [], dict(kf_capacity=-1)))]:
            kw = args[4] if len(args) > 4 else {}
            with pytest.raises(ValueError, match="sivo_localmap_ba_window: " + what):
                h.ba_window(*args[:4], **kw)
        res = device_window(h, dict(call, cand_kf=np.append(cand, cand[0])))
        assert res["rc"] == 1 and all((res[k] == S).all() for k in P.OUTPUTS)


def test_window_feeds_local_ba(lm):
    """The arrays of sivo_local_ba made from the device's window and from the restatement's are the same bytes, and so is what the
    solver makes of them."""
    from sivo_amd import optimizer
    tables, call, want = P.arrays("random_a")
    with lm.LocalMap(tables["n_kf"], **tables_of(tables)) as h:
        got = device_window(h, call)
    a, b = P.solver_arrays(got), P.solver_arrays(want)
    assert [np.asarray(x).tobytes() for x in a] == [np.asarray(x).tobytes() for x in b] and len(a[3]) == int(want["counts"][3]) > 100
    ra, rb = optimizer.local_ba(*a), optimizer.local_ba(*b)
    for k in ("poses", "points", "outlier", "cov"):
        assert ra[k].tobytes() == rb[k].tobytes(), k
    assert (ra["iterations"], ra["trials"]) == (rb["iterations"], rb["trials"]) and ra["iterations"] > 0
    assert np.isfinite(ra["poses"]).all() and not np.array_equal(ra["poses"], a[0])
