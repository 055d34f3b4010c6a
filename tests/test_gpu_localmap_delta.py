"""sivo_localmap_apply / _sizes / _export (sivo_amd/csrc/localmap.hip) through sivo_amd/local_map.py on the device: every scene of
tests/localmap_delta_cases.py byte for byte against the list-of-rows restatement (tests/localmap_delta_restatement.py) and the host build
of the same per-item bodies (tests/localmap_delta_prog.cpp) — the export after apply, and the update on the applied handle — and what stays
on the device between the calls.  Every comparison is an equality.  Reads only tests/."""
import numpy as np
import pytest

import host_prog
import localmap_cases as P
import localmap_delta_cases as Q
import localmap_delta_restatement as D
from test_gpu_localmap import device_update, tables_of
from test_localmap_delta_host import refusals, scene_ops, second_delta

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lm():
    from sivo_amd import local_map
    return local_map


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return host_prog.build("localmap_delta_prog", tmp_path_factory.mktemp("localmap_delta_prog_gpu"))


def apply(h, d):
    h.apply(d["n_kf"], d["n_points"], point_rows=d["point_rows"], kf_rows=d["kf_rows"], kf_order=d["kf_order"])


def sizes_of(t):
    return (t["n_kf"], len(t["point_bad"]), len(t["obs_kf"]), len(t["slot_point"]), len(t["covis_kf"]), len(t["child_kf"]))


@pytest.mark.parametrize("name", list(Q.CASES))
def test_scene(lm, prog, tmp_path, name):
    before, delta, after, call, want, _ = Q.arrays(name)
    host = Q.run_ops(prog, tmp_path, scene_ops(name))
    with lm.LocalMap(before["n_kf"], **tables_of(before)) as h:
        apply(h, delta)
        got_sizes, got_tables = h.sizes(), h.export()
        got = device_update(h, after["n_kf"], call)
        assert (h.n_kf, h.n_points, h._slot_off.tolist()) == (after["n_kf"], len(after["point_bad"]), after["slot_off"].tolist())
    assert [r["rc"] for r in host] == [0] * 7
    assert got_sizes == sizes_of(after) == host[2]["sizes"]
    assert Q.differing(got_tables, after) == [] and Q.differing(got_tables, host[2]["tables"]) == []
    assert P.same(got, want) == [] and P.same(got, host[3]) == []


def test_two_deltas_equal_a_fresh_handle(lm):
    """A -> apply B -> apply C equals a fresh handle on C: the second apply reads what the first wrote into the other buffer and writes
    over the buffer A was created in.  A third, empty delta changes nothing."""
    a, d1, b, call = Q.arrays("points_600")[:4]
    d2 = second_delta(b)
    c = D.apply(b, d2)
    empty = dict(Q.arrays("empty_delta")[1], n_kf=c["n_kf"], n_points=len(c["point_bad"]))
    with lm.LocalMap(a["n_kf"], **tables_of(a)) as h, lm.LocalMap(c["n_kf"], **tables_of(c)) as fresh:
        apply(h, d1)
        assert Q.differing(h.export(), b) == []
        apply(h, d2)
        apply(h, empty)
        assert h.sizes() == fresh.sizes() == sizes_of(c)
        assert Q.differing(h.export(), c) == [] and Q.differing(fresh.export(), c) == []
        assert P.same(device_update(h, c["n_kf"], call), device_update(fresh, c["n_kf"], call)) == []


def test_apply_then_set_bad_then_replace(lm):
    """apply followed by set_bad equals a fresh handle with those flags (appended rows among them); replace after apply gives the
    replaced tables."""
    a, d1, b, call = Q.arrays("points_257")[:4]
    flagged = dict(b, point_bad=b["point_bad"].copy(), kf_bad=b["kf_bad"].copy())
    flagged["point_bad"][[5, 256]] = 1 - flagged["point_bad"][[5, 256]]
    flagged["kf_bad"][[2, 12]] = 1 - flagged["kf_bad"][[2, 12]]
    other, other_call, other_want = Q.arrays("order_given")[2], Q.arrays("order_given")[3], Q.arrays("order_given")[4]
    with lm.LocalMap(a["n_kf"], **tables_of(a)) as h, lm.LocalMap(b["n_kf"], **tables_of(flagged)) as fresh:
        apply(h, d1)
        h.set_bad([5, 256], flagged["point_bad"][[5, 256]], [2, 12], flagged["kf_bad"][[2, 12]])
        assert Q.differing(h.export(), flagged) == []
        assert P.same(device_update(h, b["n_kf"], call), device_update(fresh, b["n_kf"], call)) == []
        h.replace(other["n_kf"], **tables_of(other))
        assert Q.differing(h.export(), other) == [] and h.sizes() == sizes_of(other)
        assert P.same(device_update(h, other["n_kf"], other_call), other_want) == []


def test_apply_on_a_second_handle_leaves_the_first(lm):
    a, d1, b, call, want = Q.arrays("long_rows")[:5]
    a2, d2, b2 = Q.arrays("all_rows")[:3]
    with lm.LocalMap(a["n_kf"], **tables_of(a)) as h, lm.LocalMap(a2["n_kf"], **tables_of(a2)) as second:
        apply(h, d1)
        first = h.export()
        apply(second, d2)
        assert Q.differing(h.export(), first) == [] and Q.differing(first, b) == [] and Q.differing(second.export(), b2) == []
        assert P.same(device_update(h, b["n_kf"], call), want) == []


def test_appended_keyframe_larger_than_the_old_map(lm, prog, tmp_path):
    """An appended keyframe with more slots than the whole old map, and a frame that votes for it: the grids of the point passes come
    from the new total slot count, or its points past the old total would be missing."""
    a = Q.arrays("first_and_last")[0]
    K, Pn, old_slots = a["n_kf"], len(a["point_bad"]), int(a["slot_off"][-1])
    n_new = max(3 * old_slots, 3 * 256) + 5                         # several blocks of the point passes past the old bound
    pr = dict(idx=np.arange(Pn, Pn + n_new, dtype=np.int32), bad=np.zeros(n_new, np.uint8), obs_off=np.arange(n_new + 1, dtype=np.int64),
              obs_kf=np.full(n_new, K, np.int32))
    kr = dict(idx=np.array([K], np.int32), bad=np.zeros(1, np.uint8), parent=np.array([-1], np.int32), slot_off=np.array([0, n_new], np.int64),
              slot_point=np.arange(Pn, Pn + n_new, dtype=np.int32), covis_off=np.zeros(2, np.int64), covis_kf=np.zeros(0, np.int32),
              child_off=np.zeros(2, np.int64), child_kf=np.zeros(0, np.int32))
    d = dict(n_kf=K + 1, n_points=Pn + n_new, point_rows=pr, kf_rows=kr, kf_order=None)
    after = D.apply(a, d)
    call = dict(frame_point=np.array([Pn + n_new - 1, -1, Pn], np.int32), kf_premarked=np.zeros(0, np.int32), point_premarked=np.zeros(0, np.int32),
                prev_local_kf=np.zeros(0, np.int32), kf_capacity=K + 1, point_capacity=Pn + n_new)
    host = Q.run_ops(prog, tmp_path, [P.op_create(after), P.op_update(call, K + 1)])[1]
    with lm.LocalMap(K, **tables_of(a)) as h:
        apply(h, d)
        got = device_update(h, K + 1, call)
    assert host["rc"] == 0 and host["n_local_points"] == n_new > old_slots and host["local_kf"][0] == K
    assert P.same(got, host) == [] and got["local_point"][n_new - 1] == Pn + n_new - 1


def test_a_refused_delta_leaves_the_export(lm):
    from sivo_amd import _lib
    before = Q.arrays("points_257")[0]
    with lm.LocalMap(before["n_kf"], **tables_of(before)) as h:
        first = h.export()
        for what, bad, counts in refusals():
            if counts or any(v is None for v in list(bad["point_rows"].values()) + list(bad["kf_rows"].values())):
                continue                                            # (counts and NULL arrays are not the Python layer's to bend: the host build has them)
            with pytest.raises((ValueError, _lib.SivoError), match=what.split("(")[0]):
                apply(h, bad)
            assert Q.differing(h.export(), first) == [] and (h.n_kf, h.n_points) == (before["n_kf"], len(before["point_bad"])), what
        assert Q.differing(first, before) == []
