"""The local-map kernels (sivo_amd/csrc/localmap.hip) through sivo_amd/local_map.py on the device: every scene of tests/localmap_cases.py, byte
for byte against the host build of the same per-item bodies (tests/localmap_prog.cpp) and the object-graph restatement of the reference
(tests/localmap_restatement.py) — voted, slot_cleared, local_kf, ref_kf, local_point, counts, in sentinel-filled arrays — and what stays on
the device between the calls.  Every comparison is an equality.  Reads only tests/."""
import numpy as np
import pytest

import host_prog
import localmap_cases as P

pytestmark = pytest.mark.gpu
S = P.SENTINEL


@pytest.fixture(scope="module")
def lm():
    from sivo_amd import local_map
    return local_map


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return host_prog.build("localmap_prog", tmp_path_factory.mktemp("localmap_prog_gpu"))


def tables_of(t):
    return {k: v for k, v in t.items() if k != "n_kf"}


def device_update(handle, n_kf, call, kf_capacity=None, point_capacity=None):
    """One update into sentinel-filled arrays; the outputs in the form of localmap_cases.OUTPUTS."""
    kc = call["kf_capacity"] if kf_capacity is None else kf_capacity
    pc = call["point_capacity"] if point_capacity is None else point_capacity
    out = dict(slot_cleared=np.full(len(call["frame_point"]), 255, np.uint8), local_kf=np.full(kc, S, np.int32), local_point=np.full(pc, S, np.int32),
               counts=np.full(n_kf, S, np.int32))
    r = handle.update(call["frame_point"], call["kf_premarked"], call["point_premarked"], call["prev_local_kf"], kf_capacity=kc, point_capacity=pc, out=out)
    return dict(voted=int(r.voted), n_local_kf=len(r.local_kf) if r.voted else S, ref_kf=r.ref_kf, n_local_points=len(r.local_points), **out)


@pytest.mark.parametrize("name", list(P.CASES))
def test_scene(lm, prog, tmp_path, name):
    tables, call, want, _ = P.arrays(name)
    host = P.host_update(prog, tmp_path, tables, call)
    with lm.LocalMap(tables["n_kf"], **tables_of(tables)) as h:
        got = device_update(h, tables["n_kf"], call)
    assert host["rc"] == 0 and P.same(host, want) == [] and P.same(got, want) == []


def test_a_handle_does_not_remember_its_calls(lm):
    """A, then B on a second handle, then A again on the first: the same bytes as the first time; and two frames on one handle each
    equal a fresh handle's."""
    ta, ca, wa, _ = P.arrays("random_40x60")
    tb, cb, wb, _ = P.arrays("blocks_769")
    with lm.LocalMap(ta["n_kf"], **tables_of(ta)) as a, lm.LocalMap(tb["n_kf"], **tables_of(tb)) as b:
        first = device_update(a, ta["n_kf"], ca)
        assert P.same(device_update(b, tb["n_kf"], cb), wb) == []
        again = device_update(a, ta["n_kf"], ca)
        assert P.same(first, wa) == [] and P.same(again, first) == []
        # another frame on the same handle: the frame's slots reversed and thinned, other premarks, the caller's list the other way round
        other = dict(ca, frame_point=ca["frame_point"][::-2].copy(), kf_premarked=np.array([0, 5], np.int32),
                     point_premarked=ca["point_premarked"][:3].copy(), prev_local_kf=ca["prev_local_kf"][::-1].copy())
        second = device_update(a, ta["n_kf"], other)
        third = device_update(a, ta["n_kf"], ca)
    with lm.LocalMap(ta["n_kf"], **tables_of(ta)) as fresh:
        assert P.same(second, device_update(fresh, ta["n_kf"], other)) == []
    assert P.same(third, wa) == [] and second["local_point"].tobytes() != first["local_point"].tobytes()


@pytest.mark.parametrize("a,b", [("random_40x60", "premarked"), ("premarked", "random_40x60")])
def test_replace_gives_the_new_tables_results(lm, a, b):
    """B's tables into A's handle, B smaller than A and B larger than A: B's results."""
    ta, ca, wa, _ = P.arrays(a)
    tb, cb, wb, _ = P.arrays(b)
    with lm.LocalMap(ta["n_kf"], **tables_of(ta)) as h:
        assert P.same(device_update(h, ta["n_kf"], ca), wa) == []
        h.replace(tb["n_kf"], **tables_of(tb))
        assert P.same(device_update(h, tb["n_kf"], cb), wb) == []


def test_set_bad_equals_a_fresh_handle_with_those_flags(lm, prog, tmp_path):
    tables, call, _, _ = P.arrays("random_40x60")
    pts, kfs = np.array([3, 40, 41, 3], np.int32), np.array([16, 2, 31], np.int32)
    pv, kv = np.array([1, 1, 0, 0], np.uint8), np.array([1, 0, 1], np.uint8)       # point 3 is listed twice: the later entry holds
    flagged = dict(tables, point_bad=tables["point_bad"].copy(), kf_bad=tables["kf_bad"].copy())
    flagged["point_bad"][[40, 41, 3]] = [1, 0, 0]
    flagged["kf_bad"][kfs] = kv
    assert (flagged["kf_bad"] != tables["kf_bad"]).any() and (flagged["point_bad"] != tables["point_bad"]).any()
    with lm.LocalMap(tables["n_kf"], **tables_of(tables)) as h, lm.LocalMap(tables["n_kf"], **tables_of(flagged)) as fresh:
        before = device_update(h, tables["n_kf"], call)
        h.set_bad(pts, pv, kfs, kv)
        after = device_update(h, tables["n_kf"], call)
        want = device_update(fresh, tables["n_kf"], call)
    host = P.host_update(prog, tmp_path, flagged, call)
    assert P.same(after, want) == [] and P.same(after, host) == [] and P.same(after, before) != []


@pytest.mark.parametrize("which", ["kf", "point"])
def test_capacity_one_too_small_writes_nothing(lm, which):
    from sivo_amd import _lib
    tables, call, want, _ = P.arrays("random_40x60")
    kc = want["n_local_kf"] - (which == "kf")
    pc = want["n_local_points"] - (which == "point")
    with lm.LocalMap(tables["n_kf"], **tables_of(tables)) as h:
        out = dict(slot_cleared=np.full(len(call["frame_point"]), 255, np.uint8), local_kf=np.full(kc, S, np.int32),
                   local_point=np.full(pc, S, np.int32), counts=np.full(tables["n_kf"], S, np.int32))
        with pytest.raises(_lib.SivoError, match="capacity %d" % (kc if which == "kf" else pc)) as e:
            h.update(call["frame_point"], call["kf_premarked"], call["point_premarked"], call["prev_local_kf"], kf_capacity=kc, point_capacity=pc, out=out)
        assert "error %d" % _lib.ERR_CAPACITY in str(e.value)
        assert (out["slot_cleared"] == 255).all() and all((out[k] == S).all() for k in ("local_kf", "local_point", "counts"))
        exact = device_update(h, tables["n_kf"], call, kf_capacity=want["n_local_kf"], point_capacity=want["n_local_points"])      # and exactly enough is enough
    assert exact["local_kf"].tobytes() == want["local_kf"][:want["n_local_kf"]].tobytes()
    assert exact["local_point"].tobytes() == want["local_point"][:want["n_local_points"]].tobytes()
