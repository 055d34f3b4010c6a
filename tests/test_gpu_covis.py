"""The covisibility kernels (sivo_amd/csrc/covis.hip) through sivo_amd/covisibility.py on the device: every scene of tests/covis_cases.py,
byte for byte against the host build of the same per-slot bodies (tests/covis_prog.cpp) and the object-graph restatement of the
reference (tests/covis_restatement.py) — counts, n_mps, n_redundant, decision, bad_after, status.  Reads only tests/."""
import numpy as np
import pytest

import covis_cases as P
import covis_restatement as R
import host_prog

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cov():
    from sivo_amd import covisibility
    return covisibility


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return host_prog.build("covis_prog", tmp_path_factory.mktemp("covis_prog_gpu"))


def table_of(cov, t):
    return cov.ObservationTable(t["n_kf"], t["obs_off"], t["obs_kf"], t["obs_level"], t["obs_stereo"], t["point_bad"])


@pytest.mark.parametrize("name", list(P.COUNT_CASES))
def test_counts(cov, prog, tmp_path, name):
    t, sets, selfs, want = P.count_arrays(name)
    rc, host = P.host_count(prog, tmp_path, t, sets, selfs)
    out = np.full((len(sets), t["n_kf"]), -7, np.int32)            # every entry is the call's: none keeps the -7
    got = cov.shared_counts(table_of(cov, t), sets, selfs, out=out)
    assert rc == 0 and got.tobytes() == host.tobytes() == want.tobytes()
    if name == "three_sets":                                        # several sets in one launch equal the single launches
        for s in range(len(sets)):
            assert np.array_equal(cov.shared_counts(table_of(cov, t), sets[s:s + 1], selfs[s:s + 1])[0], want[s])


@pytest.mark.parametrize("name,mono", P.KF_RUNS)
def test_keyframe_culling(cov, prog, tmp_path, name, mono):
    t, local = P.kf_arrays(name)
    want = P.kf_restatement(name, mono)
    host = P.host_kfcull(prog, tmp_path, t, local, mono)
    K = len(local)
    got = cov.keyframe_culling(table_of(cov, t), local, monocular=bool(mono),
                               out=dict(n_mps=np.full(K, P.SENTINEL, np.int32), n_redundant=np.full(K, P.SENTINEL, np.int32)))
    assert host["rc"] == 0
    for k in ("decision", "n_mps", "n_redundant", "bad_after"):     # a keyframe skipped as id 0 keeps the caller's -7 in all three
        assert got[k].tobytes() == host[k].tobytes() == want[k].tobytes(), k
    assert [cov.DECISION[d] for d in (0, 1, 2, 3)] == ["kept", "culled", "to_be_erased", "id0"]


def test_keyframe_culling_twice_gives_the_same(cov):
    """Nothing stays on the device between calls: the removed flags and the bad bytes of one call do not reach the next."""
    t, local = P.kf_arrays("family_2")
    a = cov.keyframe_culling(table_of(cov, t), local)
    t2, local2 = P.kf_arrays("chain")
    b = cov.keyframe_culling(table_of(cov, t2), local2)
    c = cov.keyframe_culling(table_of(cov, t), local)
    assert all(a[k].tobytes() == c[k].tobytes() for k in a) and b["decision"].tolist() == [1, 0]


@pytest.mark.parametrize("n,mono", P.MP_RUNS)
def test_map_point_culling(cov, prog, tmp_path, n, mono):
    want, _, _ = P.mp_restatement(n, mono)
    a = R.export_recent(P.mp_objects(n))
    rc, host = P.host_mpcull(prog, tmp_path, a, P.MP_CURRENT, mono)
    got = cov.map_point_culling(a["found"], a["visible"], a["first_kf_id"], a["n_obs"], a["bad"], P.MP_CURRENT, monocular=bool(mono))
    assert rc == 0 and got.tobytes() == host.tobytes() == want.tobytes()
    assert len(cov.STATUS) == 5
