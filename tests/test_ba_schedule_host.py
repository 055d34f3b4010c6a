"""Host side of the LocalBundleAdjustment schedule tests (no GPU): the oracle under an iteration budget, and the check that the cases of
tests/test_gpu_ba_schedule.py can see a device solver whose leveled edges lose the error that excluded them — a NumPy model of the
solver's two per-edge error sets (tests/ba_schedule_cases.py), fed by the oracle's trace, differs from the oracle in the flags of the odd
cases and in none of the controls."""
import numpy as np
import pytest

import ba_schedule_cases as S


def test_budget_5_10_is_the_plain_call(oracle):
    """orc_local_ba is the budget variant at (5, 10): the same bytes, and the new per-edge outputs say what the flags say."""
    sc = S.scene(4)
    a = oracle.local_ba(*sc, cov_pose=5)
    b = oracle.local_ba(*sc, cov_pose=5, budget=(5, 10), trace=True)
    for k in ("poses", "points", "outlier", "cov"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["iterations"], a["trials"], a["cov_ok"]) == (b["iterations"], b["trials"], b["cov_ok"])
    assert np.array_equal(b["outlier"], ((b["chi2"] > S.thresholds(sc[3])) | (b["depth_ok"] == 0)).astype(np.uint8))
    kinds = [k for k, _ in b["trace"]]
    assert kinds.count("call_start") == 2 and kinds[0] == "call_start"
    assert kinds.count("trial_accepted") + kinds.count("trial_rejected") == b["trials"]
    assert kinds.count("call_start") + kinds.count("linearisation") == b["iterations"]
    # the last record is what the final classification read
    assert b["trace"][-1][1].shape == (len(sc[3]), 3) and np.array_equal(S.chi2_of(b["trace"][-1][1], sc[3]), b["chi2"])


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_oracle_keeps_the_error_that_excluded_an_edge(case):
    """Every observation the reference excluded after the first optimize() is one it erases (Optimizer.cc:826-858): level & ~outlier is
    empty, and a leveled edge's final chi2 is the one the first classification read.  No edge of a case lies within the band around its
    threshold, at either classification: device and oracle flags can be compared exactly."""
    edges = S.scene(case[0])[3]
    o = S.reference(case)
    th = S.thresholds(edges)
    leveled = o["level"] != 0
    assert leveled.any() and not (leveled & (o["outlier"] == 0)).any()
    _, _, _, chi2_first = S.two_set_model(o, edges, mirror_on_level=True)
    assert np.array_equal(chi2_first[leveled], o["chi2"][leveled])
    assert np.abs(o["chi2"] - th).min() > S.BAND
    assert np.abs(chi2_first - th).min() > S.BAND
    assert (o["iterations"], o["trials"]) == (sum(case[1]), sum(case[1]))          # one accepted trial per iteration, none rejected


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_two_set_model_flips_flags_on_the_odd_cases_only(case):
    """The sensitivity of the GPU test, shown without a GPU.  Skipping leveled edges in both sets and classifying on the set written last
    loses flags exactly where the two classifications read different sets; copying a leveled edge's errors into the other set when it
    is leveled loses none."""
    seed, budget = case
    edges = S.scene(seed)[3]
    o = S.reference(case)
    s1, s2, flags, _ = S.two_set_model(o, edges, mirror_on_level=False)
    flips = int((flags != o["outlier"]).sum())
    print(f"[{S.case_id(case)}] edges {len(edges)}  leveled {int((o['level'] != 0).sum())}  S1 {s1}  S2 {s2}  modelled flips {flips}")
    if case in S.ODD:
        assert s2 != s1
        assert flips >= S.MIN_FLIPS[budget]
        lost = (flags != o["outlier"])
        assert (o["level"][lost] != 0).all() and (o["outlier"][lost] == 1).all()     # every flip is a leveled edge left unflagged
    else:
        assert s2 == s1 and flips == 0
    m1, m2, mflags, _ = S.two_set_model(o, edges, mirror_on_level=True)
    assert (m1, m2) == (s1, s2) and np.array_equal(mflags, o["outlier"])


def test_case_table_covers_what_the_gpu_test_needs():
    budgets = {b for _, b in S.ODD}
    assert budgets == {(1, 1), (2, 1), (3, 7), (5, 1), (5, 3)}
    assert {b for _, b in S.CONTROLS} == {(5, 10), (5, 2)}
    assert all(b[1] % 2 == 1 for _, b in S.ODD) and all(b[1] % 2 == 0 for _, b in S.CONTROLS)


def test_debug_entry_refuses_a_negative_budget():
    """The arguments are checked before a device is asked for."""
    from sivo_amd import _lib
    with pytest.raises(_lib.SivoError, match="negative iteration count") as e:
        S.device_local_ba(*S.scene(4), (5, -1))
    assert e.value.code == _lib.ERR_INVALID_ARGUMENT
