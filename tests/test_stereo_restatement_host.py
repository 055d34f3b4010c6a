"""CPU: tests/stereo_restatement.py against the oracle's ComputeStereoMatches, bit for bit, on the edge scene of
tests/stereo_edge_scene.py (every exit of the routine planted by hand), on that scene with identical images (median 0: every
match is culled) and on the random scene of the existing tests; every status code and every planted boundary reached; the
median cull's rule on hand-made SAD arrays.  No device."""
import numpy as np
import pytest

import stereo_edge_scene as ES
import stereo_restatement as SR
from conftest import synthetic_stereo

F = np.float32


def _u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _run(oracle, left, right, kpL, descL, kpR, descR, bf, b, **ex):
    el, er = oracle.OrbExtractor(**ex), oracle.OrbExtractor(**ex)
    kl, dl = el(left); kr, dr = er(right)
    if kpL is None:
        kpL, descL, kpR, descR = kl, dl, kr, dr
    pyrL = [el.level(l) for l in range(el.nlevels)]; pyrR = [er.level(l) for l in range(er.nlevels)]
    args = (kpL, descL, kpR, descR, el.scale, el.inv_scale, pyrL, pyrR, bf, b)
    return oracle.stereo_matches(*args), SR.stereo_match(*args), SR.stereo_match_begin(*args)


@pytest.fixture(scope="module")
def scenes(oracle):
    out = {}
    for name, identical in (("edge", False), ("identical", True)):
        sc = ES.build(identical=identical)
        o, r, beg = _run(oracle, sc["left"], sc["right"], sc["kpL"], sc["descL"], sc["kpR"], sc["descR"], sc["bf"], sc["b"],
                         nfeatures=ES.NFEATURES, scale_factor=ES.SCALE_FACTOR, nlevels=ES.NLEVELS)
        out[name] = dict(scene=sc, oracle=o, restated=r, begin=beg)
    return out


def _assert_equal(o, r):
    uR_o, depth_o, best_o, kept = o
    uR, depth, best, sad, status = r
    assert np.array_equal(_u32(uR), _u32(uR_o)) and np.array_equal(_u32(depth), _u32(depth_o))
    assert np.array_equal(best, best_o)
    assert int((uR >= 0).sum()) == kept == int(np.isin(status, (SR.ACCEPTED, SR.ACCEPTED_CLAMPED)).sum())


@pytest.mark.parametrize("name", ["edge", "identical"])
def test_restatement_equals_oracle_on_the_edge_scene(scenes, name):
    _assert_equal(scenes[name]["oracle"], scenes[name]["restated"])


def test_restatement_equals_oracle_on_the_random_scene(oracle):
    L, R = synthetic_stereo(21, disparity=8)
    o, r, _ = _run(oracle, L, R, None, None, None, None, 386.1448, 386.1448 / 718.856)
    _assert_equal(o, r)
    assert o[3] > 200


def test_identical_images_cull_every_match(scenes):
    """SAD 0 at the best increment of every match, median 0, thDist 0: `dist < thDist` never holds.  The reference's behaviour."""
    uR, depth, best, sad, status = scenes["identical"]["restated"]
    uR_o, depth_o, best_o, kept = scenes["identical"]["oracle"]
    assert kept == 0 and (uR_o == -1).all() and (depth_o == -1).all()
    assert (status == SR.CULLED).sum() > 20 and not np.isin(status, (SR.ACCEPTED, SR.ACCEPTED_CLAMPED)).any()
    assert (sad[status == SR.CULLED] == 0).sum() * 2 > (status == SR.CULLED).sum()       # the median is 0
    assert (best_o >= 0).sum() > 40 and (best_o[status == SR.CULLED] >= 0).all()         # best_right is still set


def test_every_status_and_every_plant_is_reached(scenes):
    s = scenes["edge"]
    sc = s["scene"]
    uR_o, depth_o, best_o, kept = s["oracle"]
    uR, depth, best, sad, status = s["restated"]
    assert set(status.tolist()) == set(range(len(SR.STATUS_NAMES))), [SR.STATUS_NAMES[i] for i in set(range(10)) - set(status.tolist())]
    for name, (i, want, best_want) in sc["plants"].items():
        assert status[i] in want, (name, SR.STATUS_NAMES[status[i]])
        if best_want is not None:
            assert best_o[i] == best_want, (name, best_o[i], best_want)
        # what the status says is what the ORACLE's outputs show
        matched = status[i] in (SR.ACCEPTED, SR.ACCEPTED_CLAMPED)
        assert (uR_o[i] >= 0) == matched and (depth_o[i] > 0) == matched, name
        if status[i] in (SR.NO_ROW, SR.MAXU_NEG, SR.NO_BEST):
            assert best_o[i] == -1, name
        else:
            assert best_o[i] >= 0, name
    # keys on all four octaves reach the SAD stage, and a match survives on each
    kl = sc["kpL"]
    for o in range(ES.NLEVELS):
        assert (np.isin(status, (SR.ACCEPTED, SR.CULLED)) & (kl["octave"] == o)).any(), o
    assert (status[kl["octave"] == 0] == SR.ACCEPTED).any()


def test_planted_boundaries_land_where_they_should(scenes):
    s = scenes["edge"]
    sc = s["scene"]
    kl, kr, dl, dr = sc["kpL"], sc["kpR"], sc["descL"], sc["descR"]
    uR_o, depth_o, best_o, _ = s["oracle"]
    P = {k: v[0] for k, v in sc["plants"].items()}
    rk = {k: v[2] for k, v in sc["plants"].items()}
    # Hamming distances of exactly 74 / 75 / 99 / 100
    for k in (74, 75, 99):
        i = P[f"hamming_{k}"]
        assert SR.hamming(dl[i], dr[best_o[i]]) == k
    i = P["hamming_100"]
    row_mates = [j for j in range(len(kr)) if abs(kr["y"][j] - kl["y"][i]) <= 2 and kl["x"][i] - 20 <= kr["x"][j] <= kl["x"][i]]
    assert min(SR.hamming(dl[i], dr[j]) for j in row_mates) == 100 and best_o[i] == -1
    # minU / maxU in float32
    max_d = F(sc["bf"]) / F(sc["b"])
    i = P["maxu_in"]; assert kr["x"][rk["maxu_in"]] == kl["x"][i] - F(0)
    i = P["minu_in"]; assert kr["x"][rk["minu_in"]] == kl["x"][i] - max_d
    for name, side in (("maxu_out", F(np.inf)), ("minu_out", F(-np.inf))):
        i = P[name]
        bound = kl["x"][i] - (F(0) if side > 0 else max_d)
        mates = [j for j in range(len(kr)) if kr["y"][j] == kl["y"][i] and SR.hamming(dl[i], dr[j]) == 80]
        assert len(mates) == 1 and kr["x"][mates[0]] == np.nextafter(bound, side) and best_o[i] == -1
    # the clamp: disparity exactly 0 becomes 0.01
    i = P["mirror"]
    assert _u32(uR_o[i:i + 1])[0] == _u32(F(np.float64(F(30.0)) - 0.01))[()] and _u32(depth_o[i:i + 1])[0] == _u32(F(sc["bf"]) / F(0.01))[()]
    # the tie: both right keys are candidates, the descriptors are the same, the lower index is named
    i = P["tie"]
    assert np.array_equal(dr[best_o[i]], dr[best_o[i] + 1]) and kr["y"][best_o[i] + 1] == kr["y"][best_o[i]]
    # the window test: round(x * inv_scale) == cols - 11 is out, cols - 12 goes on to the SAD; a negative x rounds below 0
    assert kr["x"][rk["window_hi"]] == ES.COLS - 11 and kr["x"][rk["window_hi_in"]] == ES.COLS - 12
    assert SR.roundf(kr["x"][rk["window_lo"]]) < 0
    # the number of SAD jobs is no multiple of 4: the last workgroup of stereo_sad_kernel is partial
    st_begin = s["begin"][4]
    jobs = int(np.isin(st_begin, (SR.INC_EDGE, SR.DISP_OUT, SR.ACCEPTED, SR.ACCEPTED_CLAMPED)).sum())
    assert jobs % 4 != 0 and jobs > 40, jobs


def _cull(sad, keep=None):
    sad = np.asarray(sad, np.int32)
    u = np.where(sad >= 0, 5.0, -1.0).astype(F); d = np.where(sad >= 0, 2.0, -1.0).astype(F)
    u2, d2, culled = SR.cull(sad, u, d, keep)
    assert np.array_equal(u2 >= 0, d2 >= 0)
    return (u2 >= 0).tolist()


def test_cull_rule_on_hand_made_distances():
    """median = element n / 2 of the sorted distances; thDist = 1.5f * 1.4f * median in float32; `dist < thDist` stays.
    1.5f * 1.4f rounds to 2.0999999, and 2.0999999f * 10 lies exactly half way between 21 and the float below it: the tie goes to
    the even mantissa, thDist == 21.0 exactly, so with median 10 a SAD of 20 stays and 21 goes.  (In real arithmetic 21 < 21.0000001
    would stay: the float32 product is what the reference computes.)"""
    assert F(1.5) * F(1.4) * F(10) == F(21.0) and F(1.5) * F(1.4) < F(2.1) + F(1e-6)
    assert _cull([10, 10, 10, 20, 21]) == [True, True, True, True, False]                # n = 5: median = sorted[2] = 10
    assert _cull([21, 10, 20, 10, 10]) == [False, True, True, True, True]
    assert _cull([1, 10, 22, 100]) == [True, True, True, False]                            # n = 4: median = sorted[2] = 22, th 46.2
    assert _cull([1, 10, 22, 46]) == [True, True, True, True]
    assert _cull([1, 10, 22, 47]) == [True, True, True, False]
    assert _cull([7, 7, 7, 7]) == [True] * 4                                                # all equal: 7 < 14.7
    assert _cull([9]) == [True]                                                             # a single element
    assert _cull([0]) == [False] and _cull([0, 0, 5]) == [False] * 3                        # median 0: thDist 0, nothing is < 0
    assert _cull([0, 5, 5]) == [True, True, True]
    assert _cull([-1, 10, -1, 10, 21, 10]) == [False, True, False, True, False, True]       # no match (-1) takes no part
    # a keep mask: dropped keys get -1 and do not count towards the median
    assert _cull([10, 10, 10, 100, 100], keep=[1, 1, 1, 1, 1]) == [True, True, True, False, False]
    assert _cull([10, 10, 10, 100, 100], keep=[1, 0, 0, 1, 1]) == [True, False, False, True, True]    # median 100
    assert _cull([10, 10, 10], keep=[0, 0, 0]) == [False] * 3
