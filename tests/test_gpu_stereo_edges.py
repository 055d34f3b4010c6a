"""GPU: sivo_stereo_match / _begin / _cull against tests/stereo_restatement.py, bit for bit, on the edge scene of
tests/stereo_edge_scene.py (96 x 192, hand-made keys on four octaves, every exit of ComputeStereoMatches planted; the host test
test_stereo_restatement_host.py pins the restatement and the plants to the CPU oracle), and the octave check of the entry points."""
import ctypes as C

import numpy as np
import pytest

import stereo_edge_scene as ES
import stereo_restatement as SR
from conftest import synthetic_stereo
from sivo_amd import orb
from sivo_amd._lib import SivoError, check

pytestmark = pytest.mark.gpu
F = np.float32
EX = dict(nfeatures=ES.NFEATURES, scale_factor=ES.SCALE_FACTOR, nlevels=ES.NLEVELS)


def _u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(a, b):
    return all(np.array_equal(_u32(x), _u32(y)) if x.dtype == F else np.array_equal(x, y) for x, y in zip(a, b))


class _Side:
    """One scene: its device extractors with the pyramids resident, and the restatement's results on the oracle's levels."""

    def __init__(self, oracle, identical):
        sc = self.sc = ES.build(identical=identical)
        self.eo_l, self.eo_r = oracle.OrbExtractor(**EX), oracle.OrbExtractor(**EX)
        self.eo_l(sc["left"]); self.eo_r(sc["right"])
        self.eg_l, self.eg_r = orb.ORBextractor(**EX), orb.ORBextractor(**EX)
        self.eg_l(sc["left"]); self.eg_r(sc["right"])
        self.pyrL = [self.eo_l.level(l) for l in range(ES.NLEVELS)]; self.pyrR = [self.eo_r.level(l) for l in range(ES.NLEVELS)]
        self.keys = (sc["kpL"], sc["descL"], sc["kpR"], sc["descR"])
        self.begin = SR.stereo_match_begin(*self.keys, self.eo_l.scale, self.eo_l.inv_scale, self.pyrL, self.pyrR, sc["bf"], sc["b"])
        self.full = SR.stereo_match(*self.keys, self.eo_l.scale, self.eo_l.inv_scale, self.pyrL, self.pyrR, sc["bf"], sc["b"])

    def restate(self, kpL, descL, kpR, descR):
        return SR.stereo_match(kpL, descL, kpR, descR, self.eo_l.scale, self.eo_l.inv_scale, self.pyrL, self.pyrR, self.sc["bf"], self.sc["b"])

    def match(self, kpL=None, descL=None, kpR=None, descR=None, begin=False):
        k = self.keys if kpL is None else (kpL, descL, kpR, descR)
        return (orb.stereo_match_begin if begin else orb.stereo_match)(self.eg_l, self.eg_r, *k, self.sc["bf"], self.sc["b"])


@pytest.fixture(scope="module")
def edge(oracle):
    return _Side(oracle, False)


@pytest.fixture(scope="module")
def identical(oracle):
    return _Side(oracle, True)


def test_device_levels_equal_the_oracles(edge):
    for eo, eg in ((edge.eo_l, edge.eg_l), (edge.eo_r, edge.eg_r)):
        assert np.array_equal(eg.GetScaleFactors(), eo.scale) and np.array_equal(eg.GetInverseScaleFactors(), eo.inv_scale)
        for l in range(ES.NLEVELS):
            assert np.array_equal(eg.image_pyramid(l, with_border=True), eo.level(l, with_border=True)), f"pyramid level {l}"


def test_stereo_match_equals_the_restatement(edge):
    uR, depth, best = edge.match()
    r = edge.full
    assert np.array_equal(best, r[2])
    bad = np.nonzero(_u32(uR) != _u32(r[0]))[0]
    assert len(bad) == 0, [(int(i), SR.STATUS_NAMES[r[4][i]], float(uR[i]), float(r[0][i])) for i in bad]
    assert np.array_equal(_u32(depth), _u32(r[1]))
    i = edge.sc["plants"]["mirror"][0]                       # the clamp, in numbers
    assert uR[i] == F(np.float64(F(30.0)) - 0.01) and depth[i] == F(edge.sc["bf"]) / F(0.01)


def test_stereo_match_begin_equals_the_restatement(edge):
    got = edge.match(begin=True)
    assert _same(got, edge.begin[:4])
    assert (got[3] >= 0).sum() == np.isin(edge.begin[4], (SR.ACCEPTED, SR.ACCEPTED_CLAMPED)).sum() > 30


def test_cull_equals_the_restatement(edge):
    uR0, depth0, _, sad = edge.match(begin=True)
    n = len(uR0)
    one = np.zeros(n, np.uint8); one[edge.sc["plants"]["hamming_74"][0]] = 1
    masks = [None, np.random.default_rng(1).random(n) < 0.4, np.zeros(n, np.uint8), one]
    for keep in masks:
        uR, depth = uR0.copy(), depth0.copy()
        orb.stereo_match_cull(keep, sad, uR, depth)
        wu, wd, _ = SR.cull(edge.begin[3], edge.begin[0], edge.begin[1], keep)
        assert _same((uR, depth), (wu, wd))
        if keep is not None:
            assert (uR[np.asarray(keep) == 0] == -1).all() and (depth[np.asarray(keep) == 0] == -1).all()
    assert uR[one == 1][0] >= 0                                  # a single key is its own median: dist < 2.1 dist


def test_begin_then_cull_over_a_mask_equals_the_match_of_the_masked_keys(edge):
    kpL, descL, kpR, descR = edge.keys
    keep = np.random.default_rng(2).random(len(kpL)) < 0.5
    uR, depth, best, sad = edge.match(begin=True)
    orb.stereo_match_cull(keep, sad, uR, depth)
    uR_s, depth_s, best_s = edge.match(kpL[keep], descL[keep], kpR, descR)
    r = edge.restate(kpL[keep], descL[keep], kpR, descR)
    assert _same((uR[keep], depth[keep], best[keep]), (uR_s, depth_s, best_s)) and _same((uR_s, depth_s, best_s), r[:3])
    assert 0 < (uR_s >= 0).sum() < keep.sum()


def test_identical_images_cull_every_match(identical):
    uR, depth, best = identical.match()
    assert (uR == -1).all() and (depth == -1).all()
    assert np.array_equal(best, identical.full[2]) and (best >= 0).sum() > 40
    got = identical.match(begin=True)
    assert _same(got, identical.begin[:4]) and (got[3] == 0).sum() > 20


def test_empty_and_single_key_calls(edge):
    kpL, descL, kpR, descR = edge.keys
    uR, depth, best = edge.match(kpL[:0], descL[:0], kpR, descR)
    assert len(uR) == len(depth) == len(best) == 0
    uR, depth, best, sad = edge.match(kpL, descL, kpR[:0], descR[:0], begin=True)
    assert (uR == -1).all() and (depth == -1).all() and (best == -1).all() and (sad == -1).all()
    i, _, j = edge.sc["plants"]["hamming_74"]
    got = edge.match(kpL[i:i + 1], descL[i:i + 1], kpR[j:j + 1], descR[j:j + 1])
    want = edge.restate(kpL[i:i + 1], descL[i:i + 1], kpR[j:j + 1], descR[j:j + 1])
    assert _same(got, want[:3]) and got[2][0] == 0 and got[0][0] >= 0


def test_repeated_calls_and_a_regrown_arena_give_the_same_bytes(edge):
    kpL, descL, kpR, descR = edge.keys
    first = edge.match(begin=True)
    assert _same(edge.match(begin=True), first)
    big = edge.match(np.tile(kpL, 10), np.tile(descL, (10, 1)), np.tile(kpR, 10), np.tile(descR, (10, 1)), begin=True)
    for a, b in zip(big, first):                                 # a tie between the copies of a right key names the first copy
        assert (a.reshape(10, -1).view(np.uint32) == b.view(np.uint32)[None]).all()
    assert _same(edge.match(begin=True), first) and _same(first, edge.begin[:4])


def test_octaves_outside_the_extractors_levels_are_refused():
    """Host entry points scan the keys before anything is staged: an octave outside [0, nlevels) (here 8 .. 15, left or right) is an
    invalid argument and no output is written."""
    L, R = synthetic_stereo(21, disparity=8)
    eg_l, eg_r = orb.ORBextractor(), orb.ORBextractor()          # 8 levels
    kl, dl = eg_l(L); kr, dr = eg_r(R)
    kl, dl, kr, dr = kl[:50], dl[:50], kr, dr
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    bf, b = C.c_float(386.1448), C.c_float(386.1448 / 718.856)
    good = orb.stereo_match_begin(eg_l, eg_r, kl, dl, kr, dr, bf.value, b.value)
    for side, at, octave in (("L", 0, 8), ("L", 49, 15), ("R", 0, 8), ("R", len(kr) - 1, 12)):
        bl_, br_ = kl.copy(), kr.copy()
        (bl_ if side == "L" else br_)["octave"][at] = octave
        uR = np.full(50, 7, F); depth = np.full(50, 7, F); best = np.full(50, 7, np.int32); sad = np.full(50, 7, np.int32)
        for begin in (False, True):
            with pytest.raises(SivoError):
                if begin:
                    check(eg_l._L.sivo_stereo_match_begin(eg_l._h, eg_r._h, p(bl_), p(dl), 50, p(br_), p(dr), len(br_), bf, b,
                                                              p(uR), p(depth), p(best), p(sad)))
                else:
                    check(eg_l._L.sivo_stereo_match(eg_l._h, eg_r._h, p(bl_), p(dl), 50, p(br_), p(dr), len(br_), bf, b, p(uR), p(depth), p(best)))
            assert (uR == 7).all() and (depth == 7).all() and (best == 7).all() and (sad == 7).all()
    assert _same(orb.stereo_match_begin(eg_l, eg_r, kl, dl, kr, dr, bf.value, b.value), good)      # the handle is as it was
