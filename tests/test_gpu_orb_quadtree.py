"""The quadtree keypoint distribution on the device: sivo_orb_distribute_batch_dev against the library's host routine byte for byte on
every scene of tests/orb_quadtree_cases.py and on FAST's own candidates, and the extractor's launch-mode bit 4 (the quadtree kernel
between FAST and the angle / descriptor group, one host wait per image) against mode 15 and the oracle."""
import numpy as np
import pytest
import torch

import orb_quadtree_cases as Q
from conftest import synthetic_frame, synthetic_stereo
from sivo_amd import _lib, orb

pytestmark = pytest.mark.gpu

NAMES = list(Q.SCENES)


@pytest.fixture(scope="module")
def host_lists():
    """orb.distribute_octtree (the host routine) on every scene, computed once."""
    return {name: orb.distribute_octtree(*Q.SCENES[name]) for name in NAMES}


def _batch(names):
    cols = [[Q.SCENES[n][i] for n in names] for i in range(6)]
    return orb.distribute_octtree_batch_dev(*cols)


def test_every_scene_one_set_at_a_time(host_lists):
    for name in NAMES:
        got = orb.distribute_octtree_dev(*Q.SCENES[name])
        assert got.dtype == orb.KP_DTYPE and got.tobytes() == host_lists[name].tobytes(), name


def test_every_scene_in_one_launch_twice(host_lists):
    first = _batch(NAMES)
    second = _batch(NAMES)
    for name, a, b in zip(NAMES, first, second):
        assert a.tobytes() == host_lists[name].tobytes(), name
        assert b.tobytes() == a.tobytes(), name


def test_batch_of_eight_with_an_empty_set_in_the_middle(host_lists):
    for name, got in zip(Q.BATCH, _batch(Q.BATCH)):
        assert got.tobytes() == host_lists[name].tobytes(), name


def test_out_capacity_is_reported_with_the_offsets(host_lists):
    import ctypes as C
    names = ["count_65", "empty", "count_257"]
    sets = [np.ascontiguousarray(Q.SCENES[n][0]) for n in names]
    off = np.array([0, 65, 65, 65 + 257], np.int64)
    keys = np.concatenate(sets)
    cols = [np.array([Q.SCENES[n][i] for n in names], np.int32) for i in range(1, 6)]
    out = np.zeros(4, orb.KP_DTYPE); out_off = np.full(4, -7, np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    L = _lib.lib()
    rc = L.sivo_orb_distribute_batch_dev(3, p(off), p(keys), *[p(c) for c in cols], C.c_int64(4), p(out), p(out_off), 0)
    want = np.cumsum([0] + [len(host_lists[n]) for n in names])
    assert rc == 5 and "capacity 4" in L.sivo_last_error().decode() and list(out_off) == list(want)


@pytest.mark.parametrize("frame", ["kitti", "small"])
def test_fast_candidates_level_by_level(oracle, kitti_like_bgr, frame):
    """FAST's own candidates of every level through the new entry: the host routine's list on those same candidates."""
    if frame == "kitti":
        gray, kw = oracle.bgr2gray(kitti_like_bgr), {}
    else:
        gray, kw = synthetic_frame(5, 97, 131), dict(nfeatures=50, nlevels=3, scale_factor=1.5)
    ex = orb.ORBextractor(**kw)
    ex(gray)
    sets, regions = [], []
    for l in range(ex.nlevels):
        rows, cols = ex.image_pyramid(l).shape
        sets.append(ex.candidates(l).copy())
        regions.append((16, cols - 16, 16, rows - 16, int(ex.features_per_level[l])))
    assert sum(len(s) for s in sets) > 0
    got = orb.distribute_octtree_batch_dev(sets, *[[r[i] for r in regions] for i in range(5)])
    for l, (s, r) in enumerate(zip(sets, regions)):
        want = orb.distribute_octtree(s, *r)
        assert got[l].tobytes() == want.tobytes(), f"level {l}"
        assert orb.distribute_octtree_dev(s, *r).tobytes() == want.tobytes(), f"level {l} alone"


# ---- the extractor: launch-mode bit 4 ---------------------------------------------------------------------------------------------------
def _frames(oracle, kitti_like_bgr):
    rng = np.random.default_rng(0)
    return [("kitti", oracle.bgr2gray(kitti_like_bgr), {}),
            ("synthetic 9", synthetic_frame(9), {}),
            ("97 x 131", synthetic_frame(5, 97, 131), dict(nfeatures=50, nlevels=3, scale_factor=1.5)),
            ("flat", np.full((352, 1024), 128, np.uint8), {}),
            ("low contrast", (128 + rng.integers(-9, 10, (352, 1024))).astype(np.uint8), {})]


@pytest.fixture(scope="module")
def references(oracle, kitti_like_bgr):
    """Per frame: the oracle's and mode 15's keys and descriptors and mode 15's candidate lists, computed once."""
    out = {}
    for name, gray, kw in _frames(oracle, kitti_like_bgr):
        kp_o, d_o = oracle.OrbExtractor(**kw)(gray)
        a = orb.ORBextractor(launch_mode=15, **kw)
        kp_a, d_a = a(gray)
        assert kp_a.tobytes() == kp_o.tobytes() and np.array_equal(d_a, d_o), name
        out[name] = (gray, kw, kp_a, d_a, [a.candidates(l).copy() for l in range(a.nlevels)], [a.image_pyramid(l, with_border=True) for l in range(a.nlevels)])
    return out


@pytest.mark.parametrize("mode", [16, 18, 30, 31])
def test_device_quadtree_modes_are_bit_identical(references, mode):
    """Keys (angle bits included: the whole record is compared), descriptors, candidate lists and pyramid levels of modes with bit 4
    against mode 15 — which the fixture holds against the oracle — on every frame, three calls on one handle."""
    for name, (gray, kw, kp_a, d_a, cands, levels) in references.items():
        b = orb.ORBextractor(launch_mode=mode, **kw)
        for call in range(3):
            kp_b, d_b = b(gray)
            assert kp_b.tobytes() == kp_a.tobytes(), (name, call)
            assert d_b.shape == d_a.shape and np.array_equal(d_b, d_a), (name, call)
        if name == "flat":
            assert len(kp_b) == 0 and d_b.shape == (0, 32)
        for l in range(b.nlevels):
            assert b.candidates(l).tobytes() == cands[l].tobytes(), (name, l)
            assert np.array_equal(b.image_pyramid(l, with_border=True), levels[l]), (name, l)


def test_device_quadtree_extract_pair_equals_two_calls():
    left, right = synthetic_stereo(21, disparity=8)
    dl, dr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    a, b = orb.ORBextractor(launch_mode=31), orb.ORBextractor(launch_mode=31)
    ref = orb.ORBextractor()(dl)
    for _ in range(3):
        (kl, el), (kr, er) = orb.extract_pair(a, b, dl, dr)
        kl1, el1 = a(dl); kr1, er1 = b(dr)
        assert kl.tobytes() == kl1.tobytes() and np.array_equal(el, el1) and kr.tobytes() == kr1.tobytes() and np.array_equal(er, er1)
    assert kl.tobytes() == ref[0].tobytes() and np.array_equal(el, ref[1])


def test_device_quadtree_capacity_error_and_profiling():
    import ctypes as C
    gray = synthetic_frame(9)
    ex = orb.ORBextractor(launch_mode=31)
    kp, d = ex(gray)
    assert len(kp) > 100
    kps = np.zeros(100, orb.KP_DTYPE); desc = np.zeros((100, 32), np.uint8); n = C.c_int32(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = ex._L.sivo_orb_extract(ex._h, p(gray), gray.shape[0], gray.shape[1], gray.strides[0], p(kps), p(desc), 100, C.byref(n))
    assert rc == 5 and n.value == len(kp) and "capacity 100" in ex._L.sivo_last_error().decode()
    ex.profile(True)
    kp2, d2 = ex(gray)
    ms, calls, keys = ex.profile_read()
    ex.profile(False)
    assert kp2.tobytes() == kp.tobytes() and np.array_equal(d2, d) and calls == 1 and keys == len(kp)
    assert ms["pyramid"] > 0 and ms["fast"] > 0 and ms["blur"] > 0 and ms["angle"] > 0


def test_device_quadtree_is_refused_for_too_many_features():
    ex = orb.ORBextractor(nfeatures=12000)
    assert int(ex.features_per_level.max()) + 3 > Q.MAX_CELLS
    with pytest.raises(_lib.SivoInvalidArgument, match="the device quadtree's table holds 2048 cells"):
        _lib.check(ex._L.sivo_orb_set_launch_mode(ex._h, 31))
    with pytest.raises(_lib.SivoInvalidArgument, match="bit 4"):
        _lib.check(ex._L.sivo_orb_set_launch_mode(ex._h, 32))
    gray = synthetic_frame(9)
    kp, d = ex(gray)                                    # the mode is unchanged: 15, the host quadtree
    kp15, d15 = orb.ORBextractor(nfeatures=12000, launch_mode=15)(gray)
    assert kp.tobytes() == kp15.tobytes() and np.array_equal(d, d15)
