"""The batched fusion search on the device (sivo_amd/csrc/fuse_batch.hip through sivo_amd/matcher.py) against the numpy restatement of
ORBmatcher::Fuse's per-point tests and candidate loop (tests/fuse_batch_restatement.py) on every scene of tests/fuse_batch_cases.py, and
against the single-keyframe sivo_fuse fed with the restatement's projections; the shapes at which the kernel can go wrong; the masks;
the optional outputs; buffer growth; and the C++ adapter through the product library against the host build's blob."""
import numpy as np
import pytest

import fuse_batch_cases as FC
import fuse_batch_restatement as R
import host_prog

pytestmark = pytest.mark.gpu
F32 = np.float32
REACHED = (R.MATCHED, R.NO_CANDIDATE, R.TOO_FAR)


def match_frame(f):
    from sivo_amd import matcher as M
    keys = np.zeros(f.n, M.KP_DTYPE)
    keys["x"], keys["y"], keys["octave"] = f.x, f.y, f.octave
    return M.MatchFrame(keys, f.u_right, f.desc, f.bounds, f.scale, f.scale * f.scale, f.inv_sigma2)


_FRAMES = {}


def frames_of(name):
    """The scene's keyframes on the device, made once per scene (a frame of the restatement that serves twice is uploaded once)."""
    if name not in _FRAMES:
        made = {}
        _FRAMES[name] = [made.setdefault(id(f), match_frame(f)) for f in FC.scene(name)["frames"]]
    return _FRAMES[name]


def device(name, ks=None, ns=None, frames=None, **kw):
    from sivo_amd import matcher as M
    sc = FC.scene(name)
    ks = range(len(sc["frames"])) if ks is None else ks
    ns = np.arange(len(sc["pos"])) if ns is None else np.asarray(ns)
    fr = frames_of(name) if frames is None else frames
    sp = None if sc["skip_point"] is None else sc["skip_point"][ns]
    sq = None if sc["skip_pair"] is None else sc["skip_pair"][np.ix_(list(ks), ns)]
    kw.setdefault("skip_point", sp); kw.setdefault("skip_pair", sq)
    return M.fuse_batch([fr[k] for k in ks], sc["cams"][list(ks)], sc["pos"][ns], sc["normal"][ns], sc["min_dist"][ns], sc["max_dist"][ns],
                        sc["desc"][ns], sc["th"], **kw)


def same(got, want, what, ks=None, ns=None):
    """best_idx, best_dist, status and level equal, u / v / ur bit for bit, on the pairs that reach the window query; the entries of
    every other pair as matcher.fuse_batch initialised them (NaN / -1: not written)."""
    if ks is not None:
        want = {k: v[np.ix_(list(ks), np.asarray(ns))] for k, v in want.items()}
    for k in ("best_idx", "best_dist", "status"):
        assert np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:8].tolist())
    reached = np.isin(want["status"], REACHED)
    if "u" not in got:
        return
    for k in ("u", "v", "ur"):
        assert np.array_equal(got[k][reached].view(np.uint32), want[k][reached].view(np.uint32)), (what, k)
        assert np.all(np.isnan(got[k][~reached])), (what, k, "an entry of a pair that did not reach the window query was written")
    assert np.array_equal(got["level"][reached], want["level"][reached]), (what, "level")
    assert np.all(got["level"][~reached] == -1), (what, "level of a pair that did not reach the window query was written")


@pytest.mark.parametrize("name", FC.HAND_SCENES + ("random",))
def test_every_scene_equals_the_restatement(name):
    same(device(name), FC.scene(name)["expect"], name)


def test_random_scene_equals_sivo_fuse_per_keyframe():
    """The batch against the loop it replaces: sivo_fuse on each keyframe, fed with the restatement's projection of every point."""
    from sivo_amd import matcher as M
    sc, fr = FC.scene("random"), frames_of("random")
    e = sc["expect"]
    assert [f.n for f in sc["frames"]] == list(FC.RANDOM_KEYS) and e["status"].shape == (5, 203)
    got = device("random")
    for k in range(5):
        valid = np.isin(e["status"][k], REACHED)
        z = lambda a: np.where(valid, a[k], 0).astype(a.dtype)
        scw = int(sc["cams"][k]["scw_variant"])
        nf, bi, bd = M.fuse(fr[k], valid.astype(np.uint8), z(e["u"]), z(e["v"]), None if scw else z(e["ur"]), z(e["level"]), sc["desc"], sc["th"], scw)
        assert np.array_equal(got["best_idx"][k], bi) and np.array_equal(got["best_dist"][k], bd), k
        assert nf == int((got["status"][k] == R.MATCHED).sum())
    assert (got["status"] == R.MATCHED).sum() > 40


@pytest.mark.parametrize("ks,ns", [((4,), (3,)), ((4,), (0, 1, 2)), ((2, 3, 4), (5,)), ((3, 4), (0, 1)), ((4,), (0, 1, 2, 3)), ((4,), range(5)),
                                   ((0, 1, 2, 3, 4), (7,)), ((4,), range(203)), ((1, 3), range(100, 203))])
def test_partial_workgroups_single_keyframe_single_point(ks, ns):
    """n_kf * n_mp of 1, 3, 4 and 5 (four pairs per workgroup), one keyframe, one point."""
    ns = list(ns)
    same(device("random", ks, ns), FC.scene("random")["expect"], (ks, ns), ks, ns)


def test_skip_masks():
    sc = FC.scene("random")
    e = sc["expect"]
    K, N = e["status"].shape
    none = device("random", skip_pair=np.ones((K, N), np.uint8))
    assert np.all(none["status"] == R.SKIPPED) and np.all(none["best_idx"] == -1) and np.all(np.isnan(none["u"])) and np.all(none["level"] == -1)
    by_point = device("random", skip_point=np.ones(N, np.uint8))
    assert np.all(by_point["status"] == R.SKIPPED) and np.all(by_point["best_idx"] == -1)
    last = np.ones((K, N), np.uint8)
    last[-1, -1] = 0
    got = device("random", skip_pair=last)
    assert np.all(got["status"].ravel()[:-1] == R.SKIPPED)
    for k in ("best_idx", "best_dist", "status"):
        assert got[k][-1, -1] == e[k][-1, -1], k
    # the last pair of a scene in which it matches
    e = FC.scene("masks")["expect"]
    assert e["status"][-1, -1] == R.MATCHED
    last = np.ones(e["status"].shape, np.uint8)
    last[-1, -1] = 0
    got = device("masks", skip_point=None, skip_pair=last)
    assert got["status"][-1, -1] == R.MATCHED and got["best_idx"][-1, -1] == e["best_idx"][-1, -1] and (got["status"] == R.SKIPPED).sum() == last.sum()


def test_optional_outputs_may_be_null():
    got = device("random", extras=False)
    assert set(got) == {"best_idx", "best_dist", "status"}
    same(got, FC.scene("random")["expect"], "no optional outputs")


def test_calls_of_growing_size_leave_the_frames_usable():
    """A small call, then a bigger one on the same frames (the staging buffers grow), then a plain sivo_fuse on one of the frames: its
    answer is what it was before the batches."""
    from sivo_amd import matcher as M
    sc = FC.scene("random")
    e = sc["expect"]
    fr = [match_frame(f) for f in sc["frames"]]                      # frames of this test's own: their first use is the batch
    k = 4
    valid = np.isin(e["status"][k], REACHED)
    z = lambda a: np.where(valid, a[k], 0).astype(a.dtype)
    args = (valid.astype(np.uint8), z(e["u"]), z(e["v"]), z(e["ur"]), z(e["level"]), sc["desc"], sc["th"], 0)
    same(device("random", (4,), range(3), frames=fr), e, "small", (4,), range(3))
    before = M.fuse(fr[k], *args)
    # a scene many times the size of the buffers' first allocation: every point 40 times
    N = len(sc["pos"])
    rep = np.tile(np.arange(N), 40)
    big = device("random", frames=fr, ns=rep)
    for name in ("best_idx", "best_dist", "status"):
        assert np.array_equal(big[name], np.tile(e[name], (1, 40))), name
    same(device("random", (0, 4), range(50), frames=fr), e, "small again", (0, 4), range(50))
    after = M.fuse(fr[k], *args)
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
    assert np.array_equal(after[1], e["best_idx"][k])


def test_cpp_adapter_through_the_product_library(tmp_path):
    """SIVO::FuseIntoKeyFrames and SIVO::SearchAndFuse on the descriptor-change scenes, linked against libsivo_hip: the blob the host
    build of the same program writes (tests/test_fuse_batch_host.py compares that one with the loop of single-keyframe Fuse calls)."""
    import fuse_batch_adapter_cases as AC
    host = host_prog.build("fuse_batch_adapter_prog", tmp_path)
    dev = host_prog.build("fuse_batch_adapter_prog", tmp_path, link_lib=True, defines=("FUSE_BATCH_ON_LIBRARY",))
    for mode, name in (("fuse", "descriptor_change"), ("loop", "loop_descriptor_change")):
        blob = AC.blob(AC.scene(name))
        a, b = host_prog.run(host, tmp_path, mode, blob), host_prog.run(dev, tmp_path, mode, blob)
        assert AC.strip_counters(a) == AC.strip_counters(b), name
