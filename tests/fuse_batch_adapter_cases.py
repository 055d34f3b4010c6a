"""Object graphs for tests/fuse_batch_adapter_prog.cpp: small worlds in which the sequential order of the two fusion loops matters, each
named for what happens in it (tests/test_fuse_batch_host.py asserts from the event log that it does happen).

Every keyframe stands at the identity with the hand-made scenes' camera (tests/fuse_batch_cases.py): a map point "at pixel (x, y)" is the
world point ((x - 320) / 64, (y - 240) / 64, 4), its normal looks at the camera, its distances (1, 4.4) predict level 1, so that with
th = 3 the window is 3.6 pixels; keys are stereo (right = x - 10) at octave 1 unless said otherwise.  Descriptors are sets of bit positions:
the distance of two of them is the size of the symmetric difference.  Keyframes: the targets first (their array order is the order of
std::map<KeyFrame *, ...>), then keyframes that only hold observations."""
import functools

import numpy as np

import fuse_batch_cases as FC

F32 = np.float32
EVENTS = ("replace", "add_observation", "add_map_point", "descriptor", "erase_map_point", "erase_match", "replace_match")


def desc(*bit_ranges):
    d = np.zeros(256, np.uint8)
    for lo, hi in bit_ranges:
        d[lo:hi] = 1
    return np.packbits(d)


class World:
    def __init__(self, n_targets, n_others=2, th=3.0, scw_scale=1.0):
        self.kfs = [dict(keys=[], bad=False) for _ in range(n_targets + n_others)]
        self.targets = list(range(n_targets))
        self.points, self.list, self.th, self.scw_scale = [], [], th, scw_scale
        self.names = {}

    def point(self, name, xy, d, bad=False):
        self.points.append(dict(xy=xy, desc=d, bad=bad))
        self.names[name] = len(self.points) - 1
        return self.names[name]

    def key(self, kf, xy, d, holds=None, stereo=True, octave=1):
        """A key of keyframe kf; the index of its slot."""
        self.kfs[kf]["keys"].append(dict(xy=xy, desc=d, slot=-1 if holds is None else self.names[holds], stereo=stereo, octave=octave))
        return len(self.kfs[kf]["keys"]) - 1

    def fuse(self, *names):
        self.list += [-1 if n is None else self.names[n] for n in names]


def blob(w, repair=True):
    def arr(a, dt):
        a = np.ascontiguousarray(a, dt).ravel()
        return np.array([a.size], np.int64).tobytes() + a.tobytes()

    K, P = len(w.kfs), len(w.points)
    out = np.array([K, P, 0 if repair else 1], np.int32).tobytes() + np.array([w.th], F32).tobytes()
    out += arr([FC.FX, FC.FX, FC.CX, FC.CY, FC.BF], F32) + arr([0, int(FC.W), 0, int(FC.H)], np.int32) + arr(FC.scale_factors(), F32)
    out += arr([FC.log_scale_factor()], F32)
    scw = np.eye(4, dtype=F32)
    scw[:3, :3] *= F32(w.scw_scale)
    for f in w.kfs:
        k = f["keys"]
        out += arr([f["bad"]], np.uint8) + arr(list(np.eye(3).ravel()) + [0, 0, 0], F32) + arr([0, 0, 0], F32) + arr(scw, F32)
        out += arr([q["xy"][0] for q in k], F32) + arr([q["xy"][1] for q in k], F32) + arr([q["octave"] for q in k], np.int32)
        out += arr([(q["xy"][0] - 10.0 if q["stereo"] else -1.0) for q in k], F32)
        out += arr(np.array([q["desc"] for q in k], np.uint8).reshape(len(k), 32), np.uint8) + arr([q["slot"] for q in k], np.int32)
    pos = np.array([((p["xy"][0] - FC.CX) / 64.0, (p["xy"][1] - FC.CY) / 64.0, 4.0) for p in w.points], np.float64).reshape(P, 3)
    normal = pos / np.linalg.norm(pos, axis=1)[:, None] if P else pos
    out += arr(pos, F32) + arr(normal, F32) + arr(np.full(P, 1.0), F32) + arr(np.full(P, 4.4), F32)
    out += arr(np.array([p["desc"] for p in w.points], np.uint8).reshape(P, 32), np.uint8) + arr([p["bad"] for p in w.points], np.uint8)
    out += arr(w.list, np.int32) + arr(w.targets, np.int32)
    return out


def parse(raw, w):
    """(adapter dump, loop dump, counters): a dump is a dict of n_fused, events [(kind name, a, b, c)], slots, points."""
    at = 0

    def take(dt, n):
        nonlocal at
        v = np.frombuffer(raw, dt, n, at)
        at += n * np.dtype(dt).itemsize
        return v

    dumps = []
    for _ in range(2):
        d = dict(n_fused=take(np.int32, len(w.targets)).tolist())
        ne = int(take(np.int64, 1)[0])
        d["events"] = [(EVENTS[int(e[0])], int(e[1]), int(e[2]), int(e[3])) for e in take(np.int64, 4 * ne).reshape(ne, 4)]
        d["slots"] = [take(np.int32, len(f["keys"])).tolist() for f in w.kfs]
        d["points"] = []
        for _p in w.points:
            bad = int(take(np.uint8, 1)[0])
            n_obs, found, visible, replaced = take(np.int32, 4).tolist()
            dsc = take(np.uint8, 32).tobytes()
            no = int(take(np.int64, 1)[0])
            obs = [tuple(int(x) for x in o) for o in take(np.int64, 2 * no).reshape(no, 2)]
            d["points"].append(dict(bad=bad, n_obs=n_obs, found=found, visible=visible, replaced=replaced, desc=dsc, obs=obs))
        dumps.append(d)
    counters = dict(zip(("batch", "single", "repairs"), take(np.int32, 3).tolist()))
    assert at == len(raw)
    return dumps[0], dumps[1], counters


def strip_counters(raw):
    return raw[:-12]


# ---- descriptors of the scenes ---------------------------------------------------------------------------------------------------------
D1 = desc((0, 30))                       # the list point's descriptor at the start
D2 = desc((100, 128))                    # its second observation
DC0 = desc()                             # the key it fuses with in target 0: 30 from D1, 28 from D2 -> the least median, first in order
K_ALPHA = desc((0, 30), (200, 210))      # 10 from D1, 40 from DC0
K_BETA = desc((220, 225))                # 35 from D1, 5 from DC0
K_GAMMA = desc((0, 30), (230, 255))      # 25 from D1, 55 from DC0: a match only for the old descriptor
FAR = desc((0, 128))                     # no match for anything here


def kf_id(k):
    return 100 + k


def _replaced_later_entry():
    """list = [A, B]; A's key in target 0 holds B, A has more observations: B.Replace(A) — B, bad now, is skipped at its own turn although
    it has a key of its own there, and in target 1."""
    w = World(2)
    w.point("A", (352, 256), D1); w.point("B", (288, 224), D2)
    w.key(0, (352, 256), DC0, holds="B")
    w.key(0, (288, 224), D2)                                   # B's own match in target 0, empty slot
    w.key(1, (288, 224), D2)                                   # and in target 1
    w.key(1, (352, 256), D1)
    w.key(2, (10, 10), D1, holds="A"); w.key(3, (10, 10), D2, holds="A")
    w.fuse("A", "B")
    return w


def _descriptor_change(loop=False):
    """A (observed in the two outer keyframes, descriptor D1) fuses in target 0 with a key whose point C has fewer observations:
    C.Replace(A), and ComputeDistinctiveDescriptors gives A the key's descriptor DC0.  In target 1 the old descriptor would pick the key
    K_ALPHA, the new one picks K_BETA; in target 2 the old one would match K_GAMMA and the new one matches nothing.  In the Scw form
    (loop) the Replace is the one of LoopClosing::SearchAndFuse."""
    w = World(3, th=4.0 if loop else 3.0, scw_scale=2.0 if loop else 1.0)
    w.point("A", (352, 256), D1); w.point("C", (352, 256), DC0)
    w.key(0, (352, 256), DC0, holds="C")
    w.key(1, (352, 256), K_ALPHA); w.key(1, (353, 256), K_BETA)
    w.key(2, (352, 256), K_GAMMA)
    w.key(3, (10, 10), D1, holds="A"); w.key(4, (10, 10), D2, holds="A")
    w.fuse("A")
    return w


def _enters_by_replace():
    """A's key in target 1 holds C, which target 2 observes as well: C.Replace(A) puts A into target 2, where the first search had found
    it a key of its own — at target 2's turn A is in the keyframe and is skipped."""
    w = World(3)
    w.point("A", (352, 256), D1); w.point("C", (352, 256), D1)
    w.key(0, (10, 10), FAR)
    w.key(1, (352, 256), D1, holds="C")
    w.key(2, (500, 400), D1, holds="C")                        # C's slot in target 2, far from A's projection
    w.key(2, (352, 256), D1)                                   # the key the speculative search finds for A
    w.key(3, (10, 10), D1, holds="A"); w.key(4, (10, 10), D1, holds="A")
    w.fuse("A")
    return w


def _observation_ties():
    """`pMPinKF->Observations() > pMP->Observations()` is strict: at 2 against 2 the key's point is replaced by the list's; at 4 against 2
    the list's point is replaced by the key's."""
    w = World(1)
    w.point("A", (352, 256), D1); w.point("C", (352, 256), D1); w.point("B", (288, 224), D2); w.point("D", (288, 224), D2)
    w.key(0, (352, 256), D1, holds="C")                        # C: one stereo observation, 2
    w.key(0, (288, 224), D2, holds="D")
    w.key(1, (10, 10), D1, holds="A")                          # A: 2
    w.key(1, (40, 40), D2, holds="B")                          # B: 2
    w.key(2, (40, 40), D2, holds="D")                          # D: 4
    w.fuse("A", "B")
    return w


def _null_and_bad():
    w = World(2)
    w.point("A", (352, 256), D1); w.point("X", (288, 224), D2, bad=True)
    w.key(0, (352, 256), D1); w.key(0, (288, 224), D2)
    w.key(1, (352, 256), D1); w.key(1, (288, 224), D2)
    w.key(2, (10, 10), D1, holds="A")
    w.fuse(None, "X", "A")
    return w


def _loop_same_point_two_keyframes():
    """The loop point A meets the same map point C in targets 0 and 1: after target 0's Replace loop C is bad and its slots hold A, so at
    target 1 A is among the points already found."""
    w = World(2, th=4.0, scw_scale=2.0)
    w.point("A", (352, 256), D1); w.point("C", (352, 256), D1); w.point("B", (288, 224), D2)
    w.key(0, (352, 256), D1, holds="C"); w.key(1, (352, 256), D1, holds="C")
    w.key(0, (288, 224), D2); w.key(1, (288, 224), D2)         # B: plain additions in both
    w.key(2, (10, 10), D1, holds="A"); w.key(3, (10, 10), D2, holds="B")
    w.fuse("A", "B")
    return w


SCENES = {"replaced_later_entry": ("fuse", _replaced_later_entry), "descriptor_change": ("fuse", _descriptor_change),
          "enters_by_replace": ("fuse", _enters_by_replace), "observation_ties": ("fuse", _observation_ties),
          "null_and_bad": ("fuse", _null_and_bad), "loop_same_point_two_keyframes": ("loop", _loop_same_point_two_keyframes),
          "loop_descriptor_change": ("loop", functools.partial(_descriptor_change, loop=True))}


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name][1]()


def mode(name):
    return SCENES[name][0]
