"""Scenes of the batched fusion search (tests/test_fuse_batch_host.py, tests/test_gpu_fuse_batch.py): hand-made ones, one per exit and
edge of ORBmatcher::Fuse's per-point tests and candidate loop, a random one, and the blob tests/fuse_batch_prog.cpp reads.

A scene is a dict: frames (fuse_batch_restatement.Frame), cams (CAMERA_DTYPE records), pos, normal, min_dist, max_dist, desc, th,
skip_point / skip_pair (or None), names (one per point) and `expect`, the restatement's answer.  The hand-made scenes share one camera:
R = I, t = 0, fx = fy = 256, (cx, cy) = (320, 240), bf = 40, a 640 x 480 image, scale factor 1.2, 8 levels; a point (X, Y, 4) projects
to (320 + 64 X, 240 + 64 Y) with every step exact, and a point on the optical axis stands at distance exactly 4."""
import functools

import numpy as np

import fuse_batch_restatement as R

F32 = np.float32
FX, CX, CY, BF, W, H = 256.0, 320.0, 240.0, 40.0, 640.0, 480.0
SCALE_FACTOR, NLEVELS = 1.2, 8


def scale_factors(nlevels=NLEVELS):
    s = np.ones(nlevels, F32)
    for i in range(1, nlevels):
        s[i] = s[i - 1] * F32(SCALE_FACTOR)
    return s


def inv_sigma2(nlevels=NLEVELS):
    s = scale_factors(nlevels)
    return (F32(1.0) / (s * s)).astype(F32)


def log_scale_factor():
    return R.logf(F32(SCALE_FACTOR))


def camera(Rcw=None, tcw=None, Ow=None, scw_variant=0, nlevels=NLEVELS, bounds=(0.0, W, 0.0, H)):
    c = np.zeros((), R.CAMERA_DTYPE)
    c["Rcw"] = np.eye(3, dtype=F32).ravel() if Rcw is None else np.asarray(Rcw, F32).ravel()
    c["tcw"] = 0 if tcw is None else tcw
    c["Ow"] = 0 if Ow is None else Ow
    c["fx"], c["fy"], c["cx"], c["cy"], c["bf"] = FX, FX, CX, CY, BF
    c["min_x"], c["max_x"], c["min_y"], c["max_y"] = bounds
    c["log_scale_factor"] = log_scale_factor(); c["nlevels"] = nlevels; c["scw_variant"] = scw_variant
    return c


def bits(n, seed=0):
    """A descriptor with exactly n bits set (against the all-zero descriptor of the hand-made points: distance n)."""
    d = np.zeros(256, np.uint8)
    d[np.random.default_rng(seed).permutation(256)[:n]] = 1
    return np.packbits(d)


def frame(keys, bounds=(0.0, W, 0.0, H), nlevels=NLEVELS, mono=False):
    """keys: (x, y, octave, right or None, descriptor)."""
    n = len(keys)
    right = None if mono else np.array([(-1.0 if k[3] is None else k[3]) for k in keys], F32)
    desc = np.array([k[4] for k in keys], np.uint8).reshape(n, 32)
    return R.Frame([k[0] for k in keys], [k[1] for k in keys], [k[2] for k in keys], right, desc, bounds, scale_factors(nlevels), inv_sigma2(nlevels))


def ulps(x, k):
    i = int(np.asarray(x, F32).view(np.int32))
    assert i > 0 and i + k > 0
    return np.array(i + k, np.int32).view(F32)[()]


def _scan(make, value, target):
    for step in range(64):
        for k in ((0,) if step == 0 else (step, -step)):
            x = ulps(F32(value), k)
            if make(x) == F32(target):
                return x
    raise AssertionError("no float gives %r" % (target,))


AXIS = (0.0, 0.0, 4.0)           # projects to (320, 240), ur = 310, distance 4


def _points(rows):
    """rows: (name, pos, normal, min_dist, max_dist, descriptor)."""
    return dict(names=[r[0] for r in rows], pos=np.array([r[1] for r in rows], F32), normal=np.array([r[2] for r in rows], F32),
                min_dist=np.array([r[3] for r in rows], F32), max_dist=np.array([r[4] for r in rows], F32),
                desc=np.array([r[5] for r in rows], np.uint8).reshape(len(rows), 32))


ZERO = np.zeros(32, np.uint8)
UP = (0.0, 0.0, 1.0)


def _toward(p):
    p = np.asarray(p, np.float64)
    return tuple(p / np.linalg.norm(p))


def _scene(frames, cams, rows, th=3.0, skip_point=None, skip_pair=None):
    sc = _points(rows)
    sc.update(frames=frames, cams=np.array(cams, R.CAMERA_DTYPE), th=th, skip_point=skip_point, skip_pair=skip_pair)
    return sc


def _depth_and_image():
    far = (1.0, 100.0)
    rows = [("z_zero", (0.5, 0.25, 0.0), UP, *far, ZERO), ("z_zero_axis", (0.0, 0.0, 0.0), UP, *far, ZERO),
            ("z_minus_zero", (0.5, 0.25, -0.0), UP, *far, ZERO), ("z_just_behind", (0.5, 0.25, -1e-30), UP, *far, ZERO),
            ("u_min", (-5.0, 0.0, 4.0), _toward((-5, 0, 4)), *far, ZERO), ("u_max", (5.0, 0.0, 4.0), _toward((5, 0, 4)), *far, ZERO),
            ("v_min", (0.0, -3.75, 4.0), _toward((0, -3.75, 4)), *far, ZERO), ("v_max", (0.0, 3.75, 4.0), _toward((0, 3.75, 4)), *far, ZERO),
            ("u_below_min", (ulps(5.0, 1) * -1, 0.0, 4.0), _toward((-5, 0, 4)), *far, ZERO),
            ("u_below_max", (ulps(5.0, -2), 0.0, 4.0), _toward((5, 0, 4)), *far, ZERO)]
    return _scene([frame([])], [camera()], rows)


def _distance_and_angle():
    lo = _scan(lambda m: F32(0.8) * m, 5.0, 4.0)                     # 0.8f * lo == 4 exactly
    hi = _scan(lambda m: F32(1.2) * m, 4.0 / 1.2, 4.0)               # 1.2f * hi == 4 exactly
    while F32(0.8) * ulps(lo, 1) == F32(4.0):
        lo = ulps(lo, 1)                                             # the last such float: the next one puts the point too near
    while F32(1.2) * ulps(hi, -1) == F32(4.0):
        hi = ulps(hi, -1)
    half = (np.sqrt(0.75), 0.0, 0.5)
    rows = [("at_min", AXIS, UP, lo, 100.0, ZERO), ("below_min", AXIS, UP, ulps(lo, 1), 100.0, ZERO),
            ("at_max", AXIS, UP, 0.1, hi, ZERO), ("above_max", AXIS, UP, 0.1, ulps(hi, -1), ZERO),
            ("cos_at_half", AXIS, half, 1.0, 100.0, ZERO), ("cos_below_half", AXIS, (half[0], 0.0, ulps(0.5, -1)), 1.0, 100.0, ZERO),
            ("cos_negative", AXIS, (0.0, 0.0, -1.0), 1.0, 100.0, ZERO)]
    return _scene([frame([])], [camera()], rows)


LEVEL_KS = tuple(range(0, NLEVELS + 1))
LEVEL_STEPS = tuple(range(-3, 4))


def _levels():
    """max_dist stepped through 7 consecutive floats around 4 * 1.2^k, where ceil(logf(ratio) / logf(1.2f)) changes; a ratio below 1 and
    huge ones for the clamps."""
    rows = []
    for k in LEVEL_KS:
        centre = F32(4.0 * 1.2 ** k)
        for s in LEVEL_STEPS:
            rows.append(("k%d%+d" % (k, s), AXIS, UP, 0.01, ulps(centre, s), ZERO))
    rows += [("ratio_below_one", AXIS, UP, 0.01, 3.5, ZERO), ("ratio_huge", AXIS, UP, 0.01, 1e30, ZERO), ("ratio_inf", AXIS, UP, 0.01, np.inf, ZERO)]
    return _scene([frame([]), frame([])], [camera(), camera(nlevels=3)], rows)


def _windows():
    """Level 2 is predicted (max_dist = 5.5: ratio 1.375, between 1.2 and 1.44), the window is 3 * 1.44 = 4.32 pixels."""
    p = ("p", AXIS, UP, 0.01, 5.5, ZERO)
    d = bits(10)
    empty = frame([(100.0, 100.0, 2, 90.0, d), (330.0, 240.0, 2, 320.0, d)])                          # keys, none in the window
    wrong = frame([(321.0, 240.0, 0, 311.0, d), (319.0, 241.0, 3, 309.0, d)])                         # only pred - 2 and pred + 1
    right_levels = frame([(321.0, 240.0, 1, 311.0, bits(30, 1)), (319.0, 240.0, 2, 309.0, bits(20, 2)), (320.0, 241.0, 3, 310.0, bits(5, 3))])
    return _scene([empty, wrong, right_levels, frame([])], [camera()] * 4, [p])


def _gates():
    """Level 0 (max_dist = 4: ratio 1), window 3 pixels, inv_sigma2 = 1: e2 is the squared pixel error.  Keys one at a time."""
    p = ("p", AXIS, UP, 0.01, 4.0, ZERO)
    d = bits(10)
    one = lambda dx, right: frame([(320.0 + dx, 240.0, 0, right, d)])
    frames = [one(2.79, 310.0), one(2.8, 310.0), one(2.44, None), one(2.45, None)]
    frames.append(frame([(320.0 + 2.44, 240.0, 0, None, d)], mono=True))                              # a frame without mvRight at all
    frames.append(one(1.0, 310.0 + 2.7))                                                              # the right coordinate alone: 1 + 7.29
    frames = frames + frames
    return _scene(frames, [camera()] * 6 + [camera(scw_variant=1)] * 6, [p])


def _ties_and_threshold():
    """Level 3 (max_dist = 6: ratio 1.5 between 1.44 and 1.728), window 3 * 1.728 = 5.18; the Scw form, so that no gate interferes."""
    p = ("p", AXIS, UP, 0.01, 6.0, ZERO)
    d = bits(20)
    across = frame([(325.1, 240.0, 3, None, d), (315.1, 240.0, 3, None, bits(20, 9))])        # key 1 lies in the earlier grid column
    within = frame([(321.0, 240.0, 3, None, d), (319.0, 240.0, 3, None, bits(20, 9))])        # one cell: index order
    later_better = frame([(321.0, 240.0, 3, None, d), (319.0, 240.0, 3, None, bits(19, 9))])
    at50 = frame([(321.0, 240.0, 3, None, bits(50))])
    at51 = frame([(321.0, 240.0, 3, None, bits(51))])
    all_bits = frame([(321.0, 240.0, 3, None, bits(256))])
    frames = [across, within, later_better, at50, at51, all_bits]
    sc = _scene(frames * 2, [camera(scw_variant=1)] * 6 + [camera()] * 6, [p])
    return sc


def _masks():
    """Two keyframes, four points that all match; the masks take pairs out."""
    d = bits(10)
    f = frame([(321.0, 240.0, 0, 311.0, d)])
    rows = [("p%d" % i, AXIS, UP, 0.01, 4.0, ZERO) for i in range(4)]
    return _scene([f, f], [camera(), camera(scw_variant=1)], rows, skip_point=np.array([0, 1, 0, 0], np.uint8),
                  skip_pair=np.array([[0, 0, 1, 0], [1, 0, 0, 0]], np.uint8))


def _posed():
    """A camera that is not the identity, in both forms: the rows of R * X + t and the camera centre as given."""
    a = 0.3
    Rm = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float64)
    t = np.array([0.3, -0.2, 0.5])
    Rf, tf = Rm.astype(F32), t.astype(F32)
    Ow = np.array([F32(-sum(np.float64(Rf[r, c]) * np.float64(tf[r]) for r in range(3))) for c in range(3)], F32)
    rng = np.random.default_rng(5)
    cam_pts = np.stack([rng.uniform(-4, 4, 24), rng.uniform(-3, 3, 24), rng.uniform(-1, 9, 24)], 1)
    world = ((cam_pts - t) @ Rm).astype(F32)
    rows = []
    for i, X in enumerate(world):
        po = X.astype(np.float64) - Ow
        dist = np.linalg.norm(po)
        n = po / dist if i % 5 else -po / dist
        rows.append(("r%d" % i, tuple(X), tuple(n), dist * (0.5 if i % 7 else 1.3), dist * (1.5 if i % 3 else 0.8), bits(128, i)))
    keys = [(float(x), float(y), int(o), (float(x) - 5.0 if o % 2 else None), bits(128 + (i % 9) - 4, i))
            for i, (x, y, o) in enumerate(zip(rng.uniform(0, W, 300), rng.uniform(0, H, 300), rng.integers(0, NLEVELS, 300)))]
    f = frame(keys)
    return _scene([f, f], [camera(Rf, tf, Ow), camera(Rf, tf, Ow, scw_variant=1)], rows, th=4.0)


HAND = {"depth_and_image": _depth_and_image, "distance_and_angle": _distance_and_angle, "levels": _levels, "windows": _windows,
        "gates": _gates, "ties_and_threshold": _ties_and_threshold, "masks": _masks, "posed": _posed}
HAND_SCENES = tuple(HAND)


def expect(sc):
    return R.fuse_batch(sc["frames"], sc["cams"], sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], sc["desc"], sc["th"],
                        sc["skip_point"], sc["skip_pair"])


@functools.lru_cache(maxsize=None)
def scene(name):
    sc = HAND[name]() if name in HAND else random_scene()
    sc["expect"] = expect(sc)
    for v in sc["expect"].values():
        v.setflags(write=False)
    return sc


# ---- the random scene: 5 keyframes x 203 points -------------------------------------------------------------------------------------
RANDOM_KEYS = (0, 1, 63, 300, 1200)


def random_scene():
    """Keyframes with 0, 1, 63, 300 and 1200 keys around one pose each, stereo and mono keys mixed, the Tcw and the Scw form mixed; the
    points are spread in front of the first camera.  In the last keyframe 90 keys crowd one grid cell (a window then holds more than 64
    candidates: the lane stride and the merge across lanes), and many descriptors are near copies of point descriptors, so that
    matches, ties in distance and distances around 50 all occur."""
    rng = np.random.default_rng(2024)
    N = 203
    cam_pts = np.stack([rng.uniform(-5, 5, N), rng.uniform(-3.8, 3.8, N), rng.uniform(2, 9, N)], 1)
    cam_pts[:40] = np.stack([rng.uniform(-0.05, 0.05, 40), rng.uniform(-0.05, 0.05, 40), rng.uniform(3.9, 4.1, 40)], 1)    # the crowd's viewers
    pos = cam_pts.astype(F32)
    dist = np.linalg.norm(pos.astype(np.float64), axis=1)
    normal = (pos / dist[:, None]).astype(F32)
    normal[::17] *= -1
    max_dist = (dist * rng.uniform(0.9, 3.5, N)).astype(F32)
    min_dist = (max_dist / F32(3.58)).astype(F32)
    desc = rng.integers(0, 256, (N, 32), dtype=np.uint8)

    def near_copy(i, flips):
        d = np.unpackbits(desc[i]).copy()
        d[rng.permutation(256)[:flips]] ^= 1
        return np.packbits(d)

    frames, cams = [], []
    for k, nk in enumerate(RANDOM_KEYS):
        a = 0.02 * (4 - k)                               # the last keyframe stands at the identity: the crowd's cell is (32, 24)
        Rm = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float64)
        t = np.array([0.05, -0.02, 0.03]) * (4 - k)
        Rf, tf = Rm.astype(F32), t.astype(F32)
        Ow = np.array([F32(-sum(np.float64(Rf[r, c]) * np.float64(tf[r]) for r in range(3))) for c in range(3)], F32)
        keys = []
        for j in range(nk):
            i = int(rng.integers(0, N))
            pc = Rm @ pos[i].astype(np.float64) + t
            x, y = FX * pc[0] / pc[2] + CX + rng.normal(0, 1.2), FX * pc[1] / pc[2] + CY + rng.normal(0, 1.2)
            if nk == 1200 and j < 90:
                i = j % 40
                x, y = 320.0 + rng.uniform(-3.0, 3.0), 240.0 + rng.uniform(-3.0, 3.0)
            x, y = float(np.clip(x, 0.5, W - 1)), float(np.clip(y, 0.5, H - 1))
            right = x - BF / pc[2] + rng.normal(0, 0.5) if j % 3 else None
            keys.append((x, y, int(rng.integers(0, 4)), right, near_copy(i, int(rng.choice([0, 20, 45, 50, 51, 60, 120])))))
        frames.append(frame(keys, mono=(k == 2)))
        cams.append(camera(Rf, tf, Ow, scw_variant=k % 2))
    rows = [("q%d" % i, tuple(pos[i]), tuple(normal[i]), min_dist[i], max_dist[i], desc[i]) for i in range(N)]
    return _scene(frames, cams, rows, th=3.0)


# ---- the host program's blob ----------------------------------------------------------------------------------------------------------
POINTERS = ("kfs", "cams", "pos", "normal", "min_dist", "max_dist", "mp_desc", "skip_point", "skip_pair", "best_idx", "best_dist", "status",
            "u", "v", "ur", "level")
OUT = (("best_idx", np.int32), ("best_dist", np.int32), ("status", np.uint8), ("u", F32), ("v", F32), ("ur", F32), ("level", np.int32))


def _arr(a, dt):
    a = np.ascontiguousarray(a, dt).ravel()
    return np.array([a.size], np.int64).tobytes() + a.tobytes()


def frame_blob(f, device=0, is_null=False, nlevels=None):
    nl = len(f.scale) if nlevels is None else nlevels
    head = np.array([f.n, nl, device, f.u_right is not None, is_null], np.int32).tobytes() + np.array(f.bounds, F32).tobytes()
    right = f.u_right if f.u_right is not None else np.zeros(0, F32)
    return head + _arr(f.x, F32) + _arr(f.y, F32) + _arr(f.octave, np.int32) + _arr(right, F32) + _arr(f.desc, np.uint8) + \
        _arr(f.scale[:nl], F32) + _arr(f.inv_sigma2[:nl], F32)


def blob(sc, n_kf=None, n_mp=None, null=(), devices=None, null_frames=(), pairs_out=None):
    K, N = len(sc["frames"]), len(sc["pos"])
    n_kf = K if n_kf is None else n_kf
    n_mp = N if n_mp is None else n_mp
    mask = sum(1 << POINTERS.index(p) for p in null)
    pairs = K * N if pairs_out is None else pairs_out
    out = np.array([n_kf, n_mp], np.int32).tobytes() + np.array([sc["th"]], F32).tobytes() + np.array([mask], np.uint32).tobytes()
    out += np.array([pairs, K], np.int64).tobytes()
    for k, f in enumerate(sc["frames"]):
        out += frame_blob(f, device=0 if devices is None else devices[k], is_null=k in null_frames)
    out += _arr(np.frombuffer(np.asarray(sc["cams"], R.CAMERA_DTYPE).tobytes(), np.uint8), np.uint8)
    out += _arr(sc["pos"], F32) + _arr(sc["normal"], F32) + _arr(sc["min_dist"], F32) + _arr(sc["max_dist"], F32) + _arr(sc["desc"], np.uint8)
    out += _arr(sc["skip_point"] if sc["skip_point"] is not None else np.zeros(0, np.uint8), np.uint8)
    out += _arr(sc["skip_pair"] if sc["skip_pair"] is not None else np.zeros(0, np.uint8), np.uint8)
    return out


def parse(raw, pairs, shape=None):
    rc, n = (int(v) for v in np.frombuffer(raw, np.int32, 2))
    text = raw[8:8 + n].decode()
    at, got = 8 + n, {}
    for name, dt in OUT:
        got[name] = np.frombuffer(raw, dt, pairs, at).copy()
        at += pairs * np.dtype(dt).itemsize
        if shape is not None:
            got[name] = got[name].reshape(shape)
    assert at == len(raw)
    return rc, text, got


def differences(got, want):
    """The names of the outputs that differ: integers by value, floats by their bits."""
    bad = []
    for name, dt in OUT:
        a, b = np.ascontiguousarray(got[name], dt), np.ascontiguousarray(want[name], dt)
        if a.shape != b.shape or a.tobytes() != b.tobytes():
            bad.append(name)
    return bad
