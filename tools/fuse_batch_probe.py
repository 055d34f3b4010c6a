"""Times sivo_fuse_batch against the loop it replaces, at the two shapes of its callers:
  neighbors  60 keyframes x 1500 points, 85 % of the pairs masked (LocalMapping::SearchInNeighbors: most points are in most neighbours),
  loop       100 keyframes x 4000 points, nothing masked (LoopClosing::SearchAndFuse),
each keyframe with 2000 keys of a 640 x 480 image, stereo and mono mixed, poses a few centimetres apart.

Batch: the time of the C ABI call with the arrays ready (one staged upload, one launch, one download, one synchronise inside the
library), by a host clock around the call.  Loop: one sivo_fuse per keyframe on the SAME pairs, fed with the projections the batch
returned — the device round trips of today's ORBmatcher::Fuse loop WITHOUT its host projection (pose product, norm, viewing angle,
PredictScale per pair), which today's loop pays on top; so the loop figure is a lower bound of what the batch replaces.  The answers of
the two are compared.  Medians and quartiles, one JSON line.  No pass mark; arrays only, so no surgery and no repair call.
    python tools/fuse_batch_probe.py [--repeats 30] [--warmup 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sivo_amd import _lib, matcher as M, tracking  # noqa: E402

W, H, FX, CX, CY, BF, NLEVELS, SCALE = 640.0, 480.0, 256.0, 320.0, 240.0, 40.0, 8, 1.2
REACHED = (0, 6, 7)


def scene(n_kf, n_mp, n_keys, masked, scw, seed):
    rng = np.random.default_rng(seed)
    scale = np.cumprod(np.r_[1.0, np.full(NLEVELS - 1, SCALE)]).astype(np.float32)
    cam_pts = np.stack([rng.uniform(-6, 6, n_mp), rng.uniform(-4.5, 4.5, n_mp), rng.uniform(2, 10, n_mp)], 1)
    pos = cam_pts.astype(np.float32)
    dist = np.linalg.norm(pos.astype(np.float64), axis=1)
    normal = (pos / dist[:, None]).astype(np.float32)
    max_dist = (dist * rng.uniform(0.9, 3.5, n_mp)).astype(np.float32)
    min_dist = (max_dist / np.float32(3.58)).astype(np.float32)
    desc = rng.integers(0, 256, (n_mp, 32), dtype=np.uint8)
    frames, cams = [], np.zeros(n_kf, M.FUSE_CAMERA_DTYPE)
    for k in range(n_kf):
        a = 0.002 * k
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        t = np.array([0.02, -0.01, 0.015]) * k
        keys = np.zeros(n_keys, M.KP_DTYPE)
        # half of the keys near projections of points (with near copies of their descriptors), half anywhere
        i = rng.integers(0, n_mp, n_keys)
        pc = pos[i].astype(np.float64) @ R.T + t
        near = rng.random(n_keys) < 0.5
        keys["x"] = np.clip(np.where(near, FX * pc[:, 0] / pc[:, 2] + CX + rng.normal(0, 1.0, n_keys), rng.uniform(0, W, n_keys)), 0.5, W - 1)
        keys["y"] = np.clip(np.where(near, FX * pc[:, 1] / pc[:, 2] + CY + rng.normal(0, 1.0, n_keys), rng.uniform(0, H, n_keys)), 0.5, H - 1)
        keys["octave"] = rng.integers(0, 4, n_keys)
        right = np.where(rng.random(n_keys) < 0.7, keys["x"] - BF / pc[:, 2], -1.0).astype(np.float32)
        kd = desc[i] ^ np.where(rng.random((n_keys, 32)) < 0.04, rng.integers(0, 256, (n_keys, 32)), 0).astype(np.uint8)
        frames.append(M.MatchFrame(keys, right, kd, (0.0, W, 0.0, H), scale, scale * scale, 1.0 / (scale * scale)))
        c = cams[k]
        Rf, tf = R.astype(np.float32), t.astype(np.float32)
        c["Rcw"], c["tcw"] = Rf.ravel(), tf
        c["Ow"] = (-(Rf.astype(np.float64).T @ tf.astype(np.float64))).astype(np.float32)
        c["fx"], c["fy"], c["cx"], c["cy"], c["bf"] = FX, FX, CX, CY, BF
        c["min_x"], c["max_x"], c["min_y"], c["max_y"] = 0.0, W, 0.0, H
        c["log_scale_factor"], c["nlevels"], c["scw_variant"] = tracking.log_scale_factor(SCALE), NLEVELS, scw
    skip_pair = (rng.random((n_kf, n_mp)) < masked).astype(np.uint8) if masked else None
    return dict(frames=frames, cams=cams, pos=pos, normal=normal, min_dist=min_dist, max_dist=max_dist, desc=desc, skip_pair=skip_pair, scw=scw)


def quartiles(t):
    q = np.percentile(np.array(t) * 1e3, [25, 50, 75])
    return dict(median_ms=round(float(q[1]), 3), q25_ms=round(float(q[0]), 3), q75_ms=round(float(q[2]), 3))


def timed(call, repeats, warmup):
    for _ in range(warmup):
        call()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        t.append(time.perf_counter() - t0)
    return quartiles(t)


def measure(name, sc, th, repeats, warmup):
    batch = lambda extras: M.fuse_batch(sc["frames"], sc["cams"], sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], sc["desc"], th,
                                        skip_pair=sc["skip_pair"], extras=extras)
    full = batch(True)
    valid = np.isin(full["status"], REACHED)
    z = lambda a, k: np.where(valid[k], a[k], 0).astype(a.dtype)
    per_kf = [(valid[k].astype(np.uint8), z(full["u"], k), z(full["v"], k), None if sc["scw"] else z(full["ur"], k), z(full["level"], k))
              for k in range(len(sc["frames"]))]

    def loop():
        return [M.fuse(f, *per_kf[k], sc["desc"], th, sc["scw"]) for k, f in enumerate(sc["frames"])]

    singles = loop()
    same = all(np.array_equal(full["best_idx"][k], s[1]) and np.array_equal(full["best_dist"][k], s[2]) for k, s in enumerate(singles))
    return dict(scene=name, n_kf=len(sc["frames"]), n_mp=len(sc["pos"]), keys_per_keyframe=sc["frames"][0].n,
                pairs_searched=int(valid.sum()), matched=int((full["status"] == 0).sum()), same_answers=bool(same),
                batch=timed(lambda: batch(False), repeats, warmup), loop_of_single_calls=timed(loop, repeats, warmup))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    _lib.require_gpu()
    out = [measure("neighbors", scene(60, 1500, 2000, 0.85, 0, 1), 3.0, a.repeats, a.warmup),
           measure("loop", scene(100, 4000, 2000, 0.0, 1, 2), 4.0, a.repeats, a.warmup)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
