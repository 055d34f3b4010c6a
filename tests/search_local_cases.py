"""Scenes for Tracking::SearchLocalPoints on arrays, shared by tests/test_pin_frustum.py (the C++ adapter over the host build) and
tests/test_gpu_frustum.py (the fused device path): the probes of tests/frustum_pin_cases.py as the local map, a frame whose keys lie at the
projections the REFERENCE computed for the points in view (tests/golden/frustum_reference.npz), and the expected result from the sequential
oracle (oracle/search.py) fed with the reference's track fields."""
import numpy as np

import frustum_pin_cases as P
from oracle.oracle import KP_DTYPE

F32 = np.float32
POINT_OUT = np.dtype([("visible", np.int32), ("last_seen", np.int64), ("in_view", np.int32), ("track", F32, 4), ("level", np.int32)])


def _noisy(rng, desc, bits):
    """Copies of 32-byte descriptors with `bits` random bits flipped."""
    out = np.unpackbits(desc, axis=1)
    for row in out:
        row[rng.choice(256, bits, replace=False)] ^= 1
    return np.packbits(out, axis=1)


def local_map(n_dup, seed):
    """The 600 probes and n_dup twins of points in view (same geometry, another noisy copy of the same descriptor: a twin and its original
    choose the same keypoint, so the engine's repair rounds run).  `src` maps every point to the probe whose track fields it has."""
    rng = np.random.default_rng(seed)
    g, ref = P.inputs("probes"), P.recorded("probes")
    iv = np.flatnonzero(ref["in_view"])
    src = np.concatenate([np.arange(len(g["pos"])), rng.choice(iv, n_dup, replace=False)])
    base = rng.integers(0, 256, (len(g["pos"]), 32), dtype=np.uint8)
    desc = _noisy(rng, base[src], 12)
    obs = rng.integers(0, 6, len(src)).astype(np.int32)                 # 0: a point without observations does not block its keypoint
    m = {k: np.ascontiguousarray(g[k][src]) for k in ("pos", "normal", "min_dist", "max_dist")}
    m.update(Tcw=g["Tcw"], src=src, base=base, desc=desc, obs=obs, n=len(src))
    return m


def frame_keys(m, n_keys, seed):
    """n_keys keypoints at the reference's projections of points in view (several per point once the points run out), one octave at or
    below the predicted level, a noisy copy of the point's base descriptor, mvRight near the projection into the right image or -1."""
    rng = np.random.default_rng(seed)
    ref = P.recorded("probes")
    iv = np.flatnonzero(ref["in_view"])
    of = np.concatenate([rng.permutation(iv), rng.choice(iv, max(0, n_keys - len(iv)))])[:n_keys]
    keys = np.zeros(n_keys, KP_DTYPE)
    far = np.where(rng.random(n_keys) < 0.3, 6.0, 1.0)                  # three keys in ten lie outside the window of th = 1
    keys["x"] = ref["track"][of, 0] + (far * rng.uniform(-1.5, 1.5, n_keys)).astype(F32)
    keys["y"] = ref["track"][of, 1] + (far * rng.uniform(-1.5, 1.5, n_keys)).astype(F32)
    keys["octave"] = np.maximum(ref["level"][of] - rng.integers(0, 2, n_keys), 0)
    keys["size"], keys["angle"], keys["class_id"] = 31, rng.uniform(0, 360, n_keys), -1
    ur = (ref["track"][of, 2] + rng.uniform(-1, 1, n_keys)).astype(F32)
    ur[rng.random(n_keys) < 0.2] = -1
    desc = _noisy(rng, m["base"][of], 20)
    s = P.scale_factors()
    return dict(keys=keys, u_right=ur, desc=desc, of=of, scale=s, sigma2=(s * s).astype(F32), inv_sigma2=(F32(1) / (s * s)).astype(F32))


def oracle_frame(fk):
    from oracle import search as OS
    return OS.Frame(fk["keys"], fk["u_right"], fk["desc"], P.BOUNDS, fk["scale"], fk["sigma2"], fk["inv_sigma2"])


def oracle_search(fk, m, in_view, th, nn_ratio, occ_obs, order=None):
    """SearchByProjection of the sequential oracle over the points in `order`, with the REFERENCE's mTrack* fields."""
    from oracle import search as OS
    ref = P.recorded("probes")
    order = np.arange(m["n"]) if order is None else np.asarray(order)
    s = m["src"][order]
    return OS.search_by_projection_mappoints(oracle_frame(fk), in_view[order].astype(np.uint8), ref["track"][s, 0], ref["track"][s, 1], ref["track"][s, 2],
                                             ref["level"][s], ref["track"][s, 3], m["desc"][order], m["obs"][order], th, nn_ratio, occ_obs)


# ---------------------------------------------------------------------------------------------------------------------
# the adapter's scene
# ---------------------------------------------------------------------------------------------------------------------
def bookkeeping_scene(frame_id, th=3.0, nn_ratio=0.8):
    rng = np.random.default_rng(77)
    m = local_map(20, 5)
    fk = frame_keys(m, 120, 6)
    n, nk = m["n"], 120
    ref = P.recorded("probes")
    bad = rng.random(n) < 0.1
    seen = rng.integers(1, frame_id, n).astype(np.int64)
    already = rng.random(n) < 0.05                                      # seen in this frame by some earlier step: skipped, not counted
    seen[already] = frame_id
    slot = np.full(nk, -1, np.int32)
    holders = rng.choice(np.flatnonzero(~already), 30, replace=False)
    slot[rng.choice(nk, 30, replace=False)] = holders
    bad[holders[::3]] = True; bad[holders[1::3]] = False
    obs = m["obs"].copy()
    local = rng.permutation(n).astype(np.int32)
    blob = b"".join([P.frustum_record(m["Tcw"]).tobytes(), np.array([th, nn_ratio], F32).tobytes(), np.array([frame_id, nk], np.int64).tobytes(),
                     fk["keys"].tobytes(), fk["u_right"].tobytes(), fk["desc"].tobytes(), slot.tobytes(), P.points_blob(m, n),
                     bad.astype(np.uint8).tobytes(), seen.tobytes(), obs.tobytes(), m["desc"].tobytes(), np.array([n], np.int64).tobytes(), local.tobytes()])
    slot_bad = np.zeros(nk, bool)
    slot_bad[slot >= 0] = bad[slot[slot >= 0]]
    return dict(blob=blob, m=m, fk=fk, n=n, nk=nk, bad=bad, seen=seen, slot=slot, slot_bad=slot_bad, local=local, th=th, nn_ratio=nn_ratio,
                frame_id=frame_id, ref_in_view=ref["in_view"][m["src"]] != 0)


def walk_search_local_points(sc, ref):
    """Tracking.cc:1033-1085 line by line on the scene's arrays; the cull's answers are the reference's (ref), the search the oracle's."""
    n, m = sc["n"], sc["m"]
    visible = np.zeros(n, np.int32); seen = sc["seen"].copy(); slots = sc["slot"].copy()
    for k, p in enumerate(sc["slot"]):                                  # :1035-1049
        if p < 0:
            continue
        if sc["bad"][p]:
            slots[k] = -1
        else:
            visible[p] += 1; seen[p] = sc["frame_id"]
    in_view = np.zeros(n, bool)
    for p in sc["local"]:                                               # :1054-1070
        if seen[p] == sc["frame_id"] or sc["bad"][p]:
            continue
        if sc["ref_in_view"][p]:
            in_view[p] = True; visible[p] += 1
    occ = np.array([m["obs"][p] if p >= 0 else -1 for p in slots], np.int32)
    nm, match, _ = oracle_search(sc["fk"], m, in_view, sc["th"], sc["nn_ratio"], occ, order=sc["local"])
    hit = match >= 0
    slots[hit] = sc["local"][match[hit]]
    return dict(visible=visible, last_seen=seen, in_view=in_view, slots=slots, n_matches=int(nm))
