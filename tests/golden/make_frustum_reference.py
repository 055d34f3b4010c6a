"""Writes tests/golden/frustum_reference.npz from the reference's own Frame::isInFrustum (src/orbslam/Frame.cc compiled untouched into
oracle/_ref/libref_frame.so by `make -C oracle ref` where the reference's sources are at hand): for each group of points of
tests/frustum_pin_cases.py whether the point is in view, mTrackProjX / mTrackProjY / mTrackProjXR / mTrackViewCos and mnTrackScaleLevel.
Data only.  Before it writes, it checks that the cases reach what they were built for, from the reference's answers alone:
  * on the probes, every exit of the function is taken at least 10 times and every level holds at least 10 points in view.  The function
    tells only in view or not; the exit is found by asking again with the later tests switched off (cos limit -inf: what appears was
    rejected for its viewing angle; then also min_dist 0 and max_dist inf: what appears was rejected for its distance) and, for the three
    tests in front, which cannot be switched off, from the points' geometry in float64 (none of the probes lies within 1e-3 of a bound);
  * in the sweep the level changes inside exactly the 3 x (nlevels - 1) rows that are not clamped, and the k = -1 rows are cut by the
    distance gate.
Run from the repository root:
    python tests/golden/make_frustum_reference.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import frustum_pin_cases as P   # noqa: E402
import pin_frame_common as FC   # noqa: E402


def check_probes(ref):
    g = P.inputs("probes")
    inv = ref["in_view"] != 0
    no_angle = P.reference("probes", cos_limit=-np.inf)["in_view"] != 0
    no_dist = P.reference("probes", cos_limit=-np.inf, relax_distance=True)["in_view"] != 0
    assert (no_angle | ~inv).all() and (no_dist | ~no_angle).all()
    T = g["Tcw"].astype(np.float64)
    pc = g["pos"].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    with np.errstate(all="ignore"):
        u, v = FC.FX * pc[:, 0] / pc[:, 2] + FC.CX, FC.FY * pc[:, 1] / pc[:, 2] + FC.CY
    behind = pc[:, 2] < 0
    u_out = ~behind & ((u < P.BOUNDS[0]) | (u > P.BOUNDS[1]))
    v_out = ~behind & ~u_out & ((v < P.BOUNDS[2]) | (v > P.BOUNDS[3]))
    margin = np.minimum.reduce([np.abs(pc[:, 2]), np.abs(u - P.BOUNDS[0]), np.abs(u - P.BOUNDS[1]), np.abs(v - P.BOUNDS[2]), np.abs(v - P.BOUNDS[3])])
    assert margin[~behind].min() > 1e-3 and np.abs(pc[:, 2]).min() > 1e-3
    assert np.array_equal(behind | u_out | v_out, ~no_dist), "the three tests in front: the geometry and the reference disagree"
    counts = {"in view": int(inv.sum()), "behind": int(behind.sum()), "u": int(u_out.sum()), "v": int(v_out.sum()),
              "distance": int((no_dist & ~no_angle).sum()), "angle": int((no_angle & ~inv).sum())}
    levels = np.bincount(ref["level"][inv], minlength=P.NLEVELS)
    print("probes:", counts, "in view per level:", levels.tolist())
    assert sum(counts.values()) == len(inv) and min(counts.values()) >= 10 and len(levels) == P.NLEVELS and levels.min() >= 10


def check_sweep(ref):
    steps = len(P.SWEEP_STEPS)
    inv = (ref["in_view"] != 0).reshape(-1, steps)
    level = ref["level"].reshape(-1, steps)
    k = P.inputs("sweep")["k"].reshape(-1, steps)[:, 0]
    changes = np.array([len(set(level[r][inv[r]].tolist())) > 1 for r in range(len(k))])
    print("sweep: the level changes in", int(changes.sum()), "rows; rejected points in the k = -1 rows:", int((~inv[k == -1]).sum()))
    assert np.array_equal(changes, (k >= 0) & (k <= P.NLEVELS - 2)) and int(changes.sum()) == 3 * (P.NLEVELS - 1)
    for r in np.flatnonzero(changes):
        assert sorted(set(level[r].tolist())) == [k[r], k[r] + 1] and inv[r].all() and (np.diff(level[r]) >= 0).all()
    assert inv[k >= 0].all()
    cut = inv[k == -1]
    assert (~cut).any(axis=1).all() and cut.any(axis=1).all() and (np.diff(cut.astype(int), axis=1) >= 0).all()      # rejected below, in view above


def write(path=P.GOLDEN):
    out = {}
    for group in P.GROUPS:
        ref = P.reference(group)
        {"probes": check_probes, "sweep": check_sweep}.get(group, lambda r: None)(ref)
        for key, val in ref.items():
            out[group + "." + key] = val
    hand = dict(zip(P.HAND_NAMES, out["hand.in_view"].tolist()))
    print("hand:", hand)
    for name in ("u_min", "u_max", "v_min", "v_max", "cos_above", "plain", "skipped_0", "skipped_1"):
        assert hand[name] == 1, name
    for name in ("u_below_min", "u_above_max", "v_below_min", "v_above_max", "cos_below", "z_plus_zero", "z_minus_zero"):
        assert hand[name] == 0, name
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 128 * 1024
    return path


if __name__ == "__main__":
    assert P.reference_present(), "oracle/_ref/libref_frame.so is missing: run `make -C oracle ref` where the reference's sources are"
    print(write(), os.path.getsize(P.GOLDEN), "bytes")
