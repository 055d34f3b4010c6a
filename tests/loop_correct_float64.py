"""A second opinion on tests/loop_correct_restatement.py: the two map corrections of the loop closer as plain float64 linear algebra on
rotation matrices — no Sim3 quaternions, no float32 rounding rules, numpy's inverse and a breadth-first walk in place of the chains.  It
shares nothing with the restatement or the code under test but the reading of the reference (src/orbslam/LoopClosing.cc:436-526,
:694-753), so an order-of-operations or a which-camera-centre mistake in either shows up at the size of the motion, while the two agree to
float32 rounding when both are right.  Test infrastructure, not the product."""
import collections

import numpy as np

D = np.float64


def _quat_matrix(q):
    x, y, z, w = np.asarray(q, D) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def correct_loop(a):
    """The arguments of sivo_loop_correct -> tiw_out, ow_out (n_kf), corrected_by, pos_out, normal, max_dist, min_dist (n_points; NaN where
    the call writes nothing)."""
    K, P = a["n_kf"], a["n_points"]
    T = np.asarray(a["tiw"], D).reshape(K, 4, 4)
    Twc = np.asarray(a["twc_cur"], D).reshape(4, 4)
    scw = np.asarray(a["scw"], D)
    Rs, ts, s = _quat_matrix(scw[:4]), scw[4:7], scw[7]
    Rc, tc, sc = [], [], []
    for i in range(K):
        if i == a["cur"]:
            Rc.append(Rs); tc.append(ts); sc.append(s)
        else:
            Tic = T[i] @ Twc
            Rc.append(Tic[:3, :3] @ Rs); tc.append(Tic[:3, :3] @ ts + Tic[:3, 3]); sc.append(s)
    tiw_out = np.tile(np.eye(4), (K, 1, 1))
    ow_out = np.zeros((K, 3))
    for i in range(K):
        tiw_out[i, :3, :3], tiw_out[i, :3, 3] = Rc[i], tc[i] / sc[i]
        ow_out[i] = -Rc[i].T @ tc[i] / sc[i]
    by = np.full(P, -1, np.int64)
    for i in range(K - 1, -1, -1):                          # the earliest holder overwrites the later ones
        for p in a["slot_point"][a["slot_off"][i]:a["slot_off"][i + 1]]:
            if p >= 0 and not a["skip"][p]:
                by[p] = i
    out = {"tiw_out": tiw_out, "ow_out": ow_out, "corrected_by": by, "pos_out": np.full((P, 3), np.nan), "normal": np.full((P, 3), np.nan),
           "max_dist": np.full(P, np.nan), "min_dist": np.full(P, np.nan)}
    ow = np.asarray(a["ow"], D).reshape(-1, 3)
    for p in np.flatnonzero(by >= 0):
        i = by[p]
        Y = T[i, :3, :3] @ np.asarray(a["pos"][p], D) + T[i, :3, 3]
        Z = Rc[i].T @ (Y - tc[i]) / sc[i]
        out["pos_out"][p] = Z
        obs = a["obs_kf"][a["obs_off"][p]:a["obs_off"][p + 1]]
        if len(obs) == 0:
            continue
        centre = lambda k: ow_out[k] if k < K and k < i else ow[k]
        n = np.zeros(3)
        for k in obs:
            d = Z - centre(k)
            n += d / np.linalg.norm(d)
        out["normal"][p] = n / len(obs)
        out["max_dist"][p] = np.linalg.norm(Z - centre(a["ref_kf"][p])) * D(a["level_scale"][p])
        out["min_dist"][p] = out["max_dist"][p] / D(a["last_scale"][p])
    return out


def propagate_global_ba(a):
    """The arguments of sivo_gba_propagate -> tcw_out (NaN rows for unreached keyframes), kf_reached, pos_out (NaN where nothing is
    written)."""
    K, P = a["n_kf"], a["n_points"]
    tcw = np.asarray(a["tcw"], D).reshape(K, 4, 4)
    gba = np.asarray(a["tcw_gba"], D).reshape(K, 4, 4).copy()
    bef = np.asarray(a["tcw_bef"], D).reshape(K, 4, 4).copy()
    inside = np.asarray(a["in_gba"]).astype(bool).copy()
    new = tcw.copy()
    reached = np.zeros(K, bool)
    queue = collections.deque(int(o) for o in a["origin"])
    while queue:
        k = queue.popleft()
        for c in a["child_kf"][a["child_off"][k]:a["child_off"][k + 1]]:
            if not inside[c]:
                gba[c] = tcw[c] @ np.linalg.inv(tcw[k]) @ gba[k]
                inside[c] = True
            queue.append(int(c))
        bef[k], new[k], reached[k] = tcw[k], gba[k], True
    out = {"tcw_out": np.where(reached[:, None, None], new, np.nan), "kf_reached": reached, "pos_out": np.full((P, 3), np.nan)}
    for p in range(P):
        if a["point_bad"][p]:
            continue
        if a["point_in_gba"][p]:
            out["pos_out"][p] = a["pos_gba"][p]
            continue
        r = a["ref_kf"][p]
        if not inside[r]:
            continue
        X = np.append(np.asarray(a["pos"][p], D), 1.0)
        out["pos_out"][p] = (np.linalg.inv(new[r]) @ bef[r] @ X)[:3]
    return out


def differences(name_pairs, got, want, written):
    """max |got - want| over the written entries: `pose` entries absolutely, `point` entries relative to the largest |coordinate| among
    the written entries of `want`."""
    out = {}
    for name, kind in name_pairs:
        g, w = np.asarray(got[name], D), np.asarray(want[name], D)
        m = written[name] if name in written else np.ones(len(w), bool)
        if not m.any():
            continue
        diff = float(np.max(np.abs(g[m] - w[m])))
        out[name] = diff if kind == "pose" else diff / max(1.0, float(np.max(np.abs(w[m]))))
    return out
