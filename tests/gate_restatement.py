"""numpy restatement of entropy_gate_kernel (sivo_amd/csrc/select.hip): the lookup at the truncated key position, the criteria
and the decision of both forms (sivo_entropy_gate*: accept iff reduction > th; sivo_check_semantics*: the class unless
reduction < th), around triangulate_restatement.mutual_information (gate_math.hpp) — and the edge scene of the gate tests: a
7 x 13 map whose entries are all distinct, keys on and around every border, every kind of depth, Z = 0.  No device, no library."""
import numpy as np

import triangulate_restatement as TR

KP_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("size", np.float32), ("angle", np.float32),
                     ("response", np.float32), ("octave", np.int32), ("class_id", np.int32)])
VOID, TERRAIN = 255, 8
FX = FY = 718.856
BL = 0.537


def gate(kps, depth, xyz, entropy, Sx, fx, fy, bl, level_sigma2, th, confidence=None, classes=None, th_conf=None):
    """(mutual information, reduction, accept) of the kernel.  classes given: the CheckSemantics form, accept = detected class.
    A key fails — MI 0, reduction 0, accept 0 / class 255 — unless depth > 0 (NaN is not), the truncated position is inside the map,
    the octave is inside level_sigma2 and, in the CheckSemantics form, class <= TERRAIN and confidence >= th_conf."""
    n = len(kps)
    rows, cols = entropy.shape
    depth = np.asarray(depth, np.float32); xyz = np.asarray(xyz, np.float64).reshape(n, 3)
    ls2 = np.asarray(level_sigma2, np.float32)
    col = np.trunc(kps["x"].astype(np.float64)).astype(np.int64)          # (int)kp.x: towards zero, -0.25 -> 0
    row = np.trunc(kps["y"].astype(np.float64)).astype(np.int64)
    octave = kps["octave"].astype(np.int64)
    with np.errstate(invalid="ignore"):
        ok = (depth > 0) & (row >= 0) & (row < rows) & (col >= 0) & (col < cols) & (octave >= 0) & (octave < len(ls2))
    r, c = np.where(ok, row, 0), np.where(ok, col, 0)
    cls = np.full(n, VOID, np.int64)
    if classes is not None:
        cls = np.where(ok, classes[r, c], VOID)
        ok = ok & (cls <= TERRAIN) & (confidence[r, c] >= th_conf)
    sigma2 = ls2[np.where(ok, octave, 0)].astype(np.float64)
    m = TR.mutual_information(Sx, fx, fy, bl, xyz[:, 0].copy(), xyz[:, 1].copy(), xyz[:, 2].copy(), sigma2)
    mi = np.where(ok, m, 0.0)
    with np.errstate(invalid="ignore"):
        red = np.where(ok, mi - entropy[r, c], 0.0)
        if classes is not None:
            acc = np.where(ok & ~(red < th), cls, VOID).astype(np.uint8)
        else:
            acc = (ok & (red > th)).astype(np.uint8)
    return mi, red, acc


def covariance(rng, scale=1e-3):
    A = rng.standard_normal((6, 6))
    return A @ A.T * scale + np.eye(6) * scale * 0.1


def edge_positions(n):
    """On, just inside and just outside both ends of an axis of n cells (float32)."""
    return np.array([-1.0, -0.25, 0.0, 0.999, n - 1, n - 0.001, n, n + 5], np.float32)


DEPTHS = np.array([1.0, 0.0, -0.0, -1.0, np.nan, 1e-42, np.inf], np.float32)      # 1e-42 is a float32 denormal: > 0


def build_scene(rows=7, cols=13, n=203, seed=11):
    """The keys, maps and constants of the gate's edge tests; th separates the restated reductions with no key within 1e-9."""
    rng = np.random.default_rng(seed)
    cell = np.arange(rows * cols).reshape(rows, cols)
    entropy = 0.05 + 0.031 * cell + rng.uniform(0, 0.01, (rows, cols))                      # all distinct, r and c both visible
    confidence = 0.40 + 0.006 * cell[::-1, ::-1]
    classes = ((cell * 5) % 12).astype(np.uint8)                                            # 0 .. 11: static (<= 8) and dynamic
    assert len(np.unique(entropy)) == rows * cols
    pos, dep, xyz = [], [], []
    point = lambda: (rng.uniform(-10, 10), rng.uniform(-2, 2), rng.uniform(2, 50))
    xs, ys = edge_positions(cols), edge_positions(rows)
    for x in xs:                                                                              # the borders, crossed
        for y in ys:
            pos.append((x, y)); dep.append(1.0); xyz.append(point())
    for x in xs:
        pos.append((x, 3.5)); dep.append(2.0); xyz.append(point())
    for y in ys:
        pos.append((6.5, y)); dep.append(2.0); xyz.append(point())
    for k, d in enumerate(np.tile(DEPTHS, 3)):                                                # every kind of depth
        pos.append((1.5 + (4 * k) % 11, 0.5 + k % 7)); dep.append(d); xyz.append(point())
    for k, z in enumerate((0.0, -0.0, 0.0, -0.0)):                                            # Z = 0: the Jacobian is 0
        pos.append((2.5 + 3 * k, 1.5 + k)); dep.append(3.0); xyz.append((rng.uniform(-5, 5), rng.uniform(-1, 1), z))
    while len(pos) < n:
        pos.append((rng.uniform(0, cols), rng.uniform(0, rows))); dep.append(rng.uniform(-2, 40)); xyz.append(point())
    assert len(pos) == n and n % 64 != 0
    kps = np.zeros(n, KP_DTYPE)
    kps["x"] = [p[0] for p in pos]; kps["y"] = [p[1] for p in pos]
    kps["octave"] = np.arange(n) % 8
    sc = dict(kps=kps, depth=np.array(dep, np.float32), xyz=np.array(xyz, np.float64), entropy=entropy, confidence=confidence,
              classes=classes, Sx=covariance(rng), ls2=(np.float32(1.2) ** (2 * np.arange(8))).astype(np.float32), th_conf=0.6)
    sc["th"] = pick_threshold(sc)
    return sc


def pick_threshold(sc):
    """The middle of the widest gap in the central half of the restated reductions: about half of the keys pass, none is near."""
    _, red, _ = gate(sc["kps"], sc["depth"], sc["xyz"], sc["entropy"], sc["Sx"], FX, FY, BL, sc["ls2"], -1e9)
    r = np.sort(red[np.isfinite(red) & (red != 0.0)])
    mid = r[len(r) // 4: 3 * len(r) // 4 + 1]
    k = int(np.argmax(np.diff(mid)))
    th = float(0.5 * (mid[k] + mid[k + 1]))
    assert np.abs(red[np.isfinite(red)] - th).min() > 1e-9                                    # no key is excluded
    return th
