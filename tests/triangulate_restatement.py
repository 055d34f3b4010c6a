"""numpy restatement of sivo_amd/csrc/triangulate_math.hpp (the loop over the matches of LocalMapping::CreateNewMapPoints, reference
src/orbslam/LocalMapping.cc:277-470) — every float operation as a float32 numpy operation, every double one as float64, in the
header's order — plus a float64 evaluation of the same pipeline (numpy's SVD, np.cos(2 * np.arctan2(..))) with the margin of every
comparison it takes, and the scene generator of the triangulation tests.  No device, no library."""
import os
import re

import numpy as np

from sivo_amd.local_mapping import KEYFRAME_DTYPE, MATCH_DTYPE, keyframe

F, D = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATH_HPP = os.path.join(ROOT, "sivo_amd", "csrc", "triangulate_math.hpp")
(ACCEPTED, LOW_PARALLAX, W_ZERO, Z1, Z2, REPROJ1, REPROJ2, ZERO_DIST, SCALE, SEMANTICS) = range(10)
VOID = 255


def sweeps():
    """TR_SWEEPS as the source has it."""
    return int(re.search(r"constexpr int TR_SWEEPS = (\d+);", open(MATH_HPP).read()).group(1))


# ---------------------------------------------------------------------------------------------------------------------
# the gate (gate_math.hpp), vectorised over the points
# ---------------------------------------------------------------------------------------------------------------------
def _det_lu(a):
    """det_lu of gate_math.hpp on a (n, m, m) float64 stack (destroyed)."""
    n, m = a.shape[0], a.shape[1]
    ar = np.arange(n)
    sign = np.ones(n, D)
    zero = np.zeros(n, bool)
    diag = []
    for k in range(m):
        piv = np.full(n, k)
        best = np.abs(a[:, k, k])
        for i in range(k + 1, m):
            c = np.abs(a[:, i, k]) > best
            best = np.where(c, np.abs(a[:, i, k]), best)
            piv = np.where(c, i, piv)
        zero |= (best == 0.0) & ~zero
        rk, rp = a[ar, k].copy(), a[ar, piv].copy()
        a[ar, k], a[ar, piv] = rp, rk
        a[ar, k] = rp                      # (piv == k: the row stays)
        sign = np.where(piv != k, -sign, sign)
        diag.append(a[:, k, k].copy())
        for i in range(k + 1, m):
            f = a[:, i, k] / a[:, k, k]
            a[:, i, k + 1:] = a[:, i, k + 1:] - f[:, None] * a[:, k, k + 1:]
    d = diag
    prod = (d[0] * (d[1] * d[2])) * (d[3] * (d[4] * d[5])) if m == 6 else \
        ((d[0] * d[1]) * (d[2] * d[3])) * ((d[4] * d[5]) * (d[6] * (d[7] * d[8])))
    return np.where(zero, 0.0, sign * prod)


def mutual_information(Sx, fx, fy, bl, X, Y, Z, sigma2):
    """gate_mutual_information over n points; Sx (6, 6), fx / fy / bl scalars, X / Y / Z / sigma2 (n,) float64."""
    with np.errstate(all="ignore"):
        n = X.shape[0]
        Sx = np.asarray(Sx, D).reshape(6, 6)
        fx, fy, bl = D(fx), D(fy), D(bl)
        J = np.zeros((n, 3, 6), D)
        one = np.ones(n, D)
        rows = [[fx / Z, 0.0 * one, -fx * X / (Z * Z), -fx * X * Y / (Z * Z), fx * (1.0 + (X * X) / (Z * Z)), -fx * Y / Z],
                [0.0 * one, fy / Z, -fy * Y / (Z * Z), -fy * (1 + (Y * Y) / (Z * Z)), fy * X * Y / (Z * Z), fy * X / Z],
                [fx / Z, 0.0 * one, -fx * (X - bl) / (Z * Z), -fx * (X - bl) * Y / (Z * Z), fx * (1.0 + (X * (X - bl)) / (Z * Z)), -fx * Y / Z]]
        nz = Z != 0
        for a in range(3):
            for b in range(6):
                J[:, a, b] = np.where(nz, rows[a][b], 0.0)
        JS = np.zeros((n, 3, 6), D)
        for a in range(3):
            for b in range(6):
                s = np.zeros(n, D)
                for k in range(6):
                    s = s + J[:, a, k] * Sx[k, b]
                JS[:, a, b] = s
        Sz = np.zeros((n, 3, 3), D)
        for a in range(3):
            for b in range(3):
                s = np.zeros(n, D)
                for k in range(6):
                    s = s + JS[:, a, k] * J[:, b, k]
                Sz[:, a, b] = s + (sigma2 if a == b else 0.0)
        S9 = np.zeros((n, 9, 9), D)
        S9[:, :6, :6] = Sx
        for a in range(6):
            for b in range(3):
                s = np.zeros(n, D)
                for k in range(6):
                    s = s + Sx[a, k] * J[:, b, k]
                S9[:, a, 6 + b] = s
        S9[:, 6:, :6] = JS
        S9[:, 6:, 6:] = Sz
        state_det = _det_lu(np.broadcast_to(Sx, (n, 6, 6)).copy())
        z = lambda i: Sz[:, i // 3, i % 3]
        meas_det = z(0) * (z(4) * z(8) - z(5) * z(7)) - z(1) * (z(3) * z(8) - z(5) * z(6)) + z(2) * (z(3) * z(7) - z(4) * z(6))
        cov_det = _det_lu(S9)
        return 0.5 * np.log2(state_det * meas_det / cov_det)


# ---------------------------------------------------------------------------------------------------------------------
# triangulate_math.hpp
# ---------------------------------------------------------------------------------------------------------------------
def _gemm3(a0, a1, a2, b0, b1, b2, c):
    t = a0 * b0
    t = t + a1 * b1
    t = t + a2 * b2
    return (t.astype(D) * 1.0 + c).astype(F)


def _dot3(a, b):
    s = np.zeros(np.broadcast(a[0], b[0]).shape, D)
    for i in range(3):
        s = s + np.asarray(a[i], F).astype(D) * np.asarray(b[i], F).astype(D)
    return s


def _cos_stereo(mb, depth):
    a, d = (F(mb) / F(2)).astype(D), depth.astype(D)
    return ((d * d - a * a) / (d * d + a * a)).astype(F)


def _jacobi_rot(A, V, P, Q):
    apq = A[:, P, Q].copy()
    m = apq != 0.0
    theta = (A[:, Q, Q] - A[:, P, P]) / (2.0 * apq)
    t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
    t = np.where(theta < 0.0, -t, t)
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    B, W = A.copy(), V.copy()
    B[:, P, P] = A[:, P, P] - t * apq
    B[:, Q, Q] = A[:, Q, Q] + t * apq
    B[:, P, Q] = 0.0
    B[:, Q, P] = 0.0
    for r in range(4):
        if r in (P, Q):
            continue
        arp, arq = A[:, r, P], A[:, r, Q]
        B[:, r, P] = c * arp - s * arq
        B[:, P, r] = B[:, r, P]
        B[:, r, Q] = s * arp + c * arq
        B[:, Q, r] = B[:, r, Q]
    for r in range(4):
        vrp, vrq = V[:, r, P], V[:, r, Q]
        W[:, r, P] = c * vrp - s * vrq
        W[:, r, Q] = s * vrp + c * vrq
    A[m], V[m] = B[m], W[m]


def null_vector(Af, n_sweeps=None):
    """tr_null_vector: (n, 4, 4) float32 -> (n, 4) float32."""
    n_sweeps = sweeps() if n_sweeps is None else n_sweeps
    n = Af.shape[0]
    with np.errstate(all="ignore"):
        Ad = Af.astype(D)
        A = np.zeros((n, 4, 4), D)
        for i in range(4):
            for j in range(4):
                s = np.zeros(n, D)
                for k in range(4):
                    s = s + Ad[:, k, i] * Ad[:, k, j]
                A[:, i, j] = s
        V = np.broadcast_to(np.eye(4), (n, 4, 4)).copy()
        for _ in range(n_sweeps):
            for P, Q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
                _jacobi_rot(A, V, P, Q)
        best, idx = A[:, 0, 0].copy(), np.zeros(n, np.int64)
        for k in range(1, 4):
            m = A[:, k, k] < best
            best = np.where(m, A[:, k, k], best)
            idx = np.where(m, k, idx)
        return V[np.arange(n), :, idx].astype(F)


def _kf(k):
    k = np.asarray(k, KEYFRAME_DTYPE).reshape(())
    return {name: k[name] for name in KEYFRAME_DTYPE.names}


def _reproj_fails(k, wP, z, stereo, px, py, pr, sigma2, mbf):
    R, t = k["Rcw"], k["tcw"]
    x = (_dot3(R[0:3], wP) + D(t[0])).astype(F)
    y = (_dot3(R[3:6], wP) + D(t[1])).astype(F)
    invz = F(1.0) / z
    u = k["fx"] * x * invz + k["cx"]
    v = k["fy"] * y * invz + k["cy"]
    ex, ey = u - px, v - py
    mono = (ex * ex + ey * ey).astype(D) > 5.991 * sigma2.astype(D)
    ur = u - mbf * invz
    er = ur - pr
    ster = (ex * ex + ey * ey + er * er).astype(D) > 7.8 * sigma2.astype(D)
    return np.where(stereo, ster, mono)


def _unproject(k, u, v, z):
    x = (u - k["cx"]) * z * k["invfx"]
    y = (v - k["cy"]) * z * k["invfy"]
    T = k["Twc"]
    return [_gemm3(T[4 * i], T[4 * i + 1], T[4 * i + 2], x, y, z, D(T[4 * i + 3]) * 1.0) for i in range(3)]


def matrix_A(k1, k2, m):
    """The float A of :321-325 for every match, and the normalised coordinates."""
    k1, k2 = _kf(k1), _kf(k2)
    xn1 = [(m["x1"] - k1["cx"]) * k1["invfx"], (m["y1"] - k1["cy"]) * k1["invfy"]]
    xn2 = [(m["x2"] - k2["cx"]) * k2["invfx"], (m["y2"] - k2["cy"]) * k2["invfy"]]
    A = np.zeros((m.shape[0], 4, 4), F)
    for c in range(4):
        r1 = [k1["Rcw"][c], k1["Rcw"][3 + c], k1["Rcw"][6 + c]] if c < 3 else list(k1["tcw"])
        r2 = [k2["Rcw"][c], k2["Rcw"][3 + c], k2["Rcw"][6 + c]] if c < 3 else list(k2["tcw"])
        A[:, 0, c] = r1[2] * xn1[0] - r1[0]
        A[:, 1, c] = r1[2] * xn1[1] - r1[1]
        A[:, 2, c] = r2[2] * xn2[0] - r2[0]
        A[:, 3, c] = r2[2] * xn2[1] - r2[1]
    return A


def triangulate(p, n_sweeps=None, null=None):
    """tr_match over the matches of one problem (a dict as local_mapping.triangulate_batch takes it).  Returns status, wP (with every
    NaN stored as 0x7FC00000), detected_class and, for the tests, `mi`.  `null(A) -> (n, 4)` replaces tr_null_vector (the float32-SVD
    stand-in)."""
    k1, k2 = _kf(p["kf1"]), _kf(p["kf2"])
    m = np.ascontiguousarray(p["matches"], MATCH_DTYPE).reshape(-1)
    n = m.shape[0]
    with np.errstate(all="ignore"):
        stereo1, stereo2 = m["r1"] >= 0, m["r2"] >= 0
        one = np.ones(n, F)
        xn1 = [(m["x1"] - k1["cx"]) * k1["invfx"], (m["y1"] - k1["cy"]) * k1["invfy"], one]
        xn2 = [(m["x2"] - k2["cx"]) * k2["invfx"], (m["y2"] - k2["cy"]) * k2["invfy"], one]
        R1, R2 = k1["Rcw"], k2["Rcw"]
        ray1 = [_gemm3(R1[i], R1[3 + i], R1[6 + i], xn1[0], xn1[1], xn1[2], 0.0) for i in range(3)]
        ray2 = [_gemm3(R2[i], R2[3 + i], R2[6 + i], xn2[0], xn2[1], xn2[2], 0.0) for i in range(3)]
        cos_rays = (_dot3(ray1, ray2) / (np.sqrt(_dot3(ray1, ray1)) * np.sqrt(_dot3(ray2, ray2)))).astype(F)
        cs0 = cos_rays + F(1)
        cs1 = np.where(stereo1, _cos_stereo(k1["mb"], m["depth1"]), cs0)
        cs2 = np.where(~stereo1 & stereo2, _cos_stereo(k2["mb"], m["depth2"]), cs0)
        cs = np.where(cs2 < cs1, cs2, cs1)
        tri = (cos_rays < cs) & (cos_rays > 0) & (stereo1 | stereo2 | (cos_rays.astype(D) < 0.9998))
        un1 = ~tri & stereo1 & (cs1 < cs2)
        un2 = ~tri & ~un1 & stereo2 & (cs2 < cs1)
        status = np.full(n, -1, np.int64)
        status[~tri & ~un1 & ~un2] = LOW_PARALLAX
        e = null_vector(matrix_A(p["kf1"], p["kf2"], m), n_sweeps) if null is None else null(matrix_A(p["kf1"], p["kf2"], m))
        status[tri & (e[:, 3] == 0)] = W_ZERO
        inv = (1.0 / e[:, 3].astype(D)).astype(F)
        wt = [e[:, i] * inv for i in range(3)]
        w1 = _unproject(k1, m["x1"], m["y1"], m["depth1"])
        w2 = _unproject(k2, m["x2"], m["y2"], m["depth2"])
        wP = [np.where(tri, wt[i], np.where(un1, w1[i], w2[i])) for i in range(3)]
        live = status < 0

        def reject(cond, code):
            nonlocal live
            hit = live & cond
            status[hit] = code
            live = live & ~hit

        z1 = (_dot3(R1[6:9], wP) + D(k1["tcw"][2])).astype(F)
        reject(z1 <= 0, Z1)
        z2 = (_dot3(R2[6:9], wP) + D(k2["tcw"][2])).astype(F)
        reject(z2 <= 0, Z2)
        s1, s2 = k1["level_sigma2"][m["octave1"]], k2["level_sigma2"][m["octave2"]]
        reject(_reproj_fails(k1, wP, z1, stereo1, m["x1"], m["y1"], m["r1"], s1, k1["mbf"]), REPROJ1)
        reject(_reproj_fails(k2, wP, z2, stereo2, m["x2"], m["y2"], m["r2"], s2, k1["mbf"]), REPROJ2)
        n1 = [wP[i] - k1["Ow"][i] for i in range(3)]
        n2 = [wP[i] - k2["Ow"][i] for i in range(3)]
        dist1, dist2 = np.sqrt(_dot3(n1, n1)).astype(F), np.sqrt(_dot3(n2, n2)).astype(F)
        reject((dist1 == 0) | (dist2 == 0), ZERO_DIST)
        ratio_dist = dist2 / dist1
        ratio_octave = k1["scale_factors"][m["octave1"]] / k2["scale_factors"][m["octave2"]]
        rf = F(p["ratio_factor"])
        reject((ratio_dist * rf < ratio_octave) | (ratio_dist > ratio_octave * rf), SCALE)
        mi = mutual_information(p["state_cov"], k1["fx"], k1["fy"], k1["mb"], wP[0].astype(D), wP[1].astype(D), wP[2].astype(D), s1.astype(D))
        crit = (m["depth1"] > 0) & (m["class1"] <= 8) & (m["confidence1"] >= D(p["th_confidence"]))
        cls = np.where(crit & ~(mi - m["entropy1"] < D(p["th_entropy"])), m["class1"], VOID).astype(np.int64)
        ok = (cls == m["class2"]) & (cls != VOID)
        reached = live.copy()
        reject(~ok, SEMANTICS)
        status[live] = ACCEPTED
        out_w = np.stack(wP, axis=1).astype(F)
        out_w[(status == LOW_PARALLAX) | (status == W_ZERO)] = 0.0
        bits = out_w.view(np.uint32).copy()
        bits[np.isnan(out_w)] = 0x7FC00000
        return {"status": status.astype(np.uint8), "wP": bits.view(F), "detected_class": np.where(reached, cls, VOID).astype(np.uint8),
                "mi": mi, "reached": reached, "triangulated": tri & (e[:, 3] != 0)}


# ---------------------------------------------------------------------------------------------------------------------
# the same pipeline in float64 (the unpinned pieces as numpy has them), with the margin of every comparison
# ---------------------------------------------------------------------------------------------------------------------
def null_svd(A, dtype):
    """vt.row(3) of numpy's SVD of the float A, taken in `dtype`."""
    return np.linalg.svd(A.astype(dtype))[2][:, 3, :]


def pipeline64(p, svd_dtype=D):
    """status, wP (float64) and, per match, the smallest relative distance between a compared quantity and its threshold over the
    comparisons the match went through."""
    k1, k2 = _kf(p["kf1"]), _kf(p["kf2"])
    m = np.ascontiguousarray(p["matches"], MATCH_DTYPE).reshape(-1)
    n = m.shape[0]
    A = matrix_A(p["kf1"], p["kf2"], m)
    E = null_svd(A, svd_dtype).astype(D) if n else np.zeros((0, 4))
    mi_cache, pending = {}, []
    status, W, margin = np.zeros(n, np.uint8), np.zeros((n, 3)), np.full(n, np.inf)
    g = lambda k, name: np.asarray(k[name], D)
    R1, t1, R2, t2 = g(k1, "Rcw").reshape(3, 3), g(k1, "tcw"), g(k2, "Rcw").reshape(3, 3), g(k2, "tcw")
    for j in range(n):
        q = m[j]
        mg = []

        def cmp(a, b, scale=None):          # records how close a is to b
            s = max(abs(b), 1e-300) if scale is None else scale
            mg.append(abs(a - b) / s)

        def done(code, w=(0, 0, 0)):
            status[j], W[j], margin[j] = code, w, min(mg) if mg else np.inf

        st1, st2 = q["r1"] >= 0, q["r2"] >= 0
        xn1 = np.array([(D(q["x1"]) - g(k1, "cx")) * g(k1, "invfx"), (D(q["y1"]) - g(k1, "cy")) * g(k1, "invfy"), 1.0])
        xn2 = np.array([(D(q["x2"]) - g(k2, "cx")) * g(k2, "invfx"), (D(q["y2"]) - g(k2, "cy")) * g(k2, "invfy"), 1.0])
        ray1, ray2 = R1.T @ xn1, R2.T @ xn2
        cr = ray1 @ ray2 / (np.linalg.norm(ray1) * np.linalg.norm(ray2))
        cs1 = cs2 = cr + 1
        if st1:
            cs1 = np.cos(2 * np.arctan2(g(k1, "mb") / 2, D(q["depth1"])))
        elif st2:
            cs2 = np.cos(2 * np.arctan2(g(k2, "mb") / 2, D(q["depth2"])))
        cs = min(cs1, cs2)
        cmp(cr, cs); cmp(cr, 0.0, 1.0)
        if st1 or st2:
            cmp(cs1, cs2)
        else:
            cmp(cr, 0.9998)
        if cr < cs and cr > 0 and (st1 or st2 or cr < 0.9998):
            if E[j, 3] == 0:
                done(W_ZERO); continue
            w = E[j, :3] / E[j, 3]
        elif st1 and cs1 < cs2:
            z = D(q["depth1"])
            w = g(k1, "Twc").reshape(3, 4) @ np.array([(D(q["x1"]) - g(k1, "cx")) * z * g(k1, "invfx"), (D(q["y1"]) - g(k1, "cy")) * z * g(k1, "invfy"), z, 1.0])
        elif st2 and cs2 < cs1:
            z = D(q["depth2"])
            w = g(k2, "Twc").reshape(3, 4) @ np.array([(D(q["x2"]) - g(k2, "cx")) * z * g(k2, "invfx"), (D(q["y2"]) - g(k2, "cy")) * z * g(k2, "invfy"), z, 1.0])
        else:
            done(LOW_PARALLAX); continue
        size = max(np.linalg.norm(w), 1e-300)
        c1, c2 = R1 @ w + t1, R2 @ w + t2
        cmp(c1[2], 0.0, size)
        if not c1[2] > 0:
            done(Z1, w); continue
        cmp(c2[2], 0.0, size)
        if not c2[2] > 0:
            done(Z2, w); continue
        fail = None
        for code, k, c, st, px, py, pr, oc in ((REPROJ1, k1, c1, st1, q["x1"], q["y1"], q["r1"], q["octave1"]),
                                               (REPROJ2, k2, c2, st2, q["x2"], q["y2"], q["r2"], q["octave2"])):
            u, v = g(k, "fx") * c[0] / c[2] + g(k, "cx"), g(k, "fy") * c[1] / c[2] + g(k, "cy")
            e2 = (u - D(px)) ** 2 + (v - D(py)) ** 2
            th = 5.991
            if st:
                e2 += (u - g(k1, "mbf") / c[2] - D(pr)) ** 2
                th = 7.8
            th *= D(k["level_sigma2"][oc])
            cmp(e2, th)
            if e2 > th:
                fail = code
                break
        if fail is not None:
            done(fail, w); continue
        d1, d2 = np.linalg.norm(w - g(k1, "Ow")), np.linalg.norm(w - g(k2, "Ow"))
        if d1 == 0 or d2 == 0:
            done(ZERO_DIST, w); continue
        rd, ro, rf = d2 / d1, D(k1["scale_factors"][q["octave1"]]) / D(k2["scale_factors"][q["octave2"]]), D(F(p["ratio_factor"]))
        cmp(rd * rf, ro); cmp(rd, ro * rf)
        if rd * rf < ro or rd > ro * rf:
            done(SCALE, w); continue
        pending.append((j, w, mg))
    if pending:                              # the gate of every match that reached it, in one vectorised evaluation
        ws = np.array([w for _, w, _ in pending])
        js = np.array([j for j, _, _ in pending])
        mis = mutual_information(p["state_cov"], k1["fx"], k1["fy"], k1["mb"], ws[:, 0].copy(), ws[:, 1].copy(), ws[:, 2].copy(),
                                 k1["level_sigma2"][m["octave1"][js]].astype(D))
        thc, the = D(p["th_confidence"]), D(p["th_entropy"])
        for (j, w, mg), mi in zip(pending, mis):
            q = m[j]
            cls = VOID
            mg.append(abs(q["confidence1"] - thc))
            if q["depth1"] > 0 and q["class1"] <= 8 and q["confidence1"] >= thc:
                mi_cache[j] = mi
                mg.append(abs(mi - q["entropy1"] - the) / max(1.0, abs(the)))
                cls = VOID if mi - q["entropy1"] < the else int(q["class1"])
            status[j], W[j], margin[j] = (ACCEPTED if cls == q["class2"] and cls != VOID else SEMANTICS), w, min(mg)
    return {"status": status, "wP": W, "margin": margin, "mi": mi_cache}


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
def _rot(axis, angle):
    axis = np.asarray(axis, D) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def make_keyframes(rng, nlevels=8, mbf2=None, intr=(718.856, 718.856, 607.1928, 185.2157), mbf=386.1448, degenerate_pair=False):
    """Two keyframes about 1.5 m apart.  degenerate_pair: keyframe 1 at R = I, t = (0, -1, 0), keyframe 2 yawed 5 degrees at
    t = (0, 1, 0) — a pose pair for which a match with y1 = cy1, y2 = cy2 has an A whose A'A is block diagonal in exact arithmetic
    AND in floats: the null vector has w == 0 exactly."""
    fx, fy, cx, cy = intr
    sf = F(1.2) ** np.arange(nlevels, dtype=F)
    s2 = sf * sf
    if degenerate_pair:
        c, s = np.cos(np.radians(5.0)), np.sin(np.radians(5.0))
        R1, t1 = np.eye(3), np.array([0.0, -1.0, 0.0])
        R2, t2 = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]]), np.array([0.0, 1.0, 0.0])
    else:
        R1 = _rot(rng.normal(size=3), rng.uniform(0, 0.05))
        t1 = rng.normal(size=3) * 0.1
        R2 = _rot(rng.normal(size=3), rng.uniform(0, 0.08)) @ R1
        t2 = R2 @ (-(-R1.T @ t1 + np.array([rng.uniform(0.8, 1.6), rng.uniform(-0.1, 0.1), rng.uniform(-0.6, 0.6)])))
    k1 = keyframe(R1, t1, fx, fy, cx, cy, mbf / fx, mbf, sf, s2)
    b2 = mbf if mbf2 is None else mbf2
    k2 = keyframe(R2, t2, fx * 1.01, fy * 0.99, cx + 3, cy - 2, b2 / (fx * 1.01), b2, sf, s2)
    return k1, k2


def draw_matches(rng, k1, k2, n, stereo=(0.5, 0.5), outliers=0.2, noise=0.6, octave=None):
    """n candidate matches: points in front of keyframe 1 projected into both keyframes with pixel noise, a share of outliers (a
    random pixel in keyframe 2, a wrong octave, a wrong depth), stereo measurements with the given probabilities, and the semantic
    values of both keypoints."""
    a1, a2 = _kf(k1), _kf(k2)
    nl = int(a1["nlevels"])
    m = np.zeros(n, MATCH_DTYPE)
    R1, t1 = a1["Rcw"].astype(D).reshape(3, 3), a1["tcw"].astype(D)
    R2, t2 = a2["Rcw"].astype(D).reshape(3, 3), a2["tcw"].astype(D)
    Xc = np.stack([rng.uniform(-12, 12, n), rng.uniform(-3, 3, n), rng.uniform(3, 45, n)], axis=1)
    Xw = (Xc - t1) @ R1            # R1' (Xc - t1)
    X2 = Xw @ R2.T + t2
    X2[:, 2] = np.where(np.abs(X2[:, 2]) < 0.5, 0.5, X2[:, 2])
    o1 = rng.integers(0, nl, n) if octave is None else np.full(n, octave)
    d1, d2 = np.linalg.norm(Xc, axis=1), np.linalg.norm(X2, axis=1)
    o2 = np.clip(o1 - np.round(np.log(d2 / d1) / np.log(1.2)).astype(int), 0, nl - 1) if octave is None else o1
    px = lambda k, X: (D(k["fx"]) * X[:, 0] / X[:, 2] + D(k["cx"]), D(k["fy"]) * X[:, 1] / X[:, 2] + D(k["cy"]))
    u1, v1 = px(a1, Xc)
    u2, v2 = px(a2, X2)
    sg1, sg2 = noise * a1["scale_factors"][o1].astype(D), noise * a2["scale_factors"][o2].astype(D)
    u1, v1 = u1 + rng.normal(size=n) * sg1, v1 + rng.normal(size=n) * sg1
    u2, v2 = u2 + rng.normal(size=n) * sg2, v2 + rng.normal(size=n) * sg2
    kind = rng.random(n)
    bad = kind < outliers
    far = bad & (kind < outliers / 2)
    u2 = np.where(far, rng.uniform(0, 1241, n), u2)
    v2 = np.where(far, rng.uniform(0, 376, n), v2)
    wrong = rng.integers(0, nl, n)
    if octave is None:                 # (a fixed octave holds for the outliers too)
        o2 = np.where(bad & ~far & (kind < 0.75 * outliers), wrong, o2)
    st1, st2 = rng.random(n) < stereo[0], rng.random(n) < stereo[1]
    z1 = Xc[:, 2] * np.where(bad & ~far & (kind >= 0.75 * outliers), rng.uniform(0.3, 3, n), 1 + 0.01 * rng.normal(size=n))
    z2 = np.abs(X2[:, 2]) * (1 + 0.01 * rng.normal(size=n))
    m["x1"], m["y1"], m["octave1"], m["x2"], m["y2"], m["octave2"] = u1, v1, o1, u2, v2, o2
    m["depth1"] = np.where(st1, z1, -1)
    m["depth2"] = np.where(st2, z2, -1)
    m["r1"] = np.where(st1, m["x1"] - a1["mbf"] / m["depth1"], -1)
    m["r2"] = np.where(st2, m["x2"] - a1["mbf"] / m["depth2"], -1)      # (consistent with the :414 quirk: keyframe 1's mbf)
    m["r1"] = np.where(st1 & (m["r1"] < 0), 0, m["r1"])
    m["r2"] = np.where(st2 & (m["r2"] < 0), 0, m["r2"])
    m["class1"] = np.where(rng.random(n) < 0.9, rng.integers(0, 9, n), rng.integers(9, 12, n))
    m["class2"] = np.where(rng.random(n) < 0.85, m["class1"], rng.integers(0, 12, n))
    m["confidence1"] = rng.uniform(0.5, 1.0, n)
    m["entropy1"] = rng.uniform(0.0, 1.0, n)
    return m


def make_problem(seed, n, min_margin=1e-3, extra=None, **kw):
    """One problem of n matches, none within a relative `min_margin` of a threshold of the float64 pipeline: candidates are drawn in
    bulk and those too close are replaced by the next ones (min_margin = 0: no such check).  `extra`: hand-made matches put in front
    (not checked).  The gate's threshold is the median MI of the candidates less 0.8, so that the entropy decides."""
    rng = np.random.default_rng(seed)
    kkw = {k: kw.pop(k) for k in ("nlevels", "mbf2", "degenerate_pair", "intr", "mbf") if k in kw}
    k1, k2 = make_keyframes(rng, **kkw)
    cov = rng.normal(size=(6, 6)) * 0.1
    p = {"kf1": k1, "kf2": k2, "ratio_factor": F(1.5) * F(1.2), "state_cov": 1e-4 * (np.eye(6) + cov @ cov.T),
         "th_confidence": 0.6, "th_entropy": 0.0}
    extra = np.zeros(0, MATCH_DTYPE) if extra is None else extra
    want = max(n - extra.shape[0], 0)
    cand = draw_matches(rng, k1, k2, (8 * want + 64) if min_margin else want, **kw)
    p["matches"] = cand
    r = triangulate(p)
    mis = r["mi"][r["reached"] & np.isfinite(r["mi"])]
    p["th_entropy"] = float(np.median(mis)) - 0.8 if mis.size else 0.0
    keep = cand
    if min_margin:
        keep = cand[pipeline64(p)["margin"] >= min_margin][:want]
        assert keep.shape[0] == want, "not enough candidates"
    p["matches"] = np.concatenate([extra, keep])
    return p


def special_matches(k1, k2):
    """Three hand-made matches: [0] no stereo, both keypoints at the principal point (with make_keyframes(..., degenerate_pair=True):
    w == 0 exactly), [1] no stereo, identical rays (keyframe 2's keypoint is where keyframe 1's ray at infinity lands), [2] stereo in
    keyframe 1 at depth 1, far to the left and nearly parallel rays (with the degenerate pair, whose keyframe 2 is yawed: the
    unprojected point is in front of keyframe 1 and behind keyframe 2)."""
    a1, a2 = _kf(k1), _kf(k2)
    m = np.zeros(3, MATCH_DTYPE)
    m["r1"], m["r2"], m["depth1"], m["depth2"] = -1, -1, -1, -1
    m["confidence1"], m["class1"], m["class2"] = 0.9, 2, 2
    m["x1"][0], m["y1"][0], m["x2"][0], m["y2"][0] = a1["cx"], a1["cy"], a2["cx"], a2["cy"]
    x1, y1 = F(400.0), F(150.0)
    ray = a1["Rcw"].astype(D).reshape(3, 3).T @ np.array([(x1 - a1["cx"]) / a1["fx"], (y1 - a1["cy"]) / a1["fy"], 1.0], D)
    c2 = a2["Rcw"].astype(D).reshape(3, 3) @ ray
    m["x1"][1], m["y1"][1] = x1, y1
    m["x2"][1], m["y2"][1] = a2["fx"] * c2[0] / c2[2] + a2["cx"], a2["fy"] * c2[1] / c2[2] + a2["cy"]
    m["x1"][2], m["y1"][2], m["depth1"][2], m["r1"][2] = a1["cx"] - F(13) * a1["fx"], a1["cy"], 1, 0
    m["x2"][2], m["y2"][2] = a2["cx"] - F(100) * a2["fx"], a2["cy"]
    return m


def all_status_problem(seed=11, n=400):
    """A problem in which every status value occurs.  The pose pair is the degenerate one (the w == 0 match in front); `zero distance`
    cannot be reached with a camera centre that belongs to the pose (the point would have z2 = 0 and leave at the depth test), so
    keyframe 2's Ow is set to the triangulated point of the first accepted match: the kernel takes Ow as an input of its own."""
    rng = np.random.default_rng(seed)
    k1, k2 = make_keyframes(rng, degenerate_pair=True)
    p = make_problem(seed, n, min_margin=0, degenerate_pair=True, extra=special_matches(k1, k2), stereo=(0.4, 0.4))
    r = triangulate(p)
    j = int(np.flatnonzero(r["status"] == ACCEPTED)[0])
    k2 = np.array(p["kf2"])
    k2["Ow"] = r["wP"][j]
    p["kf2"] = k2
    return p
