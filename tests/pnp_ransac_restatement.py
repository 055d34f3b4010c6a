"""numpy restatement of sivo_amd/csrc/pnp_ransac.hip (the arithmetic is sivo_amd/csrc/pnp_epnp.hpp): EPnP as the reference's
PnPsolver.cc states it, in double, operation for operation and in the kernel's order, vectorised over the hypotheses (H of them
at once, each on its own n correspondences); CheckInliers with the source's float / double mixture; the scan for the records and
the refinements as the ABI does them.  Beside it: `Sequential`, a direct transcription of iterate / find / Refine
(PnPsolver.cc:175-315) driven by callbacks, `ransac_iterations` (SetRansacParameters, :131-173), the gather of the constructor
(:72-121), and a scene generator.  Every elementwise numpy operation on float64 / float32 arrays is one correctly rounded IEEE
operation, which is what the kernel's + - * / sqrt are."""
import math

import numpy as np

SWEEPS3, SWEEPS12, SWEEPS_SVD = 4, 8, 3      # == PNP_SWEEPS3 / PNP_SWEEPS12 / PNP_SWEEPS_SVD (read from the source by the tests)
QNAN32 = np.uint32(0x7FC00000)

PNP_POINT_DTYPE = np.dtype([("xw", np.float32, 3), ("u", np.float32), ("v", np.float32), ("max_err", np.float32)])


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def _jacobi(A, V, sweeps):
    """pnp_jacobi: A (H, m, m) symmetric, V (H, m, m); in place."""
    m = A.shape[1]
    for _ in range(sweeps):
        for p in range(m - 1):
            for q in range(p + 1, m):
                apq, app, aqq = A[:, p, q].copy(), A[:, p, p].copy(), A[:, q, q].copy()
                on = apq != 0.0
                theta = (aqq - app) / (2.0 * apq)
                t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                t = np.where(theta < 0.0, -t, t)
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                arp, arq = A[:, :, p].copy(), A[:, :, q].copy()
                np_ = c[:, None] * arp - s[:, None] * arq
                nq_ = s[:, None] * arp + c[:, None] * arq
                nA = A.copy()
                nA[:, :, p] = np_; nA[:, p, :] = np_
                nA[:, :, q] = nq_; nA[:, q, :] = nq_
                nA[:, p, p] = app - t * apq
                nA[:, q, q] = aqq + t * apq
                nA[:, p, q] = 0.0; nA[:, q, p] = 0.0
                vrp, vrq = V[:, :, p].copy(), V[:, :, q].copy()
                nV = V.copy()
                nV[:, :, p] = c[:, None] * vrp - s[:, None] * vrq
                nV[:, :, q] = s[:, None] * vrp + c[:, None] * vrq
                A[on] = nA[on]
                V[on] = nV[on]


def _order(d):
    """pnp_order: d (H, m) -> ord (H, m): the k-th largest |d|, ties and everything that does not compare to the lower index."""
    H, m = d.shape
    a = np.abs(d)
    used = np.zeros((H, m), bool)
    ord_ = np.zeros((H, m), np.int64)
    rows = np.arange(H)
    for k in range(m):
        best = np.full(H, -1)
        for j in range(m):
            take = ~used[:, j] & ((best < 0) | (a[:, j] > a[rows, np.maximum(best, 0)]))
            best = np.where(take, j, best)
        ord_[:, k] = best
        used[rows, best] = True
    return ord_


def _qr_solve(A, b):
    """pnp_qr_solve: A (H, nr, nc), b (H, nr) -> X (H, nc); NaN where the reference returns early."""
    A, b = A.copy(), b.copy()
    H, nr, nc = A.shape
    A1, A2 = np.zeros((H, nc)), np.zeros((H, nc))
    dead = np.zeros(H, bool)
    for k in range(nc):
        eta = np.abs(A[:, k, k])
        for i in range(k + 1, nr):
            elt = np.abs(A[:, i - 1, k])
            eta = np.where(eta < elt, elt, eta)
        dead |= eta == 0
        inv_eta = 1.0 / eta
        s = np.zeros(H)
        for i in range(k, nr):
            A[:, i, k] = A[:, i, k] * inv_eta
            s = s + A[:, i, k] * A[:, i, k]
        sigma = np.sqrt(s)
        sigma = np.where(A[:, k, k] < 0, -sigma, sigma)
        A[:, k, k] = A[:, k, k] + sigma
        A1[:, k] = sigma * A[:, k, k]
        A2[:, k] = -eta * sigma
        for j in range(k + 1, nc):
            s = np.zeros(H)
            for i in range(k, nr):
                s = s + A[:, i, k] * A[:, i, j]
            tau = s / A1[:, k]
            for i in range(k, nr):
                A[:, i, j] = A[:, i, j] - tau * A[:, i, k]
    for j in range(nc):
        tau = np.zeros(H)
        for i in range(j, nr):
            tau = tau + A[:, i, j] * b[:, i]
        tau = tau / A1[:, j]
        for i in range(j, nr):
            b[:, i] = b[:, i] - tau * A[:, i, j]
    X = np.zeros((H, nc))
    X[:, nc - 1] = b[:, nc - 1] / A2[:, nc - 1]
    for i in range(nc - 2, -1, -1):
        s = np.zeros(H)
        for j in range(i + 1, nc):
            s = s + A[:, i, j] * X[:, j]
        X[:, i] = (b[:, i] - s) / A2[:, i]
    X[dead] = np.nan
    return X


def _find_betas(L, rho, kind):
    cols = {1: [0, 1, 3, 6], 2: [0, 1, 2], 3: [0, 1, 2, 3, 4]}[kind]
    b = _qr_solve(L[:, :, cols], rho)
    H = L.shape[0]
    be = np.zeros((H, 4))
    neg = b[:, 0] < 0
    be[:, 0] = np.sqrt(np.where(neg, -b[:, 0], b[:, 0]))
    if kind == 1:
        for i in (1, 2, 3):
            be[:, i] = np.where(neg, -b[:, i], b[:, i]) / be[:, 0]
        return be
    be[:, 1] = np.where(neg, np.where(b[:, 2] < 0, np.sqrt(-b[:, 2]), 0.0), np.where(b[:, 2] > 0, np.sqrt(b[:, 2]), 0.0))
    be[:, 0] = np.where(b[:, 1] < 0, -be[:, 0], be[:, 0])
    if kind == 3:
        be[:, 2] = b[:, 3] / be[:, 0]
    return be


def _gauss_newton(L, rho, be):
    be = be.copy()
    H = L.shape[0]
    for _ in range(5):
        A = np.zeros((H, 6, 4))
        b0, b1, b2, b3 = be[:, 0:1], be[:, 1:2], be[:, 2:3], be[:, 3:4]
        l = [L[:, :, i] for i in range(10)]
        A[:, :, 0] = 2 * l[0] * b0 + l[1] * b1 + l[3] * b2 + l[6] * b3
        A[:, :, 1] = l[1] * b0 + 2 * l[2] * b1 + l[4] * b2 + l[7] * b3
        A[:, :, 2] = l[3] * b0 + l[4] * b1 + 2 * l[5] * b2 + l[8] * b3
        A[:, :, 3] = l[6] * b0 + l[7] * b1 + l[8] * b2 + 2 * l[9] * b3
        b = rho - (l[0] * b0 * b0 + l[1] * b0 * b1 + l[2] * b1 * b1 + l[3] * b0 * b2 + l[4] * b1 * b2 + l[5] * b2 * b2 +
                   l[6] * b0 * b3 + l[7] * b1 * b3 + l[8] * b2 * b3 + l[9] * b3 * b3)
        be = be + _qr_solve(A, b)
    return be


def _dot3(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _rotation(abt, pc0, pw0, sweeps):
    """pnp_rotation: abt (H, 3, 3) -> R (H, 3, 3), t (H, 3)."""
    G = abt.copy()
    H = G.shape[0]
    W = np.tile(np.eye(3), (H, 1, 1))
    for _ in range(sweeps):
        for p in range(2):
            for q in range(p + 1, 3):
                alpha = G[:, 0, p] * G[:, 0, p] + G[:, 1, p] * G[:, 1, p] + G[:, 2, p] * G[:, 2, p]
                beta = G[:, 0, q] * G[:, 0, q] + G[:, 1, q] * G[:, 1, q] + G[:, 2, q] * G[:, 2, q]
                gamma = G[:, 0, p] * G[:, 0, q] + G[:, 1, p] * G[:, 1, q] + G[:, 2, p] * G[:, 2, q]
                on = gamma != 0.0
                zeta = (beta - alpha) / (2.0 * gamma)
                tt = 1.0 / (np.abs(zeta) + np.sqrt(zeta * zeta + 1.0))
                tt = np.where(zeta < 0.0, -tt, tt)
                c = (1.0 / np.sqrt(tt * tt + 1.0))[:, None]
                s = tt[:, None] * c
                for Mx in (G, W):
                    mp, mq = Mx[:, :, p].copy(), Mx[:, :, q].copy()
                    Mx[:, :, p] = np.where(on[:, None], c * mp - s * mq, mp)
                    Mx[:, :, q] = np.where(on[:, None], s * mp + c * mq, mq)
    for k in range(3):
        sigma = np.sqrt(G[:, 0, k] * G[:, 0, k] + G[:, 1, k] * G[:, 1, k] + G[:, 2, k] * G[:, 2, k])
        G[:, :, k] = G[:, :, k] / sigma[:, None]
    R = np.zeros((H, 3, 3))
    for i in range(3):
        for j in range(3):
            R[:, i, j] = _dot3(G[:, i, :], W[:, j, :])
    r = R.reshape(H, 9)
    det = (r[:, 0] * r[:, 4] * r[:, 8] + r[:, 1] * r[:, 5] * r[:, 6] + r[:, 2] * r[:, 3] * r[:, 7] - r[:, 2] * r[:, 4] * r[:, 6] -
           r[:, 1] * r[:, 3] * r[:, 8] - r[:, 0] * r[:, 5] * r[:, 7])
    R[:, 2, :] = np.where((det < 0)[:, None], -R[:, 2, :], R[:, 2, :])
    t = np.stack([pc0[:, i] - _dot3(R[:, i, :], pw0) for i in range(3)], axis=1)
    return R, t


def epnp(P, K, sweeps12=None, sweeps3=None, sweeps_svd=None):
    """pnp_epnp: P (H, n, 5) float64 = X Y Z u v of each hypothesis' correspondences (widened floats), K = fu fv uc vc (float64)
    -> R (H, 3, 3), t (H, 3) float64."""
    sweeps12 = SWEEPS12 if sweeps12 is None else sweeps12
    sweeps3 = SWEEPS3 if sweeps3 is None else sweeps3
    sweeps_svd = SWEEPS_SVD if sweeps_svd is None else sweeps_svd
    with np.errstate(all="ignore"):
        H, n = P.shape[:2]
        fu, fv, uc, vc = (np.float64(v) for v in K)
        pw, us = P[:, :, :3], P[:, :, 3:]
        nd = np.float64(n)
        # choose_control_points
        c0 = np.zeros((H, 3))
        for i in range(n):
            c0 = c0 + pw[:, i]
        c0 = c0 / nd
        S = np.zeros((H, 3, 3))
        for i in range(n):
            d = pw[:, i] - c0
            S = S + d[:, :, None] * d[:, None, :]
        V3 = np.tile(np.eye(3), (H, 1, 1))
        _jacobi(S, V3, sweeps3)
        dg = np.stack([S[:, i, i] for i in range(3)], axis=1)
        o3 = _order(dg)
        rows = np.arange(H)
        cws = np.zeros((H, 4, 3))
        cws[:, 0] = c0
        for i in range(1, 4):
            o = o3[:, i - 1]
            k = np.sqrt(dg[rows, o] / nd)
            cws[:, i] = c0 + k[:, None] * V3[rows, :, o]
        # compute_barycentric_coordinates
        cc = np.zeros((H, 9))
        for i in range(3):
            for j in range(1, 4):
                cc[:, 3 * i + j - 1] = cws[:, j, i] - cws[:, 0, i]
        c = [cc[:, i] for i in range(9)]
        c00, c01, c02 = c[4] * c[8] - c[5] * c[7], c[5] * c[6] - c[3] * c[8], c[3] * c[7] - c[4] * c[6]
        det = c[0] * c00 + c[1] * c01 + c[2] * c02
        ci = [c00 / det, (c[2] * c[7] - c[1] * c[8]) / det, (c[1] * c[5] - c[2] * c[4]) / det,
              c01 / det, (c[0] * c[8] - c[2] * c[6]) / det, (c[2] * c[3] - c[0] * c[5]) / det,
              c02 / det, (c[1] * c[6] - c[0] * c[7]) / det, (c[0] * c[4] - c[1] * c[3]) / det]
        rho = np.zeros((H, 6))
        r = 0
        for a in range(3):
            for b in range(a + 1, 4):
                p1, p2 = cws[:, a], cws[:, b]
                rho[:, r] = ((p1[:, 0] - p2[:, 0]) * (p1[:, 0] - p2[:, 0]) + (p1[:, 1] - p2[:, 1]) * (p1[:, 1] - p2[:, 1]) +
                             (p1[:, 2] - p2[:, 2]) * (p1[:, 2] - p2[:, 2]))
                r += 1
        # alphas of every point
        al = np.zeros((H, n, 4))
        d0, d1, d2 = pw[:, :, 0] - c0[:, 0:1], pw[:, :, 1] - c0[:, 1:2], pw[:, :, 2] - c0[:, 2:3]
        for j in range(3):
            al[:, :, 1 + j] = ci[3 * j][:, None] * d0 + ci[3 * j + 1][:, None] * d1 + ci[3 * j + 2][:, None] * d2
        al[:, :, 0] = 1.0 - al[:, :, 1] - al[:, :, 2] - al[:, :, 3]
        # fill_M and M'M: the rows in order
        du, dv = uc - us[:, :, 0], vc - us[:, :, 1]
        A = np.zeros((H, 12, 12))
        for i in range(n):
            M1, M2 = np.zeros((H, 12)), np.zeros((H, 12))
            for j in range(4):
                M1[:, 3 * j] = al[:, i, j] * fu
                M1[:, 3 * j + 2] = al[:, i, j] * du[:, i]
                M2[:, 3 * j + 1] = al[:, i, j] * fv
                M2[:, 3 * j + 2] = al[:, i, j] * dv[:, i]
            A = A + M1[:, :, None] * M1[:, None, :]
            A = A + M2[:, :, None] * M2[:, None, :]
        V = np.tile(np.eye(12), (H, 1, 1))
        _jacobi(A, V, sweeps12)
        o12 = _order(np.stack([A[:, i, i] for i in range(12)], axis=1))
        nv = np.stack([V[rows, :, o12[:, 11 - i]] for i in range(4)], axis=1)          # (H, 4, 12)
        # compute_L_6x10
        L = np.zeros((H, 6, 10))
        a, b = 0, 1
        for j in range(6):
            dvv = [nv[:, i, 3 * a:3 * a + 3] - nv[:, i, 3 * b:3 * b + 3] for i in range(4)]
            L[:, j, 0] = _dot3(dvv[0], dvv[0])
            L[:, j, 1] = 2.0 * _dot3(dvv[0], dvv[1])
            L[:, j, 2] = _dot3(dvv[1], dvv[1])
            L[:, j, 3] = 2.0 * _dot3(dvv[0], dvv[2])
            L[:, j, 4] = 2.0 * _dot3(dvv[1], dvv[2])
            L[:, j, 5] = _dot3(dvv[2], dvv[2])
            L[:, j, 6] = 2.0 * _dot3(dvv[0], dvv[3])
            L[:, j, 7] = 2.0 * _dot3(dvv[1], dvv[3])
            L[:, j, 8] = 2.0 * _dot3(dvv[2], dvv[3])
            L[:, j, 9] = _dot3(dvv[3], dvv[3])
            b += 1
            if b > 3:
                a += 1
                b = a + 1
        Rs, ts, errs = [], [], []
        for kind in (1, 2, 3):
            be = _gauss_newton(L, rho, _find_betas(L, rho, kind))
            ccs = np.zeros((H, 4, 3))
            for j in range(4):
                for k in range(3):
                    s = np.zeros(H)
                    for i in range(4):
                        s = s + be[:, i] * nv[:, i, 3 * j + k]
                    ccs[:, j, k] = s

            def pcs_of(ccs):
                return (al[:, :, 0:1] * ccs[:, None, 0, :] + al[:, :, 1:2] * ccs[:, None, 1, :] + al[:, :, 2:3] * ccs[:, None, 2, :] +
                        al[:, :, 3:4] * ccs[:, None, 3, :])
            flip = pcs_of(ccs)[:, 0, 2] < 0.0
            ccs = np.where(flip[:, None, None], -ccs, ccs)
            pcs = pcs_of(ccs)
            pc0, pw0 = np.zeros((H, 3)), np.zeros((H, 3))
            for i in range(n):
                pc0 = pc0 + pcs[:, i]
                pw0 = pw0 + pw[:, i]
            pc0, pw0 = pc0 / nd, pw0 / nd
            abt = np.zeros((H, 3, 3))
            for i in range(n):
                abt = abt + (pcs[:, i] - pc0)[:, :, None] * (pw[:, i] - pw0)[:, None, :]
            R, t = _rotation(abt, pc0, pw0, sweeps_svd)
            sum2 = np.zeros(H)
            for i in range(n):
                Xc = _dot3(R[:, 0], pw[:, i]) + t[:, 0]
                Yc = _dot3(R[:, 1], pw[:, i]) + t[:, 1]
                inv_Zc = 1.0 / (_dot3(R[:, 2], pw[:, i]) + t[:, 2])
                ue = uc + fu * Xc * inv_Zc
                ve = vc + fv * Yc * inv_Zc
                u, v = us[:, i, 0], us[:, i, 1]
                sum2 = sum2 + np.sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve))
            Rs.append(R); ts.append(t); errs.append(sum2 / nd)
        N = np.zeros(H, np.int64)
        N = np.where(errs[1] < errs[0], 1, N)
        eN = np.where(N == 1, errs[1], errs[0])
        N = np.where(errs[2] < eN, 2, N)
        Rs, ts = np.stack(Rs, axis=1), np.stack(ts, axis=1)
        return Rs[rows, N], ts[rows, N]


def check_inliers(R, t, K, pts):
    """CheckInliers for H poses over all points: -> (H, n) bool."""
    with np.errstate(all="ignore"):
        f32, f64 = np.float32, np.float64
        fu, fv, uc, vc = (np.float64(v) for v in K)
        X, Y, Z = (pts["xw"][:, i].astype(f64)[None, :] for i in range(3))
        r = R.reshape(-1, 9)
        Xc = (r[:, 0:1] * X + r[:, 1:2] * Y + r[:, 2:3] * Z + t[:, 0:1]).astype(f32)
        Yc = (r[:, 3:4] * X + r[:, 4:5] * Y + r[:, 5:6] * Z + t[:, 1:2]).astype(f32)
        invZc = (1 / (r[:, 6:7] * X + r[:, 7:8] * Y + r[:, 8:9] * Z + t[:, 2:3])).astype(f32)
        ue = uc + fu * Xc.astype(f64) * invZc.astype(f64)
        ve = vc + fv * Yc.astype(f64) * invZc.astype(f64)
        distX = (pts["u"].astype(f64)[None, :] - ue).astype(f32)
        distY = (pts["v"].astype(f64)[None, :] - ve).astype(f32)
        error2 = distX * distX + distY * distY
        return error2 < pts["max_err"][None, :]


def pack_bits(inl):
    """(H, n) bool -> (H, ceil(n / 64)) uint64"""
    H, n = inl.shape
    words = (n + 63) // 64
    b = np.zeros((H, words * 64), np.uint8)
    b[:, :n] = inl
    return np.packbits(b, axis=1, bitorder="little").view("<u8").reshape(H, words)


def store_T(R, t):
    """[R | t] as 12 floats, every NaN the quiet NaN 0x7FC00000"""
    with np.errstate(all="ignore"):
        T = np.concatenate([R.reshape(-1, 9), t.reshape(-1, 3)], axis=1).astype(np.float32)
    w = T.view(np.uint32).copy()
    w[np.isnan(T)] = QNAN32
    return w.view(np.float32)


def _points64(pts, idx):
    p = pts[idx]
    return np.concatenate([p["xw"].astype(np.float64), p["u"].astype(np.float64)[..., None], p["v"].astype(np.float64)[..., None]], axis=-1)


def evaluate(pts, K, sets, **kw):
    """EPnP on each index set of `sets` ((H, m) array), CheckInliers over all points -> count, T, inlier_bits."""
    pts = np.ascontiguousarray(pts, PNP_POINT_DTYPE).reshape(-1)
    sets = np.asarray(sets, np.int64).reshape(len(sets), -1)
    Kd = np.asarray(K, np.float32).astype(np.float64)
    words = (pts.shape[0] + 63) // 64
    if sets.shape[0] == 0:
        return np.zeros(0, np.int32), np.zeros((0, 12), np.float32), np.zeros((0, words), np.uint64)
    R, t = epnp(_points64(pts, sets), Kd, **kw)
    inl = check_inliers(R, t, Kd, pts)
    return inl.sum(axis=1).astype(np.int32), store_T(R, t), pack_bits(inl)


def pnp_ransac(pts, K, samples, min_inliers, best_in=0, **kw):
    """sivo_pnp_ransac: the hypotheses, the scan for the records, the refinements."""
    pts = np.ascontiguousarray(pts, PNP_POINT_DTYPE).reshape(-1)
    samples = np.asarray(samples, np.int32).reshape(-1, 4)
    count, T, bits = evaluate(pts, K, samples, **kw)
    nh, n = samples.shape[0], pts.shape[0]
    out = {"count": count, "T": T, "inlier_bits": bits, "refined": np.full(nh, -1, np.int32), "refined_T": np.zeros((nh, 12), np.float32),
           "refined_bits": np.zeros_like(bits), "n_records": 0}
    best = best_in
    for h in range(nh):
        if count[h] >= min_inliers and count[h] > best:
            best = int(count[h])
            idx = np.flatnonzero(unpack_bits(bits[h], n))
            c, Tr, br = evaluate(pts, K, idx[None, :], **kw)
            out["refined"][h], out["refined_T"][h], out["refined_bits"][h] = c[0], Tr[0], br[0]
            out["n_records"] += 1
    return out


def unpack_bits(words, n):
    b = np.unpackbits(np.ascontiguousarray(words, "<u8").view(np.uint8), bitorder="little")
    return b[:n].astype(bool)


# ---------------------------------------------------------------------------------------------------------------------
# SetRansacParameters, iterate / find / Refine
# ---------------------------------------------------------------------------------------------------------------------
def _to_int(x):
    """A double converted to int as the reference's build does (cvttsd2si): out of range or not finite gives INT_MIN."""
    if not math.isfinite(x) or not (-2.0 ** 31 <= x < 2.0 ** 31):
        return -2 ** 31
    return int(x)


def ransac_iterations(N, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4):
    """SetRansacParameters (:131-173) -> (mRansacMinInliers, mRansacMaxIts, mRansacEpsilon)."""
    f32 = np.float32
    eps = f32(epsilon)
    with np.errstate(all="ignore"):
        n_min = _to_int(float(f32(N) * eps))         # int nMinInliers = N * mRansacEpsilon: int * float is a float product
        n_min = max(n_min, min_inliers, min_set)
        ratio = f32(n_min) / f32(N)
        if eps < ratio:
            eps = ratio
        if n_min == N:
            n_it = 1
        else:
            # pow(float, int) is the double pow
            n_it = _to_int(float(np.ceil(np.log(1 - np.float64(probability)) / np.log(1 - np.float64(eps) ** 3))))
    return n_min, max(1, min(n_it, int(max_iterations))), eps


class Sequential:
    """iterate / find / Refine (:175-315) as written.  evaluate(h) -> (count, T12 (12 floats), inliers (N bools)) is compute_pose +
    CheckInliers of the h-th sample ever drawn; refine(inliers) -> the same triple for Refine's compute_pose + CheckInliers on the
    set.  indices[i] = mvKeyPointIndices[i], n_matches = mvpMapPointMatches.size()."""

    def __init__(self, N, min_inliers, max_its, evaluate, refine, indices=None, n_matches=None):
        self.N, self.min_inliers, self.max_its = N, min_inliers, max_its
        self.evaluate, self.refine = evaluate, refine
        self.indices = np.arange(N) if indices is None else np.asarray(indices, np.int64)
        self.n_matches = N if n_matches is None else n_matches
        self.iterations = 0
        self.best_inliers = 0
        self.best_T = None
        self.best_bits = None
        self.refine_calls = 0

    @staticmethod
    def _mat(T):
        M = np.eye(4, dtype=np.float32)
        M[:3, :3] = np.asarray(T[:9], np.float32).reshape(3, 3)
        M[:3, 3] = T[9:12]
        return M

    def _spread(self, bits):
        v = np.zeros(self.n_matches, bool)
        v[self.indices[np.asarray(bits, bool)]] = True
        return v

    def iterate(self, n_iterations):
        """-> (Tcw or None, bNoMore, vbInliers, nInliers)"""
        if self.N < self.min_inliers:
            return None, True, np.zeros(0, bool), 0
        cur = 0
        while self.iterations < self.max_its or cur < n_iterations:
            cur += 1
            h = self.iterations
            self.iterations += 1
            count, T, bits = self.evaluate(h)
            if count >= self.min_inliers:
                if count > self.best_inliers:
                    self.best_bits = np.asarray(bits, bool).copy()
                    self.best_inliers = count
                    self.best_T = self._mat(T)
                self.refine_calls += 1
                rc, rT, rbits = self.refine(self.best_bits)
                if rc > self.min_inliers:
                    return self._mat(rT), False, self._spread(rbits), rc
        if self.iterations >= self.max_its:
            if self.best_inliers >= self.min_inliers:
                return self.best_T.copy(), True, self._spread(self.best_bits), self.best_inliers
            return None, True, np.zeros(0, bool), 0
        return None, False, np.zeros(0, bool), 0

    def find(self):
        T, _, inl, n = self.iterate(self.max_its)
        return T, inl, n


# ---------------------------------------------------------------------------------------------------------------------
# the constructor's gather (:72-121) and scenes
# ---------------------------------------------------------------------------------------------------------------------
def gather(frame, th2=5.991):
    """frame: dict keys (m, 3: x y octave), sigma2 (levels,), matches (m,) index into points or -1, points (p, 3) float32, bad (p,)
    -> PNP_POINT_DTYPE array, mvKeyPointIndices, mvSigma2."""
    f32 = np.float32
    out, idx, sig2 = [], [], []
    for i, m in enumerate(frame["matches"]):
        if m < 0 or frame["bad"][m]:
            continue
        x, y, octv = frame["keys"][i]
        sig = f32(frame["sigma2"][int(octv)])
        out.append((frame["points"][m].astype(f32), f32(x), f32(y), sig * f32(th2)))
        idx.append(i)
        sig2.append(sig)
    return np.array(out, PNP_POINT_DTYPE), np.array(idx, np.int64), np.array(sig2, np.float32)


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * Kx @ Kx


K_DEFAULT = (520.9, 521.0, 325.1, 249.7)


def make_scene(seed, n, noise=0.0, outliers=0.0, duplicates=0, coplanar=False, K=K_DEFAULT, th2=5.991, exact=False):
    """n world points in front of a camera of true pose (R, t): -> dict pts (PNP_POINT_DTYPE), K, R, t, true_inlier (n,) bool.
    noise: pixel sigma; outliers: the share of gross outliers (the image point replaced by a uniform one at least 30 px away); octave-dependent max_err
    (sigma2 = 1.2^(2 octave) * th2); duplicates: that many points repeat the world point of their predecessor (image point too);
    coplanar: all world points on one plane.  exact: the image points are the float roundings of the true projections of the
    float world points (noise-free scenes for the second opinion)."""
    rng = np.random.RandomState(seed)
    R = rotation(rng.standard_normal(3), rng.uniform(0.1, 0.6))
    t = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(0.0, 1.0)])
    fx, fy, cx, cy = (float(np.float32(v)) for v in K)
    u = rng.uniform(20, 620, n); v = rng.uniform(20, 460, n)
    z = np.full(n, 5.0) if coplanar else rng.uniform(2.0, 9.0, n)
    Xc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=1)
    if coplanar:
        Xc[:, 2] += 0.3 * (Xc[:, 0] - Xc[:, 1])         # a tilted plane
    Xw = ((Xc - t) @ R).astype(np.float32)               # R' (Xc - t)
    for d in range(duplicates):
        j = 1 + (d * 7) % (n - 1)
        Xw[j] = Xw[j - 1]
    Pc = Xw.astype(np.float64) @ R.T + t
    uv = np.stack([fx * Pc[:, 0] / Pc[:, 2] + cx, fy * Pc[:, 1] / Pc[:, 2] + cy], axis=1)
    uv = uv + noise * rng.standard_normal((n, 2))
    out = rng.permutation(n)[: int(round(outliers * n))]
    gross = np.stack([rng.uniform(0, 640, out.size), rng.uniform(0, 480, out.size)], axis=1)
    near = np.hypot(gross[:, 0] - uv[out, 0], gross[:, 1] - uv[out, 1]) < 30.0      # (the largest threshold is a radius of 8.8 px)
    gross[near, 0] += 60.0
    uv[out] = gross
    true_in = np.ones(n, bool)
    true_in[out] = False
    octave = rng.randint(0, 8, n)
    pts = np.zeros(n, PNP_POINT_DTYPE)
    pts["xw"] = Xw
    pts["u"], pts["v"] = uv[:, 0].astype(np.float32), uv[:, 1].astype(np.float32)
    pts["max_err"] = (np.float32(1.2) ** (2 * octave)).astype(np.float32) * np.float32(th2)
    return {"pts": pts, "K": tuple(np.float32(v) for v in K), "R": R, "t": t, "true_inlier": true_in}


def draw_samples(rng, n, n_hyp, within=None):
    """PnPsolver.cc:203-220: four draws without replacement per hypothesis (within: draw from these indices only)."""
    S = np.zeros((n_hyp, 4), np.int32)
    for h in range(n_hyp):
        avail = list(range(n)) if within is None else list(within)
        for i in range(4):
            r = rng.randint(0, len(avail))
            S[h, i] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return S
