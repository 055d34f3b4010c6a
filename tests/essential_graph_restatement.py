"""Float64 restatement of Optimizer::OptimizeEssentialGraph (reference src/orbslam/Optimizer.cc:928-1233) with the g2o arithmetic
it relies on: g2o::Sim3::log (types/sim3/sim3.h, four branches, W.lu().solve(t)), EdgeSim3::computeError (log(Sji * Si * Sj^-1)),
BaseBinaryEdge's numeric linearizeOplus (central differences, delta = 1e-9, through VertexSim3Expmap::oplus) and
OptimizationAlgorithmLevenberg with setUserLambdaInit(1e-16).  The Sim3 primitives come from sim3_restatement; everything per edge
is vectorised over the edges (a Sim3 batch is an (n, 8) array: qx qy qz qw tx ty tz s).  The linear solve is dense numpy (or
scipy.sparse for the large scene): the checker of sivo_amd/csrc/essential_graph.hip, which agrees with it to rounding.

Also: a synthetic map (keyframes with a spanning tree, covisibility weights, loop edges, a loop closure's LoopConnections /
CorrectedSim3 / NonCorrectedSim3), the walk of Optimizer.cc:964-1175 over it, the pose write-back and the point correction, and
the text form tests/essential_graph_prog.cpp reads.  Test infrastructure, not the product."""
import math

import numpy as np

import sim3_restatement as S3

DELTA = S3.DELTA
SCALAR = S3.SCALAR
EPS = 0.00001
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0, 1], np.float64)
# a relative change of every acos result (0 = none): the sensitivity of g2o's arithmetic to a one-ulp difference of the math library,
# the measure of the parity tolerance (tests/test_essential_graph_host.py::test_one_ulp_sensitivity)
ACOS_JITTER = 0.0


# ---- Sim3 batches --------------------------------------------------------------------------------------------------
def _split(A):
    A = np.asarray(A, np.float64)
    return ([A[..., 0], A[..., 1], A[..., 2], A[..., 3]], [A[..., 4], A[..., 5], A[..., 6]], A[..., 7])


def _pack(S):
    q, t, s = S
    return np.stack([np.broadcast_to(np.asarray(v, np.float64), np.shape(s)) for v in (*q, *t, s)], -1)


def mul(A, B):
    """g2o::Sim3::operator* over batches (broadcasting)."""
    return _pack(S3.sim3_mul(_split(A), _split(B)))


def inv(A):
    return _pack(S3.sim3_inv(_split(A)))


def sim3_map(A, X):
    """s * (r * X) + t; A (n, 8), X (n, 3)."""
    q, t, s = _split(A)
    r = S3.quat_rotate(q, [X[..., 0], X[..., 1], X[..., 2]])
    return np.stack([s * r[i] + t[i] for i in range(3)], -1)


def exp(u):
    """g2o::Sim3(const Vector7d &) of one update (sim3_restatement.sim3_exp) as an (8,) array."""
    q, t, s = S3.sim3_exp(u)
    return np.array(list(q) + list(t) + [s], np.float64)


def quat_to_matrix(q):
    """Eigen's toRotationMatrix over a batch of quaternions (..., 4) -> (..., 3, 3)."""
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.stack([np.stack([1 - (tyy + tzz), txy - twz, txz + twy], -1), np.stack([txy + twz, 1 - (txx + tzz), tyz - twx], -1),
                     np.stack([txz - twy, tyz + twx, 1 - (txx + tyy)], -1)], -2)


def _lu3_solve(W, b):
    """W.lu().solve(b) for a batch of 3 x 3 (partial pivoting: the first largest |entry| of the column; unit lower L, then U)."""
    M = W.copy()
    b = b.copy()
    n = M.shape[0]
    ar = np.arange(n)
    for k in range(3):
        p = k + np.argmax(np.abs(M[:, k:, k]), axis=1)
        rows_k, rows_p = M[ar, k, :].copy(), M[ar, p, :].copy()
        M[ar, k, :], M[ar, p, :] = rows_p, rows_k
        bk, bp = b[ar, k].copy(), b[ar, p].copy()
        b[ar, k], b[ar, p] = bp, bk
        piv = M[:, k, k]
        for i in range(k + 1, 3):
            M[:, i, k] = np.where(piv != 0.0, M[:, i, k] / np.where(piv != 0.0, piv, 1.0), M[:, i, k])
            for c in range(k + 1, 3):
                M[:, i, c] = M[:, i, c] - M[:, i, k] * M[:, k, c]
    for i in range(1, 3):
        for m in range(i):
            b[:, i] = b[:, i] - M[:, i, m] * b[:, m]
    for i in (2, 1, 0):
        for m in range(i + 1, 3):
            b[:, i] = b[:, i] - M[:, i, m] * b[:, m]
        b[:, i] = b[:, i] / M[:, i, i]
    return b


def sim3_log(A):
    """g2o::Sim3::log over a batch (n, 8) -> (n, 7) = [omega, upsilon, sigma]."""
    A = np.atleast_2d(np.asarray(A, np.float64))
    s = A[:, 7]
    with np.errstate(all="ignore"):
        sigma = np.log(s)
        R = quat_to_matrix(A[:, :4])
        d = 0.5 * (R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] - 1)
        dR = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], -1)
        near = d > 1 - EPS
        theta = np.where(near, 0.0, np.arccos(np.clip(d, -1.0, 1.0)) * (1.0 + ACOS_JITTER))
        f = np.where(near, 0.5, theta / (2 * np.sqrt(1 - d * d)))
        om = f[:, None] * dR
        small_sigma = np.abs(sigma) < EPS
        theta2 = theta * theta
        sigma2 = sigma * sigma
        # |sigma| < eps
        A0 = np.where(near, 1.0 / 2.0, (1 - np.cos(theta)) / (theta2))
        B0 = np.where(near, 1.0 / 6.0, (theta - np.sin(theta)) / (theta2 * theta))
        # |sigma| >= eps
        C1 = (s - 1) / sigma
        a = s * np.sin(theta)
        b = s * np.cos(theta)
        c = theta2 + sigma2
        A1 = np.where(near, ((sigma - 1) * s + 1) / (sigma2), (a * sigma + (1 - b) * theta) / (theta * c))
        B1 = np.where(near, ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma), (C1 - ((b - 1) * sigma + a * theta) / (c)) * 1.0 / (theta2))
        Ac = np.where(small_sigma, A0, A1)
        Bc = np.where(small_sigma, B0, B1)
        Cc = np.where(small_sigma, 1.0, C1)
        z = np.zeros_like(s)
        Om = np.stack([np.stack([z, -om[:, 2], om[:, 1]], -1), np.stack([om[:, 2], z, -om[:, 0]], -1),
                       np.stack([-om[:, 1], om[:, 0], z], -1)], -2)
        Om2 = np.empty_like(Om)
        for i in range(3):
            for j in range(3):
                Om2[:, i, j] = Om[:, i, 0] * Om[:, 0, j] + Om[:, i, 1] * Om[:, 1, j] + Om[:, i, 2] * Om[:, 2, j]
        I = np.eye(3)[None]
        W = Ac[:, None, None] * Om + Bc[:, None, None] * Om2 + Cc[:, None, None] * I
        ups = _lu3_solve(W, A[:, 4:7])
    return np.concatenate([om, ups, sigma[:, None]], 1)


def sim3_exp_batch(U):
    return np.stack([exp(u) for u in U]) if len(U) else np.zeros((0, 8))


# ---- the graph -----------------------------------------------------------------------------------------------------
def edge_errors(est, ei, ej, meas):
    """EdgeSim3::computeError of every edge: log(Sji * Si * Sj^-1)."""
    return sim3_log(mul(mul(meas, est[ei]), inv(est[ej])))


def chi2(est, ei, ej, meas):
    if len(ei) == 0:
        return 0.0
    e = edge_errors(est, ei, ej, meas)
    return float(np.sum(np.sum(e * e, 1)))


def _perturbation_exps(fix_scale):
    out = []
    for d in range(7):
        for sgn in (1.0, -1.0):
            u = [0.0] * 7
            u[d] = sgn * DELTA
            if fix_scale:
                u[6] = 0.0
            out.append(exp(u))
    return np.stack(out)


def jacobians(est, ei, ej, meas, free, fix_scale):
    """BaseBinaryEdge::linearizeOplus: Ji, Jj (ne, 7, 7) [error component, dof] (zero for a fixed side), and the errors."""
    E = _perturbation_exps(fix_scale)
    ne = len(ei)
    e0 = edge_errors(est, ei, ej, meas)
    Ji, Jj = np.zeros((ne, 7, 7)), np.zeros((ne, 7, 7))
    Sj_inv = inv(est[ej])
    CSi = mul(meas, est[ei])
    for d in range(7):
        Pp, Pm = mul(E[2 * d][None], est[ei]), mul(E[2 * d + 1][None], est[ei])
        ep = sim3_log(mul(mul(meas, Pp), Sj_inv))
        em = sim3_log(mul(mul(meas, Pm), Sj_inv))
        Ji[:, :, d] = SCALAR * (ep - em)
        Qp, Qm = inv(mul(E[2 * d][None], est[ej])), inv(mul(E[2 * d + 1][None], est[ej]))
        ep = sim3_log(mul(CSi, Qp))
        em = sim3_log(mul(CSi, Qm))
        Jj[:, :, d] = SCALAR * (ep - em)
    Ji[~free[ei]] = 0.0
    Jj[~free[ej]] = 0.0
    return Ji, Jj, e0


def optimize(siw, fixed, edges, fix_scale, iterations=20, sparse=False):
    """SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg (lambda_0 = 1e-16) over the graph.  siw (n, 8),
    fixed (n,) bool, edges = SIM3_EDGE_DTYPE records.  Returns dict(siw, chi2_start, chi2, iterations, trials)."""
    est = np.array(siw, np.float64).reshape(-1, 8).copy()
    n = est.shape[0]
    fixed = np.asarray(fixed, bool)
    ei = np.asarray(edges["i"], np.int64)
    ej = np.asarray(edges["j"], np.int64)
    meas = np.asarray(edges["meas"], np.float64).reshape(-1, 8)
    on_edge = np.zeros(n, bool)
    on_edge[ei] = True
    on_edge[ej] = True
    free = on_edge & ~fixed
    var = np.flatnonzero(free)
    slot = -np.ones(n, np.int64)
    slot[var] = np.arange(len(var))
    na = len(var)
    current = chi2(est, ei, ej, meas)
    out = {"chi2_start": current, "iterations": 0, "trials": 0}
    if len(ei) == 0 or na == 0:
        out.update(siw=est, chi2=current)
        return out
    lam, ni = 1e-16, 2.0
    it = trials = 0
    for it_ in range(iterations):
        Ji, Jj, e0 = jacobians(est, ei, ej, meas, free, fix_scale)
        H = np.zeros((7 * na, 7 * na))
        b = np.zeros(7 * na)
        si, sj = slot[ei], slot[ej]
        blocks = []
        for Ja, sa in ((Ji, si), (Jj, sj)):
            JtJ = np.einsum("kmr,kmc->krc", Ja, Ja)
            Jte = -np.einsum("kmr,km->kr", Ja, e0)
            for k in np.flatnonzero(sa >= 0):
                p = 7 * sa[k]
                H[p:p + 7, p:p + 7] += JtJ[k]
                b[p:p + 7] += Jte[k]
        Hij = np.einsum("kmr,kmc->krc", Ji, Jj)
        for k in np.flatnonzero((si >= 0) & (sj >= 0)):
            p, q = 7 * si[k], 7 * sj[k]
            H[p:p + 7, q:q + 7] += Hij[k]
            H[q:q + 7, p:p + 7] += Hij[k].T
        qmax = 0
        while True:
            A = H + lam * np.eye(7 * na)
            ok = True
            try:
                if sparse:
                    import scipy.sparse
                    import scipy.sparse.linalg
                    x = scipy.sparse.linalg.spsolve(scipy.sparse.csc_matrix(A), b)
                    ok = bool(np.all(np.isfinite(x)))
                else:
                    Lc = np.linalg.cholesky(A)
                    x = np.linalg.solve(Lc.T, np.linalg.solve(Lc, b))
            except np.linalg.LinAlgError:
                ok = False
                x = np.zeros(7 * na)
            if fix_scale:
                x[6::7] = 0.0
            trial = est.copy()
            if ok:
                X = x.reshape(na, 7)
                trial[var] = mul(sim3_exp_batch(X), est[var])
            temp = chi2(trial, ei, ej, meas) if ok else np.finfo(np.float64).max
            scale = float(np.dot(x, lam * x + b)) if ok else 0.0
            rho = (current - temp) / (scale + 1e-3)
            if rho > 0 and np.isfinite(temp):
                alpha = 1.0 - (2 * rho - 1) ** 3
                alpha = min(alpha, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                current = temp
                est = trial
            else:
                lam *= ni
                ni *= 2
            qmax += 1
            trials += 1
            if not (rho < 0 and qmax < 10):
                break
        it += 1
        if qmax == 10 or rho == 0:
            break
    out.update(siw=est, chi2=current, iterations=it, trials=trials)
    return out


# ---- write-back (Optimizer.cc:1182-1233) ------------------------------------------------------------------------------
def pose_from_sim3(S):
    """SetPose(Converter::toCvSE3(eigR, eigt)) of one optimised Siw: R = toRotationMatrix, t *= 1 / s, both to float."""
    S = np.asarray(S, np.float64)
    R = quat_to_matrix(S[:4])
    t = S[4:7] * (1.0 / S[7])
    T = np.zeros((4, 4), np.float32)
    T[:3, :3] = R.astype(np.float32)
    T[:3, 3] = t.astype(np.float32)
    T[3, 3] = 1.0
    return T


def correct_points(xyz, ref, before, after):
    """correctedSwr.map(Srw.map(P)) in double from the float position, back to float; ref = -1: unchanged."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    ref = np.asarray(ref, np.int64)
    out = xyz.copy()
    k = np.flatnonzero(ref >= 0)
    if len(k):
        P = xyz[k].astype(np.float64)
        Y = sim3_map(np.asarray(before)[ref[k]], P)
        Z = sim3_map(inv(np.asarray(after)[ref[k]]), Y)
        out[k] = Z.astype(np.float32)
    return out


# ---- synthetic maps ------------------------------------------------------------------------------------------------
def sim3_from_pose(Tcw):
    """g2o::Sim3(Rcw, tcw, 1.0) from a float pose: Quaterniond(R) (trace-branch construction, not normalised)."""
    Tcw = np.asarray(Tcw, np.float32)
    R = [[float(Tcw[r, c]) for c in range(3)] for r in range(3)]
    q = S3.quat_from_matrix(R)
    return np.array(q + [float(Tcw[r, 3]) for r in range(3)] + [1.0], np.float64)


def _rot(rng, max_angle):
    return np.asarray(S3.random_rotation(rng, max_angle), np.float64)


def _pose(R, t):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


def make_map(n_kf, seed, n_loops=2, fix_scale=True, n_points=0, covis=5, falloff=45):
    """A keyframe map after a loop detection, as LoopClosing::CorrectLoop hands it to OptimizeEssentialGraph.
    Keyframes walk a closed loop with drifting odometry (the estimated poses), ids with gaps (erased keyframes) and one bad keyframe
    left in the list; the spanning tree follows the walk; covisibility weights to the previous `covis` keyframes fall off from
    above 100 to below it; `n_loops` older loop edges; the current keyframe (the last) closes the loop on an early one: its
    neighbourhood gets CorrectedSim3 (the drift removed, a scale under fix_scale = False) and NonCorrectedSim3 (its drifted poses), and
    LoopConnections joins it to the loop keyframe's neighbourhood — with a pair below weight 100 (skipped), the (current, loop) pair
    below 100 (kept), and one pair that is also a spanning-tree edge (a duplicated vertex pair)."""
    rng = np.random.default_rng(seed)
    ids, nid = [], 0
    for k in range(n_kf):
        ids.append(nid)
        nid += 1 + (1 if rng.random() < 0.05 else 0)
    R_true, t_true, R_est, t_est = [], [], [], []
    radius = 10.0 + 0.02 * n_kf
    Rd, td = np.eye(3), np.zeros(3)
    for k in range(n_kf):
        a = 2 * math.pi * k / n_kf
        c = np.array([radius * math.cos(a), radius * math.sin(a), 0.3 * math.sin(3 * a)])
        yaw = a + math.pi / 2
        Rwc = np.array([[math.cos(yaw), -math.sin(yaw), 0], [math.sin(yaw), math.cos(yaw), 0], [0, 0, 1]]) @ _rot(rng, 0.05)
        Rcw = Rwc.T
        tcw = -Rcw @ c
        R_true.append(Rcw)
        t_true.append(tcw)
        # drift: a slowly growing rotation / translation error composed on the world side
        if k:
            Rd = _rot(rng, 0.004) @ Rd
            td = td + rng.normal(size=3) * 0.01 + np.array([0.004, 0.002, 0.0])
        R_est.append(Rcw @ Rd.T)
        t_est.append(tcw - (Rcw @ Rd.T) @ td)
    Tcw = [_pose(R_est[k], t_est[k]) for k in range(n_kf)]
    kfs = []
    for k in range(n_kf):
        kfs.append({"id": ids[k], "Tcw": Tcw[k], "bad": False, "parent": k - 1 if k else -1, "children": set(), "loop": set(),
                    "weights": {}})
    for k in range(1, n_kf):
        kfs[kfs[k]["parent"]]["children"].add(k)

    def connect(a, b, w):
        kfs[a]["weights"][b] = w
        kfs[b]["weights"][a] = w

    for k in range(n_kf):
        for d in range(1, covis + 1):
            if k - d >= 0:
                connect(k, k - d, int(max(15, 260 - falloff * d + rng.integers(-20, 20))))
    # one bad keyframe left in the list (its vertex is skipped; covisibility edges to it are skipped)
    bad = n_kf // 3
    kfs[bad]["bad"] = True
    for c in list(kfs[bad]["children"]):
        kfs[c]["parent"] = bad - 1
        kfs[bad - 1]["children"].add(c)
    kfs[bad]["children"] = set()
    kfs[kfs[bad]["parent"]]["children"].discard(bad)
    kfs[bad]["parent"] = -1
    # older loop edges (both sides record them)
    for q in range(n_loops):
        a = int(n_kf * (0.45 + 0.15 * q)) if n_kf > 20 else n_kf // 2
        b = 2 + 3 * q
        if a == bad or b == bad or a <= b:
            continue
        kfs[a]["loop"].add(b)
        kfs[b]["loop"].add(a)
        connect(a, b, 140)
    cur, lp = n_kf - 1, 1
    cur_nb = [cur - d for d in range(0, 4)]
    loop_nb = [lp - 1, lp, lp + 1, lp + 2]
    # CorrectedSim3 / NonCorrectedSim3 of the current neighbourhood: corrected = the true pose (scaled under fix_scale = False)
    scale = 1.0 if fix_scale else 1.07
    corrected, noncorrected = {}, {}
    for k in cur_nb:
        Rt, tt = R_true[k], t_true[k]
        q = S3.quat_from_matrix(Rt.tolist())
        nq = math.sqrt(sum(v * v for v in q))
        corrected[k] = np.array([v / nq for v in q] + list(scale * tt) + [scale], np.float64)
        noncorrected[k] = sim3_from_pose(Tcw[k])
    # LoopConnections: the current neighbourhood to the loop neighbourhood
    conns = {}
    for a in cur_nb:
        conns[a] = set()
        for b in loop_nb:
            w = 120 + 10 * ((a + b) % 5)
            if (a, b) == (cur, lp):
                w = 40                            # (cur, loop) below 100: kept
            elif (a, b) == (cur - 1, lp + 2):
                w = 60                            # below 100: skipped
            conns[a].add(b)
            connect(a, b, w)
    # a connection that duplicates a spanning-tree edge
    conns[cur].add(cur - 1)
    return {"kfs": kfs, "ids": ids, "max_id": max(ids), "cur": cur, "loop": lp, "corrected": corrected, "noncorrected": noncorrected,
            "conns": conns, "fix_scale": fix_scale, "truth": [(R_true[k], t_true[k]) for k in range(n_kf)],
            "order": list(rng.permutation(n_kf)), "points": _make_points(rng, kfs, ids, cur, n_points)}


def _make_points(rng, kfs, ids, cur, n_points):
    pts = []
    for p in range(n_points):
        ref = int(rng.integers(0, len(kfs)))
        T = kfs[ref]["Tcw"].astype(np.float64)
        Xc = np.array([rng.normal() * 2, rng.normal(), 4 + 6 * rng.random()])
        Xw = T[:3, :3].T @ (Xc - T[:3, 3])
        corrected_by = ids[cur] if rng.random() < 0.2 else 0         # (MapPoint::mnCorrectedByKF starts at 0)
        corr_ref = int(rng.integers(0, len(kfs)))
        pts.append({"pos": Xw.astype(np.float32), "bad": bool(rng.random() < 0.05), "ref": ref, "corrected_by": corrected_by,
                    "corrected_ref": ids[corr_ref]})
    return pts


def covisibles_by_weight(kf, w):
    """KeyFrame::GetCovisiblesByWeight(w) (KeyFrame.cc:232-250) over the weight map: connections ordered by weight (descending,
    ties by index as the stand-in orders them), those with weight >= w — and, as the reference's upper_bound test has it, NONE when
    every connection has weight >= w."""
    items = sorted(kf["weights"].items(), key=lambda kv: (-kv[1], kv[0]))
    n = sum(1 for _, wt in items if wt >= w)
    if n == len(items):
        return []
    return [k for k, _ in items[:n]]


def gather(m):
    """The walk of Optimizer.cc:964-1175 over a make_map() map, keyframes in m["order"] (GetAllKeyFrames).  Returns (siw (max_id + 1,
    8) with identity where no vertex, fixed (max_id + 1,), vertex (max_id + 1,) bool, SIM3_EDGE_DTYPE edges in insertion order).
    Bad keyframes are skipped in the normal-edge walk and edges to a keyframe without a vertex are left out (the reference would
    dereference null there)."""
    from sivo_amd.optimizer import SIM3_EDGE_DTYPE
    kfs, ids = m["kfs"], m["ids"]
    n = m["max_id"] + 1
    siw = np.tile(IDENTITY, (n, 1))
    fixed = np.zeros(n, bool)
    vertex = np.zeros(n, bool)
    for k in m["order"]:
        kf = kfs[k]
        if kf["bad"]:
            continue
        i = ids[k]
        siw[i] = m["corrected"][k] if k in m["corrected"] else sim3_from_pose(kf["Tcw"])
        vertex[i] = True
        fixed[i] = k == m["loop"]
    edges = []
    inserted = set()

    def add(i, j, S):
        if vertex[i] and vertex[j]:
            edges.append((i, j, S))

    cur, lp = m["cur"], m["loop"]
    for a in sorted(m["conns"]):
        i = ids[a]
        Swi = inv(siw[i][None])[0]
        for b in sorted(m["conns"][a]):
            j = ids[b]
            if (a != cur or b != lp) and kfs[a]["weights"].get(b, 0) < 100:
                continue
            add(i, j, mul(siw[j][None], Swi[None])[0])
            inserted.add((min(i, j), max(i, j)))

    def s_w(k):
        return m["noncorrected"][k] if k in m["noncorrected"] else siw[ids[k]]

    for k in m["order"]:
        kf = kfs[k]
        if kf["bad"]:
            continue
        i = ids[k]
        Swi = inv(s_w(k)[None])[0]
        par = kf["parent"]
        if par >= 0:
            add(i, ids[par], mul(s_w(par)[None], Swi[None])[0])
        for l in sorted(kf["loop"]):
            if ids[l] < i:
                add(i, ids[l], mul(s_w(l)[None], Swi[None])[0])
        for c in covisibles_by_weight(kf, 100):
            if c == par or c in kf["children"] or c in kf["loop"]:
                continue
            if kfs[c]["bad"] or ids[c] >= i:
                continue
            if (min(i, ids[c]), max(i, ids[c])) in inserted:
                continue
            add(i, ids[c], mul(s_w(c)[None], Swi[None])[0])
    e = np.zeros(len(edges), SIM3_EDGE_DTYPE)
    for q, (i, j, S) in enumerate(edges):
        e[q]["i"], e[q]["j"], e[q]["meas"] = i, j, S
    return siw, fixed, vertex, e


def point_refs(m, vertex):
    """The reference keyframe id of every map point for the correction (-1: bad point, or no vertex of that id)."""
    ref = []
    for p in m["points"]:
        if p["bad"]:
            ref.append(-1)
            continue
        r = p["corrected_ref"] if p["corrected_by"] == m["ids"][m["cur"]] else m["ids"][p["ref"]]
        ref.append(r if 0 <= r < len(vertex) and vertex[r] else -1)
    return np.array(ref, np.int64)


def true_graph(n, seed, fix_scale, extra=3):
    """A graph whose measurements come from known Sim3 vertices (a chain plus `extra` random edges per vertex): returns (truth (n, 8),
    perturbed initial estimates, fixed (vertex 0), edges)."""
    from sivo_amd.optimizer import SIM3_EDGE_DTYPE
    rng = np.random.default_rng(seed)
    truth = np.zeros((n, 8))
    for v in range(n):
        u = np.concatenate([rng.normal(size=3) * 0.5, rng.normal(size=3) * 3, [0.0 if fix_scale else rng.normal() * 0.2]])
        truth[v] = exp(u)
    pairs = [(v, v - 1) for v in range(1, n)]
    for v in range(n):
        for _ in range(extra):
            w = int(rng.integers(0, n))
            if w != v:
                pairs.append((v, w))
    e = np.zeros(len(pairs), SIM3_EDGE_DTYPE)
    for q, (i, j) in enumerate(pairs):
        e[q]["i"], e[q]["j"] = i, j
        e[q]["meas"] = mul(truth[j][None], inv(truth[i][None]))[0]
    init = truth.copy()
    for v in range(1, n):
        # (the scales start at the truth: a residual whose |sigma| shrinks through (1e-5, ~1e-3) with a near-identity rotation meets
        # g2o's Sim3::log without the "- 1" of its B series, where W ~ 1 / sigma^3 — see test_numeric_jacobian_matches_...)
        u = np.concatenate([rng.normal(size=3) * 0.02, rng.normal(size=3) * 0.05, [0.0]])
        init[v] = mul(exp(u)[None], truth[v][None])[0]
    fixed = np.zeros(n, bool)
    fixed[0] = True
    return truth, init, fixed, e


# ---- text form of tests/essential_graph_prog.cpp ----------------------------------------------------------------------
def map_text(m):
    f = lambda v: repr(float(np.float32(v)))
    d = lambda v: repr(float(v))
    kfs, ids = m["kfs"], m["ids"]
    out = [f"{len(kfs)} {len(m['points'])} {m['cur']} {m['loop']} {int(m['fix_scale'])}"]
    out.append(" ".join(str(int(k)) for k in m["order"]))
    for k, kf in enumerate(kfs):
        out.append(f"{ids[k]} {int(kf['bad'])} {kf['parent']} " + " ".join(f(kf["Tcw"][r, c]) for r in range(3) for c in range(4)))
        out.append(f"{len(kf['children'])} " + " ".join(str(c) for c in sorted(kf["children"])))
        out.append(f"{len(kf['loop'])} " + " ".join(str(c) for c in sorted(kf["loop"])))
        items = sorted(kf["weights"].items(), key=lambda kv: (-kv[1], kv[0]))
        out.append(f"{len(items)} " + " ".join(f"{c} {w}" for c, w in items))
    for name in ("corrected", "noncorrected"):
        out.append(f"{len(m[name])} " + " ".join(f"{k} " + " ".join(d(v) for v in m[name][k]) for k in sorted(m[name])))
    out.append(f"{len(m['conns'])}")
    for a in sorted(m["conns"]):
        out.append(f"{a} {len(m['conns'][a])} " + " ".join(str(b) for b in sorted(m["conns"][a])))
    for p in m["points"]:
        out.append(" ".join(f(v) for v in p["pos"]) + f" {int(p['bad'])} {p['ref']} {p['corrected_by']} {p['corrected_ref']}")
    return "\n".join(out) + "\n"
