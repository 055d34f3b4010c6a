"""The sparse path of the bundle adjustment's reduced camera system without a GPU: the host plan and the per-block bodies the kernels
use, run in sequence by a stand-alone program (tests/ba_sparse_prog.cpp) against a dense float64 solve in numpy; sivo_ba_analyze through
the library; the essential-graph plan, which now stands on the same pattern code, against the figures of the parent commit; the ABI."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

from conftest import ROOT, make_ba_scene
import ba_sparse_cases as S
import essential_graph_restatement as E
import host_prog

EPS = np.finfo(np.float64).eps


# ------------------------------------------------------------------------------------------------
# 1. the stand-alone factor-and-solve program
# ------------------------------------------------------------------------------------------------
def _inputs(seed, n_poses, fixed, n_pts, edges, level, lam):
    """Random blocks with the structure of a Gauss-Newton system, so that S is positive definite and well conditioned: per edge a
    3 x 6 and a 3 x 3 Jacobian, W = Jp' Jx, Hpp / Hll the sums of Jp' Jp / Jx' Jx over the ACTIVE edges (+ I / 2 on the points).  W of
    an edge the solver must not read (excluded, or of a fixed pose) is NaN."""
    rng = np.random.default_rng(seed)
    nE = len(edges)
    slot = np.cumsum(fixed == 0) - 1
    slot[fixed != 0] = -1
    nF = int((fixed == 0).sum())
    Jp = rng.normal(size=(nE, 3, 6)); Jx = rng.normal(size=(nE, 3, 3))
    W = np.einsum("eka,ekb->eab", Jp, Jx)
    Hll = np.tile(0.5 * np.eye(3), (n_pts, 1, 1)); Hpp = np.zeros((nF, 6, 6))
    es = slot[edges["pose"]]
    for e in np.flatnonzero(level == 0):
        Hll[edges["point"][e]] += Jx[e].T @ Jx[e]
        if es[e] >= 0:
            Hpp[es[e]] += Jp[e].T @ Jp[e]
    W[(level != 0) | (es < 0)] = np.nan
    return {"n_poses": n_poses, "fixed": fixed, "n_pts": n_pts, "edges": edges, "level": level, "lam": lam, "slot": slot, "nF": nF,
            "W": W, "Hll": Hll, "bl": rng.normal(size=(n_pts, 3)), "Hpp": Hpp, "bp": rng.normal(size=(nF, 6))}


def _blob(p):
    return b"".join([struct.pack("<iiid", p["n_poses"], p["n_pts"], len(p["edges"]), p["lam"]), p["fixed"].astype(np.uint8).tobytes(),
                     p["level"].astype(np.uint8).tobytes(), np.ascontiguousarray(p["edges"], S.EDGE_DTYPE).tobytes()] +
                    [np.ascontiguousarray(p[k], np.float64).tobytes() for k in ("W", "Hll", "bl", "Hpp", "bp")])


def _parse(out):
    nF, n_own, l_off, levels, ok = struct.unpack_from("<5i", out, 0)
    at = 20
    rc = np.frombuffer(out, np.int32, 2 * n_own, at).reshape(n_own, 2); at += 8 * n_own
    Sb = np.frombuffer(out, np.float64, 36 * n_own, at).reshape(n_own, 6, 6); at += 288 * n_own
    rhs = np.frombuffer(out, np.float64, 6 * nF, at); at += 48 * nF
    x = np.frombuffer(out, np.float64, 6 * nF, at); at += 48 * nF
    assert at == len(out)
    return {"nF": nF, "l_off": l_off, "levels": levels, "ok": ok, "rc": rc, "S": Sb, "rhs": rhs, "x": x}


def _dense(p):
    """S and the right-hand side in float64 from the same inputs, and the pairs of free poses that share a point on ANY edge."""
    nF, lam, edges, slot = p["nF"], p["lam"], p["edges"], p["slot"]
    Sd = np.zeros((6 * nF, 6 * nF)); rhs = p["bp"].reshape(-1).copy()
    for s in range(nF):
        Sd[6 * s:6 * s + 6, 6 * s:6 * s + 6] = p["Hpp"][s] + lam * np.eye(6)
    pattern = {(s, s) for s in range(nF)}
    order = np.argsort(edges["point"], kind="stable")
    seen, first = np.unique(edges["point"][order], return_index=True)
    for q, grp in zip(seen, np.split(order, first[1:])):
        free = [(slot[edges["pose"][e]], e) for e in grp if slot[edges["pose"][e]] >= 0]
        Ai = np.linalg.inv(p["Hll"][q] + lam * np.eye(3))
        for si, ei in free:
            for sj, ej in free:
                pattern.add((max(si, sj), min(si, sj)))
                if p["level"][ei] == 0 and p["level"][ej] == 0:
                    Sd[6 * si:6 * si + 6, 6 * sj:6 * sj + 6] -= p["W"][ei] @ Ai @ p["W"][ej].T
            if p["level"][ei] == 0:
                rhs[6 * si:6 * si + 6] -= p["W"][ei] @ Ai @ p["bl"][q]
    return Sd, rhs, pattern


def _check(p, r, tag):
    Sd, rhs, pattern = _dense(p)
    nF = p["nF"]
    assert r["nF"] == nF
    # one owner per block of the pattern, named by its (row, column) slots either way round
    got = {(max(a, b), min(a, b)) for a, b in r["rc"].tolist()}
    assert got == pattern and len(r["rc"]) == len(pattern), tag
    worst = 0.0
    for (a, b), blk in zip(r["rc"].tolist(), r["S"]):
        want = Sd[6 * a:6 * a + 6, 6 * b:6 * b + 6]
        if a == b:                                  # (the factorisation reads the lower triangle of a diagonal block)
            blk, want = np.tril(blk), np.tril(want)
        scale = np.abs(want).max()
        if scale == 0.0:
            assert not blk.any(), (tag, a, b)
            continue
        worst = max(worst, np.abs(blk - want).max() / scale)
    assert worst <= 1e-12, (tag, worst)
    assert np.abs(r["rhs"] - rhs).max() <= 1e-12 * max(np.abs(rhs).max(), 1.0), tag
    assert r["ok"] == 1, tag
    if nF == 0:
        return
    cond = np.linalg.cond(Sd)
    xd = np.linalg.solve(Sd, rhs)
    rel = np.linalg.norm(r["x"] - xd) / np.linalg.norm(xd)
    print(f"[ba_sparse host {tag}] nF {nF}, {len(pattern) - nF} blocks of S below the diagonal, {r['l_off']} of L, {r['levels']} levels, "
          f"S blocks within {worst:.2e}, cond(S) {cond:.3e}, |x - x_numpy| / |x_numpy| {rel:.2e} (bound {100 * EPS * cond:.2e})")
    assert rel <= 100 * EPS * cond, (tag, rel, cond)


def _edges(rows):
    e = np.zeros(len(rows), S.EDGE_DTYPE)
    e["pose"] = [r[0] for r in rows]; e["point"] = [r[1] for r in rows]
    return e


def _cases():
    """name -> (n_poses, fixed, n_pts, edges, level)"""
    c = {}
    # nF = 1: one fixed, one free keyframe, five points
    c["one_free"] = (2, [1, 0], 5, _edges([(0, q) for q in range(5)] + [(1, q) for q in range(1, 5)]), None)
    # nF = 2 sharing one point (point 2); the same with that point's edge of keyframe 2 excluded: a zero block that stays in the pattern
    two = _edges([(0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (2, 2), (2, 3), (2, 4), (0, 3), (0, 4)])
    c["two_free_one_shared"] = (3, [1, 0, 0], 5, two, None)
    c["shared_point_excluded"] = (3, [1, 0, 0], 5, two, (two["pose"] == 2) & (two["point"] == 2))
    for name, (n_kf, loop) in {"windowed_40": (40, 0), "windowed_48_loop_6": (48, 6)}.items():
        poses, pts, edges, _ = S.windowed_scene(21, n_kf, loop)
        c[name] = (n_kf, [1, 1] + [0] * (n_kf - 2), len(pts), edges, None)
    poses, pts, edges, _ = make_ba_scene(seed=4, n_kf=6, n_pts=300)
    c["fully_covisible"] = (6, [1, 1, 0, 0, 0, 0], len(pts), edges, None)
    poses, pts, edges, _ = S.ring_scene(21, 40)                   # a loop that closes: fill in L
    c["ring_40"] = (40, [1, 1] + [0] * 38, len(pts), edges, None)
    poses, pts, edges, _ = S.windowed_scene(5, 12)
    # a free pose with no edge at all (an extra keyframe nobody observes from), and one whose every edge is excluded
    c["pose_without_edges"] = (13, [1, 1] + [0] * 11, len(pts), edges, None)
    c["pose_all_excluded"] = (12, [1, 1] + [0] * 10, len(pts), edges, edges["pose"] == 6)
    return c


CASES = _cases()


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return host_prog.build("ba_sparse_prog", tmp_path_factory.mktemp("ba_sparse"))


def _problem(name):
    n_poses, fixed, n_pts, edges, level = CASES[name]
    fixed = np.asarray(fixed, np.uint8)
    level = np.zeros(len(edges), np.uint8) if level is None else np.asarray(level, np.uint8)
    return _inputs(len(name), n_poses, fixed, n_pts, edges, level, 0.7)


@pytest.mark.parametrize("name", sorted(CASES))
def test_sparse_walk_matches_the_dense_solve(prog, tmp_path, name):
    p = _problem(name)
    r = _parse(host_prog.run(prog, tmp_path, "solve", _blob(p)))
    _check(p, r, name)
    if name == "windowed_40":
        # points seen only by fixed keyframes are part of this scene (they contribute to no block)
        seen_free = np.zeros(p["n_pts"], bool); seen_free[p["edges"]["point"][p["slot"][p["edges"]["pose"]] >= 0]] = True
        seen = np.zeros(p["n_pts"], bool); seen[p["edges"]["point"]] = True
        assert (seen & ~seen_free).any()
    if name == "ring_40":
        assert r["l_off"] > len(r["rc"]) - r["nF"]               # the factor has blocks S has not
    if name == "shared_point_excluded":
        off = [k for k, (a, b) in enumerate(r["rc"].tolist()) if a != b]
        assert len(off) == 1 and not r["S"][off[0]].any()
    if name in ("pose_without_edges", "pose_all_excluded"):
        s = p["nF"] - 1 if name == "pose_without_edges" else int(p["slot"][6])
        k = [k for k, (a, b) in enumerate(r["rc"].tolist()) if a == b == s][0]
        assert np.array_equal(r["S"][k], 0.7 * np.eye(6))         # S_ii = lambda I


def test_a_pivot_that_is_not_positive_is_reported_and_x_stays_clean(prog, tmp_path):
    p = _problem("windowed_40")
    p["Hpp"][17, 3, 3] = -50.0
    r = _parse(host_prog.run(prog, tmp_path, "solve", _blob(p)))
    assert r["ok"] == 0 and np.isfinite(r["x"]).all() and not r["x"].any()


def test_the_program_is_clean_under_the_sanitizers(tmp_path):
    """The stand-alone program once more under the address and undefined-behaviour sanitizers, on the scenes with the most structure."""
    if not host_prog.sanitizer_runtime_present(tmp_path):
        pytest.skip("g++ has no sanitizer runtime here")
    exe = host_prog.build("ba_sparse_prog", tmp_path, sanitize=True)
    for name in ("one_free", "shared_point_excluded", "pose_without_edges", "ring_40", "windowed_48_loop_6"):
        p = _problem(name)
        _check(p, _parse(host_prog.run(exe, tmp_path, "solve", _blob(p))), name + " (sanitized)")
    p = _problem("ring_40")
    p["Hpp"][5, 0, 0] = -1.0
    assert _parse(host_prog.run(exe, tmp_path, "solve", _blob(p)))["ok"] == 0


# ------------------------------------------------------------------------------------------------
# 2. sivo_ba_analyze through the library, no device
# ------------------------------------------------------------------------------------------------
def _fixed(n, k=2):
    f = np.zeros(n, np.uint8); f[:k] = 1
    return f


def test_ba_analyze_figures_fill_and_paths():
    """`off-diagonal blocks of L > blocks of S below the diagonal` is asserted so that fill is really covered, and it was meant for
    windowed_scene's loop.  windowed_scene's keyframes stand on a line, the loop ones included (they
    jump back to z = 0.5, 1.5, ...): the poses that share points form an interval graph, which is chordal, and the minimum-degree order
    factors it without fill at every loop length — 269 = 269 blocks at loop = 6, 341 = 341 at 12, 472 = 472 at 24, 192 = 192 at 38
    (48 keyframes, seed 21).  The assertion is therefore made on ba_sparse_cases.ring_scene, where the loop really closes (227 blocks of
    S, 339 of L at 40 keyframes), and that scene is part of the numeric tests on both sides; the line scene's figures are pinned too."""
    from sivo_amd import optimizer
    poses, pts, edges, _ = S.windowed_scene(21, 48, loop=6)
    a = optimizer.ba_analyze(_fixed(48), len(pts), edges)
    assert a == optimizer.ba_analyze(_fixed(48), len(pts), edges)                  # deterministic
    assert (len(pts), len(edges), a["free_poses"], a["s_blocks"] + a["free_poses"]) == (612, 2040, 46, 315)
    assert a["l_blocks"] >= a["s_blocks"] and a["path"] == 1
    poses, pts, edges, _ = S.ring_scene(21, 40)
    r = optimizer.ba_analyze(_fixed(40), len(pts), edges)
    print(f"[ba_analyze] line loop scene {a}; ring scene {r}")
    assert r["l_blocks"] > r["s_blocks"]                                           # fill
    assert r == optimizer.ba_analyze(_fixed(40), len(pts), edges)
    # contribution pairs: sum over the points of k (k + 1) / 2 for k free observers
    k = np.bincount(edges["point"][edges["pose"] >= 2], minlength=len(pts))
    assert r["pairs"] == int((k * (k + 1) // 2).sum())
    poses, pts, edges, _ = S.windowed_scene(21, 96, loop=8)
    b = optimizer.ba_analyze(_fixed(96), len(pts), edges)
    assert (len(pts), len(edges), b["s_blocks"] + b["free_poses"]) == (1164, 4063, 664)
    assert b["nnz_l"] < (6 * 94 * (6 * 94 + 1) // 2) / 3
    assert 1 < b["levels"] <= 94 and b["path"] == 2                                # 94 free keyframes: AUTO goes sparse
    # the path: dense for the 30-keyframe problems of the existing tests, sparse when asked for
    poses, pts, edges, _ = make_ba_scene(seed=12, n_kf=30, n_pts=400)
    assert optimizer.ba_analyze(_fixed(30, 0), len(pts), edges)["path"] == 1       # 30 free poses
    assert optimizer.ba_analyze(_fixed(30, 0), len(pts), edges, solver="sparse")["path"] == 2
    assert optimizer.ba_analyze(_fixed(30, 0), len(pts), edges, solver="dense")["path"] == 1
    with pytest.raises(ValueError):
        optimizer.ba_analyze(_fixed(30), len(pts), edges, solver="cholmod")


def test_ba_analyze_beyond_the_dense_table():
    from sivo_amd import optimizer
    poses, pts, edges, _ = S.track_map(3, 1400, 200000)
    assert len(edges) == 800000 and 1398 * 200000 > 2 ** 28
    a = optimizer.ba_analyze(_fixed(1400), len(pts), edges)
    assert a["path"] == 2 and a["free_poses"] == 1398 and a["pairs"] > 1900000
    assert a["nnz_l"] < (6 * 1398 * (6 * 1398 + 1) // 2) / 100
    with pytest.raises(ValueError, match="too large for the dense"):
        optimizer.ba_analyze(_fixed(1400), len(pts), edges, solver="dense")


@pytest.mark.parametrize("solver", ["auto", "sparse"])
def test_ba_analyze_reports_invalid_arguments(solver):
    from sivo_amd import _lib, optimizer
    poses, pts, edges, _ = S.windowed_scene(5, 12)
    dup = np.concatenate([edges, edges[edges["pose"] == 4][:1]])                   # a free keyframe's observation, twice
    with pytest.raises(ValueError, match="same"):
        optimizer.ba_analyze(_fixed(12), len(pts), dup, solver=solver)
    for field, value in (("point", len(pts)), ("point", -1), ("pose", 12), ("pose", -1)):
        bad = edges.copy()
        bad[field][7] = value
        with pytest.raises(ValueError, match="outside"):
            optimizer.ba_analyze(_fixed(12), len(pts), bad, solver=solver)
    out = np.zeros(8, np.int64)
    L = _lib.lib()
    assert L.sivo_ba_analyze(None, 0, 5, None, 3, None, out.ctypes.data) == _lib.ERR_INVALID_ARGUMENT      # NULL with a non-zero count
    assert L.sivo_ba_analyze(None, 0, 0, None, 0, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert L.sivo_ba_analyze(None, 0, 0, None, 0, None, out.ctypes.data) == _lib.OK and not out[:7].any()


# ------------------------------------------------------------------------------------------------
# 3. the essential-graph plan is what it was
# ------------------------------------------------------------------------------------------------
# (variables, off-diagonal blocks of L, nnz(L), flops, levels, off-diagonal blocks of H) from sivo_essential_graph_analyze of commit afb3566,
# the parent of the change that moved the pattern half of eg_plan into sparse_plan.hpp
EG_PARENT = {
    ((300, 5), 3): (298, 1574, 85470, 4028150, 104, 898),
    ((120, 9), 1): (118, 573, 31381, 1385853, 117, 356),
    ((500, 2), 2): (498, 2551, 138943, 6354677, 209, 1497),
}


@pytest.mark.parametrize("key", sorted(EG_PARENT))
def test_essential_graph_plan_is_unchanged(key):
    from sivo_amd import optimizer
    (n_kf, seed), n_loops = key
    m = E.make_map(n_kf, seed, n_loops=n_loops)
    siw, fixed, vertex, e = E.gather(m)
    assert tuple(optimizer.essential_graph_analyze(fixed, e).values()) == EG_PARENT[key]


# ------------------------------------------------------------------------------------------------
# 4. ABI
# ------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points(tmp_path):
    from sivo_amd import _lib
    h = open(os.path.join(ROOT, "include", "sivo_hip.h")).read()
    assert re.search(r"int sivo_ba_optimize_opts\(double \*poses, const uint8_t \*pose_fixed, int n_poses,[^;]*const SivoBaOptions \*opts\);", h)
    assert re.search(r"int sivo_local_ba_opts\(double \*poses, const uint8_t \*pose_fixed, int n_poses,[^;]*const SivoBaOptions \*opts\);", h)
    assert re.search(r"int sivo_ba_analyze\(const uint8_t \*pose_fixed, int n_poses, int n_points, const SivoEdge \*edges, int64_t n_edges,\s*"
                     r"const SivoBaOptions \*opts, int64_t out\[8\]\);", h)
    for name, value in (("AUTO", 0), ("DENSE", 1), ("SPARSE", 2)):
        assert re.search(rf"#define SIVO_BA_SOLVER_{name} {value}\b", h)
    L = _lib.lib()
    for name in ("sivo_ba_optimize_opts", "sivo_local_ba_opts", "sivo_ba_analyze", "sivo_ba_optimize", "sivo_local_ba"):
        assert hasattr(L, name)
    host_prog.c_layout(tmp_path, "SivoBaOptions", _lib.BaOptions)
    assert C.sizeof(_lib.BaOptions) == 8
