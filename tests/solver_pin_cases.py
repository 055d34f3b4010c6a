"""What tests/test_pin_solvers.py and tests/golden/make_solver_reference.py share: the problems handed to the reference's own
PnPsolver.cc / Sim3Solver.cc (oracle/_ref/ref_pnp, oracle/_ref/ref_sim3: oracle/ref_pnp_driver.cpp, oracle/ref_sim3_driver.cpp), the
parsing of what those print, the Python side of the `run` transcripts, and the fixture files.

The reference's results are "facts": dicts of arrays.  live_facts() runs the reference programs; load_fixture() reads
tests/golden/*_solver_reference.npz, which hold the same facts in reduced form (reduce_facts: the PnP poses as the stored floats and the
doubles as a digest, large inlier-word tables and the later Sim3 transforms only as SHA-256 digests) -- recorded results only.  Every comparison goes through the check_* functions, which
use the full arrays where the facts have them and the digests always, so the live and the fixture leg assert the same things."""
import functools
import hashlib
import io
import os
import subprocess
import zipfile

import numpy as np

import pnp_ransac_restatement as RP
import sim3_ransac_restatement as RS
import test_pnp_ransac_host as HP
import test_gpu_pnp_ransac as GP
import test_gpu_sim3_ransac as GS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")
REFERENCE = os.environ.get("REFERENCE", "/root/reference")      # as oracle/Makefile takes it (`REFERENCE ?=`), with its default
GOLDEN = {"pnp": os.path.join(ROOT, "tests", "golden", "pnp_solver_reference.npz"),
          "sim3": os.path.join(ROOT, "tests", "golden", "sim3_solver_reference.npz")}
QNAN32 = np.uint32(0x7FC00000)
FULL_WORDS = 512             # an inlier-word table of up to this many words is kept in the fixture, a larger one as its digest
SIM3_HEAD = 8                # the transforms of this many leading hypotheses of a Sim3 scene are kept in the fixture beside the digest


def reference_present():
    return os.path.isdir(os.path.join(REFERENCE, "src", "orbslam"))


@functools.lru_cache(maxsize=None)
def reference_program(name):
    """oracle/_ref/<name>, (re)built where the reference's sources are; None where neither they nor a built program are."""
    if reference_present():
        subprocess.run(["make", "-s", "-C", ORACLE, "_ref/ref_pnp", "_ref/ref_sim3"], check=True)
    exe = os.path.join(ORACLE, "_ref", name)
    return exe if os.path.exists(exe) else None


def run_reference(name, args, text):
    r = subprocess.run([reference_program(name)] + [str(a) for a in args], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def canon32(T):
    """float32 array with every NaN the quiet NaN the ABI stores"""
    T = np.array(T, np.float32)
    T.view(np.uint32)[np.isnan(T)] = QNAN32
    return T


def canon64(T):
    T = np.array(T, np.float64)
    T[np.isnan(T)] = np.nan
    return T


def hexrow(words):
    return [float.fromhex(v) for v in words]


# ---------------------------------------------------------------------------------------------------------------------
# PnP: core
# ---------------------------------------------------------------------------------------------------------------------
def pnp_digest(sc):
    return sha(sc["pts"], np.asarray(sc["K"], np.float32), np.asarray(sc["samples"], np.int32), np.int32([sc["min_inliers"], sc["best_in"]]))


def parse_pnp_core(out, n):
    rows = [ln.split() for ln in out.strip().splitlines()]
    words = (n + 63) // 64
    count = np.array([int(w[0]) for w in rows], np.int32)
    Rt = canon64([hexrow(w[1:13]) for w in rows]).reshape(-1, 12)
    bits = np.array([[int(v, 16) for v in w[13:]] for w in rows], np.uint64).reshape(-1, words)
    return count, Rt, bits


def records(count, min_inliers, best_in):
    """The iterations at which iterate() replaces mvbBestInliers (PnPsolver.cc:228-232), from the counts."""
    rec, best = [], best_in
    for h, c in enumerate(count):
        if c >= min_inliers and c > best:
            best = int(c)
            rec.append(h)
    return rec


def pnp_core(sc, run):
    """Every hypothesis of the scene through `run(sets) -> stdout of a core program`, then the refinement set of every record (found
    from the counts that came back): the facts of one PnP scene."""
    n = len(sc["pts"])
    count, Rt, bits = parse_pnp_core(run([list(s) for s in sc["samples"]]), n)
    rec = records(count, sc["min_inliers"], sc["best_in"])
    refined = np.full(len(count), -1, np.int32)
    rRt, rbits = np.zeros((0, 12)), np.zeros((0, bits.shape[1]), np.uint64)
    if rec:
        rc, rRt, rbits = parse_pnp_core(run([list(np.flatnonzero(RP.unpack_bits(bits[h], n))) for h in rec]), n)
        refined[rec] = rc
    facts = {"counts": np.stack([count, refined], 1).astype(np.int16), "T": floats_of(Rt), "refined_T": floats_of(rRt),
             "shas": np.stack([pnp_digest(sc), sha(bits, rbits), sha(Rt, rRt)]),                  # the inputs, the inlier words, the doubles
             "Rt": Rt, "refined_Rt": rRt, "all_words": np.concatenate([bits, rbits])}
    if facts["all_words"].size <= FULL_WORDS:
        facts["words"] = facts["all_words"]
    return facts


def pnp_reference_core(name):
    sc = GP.scene(name)
    return pnp_core(sc, lambda sets: run_reference("ref_pnp", ["core"], HP.core_text(sc["pts"], sc["K"], sets)))


def floats_of(Rt):
    return RP.store_T(Rt[:, :9], Rt[:, 9:]) if len(Rt) else np.zeros((0, 12), np.float32)


def check_pnp(facts, got, sc, doubles=None):
    """got: what sivo_pnp_ransac returns (count, T, inlier_bits, refined, refined_T, refined_bits as the ABI stores them) from the
    restatement, the host build or the device; doubles = (Rt, refined_Rt) where the candidate has them."""
    digest, words_sha, doubles_sha = facts["shas"]
    assert digest.tobytes() == pnp_digest(sc).tobytes(), "the scene generator drifted: the fixture holds another problem"
    count, refined = facts["counts"][:, 0], facts["counts"][:, 1]
    rec = np.flatnonzero(refined >= 0)
    assert np.array_equal(got["count"], count)
    assert np.array_equal(got["refined"], refined)
    assert canon32(got["T"]).tobytes() == facts["T"].tobytes()                                   # the stored floats, NaN positions included
    assert canon32(got["refined_T"])[rec].tobytes() == facts["refined_T"].tobytes()
    if doubles is not None:                                                                      # the doubles mRi / mti hold
        assert sha(canon64(doubles[0]), canon64(doubles[1])).tobytes() == doubles_sha.tobytes()
        if "Rt" in facts:
            assert canon64(doubles[0]).tobytes() == facts["Rt"].tobytes() and canon64(doubles[1]).tobytes() == facts["refined_Rt"].tobytes()
    gb, grb = np.asarray(got["inlier_bits"], np.uint64), np.asarray(got["refined_bits"], np.uint64)[rec]
    assert sha(gb, grb).tobytes() == words_sha.tobytes()
    for key in ("words", "all_words"):
        if key in facts:
            assert np.concatenate([gb, grb]).tobytes() == facts[key].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# Sim3: core
# ---------------------------------------------------------------------------------------------------------------------
def sim3_core_text(sc):
    hx = lambda v: float(v).hex()
    p = sc["pairs"]
    out = [f"{len(p)} {int(sc['fix_scale'])}", " ".join(hx(v) for v in sc["k1"]) + " " + " ".join(hx(v) for v in sc["k2"])]
    out += [" ".join(hx(v) for v in (*q["x1c"], *q["x2c"], q["max_err1"], q["max_err2"])) for q in p]
    out.append(str(len(sc["triples"])))
    out += [" ".join(str(int(i)) for i in t) for t in sc["triples"]]
    return "\n".join(out) + "\n"


def sim3_digest(sc):
    return sha(sc["pairs"], np.asarray(sc["k1"], np.float32), np.asarray(sc["k2"], np.float32), np.asarray(sc["triples"], np.int32),
               np.int32([sc["min_inliers"], int(sc["fix_scale"])]))


def sim3_reference_core(name, fix_scale):
    sc = GS.scene(name, fix_scale)
    n = len(sc["pairs"])
    rows = [ln.split() for ln in run_reference("ref_sim3", ["core"], sim3_core_text(sc)).strip().splitlines()]
    count = np.array([int(w[0]) for w in rows], np.int32)
    T = canon32([hexrow(w[1:14]) for w in rows])
    T12 = canon32([hexrow(w[14:26]) for w in rows])
    T21 = canon32([hexrow(w[26:38]) for w in rows])
    bits = np.array([[int(v, 16) for v in w[38:]] for w in rows], np.uint64).reshape(-1, (n + 63) // 64)
    return {"counts": count.astype(np.int16), "T_head": T[:SIM3_HEAD], "nan_rows": np.flatnonzero(np.isnan(T).any(1)).astype(np.int16),
            "shas": np.stack([sim3_digest(sc), sha(T), sha(T12, T21), sha(bits)]),               # the inputs, R t s, T12 and T21, the inlier words
            "T": T, "T12": T12, "T21": T21, "all_words": bits}


def sim3_scans(count, min_inliers):
    """first_accept / best of the ABI from the counts, by iterate()'s rules (Sim3Solver.cc:186-200): the first count above
    minInliers, the last of the largest counts."""
    first = next((h for h, c in enumerate(count) if c > min_inliers), -1)
    best, best_count = -1, 0
    for h, c in enumerate(count):
        if c >= best_count:
            best, best_count = h, c
    return first, best


def check_sim3(facts, got, sc, t12_t21=None):
    """got: what sivo_sim3_ransac returns (count, T = R t s, inlier_bits, first_accept, best); t12_t21 = the upper three rows of mT12i
    and mT21i where the candidate has them."""
    digest, T_sha, T1221_sha, words_sha = facts["shas"]
    assert digest.tobytes() == sim3_digest(sc).tobytes(), "the scene generator drifted: the fixture holds another problem"
    assert np.array_equal(got["count"], facts["counts"])
    T = canon32(got["T"])
    assert T[:SIM3_HEAD].tobytes() == facts["T_head"].tobytes()
    assert sha(T).tobytes() == T_sha.tobytes()
    assert sha(np.asarray(got["inlier_bits"], np.uint64)).tobytes() == words_sha.tobytes()
    assert (got["first_accept"], got["best"]) == sim3_scans(facts["counts"], sc["min_inliers"])
    if "T" in facts:
        assert T.tobytes() == facts["T"].tobytes() and np.asarray(got["inlier_bits"], np.uint64).tobytes() == facts["all_words"].tobytes()
    if t12_t21 is not None:
        assert sha(canon32(t12_t21[0]), canon32(t12_t21[1])).tobytes() == T1221_sha.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# run transcripts: a list of tuples, ("call", ...) followed by (matrix bytes, inlier string) where a matrix was returned
# ---------------------------------------------------------------------------------------------------------------------
def parse_transcript(out):
    lines, t, pos = out.strip().splitlines(), [], 0
    while pos < len(lines):
        w = lines[pos].split()
        assert w[0] == "call"
        t.append(("call",) + tuple(int(v) for v in w[1:]))
        pos += 1
        if int(w[4]):
            t.append((np.array(hexrow(lines[pos].split()), np.float32).tobytes(), lines[pos + 1]))
            pos += 2
    return t


def run_args(case):
    return ["run", case["max_calls"], case["n_iter"]] + [f for f in ("shared", "keep") if case.get(f)]


def replay(values):
    """value k of a draw list folded into [lo, hi]: the rule of the drivers' RandomInt and of the classes' SetDraw functors"""
    it = iter(values)
    return lambda lo, hi: lo + next(it) % (hi - lo + 1)


def draw_without_replacement(randint, n, k):
    avail, out = list(range(n)), []
    for _ in range(k):
        r = randint(0, len(avail) - 1)
        out.append(avail[r])
        avail[r] = avail[-1]
        avail.pop()
    return out


def round_robin(solvers, call, max_calls, keep=False):
    """Tracking.cc:1293-1310 / LoopClosing.cc:294-313: every live candidate in turn until it said bNoMore (keep: not even then) or was
    called max_calls times.  call(i, solver) -> (bNoMore, lines)"""
    done, calls, t = [False] * len(solvers), [0] * len(solvers), []
    while not all(done):
        for i, s in enumerate(solvers):
            if done[i]:
                continue
            no_more, lines = call(i, s)
            calls[i] += 1
            if (no_more and not keep) or calls[i] >= max_calls:
                done[i] = True
            t += lines
    return t


# ---- PnP ----
def pnp_run_text(case):
    text = f"{len(case['frames'])}\n"
    for fr, par, draws in zip(case["frames"], case["pars"], case["draws"]):
        text += HP.frame_text(fr) + f"{par[0]} {par[1]} {par[2]} {par[3]} {par[4]} {len(draws)} " + " ".join(str(d) for d in draws) + "\n"
    return text


def pnp_reference_run(case):
    return run_reference("ref_pnp", run_args(case), pnp_run_text(case))


def _pnp_call(n_iter):
    def call(i, s):
        if n_iter > 0:
            T, no_more, inl, n = s.iterate(n_iter)
        else:
            (T, inl, n), no_more = s.find(), True
        lines = [("call", i, int(no_more), int(n), int(T is not None), int(s.max_its), int(s.min_inliers))]
        if T is not None:
            lines.append((np.asarray(T, np.float32).tobytes(), "".join("1" if b else "0" for b in inl)))
        return no_more, lines
    return call


def pnp_python_run(case, eager=False):
    """The transcript of the Python side under the case's draws, and what happened inside (trace per candidate: the counts in
    order, (count of the best, refined count) of every Refine, the samples).  eager=False: tests/pnp_ransac_restatement.py
    Sequential, drawing each sample when its iteration runs as the reference does; eager=True: sivo_amd.pnp_solver.PnPsolver with the
    restatement in the place of the device, which draws all mRansacMaxIts samples when first evaluated."""
    solvers, traces = [], []
    shared = replay(case["draws"][0]) if case.get("shared") else None
    for fr, par, draws in zip(case["frames"], case["pars"], case["draws"]):
        pts, idx, sig2 = RP.gather(fr, th2=par[4])
        randint = shared or replay(draws)
        trace = {"counts": [], "refines": [], "samples": []}
        traces.append(trace)
        if eager:
            from sivo_amd import pnp_solver

            def evaluate(p, trace=trace):
                trace["samples"] += [list(s) for s in p["samples"]]
                return RP.pnp_ransac(p["points"], p["K"], p["samples"], p["min_inliers"], p["best_in"])
            s = pnp_solver.PnPsolver(pts["xw"], np.stack([pts["u"], pts["v"]], 1), sig2, fr["K"], indices=idx, n_matches=len(fr["matches"]),
                                     randint=randint, evaluate=evaluate)
            s.set_ransac_parameters(par[0], par[1], par[2], 4, par[3], par[4])
        else:
            N = len(pts)
            n_min, max_its, _ = RP.ransac_iterations(N, par[0], par[1], par[2], 4, par[3])

            def evaluate(h, pts=pts, K=fr["K"], N=N, randint=randint, trace=trace):
                sample = draw_without_replacement(randint, N, 4)
                c, T, b = RP.evaluate(pts, K, [sample])
                trace["samples"].append(sample)
                trace["counts"].append(int(c[0]))
                return int(c[0]), T[0], RP.unpack_bits(b[0], N)

            def refine(bits, pts=pts, K=fr["K"], N=N, trace=trace):
                c, T, b = RP.evaluate(pts, K, np.flatnonzero(bits)[None, :])
                trace["refines"].append((int(np.sum(bits)), int(c[0])))
                return int(c[0]), T[0], RP.unpack_bits(b[0], N)
            s = RP.Sequential(N, n_min, max_its, evaluate, refine, indices=idx, n_matches=len(fr["matches"]))
        solvers.append(s)
    if eager:
        from sivo_amd import pnp_solver
        pnp_solver.PnPsolver.solve_all(solvers + [None])
    return round_robin(solvers, _pnp_call(case["n_iter"]), case["max_calls"], case.get("keep", False)), traces, solvers


def _draws(seed, n):
    return np.random.RandomState(seed).randint(0, 1 << 20, n).tolist()


@functools.lru_cache(maxsize=None)
def pnp_run_case(name):
    """frames, per frame (probability, minInliers, maxIterations, epsilon, th2) and its draw list, the calls each candidate gets at
    most, the iterations asked per call (0: find()).  `plain`: a case tests/pnp_ransac_prog.cpp can run (iterate(5), a list per
    candidate, discarded at bNoMore), so SIVO::PnPsolver is held against its transcript on the GPU."""
    std = (0.99, 10, 300, 0.5, 5.991)
    if name == "round_robin":       # the three candidates of tests/test_gpu_pnp_ransac.py: accepting ones and an all-outlier one cut to 3 iterations
        return {"frames": [HP.make_frame(31, 40), HP.make_frame(32, 36, outliers=1.0), HP.make_frame(33, 50, outliers=0.4)],
                "pars": [std, (0.99, 10, 3, 0.5, 5.991), std], "draws": [_draws(50 + k, 4000) for k in range(3)], "max_calls": 12, "n_iter": 5, "plain": True}
    if name == "accept_first":      # one call: it returns at the first iteration whose count reaches minInliers and whose refinement is above it
        return {"frames": [HP.make_frame(31, 40)], "pars": [std], "draws": [_draws(50, 4000)], "max_calls": 1, "n_iter": 5, "plain": True}
    if name == "equal_min":         # 18 true inliers of 30 and minInliers = 18: counts equal to it, refined counts equal to it
        return {"frames": [HP.make_frame(50, 30, outliers=0.4)], "pars": [(0.99, 18, 300, 0.4, 5.991)], "draws": [_draws(1050, 4000)], "max_calls": 12,
                "n_iter": 5, "plain": True}
    if name == "too_few":           # N = 6 < minInliers
        return {"frames": [HP.make_frame(61, 6, n_extra=4, outliers=0.0)], "pars": [std], "draws": [_draws(61, 100)], "max_calls": 3, "n_iter": 5, "plain": True}
    if name == "find":
        return {"frames": [HP.make_frame(31, 40), HP.make_frame(32, 36, outliers=1.0)], "pars": [std, (0.99, 10, 7, 0.5, 5.991)],
                "draws": [_draws(70 + k, 4000) for k in range(2)], "max_calls": 1, "n_iter": 0}
    if name == "past_max":          # all outliers, 3 iterations at most, called three times whatever it says
        return {"frames": [HP.make_frame(32, 36, outliers=1.0)], "pars": [(0.99, 10, 3, 0.5, 5.991)], "draws": [_draws(80, 4000)], "max_calls": 3, "n_iter": 5,
                "keep": True}
    if name == "shared":            # two candidates on ONE stream
        return {"frames": [HP.make_frame(31, 40), HP.make_frame(33, 50, outliers=0.4)], "pars": [std, std], "draws": [_draws(90, 8000), []], "max_calls": 4,
                "n_iter": 5, "shared": True}
    raise KeyError(name)


PNP_RUN_CASES = ("round_robin", "accept_first", "equal_min", "too_few", "find", "past_max", "shared")


# ---- Sim3 ----
def sim3_candidate(name, fix_scale, seed):
    sc = GS.scene(name, fix_scale)
    kf1, kf2, pts, m12 = RS.keyframe_pair(sc, seed, random_pose=True, n_extra=14)
    return {"sc": sc, "kf1": kf1, "kf2": kf2, "points": pts, "matched12": m12, "fix_scale": fix_scale}


@functools.lru_cache(maxsize=None)
def sim3_run_case(name):
    """candidates, per candidate (probability, minInliers, maxIterations) and its draw list; the rest as pnp_run_case."""
    draws = lambda seed, n: np.random.default_rng(seed).integers(0, 1 << 20, n).tolist()
    if name == "round_robin":       # the three candidates of tests/test_gpu_sim3_ransac.py
        pars = [(0.99, 20, 300), (0.99, 100, 40), (0.99, 20, 23)]
        return {"cands": [sim3_candidate(n, f, 900 + k) for k, (n, f) in enumerate((("word_65", True), ("outliers30", False), ("all_outliers", True)))],
                "pars": pars, "draws": [draws(77 + k, 3 * p[2]) for k, p in enumerate(pars)], "max_calls": 10 ** 6, "n_iter": 5, "plain": True}
    if name == "equal_min":         # 140 true inliers of 200, no noise, and minInliers = 140: counts equal to it are not above it
        return {"cands": [sim3_candidate("outliers30", True, 910)], "pars": [(0.99, 140, 300)], "draws": [draws(91, 900)], "max_calls": 10 ** 6, "n_iter": 5,
                "plain": True}
    if name == "too_few":           # N = 20 < minInliers
        return {"cands": [sim3_candidate("min_inliers_is_n", True, 920)], "pars": [(0.99, 25, 300)], "draws": [draws(92, 30)], "max_calls": 10 ** 6, "n_iter": 5,
                "plain": True}
    if name == "find":
        return {"cands": [sim3_candidate("word_64", False, 930), sim3_candidate("all_outliers", False, 931)], "pars": [(0.99, 20, 300), (0.99, 20, 9)],
                "draws": [draws(93, 900), draws(94, 27)], "max_calls": 1, "n_iter": 0}
    if name == "stops":             # all outliers, 23 iterations at most, called seven times whatever it says
        return {"cands": [sim3_candidate("all_outliers", True, 940)], "pars": [(0.99, 20, 23)], "draws": [draws(95, 200)], "max_calls": 7, "n_iter": 5, "keep": True}
    if name == "shared":            # two candidates on ONE stream
        return {"cands": [sim3_candidate("word_65", True, 950), sim3_candidate("outliers30_noisy", False, 951)], "pars": [(0.99, 20, 300), (0.99, 20, 300)],
                "draws": [draws(96, 4000), []], "max_calls": 4, "n_iter": 5, "shared": True}
    raise KeyError(name)


SIM3_RUN_CASES = ("round_robin", "equal_min", "too_few", "find", "stops", "shared")


def sim3_run_text(case):
    text = [str(len(case["cands"]))]
    for c, par, draws in zip(case["cands"], case["pars"], case["draws"]):
        text.append(RS.scene_text(c["sc"], c["kf1"], c["kf2"], c["points"], c["matched12"], c["fix_scale"]) +
                    f"{par[0]!r} {par[1]} {par[2]} {len(draws)} " + " ".join(map(str, draws)))
    return "\n".join(text) + "\n"


def sim3_reference_run(case):
    return run_reference("ref_sim3", run_args(case), sim3_run_text(case))


def _sim3_call(n_iter):
    def call(i, s):
        if n_iter > 0:
            T, no_more, inl, n = s.iterate(n_iter)
        else:
            (T, inl, n), no_more = s.find(), True
        lines = [("call", i, int(no_more), int(n), int(T is not None), int(s.max_its))]
        if T is not None:
            m = np.concatenate([T.reshape(-1), s.estimated_rotation().reshape(-1), s.estimated_translation(), [s.estimated_scale()]])
            lines.append((m.astype(np.float32).tobytes(), "".join("1" if b else "0" for b in inl)))
        return no_more, lines
    return call


class LazySim3:
    """Sim3Solver::iterate / find as tests/sim3_ransac_restatement.py Sequential states them, drawing each triple when its iteration
    runs (the reference's order of consuming the stream) and evaluating it with the restatement."""

    def __init__(self, recs, k1, k2, fix_scale, idx, n_matches, randint, par):
        self.recs, self.k1, self.k2, self.fix, self.idx, self.n_matches = recs, k1, k2, fix_scale, idx, n_matches
        self.hyp, self.counts, self.triples = {}, [], []

        def evaluate(h):
            tri = draw_without_replacement(randint, len(recs), 3)
            r = RS.ransac(recs, k1, k2, [tri], par[1], fix_scale)
            self.hyp[h] = r
            self.counts.append(int(r["count"][0]))
            self.triples.append(tri)
            return int(r["count"][0]), h
        self.seq = RS.Sequential(len(recs), evaluate, *par)
        self.max_its = self.seq.max_its

    def iterate(self, n):
        h, no_more, count = self.seq.iterate(n)
        inl = np.zeros(self.n_matches, bool)
        if h is None:
            return None, no_more, inl, 0
        r = self.hyp[h]
        inl[self.idx[r["inliers"][0]]] = True
        T = r["T"][0]
        T12 = np.eye(4, dtype=np.float32)
        with np.errstate(all="ignore"):
            T12[:3, :3] = T[:9].reshape(3, 3) * T[12]
        T12[:3, 3] = T[9:12]
        return T12, no_more, inl, count

    def find(self):
        T, _, inl, n = self.iterate(self.max_its)
        return T, inl, n

    def _best(self):
        return self.hyp[self.seq.best]["T"][0]

    def estimated_rotation(self):
        return self._best()[:9].reshape(3, 3)

    def estimated_translation(self):
        return self._best()[9:12]

    def estimated_scale(self):
        return self._best()[12]


def sim3_python_run(case, eager=False):
    """eager=False: LazySim3; eager=True: sivo_amd.sim3_solver.Sim3Solver with the restatement's result in the place of the
    device's (all mRansacMaxIts triples drawn before the first call)."""
    solvers = []
    shared = replay(case["draws"][0]) if case.get("shared") else None
    for c, par, draws in zip(case["cands"], case["pars"], case["draws"]):
        sc = c["sc"]
        idx, recs = RS.gather(c["kf1"], c["kf2"], c["matched12"], c["points"])
        randint = shared or replay(draws)
        if eager:
            from sivo_amd import sim3_solver
            s = sim3_solver.Sim3Solver(recs, sc["k1"], sc["k2"], c["fix_scale"], indices1=idx, n_matches=len(c["matched12"]), randint=randint)
            s.set_ransac_parameters(*par)
            if s._can_run():
                s.triples = s.draw_triples()
                s.result = RS.ransac(recs, sc["k1"], sc["k2"], s.triples, s.min_inliers, c["fix_scale"])
        else:
            s = LazySim3(recs, sc["k1"], sc["k2"], c["fix_scale"], idx, len(c["matched12"]), randint, par)
        solvers.append(s)
    return round_robin(solvers, _sim3_call(case["n_iter"]), case["max_calls"], case.get("keep", False)), solvers


# ---------------------------------------------------------------------------------------------------------------------
# the fixture files
# ---------------------------------------------------------------------------------------------------------------------
def reduce_facts(facts):
    """What of a scene's facts the fixture keeps."""
    keep = ("counts", "T_head", "nan_rows", "shas") if "T_head" in facts else ("counts", "T", "refined_T", "shas", "words")
    return {k: facts[k] for k in keep if k in facts}


def write_fixture(path, entries):
    """entries: name -> dict of arrays / str.  One uncompressed zip of .npy members with a fixed date: the same bytes for the same
    results on every machine (np.load reads it as an .npz)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name in sorted(entries):
            for key in sorted(entries[name]):
                v = entries[name][key]
                a = np.frombuffer(v.encode(), np.uint8) if isinstance(v, str) else np.ascontiguousarray(v)
                buf = io.BytesIO()
                np.lib.format.write_array(buf, a, version=(1, 0), allow_pickle=False)
                info = zipfile.ZipInfo(f"{name}|{key}.npy", date_time=(1980, 1, 1, 0, 0, 0))
                info.external_attr = 0o644 << 16
                z.writestr(info, buf.getvalue())


@functools.lru_cache(maxsize=None)
def load_fixture(which):
    entries = {}
    with np.load(GOLDEN[which], allow_pickle=False) as z:
        for member in z.files:
            name, key = member.split("|")
            entries.setdefault(name, {})[key] = z[member]
    return entries


def text_of(a):
    return a if isinstance(a, str) else bytes(np.asarray(a, np.uint8)).decode()


# ---------------------------------------------------------------------------------------------------------------------
# gather and SetRansacParameters problems, and everything the reference says as fixture entries
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pnp_gather_frames():
    """frames with null entries and bad map points among the matches, keys on all eight octaves"""
    return [HP.make_frame(8, 30), HP.make_frame(9, 45, n_extra=16, outliers=0.3)]


@functools.lru_cache(maxsize=None)
def sim3_gather_candidates():
    """keyframe pairs with null matches, bad points on either side, no own point in KF1, and points missing in either keyframe"""
    out = []
    for n, seed, scale, random_pose in ((30, 8, 1.0, True), (25, 10, 1.2, False)):
        sc = RS.make_scene(n, seed, scale=scale)
        kf1, kf2, pts, m12 = RS.keyframe_pair(sc, seed + 1, random_pose=random_pose, n_extra=18)
        out.append({"sc": sc, "kf1": kf1, "kf2": kf2, "points": pts, "matched12": m12, "fix_scale": True})
    return out


def parse_gather(out):
    rows = [ln.split() for ln in out.strip().splitlines()]
    return np.array([[int(w[0]), int(w[1])] for w in rows], np.int64), np.array([hexrow(w[2:]) for w in rows], np.float32)


PNP_GRID = [(N, p, m, its, ms, eps) for N in (4, 10, 25, 100) for p in (0.9, 0.99) for m in (4, 10, 25, 50) for its in (5, 300) for ms in (4, 12)
            for eps in (0.1, 0.5, 0.9)]
SIM3_GRID = [(N, p, m, its) for N in (3, 20, 25, 100, 2000) for p in (0.9, 0.99, 0.999) for m in (3, 6, 20, 25, 100) for its in (1, 5, 300)]


def live_entries(which):
    """Everything tests/test_pin_solvers.py asks of the reference, computed by the reference programs: name -> facts."""
    e = {}
    if which == "pnp":
        for name in GP.SCENES:
            e[f"core.{name}"] = pnp_reference_core(name)
        for name in PNP_RUN_CASES:
            e[f"run.{name}"] = {"transcript": pnp_reference_run(pnp_run_case(name))}
        frames = pnp_gather_frames()
        idx, vals = parse_gather(run_reference("ref_pnp", ["gather"], f"{len(frames)}\n" + "".join(HP.frame_text(f) for f in frames)))
        e["gather"] = {"index": idx, "values": vals}
        rows = run_reference("ref_pnp", ["params"], "".join(f"{N} {p!r} {m} {its} {ms} {eps!r}\n" for N, p, m, its, ms, eps in PNP_GRID)).split()
        e["params"] = {"grid": sha(np.array(PNP_GRID, np.float64)),                              # mRansacMinInliers, mRansacMaxIts, mRansacEpsilon (float)
                       "values": np.stack([np.array(rows[0::3], np.float32), np.array(rows[1::3], np.float32), np.array(hexrow(rows[2::3]), np.float32)], 1)}
    else:
        for name in GS.SCENES:
            for fix in (True, False):
                e[f"core.{name}.{'fix' if fix else 'free'}"] = sim3_reference_core(name, fix)
        for name in SIM3_RUN_CASES:
            e[f"run.{name}"] = {"transcript": sim3_reference_run(sim3_run_case(name))}
        cands = sim3_gather_candidates()
        text = f"{len(cands)}\n" + "".join(RS.scene_text(c["sc"], c["kf1"], c["kf2"], c["points"], c["matched12"], True) for c in cands)
        idx, vals = parse_gather(run_reference("ref_sim3", ["gather"], text))
        e["gather"] = {"index": idx, "values": vals}
        rows = run_reference("ref_sim3", ["params"], "".join(f"{N} {p!r} {m} {its}\n" for N, p, m, its in SIM3_GRID)).split()
        e["params"] = {"grid": sha(np.array(SIM3_GRID, np.float64)), "values": np.array(rows, np.int16)}
    return e


def fixture_entries(which):
    """live_entries in the form the fixture file keeps"""
    return {k: (reduce_facts(v) if k.startswith("core.") else v) for k, v in live_entries(which).items()}


@functools.lru_cache(maxsize=None)
def reference_entries(which):
    """(entries, live): from the reference programs where they are, from the fixture otherwise"""
    if reference_program("ref_pnp" if which == "pnp" else "ref_sim3"):
        return live_entries(which), True
    return load_fixture(which), False
