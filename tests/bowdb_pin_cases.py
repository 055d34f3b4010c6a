"""The scripts tests/test_pin_bow_database.py replays on the reference's own KeyFrameDatabase.cc (oracle/_ref/ref_kfdb), on the restatement
(tests/bow_restatement.py), on the host path and on the device: add / erase / clear / DetectLoopCandidates / DetectRelocalizationCandidates
over keyframes whose BowVectors come from descriptors (the vocabulary transforms them) or are given as they are.  Also the one form every
replay is brought into (a Trace), the script file the C++ programs read, the text they write, and the packing of a Trace into the arrays
of tests/golden/bowdb_reference.npz.  Data only goes into the fixture; nothing of the reference's text is here."""
import hashlib

import numpy as np

import bow_restatement as BR
import test_gpu_bow as G

ADD, ERASE, LOOP, RELOC, CLEAR = range(5)
F = np.float32
ORDERS = ("asc", "desc", "mixed")          # where oracle/ref_kfdb_driver.cpp puts the keyframes: address order = id order, reversed, neither


class Script:
    """kfs / frames: ("desc", N x 32 uint8) or ("vec", (words, values)).  connected / ordered: per keyframe, ids."""

    def __init__(self, voc, levelsup, kfs, connected, ordered, frames, ops):
        self.voc, self.levelsup, self.kfs, self.connected, self.ordered, self.frames, self.ops = voc, levelsup, kfs, connected, ordered, frames, ops

    def vectors(self):
        """(words, values) of every keyframe, then of every frame: the restatement's transform where descriptors were given."""
        out = []
        for kind, x in self.kfs + self.frames:
            if kind == "desc":
                t = BR.transform(self.voc, x, self.levelsup)
                out.append((t["words"], t["values"]))
            else:
                out.append((np.asarray(x[0], np.int32), np.asarray(x[1], np.float64)))
        return out

    def to_bytes(self):
        i64 = lambda *a: np.array(a, np.int64).tobytes()

        def source(kind, x):
            if kind == "desc":
                return i64(0, len(x)) + np.ascontiguousarray(x, np.uint8).tobytes()
            return i64(1, len(x[0])) + np.asarray(x[0], np.int32).tobytes() + np.asarray(x[1], np.float64).tobytes()

        blob = [i64(self.levelsup, len(self.kfs))]
        for i, s in enumerate(self.kfs):
            blob += [source(*s), i64(len(self.connected[i]), *self.connected[i]), i64(len(self.ordered[i]), *self.ordered[i])]
        blob += [i64(len(self.frames))] + [source(*s) for s in self.frames] + [i64(len(self.ops))]
        blob += [i64(op, idx) + np.array([ms], np.float64).tobytes() for op, idx, ms in self.ops]
        return b"".join(blob)

    def digest(self):
        return np.frombuffer(hashlib.sha256(self.voc.text().encode() + self.to_bytes()).digest(), np.uint8)


class Trace:
    """What a replay leaves: cands[o] = the ids a detection returned, in order; ints[o, kf] = mnLoopQuery, mnLoopWords, mnRelocQuery,
    mnRelocWords and scores[o, kf] = mLoopScore, mRelocScore (float32) after operation o."""

    def __init__(self, n_ops, n_kf):
        self.cands = {}
        self.ints = np.zeros((n_ops, n_kf, 4), np.int64)
        self.scores = np.zeros((n_ops, n_kf, 2), np.float32)

    def differences(self, other):
        """Empty when equal byte for byte; else the first few places that differ, for the assertion message."""
        out = []
        if self.ints.shape != other.ints.shape:
            return [("shape", self.ints.shape, other.ints.shape)]
        for o in sorted(set(self.cands) | set(other.cands)):
            if self.cands.get(o) != other.cands.get(o):
                out.append(("candidates", o, self.cands.get(o), other.cands.get(o)))
        bad = np.argwhere((self.ints != other.ints).any(-1) | (self.scores.view(np.uint32) != other.scores.view(np.uint32)).any(-1))
        for o, k in bad[:5]:
            out.append(("fields", int(o), int(k), self.ints[o, k].tolist(), self.scores[o, k].tolist(), other.ints[o, k].tolist(), other.scores[o, k].tolist()))
        return out[:8]

    # the fixture holds the CHANGES from one operation to the next (all of them: nothing is left to a digest)
    def pack(self, prefix):
        prev_i = np.concatenate([np.zeros_like(self.ints[:1]), self.ints[:-1]])
        prev_s = np.concatenate([np.zeros_like(self.scores[:1]), self.scores[:-1]])
        at = np.argwhere((self.ints != prev_i).any(-1) | (self.scores.view(np.uint32) != prev_s.view(np.uint32)).any(-1))
        ops = sorted(self.cands)
        return {prefix + "shape": np.array(self.ints.shape[:2], np.int64), prefix + "at": at.astype(np.int32),
                prefix + "ints": self.ints[at[:, 0], at[:, 1]], prefix + "scores": self.scores[at[:, 0], at[:, 1]],
                prefix + "cand_op": np.array(ops, np.int32), prefix + "cand_n": np.array([len(self.cands[o]) for o in ops], np.int32),
                prefix + "cand_id": np.array([i for o in ops for i in self.cands[o]], np.int32)}

    @classmethod
    def unpack(cls, fx, prefix):
        n_ops, n_kf = fx[prefix + "shape"].tolist()
        t = cls(n_ops, n_kf)
        at = fx[prefix + "at"]
        for o in range(n_ops):
            if o:
                t.ints[o], t.scores[o] = t.ints[o - 1], t.scores[o - 1]
            rows = np.flatnonzero(at[:, 0] == o)
            t.ints[o, at[rows, 1]] = fx[prefix + "ints"][rows]
            t.scores[o, at[rows, 1]] = fx[prefix + "scores"][rows]
        ids, pos = fx[prefix + "cand_id"].tolist(), 0
        for o, n in zip(fx[prefix + "cand_op"].tolist(), fx[prefix + "cand_n"].tolist()):
            t.cands[o] = ids[pos:pos + n]
            pos += n
        return t


def parse_output(text, script):
    """The text of oracle/ref_kfdb_driver.cpp and of `bow_adapter_prog ... pin` -> (Trace, the BowVectors the program held)."""
    n_kf = len(script.kfs)
    t, bows, o = Trace(len(script.ops), n_kf), {}, -1
    seen = np.zeros((len(script.ops), n_kf), bool)
    for line in text.splitlines():
        f = line.split()
        if f[0] == "S":
            o = int(f[1])
        elif f[0] == "Q":
            assert int(f[1]) == o and int(f[2]) == len(f) - 3
            t.cands[o] = [int(x) for x in f[3:]]
        elif f[0] == "K":
            k = int(f[1])
            t.ints[o, k] = [int(x) for x in f[2:6]]
            t.scores[o, k] = [F(float.fromhex(f[6])), F(float.fromhex(f[7]))]
            assert float(t.scores[o, k, 0]) == float.fromhex(f[6]) and float(t.scores[o, k, 1]) == float.fromhex(f[7])      # floats were printed
            seen[o, k] = True
        elif f[0] in ("B", "F"):
            pairs = [p.split(":") for p in f[3:]]
            bows[(f[0], int(f[1]))] = (np.array([int(p[0]) for p in pairs], np.int32), np.array([float.fromhex(p[1]) for p in pairs], np.float64))
    assert seen.all()
    return t, [bows[("B", i)] for i in range(n_kf)] + [bows[("F", i)] for i in range(len(script.frames))]


def restate(script):
    """The script on tests/bow_restatement.py's Database."""
    n_kf = len(script.kfs)
    vec = script.vectors()
    K = [BR.KF(i, *vec[i]) for i in range(n_kf)]
    for i in range(n_kf):
        K[i].connected, K[i].best_cov = {K[j] for j in script.connected[i]}, [K[j] for j in script.ordered[i]][:10]
    Fr = [BR.KF(1000 + i, *vec[n_kf + i]) for i in range(len(script.frames))]
    db, t = BR.Database(), Trace(len(script.ops), n_kf)
    for o, (op, idx, ms) in enumerate(script.ops):
        if op == ADD:
            db.add(K[idx])
        elif op == ERASE:
            db.erase(K[idx])
        elif op == CLEAR:
            db.clear()
        elif op == LOOP:
            t.cands[o] = [k.mnId for k in db.detect_loop(K[idx], ms)]
        else:
            t.cands[o] = [k.mnId for k in db.detect_reloc(Fr[idx])]
        for k in K:
            t.ints[o, k.mnId] = [k.mnLoopQuery, k.mnLoopWords, k.mnRelocQuery, k.mnRelocWords]
            t.scores[o, k.mnId] = [k.mLoopScore, k.mRelocScore]
    return t, vec


# ---------------------------------------------------------------------------------------------------------------------
# the scripts
# ---------------------------------------------------------------------------------------------------------------------
def _from_adapter_scene(scene):
    v, kfs, connected, ordered, frames, ops = scene
    return Script(v, G.LEVELSUP, [("desc", d) for d in kfs], connected, ordered, [("desc", d) for d in frames], list(ops))


def _plain(v, vectors, frames, ops, connected=None, ordered=None):
    none = [[] for _ in vectors]
    return Script(v, 0, [("vec", e) for e in vectors], connected or none, ordered or none, [("vec", e) for e in frames], ops)


def _gpu_query(n):
    """tests/test_gpu_bow.py::test_query_equals_the_restatement_bit_for_bit: its stored vectors as keyframes, its query as one more
    keyframe (never added) and as a frame."""
    rng = np.random.default_rng(n)
    stored = G.db_vectors(n)
    q = BR.random_vector(rng, G.N_WORDS, 180)
    other = np.setdiff1d(np.arange(G.N_WORDS, dtype=np.int32), q[0])
    stored += [(other[:150], BR.random_vector(rng, G.N_WORDS, 150)[1]),
               (np.sort(np.append(other[:99], q[0][17])).astype(np.int32), BR.random_vector(rng, G.N_WORDS, 100)[1]),
               (q[0], BR.random_vector(rng, G.N_WORDS, 180)[1]), q, (np.zeros(0, np.int32), np.zeros(0))]
    m = len(stored)
    ops = [(ADD, i, 0.0) for i in range(m)] + [(LOOP, m, 0.0), (RELOC, 0, 0.0)]
    return _plain(BR.voc("k10L3_dfs"), stored + [q], [q], ops)


def _gpu_erase():
    """tests/test_gpu_bow.py::test_erase_then_query_and_clear_then_add; every query is a keyframe of its own with the vector of keyframe 11."""
    stored, fresh = G.db_vectors(70, seed=9), G.db_vectors(3, seed=10)
    q = stored[11]
    vectors = stored + fresh + [q] * 4                                  # 70 .. 72 fresh; 73 .. 76 queries
    ops = [(ADD, i, 0.0) for i in range(70)] + [(ERASE, 11, 0.0), (ERASE, 64, 0.0), (ERASE, 69, 0.0), (LOOP, 73, 0.0), (ERASE, 11, 0.0), (ADD, 11, 0.0),
                                                (LOOP, 74, 0.0), (RELOC, 0, 0.0), (CLEAR, 0, 0.0), (LOOP, 75, 0.0), (RELOC, 1, 0.0)]
    ops += [(ADD, i, 0.0) for i in (70, 71, 72)] + [(LOOP, 76, 0.0), (RELOC, 2, 0.0)]
    return _plain(BR.voc("k10L3_dfs"), vectors, [q, q, q], ops)


_big = {}


def big_voc():
    """5832 words (k = 18, L = 3): room for the 5000-word vectors of tests/test_bow_host.py."""
    if "v" not in _big:
        _big["v"] = BR.make_voc(18, 3, 17)
    return _big["v"]


def _host_query():
    """tests/test_bow_host.py::check_host's query: 70 stored vectors over 5000 words, the query as a keyframe and as a frame."""
    rng = np.random.default_rng(3)
    q = BR.random_vector(rng, 5000, 200)
    other = np.setdiff1d(np.arange(5000, dtype=np.int32), q[0])
    stored = [BR.random_vector(rng, 5000, int(n)) for n in rng.integers(1, 400, 65)]
    stored += [(other[:150], BR.random_vector(rng, 5000, 150)[1]), (np.sort(np.append(other[:99], q[0][17])).astype(np.int32), BR.random_vector(rng, 5000, 100)[1]),
               (q[0], BR.random_vector(rng, 5000, 200)[1]), q, (np.zeros(0, np.int32), np.zeros(0))]
    m = len(stored)
    return _plain(big_voc(), stored + [q], [q], [(ADD, i, 0.0) for i in range(m)] + [(LOOP, m, 0.0), (RELOC, 0, 0.0)])


def _near_uniform(words, seed):
    """Values close to 1 / n each (so that every keyframe survives the 0.75 cut), distinct per seed."""
    rng = np.random.default_rng(seed)
    v = 1.0 + 0.01 * rng.random(len(words))
    s = 0.0
    for x in v:
        s += x
    return np.array(sorted(words), np.int32), v / s


def _ids():
    """Query ids and the life of a keyframe in the inverted file.  U: ten words every keyframe below is built from.
    Keyframes 1 .. 4 share word 100 with every query, so the order of the returned vector is the order of the list of word 100."""
    U = list(range(100, 110))
    vec = {0: U, 1: U, 2: U[:9] + [200], 3: U[:9] + [201], 4: U[:9] + [203], 5: [400, 401], 7: U[:9] + [204]}
    for qid in (6, 8, 9, 10, 11, 12, 13, 14):
        vec[qid] = U
    vectors = [_near_uniform(vec[i], 50 + i) for i in range(15)]
    frames = [_near_uniform(U, 70), _near_uniform(U, 71)]
    ops = [(ADD, 3, 0.0), (ADD, 1, 0.0), (ADD, 2, 0.0),                  # add order is not the id order
           (LOOP, 0, 0.0),                                               # mnId == 0 against fresh keyframes: their mnLoopQuery is 0 already
           (LOOP, 6, 0.0), (LOOP, 6, 0.0),                               # an id used twice
           (RELOC, 0, 0.0), (RELOC, 0, 0.0),
           (LOOP, 0, 0.0),                                               # id 0 once the keyframes carry another id
           (ERASE, 1, 0.0), (LOOP, 8, 0.0), (ADD, 1, 0.0), (LOOP, 9, 0.0),         # erased and added again: now the last of its lists
           (ADD, 4, 0.0), (ADD, 2, 0.0), (LOOP, 10, 0.0),                # added twice: every word counts twice
           (ERASE, 2, 0.0), (LOOP, 11, 0.0), (RELOC, 1, 0.0),            # erased once: the FIRST entry of each list goes
           (ERASE, 7, 0.0), (LOOP, 12, 0.0),                             # never added
           (CLEAR, 0, 0.0), (LOOP, 13, 0.0), (RELOC, 0, 0.0),            # nothing stored
           (ADD, 5, 0.0), (ADD, 1, 0.0), (LOOP, 14, 0.0)]
    return _plain(BR.voc("k10L3_dfs"), vectors, frames, ops)


def _cuts():
    """The minCommonWords cut at maximum counts 10 and 5 (int(10 * 0.8f) = 8, int(5 * 0.8f) = 4: counts 8 and 4 fall, 9 and 5 stay), connected
    keyframes that share every word, and minScore equal to a candidate's score."""
    U, V = list(range(100, 110)), list(range(500, 505))
    vec = [[700],                                                        # 0: never used (a query with mnId 0 is blind to fresh keyframes: script ids)
           U, U[:9] + [200],                                             # 1, 2: connected to the query 13, share 10 and 9 words
           U, U[:9] + [201], U[:8] + [202, 203], U[:1] + [204],          # 3 .. 6: share 10, 9, 8, 1
           V,                                                            # 7: query over V
           V, V[:4] + [600], V[1:],                                      # 8 .. 10: share 5, 4, 4 (one of them without the smallest word)
           U, U,                                                         # 11, 12: queries over U with minScore at a candidate's score
           U]                                                            # 13: query over U, connected to 1 and 2
    vectors = [_near_uniform(w, 150 + i) for i, w in enumerate(vec)]
    connected = [[] for _ in vec]
    connected[13] = [1, 2]
    q11 = vectors[11]
    at_4 = float(F(BR.score(q11[0], q11[1], *vectors[4])))               # DetectLoopCandidates(11, score of keyframe 4): kept by >=
    q12 = vectors[12]
    s = sorted(float(F(BR.score(q12[0], q12[1], *vectors[i]))) for i in (1, 2, 3, 4))
    assert len(set(s)) == 4
    ops = [(ADD, i, 0.0) for i in (5, 3, 6, 1, 4, 2, 10, 8, 9)] + [(LOOP, 13, 0.0), (LOOP, 7, 0.0), (LOOP, 11, at_4), (LOOP, 12, s[-1]),
                                                                  (RELOC, 0, 0.0), (RELOC, 1, 0.0)]
    return _plain(BR.voc("k10L3_dfs"), vectors, [_near_uniform(U, 170), _near_uniform(V, 171)], ops, connected=connected)


def _groups():
    """Exact scores (values that are multiples of 1/16: every term and sum below is exact in double and in float).
    W: the query 10 holds four words at 0.25 (keyframe 0 is never used: a query with mnId 0 is blind to fresh keyframes, script ids).  A = 1 scores 1.0, B = 2 scores 0.75 = 0.75f * the best total exactly (not >: dropped),
    C = 3 scores 0.8125 (kept).  X: the query 4; R = 5 scores 1.0 and is the best neighbour of D = 6 (0.75) and E = 7 (0.8125): the two
    groups name R, which is returned once; R's own group (1.0) falls under 0.75 * 1.8125.
    Relocalisation: frame 0 over Y scores N = 8 at 1.0.  Frame 1 over Z and one word of Y meets N (one shared word: under the cut, not
    scored) and scores M = 9, whose neighbour N adds the 1.0 the EARLIER query left and, with it, represents the group."""
    W, X, Y, Z = [10, 11, 12, 13], [30, 31, 32, 33], list(range(50, 58)), list(range(60, 68))
    a = lambda words, vals: (np.array(words, np.int32), np.array(vals, np.float64))
    vectors = [a(W, [0.25] * 4),
               a(W, [0.25] * 4), a(W + [20], [0.1875] * 4 + [0.25]), a(W + [21], [0.1875, 0.1875, 0.1875, 0.25, 0.1875]),
               a(X, [0.25] * 4),
               a(X, [0.25] * 4), a(X + [40], [0.1875] * 4 + [0.25]), a(X + [41], [0.1875, 0.1875, 0.1875, 0.25, 0.1875]),
               a(Y, [0.125] * 8), a(Z, [0.125] * 8), a(W, [0.25] * 4)]
    frames = [a(Y, [0.125] * 8), a([50] + Z, [0.0625] + [0.125] * 7 + [0.0625])]
    sc = lambda q, k: BR.score(*q, *k)
    assert [sc(vectors[10], vectors[i]) for i in (1, 2, 3)] == [1.0, 0.75, 0.8125] and [sc(vectors[4], vectors[i]) for i in (5, 6, 7)] == [1.0, 0.75, 0.8125]
    assert sc(frames[0], vectors[8]) == 1.0 and sc(frames[1], vectors[9]) == 0.9375 and F(0.75) * F(1.0) == F(0.75)
    ordered = [[] for _ in vectors]
    ordered[6], ordered[7], ordered[9] = [5], [5], [8]
    ops = [(ADD, i, 0.0) for i in (3, 2, 1, 6, 7, 5, 9, 8)] + [(LOOP, 10, 0.0), (LOOP, 4, 0.0), (RELOC, 0, 0.0), (RELOC, 1, 0.0)]
    return _plain(BR.voc("k10L3_dfs"), vectors, frames, ops, ordered=ordered)


BUILDERS = {
    "path": lambda: _from_adapter_scene(G.adapter_scene()),
    "order": lambda: _from_adapter_scene(G.order_scene()),
    "gpu_query_65": lambda: _gpu_query(65),
    "gpu_query_300": lambda: _gpu_query(300),
    "gpu_erase": _gpu_erase,
    "host_query": _host_query,
    "ids": _ids,
    "cuts": _cuts,
    "groups": _groups,
}
NAMES = list(BUILDERS)
_scripts = {}


def script(name):
    if name not in _scripts:
        _scripts[name] = BUILDERS[name]()
    return _scripts[name]


_restated = {}


def restated(name):
    """restate(script(name)), computed once and shared; callers leave it unchanged."""
    if name not in _restated:
        _restated[name] = restate(script(name))
    return _restated[name]


# ---------------------------------------------------------------------------------------------------------------------
# the reference program and the fixture
# ---------------------------------------------------------------------------------------------------------------------
import functools  # noqa: E402
import os  # noqa: E402
import subprocess  # noqa: E402
import tempfile  # noqa: E402

import solver_pin_cases as S  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bowdb_reference.npz")


@functools.lru_cache(maxsize=None)
def reference_program(name="ref_kfdb"):
    """oracle/_ref/ref_kfdb (or ref_kfdb_san), (re)built where the reference's sources are; None where neither they nor a built program are."""
    if S.reference_present():
        subprocess.run(["make", "-s", "-C", S.ORACLE, "_ref/" + name], check=True)
    exe = os.path.join(S.ORACLE, "_ref", name)
    return exe if os.path.exists(exe) else None


def run_program(cmd_of, sc, tmp):
    """Writes the vocabulary and the script into tmp, runs cmd_of(voc, script, out) and returns parse_output of what it wrote."""
    fvoc, fin, fout = (os.path.join(str(tmp), x) for x in ("voc.txt", "script.bin", "out.txt"))
    with open(fvoc, "w") as f:
        f.write(sc.voc.text())
    with open(fin, "wb") as f:
        f.write(sc.to_bytes())
    r = subprocess.run(cmd_of(fvoc, fin, fout), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    with open(fout) as f:
        return parse_output(f.read(), sc)


def run_reference(name, order="asc", program="ref_kfdb"):
    with tempfile.TemporaryDirectory() as tmp:
        return run_program(lambda v, i, o: [reference_program(program), v, i, o, order], script(name), tmp)


def fixture_entries():
    """Everything the reference says on every script, with a digest of the script's inputs.  The thresholds a script takes `from a first
    pass` are checked here against the reference's own first pass."""
    entries = {}
    for name in NAMES:
        sc = script(name)
        t, bows = run_reference(name)
        e = t.pack("")
        e["inputs"] = sc.digest()
        # keyframes at other addresses (the driver's last argument) give the same lines: recorded as a flag per order
        e["orders_equal"] = np.array([int(not t.differences(run_reference(name, order)[0])) for order in ORDERS], np.int8)
        assert e["orders_equal"].all(), name
        entries[name] = e
    # cuts: DetectLoopCandidates(11, minScore) was given the score the reference itself gives keyframe 4, (12, ...) its best score
    sc, (t, _) = script("cuts"), run_reference("cuts")
    o11, o12 = [o for o, (op, idx, _) in enumerate(sc.ops) if op == LOOP and idx in (11, 12)]
    assert F(sc.ops[o11][2]) == t.scores[o11, 4, 0] and 4 in t.cands[o11]
    assert F(sc.ops[o12][2]) == t.scores[o12, 1:5, 0].max() and len(t.cands[o12]) == 1
    return entries


@functools.lru_cache(maxsize=None)
def load_fixture():
    entries = {}
    with np.load(GOLDEN, allow_pickle=False) as z:
        for member in z.files:
            name, key = member.split("|")
            entries.setdefault(name, {})[key] = z[member]
    return entries


@functools.lru_cache(maxsize=None)
def recorded_trace(name):
    """The Trace tests/golden/bowdb_reference.npz holds."""
    fx = load_fixture()[name]
    assert fx["inputs"].tobytes() == script(name).digest().tobytes(), "the script generator drifted from the recorded fixture"
    return Trace.unpack(fx, "")


@functools.lru_cache(maxsize=None)
def reference_trace(name):
    """(Trace, live): from oracle/_ref/ref_kfdb where it is, from the fixture otherwise."""
    if reference_program():
        return run_reference(name)[0], True
    return recorded_trace(name), False
