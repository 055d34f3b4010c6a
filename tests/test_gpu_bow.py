"""sivo_bow_transform / sivo_bow_transform_batch / sivo_bowdb_* (sivo_amd/csrc/bow.hip) and the C++ classes over them against the
restatement (tests/bow_restatement.py) BIT FOR BIT: word and node ids, the CSR form, the values and the scores as doubles."""
import copy
import functools
import subprocess

import numpy as np
import pytest

import bow_restatement as BR
import host_prog

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def device_voc(name):
    from sivo_amd import bow
    v = BR.voc(name)
    return bow.Vocabulary.from_arrays(v.k, v.L, v.parent, v.is_leaf, v.desc, v.weight)


@pytest.mark.parametrize("name", list(BR.VOCS))
def test_transform_equals_the_restatement_bit_for_bit(name):
    """n in {0, 1, 63, 64, 65} at every levelsup in {0, 2, 4, L, L + 1}."""
    v, dv = BR.voc(name), device_voc(name)
    assert (dv.k, dv.L, dv.n_nodes, dv.n_words) == (v.k, v.L, v.n_nodes, v.n_words)
    for lv in BR.levels(v):
        for n, s in zip(BR.SMALL_SIZES, BR.small_sets(name)):
            BR.same(dv.transform(s, lv), BR.want(name, n, s, lv))
            if lv >= v.L and n:
                assert not BR.want(name, n, s, lv)["node"].any()                 # levelsup >= L: the root for every feature


def test_vocabulary_loaded_from_text_is_the_vocabulary_from_arrays(tmp_path):
    from sivo_amd import bow
    for name in ("k10L3_dfs", "k7L4_pruned"):
        p = tmp_path / (name + ".txt")
        p.write_text(BR.voc(name).text(final_newline=True) + "\n")
        s = BR.small_sets(name)[-1]
        BR.same(bow.Vocabulary.from_text(p).transform(s, 2), BR.want(name, 65, s, 2))


@pytest.mark.parametrize("levelsup", BR.levels(BR.voc("k10L3_dfs")))
def test_transform_of_2000_features_and_of_one_descriptor_500_times(levelsup):
    dv = device_voc("k10L3_dfs")
    for tag, s in zip(("big", "repeat"), BR.big_sets()):
        BR.same(dv.transform(s, levelsup), BR.want("k10L3_dfs", tag, s, levelsup))


def test_set_at_the_cap_and_beyond_it():
    from sivo_amd import _lib, bow
    v, dv = BR.voc("k3L2"), device_voc("k3L2")
    s = BR.features(21, bow.SET_CAP, v)
    BR.same(dv.transform(s, 1), BR.transform(v, s, 1))
    with pytest.raises(_lib.SivoInvalidArgument):
        dv.transform(np.concatenate([s, s[:1]]), 1)


def test_every_feature_on_a_stopped_word_gives_empty_vectors():
    v, dv = BR.voc("stopped"), device_voc("stopped")
    s = BR.stopped_only_features(v, 40)
    got = dv.transform(s, 1)
    BR.same(got, BR.transform(v, s, 1))
    assert len(got["words"]) == 0 and len(got["fv_nodes"]) == 0 and got["fv_offsets"].tolist() == [0]


def test_batch_equals_the_single_calls():
    name = "k7L4_pruned"
    v, dv = BR.voc(name), device_voc(name)
    sets = [BR.features(30 + i, n, v) for i, n in enumerate([0, 1, 65, 300, 2])]
    got = dv.transform_batch(sets, 2)
    for s, g in zip(sets, got):
        BR.same(g, dv.transform(s, 2))
        BR.same(g, BR.transform(v, s, 2))


# ---------------------------------------------------------------------------------------------------------------------
# the database
# ---------------------------------------------------------------------------------------------------------------------
N_WORDS = 1000          # of k10L3


def db_vectors(n, seed=5):
    rng = np.random.default_rng(seed)
    return [BR.random_vector(rng, N_WORDS, int(m)) for m in rng.integers(1, 300, n)]


def same_query(got, want):
    for k in ("common", "first_word", "score"):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k


@pytest.mark.parametrize("n", [0, 1, 65, 300])
def test_query_equals_the_restatement_bit_for_bit(n):
    from sivo_amd import bow
    db = bow.BowDatabase(device_voc("k10L3_dfs"))
    rng = np.random.default_rng(n)
    stored = db_vectors(n)
    q = BR.random_vector(rng, N_WORDS, 180)
    other = np.setdiff1d(np.arange(N_WORDS, dtype=np.int32), q[0])
    if n:       # sharing no word, one word, all words; the query itself; an empty vector
        stored += [(other[:150], BR.random_vector(rng, N_WORDS, 150)[1]),
                   (np.sort(np.append(other[:99], q[0][17])).astype(np.int32), BR.random_vector(rng, N_WORDS, 100)[1]),
                   (q[0], BR.random_vector(rng, N_WORDS, 180)[1]), q, (np.zeros(0, np.int32), np.zeros(0))]
    assert [db.add(*e) for e in stored] == list(range(len(stored))) and len(db) == len(stored)
    want = BR.query(stored, *q)
    same_query(db.query(*q), want)
    if n:
        assert want["common"][n:].tolist() == [0, 1, 180, 180, 0] and want["first_word"][n:].tolist() == [-1, q[0][17], q[0][0], q[0][0], -1]
        # a vector against itself: whatever the reference's arithmetic gives, not an assumed 1.0
        assert want["score"][n + 3] == BR.score(q[0], q[1], q[0], q[1]) and abs(want["score"][n + 3] - 1.0) < 1e-12
        print("score of the query against itself:", repr(float(want["score"][n + 3])))
    same_query(db.query(np.zeros(0, np.int32), np.zeros(0)), BR.query(stored, np.zeros(0, np.int32), np.zeros(0)))


def test_erase_then_query_and_clear_then_add():
    from sivo_amd import _lib, bow
    db = bow.BowDatabase(device_voc("k10L3_dfs"))
    stored = db_vectors(70, seed=9)
    for e in stored:
        db.add(*e)
    q = stored[11]
    for slot in (11, 64, 69):
        db.erase(slot)
        stored[slot] = None
    want = BR.query(stored, *q)
    same_query(db.query(*q), want)
    assert want["common"][[11, 64, 69]].tolist() == [0, 0, 0] and (want["common"] > 0).sum() > 10
    with pytest.raises(_lib.SivoInvalidArgument):
        db.erase(11)
    assert db.add(*q) == 70                                                      # slots are never reused
    db.clear()
    assert len(db) == 0 and len(db.query(*q)["common"]) == 0
    fresh = db_vectors(3, seed=10)
    assert [db.add(*e) for e in fresh] == [0, 1, 2]
    same_query(db.query(*q), BR.query(fresh, *q))


# ---------------------------------------------------------------------------------------------------------------------
# SIVO::ORBVocabulary / SIVO::KeyFrameDatabase over stand-in SLAM types
# ---------------------------------------------------------------------------------------------------------------------
N_KF, LEVELSUP = 60, 1
ADD, ERASE, LOOP, RELOC, CLEAR = range(5)


def adapter_scene():
    """60 keyframes along a path: keyframe i sees a window of a pool of descriptors (a few bits flipped per view), so neighbours share
    words; the path returns at keyframe 50 to where keyframe 5 was.  Keyframes are added evens first, then odds: the add sequence is
    not the id order.  Covisibility: |i - j| <= 3 connected, the ordered list the nearest first; keyframe 55 is also connected to 10."""
    v = BR.voc("k10L3_dfs")
    rng = np.random.default_rng(77)
    pool = BR.features(78, 700, v, near=1.0)

    def view(start, n=90):
        d = pool[(start + np.arange(n)) % len(pool)].copy()
        flips = rng.integers(0, 32, n)
        d[np.arange(n), flips] ^= (rng.random(n) < 0.3).astype(np.uint8)
        return d

    start = [10 * i if i < 50 else 10 * (i - 45) + 3 for i in range(N_KF)]
    kfs = [view(s) for s in start]
    kfs[56] = np.concatenate([view(113, 45), view(333, 45)])          # two places at once: more than one candidate survives the 0.75 cut
    near = lambda i: sorted((j for j in range(N_KF) if j != i and abs(i - j) <= 5), key=lambda j: (abs(i - j), j))
    connected = [[j for j in near(i) if abs(i - j) <= 3] for i in range(N_KF)]
    connected[55].append(10)
    frames = [view(203), np.concatenate([view(57, 60), view(357, 60)]), kfs[12].copy()]
    order = list(range(0, 50, 2)) + list(range(1, 50, 2))
    ops = [(ADD, i, 0.0) for i in order] + [(ERASE, 9, 0.0), (LOOP, 55, 0.01), (RELOC, 0, 0.0), (ERASE, 30, 0.0), (LOOP, 56, 0.05),
                                            (RELOC, 1, 0.0), (RELOC, 2, 0.0), (CLEAR, 0, 0.0)] + [(ADD, i, 0.0) for i in (7, 3, 5, 4, 6)] + [(LOOP, 57, 0.0)]
    return v, kfs, connected, [near(i) for i in range(N_KF)], frames, ops


def order_scene():
    """Four stored keyframes without covisibility, all close enough to the query to survive both cuts, built so that the ORDER of the
    returned vector shows how the sharing keyframes were ordered.  The query holds the words W; keyframe 2 holds all of them, keyframes
    0, 1, 3 all but the smallest.  Added in the order 3, 1, 2, 0.  The reference's walk meets 2 first (it alone owns the smallest query
    word), then 3, 1, 0 (tied on the second word: the add sequence decides, against the id order)."""
    v = BR.voc("k10L3_dfs")
    reach = {}
    for i in range(1, v.n_nodes):                                       # word -> a descriptor whose descent ends on it
        if v.word[i] >= 0 and v.node_weight[i] > 0:
            leaf, _ = BR.descend(v, v.node_desc[i], 0)
            reach.setdefault(int(v.word[leaf]), v.node_desc[i])
    words = sorted(reach)[5:45]
    W, extra = words[:30], words[30:]
    rows = lambda ws: np.stack([reach[w] for w in ws])
    kfs = [rows(W[1:] + extra[0:2]), rows(W[1:] + extra[2:4]), rows(W + extra[4:5]), rows(W[1:] + extra[5:8]), rows(W), rows(W + extra[8:9])]
    none = [[] for _ in kfs]
    ops = [(ADD, i, 0.0) for i in (3, 1, 2, 0)] + [(LOOP, 4, 0.01), (RELOC, 0, 0.0), (LOOP, 5, 0.01)]
    return v, kfs, none, none, [rows(W)], ops


def adapter_expectation(v, kfs, connected, ordered, frames, ops, path_scene):
    """The same calls on plain records (tests/bow_restatement.py).  Also returns, per detection, the candidates under three other
    orders of the sharing keyframes: (smallest shared word, id), add sequence alone, id alone."""
    n_kf = len(kfs)
    T = [BR.transform(v, d, LEVELSUP) for d in kfs + frames]
    K = [BR.KF(i, T[i]["words"], T[i]["values"]) for i in range(n_kf)]
    for i in range(n_kf):
        K[i].connected, K[i].best_cov = {K[j] for j in connected[i]}, [K[j] for j in ordered[i]][:10]
    Fr = [BR.KF(1000 + i, T[n_kf + i]["words"], T[n_kf + i]["values"]) for i in range(len(frames))]
    db, want_q, others, seq = BR.Database(), {}, {}, {}
    for o, (op, idx, ms) in enumerate(ops):
        if op == ADD:
            db.add(K[idx])
            seq[idx] = o
        elif op == ERASE:
            db.erase(K[idx])
        elif op == CLEAR:
            db.clear()
        else:
            if path_scene and op == LOOP and idx == 55:       # the cases the scene was built for, before the call changes the fields
                sharing = [k for k in K[:50] if k.mnId != 9 and len(np.intersect1d(k.words, K[55].words))]
                first = {k.mnId: int(np.intersect1d(k.words, K[55].words)[0]) for k in sharing}
                assert [(a, b) for a in first for b in first if a < b and first[a] == first[b] and a % 2 == 1 and b % 2 == 0]
                best = max((k for k in sharing), key=lambda k: BR.score(K[55].words, K[55].values, k.words, k.values))
                assert best.mnId == 10 and best in K[55].connected        # the would-be best candidate is connected to the query
                assert len(np.intersect1d(K[9].words, K[55].words))      # the erased keyframe would have shared words
            q = K[idx] if op == LOOP else Fr[idx]
            first_word = lambda k: int(np.intersect1d(k.words, q.words)[0])
            rules = {"word_then_id": lambda k: (first_word(k), k.mnId), "add_sequence": lambda k: seq[k.mnId], "id": lambda k: k.mnId}
            others[o] = {}
            for name, key in rules.items():                              # on copies: a detection writes into the keyframes
                db2, q2 = copy.deepcopy((db, q))
                reorder = lambda lst, key=key: sorted(lst, key=key)
                got = db2.detect_loop(q2, ms, reorder) if op == LOOP else db2.detect_reloc(q2, reorder)
                others[o][name] = [k.mnId for k in got]
            want_q[o] = [k.mnId for k in (db.detect_loop(q, ms) if op == LOOP else db.detect_reloc(q))]
    assert all(len(want_q[o]) for o in want_q)
    return K, T, want_q, others


def run_adapter(tmp_path, v, kfs, connected, ordered, frames, ops):
    n_kf = len(kfs)
    desc = lambda d: np.array([len(d)], np.int64).tobytes() + np.ascontiguousarray(d, np.uint8).tobytes()
    ids = lambda a: np.array([len(a)] + list(a), np.int64).tobytes()
    blob = [np.array([LEVELSUP, n_kf], np.int64).tobytes()]
    for i in range(n_kf):
        blob += [desc(kfs[i]), ids(connected[i]), ids(ordered[i])]
    blob += [np.array([len(frames)], np.int64).tobytes()] + [desc(f) for f in frames] + [np.array([len(ops)], np.int64).tobytes()]
    blob += [np.array([op, idx], np.int64).tobytes() + np.array([ms], np.float64).tobytes() for op, idx, ms in ops]
    fvoc, fin, fout = tmp_path / "voc.txt", tmp_path / "scene.bin", tmp_path / "out.txt"
    fvoc.write_text(v.text())
    fin.write_bytes(b"".join(blob))
    exe = host_prog.build("bow_adapter_prog", tmp_path, link_lib=True)
    r = subprocess.run([exe, str(fvoc), str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    got_q, got_k, got_b = {}, {}, {}
    for line in fout.read_text().splitlines():
        t = line.split()
        if t[0] == "Q":
            got_q[int(t[1])] = [int(x) for x in t[3:]]
        elif t[0] == "K":
            got_k[int(t[1])] = [int(t[2]), int(t[3]), int(t[4]), int(t[5]), float.fromhex(t[6]), float.fromhex(t[7])]
        elif t[0] in ("B", "F"):
            pairs = [p.split(":") for p in t[3:]]
            got_b[(t[0], int(t[1]))] = (np.array([int(p[0]) for p in pairs], np.int32), np.array([float.fromhex(p[1]) for p in pairs], np.float64))
        elif t[0] in ("BV", "FV"):
            got_b[(t[0], int(t[1]))] = {int(p.split(":")[0]): [int(x) for x in p.split(":")[1].split(",")] for p in t[3:]}
    return got_q, got_k, got_b


def check_adapter(tmp_path, scene, path_scene):
    v, kfs = scene[0], scene[1]
    K, T, want_q, others = adapter_expectation(*scene, path_scene)
    got_q, got_k, got_b = run_adapter(tmp_path, *scene)
    for i, t in enumerate(T):                                            # ORBVocabulary::transform, both overloads
        key = ("B", i) if i < len(kfs) else ("F", i - len(kfs))
        assert got_b[key][0].tobytes() == t["words"].tobytes() and got_b[key][1].tobytes() == t["values"].tobytes(), key
        fv = {int(n): t["fv_features"][t["fv_offsets"][j]:t["fv_offsets"][j + 1]].tolist() for j, n in enumerate(t["fv_nodes"])}
        assert got_b[(key[0] + "V", key[1])] == fv, key
    assert got_q == want_q                                               # the candidates, in the reference's order
    for i in range(len(kfs)):
        assert got_k[i] == K[i].fields(), i
    return want_q, others


def test_adapter_classes_return_the_candidates_of_the_reference_walk(tmp_path):
    want_q, _ = check_adapter(tmp_path, adapter_scene(), True)
    assert 10 not in want_q[min(want_q)] and sum(len(c) > 1 for c in want_q.values()) >= 2


def test_adapter_orders_the_candidates_by_smallest_shared_word_then_add_sequence(tmp_path):
    """A scene in which the order of the returned vector depends on the order of the sharing keyframes: every other rule a
    one-launch query could sort by — (smallest shared word, id), add sequence alone, id alone — gives another vector."""
    want_q, others = check_adapter(tmp_path, order_scene(), False)
    assert len(want_q) == 3
    for o, want in want_q.items():
        assert want == [2, 3, 1, 0], (o, want)
        for rule, got in others[o].items():
            assert sorted(got) == [0, 1, 2, 3] and got != want, (o, rule, got)
