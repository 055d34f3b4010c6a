"""The keyframe database pinned against the reference's OWN src/orbslam/KeyFrameDatabase.cc.

oracle/Makefile compiles that source untouched, with its own header and the reference's ORBVocabulary.h (DBoW2's real
TemplatedVocabulary, BowVector, ScoringObject, FORB), over two data holders for KeyFrame / Frame (oracle/ref_shims_kfdb) and links it
with oracle/ref_kfdb_driver.cpp into oracle/_ref/ref_kfdb.  The driver replays the scripts of tests/bowdb_pin_cases.py and writes every
returned vector and, after every operation, the six query members of every keyframe.  tests/bow_restatement.py's Database, the host
path under SIVO::KeyFrameDatabase (tests/bow_adapter_prog.cpp over tests/bow_host_capi.hpp; tests/bow_prog.cpp's per-slot query too), the device database and the C++ classes on
the device were written from one reading of that source; this file holds each of them to every line the source itself writes.
Where the reference is absent the same assertions read tests/golden/bowdb_reference.npz (tests/golden/make_bowdb_reference.py wrote it
from the live run); the tests marked gpu read only the fixture."""
import os

import numpy as np
import pytest

from conftest import ROOT
import bow_restatement as BR
import bowdb_pin_cases as P
import host_prog
import test_bow_host as BH
import solver_pin_cases as S

F = np.float32


def same_trace(want, got, what):
    d = want.differences(got)
    assert not d, (what, d)


def test_with_the_reference_present_the_live_comparison_runs():
    _, live = P.reference_trace("order")
    assert live or not S.reference_present(), "the reference is here: the live comparison must run"
    assert sorted(P.load_fixture()) == sorted(P.NAMES)


def test_fixture_is_what_the_reference_computes(tmp_path):
    """The committed fixture, byte for byte, from a fresh run of the reference program; its size; and that every script's inputs are
    the ones it was recorded on."""
    assert os.path.getsize(P.GOLDEN) < 256 * 1024
    fx = P.load_fixture()
    for name in P.NAMES:
        assert fx[name]["inputs"].tobytes() == P.script(name).digest().tobytes(), name
        assert fx[name]["orders_equal"].tolist() == [1] * len(P.ORDERS), name
    if P.reference_program():
        import importlib.util
        spec = importlib.util.spec_from_file_location("make_bowdb_reference", os.path.join(ROOT, "tests", "golden", "make_bowdb_reference.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        assert open(mod.write(str(tmp_path)), "rb").read() == open(P.GOLDEN, "rb").read()


def test_fixture_round_trip():
    """pack / unpack of a trace loses nothing (the fixture holds changes, the assertions compare full tables)."""
    for name in ("ids", "path"):
        t, _ = P.restated(name)
        same_trace(t, P.Trace.unpack(t.pack("x."), "x."), name)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", P.NAMES)
def test_restatement_equals_the_reference(name):
    ref, _ = P.reference_trace(name)
    same_trace(ref, P.restated(name)[0], name)


def test_the_scripts_show_what_they_were_built_for():
    """Read from the REFERENCE's trace: each edge the scripts were written for is really met."""
    op_at = lambda sc, op, idx: [o for o, (a, b, _) in enumerate(sc.ops) if (a, b) == (op, idx)]
    # ids
    sc, (t, _) = P.script("ids"), P.reference_trace("ids")
    first0, again0 = op_at(sc, P.LOOP, 0)
    assert t.cands[first0] == [] and t.ints[first0, [3, 1, 2], 1].tolist() == [9, 10, 9] and t.ints[first0, [3, 1, 2], 0].tolist() == [0, 0, 0]
    assert t.cands[again0] == [3, 1, 2]                                 # (mnId 0 only blinds the database while the keyframes are fresh)
    a, b = op_at(sc, P.LOOP, 6)
    assert t.cands[a] == [3, 1, 2] and t.cands[b] == [] and t.ints[b, 1, 1] == 2 * t.ints[a, 1, 1] == 20         # an id used twice: counting goes on
    a, b = op_at(sc, P.RELOC, 0)[:2]
    assert t.cands[a] == [3, 1, 2] and t.cands[b] == [] and t.ints[b, 1, 3] == 20
    assert t.cands[op_at(sc, P.LOOP, 8)[0]] == [3, 2] and t.cands[op_at(sc, P.LOOP, 9)[0]] == [3, 2, 1]           # erased; added again, now last
    twice = op_at(sc, P.LOOP, 10)[0]
    assert t.ints[twice, 2, 1] == 18 and t.cands[twice] == [2]          # added twice: 9 shared words count 18, and the cut follows
    assert t.cands[op_at(sc, P.LOOP, 11)[0]] == [3, 1, 4, 2]            # erased once: the FIRST entry went, keyframe 2 is now behind 1 and 4
    assert t.cands[op_at(sc, P.LOOP, 12)[0]] == [3, 1, 4, 2]            # erase of a keyframe never added changes nothing
    assert t.cands[op_at(sc, P.LOOP, 13)[0]] == [] and t.cands[op_at(sc, P.LOOP, 14)[0]] == [1]                   # clear, then a query; then adds
    # cuts
    sc, (t, _) = P.script("cuts"), P.reference_trace("cuts")
    o = op_at(sc, P.LOOP, 13)[0]
    assert t.ints[o, [1, 2], 1].tolist() == [1, 1] and t.ints[o, [1, 2], 0].tolist() == [0, 0] and t.cands[o] == [3, 4]                  # connected: the count ends at 1
    o = op_at(sc, P.LOOP, 11)[0]
    assert t.ints[o, 3:7, 1].tolist() == [10, 9, 8, 1] and t.scores[o, 5, 0] == 0 and t.scores[o, 4, 0] > 0       # 8 of 10 is not enough, 9 is
    assert t.scores[o, 4, 0] == F(sc.ops[o][2]) and 4 in t.cands[o]                                              # si >= minScore at equality
    o = op_at(sc, P.LOOP, 7)[0]
    assert t.ints[o, 8:11, 1].tolist() == [5, 4, 4] and t.scores[o, 9:11, 0].tolist() == [0, 0] and t.cands[o] == [8]   # 4 of 5 is not enough
    assert int(F(10) * F(0.8)) == 8 and int(F(5) * F(0.8)) == 4
    # groups
    sc, (t, _) = P.script("groups"), P.reference_trace("groups")
    o = op_at(sc, P.LOOP, 10)[0]
    assert t.scores[o, 1:4, 0].tolist() == [1.0, 0.75, 0.8125] and t.cands[o] == [3, 1]                          # 0.75 is not > 0.75f * 1.0
    o = op_at(sc, P.LOOP, 4)[0]
    assert t.scores[o, 5:8, 0].tolist() == [1.0, 0.75, 0.8125] and t.cands[o] == [5]                             # two groups, one representative, once
    o = op_at(sc, P.RELOC, 1)[0]
    assert t.ints[o, 8, 2:].tolist() == [1001, 1] and t.scores[o, 8, 1] == 1.0 and t.scores[o, 9, 1] == 0.9375 and t.cands[o] == [8]
    # order, path: add order, id order and (in the driver) address order all differ
    assert P.reference_trace("order")[0].cands[4] == [2, 3, 1, 0]
    assert sum(len(c) > 1 for c in P.reference_trace("path")[0].cands.values()) >= 2


def test_the_result_does_not_depend_on_where_the_keyframes_lie():
    """The two std::set<KeyFrame *> are only asked for membership: keyframes at ascending, descending and scattered addresses give the
    same lines.  LIVE ONLY: where the reference program is absent nothing is replayed and the test passes without having checked anything
    (the fixture's `orders_equal` flags only say that the fixture's writer saw equal lines)."""
    if not P.reference_program():
        return
    for name in P.NAMES:
        for order in P.ORDERS[1:]:
            same_trace(P.reference_trace(name)[0], P.run_reference(name, order)[0], (name, order))


def test_reference_driver_under_address_and_undefined_sanitizers():
    """oracle/_ref/ref_kfdb_san: the same stand-alone program built with -fsanitize=address,undefined, on every script.  LIVE ONLY: where
    the reference program is absent there is nothing to run and the test passes without having checked anything."""
    if not P.reference_program():
        return
    assert P.reference_program("ref_kfdb_san")
    for name in P.NAMES:
        same_trace(P.reference_trace(name)[0], P.run_reference(name, "mixed", "ref_kfdb_san")[0], name)


# ---------------------------------------------------------------------------------------------------------------------
# the host path under SIVO::KeyFrameDatabase
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_adapter(tmp_path_factory):
    return host_prog.build("bow_adapter_prog", tmp_path_factory.mktemp("host_adapter"), defines=("SIVO_BOW_ON_HOST",))


def check_adapter(exe, name, tmp_path, trace):
    sc = P.script(name)
    got, bows = P.run_program(lambda v, i, o: [exe, v, i, o, "pin"], sc, tmp_path)
    for i, (a, b) in enumerate(zip(P.restated(name)[1], bows)):         # the BowVectors the classes held (the transform is pinned by bow_reference.npz)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (name, i)
    same_trace(trace(name), got, name)


@pytest.mark.parametrize("name", P.NAMES)
def test_host_path_under_the_adapter_equals_the_reference(host_adapter, name, tmp_path):
    check_adapter(host_adapter, name, tmp_path, lambda n: P.reference_trace(n)[0])


# ---------------------------------------------------------------------------------------------------------------------
# one query over every stored vector against the reference's lines: the restatement's, bow_prog's (the host build of bow_math.hpp), and
# further down the device's sivo_bowdb_query
# ---------------------------------------------------------------------------------------------------------------------
class PlainStore:
    """add / erase / clear / query with the slot rules of sivo_bowdb_* over tests/bow_restatement.py's query."""

    def __init__(self):
        self.stored = []

    def add(self, w, v):
        self.stored.append((w, v))
        return len(self.stored) - 1

    def erase(self, slot):
        self.stored[slot] = None

    def clear(self):
        self.stored = []

    def query(self, w, v):
        return BR.query(self.stored, w, v)


def check_store_against_trace(name, db, t):
    """Replays the script on a store of BowVectors (slots, one query per detection) and derives from the per-slot answers what the
    reference's walk must have left: the shared-word counts (mn*Words, continued where the id was used before, 1 for a keyframe connected
    to the query) and the float score of every keyframe over the cut."""
    sc = P.script(name)
    vec = sc.vectors()
    n_kf, slots, checked = len(sc.kfs), {}, 0
    for o, (op, idx, _) in enumerate(sc.ops):
        if op == P.ADD:
            slots.setdefault(idx, []).append(db.add(*vec[idx]))
        elif op == P.ERASE:
            if slots.get(idx):
                db.erase(slots[idx].pop(0))
        elif op == P.CLEAR:
            db.clear()
            slots = {}
        else:
            loop = op == P.LOOP
            qid, q = (idx, vec[idx]) if loop else (1000 + idx, vec[n_kf + idx])
            col = 0 if loop else 2
            got = db.query(*q)
            before = t.ints[o - 1] if o else np.zeros((n_kf, 4), np.int64)
            words, sharing = {}, []
            for kf, ss in slots.items():
                common = int(sum(got["common"][s] for s in ss))
                if not common:
                    continue
                if before[kf, col] == qid:
                    words[kf] = int(before[kf, col + 1]) + common
                elif loop and kf in sc.connected[idx]:
                    words[kf] = 1
                else:
                    words[kf] = common
                    sharing.append(kf)
            for kf, w in words.items():
                assert t.ints[o, kf, col + 1] == w, (name, o, kf)
            cut = int(F(max(words[kf] for kf in sharing)) * F(0.8)) if sharing else 0
            for kf in sharing:
                assert t.ints[o, kf, col] == qid
                if words[kf] > cut:
                    assert t.scores[o, kf, col // 2].tobytes() == F(got["score"][slots[kf][0]]).tobytes(), (name, o, kf)
                    checked += 1
    return checked


@pytest.mark.parametrize("name", P.NAMES)
def test_per_slot_query_of_the_restatement_gives_the_references_counts_and_scores(name):
    assert check_store_against_trace(name, PlainStore(), P.reference_trace(name)[0]) > 0


class ProgStore(PlainStore):
    """The same store with every query answered by `bow_prog query` (tests/bow_prog.cpp: bow_query_host of sivo_amd/csrc/bow_voc.hpp)."""

    def __init__(self, exe, tmp_path):
        super().__init__()
        self.exe, self.tmp_path = exe, tmp_path

    def query(self, w, v):
        empty = (np.zeros(0, np.int32), np.zeros(0))
        if not self.stored:
            return BR.query([], w, v)
        return BH.run_query(self.exe, self.tmp_path, [e if e is not None else empty for e in self.stored], (w, v))


@pytest.fixture(scope="module")
def bow_prog(tmp_path_factory):
    return host_prog.build("bow_prog", tmp_path_factory.mktemp("bow_prog"))


@pytest.mark.parametrize("name", P.NAMES)
def test_bow_prog_query_gives_the_references_counts_and_scores(bow_prog, tmp_path, name):
    assert check_store_against_trace(name, ProgStore(bow_prog, tmp_path), P.reference_trace(name)[0]) > 0


# ---------------------------------------------------------------------------------------------------------------------
# the device: reads only tests/golden
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_adapter(tmp_path_factory):
    return host_prog.build("bow_adapter_prog", tmp_path_factory.mktemp("device_adapter"), link_lib=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", P.NAMES)
def test_device_database_gives_the_recorded_references_counts_and_scores(name):
    from sivo_amd import bow
    v = P.script(name).voc
    db = bow.BowDatabase(bow.Vocabulary.from_arrays(v.k, v.L, v.parent, v.is_leaf, v.desc, v.weight))
    assert check_store_against_trace(name, db, P.recorded_trace(name)) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", P.NAMES)
def test_adapter_classes_on_the_device_equal_the_recorded_reference(device_adapter, name, tmp_path):
    check_adapter(device_adapter, name, tmp_path, P.recorded_trace)
