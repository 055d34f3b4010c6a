"""Place recognition without a device: the loader and the kernels' arithmetic (bow_voc.hpp, bow_math.hpp) compiled for the host against the
restatement, bit for bit, also under the address and undefined-behaviour sanitizers and on malformed vocabulary files; the restatement
against values recorded from the reference's own DBoW2; header, exports, ctypes signatures, argument checks; the two C++ headers in
their SIVO_HAVE_OPENCV mode."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bow_restatement as BR
import host_prog

ROOT = host_prog.ROOT
API = os.path.join(ROOT, "sivo_amd", "api")
NAMES = ("sivo_voc_create_from_text", "sivo_voc_create", "sivo_voc_info", "sivo_voc_destroy", "sivo_bow_transform", "sivo_bow_transform_batch",
         "sivo_bowdb_create", "sivo_bowdb_add", "sivo_bowdb_erase", "sivo_bowdb_clear", "sivo_bowdb_destroy",
         "sivo_bowdb_size", "sivo_bowdb_query")


def run_transform(exe, tmp_path, voc_path, sets, levelsup):
    blob = (np.array([len(sets), levelsup], np.int64).tobytes()
            + b"".join(np.array([len(s)], np.int64).tobytes() + np.ascontiguousarray(s, np.uint8).tobytes() for s in sets))
    raw, at, out = host_prog.run(exe, tmp_path, "transform", blob, extra_args=(voc_path,), timeout=120), 0, []
    for _ in sets:
        n, nw, nf, m = np.frombuffer(raw, np.int64, 4, at)
        at += 32
        o = {}
        for key, cnt, dt in (("word", n, np.int32), ("node", n, np.int32), ("words", nw, np.int32), ("fv_nodes", nf, np.int32),
                             ("fv_offsets", nf + 1, np.int32), ("fv_features", m, np.int32), ("values", nw, np.float64)):
            o[key] = np.frombuffer(raw, dt, int(cnt), at)
            at += int(cnt) * np.dtype(dt).itemsize
        out.append(o)
    assert at == len(raw)
    return out


def run_query(exe, tmp_path, stored, q):
    vec = lambda w, v: np.array([len(w)], np.int64).tobytes() + np.asarray(w, np.int32).tobytes() + np.asarray(v, np.float64).tobytes()
    raw = host_prog.run(exe, tmp_path, "query", np.array([len(stored)], np.int64).tobytes() + b"".join(vec(*e) for e in stored) + vec(*q), timeout=120)
    rec = np.frombuffer(raw, np.dtype([("common", np.int32), ("first_word", np.int32), ("score", np.float64)]))
    return {k: rec[k] for k in ("common", "first_word", "score")}


def voc_file(tmp_path, name, final_newline=False):
    p = tmp_path / (name + ".txt")
    p.write_text(BR.voc(name).text(final_newline))
    return p


def check_host(exe, tmp_path):
    stopped = leaves_above = 0
    for name in BR.VOCS:
        v = BR.voc(name)
        path = voc_file(tmp_path, name, final_newline=name == "k3L2")            # (a trailing newline adds no node)
        r = subprocess.run([exe, "load", str(path)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and [int(x) for x in r.stdout.split()] == [v.k, v.L, v.n_nodes, v.n_words], (r.stdout, r.stderr)
        sets = BR.small_sets(name)
        for lv in BR.levels(v):
            got = run_transform(exe, tmp_path, path, sets, lv)
            for n, s, g in zip(BR.SMALL_SIZES, sets, got):
                w = BR.want(name, n, s, lv)
                BR.same(g, w)
                stopped += int((v.node_weight[1:][v.is_leaf > 0][w["word"]] == 0).sum()) if n else 0
        leaves_above += int(((v.level[1:] < v.L) & (v.is_leaf > 0)).sum())
    assert stopped > 0 and leaves_above > 0
    big = BR.big_sets()
    path = voc_file(tmp_path, "k10L3_dfs")
    for lv in BR.levels(BR.voc("k10L3_dfs")):
        for tag, s, g in zip(("big", "repeat"), big, run_transform(exe, tmp_path, path, big, lv)):
            BR.same(g, BR.want("k10L3_dfs", tag, s, lv))
    assert len(BR.want("k10L3_dfs", "repeat", big[1], 0)["words"]) == 1
    v = BR.voc("stopped")
    s = BR.stopped_only_features(v, 40)
    g = run_transform(exe, tmp_path, voc_file(tmp_path, "stopped"), [s], 1)[0]
    BR.same(g, BR.transform(v, s, 1))
    assert len(g["words"]) == 0 and len(g["fv_nodes"]) == 0 and g["fv_offsets"].tolist() == [0]
    # the query: no word, one word, all words shared; a stored vector equal to the query
    rng = np.random.default_rng(3)
    q = BR.random_vector(rng, 5000, 200)
    other = np.setdiff1d(np.arange(5000, dtype=np.int32), q[0])
    stored = [BR.random_vector(rng, 5000, int(n)) for n in rng.integers(1, 400, 65)]
    stored += [(other[:150], BR.random_vector(rng, 5000, 150)[1]), (np.sort(np.append(other[:99], q[0][17])).astype(np.int32), BR.random_vector(rng, 5000, 100)[1]),
               (q[0], BR.random_vector(rng, 5000, 200)[1]), q, (np.zeros(0, np.int32), np.zeros(0))]
    got, want = run_query(exe, tmp_path, stored, q), BR.query(stored, *q)
    for k in ("common", "first_word", "score"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert want["common"][65:].tolist() == [0, 1, 200, 200, 0] and want["first_word"][66] == q[0][17]
    return want["score"][68]


def test_host_build_of_the_arithmetic_and_the_loader_equals_the_restatement(tmp_path):
    self_score = check_host(host_prog.build("bow_prog", tmp_path), tmp_path)
    print("score of a vector against itself:", repr(float(self_score)))


MALFORMED = {
    "forward_parent": lambda t: t.replace("\n0 ", "\n5 ", 1),                      # node 1 names node 5 as its parent
    "leaf_parent": None,                                                          # filled in below: a child of a word
    "truncated_line": lambda t: t[:t.rindex(" ")],                                # the last line loses its weight
    "k21": lambda t: "21" + t[t.index(" "):],
    "empty": lambda t: "",
    "blank_only": lambda t: "\n\n  \n",
    "inner_without_children": None,
    "l2_scoring": lambda t: t.replace(" 0 0\n", " 1 0\n", 1),
}


def malformed_texts():
    v = BR.voc("k3L2")
    t = v.text()
    lines = t.split("\n")
    first_leaf = int(np.flatnonzero(v.is_leaf > 0)[0]) + 1
    out = {k: f(t) for k, f in MALFORMED.items() if f}
    out["leaf_parent"] = t + "\n" + " ".join([str(first_leaf), "1"] + ["7"] * 32 + ["1.5"])
    out["inner_without_children"] = "3 2 0 0\n" + " ".join(["0", "0"] + ["7"] * 32 + ["0"])     # the root's only child is an inner node
    assert len(lines) == v.n_nodes
    return out


SAYS = {"forward_parent": "earlier inner node", "leaf_parent": "earlier inner node", "truncated_line": "truncated", "k21": "k outside", "empty": "empty",
        "blank_only": "empty", "inner_without_children": "no children", "l2_scoring": "only L1_NORM scoring with TF_IDF weighting"}


def check_loader_rejects(exe, tmp_path):
    for name, text in malformed_texts().items():
        p = tmp_path / (name + ".txt")
        p.write_text(text)
        r = subprocess.run([exe, "load", str(p)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and SAYS[name] in r.stderr, (name, r.returncode, r.stderr[-2000:])
    v = BR.voc("k3L2")
    p = tmp_path / "trailing.txt"
    p.write_text(v.text() + "\n\n\r\n  \n")                                     # trailing blank lines: the same vocabulary
    r = subprocess.run([exe, "load", str(p)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and [int(x) for x in r.stdout.split()] == [v.k, v.L, v.n_nodes, v.n_words], r.stderr[-2000:]


def test_loader_rejects_malformed_files(tmp_path):
    check_loader_rejects(host_prog.build("bow_prog", tmp_path), tmp_path)


def test_host_build_under_address_and_undefined_sanitizers(tmp_path):
    """The stand-alone program built with -fsanitize=address,undefined and run directly, on the well-formed and the malformed files."""
    if not host_prog.sanitizer_runtime_present(tmp_path):
        pytest.skip("the sanitizer runtime (libasan / libubsan) is not installed: a trivial main does not link with -fsanitize")
    exe = host_prog.build("bow_prog", tmp_path, sanitize=True)
    check_host(exe, tmp_path)
    check_loader_rejects(exe, tmp_path)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement against the reference's own DBoW2 (tests/golden/make_bow_reference.py recorded the fixture)
# ---------------------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_recorded_reference():
    fx = np.load(os.path.join(ROOT, "tests", "golden", "bow_reference.npz"))
    names = [str(n) for n in fx["names"]]
    assert len(names) >= 6
    for i, name in enumerate(names):
        v = BR.voc(name)
        assert fx[f"{i}_desc"].tobytes() == v.desc.tobytes() and fx[f"{i}_weight"].tobytes() == v.weight.tobytes()     # the fixture's inputs
        for lv in fx[f"{i}_levelsup"].tolist():
            assert not ((v.level[1:] < v.L - lv) & (v.is_leaf > 0)).any()        # no leaf above the level: the reference is determinate
            f = fx[f"{i}_features"]
            w = BR.transform(v, f, lv)
            for key in ("word", "node", "words", "values", "fv_nodes", "fv_offsets", "fv_features"):
                assert fx[f"{i}_{lv}_{key}"].tobytes() == w[key].tobytes(), (name, lv, key)
        a, b = BR.transform(v, fx[f"{i}_features"], 0), BR.transform(v, fx[f"{i}_features2"], 0)
        s = np.array([BR.score(a["words"], a["values"], b["words"], b["values"]), BR.score(a["words"], a["values"], a["words"], a["values"])])
        assert fx[f"{i}_scores"].tobytes() == s.tobytes(), name


# ---------------------------------------------------------------------------------------------------------------------
# header, exports, signatures, argument checks
# ---------------------------------------------------------------------------------------------------------------------
def declared():
    h = open(os.path.join(ROOT, "include", "sivo_hip.h")).read()
    return {m.group(1): [a.strip() for a in m.group(2).split(",")] for m in re.finditer(r"\nint (sivo_(?:voc|bow|bowdb)_\w+)\(([^)]*)\);", h)}, h


def test_header_declares_and_library_exports_the_entry_points():
    decl, h = declared()
    assert sorted(decl) == sorted(NAMES)
    assert "TemplatedVocabulary.h:1126-1194" in h and "KeyFrameDatabase.cc:72-322" in h and "ScoringObject.cpp:23-68" in h
    from sivo_amd import _lib
    L = _lib.lib()
    assert all(hasattr(L, n) for n in NAMES)
    assert f"#define SIVO_BOW_SET_CAP {__import__('sivo_amd.bow', fromlist=['x']).SET_CAP}" in h


def test_ctypes_signatures_match_the_header():
    from sivo_amd import _lib
    decl, _ = declared()
    assert sorted(decl) == sorted(NAMES)
    for name, params in decl.items():
        sig = _lib.SIGNATURES[name]
        assert len(sig) == len(params), name
        for p, t in zip(params, sig):
            if "*" in p:
                want = {C.c_void_p, C.c_char_p} if "char" in p else {C.c_void_p}
                assert t in want or (hasattr(t, "_type_") and not isinstance(t._type_, str)), (name, p, t)      # a POINTER(...) type
                if hasattr(t, "_type_") and not isinstance(t._type_, str):
                    base = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "sivo_voc_t": C.c_void_p, "sivo_bowdb_t": C.c_void_p}
                    assert t._type_ is base[p.replace("const ", "").split()[0]], (name, p, t)
            else:
                base = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "sivo_voc_t": C.c_void_p, "sivo_bowdb_t": C.c_void_p}
                assert t is base[p.split()[0]], (name, p, t)


def test_entry_points_check_arguments_and_fail_loudly_without_a_device(tmp_path):
    from sivo_amd import _lib, bow
    for name, text in malformed_texts().items():
        p = tmp_path / (name + ".txt")
        p.write_text(text)
        with pytest.raises(_lib.SivoInvalidArgument) as e:
            bow.Vocabulary.from_text(p)
        assert SAYS[name] in str(e.value), name
    with pytest.raises(_lib.SivoInvalidArgument):
        bow.Vocabulary.from_text(tmp_path / "missing.txt")
    v = BR.voc("k7L4_pruned")
    voc = bow.Vocabulary.from_text(voc_file(tmp_path, "k7L4_pruned"))
    arr = bow.Vocabulary.from_arrays(v.k, v.L, v.parent, v.is_leaf, v.desc, v.weight)
    for x in (voc, arr):
        assert (x.k, x.L, x.n_nodes, x.n_words, len(x)) == (v.k, v.L, v.n_nodes, v.n_words, v.n_words)
    bad = v.parent.copy()
    bad[3] = 100
    with pytest.raises(_lib.SivoInvalidArgument):
        bow.Vocabulary.from_arrays(v.k, v.L, bad, v.is_leaf, v.desc, v.weight)
    with pytest.raises(_lib.SivoInvalidArgument):
        bow.Vocabulary.from_arrays(v.k, 11, v.parent, v.is_leaf, v.desc, v.weight)
    # before any device is needed: the cap, a negative levelsup, unsorted words, a word outside the vocabulary
    with pytest.raises(_lib.SivoInvalidArgument):
        voc.transform(np.zeros((bow.SET_CAP + 1, 32), np.uint8))
    with pytest.raises(_lib.SivoInvalidArgument):
        voc.transform(np.zeros((3, 32), np.uint8), levelsup=-1)
    db = bow.BowDatabase(voc)
    for w in ([3, 2], [2, 2], [0, v.n_words], [-1, 4]):
        with pytest.raises(_lib.SivoInvalidArgument):
            db.add(w, [0.5, 0.5])
        with pytest.raises(_lib.SivoInvalidArgument):
            db.query(w, [0.5, 0.5])
    with pytest.raises(_lib.SivoInvalidArgument):
        db.erase(0)
    # nothing to do: no launch, no device needed
    e = voc.transform(np.zeros((0, 32), np.uint8))
    assert len(e["words"]) == 0 and e["fv_offsets"].tolist() == [0]
    assert voc.transform_batch([]) == [] and len(db) == 0 and len(db.query([1], [1.0])["common"]) == 0
    if _lib.lib().sivo_device_count() >= 1:              # (a device is visible: tests/test_gpu_bow.py checks what the calls compute)
        return
    for call in (lambda: voc.transform(np.zeros((3, 32), np.uint8)), lambda: db.add([1, 2], [0.5, 0.5])):
        with pytest.raises(_lib.SivoError) as e:
            call()
        assert e.value.code == _lib.ERR_RUNTIME


# ---------------------------------------------------------------------------------------------------------------------
# the C++ classes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("header", ["orbslam/ORBVocabulary.h", "orbslam/KeyFrameDatabase.h"])
def test_headers_compile_against_the_real_type_names(tmp_path, header):
    tu = tmp_path / "use.cpp"
    tu.write_text(f'#include "{header}"\nint main() {{ return 0; }}\n')
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-DSIVO_HAVE_OPENCV", "-I" + os.path.join(ROOT, "oracle", "ref_shims"),
                        "-I" + API, str(tu)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-I" + API, str(tu)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


def test_orbvocabulary_score_on_the_host_equals_the_restatement(tmp_path):
    """ORBVocabulary::score needs no device: the ordered L1 arithmetic over two std::maps, bit for bit."""
    rng = np.random.default_rng(12)
    q = BR.random_vector(rng, 400, 120)
    pairs = [(q, BR.random_vector(rng, 400, int(n))) for n in (1, 50, 120, 399)] + [(q, q), (q, (np.zeros(0, np.int32), np.zeros(0)))]
    fin = tmp_path / "pairs.txt"
    fin.write_text("\n".join(" ".join([str(len(w))] + [f"{int(a)} {float(b).hex()}" for a, b in zip(w, v)]) for p in pairs for w, v in p) + "\n")
    exe = host_prog.build("bow_score_prog", tmp_path, link_lib=True)
    r = subprocess.run([exe, str(fin)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = np.array([float.fromhex(x) for x in r.stdout.split()])
    want = np.array([BR.score(a[0], a[1], b[0], b[1]) for a, b in pairs])
    assert got.tobytes() == want.tobytes()
    assert np.signbit(want[-1]) and want[-1] == 0                       # no shared word: -0.0, as -sum / 2 gives
