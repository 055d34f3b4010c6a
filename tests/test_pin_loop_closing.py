"""LoopClosing::CorrectLoop, the loop fusion, SearchAndFuse and the map update behind the global bundle adjustment pinned against the
reference's OWN LoopClosing.cc.

oracle/Makefile compiles src/orbslam/LoopClosing.cc, KeyFrame.cc, MapPoint.cc, Map.cc and Converter.cc untouched, with their own headers,
over data holders for the rest of the system (oracle/ref_shims_loopclosing) and links them with oracle/ref_loopclosing_driver.cpp into
oracle/_ref/ref_loopclosing: REAL KeyFrame, MapPoint, Map and LoopClosing objects, allocated in the scene's address order, protected state
set through derived classes.  `loop` calls CorrectLoop() whole and takes its snapshot where the reference calls
Optimizer::OptimizeEssentialGraph (:582); `gba` calls RunGlobalBundleAdjustment(nLoopKF).  The kernels (loopcorrect_math.hpp), their host
build, the adapter over stand-in types and the Python restatement were written from one reading of that file and are tested against each
other; this file holds each of them against what the file itself leaves, byte for byte in sentinel-filled arrays, doubles included — there
is no tolerance anywhere:
  * correction  :436-526 on 17 graphs: mvpCurrentConnectedKFs as KeyFrame::UpdateConnections made it (and the restatement of
                UpdateConnections on the same graph), both Sim3 maps in map order, every corrected pose and centre, which keyframe moved
                which point, its position, normal and distances — against loop_correct_restatement, tests/loop_correct_prog.cpp and
                tests/loop_correct_adapter_prog.cpp, and on the device through the C ABI and sivo_amd/loop_closing.py;
  * gba         :694-753 on 9 trees: mTcwGBA, mnBAGlobalForKF, mTcwBefGBA, pose and centre of every keyframe, every point — the same four;
  * fusion      :530-542 and :609-635 with the real MapPoint::Replace / AddObservation / ComputeDistinctiveDescriptors: slots, observations,
                Observations(), bad flags, replaced-by links, found / visible and descriptors of every point, the matcher's calls in order
                with the Sim3 each was handed and the descriptor each loop point had when the call met it — against a restatement in
                loop_closing_pin_cases (restated_fusion);
  * connections :553-579: LoopConnections against covis_restatement / map_graph_restatement on the graph the fusion left.
Substitutions of this build: g2o::Sim3 / Eigen::Quaterniond (oracle/ref_shims_loopclosing/g2o_sim3_standin.hpp, g2o's and
Eigen's operation order), cv::Mat's gemm rounding (cv_min.hpp), Optimizer / LocalMapping / the threads as holders, and ORBmatcher::Fuse,
which is SCRIPTED: which loop point lands on which slot is given, so the CANDIDATE CHOICE of the fuse kernel is not pinned here
(tests/test_pin_matcher.py and test_fuse_batch_host.py hold it against this repository's matcher); the order of the keyframes, the graph
each call meets, the deferred Replace calls and Replace itself are the reference's.
  * adapter     SIVO::SearchAndFuse of api/orbslam/FusionAdapter.h (tests/fuse_batch_adapter_prog.cpp, the host build here and the product
                library under the gpu mark) on the two loop scenes of fuse_batch_adapter_cases: `ref_loopclosing fuse` runs the reference's
                SearchAndFuse alone on the same graph, the script written by hand from the scene's description; the program's event log
                must show those landings, and both of its copies must leave the reference's slots, observations, flags, replaced-by links,
                found / visible and descriptors.  So its order, its deferral, its repair step and the stand-ins' Replace /
                ComputeDistinctiveDescriptors are held against MapPoint.cc; which key its matcher picks is not.

The pin found no difference: all 17 + 9 + 17 + 17 + 2 comparisons agree.

Where the reference is absent the same assertions read tests/golden/loop_closing_reference.npz; the tests marked gpu read only that file
and tests/."""
import os

import numpy as np
import pytest

from conftest import ROOT
import essential_graph_restatement as EG
import fuse_batch_adapter_cases as AC
import host_prog
import loop_closing_pin_cases as P
import loop_correct_cases as LC
import loop_correct_restatement as LR
import map_graph_pin_cases as M
import solver_pin_cases as S

LOOP_NAMES = [n for n, *_ in LC.LOOP_OUT]
GBA_NAMES = [n for n, *_ in LC.GBA_OUT]
SENT = LC.SENTINEL


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return host_prog.build("loop_correct_prog", tmp_path_factory.mktemp("loop_correct_prog"))


@pytest.fixture(scope="module")
def adapter_prog(tmp_path_factory):
    return host_prog.build("loop_correct_adapter_prog", tmp_path_factory.mktemp("loop_correct_adapter_prog"))


def loop_want(name):
    return P.reference_facts("loop." + name)[0]


def test_with_the_reference_present_the_live_comparison_runs():
    for entry in ("loop.only_current", "loop.fuse_repair", "gba.run_40"):
        _, live = P.reference_facts(entry)
        assert live or not S.reference_present(), "the reference is here: the live comparison must run"
    assert sorted(P.load_fixture()) == sorted(P.ENTRIES)
    assert (len(P.LOOP_SCENES), len(P.TREE_SCENES), len(P.ADAPTER_SCRIPTS)) == (17, 9, 2)


def test_fixture_is_what_the_reference_computes(tmp_path):
    """The committed fixture, byte for byte, from a fresh run of the reference program; its size; the digests of the scenes' inputs."""
    assert os.path.getsize(P.GOLDEN) < 256 * 1024
    for e in P.ENTRIES:
        P.recorded_facts(e)                                             # (asserts the digest of the scene's inputs)
    if P.reference_program():
        import importlib.util
        spec = importlib.util.spec_from_file_location("make_loop_closing_reference", os.path.join(ROOT, "tests", "golden", "make_loop_closing_reference.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        assert open(mod.write(str(tmp_path)), "rb").read() == open(P.GOLDEN, "rb").read()


def test_fixture_and_live_run_say_the_same():
    if not P.reference_program():
        return
    for e in P.ENTRIES:
        M.same_facts(P.recorded_facts(e), P.live_facts(e), e)


def test_reference_program_runs_every_scene_clean_under_the_sanitizers():
    """oracle/_ref/ref_loopclosing_san — the same sources compiled with -fsanitize=address,undefined, a stand-alone program run directly —
    over every scene: no report, and the bytes of the plain build."""
    if not P.reference_program():
        return                                                          # (no reference here: the fixture stands for it)
    assert P.reference_program("ref_loopclosing_san")
    for e in P.ENTRIES:
        mode, blob = P.entry_blob(e)
        assert M.run_reference(mode, blob, "ref_loopclosing_san") == M.run_reference(mode, blob, P.PROGRAM), e


# ---------------------------------------------------------------------------------------------------------------------
# the scenes
# ---------------------------------------------------------------------------------------------------------------------
def test_scenes_show_what_they_are_named_for():
    """Each quirk in the REFERENCE's output: a scene that stopped showing it would leave its test green and empty."""
    def loop(name):
        g, f = P.loop_graph(name), loop_want(name)
        connected = f["connected"].tolist()
        table = P.table_of(g, connected)
        return g, f, connected, table, len(connected)

    def holders(g, table, p):                                           # table indices of the corrected keyframes that hold p
        return [i for i, k in enumerate(table[:g["n_kf"]]) if p in g["slots"][k]]

    for name in P.LOOP_SCENES:                                          # the reference connected exactly the keyframes meant to be corrected
        g, f, connected, table, K = loop(name)
        assert sorted(connected) == list(range(g["n_kf"])) and connected[-1] == g["cur"] and f["after"].tolist()[:3] == [1, 1, 1], name
        assert f["after"][3] == g["spec"]["ids"][g["cur"]] and f["after"][4] == 0 and f["after"][5] == 1            # mLastLoopKFid, GBA over, one big change
    assert [len(loop(n)[2]) for n in ("only_current", "two_keyframes", "sixty_five_keyframes")] == [1, 2, 65]
    g, f, connected, table, K = loop("sixty_five_keyframes")
    assert connected[:-1] != sorted(connected[:-1], key=lambda k: g["spec"]["addrs"][k])          # the vector is not the map's order
    assert np.all(f["corrected_siw"].reshape(K, 8)[:, 7] == 1.07) and len(set(f["corrected_by"].tolist())) > 40
    for name in ("three_holders_ascending", "three_holders_descending"):
        g, f, connected, table, K = loop(name)
        sp = g["spec"]
        h = holders(g, table, sp["mark"])
        assert len(h) == 3 and f["corrected_by"][sp["mark"]] == h[0]                              # the first in pointer order owns the point
        first_in_vector = min((table[i] for i in h), key=connected.index)
        assert first_in_vector != table[h[0]]                                                     # ... and is not the first of the vector
        addrs = [sp["addrs"][k] for k in range(g["n_kf"])]
        assert addrs == sorted(addrs, reverse=name.endswith("descending"))
        assert any(i > h[0] for i in h)                                                           # observers corrected later than the owner
    g, f, connected, table, K = loop("duplicate_slot")
    k = table[f["corrected_by"][g["spec"]["mark"]]]
    assert g["slots"][k].count(g["spec"]["mark"]) == 2
    g, f, connected, table, K = loop("skip")
    done, bad = g["spec"]["marks"]
    assert g["bad"][bad] and g["corrected"][done] and f["corrected_by"][bad] == -1 and f["corrected_by"][done] == -1
    assert all(any(p in g["slots"][k] for k in range(g["n_kf"])) for p in (done, bad)) and np.all(f["pos_out"].reshape(-1, 3)[[done, bad]] == SENT)
    g, f, connected, table, K = loop("null_slots")
    assert g["slots"][0][:2] == [-1, -1] and g["slots"][1][:5] == [-1] * 5
    g, f, connected, table, K = loop("reference_places")
    marks = g["spec"]["marks"]
    owner = int(f["corrected_by"][marks[0]])
    refs = [table.index(g["ref"][p]) for p in marks]
    assert np.all(f["corrected_by"][marks] == owner) and refs[0] == owner and owner < refs[1] < K and refs[2] >= K and owner > 0
    g, f, connected, table, K = loop("outside_observers")
    assert sum(k >= g["n_kf"] for k in g["obs"][g["spec"]["mark"]]) == 4 and f["corrected_by"][g["spec"]["mark"]] >= 0
    g, f, connected, table, K = loop("quaternion_branches")
    assert {LC.quat_branch(g["spec"]["poses"][k]) for k in range(g["n_kf"])} == {0, 1, 2, 3}
    assert loop("scale_one")[1]["corrected_siw"][7] == 1.0 and loop("scale_1_07")[1]["corrected_siw"][7] == 1.07
    assert loop("scale_one")[1]["tiw_out"].tobytes() != loop("scale_1_07")[1]["tiw_out"].tobytes()
    # the loop fusion: Replace over a filled slot, AddMapPoint over an empty one, the slot's own point left alone
    g, f, connected, table, K = loop("fusion")
    m = g["marks"]
    kfs, pts = P.parsed_dump(f, "fusion")
    row = kfs[g["cur"]]["slots"]
    assert f["bad"][m["replaced"]] == 1 and f["replaced"][m["replaced"]] == m["by"] and row[g["matched"].index(m["by"])] == m["by"]
    assert row[m["slot"]] == m["added"] and [g["cur"], m["slot"]] in pts[m["added"]]["obs"] and f["replaced"][m["same"]] == -1 and not f["bad"][m["same"]]
    assert f["found_visible"].reshape(-1, 2)[m["by"]].tolist() == [2, 2]
    # SearchAndFuse: the survivor's descriptor is computed anew between two keyframes' calls; a second Replace of a point already replaced
    g, f, connected, table, K = loop("fuse_repair")
    m = g["marks"]
    order = sorted(range(g["n_kf"]), key=lambda k: g["spec"]["addrs"][k])
    assert f["fuse_kf"].tolist() == order and f["fuse_action"].tolist() == [2, 2, 2]
    met = f["fuse_descriptor"].reshape(-1, 32)
    assert met[0].tobytes() != met[1].tobytes() and f["replaced"][m["victim"]] == g["loop_points"][0]
    twice = g["slots"][m["second"]][g["script"][1][2]]
    assert f["replaced"][twice] == g["loop_points"][1] and f["bad"][twice] == 1                   # replaced by 0, then "by" 1 (MapPoint.cc:241)
    kfs, pts = P.parsed_dump(f, "fuse_repair")
    assert kfs[m["second"]]["slots"][g["script"][1][2]] == g["loop_points"][0]                    # ... but the slot went to loop point 0
    assert f["found_visible"].reshape(-1, 2)[g["loop_points"][1]].tolist() == [2, 2]
    # a loop point that enters the second keyframe through the first keyframe's Replace is passed over there as already found
    g, f, connected, table, K = loop("fuse_enters_by_replace")
    assert f["fuse_action"].tolist() == [2, 1, 3] and g["marks"]["second"] in g["obs"][g["marks"]["victim"]]
    w, at, new_links = f["loop_connections"].tolist(), 0, 0                                       # the fusion tied both sides of the loop together
    while at < len(w):
        new_links += w[at + 1]
        assert all(k >= g["n_kf"] for k in w[at + 2:at + 2 + w[at + 1]])
        at += 2 + w[at + 1]
    assert new_links > 0

    def tree(name):
        sc = LC.tree_scene(name)
        return sc["args"], P.reference_facts("gba." + name)[0], sc["info"]["spec"]

    for run in (0, 1, 2, 40):
        a, f, sp = tree("run_%d" % run)
        assert max(LC.run_lengths(sp), default=0) == run and int(f["in_gba"].sum()) - int(a["in_gba"].sum()) == run and np.all(f["kf_reached"] == 1)
        assert f["after"].tolist() == [1, 1, 1, 1, 1]
    a, f, sp = tree("origin_outside")
    assert a["in_gba"][0] == 0 and f["in_gba"][0] == 0 and f["kf_reached"][0] == 1
    assert f["tcw_out"].reshape(-1, 16)[0].tobytes() == np.asarray(a["tcw_gba"], np.float32).reshape(-1, 16)[0].tobytes()
    assert (f["point_status"] == LR.POINT_REF_OUTSIDE).sum() > 0
    a, f, sp = tree("unreached_reference")
    assert np.all(f["kf_reached"][sp["marks"]] == 0) and f["point_status"][:3].tolist() == [LR.POINT_CARRIED, LR.POINT_REF_OUTSIDE, LR.POINT_CARRIED]
    a, f, sp = tree("two_origins")
    assert a["n_origins"] == 2 and np.all(f["kf_reached"] == 1) and (a["in_gba"] == 0).sum() == 4
    a, f, sp = tree("bad_point")
    assert f["point_status"][3] == LR.POINT_BAD and f["point_status"][4] == LR.POINT_BAD and a["point_in_gba"][4]
    assert tree("points_0")[0]["n_points"] == 0
    assert sum(len(P.loop_graph(n)["pos"]) for n in P.LOOP_SCENES) < 1500


# ---------------------------------------------------------------------------------------------------------------------
# the restatement, the host build and the adapter against the reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", P.LOOP_SCENES)
def test_update_connections_restatement_gives_the_reference_vector(name):
    """mvpCurrentConnectedKFs (:432-437) from covis_restatement's counter and map_graph_restatement's UpdateConnections on the same graph."""
    got, counter = P.restated_connected(name)
    assert got == loop_want(name)["connected"].tolist()
    g = P.loop_graph(name)
    assert all(counter.get(k, 0) < P.TH for k in range(g["n_kf"], g["n_all"]))


@pytest.mark.parametrize("name", P.LOOP_SCENES)
def test_loop_correction_equals_the_reference(prog, adapter_prog, tmp_path, name):
    """The restatement, handed the reference's mvpCurrentConnectedKFs, the host build of the kernels and the adapter over stand-in types,
    fed with the arguments gathered from the graph before the call."""
    want = loop_want(name)
    sc = P.realise_loop(name, want["connected"].tolist())
    a = sc["args"]
    assert P.differing(sc["expect"], want, LOOP_NAMES) == []
    rc, text, got = LC.parse(host_prog.run(prog, tmp_path, "loop", LC.loop_blob(a)), LC.LOOP_OUT, a["n_kf"], a["n_points"])
    assert rc == 0 and text == "" and P.differing(got, want, LOOP_NAMES) == []
    raw = host_prog.run(adapter_prog, tmp_path, "loop", LC.loop_adapter_blob(sc))
    rc, text, got = LC.parse(raw, LC.LOOP_OUT + LC.CALLS, a["n_kf"], a["n_points"])
    assert rc == 0 and got.pop("calls").tolist() == [1] and P.differing(got, want, LOOP_NAMES) == []


@pytest.mark.parametrize("name", P.TREE_SCENES)
def test_global_ba_map_update_equals_the_reference(prog, adapter_prog, tmp_path, name):
    want = P.reference_facts("gba." + name)[0]
    sc = LC.tree_scene(name)
    a = sc["args"]
    assert P.differing(sc["expect"], want, GBA_NAMES) == []
    rc, text, got = LC.parse(host_prog.run(prog, tmp_path, "gba", LC.gba_blob(a)), LC.GBA_OUT, a["n_kf"], a["n_points"])
    assert rc == 0 and text == "" and P.differing(got, want, GBA_NAMES) == []
    raw = host_prog.run(adapter_prog, tmp_path, "gba", LC.gba_adapter_blob(sc))
    rc, text, got = LC.parse(raw, LC.GBA_OUT + LC.CALLS, a["n_kf"], a["n_points"])
    assert rc == 0 and got.pop("calls").tolist() == [1] and P.differing(got, want, GBA_NAMES) == []


@pytest.mark.parametrize("name", P.LOOP_SCENES)
def test_loop_fusion_search_and_fuse_and_loop_connections_equal_the_reference(name):
    """What :530-542, SearchAndFuse (the scripted matcher; the module's docstring says what that leaves unpinned) and :553-579 leave."""
    want = loop_want(name)
    got = P.restated_fusion(name, want["connected"].tolist())
    keys = ("bad", "replaced", "found_visible", "has_descriptor", "descriptor", "fuse_kf", "fuse_action", "fuse_descriptor", "loop_connections")
    M.same_facts(want, got, name, keys=keys)
    if "dump" in want:                                                  # (kept whole for the fuse scenes; every scene when the run is live)
        kfs, pts = P.parsed_dump(want, name)
        assert [k["slots"] for k in kfs] == got["slots"] and [p["obs"] for p in pts] == got["obs"] and [p["n_obs"] for p in pts] == got["n_obs"]
    assert name not in P.FUSE_SCENES or "dump" in want
    g = P.loop_graph(name)
    order = sorted(range(g["n_kf"]), key=lambda k: g["spec"]["addrs"][k])
    cor = want["corrected_siw"].reshape(-1, 8)                          # Converter::toCvMat(g2oScw) of every call (:619): [s R | t]
    scw = np.tile(np.eye(4, dtype=np.float32), (len(order), 1, 1))
    for i in range(len(order)):
        scw[i, :3, :3] = (cor[i, 7] * EG.quat_to_matrix(cor[i, :4])).astype(np.float32)
        scw[i, :3, 3] = cor[i, 4:7].astype(np.float32)
    M.same_facts(want, {"fuse_scw": scw.ravel()}, name)


def adapter_against(want, exe, tmp_path, name):
    """SIVO::SearchAndFuse (the adapter's copy) and the loop of single-keyframe Fuse calls (the other copy) of
    tests/fuse_batch_adapter_prog.cpp against the graph the reference's SearchAndFuse left under the scene's script."""
    w = AC.scene(name)
    a, b, _ = AC.parse(host_prog.run(exe, tmp_path, "loop", AC.blob(w)), w)
    script, actions = P.ADAPTER_SCRIPTS[name], P.ADAPTER_ACTIONS[name]
    assert want["fuse_kf"].tolist() == w.targets and want["fuse_action"].tolist() == actions
    for dump in (a, b):
        adds, replaces = P.adapter_landings(dump, name)                 # the program's matcher chose what the script says
        assert adds == [land for land, act in zip(script, actions) if act == 3]
        assert replaces == [(w.kfs[k]["keys"][slot]["slot"], w.list[i]) for (k, i, slot), act in zip(script, actions) if act == 2]
        assert P.adapter_graph_differs(dump, want, name) == []


@pytest.mark.parametrize("name", list(P.ADAPTER_SCRIPTS))
def test_search_and_fuse_adapter_leaves_the_reference_graph(tmp_path, name):
    """The host build of tests/fuse_batch_adapter_prog.cpp on its two loop scenes: slots, observations, Observations(), bad flags,
    replaced-by links, found / visible and descriptors as the reference's SearchAndFuse, Replace and ComputeDistinctiveDescriptors leave
    them.  Which key each list point lands on is the script's (ORBmatcher::Fuse is not part of the reference build); the event log shows
    that the program's matcher chose the same keys."""
    adapter_against(P.reference_facts("fuse." + name)[0], host_prog.build("fuse_batch_adapter_prog", tmp_path), tmp_path, name)


# ---------------------------------------------------------------------------------------------------------------------
# the device against the recorded facts (tests/ and the fixture only)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lc():
    from sivo_amd import loop_closing
    return loop_closing


@pytest.mark.gpu
@pytest.mark.parametrize("name", P.LOOP_SCENES)
def test_device_loop_correction_equals_the_reference(lc, name):
    """sivo_loop_correct through the C ABI and through sivo_amd/loop_closing.py."""
    import test_gpu_loop_correct as GL
    want = P.recorded_facts("loop." + name)
    a = P.realise_loop(name, want["connected"].tolist())["args"]
    got = GL.loop_abi(lc, a)
    assert P.differing(got, want, LOOP_NAMES) == []
    still = got["corrected_by"] < 0
    assert np.all(got["pos_out"][still] == SENT) and np.all(got["normal"][still] == SENT) and np.all(got["flags"][still] == 255)
    w = GL.loop_wrapper(lc, a)
    assert P.differing(w, want, [n for n in LOOP_NAMES if n != "corrected_by"]) == [] and np.array_equal(w["corrected_by"], want["corrected_by"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", P.TREE_SCENES)
def test_device_global_ba_map_update_equals_the_reference(lc, name):
    """sivo_gba_propagate through the C ABI and through sivo_amd/loop_closing.py."""
    import test_gpu_loop_correct as GL
    want = P.recorded_facts("gba." + name)
    a = LC.tree_scene(name)["args"]
    assert P.differing(GL.gba_abi(lc, a), want, GBA_NAMES) == []
    assert P.differing(GL.gba_wrapper(lc, a), want, GBA_NAMES) == []


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(P.ADAPTER_SCRIPTS))
def test_device_search_and_fuse_adapter_leaves_the_reference_graph(tmp_path, name):
    """tests/fuse_batch_adapter_prog.cpp linked against the product library: both copies run on the device."""
    exe = host_prog.build("fuse_batch_adapter_prog", tmp_path, link_lib=True, defines=("FUSE_BATCH_ON_LIBRARY",))
    adapter_against(P.recorded_facts("fuse." + name), exe, tmp_path, name)
