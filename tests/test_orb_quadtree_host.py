"""The device quadtree keypoint distribution without a device: the round-parallel formulation (tests/orb_quadtree_restatement.py), the
kernel's own steps walked on the host (tests/orb_quadtree_prog.cpp over sivo_amd/csrc/orb_quadtree_math.hpp), the library's host routine
(orb.distribute_octtree) and the oracle agree byte for byte on every scene, every scene takes the branch it is named for, and every
refusal of sivo_orb_distribute_batch_dev comes with its message before any device is touched."""
import ctypes as C
import os

import numpy as np
import pytest

import host_prog
import orb_quadtree_cases as Q
import orb_quadtree_restatement as R
from sivo_amd import _lib, orb

NAMES = list(Q.SCENES)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return host_prog.build("orb_quadtree_prog", tmp_path_factory.mktemp("orb_quadtree_prog"))


@pytest.fixture(scope="module")
def host_lists():
    """orb.distribute_octtree (orb_host.cpp) on every scene, computed once."""
    return {name: orb.distribute_octtree(*Q.SCENES[name]) for name in NAMES}


# what the report of the restatement (rep), the kept keys (out) and the scene's keys must show for the scene to be the one its name says
BRANCH = {
    "empty": lambda rep, out, keys: len(out) == 0 and rep["rounds"] == 0,
    "one": lambda rep, out, keys: len(out) == 1 and rep["rounds"] == 1 and rep["ended_unchanged"],
    "coincident_two": lambda rep, out, keys: len(out) == 1 and rep["ended_unchanged"] and out["response"][0] == 200,
    "one_root": lambda rep, out, keys: rep["n_ini"] == 3 and int(keys["x"].max()) < 100,
    "n_ini_2p5": lambda rep, out, keys: rep["n_ini"] == 3,
    "n_ini_under_1p5": lambda rep, out, keys: rep["n_ini"] == 1,
    "root_box_quirk": lambda rep, out, keys: rep["n_ini"] == 3 and {327, 328, 329, 656, 657, 658} <= set(keys["x"].astype(int)),
    "first_round_target_1": lambda rep, out, keys: rep["rounds"] == 1 and rep["passes"] == 0 and len(out) == 4,
    "first_round_target_2": lambda rep, out, keys: rep["rounds"] == 1 and rep["passes"] == 0 and len(out) == 4,
    "first_round_target_3": lambda rep, out, keys: rep["rounds"] == 1 and rep["passes"] == 0 and len(out) == 4,
    "first_round_target_4": lambda rep, out, keys: rep["rounds"] == 1 and rep["passes"] == 0 and len(out) == 4,
    "target_above_count": lambda rep, out, keys: len(out) == len(keys) and rep["ended_unchanged"],
    "close_phase_mid_pass": lambda rep, out, keys: rep["passes"] >= 1 and any(s < g - 1 for s, g in zip(rep["stops"], rep["grown"])),
    "close_phase_tie": lambda rep, out, keys: rep["passes"] >= 1 and rep["tie_in_grown"],
    "close_phase_three_passes": lambda rep, out, keys: rep["passes"] >= 3,
    "odd_extents_one_pixel_cells": lambda rep, out, keys: rep["ended_unchanged"] and len(out) == 33 * 37 and rep["rounds"] + rep["passes"] >= 6,
    "response_ties": lambda rep, out, keys: set(keys["response"].astype(int)) == {0, 1} and len(out) < len(keys) // 4,
    "larger_than_workgroup": lambda rep, out, keys: len(keys) > 5 * Q.THREADS and len(out) >= 434,
    "many_cells": lambda rep, out, keys: Q.MAX_CELLS - 3 <= len(out) <= Q.MAX_CELLS,
}
for _n in (63, 64, 65, 255, 256, 257):
    BRANCH["count_%d" % _n] = lambda rep, out, keys, _n=_n: len(keys) == _n and len(out) >= max(_n // 3, 8)
for _n in (Q.LDS_CANDIDATES, Q.LDS_CANDIDATES + 1):
    BRANCH["count_%d" % _n] = lambda rep, out, keys, _n=_n: len(keys) == _n and len(out) >= 434


def test_every_scene_names_its_branch():
    assert set(BRANCH) == set(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_host_routine_and_oracle(oracle, host_lists, name):
    keys, x0, x1, y0, y1, target = Q.SCENES[name]
    out, rep = R.distribute(keys, x0, x1, y0, y1, target)
    assert out.tobytes() == host_lists[name].tobytes()
    assert out.tobytes() == oracle.distribute_octtree(keys, x0, x1, y0, y1, target).tobytes()
    assert BRANCH[name](rep, out, keys), rep
    # the bounds the kernel's tables rest on
    assert len(out) <= max(target + 3, 4 * rep["n_ini"]) and rep["rounds"] + rep["passes"] <= 26


def test_the_tie_rule_matters_in_the_tie_scene(host_lists):
    """Equal sizes in `grown` are split later-created first (orb_host.cpp); with the rule flipped the tie scene gives another list."""
    keys, x0, x1, y0, y1, target = Q.SCENES["close_phase_tie"]
    flipped, rep = R.distribute(keys, x0, x1, y0, y1, target, later_wins_ties=False)
    assert rep["tie_in_grown"] and flipped.tobytes() != host_lists["close_phase_tie"].tobytes()


def test_walked_kernel_steps_equal_host_routine(prog, tmp_path, host_lists):
    """The kernel's per-candidate and per-cell bodies, one item after the other, on every scene — one set per run and all in one."""
    for names in [[n] for n in NAMES] + [NAMES, Q.BATCH]:
        for name, (status, kept, rounds, passes, stop) in zip(names, Q.run_prog(prog, tmp_path, names)):
            assert status == 0, name
            assert kept.tobytes() == host_lists[name].tobytes(), name


def test_walked_kernel_steps_report_the_restatement_s_schedule(prog, tmp_path):
    for name, (status, kept, rounds, passes, stop) in zip(NAMES, Q.run_prog(prog, tmp_path, NAMES)):
        keys, x0, x1, y0, y1, target = Q.SCENES[name]
        rep = R.distribute(keys, x0, x1, y0, y1, target)[1]
        # (the walk counts a pass with nothing left to split as no pass)
        assert (rounds, passes) == (rep["rounds"], rep["passes"] - (1 if rep["grown"][-1:] == [0] else 0)), name
        if rep["stops"] and rep["grown"][-1] > 0:
            assert stop == rep["stops"][-1], name


def test_sanitizer_build_of_the_walk_agrees(prog, tmp_path, tmp_path_factory):
    """The same program under -fsanitize=address,undefined (its own main, nothing preloaded): every table has the kernel's size, so a
    step that leaves its table is a report.  The same bytes as the plain build on every scene."""
    san_dir = tmp_path_factory.mktemp("orb_quadtree_prog_san")
    if not host_prog.sanitizer_runtime_present(san_dir):
        pytest.skip("the sanitizer runtime (libasan / libubsan) is not installed: a trivial main does not link with -fsanitize")
    san = host_prog.build("orb_quadtree_prog", san_dir, sanitize=True)
    blob = Q.blob_of(NAMES)
    assert host_prog.run(prog, tmp_path, "run", blob) == host_prog.run(san, tmp_path, "run", blob)


def test_a_bound_above_the_table_is_a_status_not_a_list(prog, tmp_path):
    Q.SCENES["_over"] = Q.scene(Q.distinct(11, 3000, 1000, 320), 1000, 320, Q.MAX_CELLS - 2)
    try:
        (status, kept, *_), = Q.run_prog(prog, tmp_path, ["_over"])
    finally:
        del Q.SCENES["_over"]
    assert status == 1 and len(kept) == 0


# ---- the entry point's refusals: all of them come before any device is touched ------------------------------------------------------------
def _call(sets, out_capacity=None, device=0, bend=None):
    """sivo_orb_distribute_batch_dev on [(keys, x0, x1, y0, y1, target)]; bend(args) may change the argument list.  (rc, message, out_off)."""
    L = _lib.lib()
    off = np.zeros(len(sets) + 1, np.int64)
    for i, s in enumerate(sets):
        off[i + 1] = off[i] + len(s[0])
    keys = np.concatenate([np.ascontiguousarray(s[0], orb.KP_DTYPE) for s in sets]) if sets else np.zeros(0, orb.KP_DTYPE)
    cols = [np.array([s[i] for s in sets], np.int32) for i in range(1, 6)]
    cap = int(off[-1]) if out_capacity is None else out_capacity
    out = np.zeros(max(cap, 1), orb.KP_DTYPE)
    out_off = np.full(len(sets) + 1, -7, np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    args = [len(sets), p(off), p(keys), *[p(c) for c in cols], C.c_int64(cap), p(out), p(out_off), device]
    if bend:
        bend(args)
    rc = L.sivo_orb_distribute_batch_dev(*args)
    return rc, L.sivo_last_error().decode(), out_off


def _bent(name, field, value, index=0):
    keys, *rest = Q.SCENES[name]
    keys = keys.copy()
    keys[field][index] = value
    return (keys, *rest)


INVALID = 1
CAPACITY = 5


def refused_calls():
    good = Q.SCENES["count_65"]
    k, x0, x1, y0, y1, t = good
    null = lambda i: (lambda a: a.__setitem__(i, None))
    return [
        ("x is not an integer", dict(sets=[_bent("count_65", "x", 3.5)]), INVALID, "key 0 of set 0"),
        ("x is negative", dict(sets=[good, _bent("count_65", "x", -1.0, 7)]), INVALID, "key 7 of set 1"),
        ("x is outside the region", dict(sets=[_bent("count_65", "x", 300.0)]), INVALID, "inside the region"),
        ("y is outside the region", dict(sets=[_bent("count_65", "y", 100.0)]), INVALID, "inside the region"),
        ("y is not an integer", dict(sets=[_bent("count_65", "y", 0.25)]), INVALID, "must be integers"),
        ("x is not a number", dict(sets=[_bent("count_65", "x", np.nan)]), INVALID, "key 0 of set 0"),
        ("the response is 256", dict(sets=[_bent("count_65", "response", 256.0)]), INVALID, "response an integer in [0, 256)"),
        ("the response is a fraction", dict(sets=[_bent("count_65", "response", 0.5)]), INVALID, "response an integer in [0, 256)"),
        ("an empty region in x", dict(sets=[(k, x0, x0, y0, y1, t)]), INVALID, "empty region (set 0)"),
        ("an empty region in y", dict(sets=[good, (k[:0], x0, x1, y1, y0, t)]), INVALID, "empty region (set 1)"),
        ("an extent above 4096", dict(sets=[(k, 0, 4097, y0, y1, t)]), INVALID, "extents up to 4096"),
        ("round(W / H) < 1", dict(sets=[(k[:0], 0, 49, 0, 100, t)]), INVALID, "round(W / H) < 1"),
        ("n_features < 1", dict(sets=[(k, x0, x1, y0, y1, 0)]), INVALID, "n_features < 1 (set 0)"),
        ("offsets that do not start at 0", dict(sets=[good], bend=lambda a: a.__setitem__(1, np.array([1, 65], np.int64).ctypes.data_as(C.c_void_p))), INVALID,
         "does not start at 0"),
        ("offsets that decrease", dict(sets=[good, good], bend=lambda a: a.__setitem__(1, np.array([0, 65, 64], np.int64).ctypes.data_as(C.c_void_p))), INVALID,
         "set_off decreases at set 1"),
        ("keys is NULL", dict(sets=[good], bend=null(2)), INVALID, "keys is NULL with 65 keys"),
        ("set_off is NULL", dict(sets=[good], bend=null(1)), INVALID, "NULL array"),
        ("min_x is NULL", dict(sets=[good], bend=null(3)), INVALID, "NULL array"),
        ("n_features is NULL", dict(sets=[good], bend=null(7)), INVALID, "NULL array"),
        ("out_off is NULL", dict(sets=[good], bend=null(10)), INVALID, "NULL array"),
        ("out is NULL", dict(sets=[good], bend=null(9)), INVALID, "out is NULL"),
        ("a negative n_sets", dict(sets=[good], bend=lambda a: a.__setitem__(0, -1)), INVALID, "n_sets is negative"),
        ("a cell bound above the table", dict(sets=[good, (k, x0, x1, y0, y1, Q.MAX_CELLS - 2)]), CAPACITY,
         "set 1 can reach max(n_features + 3, 4 * n_ini) = %d cells, the kernel's table holds %d" % (Q.MAX_CELLS + 1, Q.MAX_CELLS)),
    ]


@pytest.mark.parametrize("what,kw,code,message", refused_calls(), ids=[c[0] for c in refused_calls()])
def test_refusals_come_with_their_message_and_without_a_device(what, kw, code, message):
    rc, text, out_off = _call(device=63, **kw)              # (no such device: a call that reached it would say so instead)
    assert rc == code and message in text, (what, rc, text)


def test_no_sets_and_only_empty_sets_launch_nothing():
    rc, text, out_off = _call([], device=63)
    assert rc == 0 and out_off[0] == 0
    rc, text, out_off = _call([Q.SCENES["empty"], Q.SCENES["empty"]], device=63)
    assert rc == 0 and list(out_off) == [0, 0, 0]
    # with keys the call does reach for its device
    rc, text, out_off = _call([Q.SCENES["one"]], device=63)
    assert rc == 2 and "device 63 is not available" in text


def test_python_entry_points_refuse_like_the_library():
    with pytest.raises(Exception, match="n_features < 1"):
        orb.distribute_octtree_dev(Q.SCENES["one"][0], 16, 216, 16, 80, 0)
    with pytest.raises(Exception, match="empty region"):
        orb.distribute_octtree_batch_dev([Q.SCENES["one"][0]], [16], [16], [16], [80], [40])
    assert [len(o) for o in orb.distribute_octtree_batch_dev([Q.SCENES["empty"][0]] * 2, [16] * 2, [216] * 2, [16] * 2, [80] * 2, [40] * 2)] == [0, 0]


def test_launch_mode_setter_refuses_a_null_handle():
    L = _lib.lib()
    assert L.sivo_orb_set_launch_mode(None, 31) == INVALID and "null handle" in L.sivo_last_error().decode()


def test_the_kernel_is_part_of_the_library_and_the_header():
    root = host_prog.ROOT
    mk = open(os.path.join(root, "sivo_amd", "csrc", "Makefile")).read()
    assert " orb_quadtree.hip" in mk.split("SRCS =")[1].splitlines()[0]
    header = open(os.path.join(root, "include", "sivo_hip.h")).read()
    assert "int sivo_orb_distribute_batch_dev(int n_sets, const int64_t *set_off" in header
    assert _lib.lib().sivo_orb_distribute_batch_dev.argtypes is not None
