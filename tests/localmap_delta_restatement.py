"""The yardstick of sivo_localmap_apply: what a set of tables (the dict of tests/localmap_restatement.export_tables) becomes under a delta
of replaced and appended rows, in LIST-OF-ROWS form — every CSR table is taken apart into a Python list of rows, rows are replaced or
appended, and the lists are flattened again.  No marks, no lengths, no prefix sums over blocks: nothing of how the library does it.

A delta is a dict: n_kf, n_points (the sizes after it), point_rows = dict(idx, obs_off, obs_kf, bad), kf_rows = dict(idx, bad, parent,
slot_off, slot_point, covis_off, covis_kf, child_off, child_kf), kf_order (None: the old order, the appended keyframes behind it)."""
import numpy as np

from localmap_restatement import csr


def rows_of(off, val):
    return [list(map(int, val[int(off[i]):int(off[i + 1])])) for i in range(len(off) - 1)]


def full_order(t):
    """kf_order as a handle stores it: the identity where the tables carry None."""
    return np.arange(t["n_kf"], dtype=np.int32) if t["kf_order"] is None else np.asarray(t["kf_order"], np.int32)


def apply(tables, delta):
    """The tables after the delta; kf_order always as an array."""
    K0, P0, K1, P1 = tables["n_kf"], len(tables["point_bad"]), delta["n_kf"], delta["n_points"]
    pr, kr = delta["point_rows"], delta["kf_rows"]
    obs = rows_of(tables["obs_off"], tables["obs_kf"]) + [None] * (P1 - P0)
    point_bad = list(map(int, tables["point_bad"])) + [None] * (P1 - P0)
    new_obs = rows_of(pr["obs_off"], pr["obs_kf"])
    for j, p in enumerate(map(int, pr["idx"])):
        obs[p], point_bad[p] = new_obs[j], int(bool(pr["bad"][j]))
    kf = {}
    for name, inner in (("slot", "slot_point"), ("covis", "covis_kf"), ("child", "child_kf")):
        rows = rows_of(tables[name + "_off"], tables[inner]) + [None] * (K1 - K0)
        new = rows_of(kr[name + "_off"], kr[inner])
        for j, k in enumerate(map(int, kr["idx"])):
            rows[k] = new[j]
        kf[name] = rows
    kf_bad = list(map(int, tables["kf_bad"])) + [None] * (K1 - K0)
    parent = list(map(int, tables["parent"])) + [None] * (K1 - K0)
    for j, k in enumerate(map(int, kr["idx"])):
        kf_bad[k], parent[k] = int(bool(kr["bad"][j])), int(kr["parent"][j])
    assert None not in obs and None not in point_bad and None not in kf_bad and all(None not in kf[n] for n in kf), "a new row is not listed"
    order = list(map(int, full_order(tables))) + list(range(K0, K1)) if delta["kf_order"] is None else list(map(int, delta["kf_order"]))
    out = dict(n_kf=K1, point_bad=np.array(point_bad, np.uint8), kf_bad=np.array(kf_bad, np.uint8), parent=np.array(parent, np.int32),
               kf_order=np.array(order, np.int32))
    out["obs_off"], out["obs_kf"] = csr(obs, np.int32)
    out["slot_off"], out["slot_point"] = csr(kf["slot"], np.int32)
    out["covis_off"], out["covis_kf"] = csr(kf["covis"], np.int32)
    out["child_off"], out["child_kf"] = csr(kf["child"], np.int32)
    return out
