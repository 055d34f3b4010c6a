"""CPU: tests/gate_restatement.py against the oracle's gate (orc_entropy_gate / orc_check_semantics) on the edge scene — the
borders' truncation, every kind of depth, Z = 0, a singular state covariance — at the project's bound for the gate,
rtol = atol = 1e-12, NaN where the other is NaN, the decisions equal.  No device."""
import numpy as np

import gate_restatement as GR


def _close(a, b):
    assert np.array_equal(np.isnan(a), np.isnan(b))
    f = ~np.isnan(a)
    np.testing.assert_allclose(a[f], b[f], rtol=1e-12, atol=1e-12)


def _args(sc, Sx=None):
    return (sc["kps"], sc["depth"], sc["xyz"], sc["entropy"], sc["Sx"] if Sx is None else Sx, GR.FX, GR.FY, GR.BL, sc["ls2"])


def test_scene_covers_the_edges():
    sc = GR.build_scene()
    kps, depth, ent = sc["kps"], sc["depth"], sc["entropy"]
    rows, cols = ent.shape
    assert (rows, cols) == (7, 13) and len(kps) == 203 and set(kps["octave"].tolist()) == set(range(8))
    mi, red, acc = GR.gate(*_args(sc), sc["th"])
    assert np.abs(red[np.isfinite(red)] - sc["th"]).min() > 1e-9 and 40 < acc.sum() < 120
    at = lambda x, y: int(np.nonzero((kps["x"] == np.float32(x)) & (kps["y"] == np.float32(y)))[0][0])
    # truncation: -0.25 reads column / row 0, cols - 0.001 the last column, -1 and cols are outside
    i = at(-0.25, -0.25); assert mi[i] != 0 and red[i] == mi[i] - ent[0, 0]
    i = at(cols - 0.001, rows - 0.001); assert red[i] == mi[i] - ent[rows - 1, cols - 1]
    i = at(0.999, rows - 1); assert red[i] == mi[i] - ent[rows - 1, 0]
    i = at(cols - 1, 0.0); assert red[i] == mi[i] - ent[0, cols - 1]
    for x, y in ((-1.0, 0.0), (0.0, -1.0), (cols, 0.0), (0.0, rows), (cols + 5, 3.5), (6.5, rows + 5)):
        i = at(x, y); assert mi[i] == 0 and red[i] == 0 and acc[i] == 0
    # depth: 0, -0, negative and NaN fail; a denormal and inf pass
    for d in GR.DEPTHS:
        sel = (depth.view(np.uint32) == np.float32(d).view(np.uint32)) & (np.arange(len(kps)) >= 80)
        assert sel.sum() >= 3 and ((mi[sel] != 0) == bool(d > 0)).all(), d
    # Z = 0: J = 0 and the joint covariance is block diagonal, det S9 = det Sx sigma2^3 = det Sx det Sz: the information is 0 up to
    # the one rounding by which sigma2 (sigma2 sigma2) of the cofactor form and (sigma2 sigma2) sigma2 of the LU's pivot product
    # may differ: 0.5 log2(1 +- 2^-52) = 1.6e-16
    z0 = (sc["xyz"][:, 2] == 0) & (depth > 0)
    assert z0.sum() == 4 and (np.abs(mi[z0]) <= 2.0 ** -52).all() and (mi[z0] == 0).any()
    np.testing.assert_allclose(red[z0], -ent[kps["y"][z0].astype(int), kps["x"][z0].astype(int)], rtol=0, atol=2.0 ** -52)


def test_restatement_equals_oracle(oracle):
    sc = GR.build_scene()
    for th in (-1e9, 1e9, sc["th"]):
        o = oracle.entropy_gate(*_args(sc), th)
        r = GR.gate(*_args(sc), th)
        _close(r[0], o[0]); _close(r[1], o[1])
        assert np.array_equal(r[2], o[2])
        o = oracle.check_semantics(*_args(sc)[:4], sc["confidence"], sc["classes"], *_args(sc)[4:], th, sc["th_conf"])
        r = GR.gate(*_args(sc), th, sc["confidence"], sc["classes"], sc["th_conf"])
        _close(r[0], o[0]); _close(r[1], o[1])
        assert np.array_equal(r[2], o[2])
    assert 10 < (r[2] != 255).sum() < 203 and set(np.unique(r[2])) - {255} <= set(range(9))


def test_singular_state_covariance_gives_nan(oracle):
    """det Sx = 0 and det S9 = 0: 0.5 log2(0 * det Sz / 0) is NaN.  `NaN > th` is false, the gate rejects; `NaN < th` is false too,
    CheckSemantics keeps the class."""
    sc = GR.build_scene()
    Z = np.zeros((6, 6))
    for fn in (lambda: oracle.entropy_gate(*_args(sc, Z), sc["th"]), lambda: GR.gate(*_args(sc, Z), sc["th"])):
        mi, red, acc = fn()
        live = mi != 0
        assert live.sum() > 100 and np.isnan(mi[live]).all() and np.isnan(red[live]).all() and (acc == 0).all()
    o = oracle.check_semantics(*_args(sc, Z)[:4], sc["confidence"], sc["classes"], *_args(sc, Z)[4:], sc["th"], sc["th_conf"])
    r = GR.gate(*_args(sc, Z), sc["th"], sc["confidence"], sc["classes"], sc["th_conf"])
    assert np.array_equal(np.isnan(o[0]), np.isnan(r[0])) and np.array_equal(o[2], r[2])
    live = np.isnan(r[0])
    rr, cc = sc["kps"]["y"][live].astype(int), sc["kps"]["x"][live].astype(int)
    assert live.sum() > 20 and np.array_equal(r[2][live], sc["classes"][rr, cc]) and (r[2][~live] == 255).all()
