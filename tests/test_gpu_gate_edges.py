"""GPU: entropy_gate_kernel (sivo_amd/csrc/select.hip) through every entry point against tests/gate_restatement.py on the edge
scene: a 7 x 13 map with all entries distinct, 203 keys on and around every border, every kind of depth, Z = 0, a singular
state covariance, exact equality with the threshold, the class edge 8 / 9, confidence == th, a growing staging buffer, octaves
outside the table.

Mutual information and reduction are asserted within the project's bound for the gate, rtol = atol = 1e-12 (the device's log2
and libm's are not the same function).  Largest distance measured on an MI355X on the edge scene, in ulps of the restatement's
value (a record, not an assertion; the test prints it): MI 0 ulp, reduction 0 ulp — on the 203 keys of the scene and on the
65 keys of the 352 x 1024 map the device's values were the restatement's, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import gate_restatement as GR
from sivo_amd import selection
from sivo_amd._lib import SivoError, check, lib

pytestmark = pytest.mark.gpu
K = (GR.FX, GR.FY, GR.BL)


@pytest.fixture(scope="module")
def sc():
    return GR.build_scene()


def _gate(sc, th, Sx=None, kps=None):
    return selection.entropy_gate(sc["kps"] if kps is None else kps, sc["depth"], sc["xyz"], sc["entropy"], sc["Sx"] if Sx is None else Sx, *K, sc["ls2"], th)


def _sem(sc, th, th_conf=None, Sx=None, classes=None, confidence=None, kps=None):
    return selection.check_semantics(sc["kps"] if kps is None else kps, sc["depth"], sc["xyz"], sc["entropy"],
                                     sc["confidence"] if confidence is None else confidence, sc["classes"] if classes is None else classes,
                                     sc["Sx"] if Sx is None else Sx, *K, sc["ls2"], th, sc["th_conf"] if th_conf is None else th_conf)


def _restated(sc, th, semantics=False, Sx=None, **kw):
    extra = (kw.get("confidence", sc["confidence"]), kw.get("classes", sc["classes"]), kw.get("th_conf", sc["th_conf"])) if semantics else ()
    return GR.gate(kw.get("kps", sc["kps"]), sc["depth"], sc["xyz"], sc["entropy"], sc["Sx"] if Sx is None else Sx, *K, sc["ls2"], th, *extra)


def _ulps(got, want):
    f = np.isfinite(want) & (want != 0)
    return float((np.abs(got[f] - want[f]) / np.spacing(np.abs(want[f]))).max()) if f.any() else 0.0


def _compare(got, want, th, void):
    mi, red, acc = got
    rmi, rred, racc = want
    assert np.array_equal(np.isnan(mi), np.isnan(rmi)) and np.array_equal(np.isnan(red), np.isnan(rred))
    f = ~np.isnan(rmi)
    print(f"[gate] n {len(mi)}: largest distance MI {_ulps(mi, rmi):.2f} ulp, reduction {_ulps(red, rred):.2f} ulp")
    np.testing.assert_allclose(mi[f], rmi[f], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(red[f], rred[f], rtol=1e-12, atol=1e-12)
    rejected = (rmi == 0) & (rred == 0) & (racc == void)              # (a Z = 0 key may have MI == 0 and is not among them: its reduction is not 0)
    assert (mi[rejected] == 0).all() and (red[rejected] == 0).all() and (acc[rejected] == void).all()
    with np.errstate(invalid="ignore"):
        far = ~(np.abs(rred - th) <= 1e-9)                            # NaN keys are decided too
    assert far.all()                                                  # the scene's threshold excludes no key
    assert np.array_equal(acc[far], racc[far])


def test_gate_on_the_edge_scene(sc):
    for th in (sc["th"], -1e9):
        _compare(_gate(sc, th), _restated(sc, th), th, 0)
    acc = _gate(sc, sc["th"])[2]
    assert 40 < acc.sum() < 120


def test_check_semantics_on_the_edge_scene(sc):
    for th in (sc["th"], -1e9):
        _compare(_sem(sc, th), _restated(sc, th, semantics=True), th, 255)
    det = _sem(sc, -1e9)[2]
    assert 10 < (det != 255).sum() < 203 and set(np.unique(det)) - {255} <= set(range(9))


def test_singular_state_covariance(sc):
    """MI is NaN on both sides; the gate rejects (`NaN > th`), CheckSemantics keeps the class (`NaN < th`)."""
    Z = np.zeros((6, 6))
    g, r = _gate(sc, sc["th"], Sx=Z), _restated(sc, sc["th"], Sx=Z)
    assert np.isnan(r[0]).sum() > 100 and np.array_equal(np.isnan(g[0]), np.isnan(r[0])) and np.array_equal(np.isnan(g[1]), np.isnan(r[1]))
    assert (g[2] == 0).all() and (g[0][~np.isnan(r[0])] == 0).all()
    g, r = _sem(sc, sc["th"], Sx=Z), _restated(sc, sc["th"], semantics=True, Sx=Z)
    assert np.isnan(r[0]).sum() > 20 and np.array_equal(np.isnan(g[0]), np.isnan(r[0])) and np.array_equal(g[2], r[2])
    assert (g[2][np.isnan(r[0])] != 255).all()


def test_equality_with_the_threshold(sc):
    """The device's own reduction of a finite key as the threshold: the gate (`>`) rejects at equality and accepts one float below,
    CheckSemantics (`<` rejects) keeps the class at equality and drops it one float above.  Nothing here depends on log2."""
    mi0, red0, acc0 = _gate(sc, -1e9)
    _, reds0, det0 = _sem(sc, -1e9)
    live = np.nonzero((det0 != 255) & np.isfinite(red0) & (red0 != 0))[0]
    assert len(live) > 10
    for i in live[:3]:
        t = float(red0[i])
        assert reds0[i] == red0[i] and acc0[i] == 1
        for th, want_gate, want_class in ((t, 0, det0[i]), (np.nextafter(t, -np.inf), 1, det0[i]), (np.nextafter(t, np.inf), 0, 255)):
            _, red, acc = _gate(sc, float(th))
            _, reds, det = _sem(sc, float(th))
            assert np.array_equal(red.view(np.uint64), red0.view(np.uint64)) and np.array_equal(reds.view(np.uint64), reds0.view(np.uint64))
            assert acc[i] == want_gate and det[i] == want_class, (i, th)


def test_class_and_confidence_edges(sc):
    kps, ent = sc["kps"], sc["entropy"]
    rows, cols = ent.shape
    base = _sem(sc, -1e9)
    i = int(np.nonzero(base[2] != 255)[0][0])
    r, c = int(kps["y"][i]), int(kps["x"][i])
    for cls, want in ((8, 8), (9, 255), (0, 0), (255, 255)):            # TERRAIN is the last static class
        m = sc["classes"].copy(); m[r, c] = cls
        got = _sem(sc, -1e9, classes=m)
        assert got[2][i] == want and (got[0][i] != 0) == (want != 255)
    conf = sc["confidence"][r, c]
    assert _sem(sc, -1e9, th_conf=float(conf))[2][i] == base[2][i]                                    # confidence == th passes
    assert _sem(sc, -1e9, th_conf=float(np.nextafter(conf, np.inf)))[2][i] == 255
    m = sc["confidence"].copy(); m[r, c] = np.nextafter(sc["th_conf"], -np.inf)                       # one float below th
    assert _sem(sc, -1e9, confidence=m)[2][i] == 255
    m[r, c] = sc["th_conf"]
    assert _sem(sc, -1e9, confidence=m)[2][i] == base[2][i]
    # the class and confidence lookups at the four corners: each corner its own class, confidence on / below the threshold
    corners = [(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1)]
    k4 = kps[:4].copy()
    k4["x"] = [0.5, cols - 0.5, 0.5, cols - 0.5]; k4["y"] = [0.5, 0.5, rows - 0.5, rows - 0.5]
    cm = np.full((rows, cols), 9, np.uint8); fm = np.full((rows, cols), 0.1)
    for j, (rr, cc) in enumerate(corners):
        cm[rr, cc] = 2 * j + 1; fm[rr, cc] = 0.7 if j != 2 else 0.5
    sub = dict(sc, kps=k4, depth=np.ones(4, np.float32), xyz=sc["xyz"][:4])
    got = _sem(sub, -1e9, th_conf=0.6, classes=cm, confidence=fm)
    assert got[2].tolist() == [1, 3, 255, 7]
    np.testing.assert_allclose(got[1], got[0] - np.array([ent[rr, cc] for rr, cc in corners]) * (got[2] != 255), rtol=0, atol=1e-12)


def _tiled(sc, n):
    rep = -(-n // len(sc["kps"]))
    return np.tile(sc["kps"], rep)[:n], np.tile(sc["depth"], rep)[:n], np.tile(sc["xyz"], (rep, 1))[:n]


def test_map_dev_staging_buffer_grows_and_shrinks(sc):
    d_ent = torch.from_numpy(sc["entropy"]).cuda()
    for n in (1, 3000, 65, 3000, 0, 700):
        kps, depth, xyz = _tiled(sc, n) if n else (sc["kps"][:0], sc["depth"][:0], sc["xyz"][:0])
        got = selection.entropy_gate_map_dev(kps, depth, xyz, d_ent, sc["Sx"], *K, sc["ls2"], sc["th"])
        want = selection.entropy_gate(kps, depth, xyz, sc["entropy"], sc["Sx"], *K, sc["ls2"], sc["th"])
        assert len(got[0]) == n
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes(), n


def test_device_resident_keys_equal_the_host_form(sc):
    n = len(sc["kps"])
    d_k = torch.from_numpy(sc["kps"].view(np.uint8).copy()).cuda(); d_d = torch.from_numpy(sc["depth"]).cuda()
    d_x = torch.from_numpy(sc["xyz"]).cuda(); d_e = torch.from_numpy(sc["entropy"]).cuda()
    mi = torch.empty(n, dtype=torch.float64, device="cuda"); red = torch.empty_like(mi); acc = torch.empty(n, dtype=torch.uint8, device="cuda")
    selection.entropy_gate_dev(d_k, d_d, d_x, d_e, sc["Sx"], *K, sc["ls2"], sc["th"], mi, red, acc)
    torch.cuda.synchronize()
    want = _gate(sc, sc["th"])
    for g, w in zip((mi, red, acc), want):
        assert g.cpu().numpy().tobytes() == w.tobytes()


def test_full_size_map_with_one_thread_in_the_second_block():
    rng = np.random.default_rng(5)
    n, H, W = 65, 352, 1024
    kps = np.zeros(n, GR.KP_DTYPE)
    kps["x"] = rng.uniform(0, W, n); kps["y"] = rng.uniform(0, H, n); kps["octave"] = rng.integers(0, 8, n)
    kps["x"][64], kps["y"][64] = W - 0.5, H - 0.5                      # the lone thread reads the map's last entry
    sc = dict(kps=kps, depth=rng.uniform(0.5, 60, n).astype(np.float32), entropy=rng.uniform(0, 3.9, (H, W)), Sx=GR.covariance(rng),
              xyz=np.stack([rng.uniform(-20, 20, n), rng.uniform(-3, 3, n), rng.uniform(1, 60, n)], 1),
              ls2=(np.float32(1.2) ** (2 * np.arange(8))).astype(np.float32))
    sc["th"] = GR.pick_threshold(sc)
    g, r = _gate(sc, sc["th"]), _restated(sc, sc["th"])
    _compare(g, r, sc["th"], 0)
    assert g[1][64] == g[0][64] - sc["entropy"][H - 1, W - 1] and 5 < g[2].sum() < 60


# ---------------------------------------------------------------------------------------------------------------------
# octaves outside the table: [nlevels, 16) with nlevels = 8 (inside the kernel argument's 16 entries)
def _bad(sc, at, octave):
    k = sc["kps"].copy(); k["octave"][at] = octave
    return k


def test_host_forms_refuse_an_octave_outside_the_table(sc):
    """Scanned on the host before anything is staged or launched: invalid argument, the outputs as they were."""
    n = len(sc["kps"])
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    cov = (C.c_double * 36)(*sc["Sx"].ravel())
    ent, conf, cls = (np.ascontiguousarray(sc[k]) for k in ("entropy", "confidence", "classes"))
    d_ent = torch.from_numpy(ent).cuda()
    live = int(np.nonzero(_gate(sc, -1e9)[2])[0][5])
    for at, octave in ((0, 8), (live, 8), (live, 15), (n - 1, 11)):
        k = _bad(sc, at, octave)
        mi = np.full(n, 7.0); red = np.full(n, 7.0); acc = np.full(n, 7, np.uint8)
        L = lib()
        calls = (lambda: L.sivo_entropy_gate(n, p(k), p(sc["depth"]), p(sc["xyz"]), p(ent), 7, 13, cov, *K, p(sc["ls2"]), 8, sc["th"], p(mi), p(red), p(acc)),
                 lambda: L.sivo_entropy_gate_map_dev(n, p(k), p(sc["depth"]), p(sc["xyz"]), d_ent.data_ptr(), 7, 13, cov, *K, p(sc["ls2"]), 8, sc["th"],
                                                     p(mi), p(red), p(acc)),
                 lambda: L.sivo_check_semantics(n, p(k), p(sc["depth"]), p(sc["xyz"]), p(ent), p(conf), p(cls), 7, 13, cov, *K, p(sc["ls2"]), 8, sc["th"],
                                                sc["th_conf"], p(mi), p(red), p(acc)))
        for call in calls:
            with pytest.raises(SivoError):
                check(call())
            assert (mi == 7).all() and (red == 7).all() and (acc == 7).all()
    # the same keys with the octaves as they were go through
    assert np.array_equal(_gate(sc, sc["th"])[2], _restated(sc, sc["th"])[2])


def test_device_resident_forms_fail_a_key_with_an_octave_outside_the_table(sc):
    """The device-resident forms cannot look at the keys: the kernel fails such a key (MI 0, reduction 0, accept 0 / class 255)
    without indexing anything with its octave; the keys before and after it are as they were."""
    n = len(sc["kps"])
    good_gate, good_sem = _gate(sc, -1e9), _sem(sc, -1e9)
    live = np.nonzero((good_sem[2] != 255) & (good_gate[2] == 1))[0]
    bad_at = [int(live[0]), int(live[len(live) // 2]), int(live[-1])]
    k = sc["kps"].copy()
    k["octave"][bad_at] = [8, 12, 15]
    d_k = torch.from_numpy(k.view(np.uint8).copy()).cuda(); d_d = torch.from_numpy(sc["depth"]).cuda()
    d_x = torch.from_numpy(sc["xyz"]).cuda(); d_e = torch.from_numpy(sc["entropy"]).cuda()
    d_c = torch.from_numpy(sc["confidence"]).cuda(); d_l = torch.from_numpy(sc["classes"]).cuda()
    mi = torch.full((n,), 7.0, dtype=torch.float64, device="cuda"); red = torch.full_like(mi, 7.0)
    acc = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    selection.entropy_gate_dev(d_k, d_d, d_x, d_e, sc["Sx"], *K, sc["ls2"], -1e9, mi, red, acc)
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in (mi, red, acc)]
    others = np.ones(n, bool); others[bad_at] = False
    assert (got[0][bad_at] == 0).all() and (got[1][bad_at] == 0).all() and (got[2][bad_at] == 0).all()
    for g, w in zip(got, good_gate):
        assert g[others].tobytes() == w[others].tobytes()
    cov = (C.c_double * 36)(*sc["Sx"].ravel())
    ls2 = np.ascontiguousarray(sc["ls2"], np.float32)
    check(lib().sivo_check_semantics_dev(n, d_k.data_ptr(), d_d.data_ptr(), d_x.data_ptr(), d_e.data_ptr(), d_c.data_ptr(), d_l.data_ptr(), 7, 13, cov,
                                         *K, ls2.ctypes.data_as(C.c_void_p), 8, -1e9, sc["th_conf"], mi.data_ptr(), red.data_ptr(), acc.data_ptr(),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in (mi, red, acc)]
    assert (got[0][bad_at] == 0).all() and (got[1][bad_at] == 0).all() and (got[2][bad_at] == 255).all()
    for g, w in zip(got, good_sem):
        assert g[others].tobytes() == w[others].tobytes()
    assert np.array_equal(got[2], GR.gate(k, sc["depth"], sc["xyz"], sc["entropy"], sc["Sx"], *K, sc["ls2"], -1e9, sc["confidence"], sc["classes"], sc["th_conf"])[2])
