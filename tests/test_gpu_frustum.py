"""The frustum cull and the fused local-map search on the device (sivo_amd/csrc/frustum.hip, search.hip through sivo_amd/tracking.py)
against the host build of the same arithmetic (tests/frustum_prog.cpp), the reference's recorded Frame::isInFrustum
(tests/golden/frustum_reference.npz) and the sequential oracle of SearchByProjection.  Reads only tests/golden."""
import numpy as np
import pytest

import frustum_pin_cases as P
import host_prog
import search_local_cases as S

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return host_prog.build("frustum_prog", tmp_path_factory.mktemp("frustum_prog"))


def frustum_of(group, nlevels=P.NLEVELS):
    from sivo_amd import tracking as T
    return T.frustum(P.inputs(group)["Tcw"], *(getattr(P.FC, k) for k in ("FX", "FY", "CX", "CY", "BF")), P.BOUNDS, P.SCALE_FACTOR, nlevels, P.COS_LIMIT)


def sentinels(n):
    out = {k: np.full(n, P.SENTINEL, F32) for k in P.TRACK}
    out["level"] = np.full(n, P.LEVEL_SENTINEL, np.int32)
    return out


def device_cull(group, n=None):
    from sivo_amd import tracking as T
    g = P.inputs(group)
    n = len(g["pos"]) if n is None else n
    return T.frustum_cull(frustum_of(group), g["pos"][:n], g["normal"][:n], g["min_dist"][:n], g["max_dist"][:n], g["skip"][:n], out=sentinels(n))


def same_bytes(a, b, what):
    for k in ("status", "level") + P.TRACK:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k)
    assert int(a["n_in_view"]) == int(b["n_in_view"]), what


@pytest.mark.parametrize("group", P.GROUPS)
def test_cull_equals_the_host_build_and_the_reference(prog, tmp_path, group):
    """Bit for bit on the probes (600), the ulp sweep (1440) and the hand-made points: the status byte and every output against the host
    build, in view / the track fields / the level against the reference; the entries of a point out of view keep the sentinels."""
    got = device_cull(group)
    P.same_as_reference(group, got, P.recorded(group), "device")
    same_bytes(got, P.host_cull(prog, tmp_path, group), group)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_cull_of_partial_workgroups(prog, tmp_path, n):
    same_bytes(device_cull("probes", n), P.host_cull(prog, tmp_path, "probes", n=n), n)


def device_cull_dev(group, n, count, skip):
    """sivo_frustum_cull_dev on torch tensors, in the form of frustum_cull's result."""
    import torch
    from sivo_amd import tracking as T
    g = P.inputs(group)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.array(a[:n])).to(dev)
    out = {k: up(v) for k, v in sentinels(n).items()}
    status = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    n_in_view = torch.full((1,), -5, dtype=torch.int32, device=dev) if count else None
    T.frustum_cull_dev(frustum_of(group), up(g["pos"]), up(g["normal"]), up(g["min_dist"]), up(g["max_dist"]), up(g["skip"]) if skip else None,
                       status, out["proj_x"], out["proj_y"], out["proj_xr"], out["view_cos"], out["level"], n_in_view)
    torch.cuda.synchronize(dev)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["status"] = status.cpu().numpy()
    res["n_in_view"] = int(n_in_view.item()) if count else int((res["status"] == 0).sum())
    return res


@pytest.mark.parametrize("count", [False, True], ids=["no_count", "count"])
@pytest.mark.parametrize("group,n", [("probes", None), ("hand", None), ("probes", 0), ("probes", 1), ("probes", 63), ("probes", 65), ("probes", 257)])
def test_cull_on_device_arrays_equals_the_host_array_form(group, n, count):
    """sivo_frustum_cull_dev on torch tensors and torch's stream against sivo_frustum_cull, bit for bit: the probes, the hand-made points
    (with the caller's skip flags) and partial waves and workgroups, with the in-view counter (a ballot and one atomic per wave) and
    without it; the entries of a point out of view keep the sentinels in both."""
    n = len(P.inputs(group)["pos"]) if n is None else n
    want = device_cull(group, n)
    got = device_cull_dev(group, n, count, skip=True)
    same_bytes(got, want, (group, n, count))
    if count:
        assert got["n_in_view"] == int((want["status"] == 0).sum())


def test_cull_on_device_arrays_without_skip_flags():
    """d_skip NULL: nothing is skipped — the hand-made points the caller skips are visible ones."""
    n = len(P.inputs("hand")["pos"])
    got, want = device_cull_dev("hand", n, True, skip=False), device_cull("hand")
    skipped = P.inputs("hand")["skip"] != 0
    assert (got["status"][skipped] == 0).all() and np.array_equal(got["status"][~skipped], want["status"][~skipped])
    assert got["n_in_view"] == int((got["status"] == 0).sum()) == want["n_in_view"] + int(skipped.sum())
    for k in ("level",) + P.TRACK:
        assert got[k][~skipped].tobytes() == want[k][~skipped].tobytes(), k


def test_cull_with_fewer_levels_clamps_as_the_host_build(prog, tmp_path):
    from sivo_amd import tracking as T
    g = P.inputs("sweep")
    for nlevels in (1, 3):
        got = T.frustum_cull(frustum_of("sweep", nlevels), g["pos"], g["normal"], g["min_dist"], g["max_dist"], out=sentinels(len(g["pos"])))
        same_bytes(got, P.host_cull(prog, tmp_path, "sweep", nlevels=nlevels), nlevels)
        assert got["level"][got["status"] == 0].max() == nlevels - 1


# ---------------------------------------------------------------------------------------------------------------------
# the fused search
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    """The probes and 40 twins as the local map; a frame of 300 keys at the reference's projections of the points in view; a tenth of
    its slots occupied (some by a point without observations); a few points skipped by the caller."""
    from sivo_amd import matcher as M
    m = S.local_map(40, 3)
    fk = S.frame_keys(m, 300, 4)
    rng = np.random.default_rng(9)
    occ = np.full(300, -1, np.int32)
    taken = rng.choice(300, 30, replace=False)
    occ[taken] = rng.integers(0, 4, 30)
    skip = (rng.random(m["n"]) < 0.05).astype(np.uint8)
    F = M.MatchFrame(fk["keys"], fk["u_right"], fk["desc"], P.BOUNDS, fk["scale"], fk["sigma2"], fk["inv_sigma2"])
    return dict(m=m, fk=fk, occ=occ, skip=skip, F=F)


@pytest.mark.parametrize("th", [1.0, 3.0, 5.0])
def test_fused_search_equals_cull_then_search_and_the_oracle(scene, th):
    from sivo_amd import matcher as M, tracking as T
    m, F, occ, skip = scene["m"], scene["F"], scene["occ"], scene["skip"]
    fr = frustum_of("probes")
    args = (m["pos"], m["normal"], m["min_dist"], m["max_dist"], skip)
    fused = T.search_local_points(F, fr, *args, m["desc"], m["obs"], th, 0.8, occ, out=sentinels(m["n"]))
    # (a) the cull on its own, then the existing search on its results
    cull = T.frustum_cull(fr, *args, out=sentinels(m["n"]))
    nm_a, match_a, occ_a = M.search_by_projection_mappoints(F, cull["in_view"], cull["proj_x"], cull["proj_y"], cull["proj_xr"],
                                                            np.where(cull["in_view"], cull["level"], 0), cull["view_cos"], m["desc"], m["obs"], th, 0.8, occ)
    # (b) the sequential oracle fed with the reference's recorded track fields
    ref_in_view = (P.recorded("probes")["in_view"][m["src"]] != 0) & (skip == 0)
    nm_b, match_b, occ_b = S.oracle_search(scene["fk"], m, ref_in_view, th, 0.8, occ)
    for k in ("status", "level") + P.TRACK:
        assert fused[k].tobytes() == cull[k].tobytes(), k
    assert np.array_equal(fused["in_view"], ref_in_view) and fused["n_in_view"] == cull["n_in_view"] == int(ref_in_view.sum())
    for what, nm, match, occ_out in (("cull + search", nm_a, match_a, occ_a), ("oracle", nm_b, match_b, occ_b)):
        assert np.array_equal(fused["match"], match), (what, th)
        assert np.array_equal(fused["occ_obs"], occ_out), (what, th)
        assert fused["n_matches"] == nm, (what, th)
    assert fused["n_matches"] > 100 and (fused["match"][occ > 0] == -1).all()


def test_fused_search_that_outgrows_the_slab(scene):
    """A small frame and a local map so large that the fused call's scratch does not fit the frame's slab: the engine moves the frame to
    a bigger slab inside the call, after the caller prepared the query kernel's arguments, and the kernel must read the frame's scale
    table from the new slab.  The point count is chosen from the slab the frame actually got (at least 160 bytes of scratch per
    point: the query record, its descriptor, the engine's per-query arrays and the point's own 85), so the growth happens whatever
    slabs earlier frames left in the pool.  Equal to cull-then-search on a frame of its own, and to a second call on the grown frame."""
    from sivo_amd import matcher as M, tracking as T
    m0, fk, th = scene["m"], scene["fk"], 3.0
    nk = 48
    frame = lambda: M.MatchFrame(fk["keys"][:nk], fk["u_right"][:nk], fk["desc"][:nk], P.BOUNDS, fk["scale"], fk["sigma2"], fk["inv_sigma2"])
    F = frame()
    before = F.slab_bytes()
    tiles = before // (160 * m0["n"]) + 1
    n = tiles * m0["n"]
    assert n * 160 > before and n < 1 << 20
    rng = np.random.default_rng(21)
    m = {k: np.ascontiguousarray(np.tile(m0[k], (tiles,) + (1,) * (m0[k].ndim - 1))) for k in ("pos", "normal", "min_dist", "max_dist", "obs")}
    desc = np.tile(m0["desc"], (tiles, 1))
    desc[np.arange(n), rng.integers(0, 32, n)] ^= (1 << rng.integers(0, 8, n)).astype(np.uint8)     # every copy differs by one bit
    skip = np.tile(scene["skip"], tiles)
    occ = scene["occ"][:nk].copy()
    fr = frustum_of("probes")
    args = (m["pos"], m["normal"], m["min_dist"], m["max_dist"], skip)
    fused = T.search_local_points(F, fr, *args, desc, m["obs"], th, 0.8, occ, out=sentinels(n))
    assert F.slab_bytes() > before, "the call was meant to outgrow the frame's slab"
    grown = F.slab_bytes()
    again = T.search_local_points(F, fr, *args, desc, m["obs"], th, 0.8, occ, out=sentinels(n))
    assert F.slab_bytes() == grown
    cull = T.frustum_cull(fr, *args, out=sentinels(n))
    nm, match, occ_out = M.search_by_projection_mappoints(frame(), cull["in_view"], cull["proj_x"], cull["proj_y"], cull["proj_xr"],
                                                          np.where(cull["in_view"], cull["level"], 0), cull["view_cos"], desc, m["obs"], th, 0.8, occ)
    for what, res in (("first call", fused), ("second call", again)):
        for k in ("status", "level") + P.TRACK:
            assert res[k].tobytes() == cull[k].tobytes(), (what, k)
        assert res["n_in_view"] == cull["n_in_view"] and res["n_matches"] == nm, what
        assert np.array_equal(res["match"], match) and np.array_equal(res["occ_obs"], occ_out), what
    assert fused["n_matches"] > 0


def test_fused_search_ran_repair_rounds(scene):
    """The scene is one in which the engine's speculation collides: the generic engine on the queries the cull implies needs more than
    the two rounds of a collision-free call."""
    from sivo_amd import matcher as M, tracking as T
    m, F = scene["m"], scene["F"]
    cull = T.frustum_cull(frustum_of("probes"), m["pos"], m["normal"], m["min_dist"], m["max_dist"], scene["skip"])
    q = np.zeros(m["n"], M.QUERY_DTYPE)
    iv = cull["in_view"]
    r = np.where(cull["view_cos"] > 0.998, F32(2.5), F32(4.0)) * F32(3.0) * scene["fk"]["scale"][np.where(iv, cull["level"], 0)]
    q["u"], q["v"], q["ur"], q["radius"], q["gate"] = cull["proj_x"], cull["proj_y"], cull["proj_xr"], r, r
    q["lvl_lo"], q["lvl_hi"] = cull["level"] - 1, cull["level"]
    q["flags"] = np.where(iv, M.Q_VALID | np.where(m["obs"] > 0, M.Q_BLOCKS, 0), 0)
    res = M.search(F, q, m["desc"], dict(th_dist=M.TH_HIGH, gate_mode=1, ratio_mode=1, nn_ratio=0.8, dynamic=1), blocked=scene["occ"] > 0)
    assert res["rounds"] > 2


def test_nothing_in_view(scene):
    """Every point behind the camera: no match, occ_obs as it was, and the track outputs untouched."""
    from sivo_amd import tracking as T
    m, F, occ = scene["m"], scene["F"], scene["occ"]
    behind = m["pos"].copy()
    behind[:, 2] = -np.abs(behind[:, 2]) - 5
    res = T.search_local_points(F, frustum_of("probes"), behind, m["normal"], m["min_dist"], m["max_dist"], None, m["desc"], m["obs"], 3.0, 0.8, occ,
                                out=sentinels(m["n"]))
    assert res["n_in_view"] == 0 and res["n_matches"] == 0 and (res["match"] == -1).all() and np.array_equal(res["occ_obs"], occ)
    assert (res["status"] == 1).all() and (res["level"] == P.LEVEL_SENTINEL).all() and (res["proj_x"].view(np.uint32) == P.SENTINEL.view(np.uint32)).all()
    empty = T.search_local_points(F, frustum_of("probes"), np.zeros((0, 3), F32), np.zeros((0, 3), F32), [], [], None, np.zeros((0, 32), np.uint8), [], 1.0,
                                  0.8, occ)
    assert empty["n_in_view"] == 0 and empty["n_matches"] == 0 and (empty["match"] == -1).all()


def test_invalid_arguments_are_rejected():
    from sivo_amd import tracking as T
    g = P.inputs("hand")
    for nlevels in (0, 17):
        with pytest.raises(Exception, match="nlevels"):
            T.frustum_cull(frustum_of("hand", nlevels), g["pos"], g["normal"], g["min_dist"], g["max_dist"])
    fr = frustum_of("hand")
    fr.log_scale_factor = 0.0
    with pytest.raises(Exception, match="log_scale_factor"):
        T.frustum_cull(fr, g["pos"], g["normal"], g["min_dist"], g["max_dist"])
