"""The tracking thread's local map on a map that stays on the device: Tracking::UpdateLocalMap (reference src/orbslam/Tracking.cc:1087-1235)
— the vote, mvpLocalKeyFrames, mpReferenceKF and mvpLocalMapPoints — per frame, on tables uploaded once (sivo_amd/csrc/localmap.hip).
Host numpy arrays in and out.  Integer results: exact, in the reference's order.  The handle also keeps the map points' attributes
(set_points / get_points), so that search_local_points runs the update and Tracking::SearchLocalPoints (:1033-1085) in one call
(sivo_amd/csrc/localmap_track.hip)."""
import ctypes as C

import numpy as np

from ._lib import ERR_CAPACITY, SivoError, check, lib

LDS_KF = 8192                                                                              # SIVO_COVIS_LDS_KF
TABLE_FIELDS = ("obs_off", "obs_kf", "point_bad", "kf_bad", "slot_off", "slot_point", "covis_off", "covis_kf", "child_off", "child_kf",
                "parent", "kf_order")
_DTYPE = dict(obs_off=np.int64, obs_kf=np.int32, point_bad=np.uint8, kf_bad=np.uint8, slot_off=np.int64, slot_point=np.int32,
              covis_off=np.int64, covis_kf=np.int32, child_off=np.int64, child_kf=np.int32, parent=np.int32, kf_order=np.int32)


class _Tables(C.Structure):  # == SivoLocalMapTables
    _fields_ = [("n_kf", C.c_int32), ("n_points", C.c_int32)] + [(f, C.c_void_p) for f in TABLE_FIELDS]


POINT_ROW_FIELDS = ("idx", "obs_off", "obs_kf", "bad")
KF_ROW_FIELDS = ("idx", "bad", "parent", "slot_off", "slot_point", "covis_off", "covis_kf", "child_off", "child_kf")
_ROW_DTYPE = dict(_DTYPE, idx=np.int32, bad=np.uint8)


class _Delta(C.Structure):  # == SivoLocalMapDelta
    _fields_ = ([("size", C.c_uint32), ("n_kf", C.c_int32), ("n_points", C.c_int32), ("n_point_rows", C.c_int32)]
                + [(f, C.c_void_p) for f in ("point_idx", "point_obs_off", "point_obs_kf", "point_bad")] + [("n_kf_rows", C.c_int32)]
                + [(f, C.c_void_p) for f in ("kf_idx", "kf_bad", "kf_parent", "kf_slot_off", "kf_slot_point", "kf_covis_off", "kf_covis_kf",
                                             "kf_child_off", "kf_child_kf", "kf_order")])


def _a(x, dt):
    return np.ascontiguousarray(x, dt).ravel()


def _p(x):
    return x.ctypes.data if x is not None and x.size else None


class Result:
    """What one update leaves: voted (False: keyframeCounter was empty, local_kf is None and the points are those of prev_local_kf),
    slot_cleared (one byte per frame slot), local_kf, ref_kf (-1: mpReferenceKF stays), local_points, counts (the vote, per keyframe)."""

    def __init__(self, voted, slot_cleared, local_kf, ref_kf, local_points, counts):
        self.voted, self.slot_cleared, self.local_kf, self.ref_kf = voted, slot_cleared, local_kf, ref_kf
        self.local_points, self.counts = local_points, counts


class TrackResult(Result):
    """What search_local_points leaves: the update's Result, and per local point status (SIVO_FRUSTUM_*), in_view, proj_x, proj_y,
    proj_xr, view_cos, level (the last five written for the points in view only), per keypoint match (the position in local_points of
    the matched point, or -1), and n_to_match, n_matches."""

    def __init__(self, update, **search):
        super().__init__(update.voted, update.slot_cleared, update.local_kf, update.ref_kf, update.local_points, update.counts)
        self.__dict__.update(search)


class WindowCapacity(SivoError):
    """SIVO_ERR_CAPACITY of ba_window under explicit capacities; counts = (n_local_kf, n_local_points, n_fixed_kf, n_edges), what a
    second call needs."""

    def __init__(self, msg, counts):
        super().__init__(ERR_CAPACITY, msg)
        self.counts = counts


class LocalMap:
    """The map as arrays over dense keyframe and point indices (SivoLocalMapTables of include/sivo_hip.h): obs_off / obs_kf (CSR point ->
    observing keyframes), point_bad, kf_bad, slot_off / slot_point (CSR keyframe -> GetMapPointMatches(), -1 for null), covis_off /
    covis_kf (mvpOrderedConnectedKeyFrames), child_off / child_kf (mspChildren in the set's order), parent (-1: none) and kf_order (the
    keyframes in pointer order; None: 0, 1, 2 ...).  The arrays are uploaded here and stay on the device until replace() or close();
    apply() changes and appends rows on the device, sizes() and export() read the handle back."""

    def __init__(self, n_kf, **tables):
        self._h = C.c_void_p()
        st = self._struct(n_kf, tables)
        check(lib().sivo_localmap_create(C.byref(st), C.byref(self._h)))

    def _struct(self, n_kf, tables):
        unknown = set(tables) - set(TABLE_FIELDS)
        if unknown:
            raise TypeError("unknown table " + ", ".join(sorted(unknown)))
        t = {f: None if tables.get(f) is None else _a(tables[f], _DTYPE[f]) for f in TABLE_FIELDS}
        n_points = 0 if t["point_bad"] is None else len(t["point_bad"])
        self._keep = t                                                 # alive over the call
        self.n_kf, self.n_points = int(n_kf), n_points
        off = t["slot_off"]
        self._slot_off = np.zeros(self.n_kf + 1, np.int64) if off is None or len(off) != self.n_kf + 1 else off.copy()
        return _Tables(self.n_kf, n_points, *[_p(t[f]) for f in TABLE_FIELDS])

    def replace(self, n_kf, **tables):
        """A new set of tables into the same handle."""
        st = self._struct(n_kf, tables)
        check(lib().sivo_localmap_replace(self._h, C.byref(st)))

    def apply(self, n_kf, n_points, point_rows=None, kf_rows=None, kf_order=None):
        """The rows that changed since the tables were sent, applied on the device (SivoLocalMapDelta).  n_kf, n_points: the map's sizes
        after the call.  point_rows: dict(idx, obs_off, obs_kf, bad) — the points whose observation list or flag is replaced, appended
        points included; kf_rows: dict(idx, bad, parent, slot_off, slot_point, covis_off, covis_kf, child_off, child_kf) — all rows of
        every listed keyframe, appended keyframes included.  idx is strictly increasing and lists every new index.  kf_order: the new
        order, or None for the handle's with the appended keyframes behind it.  A missing array is passed as NULL."""
        pr, kr = dict(point_rows or {}), dict(kf_rows or {})
        unknown = (set(pr) - set(POINT_ROW_FIELDS)) | (set(kr) - set(KF_ROW_FIELDS))
        if unknown:
            raise TypeError("unknown row array " + ", ".join(sorted(unknown)))
        pr = {f: None if pr.get(f) is None else _a(pr[f], _ROW_DTYPE[f]) for f in POINT_ROW_FIELDS}
        kr = {f: None if kr.get(f) is None else _a(kr[f], _ROW_DTYPE[f]) for f in KF_ROW_FIELDS}
        order = None if kf_order is None else _a(kf_order, np.int32)
        if order is not None and len(order) != int(n_kf):
            raise ValueError("kf_order must hold n_kf entries")
        n_pr = 0 if pr["idx"] is None else len(pr["idx"])
        n_kr = 0 if kr["idx"] is None else len(kr["idx"])
        for rows, n, fields in ((pr, n_pr, ("bad",)), (kr, n_kr, ("bad", "parent"))):
            for f in fields + tuple(k for k in rows if k.endswith("_off")):
                if rows[f] is not None and len(rows[f]) != n + f.endswith("_off"):
                    raise ValueError("%s must hold one entry per row%s" % (f, " and one more" if f.endswith("_off") else ""))
        for rows in (pr, kr):
            for f in rows:
                inner = f[:-4] + ("_point" if f == "slot_off" else "_kf")
                if f.endswith("_off") and rows[f] is not None and len(rows[f]) and rows[inner] is not None and len(rows[inner]) < int(rows[f][-1]):
                    raise ValueError("%s is shorter than %s says" % (inner, f))
        st = _Delta(C.sizeof(_Delta), int(n_kf), int(n_points), n_pr, _p(pr["idx"]), _p(pr["obs_off"]), _p(pr["obs_kf"]), _p(pr["bad"]), n_kr,
                    _p(kr["idx"]), _p(kr["bad"]), _p(kr["parent"]), _p(kr["slot_off"]), _p(kr["slot_point"]), _p(kr["covis_off"]),
                    _p(kr["covis_kf"]), _p(kr["child_off"]), _p(kr["child_kf"]), _p(order))
        check(lib().sivo_localmap_apply(self._h, C.byref(st)))
        length = np.zeros(int(n_kf), np.int64)
        length[:self.n_kf] = np.diff(self._slot_off)
        if n_kr:
            length[kr["idx"]] = np.diff(kr["slot_off"])
        self._slot_off = np.concatenate([np.zeros(1, np.int64), np.cumsum(length)])
        self.n_kf, self.n_points = int(n_kf), int(n_points)

    def sizes(self):
        """(n_kf, n_points, and the entries of obs_kf, slot_point, covis_kf, child_kf) of the handle."""
        out = np.zeros(6, np.int64)
        check(lib().sivo_localmap_sizes(self._h, out.ctypes.data))
        return tuple(int(v) for v in out)

    def export(self):
        """The handle's tables as a dict of arrays (n_kf and the twelve of TABLE_FIELDS): what create() would have to be given to make
        this handle.  kf_order is the identity where the creator passed None."""
        K, P, n_obs, n_slot, n_covis, n_child = self.sizes()
        n = dict(obs_off=P + 1, obs_kf=n_obs, point_bad=P, kf_bad=K, slot_off=K + 1, slot_point=n_slot, covis_off=K + 1, covis_kf=n_covis,
                 child_off=K + 1, child_kf=n_child, parent=K, kf_order=K)
        t = {f: np.zeros(n[f], _DTYPE[f]) for f in TABLE_FIELDS}
        st = _Tables(K, P, *[t[f].ctypes.data for f in TABLE_FIELDS])
        check(lib().sivo_localmap_export(self._h, C.byref(st)))
        return dict(t, n_kf=K)

    def set_bad(self, points=(), point_values=(), kfs=(), kf_values=()):
        """isBad() of the listed points / keyframes becomes the listed value."""
        pi, pv, ki, kv = _a(points, np.int32), _a(point_values, np.uint8), _a(kfs, np.int32), _a(kf_values, np.uint8)
        if len(pi) != len(pv) or len(ki) != len(kv):
            raise ValueError("one value per index")
        check(lib().sivo_localmap_set_bad(self._h, len(pi), _p(pi), _p(pv), len(ki), _p(ki), _p(kv)))

    def update(self, frame_point, kf_premarked=None, point_premarked=None, prev_local_kf=(), *, kf_capacity=None, point_capacity=None, out=None):
        """One frame.  frame_point: mCurrentFrame.mvpMapPoints as point indices, -1 for null; kf_premarked / point_premarked: the indices
        whose mnTrackReferenceForFrame already equals the frame's id; prev_local_kf: the local keyframes the caller holds.  The capacities
        default to what no result can exceed.  `out` (slot_cleared, local_kf, local_point, counts: arrays of the capacities' sizes) lets
        a caller see which entries the call wrote."""
        fp, kp, pp, prev, kcap, pcap, cleared, local_kf, local_point, counts = self._update_args(
            frame_point, kf_premarked, point_premarked, prev_local_kf, kf_capacity, point_capacity, out)
        voted, n_kf, ref, n_pts = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
        check(lib().sivo_localmap_update(self._h, len(fp), _p(fp), len(kp), _p(kp), len(pp), _p(pp), len(prev), _p(prev), C.byref(voted),
                                         _p(cleared), kcap, _p(local_kf), C.byref(n_kf), C.byref(ref), pcap, _p(local_point), C.byref(n_pts),
                                         _p(counts)))
        return Result(bool(voted.value), cleared, local_kf[:n_kf.value] if voted.value else None, int(ref.value), local_point[:n_pts.value], counts)

    def _update_args(self, frame_point, kf_premarked, point_premarked, prev_local_kf, kf_capacity, point_capacity, out):
        fp = _a(frame_point, np.int32)
        kp = _a(() if kf_premarked is None else kf_premarked, np.int32)
        pp = _a(() if point_premarked is None else point_premarked, np.int32)
        prev = _a(prev_local_kf, np.int32)
        in_range = prev[(prev >= 0) & (prev < self.n_kf)]              # (the library reports the others)
        g_max = max(int(self._slot_off[-1]), int((self._slot_off[in_range + 1] - self._slot_off[in_range]).sum()))
        kcap = self.n_kf if kf_capacity is None else int(kf_capacity)
        pcap = min(self.n_points, g_max) if point_capacity is None else int(point_capacity)
        out = out or {}
        cleared = out.get("slot_cleared", np.zeros(len(fp), np.uint8))
        local_kf = out.get("local_kf", np.zeros(max(kcap, 0), np.int32))
        local_point = out.get("local_point", np.zeros(max(pcap, 0), np.int32))
        counts = out.get("counts", np.zeros(self.n_kf, np.int32))
        for name, arr, n, dt in (("slot_cleared", cleared, len(fp), np.uint8), ("local_kf", local_kf, kcap, np.int32),
                                 ("local_point", local_point, pcap, np.int32), ("counts", counts, self.n_kf, np.int32)):
            if arr.dtype != dt or arr.ndim != 1 or len(arr) < n or not arr.flags.c_contiguous:
                raise ValueError("out[%r] must be a contiguous %s array of at least %d entries" % (name, np.dtype(dt).name, n))
        return fp, kp, pp, prev, kcap, pcap, cleared, local_kf, local_point, counts

    @staticmethod
    def _rows(idx, pos, normal, min_dist, max_dist, desc, n_obs):
        idx = _a(idx, np.int32); n = len(idx)
        rows = (_a(pos, np.float32), _a(normal, np.float32), _a(min_dist, np.float32), _a(max_dist, np.float32), _a(desc, np.uint8),
                _a(n_obs, np.int32))
        for x, per in zip(rows, (3, 3, 1, 1, 32, 1)):
            if len(x) != per * n:
                raise ValueError("the attribute arrays must hold one row per index")
        return (idx,) + rows

    def set_points(self, idx, pos, normal, min_dist, max_dist, desc, n_obs):
        """The attributes of the listed points (idx strictly increasing): pos = mWorldPos and normal = mNormalVector (n, 3) float32,
        min_dist / max_dist = mfMinDistance / mfMaxDistance raw, desc = GetDescriptor() (n, 32) uint8, n_obs = Observations().  One
        upload and a scatter on the device; the rows stay over apply(), and replace() unsets them all."""
        idx, pos, normal, lo, hi, desc, n_obs = self._rows(idx, pos, normal, min_dist, max_dist, desc, n_obs)
        check(lib().sivo_localmap_set_points(self._h, len(idx), _p(idx), _p(pos), _p(normal), _p(lo), _p(hi), _p(desc), _p(n_obs)))

    def get_points(self, idx):
        """The stored rows of the listed points (idx strictly increasing): a dict of pos, normal, min_dist, max_dist, desc, n_obs and
        is_set; a row nobody set reads as zeros."""
        idx = _a(idx, np.int32); n = len(idx)
        r = dict(pos=np.zeros((n, 3), np.float32), normal=np.zeros((n, 3), np.float32), min_dist=np.zeros(n, np.float32),
                 max_dist=np.zeros(n, np.float32), desc=np.zeros((n, 32), np.uint8), n_obs=np.zeros(n, np.int32), is_set=np.zeros(n, np.uint8))
        check(lib().sivo_localmap_get_points(self._h, n, _p(idx), *[r[k].ctypes.data for k in
                                                                     ("pos", "normal", "min_dist", "max_dist", "desc", "n_obs", "is_set")]))
        r["is_set"] = r["is_set"].astype(bool)
        return r

    def search_local_points(self, frame, frustum, frame_point, kf_premarked=None, point_premarked=None, prev_local_kf=(), seen_point=(),
                            th=1.0, nn_ratio=0.8, *, kf_capacity=None, point_capacity=None, out=None):
        """update() and Tracking::SearchLocalPoints in one call (sivo_localmap_search_local_points).  frame: a matcher.MatchFrame with as
        many keys as frame_point has slots; frustum: tracking.frustum(...); seen_point: the points whose mnLastFrameSeen already equals
        the frame's id and that the frame does not hold.  Every point of the handle must have its attributes (set_points).  `out` may
        also hold status, proj_x, proj_y, proj_xr, view_cos, level (of the point capacity's size) and match: contiguous arrays of
        the documented types are written in place.  Returns a TrackResult."""
        fp, kp, pp, prev, kcap, pcap, cleared, local_kf, local_point, counts = self._update_args(
            frame_point, kf_premarked, point_premarked, prev_local_kf, kf_capacity, point_capacity, out)
        seen = _a(seen_point, np.int32)
        out = out or {}
        n = max(pcap, 0)
        per_point = {k: (np.zeros(n, dt) if k not in out else np.ascontiguousarray(out[k], dt))
                     for k, dt in (("status", np.uint8), ("proj_x", np.float32), ("proj_y", np.float32), ("proj_xr", np.float32),
                                   ("view_cos", np.float32), ("level", np.int32))}
        match = np.zeros(len(fp), np.int32) if "match" not in out else np.ascontiguousarray(out["match"], np.int32)
        if any(len(v) < n for v in per_point.values()) or len(match) < len(fp):
            raise ValueError("a search output is shorter than its capacity")
        voted, n_kf, ref, n_pts, nt, nm = (C.c_int32(-1) for _ in range(6))
        check(lib().sivo_localmap_search_local_points(
            self._h, frame._h, C.byref(frustum), len(fp), _p(fp), len(kp), _p(kp), len(pp), _p(pp), len(prev), _p(prev), len(seen), _p(seen),
            th, nn_ratio, C.byref(voted), _p(cleared), kcap, _p(local_kf), C.byref(n_kf), C.byref(ref), pcap, _p(local_point), C.byref(n_pts),
            _p(counts), *[_p(per_point[k]) for k in ("status", "proj_x", "proj_y", "proj_xr", "view_cos", "level")], _p(match),
            C.byref(nt), C.byref(nm)))
        upd = Result(bool(voted.value), cleared, local_kf[:n_kf.value] if voted.value else None, int(ref.value), local_point[:n_pts.value], counts)
        k = n_pts.value
        search = {name: v[:k] for name, v in per_point.items()}
        return TrackResult(upd, in_view=per_point["status"][:k] == 0, match=match, n_to_match=nt.value, n_matches=nm.value, full=per_point,
                           **search)

    def ba_window(self, cand_kf, kf_local_premarked=None, kf_fixed_premarked=None, point_premarked=None, *, kf_capacity=None,
                  point_capacity=None, edge_capacity=None):
        """The window of Optimizer::LocalBundleAdjustment (Optimizer.cc:496-559, :651-670).  cand_kf: pKF, then its covisibles in their
        order; the premarked lists: the keyframes whose mnBALocalForKF / mnBAFixedForKF and the points whose mnBALocalForKF already equal
        pKF's id.  Returns local_kf, fixed_kf, local_points, edge_off, edge_pose, edge_slot (sivo_localmap_ba_window of
        include/sivo_hip.h).  The capacities default to what no result can exceed; a result beyond a given one raises WindowCapacity."""
        ck = _a(cand_kf, np.int32)
        kl, kx, pp = (_a(() if x is None else x, np.int32) for x in (kf_local_premarked, kf_fixed_premarked, point_premarked))
        K, P, n_obs, n_slot = self.sizes()[:4]
        kcap = K if kf_capacity is None else int(kf_capacity)
        pcap = min(P, n_slot) if point_capacity is None else int(point_capacity)
        ecap = n_obs if edge_capacity is None else int(edge_capacity)
        local_kf, fixed_kf = np.zeros(max(kcap, 0), np.int32), np.zeros(max(kcap, 0), np.int32)
        local_point, edge_off = np.zeros(max(pcap, 0), np.int32), np.zeros(max(pcap, 0) + 1, np.int64)
        edge_pose, edge_slot = np.zeros(max(ecap, 0), np.int32), np.zeros(max(ecap, 0), np.int32)
        counts = np.zeros(4, np.int64)
        rc = lib().sivo_localmap_ba_window(self._h, len(ck), _p(ck), len(kl), _p(kl), len(kx), _p(kx), len(pp), _p(pp), kcap, _p(local_kf),
                                           _p(fixed_kf), pcap, _p(local_point), edge_off.ctypes.data, ecap, _p(edge_pose), _p(edge_slot),
                                           counts.ctypes.data)
        if rc == ERR_CAPACITY:
            raise WindowCapacity(lib().sivo_last_error().decode(errors="replace"), tuple(int(v) for v in counts))
        check(rc)
        nl, npt, nf, ne = (int(v) for v in counts)
        return local_kf[:nl], fixed_kf[:nf], local_point[:npt], edge_off[:npt + 1], edge_pose[:ne], edge_slot[:ne]

    def close(self):
        if self._h:
            check(lib().sivo_localmap_destroy(self._h))
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
