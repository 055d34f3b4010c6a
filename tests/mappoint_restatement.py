"""numpy restatement of sivo_amd/csrc/mappoint_math.hpp (MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth,
reference src/orbslam/MapPoint.cc:284-347, :368-411), a literal transcription of the reference's sort-and-index rule, and the generator
of the refresh tests.  No device, no library."""
import numpy as np

F, D = np.float32, np.float64
NO_OBSERVATION, NO_DESCRIPTOR = 1, 2
_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def hamming_matrix(desc):
    """(N, 32) uint8 -> (N, N) distances."""
    return _POP[desc[:, None, :] ^ desc[None, :, :]].sum(-1)


def row_medians(desc):
    """mp_row_median for every row: nine halvings of [0, 256], each a count over the row."""
    N = desc.shape[0]
    dist = hamming_matrix(desc)
    k = int(0.5 * (N - 1))
    lo, hi = np.zeros(N, np.int64), np.full(N, 256, np.int64)
    for _ in range(9):
        mid = (lo + hi) >> 1
        count = (dist <= mid[:, None]).sum(1)
        act = lo < hi
        up = count > k
        hi = np.where(act & up, mid, hi)
        lo = np.where(act & ~up, mid + 1, lo)
    return lo


def best_index(desc):
    """The first row with the strictly smallest median."""
    med = row_medians(desc)
    return int(np.argmin(med))          # (argmin returns the first minimum)


def best_index_literal(desc):
    """MapPoint.cc:315-341 line by line."""
    N = len(desc)
    Distances = [[0.0] * N for _ in range(N)]
    for i in range(N):
        Distances[i][i] = 0
        for j in range(i + 1, N):
            distij = int(np.unpackbits(np.bitwise_xor(desc[i], desc[j])).sum())
            Distances[i][j] = distij
            Distances[j][i] = distij
    BestMedian, BestIdx = 2 ** 31 - 1, 0
    for i in range(N):
        vDists = sorted(int(v) for v in Distances[i])
        median = vDists[int(0.5 * (N - 1))]
        if median < BestMedian:
            BestMedian, BestIdx = median, i
    return BestIdx


def refresh(desc_off, desc, obs_off, obs_ow, pos, ref_ow, level_scale, last_scale):
    """sivo_mappoint_refresh: best_idx, max_dist, min_dist, normal, flags; entries of a flagged point stay 0."""
    desc_off, obs_off = np.asarray(desc_off, np.int64), np.asarray(obs_off, np.int64)
    n = desc_off.shape[0] - 1
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    obs_ow = np.asarray(obs_ow, F).reshape(-1, 3)
    pos, ref_ow = np.asarray(pos, F).reshape(n, 3), np.asarray(ref_ow, F).reshape(n, 3)
    level_scale, last_scale = np.asarray(level_scale, F).reshape(n), np.asarray(last_scale, F).reshape(n)
    N, M = np.diff(desc_off), np.diff(obs_off)
    flags = np.where(M == 0, NO_OBSERVATION | NO_DESCRIPTOR, np.where(N == 0, NO_DESCRIPTOR, 0)).astype(np.uint8)
    best = np.zeros(n, np.int32)
    for p in np.flatnonzero(flags == 0):
        best[p] = best_index(desc[desc_off[p]:desc_off[p + 1]])
    with np.errstate(all="ignore"):
        normal = np.zeros((n, 3), F)
        for j in range(int(M.max()) if n else 0):
            act = np.flatnonzero(M > j)
            d = pos[act] - obs_ow[obs_off[act] + j]
            s = np.zeros(act.shape[0], D)
            for i in range(3):
                s = s + d[:, i].astype(D) * d[:, i].astype(D)
            f = (1.0 / np.sqrt(s)).astype(F)
            normal[act] = normal[act] + d * f[:, None]
        pc = pos - ref_ow
        s = np.zeros(n, D)
        for i in range(3):
            s = s + pc[:, i].astype(D) * pc[:, i].astype(D)
        dist = np.sqrt(s).astype(F)
        mx = dist * level_scale
        mn = mx / last_scale
        normal = normal * (1.0 / np.maximum(M, 1).astype(D)).astype(F)[:, None]
    live = M > 0

    def store(a):
        bits = np.where(live.reshape((-1,) + (1,) * (a.ndim - 1)), a, 0).astype(F).view(np.uint32).copy()
        bits[np.isnan(a) & live.reshape((-1,) + (1,) * (a.ndim - 1))] = 0x7FC00000
        return bits.view(F)
    return {"best_idx": best, "max_dist": store(mx), "min_dist": store(mn), "normal": store(normal), "flags": flags}


def make_points(seed, sizes, bad=0.0, ties=False, identical=False):
    """One map point per entry of `sizes` (its number of observations).  A share `bad` of the observations comes from bad keyframes:
    they have a camera centre and no descriptor.  ties: descriptors drawn from a handful of patterns, so that medians and distances
    repeat; identical: every descriptor of a point is the same."""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, np.int64)
    n = sizes.shape[0]
    obs_off = np.concatenate([[0], np.cumsum(sizes)])
    no = int(obs_off[-1])
    has_desc = rng.random(no) >= bad
    nd = np.zeros(n, np.int64)
    descs = []
    for p in range(n):
        k = int(has_desc[obs_off[p]:obs_off[p + 1]].sum())
        nd[p] = k
        if identical:
            d = np.repeat(rng.integers(0, 256, (1, 32), dtype=np.uint8), k, axis=0)
        elif ties:
            pool = rng.integers(0, 256, (3, 32), dtype=np.uint8)
            d = pool[rng.integers(0, 3, k)]
            flip = rng.random(k) < 0.3                       # a few one-bit neighbours of the patterns
            d = d.copy()
            d[flip, 0] ^= 1
        else:
            base = rng.integers(0, 256, (1, 32), dtype=np.uint8)
            d = base ^ (rng.random((k, 32, 8)) < 0.12).dot(1 << np.arange(8)).astype(np.uint8)
        descs.append(d.reshape(k, 32))
    pos = rng.normal(size=(n, 3)) * 10
    ow = np.repeat(pos, sizes, axis=0) + rng.normal(size=(no, 3)) * 8
    levels = rng.integers(0, 8, n)
    sf = F(1.2) ** np.arange(8, dtype=F)
    first = np.minimum(obs_off[:-1], max(no - 1, 0))
    return {"desc_off": np.concatenate([[0], np.cumsum(nd)]), "desc": np.concatenate(descs) if descs else np.zeros((0, 32), np.uint8),
            "obs_off": obs_off, "obs_ow": ow.astype(F), "pos": pos.astype(F),
            "ref_ow": (ow[first] if no else np.zeros((n, 3))).astype(F), "level_scale": sf[levels], "last_scale": np.full(n, sf[-1], F)}
