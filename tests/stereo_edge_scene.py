"""A 96 x 192 stereo pair with hand-made keys and descriptors that takes every exit of ComputeStereoMatches on purpose
(tests/stereo_restatement.py names them).  Left is uint8 noise, right is left seen with a disparity of 4 px plus noise of one
grey level, and a few patches are painted by hand.  The extractors (nfeatures=200, scale_factor=1.2, nlevels=4) only supply
their pyramids: the C ABI matches any keys against the resident pyramids.

build() returns the images, the keys / descriptors of both sides, bf / b, and `plants`: name -> (left index, the set of
statuses the plant is made for, the right index best_right must name or None).  No device, no library."""
import numpy as np

import stereo_restatement as SR

KP_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("size", np.float32), ("angle", np.float32),
                     ("response", np.float32), ("octave", np.int32), ("class_id", np.int32)])
F = np.float32
ROWS, COLS, DISPARITY = 96, 192, 4
NLEVELS, SCALE_FACTOR, NFEATURES = 4, 1.2, 200
BF, B = 40.0, 2.0                  # maxD = bf / b = 20 px, exact in float32
MAX_D = F(BF) / F(B)
MATCHED = {SR.ACCEPTED, SR.CULLED}


def flip_bits(desc, k, rng):
    """A copy of the 32-byte descriptor with exactly k of its 256 bits flipped."""
    bits = np.unpackbits(desc)
    bits[rng.choice(256, k, replace=False)] ^= 1
    return np.packbits(bits)


def _quadratic(img, y0, xc, a=0.75):
    """Rows y0-5 .. y0+5, columns xc-20 .. xc+20: a * (x - xc)^2.  Two such patches whose centres are s columns apart have,
    centre-subtracted, windows that differ by 2 a dx (inc - s): the SAD is proportional to |inc - s|, monotone over -5 .. 5
    when |s| >= 6 — the best increment is at the end."""
    xs = np.arange(xc - 20, xc + 21)
    img[y0 - 5:y0 + 6, xs] = np.clip(np.rint(a * (xs - xc) ** 2), 0, 255).astype(np.uint8)[None, :]


class _Scene:
    def __init__(self, rng):
        self.rng = rng
        self.kl, self.dl, self.kr, self.dr = [], [], [], []
        self.plants = {}

    def right(self, x, y, octave, desc):
        self.kr.append((x, y, octave)); self.dr.append(desc)
        return len(self.kr) - 1

    def left(self, name, x, y, octave, desc, statuses, best=None):
        self.kl.append((x, y, octave)); self.dl.append(desc)
        self.plants[name] = (len(self.kl) - 1, set(statuses) if not isinstance(statuses, int) else {statuses}, best)
        return len(self.kl) - 1

    def desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def pair(self, name, xl, yl, ol, xr, yr, o_r, flips, statuses, names_best=True):
        """One left key and one right key whose descriptors differ in exactly `flips` bits."""
        d = self.desc()
        r = self.right(xr, yr, o_r, flip_bits(d, flips, self.rng))
        self.left(name, xl, yl, ol, d, statuses, r if names_best else -1)
        return r


def build(identical=False, seed=7, n_background=41):
    """identical: the right image IS the left image (every SAD minimum is 0, so is the median, and every match is culled)."""
    rng = np.random.default_rng(seed)
    left = rng.integers(0, 256, (ROWS, COLS), dtype=np.uint8)
    right = rng.integers(0, 256, (ROWS, COLS), dtype=np.uint8)
    right[:, :COLS - DISPARITY] = left[:, DISPARITY:]
    right = np.clip(right.astype(np.int32) + rng.integers(-1, 2, right.shape), 0, 255).astype(np.uint8)
    S = _Scene(rng)
    W, NB = SR.WEAK, SR.NO_BEST

    # ---- the row table: spans clamped at row 0 and at the last row, (int)y truncation, rows outside the table
    dA = S.desc(); A = S.right(50.0, 1.0, 0, dA)                               # rows floor(-1) -> 0 .. 3
    S.left("row0_clamped", 52.0, 0.2, 0, flip_bits(dA, 80, rng), W, A)
    S.left("row_trunc_neg", 53.0, -0.5, 0, flip_bits(dA, 80, rng), W, A)       # (int)-0.5 == 0
    S.left("row_minus1", 54.0, -1.0, 0, flip_bits(dA, 80, rng), SR.NO_ROW, -1)
    S.left("maxu_neg", -0.5, 1.0, 0, flip_bits(dA, 80, rng), SR.MAXU_NEG, -1)
    dB = S.desc(); Bk = S.right(50.0, 94.5, 0, dB)                             # rows 92 .. ceil(96.5) -> 95
    S.left("rowlast_clamped", 52.0, 95.9, 0, flip_bits(dB, 80, rng), W, Bk)
    S.left("row_96", 54.0, 96.0, 0, flip_bits(dB, 80, rng), SR.NO_ROW, -1)
    # first and last row of a span and one row beyond each end (rows 17 and 24 hold no right key at all)
    dC = S.desc(); Ck = S.right(50.0, 20.3, 0, dC)                             # rows floor(18.3) = 18 .. ceil(22.3) = 23
    S.left("span_first", 52.0, 18.0, 0, flip_bits(dC, 80, rng), W, Ck)
    S.left("span_last", 52.0, 23.9, 0, flip_bits(dC, 80, rng), W, Ck)
    S.left("span_before", 52.0, 17.9, 0, flip_bits(dC, 80, rng), SR.NO_ROW, -1)
    S.left("span_after", 52.0, 24.0, 0, flip_bits(dC, 80, rng), SR.NO_ROW, -1)

    # ---- the Hamming thresholds: 74 goes on to the SAD, 75 and 99 are weak, 100 is no match
    for i, (k, st) in enumerate(((74, MATCHED), (75, W), (99, W), (100, NB))):
        x = 40.0 + 30.0 * i
        S.pair(f"hamming_{k}", x, 32.0, 0, x - DISPARITY, 32.0, 0, k, st, names_best=k < 100)
    # the window test at the left end: x rounds below 0
    S.pair("window_lo", 10.0, 32.0, 0, -1.0, 32.0, 0, 20, SR.WINDOW_OUT)

    # ---- minU / maxU in float32, and one nextafter outside each
    for i, name in enumerate(("maxu_in", "maxu_out", "minu_in", "minu_out")):
        uL = F(40.3 + 40.0 * i)
        min_u, max_u = uL - MAX_D, uL - F(0)
        xr = {"maxu_in": max_u, "maxu_out": np.nextafter(max_u, F(np.inf)), "minu_in": min_u, "minu_out": np.nextafter(min_u, F(-np.inf))}[name]
        S.pair(name, uL, 40.0, 0, xr, 40.0, 0, 80, W if name.endswith("_in") else NB, names_best=name.endswith("_in"))

    # ---- the octave filter: l +- 1 is in, l +- 2 is out
    for i, (ol, o_r) in enumerate(((2, 0), (2, 1), (2, 3), (1, 3), (1, 0), (0, 1), (0, 2), (3, 1), (1, 2), (3, 2))):
        x = 14.0 + 18.0 * i
        ok = abs(ol - o_r) <= 1
        S.pair(f"octave_{ol}_{o_r}", x, 50.0, ol, x - DISPARITY, 50.0, o_r, 80, W if ok else NB, names_best=ok)

    # ---- a tie: two right keys with one descriptor in one candidate list, the lower index wins
    d = S.desc(); dr = flip_bits(d, 30, rng)
    T1 = S.right(54.0, 59.0, 0, dr); S.right(56.0, 59.0, 0, dr.copy())
    S.left("tie", 60.0, 59.0, 0, d, MATCHED, T1)
    # the window test at the right end: round(x * inv_scale) == cols - 11 is out, cols - 12 is in
    S.pair("window_hi", 185.0, 82.0, 0, 181.0, 82.0, 0, 20, SR.WINDOW_OUT)
    S.pair("window_hi_in", 184.0, 59.0, 0, 180.0, 59.0, 0, 20, MATCHED)

    # ---- painted patches (octave 0: level 0 is the image itself), rows 65 .. 75 and 77 .. 87
    # mirrored about column 30 in both images: d1 == d3, deltaR == 0, disparity exactly 0 -> the 0.01 clamp
    half = rng.integers(0, 256, (11, 17), dtype=np.uint8)
    patch = np.concatenate([half[:, :0:-1], half], axis=1)                      # 33 columns, patch[:, 16 - k] == patch[:, 16 + k]
    left[65:76, 14:47] = patch; right[65:76, 14:47] = patch
    S.pair("mirror", 30.0, 70.0, 0, 30.0, 70.0, 0, 20, SR.ACCEPTED_CLAMPED)
    # right content 2 px to the right of a right key at x == uL: a negative disparity
    right[65:76, 72:93] = left[65:76, 70:91]
    S.pair("disp_neg", 80.0, 70.0, 0, 80.0, 70.0, 0, 20, SR.DISP_OUT)
    # right content 7 px away from the right key, either way: the best increment is +5 / -5
    _quadratic(left, 70, 130); _quadratic(right, 70, 126 + 7)
    S.pair("inc_edge_plus", 130.0, 70.0, 0, 126.0, 70.0, 0, 20, SR.INC_EDGE)
    _quadratic(left, 82, 40); _quadratic(right, 82, 36 - 7)
    S.pair("inc_edge_minus", 40.0, 82.0, 0, 36.0, 82.0, 0, 20, SR.INC_EDGE)
    # a right window with heavy noise: the match is found and the median cull takes it
    reg = right[77:88, 86:107].astype(np.int32) + rng.integers(-30, 31, (11, 21))
    right[77:88, 86:107] = np.clip(reg, 0, 255).astype(np.uint8)
    S.pair("culled", 100.0, 82.0, 0, 96.0, 82.0, 0, 20, SR.CULLED)

    # ---- ordinary matches on all four octaves (rows 30 .. 58: clear of the patches and of the empty rows 17 and 24).  Most are on
    # octave 0, where the SAD of a true match is about 120 (one grey level of noise): the median stays there, and the resampled
    # levels, whose 4 / scale px shift is no whole pixel, give the large distances that the cull takes.
    for i in range(n_background):
        x, y = float(F(rng.uniform(45, 150))), float(F(rng.uniform(30, 58)))
        o = (0, 0, 0, 0, 0, 1, 2, 3)[i % 8]
        S.pair(f"background_{i}", x, y, o, x - DISPARITY, y, o, 20, {SR.ACCEPTED, SR.CULLED, SR.INC_EDGE, SR.DISP_OUT})

    if identical:
        right = left.copy()
    mk = lambda keys: np.array([(x, y, 31.0, 0.0, 50.0, o, -1) for x, y, o in keys], KP_DTYPE)
    return dict(left=left, right=right, kpL=mk(S.kl), descL=np.stack(S.dl), kpR=mk(S.kr), descR=np.stack(S.dr),
                bf=BF, b=B, plants=S.plants)
