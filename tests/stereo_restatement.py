"""Plain Python / numpy restatement of sivo_stereo_match_begin + sivo_stereo_match_cull (sivo_amd/csrc/orb.hip; Frame::ComputeStereoMatches,
reference src/orbslam/Frame.cc:444-629) that also says WHY every left key ended where it did.  Every `float` of the C++ is an np.float32 here
and the operations come in the C++'s order; no device, no library.

Status codes, one per left key, naming the step that ended it:
  NO_ROW            (int)y outside the row table, or no right key spans that row
  MAXU_NEG          maxU = uL - minD < 0
  NO_BEST           no candidate, or the best Hamming distance >= TH_HIGH (100)
  WEAK              (TH_HIGH + TH_LOW) / 2 = 75 <= best < 100: best_right is set and nothing else
  WINDOW_OUT        iniu < 0 or endu >= cols of the level: the 11 windows would leave the right level image
  INC_EDGE          the best of the 11 SAD increments is -5 or +5
  DISP_OUT          the disparity is not in [minD, maxD) (negative, too large, or NaN)
  ACCEPTED          a match; survives the median cull
  ACCEPTED_CLAMPED  a match whose disparity was <= 0 and became 0.01 (uR = uL - 0.01, depth = bf / 0.01); survives the cull
  CULLED            a match (clamped or not) whose SAD distance is >= 1.5 * 1.4 * median

The `deltaR < -1 || deltaR > 1` test of Frame.cc:596 has no code here because it cannot fail: the best increment is interior, so
d2 is the FIRST minimum of the eleven distances, hence d1 > d2 and d3 >= d2.  With a = d1 - d2 > 0 and c = d3 - d2 >= 0,
deltaR = (a - c) / (2 (a + c)) and |a - c| <= a + c, so |deltaR| <= 1/2.  (The distances are integers below 2^24: d1 - d3 and
d1 + d3 - 2 d2 are exact in float32, the quotient is rounded once and 1/2 is representable.)

Precondition of the inputs (asserted by stereo_match): the 11 x 11 window of a left key that reaches the SAD stage, and the windows
of its best right key over the increments -5 .. 5, lie inside the level image — round(xR * inv_scale) is never in [0, 10).  The
reference would throw there and the CPU oracle reads the level without its border, so such inputs are outside the contract."""
import math

import numpy as np

F = np.float32
(NO_ROW, MAXU_NEG, NO_BEST, WEAK, WINDOW_OUT, INC_EDGE, DISP_OUT, ACCEPTED, ACCEPTED_CLAMPED, CULLED) = range(10)
STATUS_NAMES = ["NO_ROW", "MAXU_NEG", "NO_BEST", "WEAK", "WINDOW_OUT", "INC_EDGE", "DISP_OUT", "ACCEPTED", "ACCEPTED_CLAMPED", "CULLED"]
TH_HIGH, TH_LOW = 100, 50
INT32_MAX = 2 ** 31 - 1


def roundf(v):
    """std::round on a float: halves away from zero (np.round goes to even)."""
    v = float(v)
    return F(math.copysign(math.floor(abs(v) + 0.5), v))


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def sad11(imL, imR, cy, cxl, cxr0):
    """The 11 distances of stereo_sad_kernel: L1 between the centre-subtracted 11 x 11 windows, right window at cxr0 + inc."""
    wl = imL[cy - 5:cy + 6, cxl - 5:cxl + 6].astype(np.int64) - int(imL[cy, cxl])
    out = []
    for inc in range(-5, 6):
        c = cxr0 + inc
        wr = imR[cy - 5:cy + 6, c - 5:c + 6].astype(np.int64) - int(imR[cy, c])
        out.append(int(np.abs(wl - wr).sum()))
    return out


def cull(sad, u_right, depth, keep=None):
    """sivo_stereo_match_cull on copies: returns (u_right, depth, culled mask).  Keys with keep[i] == 0 get -1 and take no part;
    the median is the element n / 2 of the sorted (sad, index) pairs with sad >= 0 and u_right >= 0; thDist = 1.5f * 1.4f * median
    in float32 (the product of the two constants first); from the top, every distance that is not < thDist goes."""
    sad = np.asarray(sad, np.int32)
    u_right = np.array(u_right, F); depth = np.array(depth, F)
    culled = np.zeros(len(sad), bool)
    pairs = []
    for i in range(len(sad)):
        if keep is not None and not keep[i]:
            u_right[i] = F(-1); depth[i] = F(-1)
            continue
        if sad[i] >= 0 and u_right[i] >= 0:
            pairs.append((int(sad[i]), i))
    if pairs:
        pairs.sort()
        median = F(pairs[len(pairs) // 2][0])
        th_dist = (F(1.5) * F(1.4)) * median
        for d, i in reversed(pairs):
            if F(d) < th_dist:
                break
            u_right[i] = F(-1); depth[i] = F(-1); culled[i] = True
    return u_right, depth, culled


def stereo_match_begin(kpL, descL, kpR, descR, scale, inv_scale, pyrL, pyrR, bf, b):
    """sivo_stereo_match_begin.  kp*: records with x, y (float32) and octave; pyr*: the level images without border.
    Returns u_right, depth (float32), best_right, sad (int32), status — ACCEPTED / ACCEPTED_CLAMPED before any cull."""
    nL, nR = len(kpL), len(kpR)
    scale = np.asarray(scale, F); inv_scale = np.asarray(inv_scale, F)
    bf, b = F(bf), F(b)
    u_right = np.full(nL, -1, F); depth = np.full(nL, -1, F)
    best_right = np.full(nL, -1, np.int32); sad = np.full(nL, -1, np.int32)
    status = np.full(nL, NO_ROW, np.int32)
    if nL == 0:
        return u_right, depth, best_right, sad, status
    n_rows = pyrL[0].shape[0]
    th_orb = (TH_HIGH + TH_LOW) // 2
    # row table (:454-477), rows clamped to the table
    rows = [[] for _ in range(n_rows)]
    for iR in range(nR):
        r = F(2.0) * scale[kpR["octave"][iR]]
        y = F(kpR["y"][iR])
        maxr = min(int(math.ceil(float(y + r))), n_rows - 1)
        minr = max(int(math.floor(float(y - r))), 0)
        for yi in range(minr, maxr + 1):
            rows[yi].append(iR)
    min_z, min_d = b, F(0)
    max_d = bf / min_z
    with np.errstate(all="ignore"):
        for iL in range(nL):
            lvl = int(kpL["octave"][iL])
            uL, vL = F(kpL["x"][iL]), F(kpL["y"][iL])
            row = int(vL)                                           # (int)kp.y: truncation towards zero
            if row < 0 or row >= n_rows or not rows[row]:
                status[iL] = NO_ROW
                continue
            min_u, max_u = uL - max_d, uL - min_d
            if max_u < 0:
                status[iL] = MAXU_NEG
                continue
            best, bi = TH_HIGH, -1
            for iR in rows[row]:
                oR = int(kpR["octave"][iR])
                if oR < lvl - 1 or oR > lvl + 1:
                    continue
                xR = F(kpR["x"][iR])
                if xR >= min_u and xR <= max_u:
                    d = hamming(descL[iL], descR[iR])
                    if d < best:
                        best, bi = d, iR
            if best >= TH_HIGH:
                status[iL] = NO_BEST
                continue
            best_right[iL] = bi
            if best >= th_orb:
                status[iL] = WEAK
                continue
            sf = inv_scale[lvl]
            suL, svL, suR0 = roundf(uL * sf), roundf(vL * sf), roundf(F(kpR["x"][bi]) * sf)
            iniu = suR0 + F(5) - F(5)
            endu = suR0 + F(5) + F(5) + F(1)
            cols = pyrR[lvl].shape[1]
            if iniu < 0 or endu >= F(cols):
                status[iL] = WINDOW_OUT
                continue
            cy, cxl, cxr0 = int(svL), int(suL), int(suR0)
            lr, lc = pyrL[lvl].shape
            assert 5 <= cy < lr - 5 and 5 <= cxl < lc - 5 and cxr0 >= 10, f"left key {iL}: a SAD window leaves level {lvl} (outside the contract)"
            dists = sad11(pyrL[lvl], pyrR[lvl], cy, cxl, cxr0)
            best_dist, best_inc = INT32_MAX, 0
            vD = []
            for inc in range(-5, 6):
                dist = F(dists[inc + 5])
                if dist < F(best_dist):
                    best_dist, best_inc = int(dist), inc
                vD.append(dist)
            if best_inc == -5 or best_inc == 5:
                status[iL] = INC_EDGE
                continue
            d1, d2, d3 = vD[5 + best_inc - 1], vD[5 + best_inc], vD[5 + best_inc + 1]
            delta_r = (d1 - d3) / (F(2.0) * (d1 + d3 - F(2.0) * d2))
            best_ur = scale[lvl] * (F(cxr0) + F(best_inc) + delta_r)
            disparity = uL - best_ur
            if disparity >= min_d and disparity < max_d:
                status[iL] = ACCEPTED
                if disparity <= 0:
                    disparity = F(0.01)
                    best_ur = F(np.float64(uL) - 0.01)
                    status[iL] = ACCEPTED_CLAMPED
                depth[iL] = bf / disparity
                u_right[iL] = best_ur
                sad[iL] = best_dist
            else:
                status[iL] = DISP_OUT
    return u_right, depth, best_right, sad, status


def stereo_match(kpL, descL, kpR, descR, scale, inv_scale, pyrL, pyrR, bf, b, keep=None):
    """sivo_stereo_match (begin, then the cull over every key or over `keep`).  Returns u_right, depth, best_right, sad, status."""
    u_right, depth, best_right, sad, status = stereo_match_begin(kpL, descL, kpR, descR, scale, inv_scale, pyrL, pyrR, bf, b)
    u_right, depth, culled = cull(sad, u_right, depth, keep)
    status = status.copy()
    status[culled] = CULLED
    return u_right, depth, best_right, sad, status
