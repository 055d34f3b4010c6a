"""GPU: hamming_argmin2_kernel / hamming_matrix_kernel (sivo_amd/csrc/match.hip) at the shapes where a wave-per-query kernel
goes wrong — a partial last workgroup (four queries each), candidate lists of exactly 0 / 1 / 2 / 63 / 64 / 65 / 128 / 129 / 300,
lists of 256-distance candidates only, ties inside one lane (64 positions apart) and between neighbour lanes — bit for bit
against the oracle's sequential scan."""
import numpy as np
import pytest
import torch

from sivo_amd import matcher

pytestmark = pytest.mark.gpu
LENS = (0, 1, 2, 63, 64, 65, 128, 129, 300)


def _both(oracle, A, B, off, idx):
    off = np.asarray(off, np.int32); idx = np.asarray(idx, np.int32)
    got = matcher.argmin2(A, B, off, idx)
    want = oracle.hamming_argmin2(A, B, off, idx)
    for g, w, what in zip(got, want, ("best index", "best distance", "second distance")):
        assert np.array_equal(g, w), (what, g, w)
    return got


def _lists(rng, lens, nB):
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return off, rng.integers(0, nB, int(off[-1])).astype(np.int32)


@pytest.mark.parametrize("nA", [1, 2, 3, 5, 63, 65])
@pytest.mark.parametrize("shift", [0, 4])
def test_argmin2_partial_workgroups_and_list_lengths(oracle, nA, shift):
    """Every nA leaves the last workgroup partial (or is one); the list lengths cycle through LENS, from another start per `shift`."""
    rng = np.random.default_rng(100 * nA + shift)
    nB = 400
    A = rng.integers(0, 256, (nA, 32), dtype=np.uint8); B = rng.integers(0, 256, (nB, 32), dtype=np.uint8)
    lens = np.array([LENS[(q + shift) % len(LENS)] for q in range(nA)])
    off, idx = _lists(rng, lens, nB)
    bi, bd, sd = _both(oracle, A, B, off, idx)
    assert (bi[lens == 0] == -1).all() and (bd[lens == 0] == 256).all() and (sd[lens == 0] == 256).all()
    assert (bi[lens == 1] == idx[off[:-1][lens == 1]]).all() and (sd[lens == 1] == 256).all()       # one candidate: second = 256
    assert (bi[lens > 0] >= 0).all() and (sd[lens > 1] < 256).all()


@pytest.mark.parametrize("length", [1, 2, 64, 65, 129])
def test_argmin2_lists_of_complements_only(oracle, length):
    """Every candidate at distance 256: the reference's `dist < 256` never holds — index -1, best 256, second 256.  One real
    candidate among them is best with second 256, wherever it stands."""
    rng = np.random.default_rng(length)
    nA = 6
    A = rng.integers(0, 256, (nA, 32), dtype=np.uint8)
    B = np.concatenate([~A, A ^ np.uint8(1)])                      # rows 0 .. 5: complements; rows 6 .. 11: distance 32
    off = (np.arange(nA + 1) * length).astype(np.int32)
    idx = np.repeat(np.arange(nA), length).astype(np.int32)
    bi, bd, sd = _both(oracle, A, B, off, idx)
    assert (bi == -1).all() and (bd == 256).all() and (sd == 256).all()
    for pos in {0, length // 2, length - 1}:
        idx2 = idx.copy(); idx2[off[:-1] + pos] = np.arange(nA) + nA
        bi, bd, sd = _both(oracle, A, B, off, idx2)
        assert np.array_equal(bi, np.arange(nA) + nA) and (bd == 32).all() and (sd == 256).all()


@pytest.mark.parametrize("gap", [1, 64, 128])
@pytest.mark.parametrize("p", [0, 5, 63, 70])
def test_argmin2_ties_keep_the_earlier_candidate(oracle, p, gap):
    """The same descriptor in two rows of B, listed at positions p and p + gap: gap 64 / 128 puts both into one lane, gap 1 into
    neighbour lanes (p = 63: the two ends of the wave).  The earlier position wins, whichever row index is smaller, and the second
    distance equals the best.  The third query lists ONE row twice."""
    rng = np.random.default_rng(1000 * gap + p)
    nB, length = 300, 200
    a = rng.integers(0, 256, (1, 32), dtype=np.uint8); B = rng.integers(0, 256, (nB, 32), dtype=np.uint8)
    lo, hi = 7, 250
    B[lo] = B[hi] = a[0] ^ np.uint8(1)                             # distance 32: far below the random rows
    base = rng.integers(10, 240, length).astype(np.int32)
    for first, second in ((lo, hi), (hi, lo), (lo, lo)):
        idx = base.copy(); idx[p], idx[p + gap] = first, second
        bi, bd, sd = _both(oracle, a, B, [0, length], idx)
        assert bi[0] == first and bd[0] == 32 and sd[0] == 32


@pytest.mark.parametrize("nA", [1, 5, 66])
@pytest.mark.parametrize("nB", [1, 2, 63, 64, 65, 257])
def test_bruteforce_shapes(oracle, nA, nB):
    rng = np.random.default_rng(10 * nA + nB)
    A = rng.integers(0, 256, (nA, 32), dtype=np.uint8); B = rng.integers(0, 256, (nB, 32), dtype=np.uint8)
    if nB >= 63:
        B[nB - 1] = B[nB - 63]                                     # a tie between two lanes' candidates / inside one lane (nB = 257: 194, 256)
    bi, bd, sd = (t.cpu().numpy() for t in matcher.bruteforce(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()))
    D = oracle.hamming_matrix(A, B)
    assert D.max() < 256
    assert np.array_equal(bd, D.min(1)) and np.array_equal(bi, D.argmin(1))                # argmin: the first minimum
    if nB == 1:
        assert (sd == 256).all()
    else:
        assert np.array_equal(sd, np.sort(D, 1)[:, 1])
    # the same through the oracle's sequential scan over the full list
    off = (np.arange(nA + 1) * nB).astype(np.int32); idx = np.tile(np.arange(nB, dtype=np.int32), nA)
    obi, obd, osd = oracle.hamming_argmin2(A, B, off, idx)
    assert np.array_equal(bi, obi) and np.array_equal(bd, obd) and np.array_equal(sd, osd)


def test_bruteforce_complement_and_empty_b(oracle):
    """A single row at distance 256 is no match (`dist < 256`); an empty B (the binding passes a null pointer with n_b = 0, which
    the entry point allows) gives -1 / 256 / 256 for every query."""
    rng = np.random.default_rng(3)
    A = rng.integers(0, 256, (5, 32), dtype=np.uint8)
    dA = torch.from_numpy(A).cuda()
    bi, bd, sd = (t.cpu().numpy() for t in matcher.bruteforce(dA[:1], torch.from_numpy(~A[:1]).cuda()))
    assert bi[0] == -1 and bd[0] == 256 and sd[0] == 256
    bi, bd, sd = (t.cpu().numpy() for t in matcher.bruteforce(dA, torch.empty((0, 32), dtype=torch.uint8, device="cuda")))
    assert (bi == -1).all() and (bd == 256).all() and (sd == 256).all()


@pytest.mark.parametrize("nA,nB", [(32, 256), (31, 513), (1, 257)])
def test_hamming_matrix_tile_edges(oracle, nA, nB):
    """HM_ROWS = 32 rows x 256 columns per workgroup: exactly one tile, one row short with a third column tile of one thread, one row."""
    rng = np.random.default_rng(nA * nB)
    A = rng.integers(0, 256, (nA, 32), dtype=np.uint8); B = rng.integers(0, 256, (nB, 32), dtype=np.uint8)
    B[nB - 1] = ~A[nA - 1]; B[0] = A[nA - 1]
    ref = oracle.hamming_matrix(A, B)
    assert ref[nA - 1, nB - 1] == 256 and ref[nA - 1, 0] == 0
    assert np.array_equal(matcher.descriptor_distance_matrix(A, B), ref)
    out = matcher.descriptor_distance_matrix(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda())
    assert np.array_equal(out.cpu().numpy(), ref)
