"""The layout restatements in tests/helpers.py that the kernel-level GEMM tests rely on, checked on synthetic arrays
against the literal per-element formulas of csrc/gemm.h."""
import numpy as np

from tests.helpers import colsum_groups, colsum_rows, mask_decode, mask_encode


def _relu_mask_bit(words, row, col):
    """relu_mask_bit() of gemm.h, word for word"""
    rr = row & 31
    w = int(words[row >> 5, col, (rr >> 2) & 1])
    return (w >> ((rr & 3) | ((rr >> 3) << 2))) & 1


def test_mask_decode_matches_the_device_formula():
    rng = np.random.default_rng(3)
    m, n, ldm = 75, 40, 48
    words = rng.integers(0, 1 << 16, size=(3, ldm, 2), dtype=np.uint16)
    got = mask_decode(words, m, n)
    want = np.array([[_relu_mask_bit(words, r, c) for c in range(n)] for r in range(m)], dtype=bool)
    np.testing.assert_array_equal(got, want)


def test_mask_decode_places_accumulator_registers():
    """bit r of the word of lane half h is row (r & 3) + 8 (r >> 2) + 4 h of the 32-row block"""
    for blk in range(2):
        for half in range(2):
            for r in range(16):
                words = np.zeros((2, 8, 2), dtype=np.uint16)
                words[blk, 5, half] = 1 << r
                bits = mask_decode(words, 64, 8)
                assert bits.sum() == 1 and bits[32 * blk + (r & 3) + 8 * (r >> 2) + 4 * half, 5]


def test_mask_encode_inverts_decode():
    rng = np.random.default_rng(4)
    bits = rng.random((50, 24)) < 0.5
    words = mask_encode(bits, 32)
    assert words.shape == (2, 32, 2) and words.dtype == np.uint16
    np.testing.assert_array_equal(mask_decode(words, 50, 24), bits)
    assert not words[:, 24:, :].any()
    assert not mask_decode(words, 64, 24)[50:].any()


def test_colsum_layout():
    rng = np.random.default_rng(5)
    nbatch, m, n = 3, 150, 7
    v = rng.standard_normal((nbatch, m, n))
    tiles_m, prow = colsum_rows(m, nbatch)
    assert tiles_m == 3 and prow.shape == (nbatch, m)
    assert prow[0, 63] == 0 and prow[0, 64] == 1 and prow[1, 0] == 3 and prow[2, 149] == 8
    got = colsum_groups(v)
    assert got.shape == (9, n)
    for b in range(nbatch):
        for t in range(tiles_m):
            np.testing.assert_allclose(got[b * tiles_m + t], v[b, 64 * t:64 * (t + 1)].sum(0), rtol=1e-12, atol=1e-12)
