"""The problems of tests/evaluation_ref.py, the parts that need no GPU: these tests hold the cases, not the engine.  The error
counts the labels plant, the mirror's identities on the evaluation forward, and the condition under which the GPU tests may
compare classes at all (few rows whose class the allowed deviation could flip)."""
import math

import numpy as np
import pytest

from oracle import mrgan_oracle as O
from tests import evaluation_ref as R
from tests.helpers import rel_err

NAMES = tuple(R.PROBLEMS)


def test_shapes_are_the_chunk_edges():
    assert R.S == 128 and R.CHUNK == 384 and R.N == 2 * R.CHUNK + 5 and R.S - R.B == 78
    assert R.rows().shape == (R.N, R.D) and R.rows().dtype == np.float32
    idx = R.gather_index()
    assert len(idx) == 810 and 2 * R.CHUNK < len(idx) <= 3 * R.CHUNK and set(idx) == set(range(R.N))
    assert np.array_equal(idx, R.gather_index())
    for name in NAMES:
        case = R.problem(name)
        assert (case.D, case.B, case.K) == (R.D, R.B, R.classes(name))
        assert case.d0[-2].shape == (case.d_hidden[4], case.K)
    assert R.problem('wide').d_hidden[4] == 512 and R.problem('stock').d_hidden[4] == 250


@pytest.mark.parametrize("name", NAMES)
def test_error_counts(name):
    ref, y, K = R.reference(name), R.labels(name), R.classes(name)
    assert ref.shape == (R.N, K) and ref.dtype == np.float64
    assert R.top_two_gap(ref).min() > 0                       # no exact ties: the argmax is what any tie rule gives
    assert y.dtype == np.int32 and y.min() >= 0 and y.max() < K
    wrong = R.argmax_first(ref) != y
    assert np.array_equal(wrong, np.arange(R.N) % 3 == 0)
    for n in R.PREFIXES:
        assert R.error_count(ref[:n], y[:n]) == math.ceil(n / 3)
    assert R.error_count(ref, y) == 258
    idx = R.gather_index()
    assert R.error_count(ref[idx], y[idx]) == int(np.sum(idx % 3 == 0))
    assert len(set(y[::3])) == K                              # (the planted wrong labels reach every class)


@pytest.mark.parametrize("name", NAMES)
def test_mirror_identities(name):
    case, x = R.problem(name), R.rows().astype(np.float64)
    plain = O.MRGANMirror(case.g0, case.d0, quantize=None).predict_logits(x)
    e = rel_err(plain, R.reference(name))
    print("%s: unrounded mirror against the oracle %.1e" % (name, e))
    assert e < 1e-13
    # evaluation stays bf16 in the fp8 mode: the same bits
    assert np.array_equal(R.reference(name, 'fp8').view(np.uint64), R.reference(name, 'bf16').view(np.uint64))
    assert 0 < rel_err(R.reference(name, 'bf16'), R.reference(name)) < R.LOOSE_TOL


@pytest.mark.parametrize("name", NAMES)
def test_few_rows_are_undecided(name):
    """a condition on the inputs, not a tolerance: should another seed or shape break it, other inputs are chosen"""
    for quantize in ('bf16', 'fp8'):
        rel, bound = R.mirror_bound(name, quantize)
        assert rel >= R.BF16_TOL and bound == rel * np.abs(R.reference(name, quantize)).max()
        share = R.undecided(name, quantize).mean()
        print("%s %s: bound %.2e relative, undecided %.1f %%" % (name, quantize, rel, 100 * share))
        assert share <= R.MAX_UNDECIDED
    n32 = int(R.undecided(name).sum())
    print("%s fp32: %d undecided rows" % (name, n32))
    assert n32 <= R.MAX_UNDECIDED * R.N
