"""The problems and references of the evaluation tests (mrgan_predict_logits, mrgan_eval_error): numpy only.

Every problem has D = 96 and B = 50, so S = 128: the evaluation walks the caller's rows in chunks of 3 S = 384 rows, and a
segment has 78 padding rows.  X has 773 = 2 * 384 + 5 rows: two full chunks and a tail of five.  The references are the fp64
oracle (fp32 handles) and the bf16 mirror (bf16 and fp8 handles: the evaluation of an fp8 handle stays in the bf16 dataflow,
which MRGANMirror('fp8').predict_logits restates).

Labels: with t the first-index argmax of the fp64 logits, y[i] = t[i] unless i % 3 == 0, where it is another class -- so the
fp64 forward is wrong on exactly ceil(n / 3) rows of every prefix of n rows, and on 258 of the 773.

A row is *undecided* when its top-two gap in the reference is within what the engine may deviate: there the engine's argmax may
differ from the reference's.  For bf16 / fp8 handles the deviation allowed per logit is the bound of the logits test,
max(2e-3, 0.6 rel_err(mirror, fp64)) max|mirror|, and a gap below twice that is undecided; for fp32 handles a gap below
2e-5 max|fp64| (twice the 1e-5 of the logits test)."""
import functools

import numpy as np

from oracle import mrgan_oracle as O
from tests.helpers import Case, rel_err
from tests.saliency_ref import WIDE_HEAD

D, B, S, N = 96, 50, 128, 773
CHUNK = 3 * S
PROBLEMS = {'stock': (6, None), 'k10': (10, None), 'wide': (6, WIDE_HEAD)}      # name -> (classes, d_hidden or the reference's)
PREFIXES = (1, 127, 128, 129, 383, 384, 385, 773)      # around S, around 3 S, the whole set
SUFFIXES = (1, 129, 385)
BF16_TOL, MIRROR_FRAC, LOOSE_TOL, FP32_TOL = 2e-3, 0.6, 3e-2, 1e-5
MAX_UNDECIDED = 0.10


@functools.lru_cache(maxsize=None)
def rows():
    """the 773 rows as the engine gets them (never modified)"""
    return np.random.default_rng(11).standard_normal((N, D)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def problem(name):
    K, d_hidden = PROBLEMS[name]
    kw = dict(d_hidden=d_hidden) if d_hidden else {}
    return Case(D=D, B=B, steps=1, K=None if K == 6 else K, **kw)


def d_hidden(name):
    """the engine's d_hidden argument: None for the reference widths"""
    return PROBLEMS[name][1]


def classes(name):
    return PROBLEMS[name][0]


@functools.lru_cache(maxsize=None)
def reference(name, quantize=None):
    """logits [773, K] in fp64: the oracle (quantize None), or the mirror with the engine's storage roundings ('bf16' | 'fp8')"""
    case = problem(name)
    x = rows().astype(np.float64)
    ref = O.MRGANOracle(case.g0, case.d0) if quantize is None else O.MRGANMirror(case.g0, case.d0, quantize=quantize)
    out = ref.predict_logits(x)
    out.setflags(write=False)
    return out


def argmax_first(logits):
    """the class of every row, ties to the first (np.argmax's rule and head_kernel's)"""
    return np.argmax(logits, axis=1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def labels(name):
    K = classes(name)
    t = argmax_first(reference(name))
    i = np.arange(N)
    return np.where(i % 3 != 0, t, (t + 1 + i % (K - 1)) % K).astype(np.int32)


def gather_index():
    """810 rows: a permutation of the 773, then 37 repeats -- three chunks"""
    rng = np.random.default_rng(11)
    return np.concatenate([rng.permutation(N), rng.integers(0, N, 37)]).astype(np.int32)


def top_two_gap(logits):
    s = np.sort(logits, axis=1)
    return s[:, -1] - s[:, -2]


def mirror_bound(name, quantize):
    """(the relative bound of engine against mirror, the same as an absolute bound on a logit)"""
    mir, ref = reference(name, quantize), reference(name)
    rel = max(BF16_TOL, MIRROR_FRAC * rel_err(mir, ref))
    return rel, rel * float(np.max(np.abs(mir)))


@functools.lru_cache(maxsize=None)
def undecided(name, quantize=None):
    """bool [773]: rows whose class the engine may decide otherwise than the reference of `quantize`"""
    ref = reference(name, quantize)
    if quantize is None:
        u = top_two_gap(ref) < 2 * FP32_TOL * float(np.max(np.abs(ref)))
    else:
        u = top_two_gap(ref) < 2 * mirror_bound(name, quantize)[1]
    u.setflags(write=False)
    return u


def error_count(logits, y):
    return int(np.sum(argmax_first(logits) != y))
