"""The reference of mrgan_attribution (tests/attribution_ref.py) against the existing saliency reference and against what
integrated gradients must satisfy, the undecided-row cap of every GPU case, and the keyword validation -- no device."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import attribution_ref as A
from tests import saliency_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- ties to the existing reference --------------------------------------------------------------------------------
@pytest.mark.parametrize("objective", R.OBJECTIVES)
def test_one_noise_free_draw_is_the_input_gradient(objective):
    K, D, dh = A.SHAPES[0]
    case, x32 = A.problem(K, D, dh)
    want, _, t, _ = R.input_gradient(case.d0, x32.astype(np.float64), None, objective)
    got, t2, _ = A.attribution(case.d0, x32, None, objective, 'noise', 1)
    assert np.array_equal(t, t2) and np.array_equal(got, want)
    again, _, _ = A.attribution(case.d0, x32, t, objective, 'noise', 1, quantize='bf16')
    want_m = R.input_gradient(case.d0, x32.astype(np.float64), t, objective, quantize='bf16')[0]
    assert np.array_equal(again, want_m)


def test_one_path_draw_is_the_gradient_at_the_midpoint():
    K, D, dh = A.SHAPES[0]
    case, x32 = A.problem(K, D, dh)
    t = R.input_gradient(case.d0, x32.astype(np.float64), None, 'logit')[2]
    got, _, _ = A.attribution(case.d0, x32, t, 'logit', 'path', 1)
    want = R.input_gradient(case.d0, 0.5 * x32.astype(np.float64), t, 'logit')[0]
    assert np.array_equal(got, want)
    b = A.random_baseline(D)
    got, _, _ = A.attribution(case.d0, x32, t, 'logit', 'path', 1, baseline=b, multiply=1)
    mid = A.path_point(x32, b, 0, 1).astype(np.float64)
    assert np.abs(mid - 0.5 * (x32.astype(np.float64) + b)).max() < 1e-6
    want = R.input_gradient(case.d0, mid, t, 'logit')[0] * (x32.astype(np.float64) - b)
    assert np.array_equal(got, want)


def test_path_points_are_the_midpoints_in_fp32():
    x, b = np.float32([1.0, -3.5, 0.1]), np.float32([0.0, 1.0, 0.1])
    for draws in (1, 3, 16):
        for d in range(draws):
            alpha = np.float32((np.float32(d) + np.float32(0.5)) / np.float32(draws))
            v = A.path_point(x, b, d, draws)
            assert v.dtype == np.float32 and v[2] == np.float32(0.1)
            assert np.abs(v.astype(np.float64) - (b + np.float64(alpha) * (x - b))).max() <= 2.0 ** -23 * 3.5


# ---- completeness of integrated gradients --------------------------------------------------------------------------
@pytest.mark.parametrize("K,D,dh", A.SHAPES)
@pytest.mark.parametrize("base", ["zero", "random"])
def test_integrated_gradients_sum_to_the_change_of_the_class_score(K, D, dh, base):
    """e(N) = max_row |sum_j attr_j - (l_t(x) - l_t(b))| of the N-point midpoint rule: e(256) <= e(16) / 4 and
    e(256) <= 2e-2 max |l_t(x) - l_t(b)|.  Measured on this reference: e(16) / e(256) between 9.6 and 17.7, e(256) / max |want|
    between 2.4e-3 and 1.04e-2 over the six cases."""
    case, x32 = A.problem(K, D, dh)
    x = x32.astype(np.float64)
    b = A.random_baseline(D) if base == "random" else np.zeros(D, np.float32)
    _, lx, t, _ = R.input_gradient(case.d0, x, None, 'logit')
    lb = R.input_gradient(case.d0, b.astype(np.float64)[None, :], t[:1], 'logit')[1][0]
    rows = np.arange(len(t))
    want = lx[rows, t] - lb[t]
    e = {}
    for n in (16, 256):
        attr, _, _ = A.attribution(case.d0, x32, t, 'logit', 'path', n, baseline=b, multiply=1)
        e[n] = np.abs(attr.sum(axis=1) - want).max()
    print("completeness (%d, %d)%s %s baseline: e(16) %.3e e(256) %.3e ratio %.1f, e(256) / max|want| %.2e"
          % (K, D, " wide head" if dh else "", base, e[16], e[256], e[16] / e[256], e[256] / np.abs(want).max()))
    assert e[256] <= e[16] / 4
    assert e[256] <= 2e-2 * np.abs(want).max()


# ---- the undecided-row cap of every GPU case -----------------------------------------------------------------------
@pytest.mark.parametrize("K,D,dh", A.SHAPES)
def test_at_most_a_quarter_of_the_rows_of_a_gpu_case_is_undecided(K, D, dh):
    """counted on this reference, of 130 rows at 3 draws (own sigmas, input-only 0.3, path from zero, path from the random
    baseline): (6, 72) 4 8 25 16; (10, 400) 1 6 18 3; (6, 96, wide head) 8 5 22 10"""
    counts = {}
    for mode in A.MODES:
        _, _, decided = A.reference(K, D, dh, mode)
        counts[mode] = int(A.N - decided.sum())
    print("undecided rows of %d (%d, %d)%s:" % (A.N, K, D, " wide head" if dh else ""), counts)
    for mode, c in counts.items():
        assert c <= 0.25 * A.N, (mode, c)


# ---- keyword validation without a device ---------------------------------------------------------------------------
def test_saliency_keywords_are_validated_without_a_device():
    from mr_gan_amd import engine as E
    plan = E.attribution_plan
    assert plan('gradient') == dict(method=E.ATTR_NOISE, draws=1, sigma_input=0.0, sigma_hidden=0.0, baseline=None, multiply=0)
    assert plan('gradient', times_input=True) == dict(method=E.ATTR_NOISE, draws=1, sigma_input=0.0, sigma_hidden=0.0, baseline=None,
                                                      multiply=1)
    p = plan('smoothgrad')
    assert (p['method'], p['draws'], p['multiply'], p['baseline']) == (E.ATTR_NOISE, 16, 0, None)
    assert (np.float32(p['sigma_input']), np.float32(p['sigma_hidden'])) == (np.float32(0.3), np.float32(0.5))
    p = plan('smoothgrad', draws=5, sigma=0.25, times_input=True)
    assert (p['draws'], p['sigma_input'], p['sigma_hidden'], p['multiply']) == (5, 0.25, 0.0, 1)
    p = plan('smoothgrad', sigma=(0.1, 0.2))
    assert (p['sigma_input'], p['sigma_hidden']) == (0.1, 0.2)
    p = plan('integrated', d_in=4)
    assert (p['method'], p['draws'], p['multiply'], p['baseline'], p['sigma_input']) == (E.ATTR_PATH, 16, 1, None, 0.0)
    p = plan('integrated', draws=E.ATTR_MAX_DRAWS, baseline=[0, 1, 2, 3], d_in=4)
    assert p['baseline'].dtype == np.float32 and p['baseline'].shape == (4,) and p['draws'] == 4096
    for bad in (dict(method='smooth'), dict(method='gradient', draws=4), dict(method='gradient', sigma=0.1),
                dict(method='gradient', baseline=[0.0] * 4), dict(method='smoothgrad', draws=0),
                dict(method='smoothgrad', draws=E.ATTR_MAX_DRAWS + 1), dict(method='smoothgrad', draws=2.5),
                dict(method='smoothgrad', draws=True), dict(method='smoothgrad', sigma=-0.1), dict(method='smoothgrad', sigma=float('nan')),
                dict(method='smoothgrad', sigma=(0.1, float('inf'))), dict(method='smoothgrad', sigma=(0.1, 0.2, 0.3)),
                dict(method='smoothgrad', sigma='big'), dict(method='smoothgrad', baseline=[0.0] * 4),
                dict(method='integrated', sigma=0.1), dict(method='integrated', baseline=[0.0] * 3),
                dict(method='integrated', baseline=[[0.0] * 4]), dict(method='integrated', baseline=[0.0, 0.0, float('nan'), 0.0])):
        with pytest.raises(ValueError):
            plan(d_in=4, **bad)


def test_constants_match_the_header():
    from mr_gan_amd import engine as E
    src = open(os.path.join(ROOT, "include", "mrgan_abi.h")).read()
    header = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bMRGAN_(ATTR_[A-Z_]+)\s*=\s*(\d+)", src)}
    assert header == dict(ATTR_NOISE=E.ATTR_NOISE, ATTR_PATH=E.ATTR_PATH, ATTR_MAX_DRAWS=E.ATTR_MAX_DRAWS, ATTR_NOISE_SEG=E.ATTR_NOISE_SEG)
    assert E.ATTR_NOISE_SEG == A.NOISE_SEG == 255
    assert "fmaf(alpha_d, x - b, b)" in src and "(d + 0.5f) / (float)draws" in src
    # the Python struct is the header's: the saliency fields first, then the new ones
    names = [f[0] for f in E.AttributionArgs._fields_]
    assert names[:len(E.SaliencyArgs._fields_)] == [f[0] for f in E.SaliencyArgs._fields_]
    assert names[len(E.SaliencyArgs._fields_):] == ["method", "draws", "sigma_input", "sigma_hidden", "baseline", "multiply", "reserved"]


def test_struct_layout_matches_the_header():
    """mrgan_attribution_args against engine.AttributionArgs, and mrgan_saliency_args (which must stay as it is) as its prefix"""
    from mr_gan_amd import engine as E
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "mrgan_abi.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(mrgan_saliency_args), sizeof(mrgan_attribution_args), offsetof(mrgan_attribution_args, classes_out_dev),
         offsetof(mrgan_attribution_args, method), offsetof(mrgan_attribution_args, sigma_hidden), offsetof(mrgan_attribution_args, baseline_dev),
         offsetof(mrgan_attribution_args, multiply));
  return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", os.path.join(d, "t")])
        vals = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).split()]
    T = E.AttributionArgs
    assert vals == [ctypes.sizeof(E.SaliencyArgs), ctypes.sizeof(T), T.classes_out.offset, T.method.offset, T.sigma_hidden.offset,
                    T.baseline.offset, T.multiply.offset]
    assert ctypes.sizeof(E.SaliencyArgs) == 72 and E.SaliencyArgs.classes_out.offset == T.classes_out.offset == 64
