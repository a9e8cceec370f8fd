"""Input-gradient saliency, the parts that need no GPU: the reference arithmetic of tests/saliency_ref.py against autograd, the
heat-map's properties, the C ABI's new struct and constants against engine.py, and the front ends' argument check."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from oracle import mrgan_oracle as O
from tests import saliency_ref as R
from tests.helpers import Case, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem(K, D, n=40):
    case = Case(K=K, D=D, B=50, steps=1)
    return case, np.random.default_rng(3).standard_normal((n, D))


def _autograd(d, x, targets, objective):
    """the same gradient by torch.autograd in fp64 on a torch restatement of the noise-free forward"""
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    a = xt
    for l in range(5):
        a = torch.relu(a @ torch.tensor(d[2 * l]) + torch.tensor(d[2 * l + 1]))
    logits = a @ torch.tensor(d[10]) + torch.tensor(d[11])
    t = torch.tensor(np.asarray(targets), dtype=torch.int64)
    if objective == 'logit':
        obj = logits.gather(1, t[:, None]).sum()
    elif objective == 'xent':
        obj = torch.nn.functional.cross_entropy(logits, t, reduction='sum')
    else:
        obj = ((logits - torch.nn.functional.one_hot(t, logits.shape[1]).double()) ** 2).mean(dim=1).sum()
    obj.backward()                                       # rows are independent: the sum's gradient is the per-row gradients
    return xt.grad.numpy(), logits.detach().numpy()


@pytest.mark.parametrize("K,D", [(6, 16), (10, 72)])
@pytest.mark.parametrize("objective", R.OBJECTIVES)
def test_reference_gradient_equals_autograd(K, D, objective):
    case, x = _problem(K, D)
    targets = np.random.default_rng(5).integers(0, K, len(x))
    g, logits, t, _ = R.input_gradient(case.d0, x, targets, objective)
    want, want_logits = _autograd(case.d0, x, targets, objective)
    assert np.array_equal(t, targets)
    assert rel_err(logits, want_logits) < 1e-12
    assert np.abs(want).max() > 0
    assert rel_err(g, want) < 1e-10, rel_err(g, want)


def test_reference_logits_and_default_targets():
    case, x = _problem(10, 72)
    g, logits, t, _ = R.input_gradient(case.d0, x, None, 'xent')
    want = O.MRGANOracle(case.g0, case.d0).predict_logits(x)
    np.testing.assert_allclose(logits, want, rtol=1e-12, atol=1e-13)
    assert np.array_equal(t, np.argmax(want, axis=1)) and t.dtype == np.int32
    g2 = R.input_gradient(case.d0, x, t, 'xent')[0]
    assert np.array_equal(g, g2)
    # the bf16 mirror rounds: close to, and different from, the exact gradient
    gq = R.input_gradient(case.d0, x, t, 'xent', quantize='bf16')[0]
    assert 0 < rel_err(gq, g) < 0.2


def test_heatmap_properties():
    rng = np.random.default_rng(0)
    g = rng.standard_normal((9, 37)).astype(np.float32) * np.exp(rng.uniform(-12, 3, (9, 1))).astype(np.float32)
    g[4] = 0.0                                           # an all-dead row
    g[7] = 0.25                                          # constant magnitude
    g[7, ::2] *= -1
    h = R.heatmap(g)
    assert h.shape == g.shape and h.dtype == np.float32 and np.isfinite(h).all()
    assert h.min() >= 0.0 and h.max() <= 1.0
    for r in range(9):
        if r in (4, 7):
            assert not h[r].any()
        else:
            assert h[r].min() == 0.0 and h[r].max() == 1.0
            assert np.argmax(h[r]) == np.argmax(np.abs(g[r])) and np.argmin(h[r]) == np.argmin(np.abs(g[r]))
    # the reference script's three lines on one ordinary row
    x = g[0].astype(np.float64)
    a = np.abs(x / (np.sqrt(np.mean(np.square(x))) + 1e-5))
    np.testing.assert_allclose(h[0], (a - a.min()) / (a.max() - a.min()), atol=1e-6)


def test_header_struct_and_constants_match_binding():
    from mr_gan_amd import engine as E
    fields = [f for f, _ in E.SaliencyArgs._fields_]
    cnames = {'x': 'x_dev', 'idx': 'idx_dev', 'targets': 'targets_dev', 'out': 'out_dev', 'classes_out': 'classes_out_dev'}
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "mrgan_abi.h"\nint main(void) {\n'
            '  printf("%%zu", sizeof(mrgan_saliency_args));\n%s'
            '  printf(" %%d %%d %%d %%d %%d\\n", MRGAN_SAL_LOGIT, MRGAN_SAL_XENT, MRGAN_SAL_MSE, MRGAN_SAL_RAW, MRGAN_SAL_HEATMAP);\n  return 0; }\n'
            % "".join('  printf(" %%zu", offsetof(mrgan_saliency_args, %s));\n' % cnames.get(f, f) for f in fields))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", os.path.join(d, "t")])
        vals = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).split()]
    S = E.SaliencyArgs
    assert vals == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in fields] + [E.SAL_LOGIT, E.SAL_XENT, E.SAL_MSE, E.SAL_RAW, E.SAL_HEATMAP]
    assert E.SAL_OBJECTIVES == {'logit': E.SAL_LOGIT, 'xent': E.SAL_XENT, 'mse': E.SAL_MSE}
    # the head kinds behind the objectives follow each other in the objectives' order (engine.hip indexes them)
    src = open(os.path.join(ROOT, "mr_gan_amd", "csrc", "aux_kernels.h")).read()
    k = [int(re.search(r"\b%s = (\d+)" % n, src).group(1)) for n in ("HEAD_SAL_LOGIT", "HEAD_SAL_XENT", "HEAD_SAL_MSE")]
    assert k[1] == k[0] + 1 and k[2] == k[0] + 2
    assert "mrgan_input_gradient" in E.EXPORTS


@pytest.mark.parametrize("cls", ["MRGAN", "MRNN", "MRGANGroup"])
def test_front_ends_reject_an_unknown_objective(cls):
    """the objective is checked before anything touches the device, so this needs no handle"""
    from mr_gan_amd import model, mr_nn
    C = getattr(mr_nn if cls == "MRNN" else model, cls)
    obj = object.__new__(C)
    args = (0, np.zeros((2, 4), np.float32)) if cls == "MRGANGroup" else (np.zeros((2, 4), np.float32),)
    with pytest.raises(ValueError, match="objective"):
        C.saliency(obj, *args, objective='hinge')
