"""mrgan_input_gradient on the GPU: the engine's own forward and dX products as a per-row input gradient, against the reference
arithmetic of tests/saliency_ref.py (fp64 for the fp32 engine, the bf16 mirror for the bf16 engine), and what the call must
leave alone."""
import ctypes as C

import numpy as np
import pytest
import torch

from mr_gan_amd import engine as E
from tests import parity as P
from tests import saliency_gpu as G
from tests import saliency_ref as R
from tests.helpers import Case, cosine, frob_rel_err, rel_err

pytestmark = pytest.mark.gpu

B, WIDE_HEAD, FP32_TOL = G.B, G.WIDE_HEAD, G.FP32_TOL      # B = 50: S = 128, so 200 rows are two chunks
_problem, _reference, _engine = R.decided_problem, R.reference, G.engine


def _grad(eng, x, targets=None, objective='xent', post=E.SAL_RAW, **kw):
    t = None if targets is None else P.to_dev(targets, torch.int32)
    out, cls = eng.input_gradient(x if isinstance(x, torch.Tensor) else P.to_dev(x), t, E.SAL_OBJECTIVES[objective], post, **kw)
    return out.cpu().numpy(), cls.cpu().numpy()


# ---- 1. fp32 against fp64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,D,n", [(6, 16, 77), (6, 72, 200), (10, 400, 200)])
def test_fp32_raw_gradient_matches_fp64(K, D, n):
    case, x32, _, decided = _problem(K, D, n)
    print("undecided rows: %d of %d" % (n - decided.sum(), n))
    assert n - decided.sum() <= 0.1 * n
    eng = _engine(case, D, E.F32)
    errs = {}
    for objective in R.OBJECTIVES:
        want, t = _reference(K, D, n, objective, False)
        got, cls = _grad(eng, x32, t, objective)
        assert got.shape == (n, D) and np.isfinite(got).all() and np.array_equal(cls, t)
        errs[objective] = rel_err(got[decided], want[decided])
    eng.close()
    print("rel_err per objective:", errs)
    for objective, e in errs.items():
        assert e < FP32_TOL, (objective, e)


# ---- 2. explicit targets versus argmax ------------------------------------------------------------------------------
def test_targets_default_to_the_predicted_class():
    K, D, n = 6, 72, 200
    case, x32, _, decided = _problem(K, D, n)
    eng = _engine(case, D, E.F32)
    xd = P.to_dev(x32)
    got, cls = _grad(eng, xd)
    assert cls.dtype == np.int32
    assert np.array_equal(cls, np.argmax(eng.predict_logits(xd).cpu().numpy(), axis=1))
    again, cls2 = _grad(eng, xd, cls)
    assert np.array_equal(cls2, cls) and np.array_equal(again.view(np.uint32), got.view(np.uint32))
    want, t = _reference(K, D, n, 'xent', True)
    planted, cls3 = _grad(eng, xd, t)
    eng.close()
    assert np.array_equal(cls3, t) and (t != cls).mean() > 0.9
    e = rel_err(planted[decided], want[decided])
    print("planted targets: rel_err %.2e" % e)
    assert e < FP32_TOL, e


# ---- 3. gather and pitches -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [E.F32, E.BF16])
def test_gather_and_pitches_reproduce_the_plain_call(dtype):
    K, D, n = 6, 72, 200
    case, x32, _, _ = _problem(K, D, n)
    eng = _engine(case, D, dtype)
    rng = np.random.default_rng(11)
    idx = np.concatenate([rng.permutation(n), rng.integers(0, n, 37)]).astype(np.int32)      # permuted, then repeated
    plain, cls = _grad(eng, x32[idx])
    out, cls_out = G.sentinel_buffers(len(idx), D)
    eng.input_gradient(G.wide_rows(x32), None, E.SAL_XENT, E.SAL_RAW, idx=P.to_dev(idx, torch.int32), out=out, classes_out=cls_out)
    got = out.cpu().numpy()
    eng.close()
    assert np.array_equal(got[:, :D].view(np.uint32), plain.view(np.uint32))
    assert (got[:, D:] == G.SENT).all()
    assert np.array_equal(cls_out.cpu().numpy(), cls)


# ---- 4. bf16 against the bf16 mirror -------------------------------------------------------------------------------
@pytest.mark.parametrize("K,D,n,d_hidden", [(6, 400, 130, None), (10, 96, 130, None), (6, 96, 130, WIDE_HEAD)])
def test_bf16_raw_gradient_matches_the_mirror(K, D, n, d_hidden):
    """parity.grad_parity's rule for bf16 gradients, on the per-row input gradients of one call (Frobenius errors over the whole
    matrix): err(engine, mirror) < max(3e-3, 0.6 err(mirror, fp64)), and loosely the direction against fp64.  The targets are
    the fp64 argmax for all three, so a near-tie between two classes does not enter."""
    case, x32, _, _ = _problem(K, D, n, d_hidden)
    want_o, t = _reference(K, D, n, 'xent', False, None, d_hidden)
    want_m, _ = _reference(K, D, n, 'xent', False, 'bf16', d_hidden)
    eng = _engine(case, D, E.BF16)
    got, cls = _grad(eng, x32, t)
    eng.close()
    em, eo, emo = frob_rel_err(got, want_m), frob_rel_err(got, want_o), frob_rel_err(want_m, want_o)
    cs = cosine(got, want_o)
    print("bf16 input gradient (%d, %d, %d)%s: engine-mirror %.2e engine-fp64 %.2e mirror-fp64 %.2e cosine %.5f"
          % (K, D, n, " wide head" if d_hidden else "", em, eo, emo, cs))
    assert np.array_equal(cls, t) and np.isfinite(got).all()
    assert em < max(3e-3, 0.6 * emo), (em, emo)
    assert cs > 0.98, cs


# ---- 5. heat-map ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [E.F32, E.BF16])
def test_heatmap_is_the_reference_map_of_the_raw_gradient(dtype):
    K, D, n = 6, 72, 200
    case, x32, _, _ = _problem(K, D, n)
    eng = _engine(case, D, dtype)
    xd = P.to_dev(x32)
    raw, cls = _grad(eng, xd)
    hm, cls2 = _grad(eng, xd, post=E.SAL_HEATMAP)
    eng.close()
    want = R.heatmap(raw)
    print("heat-map: max abs difference %.2e" % np.abs(hm - want).max())
    assert np.array_equal(cls, cls2)
    assert hm.min() >= 0.0 and hm.max() <= 1.0
    assert np.abs(hm - want).max() < 1e-5
    assert (hm.max(axis=1) == 1.0).all() and (hm.min(axis=1) == 0.0).all()


@pytest.mark.parametrize("dtype", [E.F32, E.BF16])
def test_heatmap_of_an_all_dead_row_is_zero(dtype):
    eng, x = G.dead_row_engine(dtype, 6, 72, 200)
    raw, _ = _grad(eng, x)
    hm, _ = _grad(eng, x, post=E.SAL_HEATMAP)
    eng.close()
    assert not raw[2].any() and np.abs(raw[[0, 1, 3, 4]]).max(axis=1).min() > 0
    assert np.isfinite(hm).all() and not hm[2].any() and (hm[[0, 1, 3, 4]].max(axis=1) == 1.0).all()


# ---- 6. training is undisturbed ------------------------------------------------------------------------------------
_state, _assert_same_state, _assert_finite_state = G.state, G.assert_same_state, G.assert_finite_state


def test_training_is_undisturbed_by_saliency_calls():
    def disturb(eng, big, t):
        out, _ = eng.input_gradient(big, None, E.SAL_XENT, E.SAL_HEATMAP if t == 1 else E.SAL_RAW)
        assert bool(torch.isfinite(out).all())
    G.training_is_undisturbed_by(disturb)


def test_training_is_undisturbed_by_evaluation_calls():
    """predict_logits / eval_error use the training activations as scratch.  A ragged batch (B = 50, S = 128) of a bf16 handle
    reduces its weight gradients over all S rows of a segment, zero dY x the padding rows of X: NaN rows (3 S + 7 of them: two
    chunks, every padding row of every segment) in front of every step must leave no trace.  Only a non-finite value shows a
    missing re-zero (0 x NaN); a large finite one meets exact zeros."""
    D = 16
    case = Case(D=D, B=B, steps=2, device_z=True)
    n = 3 * 128 + 7
    nan = torch.full((n, D), float("nan"), device=P.DEV)
    labels = P.to_dev(np.arange(n) % 6, torch.int32)
    states = []
    for disturb in (False, True):
        eng = P.engine(D, B, E.BF16)
        P.load(eng, case)
        for t in range(case.steps):
            if disturb:
                assert eng.predict_logits(nan).shape == (n, 6)
                eng.eval_error(nan, labels)
            eng.disc_step(P.disc_args(case, t, True))
            eng.gen_step(P.gen_args(case, t, True))
        states.append(_state(eng))
        eng.close()
    assert states[0][1] == 2 * case.steps
    _assert_finite_state(states[0])
    _assert_same_state(*states)


def test_group_training_is_undisturbed_by_evaluation_calls():
    """the same on a group handle of two models: NaN rows evaluated on model 1 between two grouped (D, G) steps; both models'
    states equal the undisturbed group's"""
    D, G = 16, 2
    cases = [Case(D=D, B=B, steps=2, seed=7 + m, device_z=True) for m in range(G)]
    n = 3 * 128 + 7
    nan = torch.full((n, D), float("nan"), device=P.DEV)
    labels = P.to_dev(np.arange(n) % 6, torch.int32)
    states = []
    for disturb in (False, True):
        eng = P.engine(D, B, E.BF16, models=G)
        for m, case in enumerate(cases):
            eng.select_model(m)
            P.load(eng, case)
        for t in range(cases[0].steps):
            if disturb and t == 1:
                eng.select_model(1)
                assert eng.predict_logits(nan).shape == (n, 6)
                eng.eval_error(nan, labels)
            eng.disc_step_group(E.Engine.disc_group_args(P.to_dev(np.stack([c.x_lab[t] for c in cases])),
                                                         P.to_dev(np.stack([c.labels[t] for c in cases]), torch.int32),
                                                         P.to_dev(np.stack([c.x_unl[t] for c in cases]))))
            eng.gen_step_group(E.Engine.gen_group_args(P.to_dev(np.stack([c.x_unl2[t] for c in cases]))))
        per_model = []
        for m in range(G):
            eng.select_model(m)
            per_model.append(_state(eng))
        states.append(per_model)
        eng.close()
    for m in range(G):
        assert states[0][m][1] == 2 * cases[0].steps
        _assert_finite_state(states[0][m])
        _assert_same_state(states[0][m], states[1][m])
    assert not np.array_equal(states[0][0][0][0], states[0][1][0][0])      # (the models differ from each other)


def test_graph_replay_is_undisturbed_by_saliency_calls():
    G.graph_replay_is_undisturbed_by(lambda eng, big, t: eng.input_gradient(big, None, E.SAL_XENT, E.SAL_RAW))


# ---- 7. determinism ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [E.F32, E.BF16])
def test_two_calls_give_identical_bits(dtype):
    K, D, n = 10, 400, 200
    case, x32, _, _ = _problem(K, D, n)
    eng = _engine(case, D, dtype)
    xd = P.to_dev(x32)
    for post in (E.SAL_RAW, E.SAL_HEATMAP):
        a, ca = _grad(eng, xd, post=post)
        b, cb = _grad(eng, xd, post=post)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(ca, cb)
    eng.close()


# ---- 8. group handle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_group_handle_serves_the_selected_model(dtype):
    for maps, _ in G.group_handle_serves_the_selected_model(dtype, 77):
        assert maps.max() == 1.0


# ---- 9. the baseline's front end -----------------------------------------------------------------------------------
def test_mrnn_saliency():
    from mr_gan_amd.mr_nn import MRNN
    D, K, n = 24, 10, 100
    rng = np.random.default_rng(4)
    y = (np.arange(n) % K).astype(np.int32)
    X = (rng.standard_normal((n, D)) + 2.0 * np.eye(K, D)[y]).astype(np.float32)
    nn = MRNN(D, batch_size=20, num_classes=K, seed=5)
    nn.fit(X, y, epochs=1)
    maps, cls = nn.saliency(X[:33])
    raw, cls2 = nn.saliency(X[:33], y=y[:33], objective='logit', heatmap=False)
    pred = np.argmax(nn.predict_logits(X[:33]), axis=1)
    nn.engine.close()
    assert maps.shape == (33, D) and cls.shape == (33,) and maps.dtype == np.float32 and cls.dtype == np.int32
    assert np.isfinite(maps).all() and maps.min() >= 0.0 and maps.max() <= 1.0
    assert np.array_equal(cls, pred)
    assert raw.shape == (33, D) and np.isfinite(raw).all() and np.array_equal(cls2, y[:33])


# ---- 10. refusals --------------------------------------------------------------------------------------------------
def test_fp8_handle_is_refused():
    G.fp8_handle_is_refused(lambda eng, x: eng.input_gradient(x))


def test_bad_arguments_are_refused():
    D = 16
    eng = P.engine(D, B, E.F32)
    x = torch.zeros((8, D), device=P.DEV)
    out = torch.zeros((8, D), device=P.DEV)
    good = dict(x=x.data_ptr(), ld_x=D, n=8, objective=E.SAL_XENT, post=E.SAL_RAW, out=out.data_ptr(), ld_out=D)

    def call(**kw):
        a = E.SaliencyArgs()
        for k, v in dict(good, **kw).items():
            setattr(a, k, v)
        return eng.lib.mrgan_input_gradient(eng.handle, C.byref(a), E._stream())
    assert call() == 0
    for bad in (dict(x=None), dict(out=None), dict(ld_x=D - 1), dict(ld_out=D - 1), dict(objective=3), dict(objective=-1), dict(post=2),
                dict(n=-1)):
        assert call(**bad) == -2, bad
        assert b"input_gradient" in eng.lib.mrgan_last_error()
    assert eng.lib.mrgan_input_gradient(eng.handle, None, E._stream()) == -2
    assert call(n=0) == 0
    eng.close()


# ---- 11. kernel names ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d_hidden", [(E.F32, None), (E.BF16, None), (E.BF16, WIDE_HEAD)])
def test_kernels_of_one_call(dtype, d_hidden):
    """the scalar head and the one kernel that writes a map; no matrix-core head, no chain launch, no weight gradient, no update"""
    eng, x = G.profiled_engine(dtype, d_hidden, 130)
    eng.profile_begin()
    eng.input_gradient(x, None, E.SAL_XENT, E.SAL_HEATMAP)
    prof = eng.profile_end()
    eng.close()
    print(sorted((k, v[1]) for k, v in prof.items()))
    assert prof["attribution_accum_kernel"][1] == 2 and prof["head_kernel"][1] == 2 and prof["stage_kernel"][1] == 2
    G.assert_no_training_kernels(prof, 20)
