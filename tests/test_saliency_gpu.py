"""mrgan_input_gradient on the GPU: the engine's own forward and dX products as a per-row input gradient, against the reference
arithmetic of tests/saliency_ref.py (fp64 for the fp32 engine, the bf16 mirror for the bf16 engine), and what the call must
leave alone."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from mr_gan_amd import engine as E
from oracle import mrgan_oracle as O
from tests import parity as P
from tests import saliency_ref as R
from tests.helpers import Case, cosine, frob_rel_err, rel_err

pytestmark = pytest.mark.gpu

B = 50                                # local batch of every handle here: S = 128, so padding rows exist and 200 rows are two chunks
WIDE_HEAD = (256, 256, 256, 256, 512)  # a feature layer of two HEAD_CHUNKs
DECIDED = 1e-5                        # a row is decided when every fp64 pre-activation is at least this far from zero
FP32_TOL = 2e-4                       # parity.fp32_gradients_match_oracle's bound on gradients behind the same dX chain


@functools.lru_cache(maxsize=None)
def _problem(K, D, n, d_hidden=None):
    """(case, rows as the engine gets them, the same rows in fp64, decided rows); shared, never modified"""
    kw = dict(d_hidden=d_hidden) if d_hidden else {}
    case = Case(K=K, D=D, B=B, steps=1, **kw)
    x32 = np.random.default_rng(3).standard_normal((n, D)).astype(np.float32)
    x = x32.astype(np.float64)
    decided = np.all([np.abs(p).min(axis=1) >= DECIDED for p in R.preactivations(case.d0, x)], axis=0)
    return case, x32, x, decided


@functools.lru_cache(maxsize=None)
def _reference(K, D, n, objective, planted, quantize=None, d_hidden=None):
    """fp64 (or mirror) gradient at the fp64 argmax, or at planted targets (argmax + 1); shared, never modified"""
    case, _, x, _ = _problem(K, D, n, d_hidden)
    t = R.input_gradient(case.d0, x, None, objective)[2]
    if planted:
        t = ((t + 1) % K).astype(np.int32)
    g, _, t, _ = R.input_gradient(case.d0, x, t, objective, quantize=quantize)
    return g, t


def _engine(case, D, dtype, **kw):
    if case.d_hidden != tuple(O.D_HIDDEN):
        kw['d_hidden'] = case.d_hidden
    eng = P.engine(D, B, dtype, num_classes=case.K, **kw)
    P.load(eng, case)
    return eng


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
    wide = torch.full((n, D + 9), float("nan"), device=P.DEV)
    wide[:, :D] = P.to_dev(x32)
    SENT = -768.0
    out = torch.full((len(idx), D + 5), SENT, device=P.DEV)
    cls_out = torch.full((len(idx),), -1, dtype=torch.int32, device=P.DEV)
    eng.input_gradient(wide, None, E.SAL_XENT, E.SAL_RAW, idx=P.to_dev(idx, torch.int32), out=out, classes_out=cls_out)
    got = out.cpu().numpy()
    eng.close()
    assert np.array_equal(got[:, :D].view(np.uint32), plain.view(np.uint32))
    assert (got[:, D:] == SENT).all()
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
    K, D, n = 6, 72, 200
    case, x32, _, _ = _problem(K, D, n)
    eng = P.engine(D, B, dtype, num_classes=K)
    d = [p.astype(np.float32) for p in case.d0]
    d[1] = -np.abs(d[1]) - 0.5                          # first-layer biases negative: a zero row has every unit of layer 1 dead
    eng.set_weights(E.NET_D, d)
    x = x32[:5].copy()
    x[2] = 0.0
    raw, _ = _grad(eng, x)
    hm, _ = _grad(eng, x, post=E.SAL_HEATMAP)
    eng.close()
    assert not raw[2].any() and np.abs(raw[[0, 1, 3, 4]]).max(axis=1).min() > 0
    assert np.isfinite(hm).all() and not hm[2].any() and (hm[[0, 1, 3, 4]].max(axis=1) == 1.0).all()


# ---- 6. training is undisturbed ------------------------------------------------------------------------------------
def _state(eng):
    out = []
    for net in (E.NET_G, E.NET_D):
        out += eng.get_weights(net) + eng.get_slot(net, 0) + eng.get_slot(net, 1)
    return out, eng.get_iterations(), eng.read_metrics(reset=False)


def _assert_same_state(a, b):
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert a[1] == b[1]
    assert np.array_equal(np.asarray(a[2], np.float32).view(np.uint32), np.asarray(b[2], np.float32).view(np.uint32))


def test_training_is_undisturbed_by_saliency_calls():
    D = 400
    case = Case(D=D, B=B, steps=3, device_z=True)
    big = P.to_dev(1e3 * np.random.default_rng(9).standard_normal((3 * 64 + 7, D)).astype(np.float32))
    states = []
    for disturb in (False, True):
        eng = P.engine(D, B, E.BF16)
        P.load(eng, case)
        for t in range(case.steps):
            if disturb:
                out, _ = eng.input_gradient(big, None, E.SAL_XENT, E.SAL_HEATMAP if t == 1 else E.SAL_RAW)
                assert bool(torch.isfinite(out).all())
            eng.disc_step(P.disc_args(case, t, True))
            eng.gen_step(P.gen_args(case, t, True))
        states.append(_state(eng))
        eng.close()
    assert states[0][1] == 2 * case.steps
    _assert_same_state(*states)


def _assert_finite_state(a):
    assert all(np.isfinite(x).all() for x in a[0]) and np.isfinite(np.asarray(a[2], np.float32)).all()


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
    from mr_gan_amd import MRGAN
    D, n = 400, 4 * B
    case = Case(D=D, B=B, steps=1, device_z=True)
    rs = np.random.RandomState(3)
    X, xl = rs.randn(n, D).astype(np.float32), rs.randn(2 * B, D).astype(np.float32)
    yl = rs.randint(0, 6, size=2 * B).astype(np.int32)
    big = 1e3 * rs.randn(3 * 64 + 7, D).astype(np.float32)
    states = []
    for disturb in (False, True):
        m = MRGAN(D, batch_size=B, dtype='bfloat16', seed=77, use_graph=True, init_weights=False)
        P.load(m.engine, case)
        with m._on_stream():
            xu, xlab, bigd = m._dev(X), m._dev(xl), m._dev(big)
            idx_lab = m._dev(np.arange(n, dtype=np.int32) % (2 * B), torch.int32)
            labs = m._dev(yl[np.arange(n) % (2 * B)], torch.int32)
            idx_u1 = m._dev(np.arange(n, dtype=np.int32)[::-1].copy(), torch.int32)
            idx_u2 = m._dev(np.roll(np.arange(n, dtype=np.int32), 7), torch.int32)
            dargs = E.Engine.disc_args(xlab, labs, xu, None, idx_lab, idx_u1, stream_mode=1)
            gargs = E.Engine.gen_args(xu, None, idx_u2, stream_mode=1)
            m.engine.set_iterations(0, 0)
            for _ in range(n // B):
                if disturb:
                    m.engine.input_gradient(bigd, None, E.SAL_XENT, E.SAL_RAW)
                m.engine.train_pair(dargs, gargs)
            torch.cuda.synchronize()
            states.append(_state(m.engine))
        m.engine.close()
    assert states[0][1] == 2 * (n // B)
    _assert_same_state(*states)


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
    from mr_gan_amd import MRGAN, MRGANGroup
    D, seed = 40, 123
    X = np.random.default_rng(3).standard_normal((77, D)).astype(np.float32)
    grp = MRGANGroup(D, 3, batch_size=B, dtype=dtype, seed=seed)
    got = [grp.saliency(m, X) for m in (2, 0, 1)]
    grp.engine.close()
    for (maps, cls), m in zip(got, (2, 0, 1)):
        one = MRGAN(D, batch_size=B, dtype=dtype, seed=seed + m)
        want, wcls = one.saliency(X)
        one.engine.close()
        assert maps.shape == (77, D) and maps.dtype == np.float32 and maps.max() == 1.0
        assert np.array_equal(maps.view(np.uint32), want.view(np.uint32)) and np.array_equal(cls, wcls)
    assert not np.array_equal(got[0][0], got[1][0])


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
    eng = P.engine(64, 128, E.FP8)
    with pytest.raises(E.MrganError) as ei:
        eng.input_gradient(torch.zeros((4, 64), device=P.DEV))
    eng.close()
    msg = str(ei.value)
    assert "error -3" in msg and "fp32" in msg and "bf16" in msg


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
    """the scalar head and the finishing kernel; no matrix-core head, no chain launch, no weight gradient, no update"""
    D = 96
    kw = dict(d_hidden=d_hidden) if d_hidden else {}
    eng = P.engine(D, B, dtype, **kw)
    P.load(eng, Case(D=D, B=B, steps=1, **kw))
    x = P.to_dev(np.random.default_rng(3).standard_normal((130, D)).astype(np.float32))
    eng.profile_begin()
    eng.input_gradient(x, None, E.SAL_XENT, E.SAL_HEATMAP)
    prof = eng.profile_end()
    eng.close()
    print(sorted((k, v[1]) for k, v in prof.items()))
    assert prof["saliency_finish_kernel"][1] == 2 and prof["head_kernel"][1] == 2 and prof["stage_kernel"][1] == 2
    for name in prof:
        assert not any(s in name for s in ("head_wide", "chain_kernel", "adam", "_ks_", "w6_split", "reduce_partials", "fm_kernel")), name
        assert not name.startswith(("gemm_f32_kernel<2", "gemm_bf16_kc_kernel<2")), name
    assert sum(v[1] for k, v in prof.items() if k.startswith("gemm")) == 20
