"""mrgan_attribution on the GPU: SmoothGrad and integrated gradients accumulated over draws on the device, against the reference
arithmetic of tests/attribution_ref.py (fp64 for the fp32 engine, the bf16 mirror for the bf16 engine), its noise keys, and what
the call must leave alone.  Every handle has B = 50 (S = 128); 130 rows are two chunks of 128 + 2 rows, 3 draws."""
import ctypes as C

import numpy as np
import pytest
import torch

from mr_gan_amd import engine as E
from tests import attribution_ref as A
from tests import parity as P
from tests import saliency_gpu as G
from tests import saliency_ref as R
from tests.helpers import Case, cosine, frob_rel_err, rel_err

pytestmark = pytest.mark.gpu

B, N, DRAWS = A.B, A.N, A.DRAWS
FP32_TOL, SENT = G.FP32_TOL, G.SENT   # the saliency tests' bound; a mean over draws cannot exceed the worst draw's error
METHOD = {'noise': E.ATTR_NOISE, 'path': E.ATTR_PATH}
_engine, _bits = G.engine, G.bits


def _mode_kw(mode, D):
    method, (s_in, s_hid), baseline, multiply = A.MODES[mode]
    b = P.to_dev(A.random_baseline(D)) if baseline == 'random' else None
    return dict(method=METHOD[method], sigma_input=s_in, sigma_hidden=s_hid, baseline=b, multiply=multiply)


def _attr(eng, x, targets=None, objective='xent', post=E.SAL_RAW, draws=DRAWS, **kw):
    t = None if targets is None else P.to_dev(targets, torch.int32)
    out, cls = eng.attribution(x if isinstance(x, torch.Tensor) else P.to_dev(x), t, E.SAL_OBJECTIVES[objective], post, draws=draws, **kw)
    return out.cpu().numpy(), cls.cpu().numpy()


# ---- 1. the degenerate call ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [E.F32, E.BF16])
@pytest.mark.parametrize("post", [E.SAL_RAW, E.SAL_HEATMAP])
def test_one_noise_free_draw_gives_the_bits_of_input_gradient(dtype, post):
    K, D, dh = A.SHAPES[0]
    case, x32 = A.problem(K, D, dh)
    eng = _engine(case, D, dtype)
    rng = np.random.default_rng(11)
    idx = P.to_dev(np.concatenate([rng.permutation(N), rng.integers(0, N, 23)]).astype(np.int32), torch.int32)
    wide = G.wide_rows(x32)
    outs = []
    for call in (eng.input_gradient, eng.attribution):
        out, cls = G.sentinel_buffers(idx.numel(), D)
        call(wide, None, E.SAL_XENT, post, idx=idx, out=out, classes_out=cls)      # (attribution's defaults: NOISE, 1 draw, sigmas 0)
        outs.append((out.cpu().numpy(), cls.cpu().numpy()))
    eng.close()
    (want, wcls), (got, cls) = outs
    assert np.isfinite(want[:, :D]).all() and np.abs(want[:, :D]).max() > 0
    assert np.array_equal(_bits(got), _bits(want)) and (got[:, D:] == SENT).all()
    assert np.array_equal(cls, wcls) and cls.min() >= 0


# ---- 2. fp32 against fp64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,D,dh", A.SHAPES)
@pytest.mark.parametrize("mode", list(A.MODES))
def test_fp32_attribution_matches_fp64(K, D, dh, mode):
    case, x32 = A.problem(K, D, dh)
    eng = _engine(case, D, E.F32)
    xd = P.to_dev(x32)
    kw = _mode_kw(mode, D)
    errs = {}
    for objective in (R.OBJECTIVES if (K, D, dh) == A.SHAPES[0] else ('xent',)):
        for planted in (False, True) if objective == 'xent' else (False,):
            want, t, decided = A.reference(K, D, dh, mode, objective, planted)
            assert N - decided.sum() <= 0.25 * N
            got, cls = _attr(eng, xd, t, objective, **kw)
            assert got.shape == (N, D) and np.isfinite(got).all() and np.array_equal(cls, t)
            errs[(objective, planted)] = rel_err(got[decided], want[decided])
    # targets NULL: the classes of the clean call, used for every draw
    clean_cls = eng.input_gradient(xd)[1].cpu().numpy()
    got0, cls0 = _attr(eng, xd, None, 'xent', **kw)
    got1, cls1 = _attr(eng, xd, clean_cls, 'xent', **kw)
    eng.close()
    print("(%d, %d)%s %s: undecided %d, rel_err %s" % (K, D, " wide head" if dh else "", mode, N - decided.sum(), errs))
    for key, e in errs.items():
        assert e < FP32_TOL, (key, e)
    assert np.array_equal(cls0, clean_cls) and np.array_equal(cls1, clean_cls)
    assert np.array_equal(_bits(got0), _bits(got1))
    want, t, decided = A.reference(K, D, dh, mode, 'xent', False)
    same = decided & (t == clean_cls)
    assert same.sum() >= 0.7 * N and rel_err(got0[same], want[same]) < FP32_TOL


# ---- 3. a true-Gaussian handle -------------------------------------------------------------------------------------
def test_gaussian_handle_draws_its_sites_from_the_gaussian_generator():
    K, D, dh = A.SHAPES[0]
    case, x32 = A.problem(K, D, dh)
    xd = P.to_dev(x32)
    t = A.reference(K, D, dh, 'own')[1]
    eng = _engine(case, D, E.F32, flags=E.FLAG_GAUSS_NOISE)
    got, _ = _attr(eng, xd, t, **_mode_kw('own', D))

    def own_draws(site, d, cols):      # (pinned to the restated generator by the true-Gaussian tests)
        return eng.debug_noise(site, E.ATTR_NOISE_SEG, d, N, cols, 0).cpu().numpy().astype(np.float64)
    want, _, margin = A.attribution(case.d0, x32, t, 'xent', 'noise', DRAWS, A.OWN, noise_fn=own_draws)
    eng.close()
    eng = _engine(case, D, E.F32)
    default, _ = _attr(eng, xd, t, **_mode_kw('own', D))
    eng.close()
    decided = margin >= A.DECIDED
    e = rel_err(got[decided], want[decided])
    print("true-Gaussian handle: undecided %d, rel_err %.2e, against the default handle %.2e" % (N - decided.sum(), e, rel_err(got, default)))
    assert N - decided.sum() <= 0.25 * N
    assert e < FP32_TOL, e
    assert rel_err(got, default) > 1e-2


# ---- 4. bf16 against the bf16 mirror -------------------------------------------------------------------------------
@pytest.mark.parametrize("K,D,dh", A.BF16_SHAPES)
@pytest.mark.parametrize("mode", ['own', 'path0'])
def test_bf16_attribution_matches_the_mirror(K, D, dh, mode):
    """the project's rule for bf16 gradients, Frobenius over the whole matrix: err(engine, mirror) < max(3e-3, 0.6 err(mirror, fp64)).
    Measured: see DESIGN.md 4, "Saliency"."""
    case, x32 = A.problem(K, D, dh)
    want_o, t, _ = A.reference(K, D, dh, mode)
    want_m, _, _ = A.reference(K, D, dh, mode, quantize='bf16')
    eng = _engine(case, D, E.BF16)
    got, cls = _attr(eng, x32, t, **_mode_kw(mode, D))
    eng.close()
    em, eo, emo = frob_rel_err(got, want_m), frob_rel_err(got, want_o), frob_rel_err(want_m, want_o)
    print("bf16 attribution (%d, %d)%s %s: engine-mirror %.2e engine-fp64 %.2e mirror-fp64 %.2e cosine %.5f"
          % (K, D, " wide head" if dh else "", mode, em, eo, emo, cosine(got, want_o)))
    assert np.array_equal(cls, t) and np.isfinite(got).all()
    assert em < max(3e-3, 0.6 * emo), (em, emo)


# ---- 5. multiply ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [E.F32, E.BF16])
def test_multiply_is_the_mean_gradient_times_the_input_difference(dtype):
    K, D, dh = A.SHAPES[0]
    case, x32 = A.problem(K, D, dh)
    eng = _engine(case, D, dtype)
    xd = P.to_dev(x32)
    b = A.random_baseline(D)
    for kw, base in ((dict(method=E.ATTR_NOISE, sigma_input=0.3, sigma_hidden=0.5), None), (dict(method=E.ATTR_PATH), None),
                     (dict(method=E.ATTR_PATH, baseline=P.to_dev(b)), b)):
        plain, cls = _attr(eng, xd, multiply=0, **kw)
        times, cls2 = _attr(eng, xd, multiply=1, **kw)
        want = plain * (x32 - (np.float32(0) if base is None else base)).astype(np.float32)
        assert want.dtype == np.float32 and np.array_equal(cls, cls2) and np.abs(want).max() > 0
        assert (np.abs(times - want) <= 3 * 2.0 ** -24 * np.abs(want)).all(), kw
    eng.close()


# ---- 6. heat-map ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [E.F32, E.BF16])
@pytest.mark.parametrize("mode", ['own', 'pathb'])
def test_heatmap_is_the_reference_map_of_the_raw_result(dtype, mode):
    K, D, dh = A.SHAPES[0]
    case, x32 = A.problem(K, D, dh)
    eng = _engine(case, D, dtype)
    xd = P.to_dev(x32)
    raw, cls = _attr(eng, xd, **_mode_kw(mode, D))
    hm, cls2 = _attr(eng, xd, post=E.SAL_HEATMAP, **_mode_kw(mode, D))
    eng.close()
    want = R.heatmap(raw)
    print("heat-map %s: max abs difference %.2e" % (mode, np.abs(hm - want).max()))
    assert np.array_equal(cls, cls2)
    assert hm.min() >= 0.0 and hm.max() <= 1.0
    assert np.abs(hm - want).max() < 1e-5
    assert (hm.max(axis=1) == 1.0).all() and (hm.min(axis=1) == 0.0).all()


@pytest.mark.parametrize("dtype", [E.F32, E.BF16])
def test_heatmap_of_an_all_dead_row_is_zero(dtype):
    K, D, _ = A.SHAPES[0]
    eng, x = G.dead_row_engine(dtype, K, D, N)
    # hidden noise only (the input stays zero) and the path from zero (every point of it is zero)
    for kw in (dict(method=E.ATTR_NOISE, sigma_hidden=0.5), dict(method=E.ATTR_PATH, multiply=1)):
        raw, _ = _attr(eng, x, **kw)
        hm, _ = _attr(eng, x, post=E.SAL_HEATMAP, **kw)
        assert not raw[2].any() and np.abs(raw[[0, 1, 3, 4]]).max(axis=1).min() > 0
        assert np.isfinite(hm).all() and not hm[2].any() and (hm[[0, 1, 3, 4]].max(axis=1) == 1.0).all()
    eng.close()


# ---- 7. keys -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [E.F32, E.BF16])
def test_maps_do_not_depend_on_the_iteration_or_on_training(dtype):
    K, D, dh = A.SHAPES[0]
    case = Case(D=D, B=B, steps=3, device_z=True)
    _, x32 = A.problem(K, D, dh)
    eng = P.engine(D, B, dtype)
    P.load(eng, case)
    xd = P.to_dev(x32)
    kw = _mode_kw('own', D)
    first, cls = _attr(eng, xd, **kw)
    again, _ = _attr(eng, xd, **kw)
    assert np.array_equal(_bits(first), _bits(again))
    eng.set_iterations(7, 3)
    moved, _ = _attr(eng, xd, **kw)
    assert np.array_equal(_bits(first), _bits(moved))
    for t in range(case.steps):
        eng.train_pair(P.disc_args(case, t, True), P.gen_args(case, t, True))
    trained, _ = _attr(eng, xd, **kw)
    P.load(eng, case)
    restored, cls2 = _attr(eng, xd, **kw)
    its = eng.get_iterations()
    eng.close()
    assert its == 7 + 2 * case.steps
    assert not np.array_equal(trained, first)
    assert np.array_equal(_bits(first), _bits(restored)) and np.array_equal(cls, cls2)
    # the draws differ from each other and from the noise-free gradient
    assert rel_err(first, _one_draw(case, D, dtype, xd, kw)) > 1e-2


def _one_draw(case, D, dtype, xd, kw):
    eng = P.engine(D, B, dtype)
    P.load(eng, case)
    out, _ = _attr(eng, xd, draws=1, **kw)
    eng.close()
    return out


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_group_handle_serves_the_selected_model(dtype):
    G.group_handle_serves_the_selected_model(dtype, N, method='smoothgrad', draws=DRAWS, heatmap=False)


# ---- 8. training is undisturbed ------------------------------------------------------------------------------------
def _disturb(eng, big, t):
    """one NOISE call and one PATH call of 199 large rows: two chunks, every padding row of segment 0"""
    out, _ = eng.attribution(big, None, E.SAL_XENT, E.SAL_HEATMAP if t == 1 else E.SAL_RAW, method=E.ATTR_NOISE, draws=2,
                             sigma_input=0.3, sigma_hidden=0.5)
    assert bool(torch.isfinite(out).all())
    out, _ = eng.attribution(big, None, E.SAL_XENT, E.SAL_RAW, method=E.ATTR_PATH, draws=2, multiply=1)
    assert bool(torch.isfinite(out).all())


def test_training_is_undisturbed_by_attribution_calls():
    G.training_is_undisturbed_by(_disturb)


def test_graph_replay_is_undisturbed_by_attribution_calls():
    G.graph_replay_is_undisturbed_by(_disturb)


# ---- 9. refusals ---------------------------------------------------------------------------------------------------
def test_fp8_handle_is_refused():
    G.fp8_handle_is_refused(lambda eng, x: eng.attribution(x, draws=2, sigma_input=0.3))


def test_bad_arguments_are_refused():
    D = 16
    eng = P.engine(D, B, E.F32)
    x = torch.zeros((8, D), device=P.DEV)
    out = torch.zeros((8, D), device=P.DEV)
    cls = torch.zeros((8,), dtype=torch.int32, device=P.DEV)
    base = torch.zeros((D,), device=P.DEV)
    good = dict(x=x.data_ptr(), ld_x=D, n=8, objective=E.SAL_XENT, post=E.SAL_RAW, out=out.data_ptr(), ld_out=D, classes_out=cls.data_ptr(),
                method=E.ATTR_NOISE, draws=2, sigma_input=0.3, sigma_hidden=0.5)

    def call(**kw):
        a = E.AttributionArgs()
        for k, v in dict(good, **kw).items():
            setattr(a, k, v)
        return eng.lib.mrgan_attribution(eng.handle, C.byref(a), E._stream())
    assert call() == 0
    assert call(method=E.ATTR_PATH, sigma_input=0.0, sigma_hidden=0.0, baseline=base.data_ptr(), multiply=1) == 0
    assert call(classes_out=None, targets=cls.data_ptr()) == 0
    path = dict(method=E.ATTR_PATH, sigma_input=0.0, sigma_hidden=0.0)
    for bad, field in ((dict(x=None), b"x"), (dict(out=None), b"out"), (dict(ld_x=D - 1), b"ld_x"), (dict(ld_out=D - 1), b"ld_out"),
                       (dict(objective=3), b"objective"), (dict(objective=-1), b"objective"), (dict(post=2), b"post"), (dict(n=-1), b"n"),
                       (dict(method=2), b"method"), (dict(method=-1), b"method"), (dict(draws=0), b"draws"), (dict(draws=-3), b"draws"),
                       (dict(draws=E.ATTR_MAX_DRAWS + 1), b"draws"), (dict(multiply=2), b"multiply"),
                       (dict(sigma_input=-0.1), b"sigma_input"), (dict(sigma_input=float("nan")), b"sigma_input"),
                       (dict(sigma_hidden=float("inf")), b"sigma_hidden"), (dict(sigma_hidden=-1.0), b"sigma_hidden"),
                       (dict(path, sigma_input=0.3), b"sigma"), (dict(path, sigma_hidden=0.5), b"sigma"),
                       (dict(baseline=base.data_ptr()), b"baseline"), (dict(classes_out=None), b"classes_out")):
        assert call(**bad) == -2, bad
        msg = eng.lib.mrgan_last_error()
        assert b"attribution" in msg and field in msg, (bad, msg)
    assert eng.lib.mrgan_attribution(eng.handle, None, E._stream()) == -2
    assert call(n=0) == 0 and call(draws=E.ATTR_MAX_DRAWS, n=0) == 0
    eng.close()


# ---- 10. kernel names ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,dh", [(E.F32, None), (E.BF16, None), (E.BF16, A.WIDE_HEAD)])
def test_kernels_of_one_call(dtype, dh):
    """a 3-draw call of one chunk: per draw one stage, five forward and five dX products, the scalar head and the accumulate
    launch, plus one clean forward and head when the targets are not given; nothing of a training step"""
    eng, x = G.profiled_engine(dtype, dh, 100)
    profs = []
    for call in (dict(method=E.ATTR_NOISE, sigma_input=0.3, sigma_hidden=0.5), dict(method=E.ATTR_PATH, multiply=1),
                 dict(method=E.ATTR_NOISE, targets=torch.zeros(100, dtype=torch.int32, device=P.DEV))):
        eng.profile_begin()
        eng.attribution(x, call.pop('targets', None), E.SAL_XENT, E.SAL_HEATMAP, draws=3, **call)
        profs.append(eng.profile_end())
    eng.close()

    def count(prof, name):
        return prof[name][1] if name in prof else 0
    for prof, (stage, pstage, head, gemms) in zip(profs, ((4, 0, 4, 35), (1, 3, 4, 35), (3, 0, 3, 30))):
        print(sorted((k, v[1]) for k, v in prof.items()))
        assert count(prof, "stage_kernel") == stage and count(prof, "path_stage_kernel") == pstage and count(prof, "head_kernel") == head
        assert count(prof, "attribution_accum_kernel") == 3
        G.assert_no_training_kernels(prof, gemms)


# ---- 11. the front ends --------------------------------------------------------------------------------------------
def test_mrgan_saliency_keywords():
    from mr_gan_amd import MRGAN
    D, n = 24, 77
    X = np.random.default_rng(4).standard_normal((n, D)).astype(np.float32)
    m = MRGAN(D, batch_size=B, seed=5)
    plain, cls = m.saliency(X)
    sg, cls_sg = m.saliency(X, method='smoothgrad')
    sg2, _ = m.saliency(X, method='smoothgrad', draws=16, sigma=(0.3, 0.5))
    sg_in, _ = m.saliency(X, method='smoothgrad', draws=4, sigma=0.2, heatmap=False)
    ig, cls_ig = m.saliency(X, method='integrated', objective='logit', heatmap=False)
    ig_b, _ = m.saliency(X, method='integrated', objective='logit', heatmap=False, baseline=np.full(D, 0.25, np.float32), draws=8)
    gxi, _ = m.saliency(X, times_input=True, heatmap=False)
    raw, _ = m.saliency(X, heatmap=False)
    logits = m.predict_logits(X)
    l0 = m.predict_logits(np.zeros((1, D), np.float32))[0]
    with pytest.raises(ValueError):
        m.saliency(X, method='integrated', sigma=0.1)
    with pytest.raises(ValueError):
        m.saliency(X, method='integrated', baseline=np.zeros(D + 1))
    m.engine.close()
    for maps in (plain, sg, sg2, sg_in, ig, ig_b, gxi):
        assert maps.shape == (n, D) and maps.dtype == np.float32 and np.isfinite(maps).all()
    assert sg.min() >= 0.0 and sg.max() == 1.0 and np.array_equal(cls_sg, cls) and np.array_equal(cls_ig, cls)
    assert np.array_equal(_bits(sg), _bits(sg2)) and not np.array_equal(sg, plain)      # the defaults are 16 draws at the network's sigmas
    assert (np.abs(gxi - raw * X) <= 3 * 2.0 ** -24 * np.abs(raw * X)).all()
    # integrated gradients sum to the change of the class score (16 midpoints: loosely)
    want = logits[np.arange(n), cls] - l0[cls]
    assert np.abs(ig.sum(axis=1) - want).max() < 0.1 * np.abs(want).max()
    assert not np.array_equal(ig, ig_b)


def test_mrnn_saliency_smoothgrad():
    from mr_gan_amd.mr_nn import MRNN
    D, K, n = 24, 10, 100
    rng = np.random.default_rng(4)
    y = (np.arange(n) % K).astype(np.int32)
    X = (rng.standard_normal((n, D)) + 2.0 * np.eye(K, D)[y]).astype(np.float32)
    nn = MRNN(D, batch_size=20, num_classes=K, seed=5)
    nn.fit(X, y, epochs=1)
    maps, cls = nn.saliency(X[:33], method='smoothgrad', draws=4)
    again, cls2 = nn.saliency(X[:33], method='smoothgrad', draws=4)
    raw, cls3 = nn.saliency(X[:33], y=y[:33], objective='logit', heatmap=False, method='integrated', draws=4)
    pred = np.argmax(nn.predict_logits(X[:33]), axis=1)
    nn.engine.close()
    assert maps.shape == (33, D) and cls.shape == (33,) and maps.dtype == np.float32 and cls.dtype == np.int32
    assert np.isfinite(maps).all() and maps.min() >= 0.0 and maps.max() <= 1.0
    assert np.array_equal(cls, pred) and np.array_equal(_bits(maps), _bits(again)) and np.array_equal(cls, cls2)
    assert raw.shape == (33, D) and np.isfinite(raw).all() and np.array_equal(cls3, y[:33])
