"""Model groups, the GAN hot loop: one D sub-step and one G sub-step of G equal-shape trainings as one launch set each
(mrgan_disc_step_group / mrgan_gen_step_group / mrgan_train_pair_group).

Built like tests/test_model_groups_gpu.py: the reference of a group is G single handles -- model m against a handle created
with seed + m and loaded with model m's weights -- and the bound is bit identity (assert_array_equal, no tolerance).
Problems come from tests.helpers.Case (one per model, seeds 7 + m), handles from tests.parity.engine.  Where a single handle
would take the matrix-core head kernel (the 32-class pitch) the reference handle runs with MRGAN_TUNE_HEAD_MFMA = 0: a group
takes the scalar head kernel there."""
import functools

import numpy as np
import pytest
import torch

from tests import parity as P
from tests.helpers import SEED, Case, planted as _planted

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
GAUSS = 16                                     # MRGAN_FLAG_GAUSS_NOISE
_t = P.to_dev


def _engine(D, B, dtype, models=0, seed=SEED, flags=0, K=None, chain=None, head_mfma=None):
    from mr_gan_amd import engine as E
    kw = {} if K is None else dict(num_classes=K)
    eng = P.engine(D, B, dtype, flags=flags, models=models, seed=seed, **kw)
    if chain is not None:
        eng.set_tuning(E.TUNE_CHAIN, chain)
    if head_mfma is not None:
        eng.set_tuning(E.TUNE_HEAD_MFMA, head_mfma)
    return eng


@functools.lru_cache(maxsize=None)
def _cases(G, D, B, K=None, steps=3):
    """one problem per model; shared, never modified"""
    return tuple(Case(D=D, B=B, steps=steps, seed=7 + m, K=K) for m in range(G))


def _state(eng, xin0=True):
    """everything a GAN sub-step leaves behind, for the selected model of a group or for a single handle: 8 G + 12 D weights,
    both Adam slots of both nets, the stored xin / dpre buffers, the four device metrics (sums and last values)"""
    from mr_gan_amd import engine as E
    out = eng.get_weights(E.NET_G) + eng.get_weights(E.NET_D)
    for which in (0, 1):
        out += eng.get_slot(E.NET_G, which) + eng.get_slot(E.NET_D, which)
    out += [eng.debug_buffer(0, l).cpu().numpy() for l in range(0 if xin0 else 1, 5)]
    out += [eng.debug_buffer(1, l).cpu().numpy() for l in range(5)]
    out.append(np.array(eng.read_metrics(reset=False), np.float32))
    return out


def _load_group(eng, cases):
    for m, case in enumerate(cases):
        eng.select_model(m)
        P.load(eng, case)
    eng.select_model(0)


def _unl(case, t, nan):
    """(x_unl of the D sub-step, x_unl of the G sub-step) of pair t; nan: the rows are NaN"""
    if nan:
        return np.full_like(case.x_unl[t], np.nan), np.full_like(case.x_unl2[t], np.nan)
    return case.x_unl[t], case.x_unl2[t]


@functools.lru_cache(maxsize=None)
def _singles(dtype, G, D, B, K=None, flags=0, chain=None, device_z=False):
    """G single handles, model m with seed + m: -> [(outputs per sub-step, state, iterations)]"""
    from mr_gan_amd import engine as E
    res = []
    for m, case in enumerate(_cases(G, D, B, K)):
        eng = _engine(D, B, dtype, seed=SEED + m, flags=flags, K=K, chain=chain, head_mfma=0 if K else None)
        P.load(eng, case)
        outs = []
        for t in range(case.steps):
            outs.append(eng.disc_step(P.disc_args(case, t, device_z)) + (eng.gen_step(P.gen_args(case, t, device_z)),))
        res.append((outs, _state(eng), eng.get_iterations()))
        eng.close()
    return res


def _run_group(dtype, G, D, B, K=None, flags=0, chain=None, device_z=False, nan_model=-1):
    """the same sub-steps on one group handle -> [(outputs per sub-step, state, iterations)] per model"""
    from mr_gan_amd import engine as E
    cases = _cases(G, D, B, K)
    eng = _engine(D, B, dtype, models=G, flags=flags, K=K, chain=chain)
    _load_group(eng, cases)
    outs = []
    for t in range(cases[0].steps):
        unl = [_unl(c, t, m == nan_model) for m, c in enumerate(cases)]
        z1 = None if device_z else _t(np.stack([c.z1[t] for c in cases]))
        z2 = None if device_z else _t(np.stack([c.z2[t] for c in cases]))
        da = E.Engine.disc_group_args(_t(np.stack([c.x_lab[t] for c in cases])), _t(np.stack([c.labels[t] for c in cases]), torch.int32),
                                      _t(np.stack([u[0] for u in unl])), z1)
        ga = E.Engine.gen_group_args(_t(np.stack([u[1] for u in unl])), z2)
        assert da.x_lab_model_stride == B * D and da.labels_model_stride == B and da.x_unl_model_stride == B * D
        assert da.z_model_stride == ga.z_model_stride == (0 if device_z else B * 100) and ga.x_unl_model_stride == B * D
        d = eng.disc_step_group(da)
        g = eng.gen_step_group(ga)
        outs.append([d[m] + (g[m],) for m in range(G)])
    it = eng.get_iterations()
    res = []
    for m in range(G):
        eng.select_model(m)
        res.append(([o[m] for o in outs], _state(eng), it))
    eng.close()
    return res


@functools.lru_cache(maxsize=None)
def _group(*args, **kw):
    return _run_group(*args, **kw)


def _assert_same(got, want, what, models=None, ntensors=71):
    for m, ((o_g, s_g, it_g), (o_w, s_w, it_w)) in enumerate(zip(got, want)):
        if models is not None and m not in models:
            continue
        assert it_g == it_w, (what, m, it_g, it_w)
        np.testing.assert_array_equal(np.array(o_g, np.float32), np.array(o_w, np.float32), err_msg="%s: outputs of model %d" % (what, m))
        assert len(s_g) == len(s_w) == ntensors
        for i, (a, b) in enumerate(zip(s_g, s_w)):
            np.testing.assert_array_equal(a, b, err_msg="%s: model %d, tensor %d (8 G + 12 D weights | their m | their v | xin | 5 dpre | "
                                                        "metrics)" % (what, m, i))


# ---------------------------------------------------------------------------------------------------------
# 1. bit identity with single handles
# ---------------------------------------------------------------------------------------------------------
# (dtype, G, D, B, classes, flags, MRGAN_TUNE_CHAIN, z drawn on the device): the smallest shapes at which each per-model offset
# can be wrong without the others hiding it
STEP_CASES = [
    (F32, 3, 48, 20, None, 0, None, False),      # per-layer tail, scalar head
    (BF16, 3, 72, 50, None, 0, 0, False),        # bf16 without chains: ragged, one 64-row tile
    (BF16, 3, 72, 50, None, 0, None, True),      # default tuning: the three chains; z drawn on the device with seed + m
    (BF16, 2, 200, 130, None, 0, None, False),   # three 64-row blocks (the last with two rows) in the D-tail chain, 32-row blocks with a
                                                 # ragged last one in the G chains, several column-sum partial rows, column tiles in D1
    (F32, 2, 48, 20, 10, 0, None, False),        # class pitch 32: the scalar head on both sides
    (BF16, 2, 48, 20, 10, 0, None, False),
    (BF16, 2, 72, 50, None, GAUSS, None, False),
]


@pytest.mark.parametrize("dtype,G,D,B,K,flags,chain,device_z", STEP_CASES)
def test_group_gan_steps_equal_single_handles(dtype, G, D, B, K, flags, chain, device_z):
    """three (D, G) pairs: all 20 weights, both Adam slots of both nets, the iteration count, the 3 + 1 outputs of every pair,
    the four device metrics and the stored xin / dpre buffers of every model equal those of the single handle with seed + m"""
    got = _group(dtype, G, D, B, K, flags, chain, device_z)
    want = _singles(dtype, G, D, B, K, flags, chain, device_z)
    assert got[0][2] == 6
    _assert_same(got, want, "group vs singles")
    # the models differ from each other: a group that trained model 0 G times would pass the comparison of model 0 only
    assert not np.array_equal(got[0][1][0], got[1][1][0]) and not np.array_equal(got[0][1][8], got[1][1][8])
    assert got[0][0][0] != got[1][0][0]


def _pair_problem(G, D, B, nb, seed=11):
    rng = np.random.default_rng(seed)
    n = 400
    X = rng.standard_normal((n, D)).astype(np.float32)
    XL = rng.standard_normal((120, D)).astype(np.float32)
    YL = rng.integers(0, 6, 120).astype(np.int32)
    idx_lab = rng.integers(0, 120, (G, nb * B)).astype(np.int32)       # (nb * B entries per model: every batch of the stream)
    assert nb * B <= n
    idx_u1 = np.stack([rng.permutation(n)[:nb * B] for _ in range(G)]).astype(np.int32)
    idx_u2 = np.stack([rng.permutation(n)[:nb * B] for _ in range(G)]).astype(np.int32)
    return X, XL, YL[idx_lab], idx_lab, idx_u1, idx_u2


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_group_train_pair_equals_single_train_pairs(dtype):
    """G = 3, stream mode over four batches, graph replay on both sides, x_unl_model_stride = 0: all models gather from one
    matrix through their own index vectors; against the single handles' train_pair at default tuning (whose two generator
    forwards run as one paired pass: the G sub-step's rows then live in slots 3 .. 4 of xin[0], the one buffer left out here)"""
    from mr_gan_amd import engine as E
    G, D, B, nb = 3, 72, 50, 4
    cases = _cases(G, D, B)
    X, XL, lab, idx_lab, idx_u1, idx_u2 = _pair_problem(G, D, B, nb)
    stream = torch.cuda.Stream(P.DEV)
    with torch.cuda.stream(stream):
        xd, xl = _t(X), _t(XL)
        want = []
        for m in range(G):
            eng = _engine(D, B, dtype, seed=SEED + m, flags=E.FLAG_GRAPH)
            P.load(eng, cases[m])
            da = E.Engine.disc_args(xl, _t(lab[m], torch.int32), xd, None, _t(idx_lab[m], torch.int32), _t(idx_u1[m], torch.int32), stream_mode=1)
            ga = E.Engine.gen_args(xd, None, _t(idx_u2[m], torch.int32), stream_mode=1)
            for _ in range(nb):
                eng.train_pair(da, ga)
            want.append(([], _state(eng, xin0=False), eng.get_iterations()))
            eng.close()
        eng = _engine(D, B, dtype, models=G, flags=E.FLAG_GRAPH)
        _load_group(eng, cases)
        da = E.Engine.disc_group_args(xl, _t(lab, torch.int32), xd, None, _t(idx_lab, torch.int32), _t(idx_u1, torch.int32), stream_mode=1)
        ga = E.Engine.gen_group_args(xd, None, _t(idx_u2, torch.int32), stream_mode=1)
        assert da.x_unl_model_stride == 0 and da.x_lab_model_stride == 0 and ga.x_unl_model_stride == 0
        assert da.idx_unl_model_stride == da.idx_lab_model_stride == da.labels_model_stride == ga.idx_unl_model_stride == nb * B
        for _ in range(nb):
            eng.train_pair_group(da, ga)
        got = []
        for m in range(G):
            eng.select_model(m)
            got.append(([], _state(eng, xin0=False), eng.get_iterations()))
        eng.close()
    assert got[0][2] == 2 * nb
    _assert_same(got, want, "train_pair_group", ntensors=70)
    assert not np.array_equal(got[0][1][0], got[1][1][0])


# ---------------------------------------------------------------------------------------------------------
# 2. isolation
# ---------------------------------------------------------------------------------------------------------
def test_a_model_with_nan_inputs_leaves_the_others_alone():
    """model 1's unlabelled rows are NaN: models 0 and 2 are bit-identical to the clean run (BatchNorm statistics,
    feature-matching moments, the loss scalars or a chain block reading a neighbour's copy would show here)"""
    G, D, B = 3, 72, 50
    clean = _group(BF16, G, D, B, None, 0, None, True)
    dirty = _run_group(BF16, G, D, B, None, 0, None, True, nan_model=1)
    _assert_same(dirty, clean, "NaN rows in model 1", models=(0, 2))
    assert np.isnan(dirty[1][1][8]).any(), "model 1 trained on NaN rows"
    for w in dirty[0][1][:20] + dirty[2][1][:20]:
        assert np.isfinite(w).all()


# ---------------------------------------------------------------------------------------------------------
# 3. one launch set
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_a_grouped_gan_pair_is_one_launch_set(dtype):
    """G = 4: the kernel names and the launch count per name of one grouped pair are those of one single handle's pair (with
    MRGAN_TUNE_PAIR_GEN = 0: a group runs its two generator forwards separately)"""
    from mr_gan_amd import engine as E
    G, D, B = 4, 72, 50
    cases = _cases(G, D, B)
    one = _engine(D, B, dtype)
    one.set_tuning(E.TUNE_PAIR_GEN, 0)
    P.load(one, cases[0])
    one.profile_begin()
    one.train_pair(P.disc_args(cases[0], 0, True), P.gen_args(cases[0], 0, True))
    single = {k: v[1] for k, v in one.profile_end().items()}
    one.close()
    grp = _engine(D, B, dtype, models=G)
    _load_group(grp, cases)
    da = E.Engine.disc_group_args(_t(np.stack([c.x_lab[0] for c in cases])), _t(np.stack([c.labels[0] for c in cases]), torch.int32),
                                  _t(np.stack([c.x_unl[0] for c in cases])))
    ga = E.Engine.gen_group_args(_t(np.stack([c.x_unl2[0] for c in cases])))
    grp.profile_begin()
    grp.train_pair_group(da, ga)
    grouped = {k: v[1] for k, v in grp.profile_end().items()}
    grp.close()
    assert grouped == single, (grouped, single)
    assert "stage_kernel" in single and "adam_kernel" in single and "bn_apply_kernel" in single and "bn_bwd_kernel" in single
    if dtype == BF16:
        assert {"chain_kernel<0>", "chain_kernel<1>", "chain_kernel<2>"} <= set(single) and sum(single.values()) >= 20
    else:
        assert "fm_kernel" in single and "head_kernel" in single


# ---------------------------------------------------------------------------------------------------------
# 4. reproducibility
# ---------------------------------------------------------------------------------------------------------
def test_grouped_substeps_are_bit_reproducible():
    """two runs from the same state give equal bits: the race detector of the chains with grid.y = models"""
    _assert_same(_run_group(BF16, 3, 72, 50, None, 0, None, True), _group(BF16, 3, 72, 50, None, 0, None, True), "second fresh group handle")


# ---------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------
def test_refusals():
    from mr_gan_amd import engine as E
    D, B = 48, 20
    cases = _cases(2, D, B)
    xs, ys = _t(np.stack([c.x_lab[0] for c in cases])), _t(np.stack([c.labels[0] for c in cases]), torch.int32)
    da, ga = E.Engine.disc_group_args(xs, ys, xs), E.Engine.gen_group_args(xs)
    one = _engine(D, B, BF16)
    for call in (lambda: one.disc_step_group(da), lambda: one.gen_step_group(ga), lambda: one.train_pair_group(da, ga)):
        with pytest.raises(E.MrganError, match=r"error -3: .*not a group handle"):
            call()
    assert one.get_iterations() == 0
    one.close()
    grp = _engine(D, B, BF16, models=2)
    _load_group(grp, cases)
    x, y = xs[0], ys[0]
    sa, sg = E.Engine.disc_args(x, y, x), E.Engine.gen_args(x)
    for call in (lambda: grp.disc_step(sa), lambda: grp.gen_step(sg), lambda: grp.train_pair(sa, sg)):
        with pytest.raises(E.MrganError, match=r"error -3: .*group.*_group entries"):
            call()
    for field in ("x_lab_model_stride", "idx_lab_model_stride", "labels_model_stride", "x_unl_model_stride", "idx_unl_model_stride",
                  "z_model_stride"):
        bad = E.Engine.disc_group_args(xs, ys, xs)
        setattr(bad, field, -1)
        for call in (lambda: grp.disc_step_group(bad), lambda: grp.train_pair_group(bad, ga)):
            with pytest.raises(E.MrganError, match=r"error -2: .*negative model stride"):
                call()
    for field in ("x_unl_model_stride", "idx_unl_model_stride", "z_model_stride"):
        bad = E.Engine.gen_group_args(xs)
        setattr(bad, field, -1)
        for call in (lambda: grp.gen_step_group(bad), lambda: grp.train_pair_group(da, bad)):
            with pytest.raises(E.MrganError, match=r"error -2: .*negative model stride"):
                call()
    bad = E.Engine.disc_group_args(xs, ys, xs)
    bad.ld_x_unl = D - 1
    with pytest.raises(E.MrganError, match=r"error -2: .*row pitch"):
        grp.disc_step_group(bad)
    bad = E.Engine.gen_group_args(xs)
    bad.ld_x_unl = D - 1
    with pytest.raises(E.MrganError, match=r"error -2: .*row pitch"):
        grp.gen_step_group(bad)
    assert grp.get_iterations() == 0
    grp.close()


# ---------------------------------------------------------------------------------------------------------
# 6. host level
# ---------------------------------------------------------------------------------------------------------
def test_mrgan_group_fit_equals_single_fits():
    """MRGANGroup.fit for 2 epochs, G 3, D 40, B 32, n 128 against three MRGAN(seed + m).fit runs with the same rngs: weights,
    history and evaluate"""
    from mr_gan_amd import MRGAN, MRGANGroup, engine as E
    G, D, B, n = 3, 40, 32, 128
    sets = [_planted(n, D, 20 + m) for m in range(G)]
    labs = [(x[:48], y[:48]) for x, y in sets]
    tests = [_planted(96, D, 40 + m) for m in range(G)]
    grp = MRGANGroup(D, G, batch_size=B, dtype='bfloat16', seed=11)
    hist = grp.fit([l[0] for l in labs], [l[1] for l in labs], [s[0] for s in sets], epochs=2, validation_data=tests,
                   rngs=[np.random.RandomState(100 + m) for m in range(G)])
    errs = grp.evaluate([t[0] for t in tests], [t[1] for t in tests])
    assert grp.engine.get_iterations() == 2 * 2 * (n // B) and len(hist) == 2
    for m in range(G):
        one = MRGAN(D, batch_size=B, dtype='bfloat16', seed=11 + m)
        h1 = one.fit(labs[m][0], labs[m][1], sets[m][0], epochs=2, validation_data=tests[m], rng=np.random.RandomState(100 + m))
        grp.engine.select_model(m)
        for net in (E.NET_G, E.NET_D):
            for a, b in zip(grp.engine.get_weights(net), one.engine.get_weights(net)):
                np.testing.assert_array_equal(a, b)
        for ep in range(2):
            for k in ('loss_lab', 'loss_unl', 'train_err', 'loss_gen', 'test_err'):
                assert hist[ep][k][m] == h1[ep][k], (m, ep, k, hist[ep][k][m], h1[ep][k])
        assert errs[m] == one.evaluate(tests[m][0], tests[m][1])
        np.testing.assert_array_equal(grp.predict_logits(m, tests[m][0]), one.predict_logits(tests[m][0]))
        one.engine.close()
    with pytest.raises(ValueError, match="equal length"):
        grp.fit([l[0] for l in labs], [l[1] for l in labs], [sets[0][0], sets[1][0], sets[2][0][:100]], epochs=1)
    grp.engine.close()
    with pytest.raises((ValueError, KeyError)):
        MRGANGroup(D, G, batch_size=B, dtype='fp8')


def test_mr_gan_folds_equals_six_hand_built_trainings():
    """N = 360, D = 40, six folds, one epoch of six batches; 25 labelled rows per class.  Fold f: mr_gan()'s prologue and index
    streams from RandomState(seed + f), model MRGAN(seed = s + f)"""
    from sklearn.model_selection import StratifiedKFold
    from sklearn.utils import shuffle
    from mr_gan_amd import MRGAN
    from mr_gan_amd.data import select_labeled, standard_scale
    from mr_gan_amd.mr_gan import UnequalFolds, mr_gan_folds
    X, y = _planted(360, 40, 3)
    skf = StratifiedKFold(n_splits=6, shuffle=True, random_state=1)
    sets = [[X[tr], X[te], y[tr], y[te]] for tr, te in skf.split(X, y)]
    got = mr_gan_folds(sets, percentlabeled=2.5, epochs=1, seed=5)
    s = int(np.random.RandomState(5).randint(1 << 30))
    want = []
    for f, (xtr, xte, ytr, yte) in enumerate(sets):
        rs = np.random.RandomState(5 + f)
        xtr, xte = standard_scale(xtr, xte)
        xtr, ytr = shuffle(xtr, ytr, random_state=rs)
        xl, yl, xu = select_labeled(xtr, ytr, 25, None)
        assert xl.shape == (150, 40) and xtr.shape == (300, 40)
        model = MRGAN(40, seed=s + f)
        model.fit(xl, yl, xtr, epochs=1, validation_data=(xte, yte), x_unlabeled_pool=xu, rng=rs)
        want.append(model.evaluate(xte, yte))
        model.engine.close()
    assert got == want, (got, want)
    assert len(got) == 6 and all(0.0 <= e <= 1.0 for e in got)
    with pytest.raises(UnequalFolds):
        mr_gan_folds([sets[0], [sets[1][0][:250], sets[1][1], sets[1][2][:250], sets[1][3]]], percentlabeled=2.5, epochs=1, seed=5)


def test_verbose_mr_gan_folds_prints_the_lines_of_verbose_mr_gan_calls(capsys):
    """two folds, two epochs: fold by fold the lines a verbose mr_gan() prints (prologue, sizes, one line per epoch, test error),
    compared with the numbers that depend on the model's seed (and the times) masked"""
    import re
    from sklearn.model_selection import StratifiedKFold
    from mr_gan_amd.mr_gan import mr_gan, mr_gan_folds
    X, y = _planted(360, 40, 3)
    skf = StratifiedKFold(n_splits=6, shuffle=True, random_state=1)
    sets = [[X[tr], X[te], y[tr], y[te]] for tr, te in skf.split(X, y)][:2]
    mr_gan_folds(sets, percentlabeled=2.5, epochs=2, seed=5, verbose=True)
    grouped = capsys.readouterr().out
    for f in range(2):
        mr_gan(None, None, percentlabeled=2.5, epochs=2, trainTestSets=sets[f], seed=5 + f, verbose=True)
    plain = capsys.readouterr().out
    mask = lambda s: re.sub(r"(?<== )[-0-9.]+(?:e-?\d+)?s?|nan|(?<=Test error: ).*", "#", s)
    assert mask(grouped) == mask(plain)
    assert grouped.count("Epoch 2, time") == 2 and grouped.count("Testing batches per epoch: 1") == 2 and grouped.count("Test error: ") == 2
