"""Model groups (mrgan_config.models > 1): G supervised trainings of one shape in one launch set.

The reference of a group is G single handles -- model m against a handle created with seed + m and loaded with model m's
weights -- and the bound is bit identity: the single handles are what the other test files hold against the oracle and the
mirror.  Problems come from tests.helpers.Case (one per model, seeds 7 + m), handles from tests.parity.engine."""
import functools

import numpy as np
import pytest
import torch

from oracle import mrgan_oracle as O
from tests import parity as P
from tests.helpers import SEED, Case, planted as _planted

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
_t = P.to_dev


def _engine(D, B, dtype, models=0, seed=SEED, flags=0, K=None, **kw):
    if K is not None:
        kw['num_classes'] = K
    return P.engine(D, B, dtype, flags=flags, models=models, seed=seed, lr=O.NN_ADAM_LR, beta1=O.NN_ADAM_B1, **kw)


@functools.lru_cache(maxsize=None)
def _cases(G, D, B, K=None, steps=3):
    """one problem per model; shared, never modified"""
    return tuple(Case(D=D, B=B, steps=steps, seed=7 + m, K=K) for m in range(G))


def _batch(case, t, B, n):
    """(x [B, D], labels [B] with -1 behind the first n rows) of step t"""
    y = case.labels[t].copy()
    y[n:] = -1
    return case.x_lab[t], y


def _state(eng, B):
    """everything a supervised step leaves behind, for the selected model of a group or for a single handle"""
    from mr_gan_amd import engine as E
    out = eng.get_weights(E.NET_D) + eng.get_slot(E.NET_D, 0) + eng.get_slot(E.NET_D, 1)
    out += [eng.debug_buffer(0, l, 1).cpu().numpy() for l in range(5)]           # stored xin (segment 0: all S rows)
    out += [eng.debug_buffer(1, l, 1).cpu().numpy() for l in range(5)]           # stored dpre
    return out


def _rows(steps, B, short):
    return [short if (short and t == steps - 1) else B for t in range(steps)]


@functools.lru_cache(maxsize=None)
def _singles(dtype, G, D, B, short=0, K=None, flags=0, nan_model=-1):
    """G single handles, model m with seed + m: -> [(outputs per step, state, iterations)]"""
    from mr_gan_amd import engine as E
    res = []
    for m, case in enumerate(_cases(G, D, B, K)):
        eng = _engine(D, B, dtype, seed=SEED + m, flags=flags, K=K)
        P.load(eng, case)
        outs = []
        for t, n in enumerate(_rows(case.steps, B, short)):
            x, y = _batch(case, t, B, n)
            if m == nan_model:
                x = np.full_like(x, np.nan)
            outs.append(eng.sup_step(E.Engine.sup_args(_t(x), _t(y, torch.int32), rows_valid=0 if n == B else n)))
        res.append((outs, _state(eng, B), eng.get_iterations()))
        eng.close()
    return res


def _load_group(eng, cases):
    for m, case in enumerate(cases):
        eng.select_model(m)
        P.load(eng, case)
    eng.select_model(0)


def _run_group(dtype, G, D, B, short=0, K=None, flags=0, nan_model=-1):
    """the same steps on one group handle -> [(outputs per step, state, iterations)] per model"""
    from mr_gan_amd import engine as E
    cases = _cases(G, D, B, K)
    eng = _engine(D, B, dtype, models=G, flags=flags, K=K)
    _load_group(eng, cases)
    outs = []
    for t, n in enumerate(_rows(cases[0].steps, B, short)):
        xs, ys = zip(*[_batch(c, t, B, n) for c in cases])
        xs = np.stack(xs)
        if nan_model >= 0:
            xs[nan_model] = np.nan
        outs.append(eng.sup_step_group(E.Engine.sup_group_args(_t(xs), _t(np.stack(ys), torch.int32), rows_valid=0 if n == B else n)))
    it = eng.get_iterations()
    res = []
    for m in range(G):
        eng.select_model(m)
        res.append(([o[m] for o in outs], _state(eng, B), it))
    eng.close()
    return res


@functools.lru_cache(maxsize=None)
def _group(*args, **kw):
    return _run_group(*args, **kw)


def _assert_same(got, want, what, models=None):
    for m, ((o_g, s_g, it_g), (o_w, s_w, it_w)) in enumerate(zip(got, want)):
        if models is not None and m not in models:
            continue
        assert it_g == it_w, (what, m, it_g, it_w)
        np.testing.assert_array_equal(np.array(o_g, np.float32), np.array(o_w, np.float32), err_msg="%s: outputs of model %d" % (what, m))
        assert len(s_g) == len(s_w) == 46
        for i, (a, b) in enumerate(zip(s_g, s_w)):
            np.testing.assert_array_equal(a, b, err_msg="%s: model %d, tensor %d (12 weights | 12 m | 12 v | 5 xin | 5 dpre)" % (what, m, i))


# ---------------------------------------------------------------------------------------------------------
# 1. bit identity with single handles
# ---------------------------------------------------------------------------------------------------------
STEP_CASES = [
    (F32, 3, 48, 20, 7, None, 0),                  # three steps, the last one short
    (BF16, 3, 72, 50, 33, None, 0),
    (BF16, 2, 200, 130, 0, None, 0),               # three 64-row column-sum tiles per model, the last with two rows; D1 has several column tiles
    (F32, 2, 48, 20, 0, 10, 0),                    # class pitch 32
    (BF16, 2, 48, 20, 0, 10, 0),
    (BF16, 2, 72, 50, 0, None, 16),                # MRGAN_FLAG_GAUSS_NOISE
]


@pytest.mark.parametrize("dtype,G,D,B,short,K,flags", STEP_CASES)
def test_group_steps_equal_single_handles(dtype, G, D, B, short, K, flags):
    """every D weight, both Adam slots, the iteration count, the two outputs of every step and the stored xin / dpre buffers of
    every model equal those of the single handle with seed + m, bit for bit"""
    got = _group(dtype, G, D, B, short, K, flags)
    want = _singles(dtype, G, D, B, short, K, flags)
    assert got[0][2] == 3
    _assert_same(got, want, "group vs singles")
    # and the models differ from each other: a group that trained model 0 three times would pass the comparison of model 0 only
    assert not np.array_equal(got[0][1][0], got[1][1][0])


def test_group_stream_mode_one_matrix_own_index_vectors():
    """bf16, G = 3, stream_mode = 1 over two batches, x_model_stride = 0: all models gather from one matrix through their own
    index vectors; labels are streams of their own"""
    from mr_gan_amd import engine as E
    G, D, B, nb = 3, 72, 50, 2
    cases = _cases(G, D, B)
    rng = np.random.default_rng(11)
    X = rng.standard_normal((400, D)).astype(np.float32)
    Y = rng.integers(0, 6, 400).astype(np.int32)
    idx = np.stack([rng.permutation(400)[:nb * B] for _ in range(G)]).astype(np.int32)
    lab = Y[idx]
    xd = _t(X)
    want = []
    for m in range(G):
        eng = _engine(D, B, BF16, seed=SEED + m)
        P.load(eng, cases[m])
        a = E.Engine.sup_args(xd, _t(lab[m], torch.int32), idx=_t(idx[m], torch.int32), stream_mode=1)
        outs = [eng.sup_step(a) for _ in range(nb)]
        want.append((outs, _state(eng, B), eng.get_iterations()))
        eng.close()
    eng = _engine(D, B, BF16, models=G)
    _load_group(eng, cases)
    a = E.Engine.sup_group_args(xd, _t(lab, torch.int32), idx=_t(idx, torch.int32), stream_mode=1)
    assert a.x_model_stride == 0 and a.idx_model_stride == nb * B and a.labels_model_stride == nb * B
    outs = [eng.sup_step_group(a) for _ in range(nb)]
    got = []
    for m in range(G):
        eng.select_model(m)
        got.append(([o[m] for o in outs], _state(eng, B), eng.get_iterations()))
    eng.close()
    assert got[0][2] == nb
    _assert_same(got, want, "stream mode")


# ---------------------------------------------------------------------------------------------------------
# 2. isolation
# ---------------------------------------------------------------------------------------------------------
def test_a_model_with_nan_inputs_leaves_the_others_alone():
    """model 1's input rows are NaN: models 0 and 2 are bit-identical to the clean run, model 1's first-layer weights are NaN"""
    G, D, B = 3, 72, 50
    clean = _group(BF16, G, D, B, 33, None, 0)
    dirty = _run_group(BF16, G, D, B, 33, None, 0, nan_model=1)
    _assert_same(dirty, clean, "NaN rows in model 1", models=(0, 2))
    # relu maps NaN to zero (fmaxf), so the NaN rows reach the weights through the first layer's weight gradient X^T dY
    assert np.isnan(dirty[1][1][0]).all(), "model 1 trained on NaN rows"
    for w in dirty[0][1][:12] + dirty[2][1][:12]:
        assert np.isfinite(w).all()


def test_set_weights_of_one_model_leaves_the_others_alone():
    from mr_gan_amd import engine as E
    G, D, B = 3, 72, 50
    cases = _cases(G, D, B)
    eng = _engine(D, B, BF16, models=G)
    _load_group(eng, cases)
    eng.select_model(2)
    eng.set_weights(E.NET_D, [np.full(p.shape, 3.0, np.float32) for p in cases[2].d0])
    for m in (0, 1):
        eng.select_model(m)
        for a, b in zip(eng.get_weights(E.NET_D), cases[m].d0):
            np.testing.assert_array_equal(a, b.astype(np.float32))
    eng.select_model(2)
    assert all((w == 3.0).all() for w in eng.get_weights(E.NET_D))
    eng.close()


# ---------------------------------------------------------------------------------------------------------
# 3. one launch set
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_a_grouped_step_is_one_launch_set(dtype):
    """G = 4: the kernel names and the launch count per name of one grouped step are those of one single step"""
    from mr_gan_amd import engine as E
    G, D, B = 4, 72, 50
    cases = _cases(G, D, B)
    one = _engine(D, B, dtype)
    P.load(one, cases[0])
    x, y = _batch(cases[0], 0, B, B)
    one.profile_begin()
    one.sup_step(E.Engine.sup_args(_t(x), _t(y, torch.int32)))
    single = {k: v[1] for k, v in one.profile_end().items()}
    one.close()
    grp = _engine(D, B, dtype, models=G)
    _load_group(grp, cases)
    xs, ys = zip(*[_batch(c, 0, B, B) for c in cases])
    grp.profile_begin()
    grp.sup_step_group(E.Engine.sup_group_args(_t(np.stack(xs)), _t(np.stack(ys), torch.int32)))
    grouped = {k: v[1] for k, v in grp.profile_end().items()}
    grp.close()
    assert grouped == single, (grouped, single)
    assert sum(single.values()) >= 13 and "stage_kernel" in single and "adam_kernel" in single and "head_kernel" in single


# ---------------------------------------------------------------------------------------------------------
# 4. per-model entries
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_per_model_entries_equal_single_handles(dtype):
    """weights and Adam slots in and out, eval_error and predict_logits per model, on a probe set larger than one pass of the
    evaluation (n > 3 S)"""
    from mr_gan_amd import engine as E
    G, D, B, n = 3, 72, 50, 3 * 128 + 17
    cases = _cases(G, D, B)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n, D)).astype(np.float32)
    y = rng.integers(0, 6, n).astype(np.int32)
    slots = [[[rng.standard_normal(p.shape).astype(np.float32) ** 2 for p in c.d0] for _ in range(2)] for c in cases]
    grp = _engine(D, B, dtype, models=G)
    _load_group(grp, cases)
    for m in range(G):
        grp.select_model(m)
        for which in (0, 1):
            grp.set_slot(E.NET_D, which, slots[m][which])
    for m in range(G):
        one = _engine(D, B, dtype, seed=SEED + m)
        P.load(one, cases[m])
        grp.select_model(m)
        for a, b, c in zip(grp.get_weights(E.NET_D), one.get_weights(E.NET_D), cases[m].d0):
            np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(a, c.astype(np.float32))
        for which in (0, 1):
            for a, b in zip(grp.get_slot(E.NET_D, which), slots[m][which]):
                np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(grp.predict_logits(_t(x)).cpu().numpy(), one.predict_logits(_t(x)).cpu().numpy())
        assert grp.eval_error(_t(x), _t(y, torch.int32)) == one.eval_error(_t(x), _t(y, torch.int32))
        assert grp.full_shape(E.NET_D, 0) == one.full_shape(E.NET_D, 0) and grp.num_tensors(E.NET_D) == 12
        one.close()
    with pytest.raises(E.MrganError, match="select_model"):
        grp.select_model(G)
    grp.close()


# ---------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------
def test_what_a_group_does_not_do_is_refused():
    from mr_gan_amd import engine as E
    D, B = 48, 20
    with pytest.raises(E.MrganError, match="models must be"):
        _engine(D, B, BF16, models=17)
    with pytest.raises(E.MrganError, match="group"):
        _engine(128, 64, E.FP8, models=2)
    with pytest.raises(E.MrganError, match="group"):
        _engine(D, B, BF16, models=2, flags=E.FLAG_FLAT_GRADS)
    with pytest.raises(E.MrganError, match="group .* needs world = 1"):
        P.engine(D, B, F32, flags=E.FLAG_FLAT_GRADS, rank=0, world=2, models=2)
    case = _cases(2, D, B)[0]
    grp = _engine(D, B, BF16, models=2)
    x, y = _t(case.x_lab[0]), _t(case.labels[0], torch.int32)
    da, ga = E.Engine.disc_args(x, y, x), E.Engine.gen_args(x)
    for call in (lambda: grp.disc_step(da), lambda: grp.gen_step(ga), lambda: grp.train_pair(da, ga),
                 lambda: grp.sup_step(E.Engine.sup_args(x, y))):
        with pytest.raises(E.MrganError, match=r"error -3: .*group"):
            call()
    assert grp.get_iterations() == 0
    grp.close()
    one = _engine(D, B, BF16)
    with pytest.raises(E.MrganError, match=r"error -3: .*not a group handle"):
        one.sup_step_group(E.Engine.sup_group_args(_t(np.stack([case.x_lab[0]] * 2)), _t(np.stack([case.labels[0]] * 2), torch.int32)))
    one.close()


# ---------------------------------------------------------------------------------------------------------
# 6. reproducibility
# ---------------------------------------------------------------------------------------------------------
def test_grouped_steps_are_bit_reproducible():
    _assert_same(_run_group(BF16, 3, 72, 50, 33, None, 0), _group(BF16, 3, 72, 50, 33, None, 0), "second fresh group handle")


# ---------------------------------------------------------------------------------------------------------
# 7. the default path is untouched
# ---------------------------------------------------------------------------------------------------------
def test_default_path_is_untouched():
    """two single bf16 handles at (72, 50), the second created after a group handle has trained on the device: identical bits,
    identical kernels; and models = 1 is models = 0"""
    import ctypes as C
    from mr_gan_amd import engine as E
    D, B = 72, 50
    case = _cases(3, D, B)[0]

    def run():
        eng = _engine(D, B, BF16)
        P.load(eng, case)
        eng.profile_begin()
        outs = [eng.sup_step(E.Engine.sup_args(_t(case.x_lab[t]), _t(case.labels[t], torch.int32))) for t in range(3)]
        names = {k: v[1] for k, v in eng.profile_end().items()}
        res = (outs, _state(eng, B), eng.get_iterations())
        eng.close()
        return res, names

    a, names_a = run()
    _run_group(BF16, 3, D, B, 33, None, 0)
    b, names_b = run()
    _assert_same([b], [a], "single handle after a group")
    assert names_a == names_b, (names_a, names_b)
    sizes = []
    for models in (0, 1, 2):
        cfg = E.default_config(D, B)
        cfg.dtype, cfg.models = BF16, models
        n = C.c_size_t(0)
        assert E.load_library().mrgan_workspace_bytes(C.byref(cfg), C.byref(n)) == 0
        sizes.append(n.value)
    assert sizes[0] == sizes[1] and sizes[2] == 2 * sizes[0]


# ---------------------------------------------------------------------------------------------------------
# 8. host level
# ---------------------------------------------------------------------------------------------------------
def test_mrnn_group_equals_single_mrnn_runs():
    """three planted 90-row sets, batch 20 (a short last batch), two epochs"""
    from mr_gan_amd import engine as E
    from mr_gan_amd.mr_nn import MRNN, MRNNGroup
    sets = [_planted(90, 40, 20 + m) for m in range(3)]
    grp = MRNNGroup(40, models=3, seed=11)
    hist = grp.fit([s[0] for s in sets], [s[1] for s in sets], epochs=2)
    errs = grp.evaluate([s[0] for s in sets], [s[1] for s in sets])
    assert grp.engine.get_iterations() == 10 and len(hist[-1]['loss']) == 3
    for m, (x, y) in enumerate(sets):
        one = MRNN(40, seed=11 + m)
        h1 = one.fit(x, y, epochs=2)
        grp.engine.select_model(m)
        for a, b in zip(grp.engine.get_weights(E.NET_D), one.engine.get_weights(E.NET_D)):
            np.testing.assert_array_equal(a, b)
        assert errs[m] == one.evaluate(x, y)
        assert hist[-1]['loss'][m] == h1[-1]['loss']
        np.testing.assert_array_equal(grp.predict_logits(m, x), one.predict_logits(x))
        one.engine.close()
    grp.engine.close()


def test_mr_nn_folds_equals_six_hand_built_trainings():
    """N = 360, D = 40, six folds, one epoch; 25 labeled rows per class: 150 rows = seven batches and a short one"""
    from sklearn.model_selection import StratifiedKFold
    from sklearn.utils import shuffle
    from mr_gan_amd.data import select_labeled, standard_scale
    from mr_gan_amd.mr_nn import MRNN, mr_nn_folds
    X, y = _planted(360, 40, 3)
    skf = StratifiedKFold(n_splits=6, shuffle=True, random_state=1)
    sets = [[X[tr], X[te], y[tr], y[te]] for tr, te in skf.split(X, y)]
    got = mr_nn_folds(sets, percentlabeled=2.5, epochs=1, seed=5)
    s = int(np.random.RandomState(5).randint(1 << 30))
    want = []
    for f, (xtr, xte, ytr, yte) in enumerate(sets):
        rs = np.random.RandomState(5 + f)
        xtr, xte = standard_scale(xtr, xte)
        xtr, ytr = shuffle(xtr, ytr, random_state=rs)
        xl, yl, _ = select_labeled(xtr, ytr, 25)
        assert xl.shape == (150, 40)
        model = MRNN(40, seed=s + f)
        model.fit(xl, yl, epochs=1, rng=rs)
        want.append(model.evaluate(xte, yte))
        model.engine.close()
    assert got == want, (got, want)
    assert len(got) == 6 and all(0.0 <= e <= 1.0 for e in got)
