"""Autoencoder handles (MRGAN_FLAG_AUTOENCODER) on the GPU: mrgan_ae_step / mrgan_ae_encode / mrgan_ae_reconstruct through the C
ABI against the numpy restatement and its bf16 mirror (tests/autoencoder_ref.py), and the front end (mr_gan_amd/autoencoder.py).

Shapes (nodes = encoder_nodes):
  A  D 200, B  32, (128, 64, 16)   ragged D (padded to 256), a code narrower than one pad unit, one row block
  B  D  96, B 130, (64, 64, 64)    three 64-row blocks, the last with 2 rows
  C  D 520, B  64, (256, 128, 64)  several column tiles in the last product, under every entry of the tile table
Bounds are those of the supervised step's tests (tests/parity.py): fp32 gradients 2e-4 (Frobenius) against fp64, bf16 by the
mirror rule err(engine, mirror) < max(3e-3, 0.6 err(mirror, fp64)), weights relative to the size of their update."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from mr_gan_amd import engine as E
from tests import autoencoder_ref as R
from tests import parity as P
from tests.helpers import Case, frob_rel_err, rel_err, update_rel_err

pytestmark = pytest.mark.gpu

SHAPES = {'A': (200, 32, (128, 64, 16)), 'B': (96, 130, (64, 64, 64)), 'C': (520, 64, (256, 128, 64))}
B1, B2 = 0.9, 0.999
_t = P.to_dev


def ae_engine(D, B, dtype, nodes, flags=0, **fields):
    """an autoencoder handle: zero sigmas, Keras' Adam defaults"""
    kw = dict(sigma=(C.c_float * 5)(), lr=R.AE_LR, beta1=R.AE_B1)
    kw.update(fields)
    return P.engine(D, B, dtype, flags=E.FLAG_AUTOENCODER | flags, d_hidden=R.widths(nodes), **kw)


@functools.lru_cache(maxsize=None)
def problem(name, steps=3):
    """(initial weights fp64, the batches float32 [steps, B, D]) of a shape; shared, never modified"""
    D, B, nodes = SHAPES[name]
    rng = np.random.default_rng(17 + ord(name))
    return R.init(D, nodes, seed=ord(name)), rng.standard_normal((steps, B, D)).astype(np.float32)


def loaded(name, dtype, **kw):
    D, B, nodes = SHAPES[name]
    eng = ae_engine(D, B, dtype, nodes, **kw)
    eng.set_weights(E.NET_D, [p.astype(np.float32) for p in problem(name)[0]])
    return eng


def f32_weights(name):
    """what a handle holds after set_weights: the fp32 roundings of the problem's weights, as fp64"""
    return [p.astype(np.float32).astype(np.float64) for p in problem(name)[0]]


def step(eng, x, rows_valid=0, want_outputs=True):
    return eng.ae_step(E.Engine.ae_args(_t(x), rows_valid=rows_valid), want_outputs=want_outputs)


# ---------------------------------------------------------------------------------------------------------
# 1. create and refusals
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("name", ['A', 'B', 'C'])
def test_create_tensor_shapes(name, dtype):
    D, B, nodes = SHAPES[name]
    eng = ae_engine(D, B, dtype, nodes)
    w = R.widths(nodes)
    dims = (D,) + w + (D,)
    assert eng.num_tensors(E.NET_D) == 12
    for l in range(6):
        assert eng.full_shape(E.NET_D, 2 * l) == (dims[l], dims[l + 1]) and eng.full_shape(E.NET_D, 2 * l + 1) == (dims[l + 1],)
    assert eng.tensor_shape(E.NET_D, 10) == (w[4], D) and eng.tensor_shape(E.NET_D, 11) == (1, D)
    # weights travel in and out at full width (the padding of the last layer is that of a hidden layer, not the class pitch)
    ws = [p.astype(np.float32) for p in problem(name)[0]]
    eng.set_weights(E.NET_D, ws)
    for a, b in zip(eng.get_weights(E.NET_D), ws):
        np.testing.assert_array_equal(a, b)
    eng.close()


def test_create_refuses_what_is_not_built():
    D, B, nodes = SHAPES['A']
    for kw in (dict(flags=E.FLAG_FLAT_GRADS), dict(flags=E.FLAG_SYNC_STATS), dict(flags=E.FLAG_FLAT_GRADS | E.FLAG_GRAD_BF16),
               dict(flags=E.FLAG_GRAD_BF16), dict(models=2), dict(world=2), dict(world=2, flags=E.FLAG_FLAT_GRADS)):
        with pytest.raises(E.MrganError, match="error -3: an autoencoder handle"):
            ae_engine(D, B, 0, nodes, **kw)
    with pytest.raises(E.MrganError, match="error -3: an autoencoder handle cannot be an fp8 handle"):
        ae_engine(128, 64, E.FP8, (128, 128, 128))
    for i in range(5):
        sigma = (C.c_float * 5)()
        sigma[i] = 0.3
        with pytest.raises(E.MrganError, match=r"error -1: an autoencoder handle needs sigma\[%d\] = 0" % i):
            ae_engine(D, B, 0, nodes, sigma=sigma)
    with pytest.raises(E.MrganError, match="error -1: an autoencoder handle needs sigma"):      # mrgan_default_config's sigmas
        P.engine(D, B, 0, flags=E.FLAG_AUTOENCODER)
    with pytest.raises(E.MrganError, match="error -1: num_classes"):                            # validated as on any handle
        ae_engine(D, B, 0, nodes, num_classes=1)


def test_entries_refuse_the_other_kind_of_handle():
    D, B, nodes = SHAPES['A']
    x, y, idx = _t(np.zeros((B, D), np.float32)), _t(np.zeros(B), torch.int32), _t(np.arange(B), torch.int32)
    ae = ae_engine(D, B, 1, nodes)
    da, ga = E.Engine.disc_args(x, y, x), E.Engine.gen_args(x)
    dga, gga = E.Engine.disc_group_args(x, y, x), E.Engine.gen_group_args(x)
    calls = [lambda: ae.disc_step(da), lambda: ae.gen_step(ga), lambda: ae.train_pair(da, ga),
             lambda: ae.sup_step(E.Engine.sup_args(x, y)), lambda: ae.sup_step_group(E.Engine.sup_group_args(x, y)),
             lambda: ae.disc_step_group(dga), lambda: ae.gen_step_group(gga), lambda: ae.train_pair_group(dga, gga),
             lambda: ae.fp8_calibration(0, E.Engine.FP8_CAL_QUERY), lambda: ae.fp8_calibration(1, E.Engine.FP8_CAL_BEGIN),
             lambda: ae.eval_error(x, y), lambda: ae.predict_logits(x), lambda: ae.input_gradient(x, y),
             lambda: ae.attribution(x, y, draws=2, sigma_input=0.1)]
    for i, call in enumerate(calls):
        with pytest.raises(E.MrganError, match="error -3: .*autoencoder handle"):
            call()
    assert ae.get_iterations() == 0
    # what the new entries refuse of their own arguments
    with pytest.raises(E.MrganError, match="error -2: ae_reconstruct: out_dev and mse_host are both null"):
        ae.ae_reconstruct(x, want_out=False, want_mse=False)
    with pytest.raises(E.MrganError, match="error -2: ae_step: a short batch cannot be combined with stream mode"):
        ae.ae_step(E.Engine.ae_args(x, idx, stream_mode=1, rows_valid=3))
    with pytest.raises(E.MrganError, match="error -2: ae_step: rows_valid"):
        ae.ae_step(E.Engine.ae_args(x, rows_valid=B + 1))
    with pytest.raises(E.MrganError, match="error -2: ae_encode: row pitch ld_code"):
        ae.ae_encode(x, out=torch.empty((B, nodes[2] - 1), device=x.device))
    with pytest.raises(E.MrganError, match="error -2: ae_reconstruct: row pitch ld_out"):
        ae.ae_reconstruct(x, out=torch.empty((B, D - 1), device=x.device))
    with pytest.raises(E.MrganError, match="error -2: ae_encode: row pitch ld_x"):
        ae.ae_encode(torch.zeros((B, D - 8), device=x.device))
    ae.close()
    gan = P.engine(D, B, 1)
    for call in (lambda: gan.ae_step(E.Engine.ae_args(x)), lambda: gan.ae_encode(x), lambda: gan.ae_reconstruct(x)):
        with pytest.raises(E.MrganError, match="error -3: ae_.*not an autoencoder handle"):
            call()
    gan.close()


# ---------------------------------------------------------------------------------------------------------
# 2. gradients and loss of the first step
# ---------------------------------------------------------------------------------------------------------
def _first_step_gradients(name, dtype, kc_cfg=-1):
    d0, xs = problem(name)
    x = xs[0]
    loss_o, g_o = R.Restatement(f32_weights(name)).grads(x.astype(np.float64))
    loss_m, g_m = R.Mirror(f32_weights(name)).grads(x.astype(np.float64))
    eng = loaded(name, dtype)
    if kc_cfg != -1:
        eng.set_tuning(E.TUNE_KC_CFG, kc_cfg)
    loss = step(eng, x)
    got = [m / (1.0 - B1) for m in eng.get_slot(E.NET_D, 0)]       # zero slots before: m = (1 - beta_1) g
    v = eng.get_slot(E.NET_D, 1)
    metrics = eng.read_metrics(reset=False)
    assert eng.get_iterations() == 1
    eng.close()
    report = []
    try:
        for i, (a, m, o) in enumerate(zip(got, g_m, g_o)):
            em, eo, emo = frob_rel_err(a, m), frob_rel_err(a, o), frob_rel_err(m, o)
            report.append("g%-2d %.1e %.1e %.1e" % (i, em, eo, emo))
            assert a.shape == o.shape
            if dtype == 0:
                assert eo < 2e-4, (i, eo)
            else:
                assert em < max(3e-3, 0.6 * emo), (i, em, emo)
            # the second slot from zero: v = (1 - beta_2) g^2
            assert frob_rel_err(np.sqrt(v[i] / (1.0 - B2)), np.abs(a)) < 1e-3, i
        report.append("loss %.8g fp64 %.8g mirror %.8g" % (loss, loss_o, loss_m))
        if dtype == 0:
            assert abs(loss - loss_o) < 2e-4 * loss_o, (loss, loss_o)
        else:
            assert abs(loss - loss_m) < max(3e-3, 0.6 * abs(loss_m - loss_o) / loss_o) * loss_o, (loss, loss_m, loss_o)
        assert metrics[0] == loss and metrics[4] == loss and metrics[1:4] == [0.0, 0.0, 0.0]
    finally:
        print("\n(%s, dtype %d, kc_cfg %d) tensor: err vs mirror | vs fp64 | mirror vs fp64\n  " % (name, dtype, kc_cfg) + "\n  ".join(report))


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("name", ['A', 'B', 'C'])
def test_first_step_gradients(name, dtype):
    _first_step_gradients(name, dtype)


@pytest.mark.parametrize("kc_cfg", [0, 1, 3, 5, 7, 9])
def test_first_step_gradients_under_every_tile(kc_cfg):
    """shape C in bf16: the last layer's forward and dX products (N = 576 / 256 padded columns) under each forced block tile"""
    _first_step_gradients('C', 1, kc_cfg)


# ---------------------------------------------------------------------------------------------------------
# 3. three steps, the second one short
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("name,short", [('A', 16), ('B', 33)])
def test_three_steps_match_restatement(name, short, dtype):
    d0, xs = problem(name)
    B = SHAPES[name][1]
    ref, mir = R.Restatement(f32_weights(name)), R.Mirror(f32_weights(name), q=None if dtype == 0 else R.O.bf16_round)
    eng = loaded(name, dtype)
    for t in range(3):
        n = short if t == 1 else B
        got = step(eng, xs[t], rows_valid=0 if n == B else n)
        want, wm = ref.step(xs[t].astype(np.float64), n), mir.step(xs[t].astype(np.float64), n)
        slack = 0.0 if t == 0 else 0.25
        if dtype == 0:
            assert abs(got - want) < (2e-4 + slack * 0.02) * want, (t, got, want)
        else:
            assert abs(got - wm) < max(3e-3, 0.6 * abs(wm - want) / want + slack * 0.2) * want, (t, got, wm, want)
    w0 = f32_weights(name)
    for i, (a, b, m, w) in enumerate(zip(eng.get_weights(E.NET_D), ref.d, mir.d, w0)):
        if dtype == 0:
            assert update_rel_err(a, b, w) < 0.03, (i, update_rel_err(a, b, w))
        else:
            assert update_rel_err(a, m, w) < max(0.05, 0.85 * update_rel_err(m, b, w)), (i, update_rel_err(a, m, w), update_rel_err(m, b, w))
    assert eng.get_iterations() == 3
    eng.close()


# ---------------------------------------------------------------------------------------------------------
# 4. what a step must not read: rows beyond rows_valid, pitch columns beyond d_in
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("name,short", [('A', 16), ('B', 33)])
def test_rows_beyond_rows_valid_and_pitch_columns_do_not_count(name, short, dtype):
    D, B, _ = SHAPES[name]
    x = problem(name)[1][0]
    rng = np.random.default_rng(2)
    res = []
    for fill in (False, True):
        buf = np.zeros((B, D + 13), np.float32)                    # (a pitch that is no multiple of 4: the scalar row loads)
        if fill:
            buf[:] = rng.permutation(B * (D + 13)).reshape(B, D + 13).astype(np.float32) * (1e3 / (B * (D + 13))) * rng.choice([-1.0, 1.0], (B, D + 13))
        buf[:short, :D] = x[:short]
        xd = _t(buf)
        eng = loaded(name, dtype)
        loss = eng.ae_step(E.Engine.ae_args(xd[:, :D], rows_valid=short))
        res.append((np.float32(loss), eng.get_weights(E.NET_D), eng.get_slot(E.NET_D, 1)))
        eng.close()
    assert res[0][0].tobytes() == res[1][0].tobytes() and np.isfinite(res[0][0])
    for a, b in zip(res[0][1] + res[0][2], res[1][1] + res[1][2]):
        assert np.array_equal(a, b) and np.isfinite(a).all()


# ---------------------------------------------------------------------------------------------------------
# 5. encode / reconstruct
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("name", ['A', 'B'])
def test_encode_and_reconstruct(name, dtype):
    D, B, nodes = SHAPES[name]
    S = -(-B // 128) * 128
    ref, mir = R.Restatement(f32_weights(name)), R.Mirror(f32_weights(name))
    rng = np.random.default_rng(8)
    pool = rng.standard_normal((3 * S + 50, D)).astype(np.float32)
    eng = loaded(name, dtype)
    pd = _t(pool)
    for n, gather in ((1, False), (B, False), (3 * S + 7, True)):
        idx = rng.permutation(len(pool))[:n].astype(np.int32) if gather else None
        rows = pool[idx] if gather else pool[:n]
        xd, idd = (pd, _t(idx, torch.int32)) if gather else (pd[:n], None)
        r64 = rows.astype(np.float64)
        outs = []
        for rep in range(2):
            code = torch.full((n, nodes[2] + 3), -7777.0, device=pd.device)
            y = torch.full((n, D + 5), -7777.0, device=pd.device)
            assert eng.ae_encode(xd, idd, out=code) is code
            _, mse = eng.ae_reconstruct(xd, idd, out=y)
            _, mse_only = eng.ae_reconstruct(xd, idd, want_out=False)
            outs.append((code.cpu().numpy(), y.cpu().numpy(), np.float32(mse), np.float32(mse_only)))
        (code, y, mse, mse_only), again = outs
        assert all(np.array_equal(a, b) for a, b in zip(outs[0], again))                      # two calls: identical bits
        assert (code[:, nodes[2]:] == -7777.0).all() and (y[:, D:] == -7777.0).all()           # columns beyond the valid width
        code, y = code[:, :nodes[2]], y[:, :D]
        for got, want_o, want_m, what in ((code, ref.encode(r64), mir.encode(r64), 'code'), (y, ref.reconstruct(r64), mir.reconstruct(r64), 'y')):
            if dtype == 0:
                assert rel_err(got, want_o) < 1e-5, (what, n, rel_err(got, want_o))
            else:
                assert rel_err(got, want_m) < max(3e-3, 0.6 * rel_err(want_m, want_o)), (what, n, rel_err(got, want_m), rel_err(want_m, want_o))
        want_mse = float(((y.astype(np.float64) - r64) ** 2).mean())                          # the mean over the returned y
        assert abs(mse - want_mse) < 1e-6 * want_mse and mse.tobytes() == mse_only.tobytes(), (n, mse, want_mse, mse_only)
    assert eng.get_iterations() == 0 and eng.read_metrics(reset=False) == [0.0] * 8
    eng.close()


# ---------------------------------------------------------------------------------------------------------
# 6. the read-only entries leave training untouched
# ---------------------------------------------------------------------------------------------------------
def _state(eng):
    return (eng.get_weights(E.NET_D) + eng.get_slot(E.NET_D, 0) + eng.get_slot(E.NET_D, 1),
            eng.get_iterations(), eng.read_metrics(reset=False))


def test_read_only_entries_leave_training_untouched():
    """shape B in bf16 (ragged batch, S = 256): rows of magnitude 1e3 through every padding row between two steps"""
    D, B, nodes = SHAPES['B']
    xs = problem('B')[1]
    big = _t(1e3 * np.random.default_rng(4).standard_normal((3 * 256 + 7, D)).astype(np.float32))
    states = []
    for reads in (True, False):
        eng = loaded('B', 1)
        step(eng, xs[0], want_outputs=False)
        if reads:
            eng.ae_encode(big)
            eng.ae_reconstruct(big)
        step(eng, xs[1], want_outputs=False)
        states.append(_state(eng))
        eng.close()
    (ta, ia, ma), (tb, ib, mb) = states
    assert ia == ib == 2 and ma == mb and np.isfinite(ma).all()
    for i, (a, b) in enumerate(zip(ta, tb)):
        assert np.array_equal(a, b) and np.isfinite(a).all(), i


# ---------------------------------------------------------------------------------------------------------
# 7. bit reproducibility; the index stream
# ---------------------------------------------------------------------------------------------------------
def test_steps_are_bit_reproducible():
    xs = problem('C')[1]
    states = []
    for _ in range(2):
        eng = loaded('C', 1)
        losses = [np.float32(step(eng, xs[t])) for t in range(3)]
        states.append((_state(eng), losses))
        eng.close()
    ((ta, ia, ma), la), ((tb, ib, mb), lb) = states
    assert ia == ib == 3 and ma == mb and [v.tobytes() for v in la] == [v.tobytes() for v in lb]
    for a, b in zip(ta, tb):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("dtype", [0, 1])
def test_index_stream_equals_gathered_batches(dtype):
    """stream mode: three batches from one whole-epoch index vector and the device batch counter = the same rows given batch by
    batch, and = the same rows gathered through per-batch index vectors"""
    D, B, _ = SHAPES['A']
    rng = np.random.default_rng(6)
    pool = rng.standard_normal((5 * B, D)).astype(np.float32)
    idx = rng.permutation(5 * B)[:3 * B].astype(np.int32)
    pd, idd = _t(pool), _t(idx, torch.int32)
    states = []
    for mode in range(3):
        eng = loaded('A', dtype)
        args = E.Engine.ae_args(pd, idd, stream_mode=1)
        for t in range(3):
            if mode == 0:
                eng.ae_step(args, want_outputs=False)
            elif mode == 1:
                eng.ae_step(E.Engine.ae_args(pd, idd[t * B:(t + 1) * B]), want_outputs=False)
            else:
                step(eng, pool[idx[t * B:(t + 1) * B]], want_outputs=False)
        states.append(_state(eng))
        eng.close()
    for other in states[1:]:
        assert other[1] == states[0][1] == 3 and other[2] == states[0][2]
        for a, b in zip(states[0][0], other[0]):
            assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------
# 8. the front end learns
# ---------------------------------------------------------------------------------------------------------
LEARN = dict(D=96, rows=512, nodes=(64, 32, 16), batch=32, seed=21, epochs=12)
LEARN_FRACTION = 0.07


def planted_rank8(rows=LEARN['rows'], D=LEARN['D'], seed=5):
    """rows of a planted 8-dimensional subspace of R^D (unit variance per column, 1 % noise)"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((rows, 8)) @ rng.standard_normal((8, D)) / np.sqrt(8.0)
    return (X + 0.01 * rng.standard_normal((rows, D))).astype(np.float32)


def restatement_learning_curve(epochs=LEARN['epochs']):
    """the schedule of Autoencoder.fit on the fp64 restatement: the front end's initial weights (glorot from RandomState(seed),
    zero biases), a permutation per epoch from RandomState(seed + 1), batches of 32 -> Keras' epoch losses"""
    from mr_gan_amd.model import glorot_uniform
    X, D, B = planted_rank8().astype(np.float64), LEARN['D'], LEARN['batch']
    rng = np.random.RandomState(LEARN['seed'])
    dims = (D,) + R.widths(LEARN['nodes']) + (D,)
    d0 = []
    for l in range(6):
        d0 += [glorot_uniform(rng, dims[l], dims[l + 1]).astype(np.float64), np.zeros(dims[l + 1])]
    ref, perm_rng, out = R.Restatement(d0), np.random.RandomState(LEARN['seed'] + 1), []
    for _ in range(epochs):
        Xp, tot = X[perm_rng.permutation(len(X))], 0.0
        for b in range(0, len(X), B):
            tot += ref.step(Xp[b:b + B].copy()) * len(Xp[b:b + B])
        out.append(tot / len(X))
    return out


@pytest.mark.parametrize("dtype", ['float32', 'bfloat16'])
def test_front_end_learns(dtype):
    """Autoencoder.fit on planted rank-8 data (D 96, 512 rows, nodes (64, 32, 16), batch 32, seed 21, permutations from
    RandomState(22)): after 12 epochs the last epoch's loss is below 0.07 of the first epoch's.
    The condition comes from the fp64 restatement on the same schedule (restatement_learning_curve, run on the CPU): its epoch
    losses fall from 1.0587 (epoch 1) to 0.0344 (epoch 12), a fraction of 0.0325; the bound is twice that fraction, rounded up."""
    from mr_gan_amd.autoencoder import Autoencoder
    X = planted_rank8()
    model = Autoencoder(LEARN['D'], encoder_nodes=LEARN['nodes'], batch_size=LEARN['batch'], dtype=dtype, seed=LEARN['seed'], device=P.DEV)
    hist = model.fit(X, epochs=LEARN['epochs'], validation_data=X[:100], rng=np.random.RandomState(LEARN['seed'] + 1))
    print("\nepoch losses:", " ".join("%.4f" % h['loss'] for h in hist))
    assert len(hist) == LEARN['epochs'] and [h['epoch'] for h in hist] == list(range(1, LEARN['epochs'] + 1))
    assert hist[-1]['loss'] < LEARN_FRACTION * hist[0]['loss'], (hist[0]['loss'], hist[-1]['loss'])
    # the history's val_loss is evaluate() of those rows, and the codes have the width n2
    assert hist[-1]['val_loss'] == model.evaluate(X[:100]) and model.encode(X[:40]).shape == (40, 16)
    y = model.reconstruct(X[:100])
    assert abs(float(((y.astype(np.float64) - X[:100]) ** 2).mean()) - hist[-1]['val_loss']) < 1e-5 * hist[-1]['val_loss']
    assert len(model.get_weights()) == 12 and model.get_weights()[10].shape == (64, 96)
    model.close()


# ---------------------------------------------------------------------------------------------------------
# 9. the GAN path is untouched
# ---------------------------------------------------------------------------------------------------------
def test_gan_path_is_untouched_by_an_autoencoder_handle():
    """a default bf16 handle at (400, 50), three train_pair steps, before and after an autoencoder handle has trained on the
    device: the same weights, kernel names and launch counts (the LDS-limit cache of the kernels is process-wide)"""
    case = Case(D=400, B=50, steps=3, device_z=True)

    def gan():
        eng = P.engine(400, 50, 1)
        P.load(eng, case)
        eng.profile_begin()
        for t in range(3):
            eng.train_pair(P.disc_args(case, t, device_z=True), P.gen_args(case, t, device_z=True))
        prof = eng.profile_end()
        out = eng.get_weights(E.NET_D) + eng.get_weights(E.NET_G), {k: v[1] for k, v in prof.items()}, eng.get_iterations()
        eng.close()
        return out
    before = gan()
    for dtype in (0, 1):
        ae = loaded('C', dtype)
        for t in range(2):
            step(ae, problem('C')[1][t], want_outputs=False)
        ae.ae_reconstruct(_t(problem('C')[1][2]))
        ae.close()
    after = gan()
    assert before[1] == after[1] and before[2] == after[2] == 6 and len(before[1]) > 5
    assert not any(k.startswith(("recon_head", "cast_rows", "fold_loss")) for k in after[1])
    for a, b in zip(before[0], after[0]):
        assert np.array_equal(a, b)
