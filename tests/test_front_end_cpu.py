"""The Python front end without a GPU: the data prologue against a hand restatement, and the two epoch loops (model.gan_epochs,
model.sup_epochs) driven through the four front classes on a recording stand-in engine: draw order, argument structs, the
calls per batch and per epoch, and the history."""
import contextlib
import types

import numpy as np
import pytest
import torch

from tests.helpers import planted

D, B = 8, 4


# ---- 1. the data prologue ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("percentunlabeled", [None, 1.0])
def test_prologue_equals_hand_restatement(percentunlabeled):
    from sklearn.model_selection import StratifiedKFold
    from sklearn.utils import shuffle
    from mr_gan_amd.data import prologue, select_labeled, standard_scale
    X, y = planted(360, 40, 3)
    tr, te = next(iter(StratifiedKFold(n_splits=6, shuffle=True, random_state=1).split(X, y)))
    sets = [X[tr], X[te], y[tr], y[te]]
    rs = np.random.RandomState(5)
    xl, yl, pool, xtr, xte, yte, lines = prologue(sets, 2.5, percentunlabeled, rs, 6)

    rs2 = np.random.RandomState(5)
    wtr, wte = standard_scale(X[tr], X[te])
    wtr, wytr = shuffle(wtr, y[tr], random_state=rs2)
    wl, wyl, wpool = select_labeled(wtr, wytr, 25, None if percentunlabeled is None else 10)
    for got, want in ((xl, wl), (yl, wyl), (xtr, wtr), (xte, wte), (yte, y[te])):
        np.testing.assert_array_equal(got, want)
    if percentunlabeled is None:
        assert pool is None and wpool is None
    else:
        assert pool.shape == (6 * 35, 40)
        np.testing.assert_array_equal(pool, wpool)
    assert rs.randint(1 << 31) == rs2.randint(1 << 31)             # (the shuffle is the one draw)
    assert lines == [('Num of class examples in test set:', [10, 10, 10, 10, 10, 10]),
                     ('X_train:', (300, 40), 'y_train:', (300,), 'X_test:', (60, 40), 'y_test:', (60,)),
                     ('x_labeled:', (150, 40), 'y_labeled:', (150,))]


# ---- the stand-in engine -------------------------------------------------------------------------------------------
class Recorder(object):
    """what the epoch loops call on an Engine, written down in call order"""

    def __init__(self, models):
        self.cfg = types.SimpleNamespace(batch=B, noise_size=3, d_in=D)
        self.models, self.sel, self.log = models, 0, []

    def set_iterations(self, iterations, batch_counter):
        self.log.append(('iterations', iterations, batch_counter))

    def train_pair(self, dargs, gargs):
        self.log.append(('pair', dargs, gargs))

    def train_pair_group(self, dargs, gargs):
        self.log.append(('pair_group', dargs, gargs))

    def select_model(self, m):
        self.sel = m
        self.log.append(('select', m))

    def metrics(self, m, reads):
        return [float(3 * (10 * reads + m) + k) for k in range(8)]

    def read_metrics(self, reset=True):
        reads = sum(1 for e in self.log if e == ('metrics', self.sel))
        self.log.append(('metrics', self.sel))
        return self.metrics(self.sel, reads)

    def eval_error(self, x, labels):
        self.log.append(('eval', self.sel, tuple(x.shape), tuple(labels.shape)))
        return 0.125 * (self.sel + 1)

    def _sup(self, name, args, want_outputs):
        x, labels, _ = args._refs
        self.log.append((name, args.rows_valid, x.clone(), labels.clone(), want_outputs))
        return (0.5, 0.25) if want_outputs else None

    def sup_step(self, args, want_outputs=True):
        return self._sup('sup', args, want_outputs)

    def sup_step_group(self, args, want_outputs=True):
        out = self._sup('sup_group', args, want_outputs)
        return out and [(out[0] + m, out[1] + m) for m in range(self.models)]


def shell(cls, models, seed=9):
    """an object of a front class around a Recorder, on device 'cpu' and without a stream"""
    obj = object.__new__(cls)
    obj.engine, obj.device, obj.seed, obj.models = Recorder(models), torch.device('cpu'), seed, models
    obj.input_dim, obj.batch_size, obj.iterations, obj.history = D, B, 0, []
    obj._on_stream = contextlib.nullcontext
    obj.stream = types.SimpleNamespace(synchronize=lambda: None)
    return obj


# ---- 2. the GAN epoch loop -----------------------------------------------------------------------------------------
def _gan_data(G, pool_rows):
    rng = np.random.default_rng(1)
    f = lambda n: [rng.standard_normal((n, D)).astype(np.float32) for _ in range(G)]
    xl, xu, xv = f(6), f(12), f(10)
    yl = [((np.arange(6) + m) % 6).astype(np.int64) for m in range(G)]
    yv = [(np.arange(10) % 6).astype(np.int32) for _ in range(G)]
    return xl, yl, xu, (f(pool_rows) if pool_rows else None), list(zip(xv, yv))


@pytest.mark.parametrize("pool_rows", [None, 8])
@pytest.mark.parametrize("G", [1, 3])
def test_gan_epoch_loop(G, pool_rows):
    from mr_gan_amd import engine as E
    from mr_gan_amd.model import MRGAN, MRGANGroup, epoch_streams
    xl, yl, xu, pools, val = _gan_data(G, pool_rows)
    rngs = [np.random.RandomState(100 + m) for m in range(G)]
    if G == 1:
        model = shell(MRGAN, 1)
        hist = model.fit(xl[0], yl[0], xu[0], epochs=2, validation_data=val[0], x_unlabeled_pool=pools and pools[0], rng=rngs[0])
    else:
        model = shell(MRGANGroup, G)
        hist = model.fit(xl, yl, xu, epochs=2, validation_data=val, x_unlabeled_pools=pools, rngs=rngs)
    nb, log = 3, model.engine.log
    per_epoch = 1 + nb + 3 * G + 1
    assert len(log) == 2 * per_epoch and model.iterations == 2 * 2 * nb and hist is model.history and len(hist) == 2
    want_rngs = [np.random.RandomState(100 + m) for m in range(G)]
    stacked = (lambda a: np.stack(a)) if G > 1 else (lambda a: a[0])
    for ep in range(2):
        calls = log[ep * per_epoch:(ep + 1) * per_epoch]
        assert calls[0] == ('iterations', 2 * nb * ep, 0)
        pairs = calls[1:1 + nb]
        assert all(c[0] == ('pair_group' if G > 1 else 'pair') and c[1] is pairs[0][1] and c[2] is pairs[0][2] for c in pairs)
        dargs, gargs = pairs[0][1:]
        assert isinstance(dargs, E.DiscGroupArgs if G > 1 else E.DiscArgs) and isinstance(gargs, E.GenGroupArgs if G > 1 else E.GenArgs)
        inds, unl = zip(*[epoch_streams(r, 6, 12, pool_rows) for r in want_rngs])
        x_lab, labels, x_unl, z, idx_lab, idx_unl = dargs._refs
        x_unl2, z2, idx_unl2 = gargs._refs
        for got, want in ((idx_lab, stacked(inds)), (labels, stacked([y[i] for y, i in zip(yl, inds)])),
                          (idx_unl, stacked([u[0] for u in unl])), (idx_unl2, stacked([u[1] for u in unl])),
                          (x_lab, stacked(xl)), (x_unl, stacked(pools or xu))):
            assert got.dtype == (torch.float32 if got is x_lab or got is x_unl else torch.int32)
            np.testing.assert_array_equal(got.numpy(), want)
        assert x_unl2 is x_unl and z is None and z2 is None and dargs.stream_mode == 1 and gargs.stream_mode == 1
        assert (dargs.idx_lab, dargs.labels, dargs.idx_unl, gargs.idx_unl) == tuple(t.data_ptr() for t in (idx_lab, labels, idx_unl, idx_unl2))
        if G > 1:
            assert (dargs.idx_lab_model_stride, dargs.labels_model_stride, dargs.idx_unl_model_stride, gargs.idx_unl_model_stride) == (12,) * 4
            assert (dargs.x_lab_model_stride, dargs.x_unl_model_stride) == (6 * D, (pool_rows or 12) * D)
        want_tail = []
        for m in range(G):                                         # whole validation batches: 8 of the 10 rows
            want_tail += [('select', m), ('metrics', m), ('eval', m, (8, D), (8,))]
        assert calls[1 + nb:] == want_tail + [('select', 0)]
        for k, name in enumerate(('loss_lab', 'loss_unl', 'train_err', 'loss_gen')):
            want = [model.engine.metrics(m, ep)[k] / nb for m in range(G)]
            assert hist[ep][name] == (want if G > 1 else want[0])
        assert hist[ep]['test_err'] == ([0.125 * (m + 1) for m in range(G)] if G > 1 else 0.125)
        assert hist[ep]['epoch'] == ep + 1 and isinstance(hist[ep]['time'], float)


def test_gan_epoch_loop_host_z():
    """z_source='host': after the epoch's index streams, one normal draw of [nb, 2, B, noise]; z1 = [:, 0], z2 = [:, 1]"""
    from mr_gan_amd.model import MRGAN, epoch_streams
    xl, yl, xu, _, _ = _gan_data(1, None)
    model = shell(MRGAN, 1)
    model.fit(xl[0], yl[0], xu[0], epochs=2, rng=np.random.RandomState(3), z_source='host')
    rng = np.random.RandomState(3)
    pairs = [c for c in model.engine.log if c[0] == 'pair']
    for ep in range(2):
        inds, unl = epoch_streams(rng, 6, 12)
        zz = rng.normal(0.0, 1.0, size=(3, 2, B, 3)).astype(np.float32)
        dargs, gargs = pairs[3 * ep][1:]
        np.testing.assert_array_equal(dargs._refs[4].numpy(), inds)
        np.testing.assert_array_equal(dargs._refs[3].numpy(), zz[:, 0].reshape(12, 3))
        np.testing.assert_array_equal(gargs._refs[1].numpy(), zz[:, 1].reshape(12, 3))
        assert (dargs.z, gargs.z) == (dargs._refs[3].data_ptr(), gargs._refs[1].data_ptr())
    assert [c for c in model.engine.log if c[0] == 'eval'] == []   # (no validation data: nothing evaluated)
    assert all(np.isnan(rec['test_err']) for rec in model.history)
    with pytest.raises(ValueError, match="z_source"):
        model.fit(xl[0], yl[0], xu[0], epochs=1, z_source='file')
    with pytest.raises(ValueError, match="fewer training rows"):
        model.fit(xl[0], yl[0], xu[0][:3], epochs=1)


# ---- 3. the supervised epoch loop ----------------------------------------------------------------------------------
@pytest.mark.parametrize("verbose", [0, 1])
@pytest.mark.parametrize("G", [1, 3])
def test_supervised_epoch_loop(G, verbose, capsys):
    from mr_gan_amd.mr_nn import MRNN, MRNNGroup
    n, nb = 10, 3
    rng = np.random.default_rng(2)
    xs = [rng.standard_normal((n, D)).astype(np.float32) for _ in range(G)]
    ys = [((np.arange(n) + m) % 6).astype(np.int64) for m in range(G)]
    if G == 1:
        model = shell(MRNN, 1, seed=9)
        hist = model.fit(xs[0], ys[0], epochs=2, verbose=verbose)  # (default rng: RandomState(seed))
    else:
        model = shell(MRNNGroup, G, seed=9)
        hist = model.fit(xs, ys, epochs=2, verbose=verbose)        # (default rngs: RandomState(seed + m))
    log, rngs = model.engine.log, [np.random.RandomState(9 + m) for m in range(G)]
    assert len(log) == 2 * nb and all(c[0] == ('sup_group' if G > 1 else 'sup') for c in log)
    for ep in range(2):
        perms = [r.permutation(n) for r in rngs]                   # model by model
        want_x = np.zeros((G, nb * B, D), np.float32)
        want_y = np.full((G, nb * B), -1, np.int32)
        for m in range(G):
            want_x[m, :n], want_y[m, :n] = xs[m][perms[m]], ys[m][perms[m]]
        for b in range(nb):
            _, rows_valid, x, labels, want_outputs = log[ep * nb + b]
            assert rows_valid == (0, 0, 2)[b]
            assert want_outputs is (b == nb - 1 and (ep == 1 or verbose == 1))
            sl = slice(b * B, (b + 1) * B)
            np.testing.assert_array_equal(x.numpy(), want_x[:, sl] if G > 1 else want_x[0, sl])
            np.testing.assert_array_equal(labels.numpy(), want_y[:, sl] if G > 1 else want_y[0, sl])
            assert labels.dtype == torch.int32
    assert np.array_equal(log[-1][3].numpy().reshape(G, B)[:, 2:], np.full((G, 2), -1))
    want = [dict(epoch=ep, loss=[0.5 + m for m in range(G)] if G > 1 else 0.5, train_err=[0.25 + m for m in range(G)] if G > 1 else 0.25)
            for ep in ((0, 1) if verbose else (1,))]
    assert hist == want
    out = capsys.readouterr().out
    if not verbose:
        assert out == ''
    elif G == 1:
        assert out == 'Epoch 1: loss 0.50000, train err 0.2500\nEpoch 2: loss 0.50000, train err 0.2500\n'
    else:
        assert out == ''.join('Epoch %d: loss 0.50000 1.50000 2.50000, train err 0.2500 1.2500 2.2500\n' % e for e in (1, 2))
