"""Autoencoder pre-stage without a GPU: the restatement of tests/autoencoder_ref.py against autograd, the mirror against the
restatement, the front end (mr_gan_amd/autoencoder.py, model.ae_epochs) on a recording stand-in engine, the pipeline
mr_gan_autoencoder on stand-in classes, and the layout of mrgan_ae_args."""
import contextlib
import ctypes
import os
import subprocess
import tempfile
import types

import numpy as np
import pytest
import torch

from tests import autoencoder_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, NODES, ROWS = 20, (12, 8, 4), 7


def _problem(seed=3):
    rng = np.random.default_rng(seed)
    return R.init(D, NODES, seed), rng.standard_normal((ROWS, D))


# ---- 1. the restatement against autograd -----------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_valid", [None, 5])
def test_restatement_gradients_match_autograd(rows_valid):
    d, x = _problem()
    loss, g = R.grads(d, x, rows_valid)
    ps = [torch.tensor(p, dtype=torch.float64, requires_grad=True) for p in d]
    a = torch.tensor(x, dtype=torch.float64)
    t = a
    for l in range(5):
        a = torch.relu(a @ ps[2 * l] + ps[2 * l + 1])
    y = a @ ps[10] + ps[11]
    rv = rows_valid or ROWS
    want = ((y[:rv] - t[:rv]) ** 2).mean()                          # Keras 'mse' over the counted rows
    want.backward()
    assert abs(loss - want.item()) < 1e-12 * abs(want.item())
    assert len(g) == 12
    for i, (got, p) in enumerate(zip(g, ps)):
        ref = p.grad.numpy()
        assert got.shape == ref.shape and np.linalg.norm(ref) > 0
        assert np.linalg.norm(got - ref) / np.linalg.norm(ref) < 1e-10, i


def test_mirror_without_rounding_is_the_restatement():
    d, x = _problem(5)
    ref, mir = R.Restatement(d), R.Mirror(d, q=None)
    for rv in (None, 4, None):
        l0, g0 = ref.grads(x, rv)
        l1, g1 = mir.grads(x, rv)
        assert abs(l0 - l1) <= 1e-12 * abs(l0)
        for a, b in zip(g0, g1):
            assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(a).max())
        assert abs(ref.step(x, rv) - mir.step(x, rv)) <= 1e-12
    for a, b in zip(ref.d, mir.d):
        assert np.abs(a - b).max() <= 1e-12
    assert np.abs(ref.encode(x) - mir.encode(x)).max() <= 1e-12 and ref.encode(x).shape == (ROWS, NODES[2])
    assert np.abs(ref.reconstruct(x) - mir.reconstruct(x)).max() <= 1e-12
    # and the bf16 mirror is another function: it rounds
    assert np.abs(R.Mirror(d).reconstruct(x) - ref.reconstruct(x)).max() > 1e-6


# ---- 2. the front end on a recording stand-in engine -----------------------------------------------------------------------
B, DIN = 32, 6


class Recorder(object):
    """what ae_epochs calls on an Engine, written down in call order"""

    def __init__(self):
        self.cfg = types.SimpleNamespace(batch=B, d_in=DIN)
        self.models, self.log, self.reads = 1, [], 0

    def ae_step(self, args, want_outputs=True):
        x, idx = args._refs
        self.log.append(('ae', args.rows_valid, x.clone(), idx, want_outputs, args.stream_mode))
        return 0.5 if want_outputs else None

    def metrics(self, reads):
        return [10.0 + reads, 0.0, 0.0, 0.0, 1.0 + 0.5 * reads, 0.0, 0.0, 0.0]

    def read_metrics(self, reset=True):
        self.log.append(('metrics', reset))
        self.reads += 1
        return self.metrics(self.reads - 1)

    def ae_reconstruct(self, x, idx=None, out=None, want_out=True, want_mse=True):
        self.log.append(('reconstruct', tuple(x.shape), want_out, want_mse))
        return None, 0.25

    def ae_encode(self, x, idx=None, out=None):
        self.log.append(('encode', tuple(x.shape)))
        return torch.zeros((x.shape[0], 3))


def shell(seed=9):
    from mr_gan_amd.autoencoder import Autoencoder
    obj = object.__new__(Autoencoder)
    obj.engine, obj.device, obj.seed, obj.models = Recorder(), torch.device('cpu'), seed, 1
    obj.input_dim, obj.batch_size, obj.iterations, obj.history = DIN, B, 0, []
    obj._on_stream = contextlib.nullcontext
    obj.stream = types.SimpleNamespace(synchronize=lambda: None)
    return obj


@pytest.mark.parametrize("validation", [False, True])
def test_fit_epoch_loop(validation):
    from mr_gan_amd import engine as E
    n, nb, epochs = 100, 4, 3
    rng = np.random.default_rng(4)
    X = rng.standard_normal((n, DIN)).astype(np.float32)
    Xv = rng.standard_normal((11, DIN)).astype(np.float32)
    model = shell()
    hist = model.fit(X, epochs=epochs, validation_data=Xv if validation else None)      # (default rng: RandomState(seed))
    log, want_rng = model.engine.log, np.random.RandomState(9)
    per_epoch = nb + 1 + (1 if validation else 0)
    assert hist is model.history and len(hist) == epochs and len(log) == epochs * per_epoch
    for ep in range(epochs):
        calls = log[ep * per_epoch:(ep + 1) * per_epoch]
        perm = want_rng.permutation(n)                             # a fresh permutation per epoch
        want = np.zeros((nb * B, DIN), np.float32)
        want[:n] = X[perm]
        for b in range(nb):
            name, rows_valid, x, idx, want_outputs, stream_mode = calls[b]
            assert name == 'ae' and rows_valid == (0, 0, 0, 4)[b] and idx is None and want_outputs is False and stream_mode == 0
            assert tuple(x.shape) == (B, DIN) and x.dtype == torch.float32
            np.testing.assert_array_equal(x.numpy(), want[b * B:(b + 1) * B])      # full batches, then the short one, zero padded
        assert calls[nb] == ('metrics', True)
        if validation:
            assert calls[nb + 1] == ('reconstruct', (11, DIN), False, True)
        # Keras' epoch loss: the batch means weighted by their rows -- three batches of 32 and one of 4
        total, last = model.engine.metrics(ep)[0], model.engine.metrics(ep)[4]
        assert hist[ep]['loss'] == pytest.approx(((total - last) * 32 + last * 4) / 100.0, rel=1e-12)
        assert hist[ep]['epoch'] == ep + 1
        assert hist[ep]['val_loss'] == 0.25 if validation else np.isnan(hist[ep]['val_loss'])
    assert isinstance(log[0][2], torch.Tensor) and isinstance(E.Engine.ae_args(log[0][2]), E.AeArgs)
    # encode / reconstruct / evaluate go to the engine's read-only entries
    model.engine.log[:] = []
    assert model.encode(Xv).shape == (11, 3) and model.evaluate(Xv) == 0.25
    assert model.engine.log == [('encode', (11, DIN)), ('reconstruct', (11, DIN), False, True)]


def test_sup_epochs_and_ae_epochs_share_their_batches():
    """one generator behind both loops (model.shuffled_epochs): the supervised loop's own test pins its call sequence"""
    from mr_gan_amd import model as M
    import inspect
    assert 'shuffled_epochs(' in inspect.getsource(M.sup_epochs) and 'shuffled_epochs(' in inspect.getsource(M.ae_epochs)


@pytest.mark.parametrize("nodes", [(16, 8), (32, 16, 8, 4)])
def test_encoder_nodes_must_be_three(nodes):
    from mr_gan_amd.autoencoder import Autoencoder, mr_gan_autoencoder
    with pytest.raises(ValueError, match="six layers"):
        Autoencoder(40, encoder_nodes=nodes, device='cpu')          # (raises before any device is touched)
    with pytest.raises(ValueError, match="six layers"):
        mr_gan_autoencoder(None, None, encoderNodes=nodes)


def test_encoder_widths():
    from mr_gan_amd.autoencoder import encoder_widths
    assert encoder_widths((128, 64, 16)) == (128, 64, 16, 64, 128) and encoder_widths([9, 5, 2]) == (9, 5, 2, 5, 9)


# ---- 3. the pipeline on stand-in classes -----------------------------------------------------------------------------------
def test_pipeline_on_stand_ins(monkeypatch):
    from mr_gan_amd import autoencoder as A
    from mr_gan_amd.data import synthetic_mreo
    X, y, _ = synthetic_mreo(d=40, objects_per_class=3, trials=40)
    X = X * 3.0 + 7.0                                              # (far from standard scale)
    rng = np.random.default_rng(0)
    te = np.zeros(len(y), bool)
    for c in range(6):
        te[rng.permutation(np.flatnonzero(y == c))[:10]] = True
    sets = [X[~te], X[te], y[~te], y[te]]
    seen = {}

    class FakeAE(object):
        def __init__(self, d_in, encoder_nodes, batch_size, dtype, seed, device):
            seen['ae'] = (d_in, tuple(encoder_nodes), batch_size, dtype)
            self.code = encoder_nodes[2]

        def fit(self, X, epochs, validation_data, verbose):
            seen['fit'] = (X.copy(), epochs, validation_data.copy())

        def encode(self, X):
            return np.full((len(X), self.code), float(len(X)), np.float32) + np.arange(len(X), dtype=np.float32)[:, None]

        def close(self):
            seen['ae_closed'] = True

    class FakeGAN(object):
        def __init__(self, input_dim, **kw):
            seen['gan'] = (input_dim, kw['batch_size'], kw['num_classes'])

        def fit(self, x_labeled, y_labeled, x_unlabeled, epochs, verbose, validation_data, x_unlabeled_pool, rng):
            seen['gan_fit'] = (x_labeled.shape, x_unlabeled.shape, validation_data[0].shape, epochs, x_unlabeled_pool)
            seen['train_codes'], seen['test_codes'] = x_unlabeled.copy(), validation_data[0].copy()
            return [dict(test_err=0.5)]

        def evaluate(self, X, y):
            seen['eval'] = X.shape
            return 0.125

        def close(self):
            pass
    monkeypatch.setattr(A, 'Autoencoder', FakeAE)
    monkeypatch.setattr(A, 'MRGAN', FakeGAN)
    acc = A.mr_gan_autoencoder(None, None, percentlabeled=2, epochs=3, trainTestSets=sets, encoderNodes=(24, 12, 5), ae_epochs=7, seed=1)
    assert acc == 1.0 - 0.125                                      # the ACCURACY, as the reference's function returns
    n_tr, n_te = int((~te).sum()), int(te.sum())
    assert seen['ae'] == (40, (24, 12, 5), 32, 'float32') and seen['ae_closed']
    Xtr, ep, Xte = seen['fit']
    assert ep == 7 and Xtr.shape == (n_tr, 40) and Xte.shape == (n_te, 40)
    # the scaler is fitted on the training rows only: they come out standardised, the test rows by the same map
    mu, sd = sets[0].mean(axis=0), sets[0].std(axis=0)
    np.testing.assert_allclose(Xtr, (sets[0] - mu) / sd, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(Xte, (sets[1] - mu) / sd, rtol=1e-9, atol=1e-9)
    # the GAN sees codes of width n2 for train and test, not rescaled
    assert seen['gan'] == (5, 50, 6)
    assert seen['gan_fit'] == ((6 * 20, 5), (n_tr, 5), (n_te, 5), 3, None) and seen['eval'] == (n_te, 5)
    assert sorted(seen['train_codes'][:, 0]) == sorted(n_tr + np.arange(n_tr)) and seen['test_codes'][0, 0] == n_te


# ---- 4. the C struct -------------------------------------------------------------------------------------------------------
def test_ae_args_layout_matches_header():
    from mr_gan_amd import engine as E
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "mrgan_abi.h"
int main(void) {
  printf("%zu %zu %zu %zu %d\n", sizeof(mrgan_ae_args), offsetof(mrgan_ae_args, ld_x), offsetof(mrgan_ae_args, stream_mode),
         offsetof(mrgan_ae_args, rows_valid), (int)MRGAN_FLAG_AUTOENCODER);
  return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", os.path.join(d, "t")])
        vals = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).split()]
    A = E.AeArgs
    assert vals == [ctypes.sizeof(A), A.ld_x.offset, A.stream_mode.offset, A.rows_valid.offset, E.FLAG_AUTOENCODER] and vals[4] == 32
    for name in ("mrgan_ae_step", "mrgan_ae_encode", "mrgan_ae_reconstruct"):
        assert name in E.EXPORTS and hasattr(E.load_library(), name)
