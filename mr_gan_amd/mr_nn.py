"""Supervised neural-network baseline of the reference (mr_nn.py:69-119 and its --tables 2 4 loops, :128-168) on the HIP
engine: the discriminator stack of mr_gan.py (GaussianNoise 0.3 / 0.5, Dense 1000-500-250-250-250 relu, linear Dense(6))
trained on the labeled subset only with loss = 'mse' against the one-hot label and Keras' default Adam.

    python -m mr_gan_amd.mr_nn --tables 2 4 [-v] [--dtype bfloat16] [--group-folds]

Every train_on_batch is one mrgan_sup_step (include/mrgan_abi.h): the same stage / dense / dX / dW / Adam kernels as the GAN
step, with the mse head.  There is no CPU path.

--group-folds trains the six folds of each (modality, percentage) of table 2 as ONE model group (MRNNGroup: one
mrgan_sup_step_group per batch, one launch set for the six trainings) and prints the same lines."""
import argparse

import numpy as np
import torch

from mr_gan_amd import engine as E
from mr_gan_amd.data import prologue, resolve_num_classes, train_test_sets
from mr_gan_amd.model import Front, group_size, sup_epochs
from mr_gan_amd.mr_gan import dataset, print_lines
from mr_gan_amd.mr_svm import baseline_tables

NN_LR, NN_BETA_1 = 0.001, 0.9              # Keras-2.0.9 Adam defaults (mr_nn.py:112 optimizer='adam')


class MRNN(Front):
    """model.compile(loss='mse', optimizer='adam') + fit / evaluate of mr_nn.py:101-118 on one MI355X."""

    nets = (E.NET_D,)

    def __init__(self, input_dim, batch_size=20, dtype='float32', seed=None, device='cuda:0', num_classes=6,
                 d_hidden=(1000, 500, 250, 250, 250), lr=NN_LR, beta_1=NN_BETA_1, init_weights=True, noise='irwin-hall'):
        Front.__init__(self, input_dim, batch_size, dtype, seed, device, noise, init_weights, d_hidden, fp8=False,
                       num_classes=num_classes, lr=lr, beta1=beta_1)                # mr_nn.py:71 is unseeded

    def train_on_batch(self, x, labels):
        """one batch of at most batch_size rows -> (mse, training error)"""
        B, n = self.batch_size, len(x)
        with self._on_stream():
            xb = torch.zeros((B, self.input_dim), device=self.device)
            yb = torch.full((B,), -1, dtype=torch.int32, device=self.device)
            xb[:n], yb[:n] = self._dev(x), self._dev(labels, torch.int32)
            self._hold = a = E.Engine.sup_args(xb, yb, rows_valid=0 if n == B else n)
            return self.engine.sup_step(a)

    def fit(self, x, y, epochs=100, verbose=0, rng=None):
        """sup_epochs for this model; rng: the source of the permutations (default RandomState(seed))"""
        with self._on_stream():
            hist = sup_epochs(self.engine, self._dev, [x], [y], [rng or np.random.RandomState(self.seed)], epochs, verbose)
            self.stream.synchronize()
        return hist

    def predict_logits(self, X):
        return self._predict_logits(0, X)

    def evaluate(self, X, y):
        """1 - accuracy over the whole set (mr_nn.py:118)"""
        return self._evaluate(0, X, y)

    def saliency(self, X, y=None, objective='mse', heatmap=True, **kw):
        """Front._saliency for the baseline (kw: method, draws, sigma, baseline, times_input); the default objective is its
        training loss, as in the reference's others/mr_nn_activation_map.py -> (maps [n, D] float32, classes [n] int32)"""
        return self._saliency(0, X, y, objective, heatmap, **kw)


class MRNNGroup(Front):
    """`models` MRNN trainings of one shape on one group handle (mrgan_config.models): model m is initialised and seeded exactly
    as MRNN(seed=seed + m) -- glorot from RandomState(seed + m), engine seed seed + m -- and every batch of all models is one
    mrgan_sup_step_group.  The results are those of the `models` single MRNN runs bit for bit."""

    nets = (E.NET_D,)

    def __init__(self, input_dim, models, batch_size=20, dtype='float32', seed=None, device='cuda:0', num_classes=6,
                 d_hidden=(1000, 500, 250, 250, 250), lr=NN_LR, beta_1=NN_BETA_1, init_weights=True, noise='irwin-hall'):
        Front.__init__(self, input_dim, batch_size, dtype, seed, device, noise, init_weights, d_hidden, fp8=False,
                       models=group_size(models, 'MRNN'), num_classes=num_classes, lr=lr, beta1=beta_1)

    def fit(self, xs, ys, epochs=100, verbose=0, rngs=None):
        """MRNN.fit of every model at once: `models` arrays of equal length; model m's permutations come from rngs[m]
        (default RandomState(seed + m), MRNN.fit's default).  One sup_step_group per batch, the short last one included."""
        G = self.models
        if len(xs) != G or len(ys) != G or len({len(x) for x in xs} | {len(y) for y in ys}) != 1:
            raise ValueError("fit: a group trains %d sets of equal length" % G)
        with self._on_stream():
            hist = sup_epochs(self.engine, self._dev, xs, ys, rngs or [np.random.RandomState(self.seed + m) for m in range(G)], epochs, verbose)
            self.stream.synchronize()
        return hist

    def predict_logits(self, m, X):
        return self._predict_logits(m, X)

    def evaluate(self, Xs, ys):
        """[1 - accuracy of model m over (Xs[m], ys[m])], model by model"""
        return [self._evaluate(m, Xs[m], ys[m]) for m in range(self.models)]


def mr_nn_folds(sets, percentlabeled=50, verbose=False, epochs=100, batch_size=20, dtype='float32', seed=None, device='cuda:0',
                noise='irwin-hall', num_classes=None):
    """mr_nn() of every [X_train, X_test, y_train, y_test] of `sets` (the folds of one table-2 cell: equal shapes) as one
    model group -> their test errors.  Fold f runs mr_nn()'s prologue and its permutation stream from RandomState(seed + f);
    its model is MRNN(seed=s + f) with s drawn from RandomState(seed)."""
    E.noise_flags(noise)
    base = int(seed if seed is not None else np.random.randint(1 << 30))
    num_classes = resolve_num_classes(num_classes)
    rss = [np.random.RandomState(base + f) for f in range(len(sets))]
    folds = []
    for s, rs in zip(sets, rss):
        folds.append(prologue(s, percentlabeled, None, rs, num_classes))
        print_lines(folds[-1][-1], verbose)
    x_labeled, y_labeled, _, _, X_test, y_test, _ = zip(*folds)
    model = MRNNGroup(x_labeled[0].shape[1], len(sets), batch_size=batch_size, dtype=dtype, seed=int(np.random.RandomState(base).randint(1 << 30)),
                      device=device, noise=noise, num_classes=num_classes)
    model.fit(x_labeled, y_labeled, epochs=epochs, rngs=rss)
    errors = model.evaluate(X_test, y_test)
    model.close()
    return errors


def mr_nn(X, y, percentlabeled=50, trainTestSets=None, verbose=False, epochs=100, batch_size=20, dtype='float32',
          seed=None, device='cuda:0', noise='irwin-hall', num_classes=None):
    E.noise_flags(noise)
    rs = np.random.RandomState(seed if seed is not None else np.random.randint(1 << 31))     # mr_nn.py:71 is unseeded
    num_classes = resolve_num_classes(num_classes)                 # None: the reference's six materials
    sets = train_test_sets(X, y, trainTestSets, rs, num_classes)   # mr_nn.py:74-81
    x_labeled, y_labeled, _, _, X_test, y_test, lines = prologue(sets, percentlabeled, None, rs, num_classes)
    print_lines(lines, verbose)
    model = MRNN(x_labeled.shape[1], batch_size=batch_size, dtype=dtype, seed=int(rs.randint(1 << 31)), device=device, noise=noise,
                 num_classes=num_classes)
    model.fit(x_labeled, y_labeled, epochs=epochs, rng=rs)         # mr_nn.py:117
    testerror = model.evaluate(X_test, y_test)                     # mr_nn.py:118
    model.close()
    return testerror


def main(argv=None, dataset_fn=dataset, fn=None, folds_fn=None):
    parser = argparse.ArgumentParser(description='Supervised NN baseline for material recognition on haptic data.')
    parser.add_argument('-t', '--tables', nargs='+', help='[Required] Tables to recompute', required=True)
    parser.add_argument('-v', '--verbose', help='Verbose', action='store_true')
    parser.add_argument('--dtype', default='float32', choices=['float32', 'bfloat16'])
    parser.add_argument('--noise', default='irwin-hall', choices=['irwin-hall', 'gaussian'],
                        help="generator of the GaussianNoise layers: the engine's default, or true normals as the reference draws")
    parser.add_argument('--group-folds', action='store_true',
                        help='table 2: train the six folds of each (modality, percentage) as one model group (one launch set)')
    args = parser.parse_args(argv)
    if fn is None:
        def fn(X, y, **kw):
            return mr_nn(X, y, dtype=args.dtype, noise=args.noise, **kw)
    if args.group_folds and folds_fn is None:
        def folds_fn(sets, **kw):
            return mr_nn_folds(sets, dtype=args.dtype, noise=args.noise, **kw)
    baseline_tables(args.tables, fn, dataset_fn, args.verbose, folds_fn=folds_fn if args.group_folds else None)


if __name__ == '__main__':
    main()
