"""Supervised neural-network baseline of the reference (mr_nn.py:69-119 and its --tables 2 4 loops, :128-168) on the HIP
engine: the discriminator stack of mr_gan.py (GaussianNoise 0.3 / 0.5, Dense 1000-500-250-250-250 relu, linear Dense(6))
trained on the labeled subset only with loss = 'mse' against the one-hot label and Keras' default Adam.

    python -m mr_gan_amd.mr_nn --tables 2 4 [-v] [--dtype bfloat16] [--group-folds]

Every train_on_batch is one mrgan_sup_step (include/mrgan_abi.h): the same stage / dense / dX / dW / Adam kernels as the GAN
step, with the mse head.  There is no CPU path.

--group-folds trains the six folds of each (modality, percentage) of table 2 as ONE model group (MRNNGroup: one
mrgan_sup_step_group per batch, one launch set for the six trainings) and prints the same lines."""
import argparse
import sys

import numpy as np
import torch

from mr_gan_amd import engine as E
from mr_gan_amd.data import resolve_num_classes, select_labeled, standard_scale
from mr_gan_amd.model import MRGAN, glorot_uniform
from mr_gan_amd.mr_gan import dataset
from mr_gan_amd.mr_svm import baseline_tables

NN_LR, NN_BETA_1 = 0.001, 0.9              # Keras-2.0.9 Adam defaults (mr_nn.py:112 optimizer='adam')


def nn_config(input_dim, batch_size, dtype, seed, num_classes, d_hidden, lr, beta_1, noise, models=0):
    """the mrgan_config of MRNN (models = 0) and MRNNGroup (model m draws what a handle with seed + m draws)"""
    cfg = E.default_config(input_dim, batch_size)
    cfg.dtype = {'float32': E.F32, 'fp32': E.F32, 'bfloat16': E.BF16, 'bf16': E.BF16}[dtype]      # (fp8 covers the GAN step only)
    cfg.num_classes = num_classes
    for i, w in enumerate(d_hidden):
        cfg.d_hidden[i] = w
    cfg.lr, cfg.beta1 = lr, beta_1
    cfg.seed = seed
    if models:
        cfg.models = models
    cfg.flags |= E.noise_flags(noise)                              # the GaussianNoise layers' generator (engine.noise_flags)
    return cfg


def init_discriminator(engine, seed):
    """Keras defaults for the (selected model's) discriminator stack: kernels glorot_uniform from RandomState(seed), biases zero"""
    rng = np.random.RandomState(seed)
    ws = []
    for i in range(engine.num_tensors(E.NET_D)):
        shp = engine.full_shape(E.NET_D, i)
        ws.append(glorot_uniform(rng, shp[0], shp[1]) if len(shp) == 2 else np.zeros(shp, np.float32))
    engine.set_weights(E.NET_D, ws)


class MRNN(object):
    """model.compile(loss='mse', optimizer='adam') + fit / evaluate of mr_nn.py:101-118 on one MI355X."""

    def __init__(self, input_dim, batch_size=20, dtype='float32', seed=None, device='cuda:0', num_classes=6,
                 d_hidden=(1000, 500, 250, 250, 250), lr=NN_LR, beta_1=NN_BETA_1, init_weights=True, noise='irwin-hall'):
        self.input_dim, self.batch_size = int(input_dim), int(batch_size)
        self.seed = int(np.random.randint(1 << 31)) if seed is None else int(seed)      # mr_nn.py:71 is unseeded
        self.engine = E.Engine(nn_config(self.input_dim, self.batch_size, dtype, self.seed, num_classes, d_hidden, lr, beta_1, noise), device)
        self.device = self.engine.device
        self.stream = torch.cuda.Stream(self.device)
        if init_weights:
            init_discriminator(self.engine, self.seed)

    def _dev(self, a, dtype=torch.float32):
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dtype).contiguous()
        return torch.from_numpy(np.ascontiguousarray(a)).to(device=self.device, dtype=dtype).contiguous()

    def _on_stream(self):
        return torch.cuda.stream(self.stream)

    def train_on_batch(self, x, labels):
        """one batch of at most batch_size rows -> (mse, training error)"""
        B, n = self.batch_size, len(x)
        xb = torch.zeros((B, self.input_dim), device=self.device)
        yb = torch.full((B,), -1, dtype=torch.int32, device=self.device)
        xb[:n], yb[:n] = self._dev(x), self._dev(labels, torch.int32)
        with torch.cuda.stream(self.stream):
            self.stream.wait_stream(torch.cuda.current_stream(self.device))
            return self.engine.sup_step(E.Engine.sup_args(xb, yb, rows_valid=0 if n == B else n))

    def fit(self, x, y, epochs=100, verbose=0, rng=None):
        """Keras fit(batch_size, epochs, shuffle=True): a fresh permutation per epoch, batches in order, the last one short."""
        rng = rng or np.random.RandomState(self.seed)
        B, n = self.batch_size, len(x)
        nb = (n + B - 1) // B
        xd, yd = self._dev(x), self._dev(y, torch.int32)
        xs = torch.zeros((nb * B, self.input_dim), device=self.device)
        ys = torch.full((nb * B,), -1, dtype=torch.int32, device=self.device)
        hist = []
        with torch.cuda.stream(self.stream):
            self.stream.wait_stream(torch.cuda.current_stream(self.device))
            for ep in range(epochs):
                perm = torch.from_numpy(rng.permutation(n)).to(self.device)
                xs[:n], ys[:n] = xd[perm], yd[perm]
                last = ep == epochs - 1 or verbose
                out = None
                for b in range(nb):
                    short = n - b * B if (b + 1) * B > n else 0
                    out = self.engine.sup_step(E.Engine.sup_args(xs[b * B:(b + 1) * B], ys[b * B:(b + 1) * B], rows_valid=short),
                                               want_outputs=bool(last and b == nb - 1))
                if out is not None:
                    hist.append(dict(epoch=ep, loss=out[0], train_err=out[1]))
                    if verbose:
                        print('Epoch %d: loss %.5f, train err %.4f' % (ep + 1, out[0], out[1]))
            self.stream.synchronize()
        return hist

    def predict_logits(self, X):
        with torch.cuda.stream(self.stream):
            return self.engine.predict_logits(self._dev(X)).cpu().numpy()

    def evaluate(self, X, y):
        """1 - accuracy over the whole set (mr_nn.py:118)"""
        with torch.cuda.stream(self.stream):
            return self.engine.eval_error(self._dev(X), self._dev(y, torch.int32))

    def saliency(self, X, y=None, objective='mse', heatmap=True, **kw):
        """MRGAN.saliency for the baseline (kw: method, draws, sigma, baseline, times_input); the default objective is its
        training loss, as in the reference's others/mr_nn_activation_map.py -> (maps [n, D] float32, classes [n] int32)"""
        return MRGAN.saliency(self, X, y, objective, heatmap, **kw)


class MRNNGroup(object):
    """`models` MRNN trainings of one shape on one group handle (mrgan_config.models): model m is initialised and seeded exactly
    as MRNN(seed=seed + m) -- glorot from RandomState(seed + m), engine seed seed + m -- and every batch of all models is one
    mrgan_sup_step_group.  The results are those of the `models` single MRNN runs bit for bit."""

    def __init__(self, input_dim, models, batch_size=20, dtype='float32', seed=None, device='cuda:0', num_classes=6,
                 d_hidden=(1000, 500, 250, 250, 250), lr=NN_LR, beta_1=NN_BETA_1, init_weights=True, noise='irwin-hall'):
        self.input_dim, self.batch_size, self.models = int(input_dim), int(batch_size), int(models)
        if not 2 <= self.models <= E.MAX_MODELS:
            raise ValueError("a model group has 2 .. %d models, got %d (one model: MRNN)" % (E.MAX_MODELS, self.models))
        self.seed = int(np.random.randint(1 << 31)) if seed is None else int(seed)
        self.engine = E.Engine(nn_config(self.input_dim, self.batch_size, dtype, self.seed, num_classes, d_hidden, lr, beta_1, noise,
                                         models=self.models), device)
        self.device = self.engine.device
        self.stream = torch.cuda.Stream(self.device)
        if init_weights:
            for m in range(self.models):
                self.engine.select_model(m)
                init_discriminator(self.engine, self.seed + m)
            self.engine.select_model(0)

    _dev = MRNN._dev

    def fit(self, xs, ys, epochs=100, verbose=0, rngs=None):
        """MRNN.fit of every model at once: `models` arrays of equal length; model m's permutations come from rngs[m]
        (default RandomState(seed + m), MRNN.fit's default).  One sup_step_group per batch, the short last one included."""
        G, B = self.models, self.batch_size
        if len(xs) != G or len(ys) != G or len({len(x) for x in xs} | {len(y) for y in ys}) != 1:
            raise ValueError("fit: a group trains %d sets of equal length" % G)
        rngs = rngs or [np.random.RandomState(self.seed + m) for m in range(G)]
        n = len(xs[0])
        nb = (n + B - 1) // B
        xd = torch.stack([self._dev(x) for x in xs])
        yd = torch.stack([self._dev(y, torch.int32) for y in ys])
        xb = torch.zeros((G, nb * B, self.input_dim), device=self.device)
        yb = torch.full((G, nb * B), -1, dtype=torch.int32, device=self.device)
        hist = []
        with torch.cuda.stream(self.stream):
            self.stream.wait_stream(torch.cuda.current_stream(self.device))
            for ep in range(epochs):
                for m in range(G):
                    perm = torch.from_numpy(rngs[m].permutation(n)).to(self.device)
                    xb[m, :n], yb[m, :n] = xd[m][perm], yd[m][perm]
                last = ep == epochs - 1 or verbose
                out = None
                for b in range(nb):
                    short = n - b * B if (b + 1) * B > n else 0
                    out = self.engine.sup_step_group(E.Engine.sup_group_args(xb[:, b * B:(b + 1) * B], yb[:, b * B:(b + 1) * B], rows_valid=short),
                                                     want_outputs=bool(last and b == nb - 1))
                if out is not None:
                    hist.append(dict(epoch=ep, loss=[o[0] for o in out], train_err=[o[1] for o in out]))
                    if verbose:
                        print('Epoch %d: loss %s, train err %s' % (ep + 1, ' '.join('%.5f' % o[0] for o in out), ' '.join('%.4f' % o[1] for o in out)))
            self.stream.synchronize()
        return hist

    def predict_logits(self, m, X):
        with torch.cuda.stream(self.stream):
            self.engine.select_model(m)
            return self.engine.predict_logits(self._dev(X)).cpu().numpy()

    def evaluate(self, Xs, ys):
        """[1 - accuracy of model m over (Xs[m], ys[m])], model by model"""
        errs = []
        with torch.cuda.stream(self.stream):
            for m in range(self.models):
                self.engine.select_model(m)
                errs.append(self.engine.eval_error(self._dev(Xs[m]), self._dev(ys[m], torch.int32)))
        return errs


def _prologue(sets, percentlabeled, rs, num_classes, verbose):
    """the data prologue of mr_nn() for given [X_train, X_test, y_train, y_test] -> (x_labeled, y_labeled, X_test, y_test)"""
    from sklearn.utils import shuffle
    X_train, X_test, y_train, y_test = sets
    if verbose:
        print('Num of class examples in test set:', [int(np.sum(y_test == i)) for i in range(num_classes)])
        print('X_train:', np.shape(X_train), 'y_train:', np.shape(y_train), 'X_test:', np.shape(X_test), 'y_test:', np.shape(y_test))
    X_train, X_test = standard_scale(X_train, X_test)              # mr_nn.py:86-88
    X_train, y_train = shuffle(X_train, y_train, random_state=rs)  # mr_nn.py:91
    x_labeled, y_labeled, _ = select_labeled(X_train, y_train, int(10 * percentlabeled), num_classes=num_classes)      # mr_nn.py:75
    if verbose:
        print('x_labeled:', np.shape(x_labeled), 'y_labeled:', np.shape(y_labeled))
    return x_labeled, y_labeled, X_test, y_test


def mr_nn_folds(sets, percentlabeled=50, verbose=False, epochs=100, batch_size=20, dtype='float32', seed=None, device='cuda:0',
                noise='irwin-hall', num_classes=None):
    """mr_nn() of every [X_train, X_test, y_train, y_test] of `sets` (the folds of one table-2 cell: equal shapes) as one
    model group -> their test errors.  Fold f runs mr_nn()'s prologue and its permutation stream from RandomState(seed + f);
    its model is MRNN(seed=s + f) with s drawn from RandomState(seed)."""
    E.noise_flags(noise)
    base = int(seed if seed is not None else np.random.randint(1 << 30))
    num_classes = resolve_num_classes(num_classes)
    rss = [np.random.RandomState(base + f) for f in range(len(sets))]
    folds = [_prologue(s, percentlabeled, rs, num_classes, verbose) for s, rs in zip(sets, rss)]
    model = MRNNGroup(folds[0][0].shape[1], len(sets), batch_size=batch_size, dtype=dtype, seed=int(np.random.RandomState(base).randint(1 << 30)),
                      device=device, noise=noise, num_classes=num_classes)
    model.fit([f[0] for f in folds], [f[1] for f in folds], epochs=epochs, rngs=rss)
    errors = model.evaluate([f[2] for f in folds], [f[3] for f in folds])
    model.engine.close()
    return errors


def mr_nn(X, y, percentlabeled=50, trainTestSets=None, verbose=False, epochs=100, batch_size=20, dtype='float32',
          seed=None, device='cuda:0', noise='irwin-hall', num_classes=None):
    from sklearn.model_selection import train_test_split
    E.noise_flags(noise)
    rs = np.random.RandomState(seed if seed is not None else np.random.randint(1 << 31))     # mr_nn.py:71 is unseeded
    num_classes = resolve_num_classes(num_classes)                 # None: the reference's six materials
    test_ratio = 200 * num_classes                                 # mr_nn.py:74
    if trainTestSets is None:                                      # mr_nn.py:78-81
        trainTestSets = train_test_split(X, y, test_size=test_ratio, stratify=y, random_state=rs)
    x_labeled, y_labeled, X_test, y_test = _prologue(trainTestSets, percentlabeled, rs, num_classes, verbose)
    model = MRNN(x_labeled.shape[1], batch_size=batch_size, dtype=dtype, seed=int(rs.randint(1 << 31)), device=device, noise=noise,
                 num_classes=num_classes)
    model.fit(x_labeled, y_labeled, epochs=epochs, rng=rs)         # mr_nn.py:117
    testerror = model.evaluate(X_test, y_test)                     # mr_nn.py:118
    model.engine.close()
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
