"""Keras-shaped front end of the HIP training path.

The reference script exposes no class -- its model lives in local variables of mr_gan()
(mr_gan.py:109-171).  The fit / evaluate / predict shape mirrors how the same authors drive Keras
models elsewhere in the repository (mr_nn.py:117-118, others/mr_gan_autoencoder.py:125-139).

Front is what the four public classes share (MRGAN and MRGANGroup here, MRNN and MRNNGroup in mr_nn.py); gan_epochs and
sup_epochs are the two epoch loops, each for the G >= 1 models of a handle; ae_epochs (autoencoder.py) shares the shuffled
batches of sup_epochs.
"""
import contextlib
import sys
import time

import numpy as np
import torch

from mr_gan_amd import engine as E
from mr_gan_amd.data import tiled_permutation


# the per-epoch line of mr_gan.py:227
EPOCH_LINE = 'Epoch %d, time = %ds, loss labeled = %.4f, loss unlabeled = %.4f, train error = %.4f, test error = %.4f'


def epoch_line(rec, m=None):
    """EPOCH_LINE of a history record of gan_epochs (m: the model, where the record is a group's)"""
    return EPOCH_LINE % ((rec['epoch'], rec['time']) + tuple(rec[k] if m is None else rec[k][m]
                                                              for k in ('loss_lab', 'loss_unl', 'train_err', 'test_err')))


def glorot_uniform(rng, fan_in, fan_out):
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, size=(fan_in, fan_out)).astype(np.float32)


def init_weights(engine, nets, seed):
    """Keras defaults for `nets` of the selected model, from one RandomState(seed) walked in the nets' order: Dense kernels
    glorot_uniform, biases zero, BN gamma (generator tensor 2) one / beta zero."""
    rng = np.random.RandomState(seed)
    for net in nets:
        ws = []
        for i in range(engine.num_tensors(net)):
            shp = engine.full_shape(net, i)
            if len(shp) == 2:
                ws.append(glorot_uniform(rng, shp[0], shp[1]))
            else:
                ws.append((np.ones if net == E.NET_G and i == 2 else np.zeros)(shp, np.float32))
        engine.set_weights(net, ws)


DTYPES = {'float32': E.F32, 'fp32': E.F32, 'bfloat16': E.BF16, 'bf16': E.BF16, 'fp8': E.FP8, 'float8': E.FP8}


def front_config(input_dim, batch_size, dtype, seed, noise, d_hidden, models=0, flags=0, g_hidden=None, fp8=True, **fields):
    """the mrgan_config of a front class: models = 0 for one model, else a group (model m draws what a handle with seed + m
    draws); fields: further scalar fields under their C names; fp8 False: the supervised step has no fp8 form"""
    cfg = E.default_config(input_dim, batch_size)                  # (leaves flags at 0)
    if DTYPES[dtype] == E.FP8 and not fp8:
        raise KeyError(dtype)
    cfg.dtype, cfg.seed = DTYPES[dtype], seed
    for i, w in enumerate(g_hidden or ()):
        cfg.g_hidden[i] = w
    for i, w in enumerate(d_hidden):
        cfg.d_hidden[i] = w
    for k, v in fields.items():
        setattr(cfg, k, v)
    if models:
        cfg.models = models
    cfg.flags = flags | E.noise_flags(noise)                       # the generator of the GaussianNoise sites and the device-drawn z
    return cfg


def group_size(models, single):
    if not 2 <= int(models) <= E.MAX_MODELS:
        raise ValueError("a model group has 2 .. %d models, got %d (one model: %s)" % (E.MAX_MODELS, models, single))
    return int(models)


def epoch_streams(rng, n_lab, n_train, n_pool=None):
    """One epoch's index streams, drawn from rng in the reference's order (the draws and their order are part of the results):
    the labelled tiling (mr_gan.py:189), then three unlabelled permutations (:193-195; the third is unused) or, with a table-6
    pool of n_pool rows, three tilings of it (:197-202) -> (inds, [unl, unl2, unused])"""
    inds = tiled_permutation(rng, n_lab, n_train)
    if n_pool is None:
        return inds, [rng.permutation(n_train).astype(np.int32) for _ in range(3)]
    return inds, [tiled_permutation(rng, n_pool, n_train) for _ in range(3)]


def gan_epochs(engine, dev, x_labeled, y_labeled, x_unlabeled, pools, validation, rngs, epochs, iterations, history, verbose=0,
               z_source='device'):
    """The epoch loop of mr_gan.py:183-228 for the G = len(rngs) models of `engine` (G > 1: a group handle), appending one
    record per epoch to `history` -> the Keras iteration count afterwards.

    x_labeled / y_labeled: per model the class-sorted labeled subset (mr_gan.py:102-103); x_unlabeled: per model X_train (every
    training row is used as unlabeled data, mr_gan.py:193-194); pools: per model the table-6 restricted pool (:197-202), or
    None; validation: per model (X, y), or None; dev(array, dtype) uploads.  The matrices are uploaded once and stay resident
    ([n, D], stacked [G, n, D] for a group); per epoch only the index streams (model m's from rngs[m], in the reference's order)
    go to the device, every batch is one (D, G) pair call for all models, and the per-batch scalars are accumulated on the
    device and read back once per epoch, model by model.
    z_source: 'device' draws the generator input on the GPU (the engine's counter-based generator);
    'host' draws it as the reference does, np.random.normal(0, 1, [B, noise]) twice per iteration (mr_gan.py:206, :212), from
    the model's rng after its index streams, and uploads one epoch's worth at a time."""
    G, B = len(rngs), engine.cfg.batch
    group = engine.models > 1                                      # the one choice between a single handle's entries and a group's
    disc_args, gen_args, pair = ((E.Engine.disc_group_args, E.Engine.gen_group_args, engine.train_pair_group) if group else
                                 (E.Engine.disc_args, E.Engine.gen_args, engine.train_pair))
    resident = lambda arrays: torch.stack([dev(a) for a in arrays]) if group else dev(arrays[0])
    stream = lambda arrays, dtype=torch.int32: dev(np.stack(arrays) if group else arrays[0], dtype)
    xl, xu = resident(x_labeled), resident(x_unlabeled)
    src = xu if pools is None else resident(pools)
    yl = [np.asarray(y).astype(np.int32) for y in y_labeled]
    n_train, n_lab, n_pool = xu.shape[-2], xl.shape[-2], None if pools is None else src.shape[-2]
    nb = n_train // B                                              # mr_gan.py:173 (remainder rows dropped)
    if nb < 1:
        raise ValueError("fewer training rows (%d) than one batch (%d)" % (n_train, B))
    if z_source not in ('device', 'host'):
        raise ValueError("z_source must be 'device' or 'host'")
    val = None if validation is None else [(dev(x), dev(y, torch.int32)) for x, y in validation]
    for epoch in range(1, epochs + 1):
        begin = time.time()
        inds, unl, zs = [], [], []
        for rng in rngs:                                           # model by model: its streams, then its z
            i, u = epoch_streams(rng, n_lab, n_train, n_pool)
            inds.append(i)
            unl.append(u)
            if z_source == 'host':                                 # :206 then :212, per iteration
                zs.append(rng.normal(0.0, 1.0, size=(nb, 2, B, engine.cfg.noise_size)).astype(np.float32))
        z1, z2 = [stream([z[:, k].reshape(nb * B, -1) for z in zs], torch.float32) for k in (0, 1)] if zs else (None, None)
        dargs = disc_args(xl, stream([y[i] for y, i in zip(yl, inds)]), src, z1, stream(inds), stream([u[0] for u in unl]), stream_mode=1)
        gargs = gen_args(src, z2, stream([u[1] for u in unl]), stream_mode=1)
        engine.set_iterations(iterations, 0)
        for _ in range(nb):                                        # mr_gan.py:204-213
            pair(dargs, gargs)
        iterations += 2 * nb
        rec = dict(epoch=epoch, time=0.0, loss_lab=[], loss_unl=[], train_err=[], loss_gen=[], test_err=[])
        for m in range(G):                                         # metrics (one sync per model) and evaluation: model by model
            engine.select_model(m)
            for k, v in zip(('loss_lab', 'loss_unl', 'train_err', 'loss_gen'), engine.read_metrics(reset=True)[:4]):
                rec[k].append(v / nb)
            test_err = float('nan')
            if val is not None:
                nte = (val[m][0].shape[0] // B) * B                # mr_gan.py:221-223: mean over whole test batches
                if nte > 0:
                    test_err = engine.eval_error(val[m][0][:nte], val[m][1][:nte])
            rec['test_err'].append(test_err)
        engine.select_model(0)
        rec['time'] = time.time() - begin
        if not group:                                              # one model's record holds scalars
            rec = {k: v[0] if isinstance(v, list) else v for k, v in rec.items()}
        history.append(rec)
        if verbose:                                                # mr_gan.py:227, once per model
            for m in range(G):
                print('Model %d: ' % m + epoch_line(rec, m) if group else epoch_line(rec))
            sys.stdout.flush()
    return iterations


def shuffled_epochs(engine, dev, xs, ys, rngs, epochs, make, step):
    """The batches of Keras fit(batch_size, epochs, shuffle=True) for the G = len(rngs) models of `engine`, as a generator: per
    epoch a fresh permutation per model, drawn model by model from rngs[m], fills the resident rows ([G, nb * B, D], and the
    labels where ys is given; their padding -- zeros, label -1 -- stays), then (epoch, batches, run) is yielded: run(read)
    launches the batches in order, the last one short (rows_valid), as step(args, want_outputs=b == read) and returns the
    outputs of batch `read` (-1: none are read).  make(x[, labels], rows_valid=...) builds a batch's argument struct, once: every
    epoch reuses them."""
    G, B, n = len(rngs), engine.cfg.batch, len(xs[0])
    group = engine.models > 1                                      # the one choice between a single handle's entries and a group's
    nb = (n + B - 1) // B
    xd = [dev(x) for x in xs]
    yd = None if ys is None else [dev(y, torch.int32) for y in ys]
    device = xd[0].device
    xb = torch.zeros((G, nb * B, engine.cfg.d_in), device=device)
    yb = None if ys is None else torch.full((G, nb * B), -1, dtype=torch.int32, device=device)
    xv = xb if group else xb[0]
    yv = None if yb is None else (yb if group else yb[0])
    args = []                                                      # one struct per batch, reused by every epoch

    def first_epoch():                                             # (builds them between its launches, not ahead of the first one)
        for b in range(nb):
            cols = (xv.narrow(-2, b * B, B),) + (() if yv is None else (yv.narrow(-1, b * B, B),))
            args.append(make(*cols, rows_valid=n - b * B if (b + 1) * B > n else 0))
            yield args[-1]
    for ep in range(epochs):
        for m, rng in enumerate(rngs):
            perm = torch.from_numpy(rng.permutation(n)).to(device)
            torch.index_select(xd[m], 0, perm, out=xb[m, :n])      # what an epoch's permutation fills; the padding stays
            if yd is not None:
                torch.index_select(yd[m], 0, perm, out=yb[m, :n])

        def run(read, ep=ep):
            out = None
            for b, a in enumerate(args if ep else first_epoch()):
                out = step(a, want_outputs=b == read)
            return out if read == nb - 1 else None
        yield ep, nb, run


def sup_epochs(engine, dev, xs, ys, rngs, epochs, verbose=0):
    """shuffled_epochs of mr_nn.py:117 for the G = len(rngs) models of `engine` (G > 1: a group handle): every batch is one
    supervised step call for all models, the padding of the short last batch carries label -1.  The loss and training error
    of an epoch's last batch are read on the last epoch (verbose: on every epoch) -> [records of those epochs]"""
    group = engine.models > 1
    make, step = (E.Engine.sup_group_args, engine.sup_step_group) if group else (E.Engine.sup_args, engine.sup_step)
    hist = []
    for ep, nb, run in shuffled_epochs(engine, dev, xs, ys, rngs, epochs, make, step):
        out = run(nb - 1 if ep == epochs - 1 or verbose else -1)   # the batch whose outputs are read, if any
        if out is not None:
            loss, err = zip(*(out if group else [out]))
            hist.append(dict(epoch=ep, loss=list(loss), train_err=list(err)) if group else dict(epoch=ep, loss=loss[0], train_err=err[0]))
            if verbose:
                print('Epoch %d: loss %s, train err %s' % (ep + 1, ' '.join('%.5f' % v for v in loss), ' '.join('%.4f' % v for v in err)))
    return hist


def ae_epochs(engine, dev, x, rng, epochs, history, validation=None, verbose=0):
    """shuffled_epochs of others/mr_gan_autoencoder.py:127, autoencoder.fit(X, X, batch_size, shuffle=True), appending one record
    per epoch to `history`: loss = the mean of the batch losses weighted by their rows, as Keras reports it -- from the epoch
    metrics accumulated on the device (their sum and the last batch's loss, one read per epoch) -- and val_loss = the mse over
    `validation` (nan without)."""
    n, B = len(x), engine.cfg.batch
    xv = None if validation is None else dev(validation)
    for ep, nb, run in shuffled_epochs(engine, dev, [x], None, [rng], epochs, E.Engine.ae_args, engine.ae_step):
        run(-1)
        m = engine.read_metrics(reset=True)
        total, last = m[0], m[4]                                   # sum over the epoch's batches, the (short) last batch
        loss = ((total - last) * B + last * (n - (nb - 1) * B)) / n
        val = float('nan') if xv is None else engine.ae_reconstruct(xv, want_out=False)[1]
        history.append(dict(epoch=ep + 1, loss=loss, val_loss=val))
        if verbose:
            print('Epoch %d/%d - loss: %.4f - val_loss: %.4f' % (ep + 1, epochs, loss, val))
            sys.stdout.flush()
    return history


class Front(object):
    """What the front classes share: the seed (None: drawn, the reference is unseeded), the config, the Engine on `device`, a
    private HIP stream (graph capture is not permitted on the legacy default stream), Keras-default weights for every model
    (model m from seed + m), and the per-model forms of predict_logits / evaluate / saliency."""

    nets = (E.NET_G, E.NET_D)                                      # what init_weights fills, in its order

    def __init__(self, input_dim, batch_size, dtype, seed, device, noise, init, d_hidden, **config):
        self.input_dim, self.batch_size = int(input_dim), int(batch_size)
        self.seed = int(np.random.randint(1 << 31)) if seed is None else int(seed)
        self.cfg = front_config(self.input_dim, self.batch_size, dtype, self.seed, noise, d_hidden, **config)
        self.engine = E.Engine(self.cfg, device)
        self.device, self.models = self.engine.device, self.engine.models
        self.stream = torch.cuda.Stream(self.device)
        self.iterations = 0
        self.history = []
        if init:
            for m in range(self.models):
                self.engine.select_model(m)
                init_weights(self.engine, self.nets, self.seed + m)
            self.engine.select_model(0)

    def close(self):
        self.engine.close()

    def _dev(self, a, dtype=torch.float32):
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dtype).contiguous()
        return torch.from_numpy(np.ascontiguousarray(a)).to(device=self.device, dtype=dtype).contiguous()

    def _on_stream(self):
        """the private stream, behind what the caller's current stream has been given so far"""
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        return torch.cuda.stream(self.stream)

    @contextlib.contextmanager
    def _model(self, m):
        """_on_stream with model m selected; model 0 again afterwards"""
        with self._on_stream():
            self.engine.select_model(m)
            try:
                yield
            finally:
                self.engine.select_model(0)

    def _predict_logits(self, m, X):
        with self._model(m):
            return self.engine.predict_logits(self._dev(X)).cpu().numpy()

    def _evaluate(self, m, X, y):
        with self._model(m):
            return self.engine.eval_error(self._dev(X), self._dev(y, torch.int32))

    def _saliency(self, m, X, y=None, objective='xent', heatmap=True, method='gradient', draws=None, sigma=None, baseline=None,
                  times_input=False):
        """Saliency maps of model m's discriminator (the reference's others/mr_nn_activation_map.py): per row of X the gradient
        of `objective` -- 'xent' (the labelled loss term), 'logit' (the class score) or 'mse' -- at class y[i], or at the
        predicted class when y is None, with respect to the input; heatmap: |g / (rms(g) + 1e-5)| min-max scaled to [0, 1]
        per row (a zero gradient gives a zero row), else the raw values.  method (engine.attribution_plan):
          'gradient'    one gradient of the noise-free forward
          'smoothgrad'  the mean over `draws` (16) forwards with GaussianNoise, accumulated on the device; sigma None: the
                        network's own sigmas (the training forward), a float: input-only noise, (input, hidden): both
          'integrated'  integrated gradients over `draws` (16) points of the path from `baseline` (None: zeros, the training
                        mean of scaled data) to the row, times (x - baseline)
        times_input multiplies the 'gradient' / 'smoothgrad' map by the input.  The noise of a 'smoothgrad' map depends on
        the seed, the rows and the arguments only, not on how far the model has trained.
        -> (maps [n, D] float32, classes [n] int32)"""
        code = E.saliency_objective(objective)                     # (checked before anything touches the object or the device)
        plan = E.attribution_plan(method, draws, sigma, baseline, times_input, d_in=self.input_dim,
                                  own_sigmas=(float(self.cfg.sigma[0]), float(self.cfg.sigma[1])))
        post = E.SAL_HEATMAP if heatmap else E.SAL_RAW
        with self._model(m):
            x, t = self._dev(X), None if y is None else self._dev(y, torch.int32)
            if plan['baseline'] is not None:
                plan['baseline'] = self._dev(plan['baseline'])
            maps, cls = self.engine.attribution(x, t, code, post, **plan)
            return maps.cpu().numpy(), cls.cpu().numpy()


class MRGAN(Front):
    """Feature-matching semi-supervised GAN of mr_gan.py on one MI355X.

    dtype: 'float32' (fp32 MFMA: logits within 1e-3 of the reference arithmetic) or 'bfloat16'
    (bf16 MFMA, fp32 accumulate and fp32 master weights: the throughput mode).
    noise: 'irwin-hall' (default) or 'gaussian': the generator of the five GaussianNoise sites and of the device-drawn z
    (engine.noise_flags); 'gaussian' draws true normals as the reference's K.random_normal does, at a slower step.
    """

    def __init__(self, input_dim, batch_size=50, dtype='float32', seed=None, device='cuda:0', num_classes=6,
                 noise_size=100, g_hidden=(500, 500), d_hidden=(1000, 500, 250, 250, 250), lr=0.0006, beta_1=0.5,
                 unlabeled_weight=1.0, use_graph=True, rank=0, world=1, flags=0, init_weights=True, noise='irwin-hall'):
        Front.__init__(self, input_dim, batch_size, dtype, seed, device, noise, init_weights, d_hidden, g_hidden=g_hidden,
                       flags=flags | (E.FLAG_GRAPH if use_graph else 0), num_classes=num_classes, noise_size=noise_size,
                       lr=lr, beta1=beta_1, unlabeled_weight=unlabeled_weight, rank=rank, world=world)

    def get_weights(self, net='discriminator'):
        return self.engine.get_weights(E.NET_D if net.startswith('d') else E.NET_G)

    def set_weights(self, weights, net='discriminator'):
        self.engine.set_weights(E.NET_D if net.startswith('d') else E.NET_G, weights)

    # ---- the three compiled functions (mr_gan.py:169-171) on host arrays --------------------------------------
    def train_batch_disc(self, x_lab, labels, x_unl, noise=None):
        with self._on_stream():
            self._hold = a = E.Engine.disc_args(self._dev(x_lab), self._dev(labels, torch.int32), self._dev(x_unl),
                                                None if noise is None else self._dev(noise))
            self.iterations += 1
            return self.engine.disc_step(a)

    def train_batch_gen(self, x_unl, noise=None):
        with self._on_stream():
            self._hold = a = E.Engine.gen_args(self._dev(x_unl), None if noise is None else self._dev(noise))
            self.iterations += 1
            return self.engine.gen_step(a)

    def test_batch(self, x, labels):
        return self._evaluate(0, x, labels)

    # ---- Keras-shaped API ---------------------------------------------------------------------------------------
    def fit(self, x_labeled, y_labeled, x_unlabeled, epochs=100, batch_size=None, verbose=0, validation_data=None,
            x_unlabeled_pool=None, rng=None, z_source='device'):
        """gan_epochs for this model: x_unlabeled_pool is the table-6 pool, rng the source of the index streams (and of a
        'host' z); the default is seeded by the model's seed -> history"""
        if batch_size is not None and batch_size != self.batch_size:
            raise ValueError("batch_size is fixed at construction (%d)" % self.batch_size)
        with self._on_stream():
            self.iterations = gan_epochs(self.engine, self._dev, [x_labeled], [y_labeled], [x_unlabeled],
                                         None if x_unlabeled_pool is None else [x_unlabeled_pool],
                                         None if validation_data is None else [validation_data],
                                         [rng or np.random.RandomState(self.seed ^ 0x5bd1e995)], epochs, self.iterations, self.history,
                                         verbose, z_source)
        return self.history

    def predict_logits(self, X):
        return self._predict_logits(0, X)

    def predict(self, X):
        return np.argmax(self.predict_logits(X), axis=1)

    def evaluate(self, X, y):
        """test_batch([0, X, y]) over the whole set (mr_gan.py:230) -> error rate."""
        return self._evaluate(0, X, y)

    def saliency(self, X, y=None, objective='xent', heatmap=True, **kw):
        """Front._saliency of the model (kw: method, draws, sigma, baseline, times_input)"""
        return self._saliency(0, X, y, objective, heatmap, **kw)


class MRGANGroup(Front):
    """`models` MRGAN trainings of one shape on one group handle (mrgan_config.models): model m is MRGAN(seed=seed + m) -- the
    same glorot streams for G and D, engine seed seed + m -- and every (D, G) pair of all models is one train_pair_group (one
    launch set per sub-step).  The results are those of the `models` single MRGAN runs bit for bit."""

    def __init__(self, input_dim, models, batch_size=50, dtype='float32', seed=None, device='cuda:0', num_classes=6,
                 noise_size=100, g_hidden=(500, 500), d_hidden=(1000, 500, 250, 250, 250), lr=0.0006, beta_1=0.5,
                 unlabeled_weight=1.0, use_graph=True, flags=0, init_weights=True, noise='irwin-hall'):
        models = group_size(models, 'MRGAN')
        if dtype in ('fp8', 'float8'):
            raise ValueError("a model group cannot be an fp8 handle")
        Front.__init__(self, input_dim, batch_size, dtype, seed, device, noise, init_weights, d_hidden, g_hidden=g_hidden,
                       models=models, flags=flags | (E.FLAG_GRAPH if use_graph else 0), num_classes=num_classes,
                       noise_size=noise_size, lr=lr, beta1=beta_1, unlabeled_weight=unlabeled_weight)

    def fit(self, x_labeled, y_labeled, x_unlabeled, epochs=100, verbose=0, validation_data=None, x_unlabeled_pools=None, rngs=None):
        """MRGAN.fit (z drawn on the device) of every model at once.  x_labeled / y_labeled / x_unlabeled: `models` arrays each,
        of equal length across the models; validation_data: `models` (X, y) pairs, or None; x_unlabeled_pools: `models` table-6
        pools of equal length, or None.  Model m's permutation streams come from rngs[m] (default: MRGAN.fit's default for
        seed + m).  The matrices stay resident as [models][n][D]; one train_pair_group per batch, metrics per model once per epoch."""
        G, pools = self.models, x_unlabeled_pools
        groups = [x_labeled, y_labeled, x_unlabeled] + ([pools] if pools is not None else [])
        if any(len(g) != G for g in groups) or any(len({len(a) for a in g}) != 1 for g in groups) or len(x_labeled[0]) != len(y_labeled[0]):
            raise ValueError("fit: a group trains %d sets of equal length" % G)
        if validation_data is not None and len(validation_data) != G:
            raise ValueError("fit: validation_data is one (X, y) pair per model")
        rngs = rngs or [np.random.RandomState((self.seed + m) ^ 0x5bd1e995) for m in range(G)]
        with self._on_stream():
            self.iterations = gan_epochs(self.engine, self._dev, x_labeled, y_labeled, x_unlabeled, pools, validation_data, rngs, epochs,
                                         self.iterations, self.history, verbose)
        return self.history

    def predict_logits(self, m, X):
        return self._predict_logits(m, X)

    def saliency(self, m, X, y=None, objective='xent', heatmap=True, **kw):
        """Front._saliency of model m (kw: method, draws, sigma, baseline, times_input)"""
        return self._saliency(m, X, y, objective, heatmap, **kw)

    def evaluate(self, Xs, ys):
        """[test error of model m over (Xs[m], ys[m])], model by model"""
        return [self._evaluate(m, Xs[m], ys[m]) for m in range(self.models)]
