"""Keras-shaped front end of the HIP training path.

The reference script exposes no class -- its model lives in local variables of mr_gan()
(mr_gan.py:109-171).  The fit / evaluate / predict shape mirrors how the same authors drive Keras
models elsewhere in the repository (mr_nn.py:117-118, others/mr_gan_autoencoder.py:125-139).
"""
import sys
import time

import numpy as np
import torch

from mr_gan_amd import engine as E
from mr_gan_amd.data import tiled_permutation


# the per-epoch line of mr_gan.py:227
EPOCH_LINE = 'Epoch %d, time = %ds, loss labeled = %.4f, loss unlabeled = %.4f, train error = %.4f, test error = %.4f'


def glorot_uniform(rng, fan_in, fan_out):
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, size=(fan_in, fan_out)).astype(np.float32)


DTYPES = {'float32': E.F32, 'fp32': E.F32, 'bfloat16': E.BF16, 'bf16': E.BF16, 'fp8': E.FP8, 'float8': E.FP8}


def gan_config(input_dim, batch_size, dtype, seed, num_classes, noise_size, g_hidden, d_hidden, lr, beta_1, unlabeled_weight,
               use_graph, flags, noise, models=0, rank=0, world=1):
    """the mrgan_config of MRGAN (models = 0) and MRGANGroup (model m draws what a handle with seed + m draws)"""
    cfg = E.default_config(input_dim, batch_size)
    cfg.dtype = DTYPES[dtype]
    cfg.num_classes, cfg.noise_size = num_classes, noise_size
    cfg.g_hidden[0], cfg.g_hidden[1] = g_hidden
    for i, w in enumerate(d_hidden):
        cfg.d_hidden[i] = w
    cfg.lr, cfg.beta1, cfg.unlabeled_weight = lr, beta_1, unlabeled_weight
    cfg.seed = seed
    cfg.rank, cfg.world = rank, world
    if models:
        cfg.models = models
    cfg.flags = flags | (E.FLAG_GRAPH if use_graph else 0) | E.noise_flags(noise)
    return cfg


def epoch_streams(rng, n_lab, n_train, n_pool=None):
    """One epoch's index streams, drawn from rng in the reference's order (the draws and their order are part of the results):
    the labelled tiling (mr_gan.py:189), then three unlabelled permutations (:193-195; the third is unused) or, with a table-6
    pool of n_pool rows, three tilings of it (:197-202) -> (inds, [unl, unl2, unused])"""
    inds = tiled_permutation(rng, n_lab, n_train)
    if n_pool is None:
        return inds, [rng.permutation(n_train).astype(np.int32) for _ in range(3)]
    return inds, [tiled_permutation(rng, n_pool, n_train) for _ in range(3)]


class MRGAN(object):
    """Feature-matching semi-supervised GAN of mr_gan.py on one MI355X.

    dtype: 'float32' (fp32 MFMA: logits within 1e-3 of the reference arithmetic) or 'bfloat16'
    (bf16 MFMA, fp32 accumulate and fp32 master weights: the throughput mode).
    noise: 'irwin-hall' (default) or 'gaussian': the generator of the five GaussianNoise sites and of the device-drawn z
    (engine.noise_flags); 'gaussian' draws true normals as the reference's K.random_normal does, at a slower step.
    """

    def __init__(self, input_dim, batch_size=50, dtype='float32', seed=None, device='cuda:0', num_classes=6,
                 noise_size=100, g_hidden=(500, 500), d_hidden=(1000, 500, 250, 250, 250), lr=0.0006, beta_1=0.5,
                 unlabeled_weight=1.0, use_graph=True, rank=0, world=1, flags=0, init_weights=True, noise='irwin-hall'):
        self.input_dim = int(input_dim)
        self.batch_size = int(batch_size)
        self.seed = int(np.random.randint(1 << 31)) if seed is None else int(seed)   # mr_gan.py:75 is unseeded
        self.cfg = gan_config(self.input_dim, self.batch_size, dtype, self.seed, num_classes, noise_size, g_hidden, d_hidden, lr, beta_1,
                              unlabeled_weight, use_graph, flags, noise, rank=rank, world=world)
        self.engine = E.Engine(self.cfg, device)
        self.device = self.engine.device
        # a private HIP stream: graph capture is not permitted on the legacy default stream
        self.stream = torch.cuda.Stream(self.device)
        self.iterations = 0
        self.history = []
        if init_weights:
            self.initialize(self.seed)

    # ---- weights ---------------------------------------------------------------------------------------
    def initialize(self, seed):
        """Keras defaults: Dense kernels glorot_uniform, biases zero, BN gamma one / beta zero."""
        rng = np.random.RandomState(seed)
        for net in (E.NET_G, E.NET_D):
            ws = []
            for i in range(self.engine.num_tensors(net)):
                shp = self.engine.full_shape(net, i)
                if len(shp) == 2:
                    ws.append(glorot_uniform(rng, shp[0], shp[1]))
                elif net == E.NET_G and i == 2:
                    ws.append(np.ones(shp, np.float32))
                else:
                    ws.append(np.zeros(shp, np.float32))
            self.engine.set_weights(net, ws)

    def get_weights(self, net='discriminator'):
        return self.engine.get_weights(E.NET_D if net.startswith('d') else E.NET_G)

    def set_weights(self, weights, net='discriminator'):
        self.engine.set_weights(E.NET_D if net.startswith('d') else E.NET_G, weights)

    # ---- the three compiled functions (mr_gan.py:169-171) on host arrays --------------------------------------
    def _dev(self, a, dtype=torch.float32):
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dtype).contiguous()
        return torch.from_numpy(np.ascontiguousarray(a)).to(device=self.device, dtype=dtype).contiguous()

    def _on_stream(self):
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        return torch.cuda.stream(self.stream)

    def train_batch_disc(self, x_lab, labels, x_unl, noise=None):
        with self._on_stream():
            return self._train_batch_disc(x_lab, labels, x_unl, noise)

    def train_batch_gen(self, x_unl, noise=None):
        with self._on_stream():
            return self._train_batch_gen(x_unl, noise)

    def test_batch(self, x, labels):
        with self._on_stream():
            return self.engine.eval_error(self._dev(x), self._dev(labels, torch.int32))

    def fit(self, *args, **kwargs):
        with self._on_stream():
            return self._fit(*args, **kwargs)

    def predict_logits(self, X):
        with self._on_stream():
            return self.engine.predict_logits(self._dev(X)).cpu().numpy()

    def saliency(self, X, y=None, objective='xent', heatmap=True, method='gradient', draws=None, sigma=None, baseline=None,
                 times_input=False):
        """Saliency maps of the discriminator (the reference's others/mr_nn_activation_map.py): per row of X the gradient of
        `objective` -- 'xent' (the labelled loss term), 'logit' (the class score) or 'mse' -- at class y[i], or at the
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
        code = E.saliency_objective(objective)                     # (checked before anything touches the device)
        plan = E.attribution_plan(method, draws, sigma, baseline, times_input, d_in=self.input_dim,
                                  own_sigmas=(float(self.engine.cfg.sigma[0]), float(self.engine.cfg.sigma[1])))
        post = E.SAL_HEATMAP if heatmap else E.SAL_RAW
        with self._on_stream():
            x, t = self._dev(X), None if y is None else self._dev(y, torch.int32)
            if plan['baseline'] is not None:
                plan['baseline'] = self._dev(plan['baseline'])
            maps, cls = self.engine.attribution(x, t, code, post, **plan)
            return maps.cpu().numpy(), cls.cpu().numpy()

    def evaluate(self, X, y):
        """test_batch([0, X, y]) over the whole set (mr_gan.py:230) -> error rate."""
        with self._on_stream():
            return self.engine.eval_error(self._dev(X), self._dev(y, torch.int32))

    def _train_batch_disc(self, x_lab, labels, x_unl, noise=None):
        a = E.Engine.disc_args(self._dev(x_lab), self._dev(labels, torch.int32), self._dev(x_unl),
                               None if noise is None else self._dev(noise))
        self._hold = a
        self.iterations += 1
        return self.engine.disc_step(a)

    def _train_batch_gen(self, x_unl, noise=None):
        a = E.Engine.gen_args(self._dev(x_unl), None if noise is None else self._dev(noise))
        self.iterations += 1
        return self.engine.gen_step(a)

    # ---- Keras-shaped API ---------------------------------------------------------------------------------------
    def _fit(self, x_labeled, y_labeled, x_unlabeled, epochs=100, batch_size=None, verbose=0, validation_data=None,
            x_unlabeled_pool=None, rng=None, z_source='device'):
        """The epoch loop of mr_gan.py:183-228.

        x_labeled / y_labeled: the class-sorted labeled subset (mr_gan.py:102-103);
        x_unlabeled: X_train (every training row is used as unlabeled data, mr_gan.py:193-194);
        x_unlabeled_pool: table-6 restricted pool (mr_gan.py:197-202), else None.
        The matrices are uploaded once and stay resident in HBM; per epoch only the permutation index
        streams (mr_gan.py:189-195) go to the device, and the per-batch scalars are accumulated on the
        device and read back once per epoch.
        z_source: 'device' draws the generator input on the GPU (the engine's counter-based generator);
        'host' draws it as the reference does, np.random.normal(0, 1, [B, noise]) twice per iteration (mr_gan.py:206, :212),
        from `rng`, and uploads one epoch's worth at a time."""
        if batch_size is not None and batch_size != self.batch_size:
            raise ValueError("batch_size is fixed at construction (%d)" % self.batch_size)
        rng = rng or np.random.RandomState(self.seed ^ 0x5bd1e995)
        B = self.batch_size
        xl = self._dev(x_labeled)
        xu = self._dev(x_unlabeled)
        yl = np.asarray(y_labeled).astype(np.int32)
        pool = self._dev(x_unlabeled_pool) if x_unlabeled_pool is not None else None
        n_train, n_lab = xu.shape[0], xl.shape[0]
        nb = n_train // B                                          # mr_gan.py:173 (remainder rows dropped)
        if nb < 1:
            raise ValueError("fewer training rows (%d) than one batch (%d)" % (n_train, B))
        xt = yt = None
        if validation_data is not None:
            xt, yt = self._dev(validation_data[0]), self._dev(validation_data[1], torch.int32)
        for epoch in range(1, epochs + 1):
            begin = time.time()
            inds, unl = epoch_streams(rng, n_lab, n_train, None if pool is None else pool.shape[0])
            unl_src = xu if pool is None else pool
            idx_lab = self._dev(inds, torch.int32)
            lab_stream = self._dev(yl[inds], torch.int32)
            idx_unl = self._dev(unl[0], torch.int32)
            idx_unl2 = self._dev(unl[1], torch.int32)
            z1 = z2 = None
            if z_source == 'host':
                zz = rng.normal(0.0, 1.0, size=(nb, 2, B, self.cfg.noise_size)).astype(np.float32)       # :206 then :212, per iteration
                z1, z2 = self._dev(zz[:, 0].reshape(nb * B, -1)), self._dev(zz[:, 1].reshape(nb * B, -1))
            elif z_source != 'device':
                raise ValueError("z_source must be 'device' or 'host'")
            dargs = E.Engine.disc_args(xl, lab_stream, unl_src, z1, idx_lab, idx_unl, stream_mode=1)
            gargs = E.Engine.gen_args(unl_src, z2, idx_unl2, stream_mode=1)
            self.engine.set_iterations(self.iterations, 0)
            for _ in range(nb):                                    # mr_gan.py:204-213
                self.engine.train_pair(dargs, gargs)
            self.iterations += 2 * nb
            m = self.engine.read_metrics(reset=True)               # one sync per epoch
            loss_lab, loss_unl, train_err, loss_gen = [v / nb for v in m[:4]]
            test_err = float('nan')
            if xt is not None:
                nte = (xt.shape[0] // B) * B                       # mr_gan.py:221-223: mean over whole test batches
                if nte > 0:
                    test_err = self.engine.eval_error(xt[:nte], yt[:nte])
            rec = dict(epoch=epoch, time=time.time() - begin, loss_lab=loss_lab, loss_unl=loss_unl, train_err=train_err,
                       loss_gen=loss_gen, test_err=test_err)
            self.history.append(rec)
            if verbose:
                # mr_gan.py:227
                print(EPOCH_LINE % (epoch, rec['time'], loss_lab, loss_unl, train_err, test_err))
                sys.stdout.flush()
        return self.history

    def predict(self, X):
        return np.argmax(self.predict_logits(X), axis=1)


class MRGANGroup(object):
    """`models` MRGAN trainings of one shape on one group handle (mrgan_config.models): model m is MRGAN(seed=seed + m) -- the
    same glorot streams for G and D, engine seed seed + m -- and every (D, G) pair of all models is one train_pair_group (one
    launch set per sub-step).  The results are those of the `models` single MRGAN runs bit for bit."""

    def __init__(self, input_dim, models, batch_size=50, dtype='float32', seed=None, device='cuda:0', num_classes=6,
                 noise_size=100, g_hidden=(500, 500), d_hidden=(1000, 500, 250, 250, 250), lr=0.0006, beta_1=0.5,
                 unlabeled_weight=1.0, use_graph=True, flags=0, init_weights=True, noise='irwin-hall'):
        self.input_dim, self.batch_size, self.models = int(input_dim), int(batch_size), int(models)
        if not 2 <= self.models <= E.MAX_MODELS:
            raise ValueError("a model group has 2 .. %d models, got %d (one model: MRGAN)" % (E.MAX_MODELS, self.models))
        if dtype in ('fp8', 'float8'):
            raise ValueError("a model group cannot be an fp8 handle")
        self.seed = int(np.random.randint(1 << 31)) if seed is None else int(seed)
        self.cfg = gan_config(self.input_dim, self.batch_size, dtype, self.seed, num_classes, noise_size, g_hidden, d_hidden, lr, beta_1,
                              unlabeled_weight, use_graph, flags, noise, models=self.models)
        self.engine = E.Engine(self.cfg, device)
        self.device = self.engine.device
        self.stream = torch.cuda.Stream(self.device)               # (graph capture is not permitted on the legacy default stream)
        self.iterations = 0
        self.history = []
        if init_weights:
            for m in range(self.models):
                self.engine.select_model(m)
                MRGAN.initialize(self, self.seed + m)
            self.engine.select_model(0)

    _dev = MRGAN._dev
    _on_stream = MRGAN._on_stream

    def fit(self, x_labeled, y_labeled, x_unlabeled, epochs=100, verbose=0, validation_data=None, x_unlabeled_pools=None, rngs=None):
        """MRGAN.fit (z drawn on the device) of every model at once.  x_labeled / y_labeled / x_unlabeled: `models` arrays each,
        of equal length across the models; validation_data: `models` (X, y) pairs, or None; x_unlabeled_pools: `models` table-6
        pools of equal length, or None.  Model m's permutation streams come from rngs[m] (default: MRGAN.fit's default for
        seed + m).  The matrices stay resident as [models][n][D]; one train_pair_group per batch, metrics per model once per epoch."""
        with self._on_stream():
            return self._fit(x_labeled, y_labeled, x_unlabeled, epochs, verbose, validation_data, x_unlabeled_pools, rngs)

    def _fit(self, x_labeled, y_labeled, x_unlabeled, epochs, verbose, validation_data, pools, rngs):
        G, B = self.models, self.batch_size
        groups = [x_labeled, y_labeled, x_unlabeled] + ([pools] if pools is not None else [])
        if any(len(g) != G for g in groups) or any(len({len(a) for a in g}) != 1 for g in groups) or len(x_labeled[0]) != len(y_labeled[0]):
            raise ValueError("fit: a group trains %d sets of equal length" % G)
        if validation_data is not None and len(validation_data) != G:
            raise ValueError("fit: validation_data is one (X, y) pair per model")
        rngs = rngs or [np.random.RandomState((self.seed + m) ^ 0x5bd1e995) for m in range(G)]
        xl = torch.stack([self._dev(x) for x in x_labeled])
        xu = torch.stack([self._dev(x) for x in x_unlabeled])
        yl = [np.asarray(y).astype(np.int32) for y in y_labeled]
        pool = torch.stack([self._dev(p) for p in pools]) if pools is not None else None
        n_train, n_lab = xu.shape[1], xl.shape[1]
        nb = n_train // B                                          # mr_gan.py:173 (remainder rows dropped)
        if nb < 1:
            raise ValueError("fewer training rows (%d) than one batch (%d)" % (n_train, B))
        val = None
        if validation_data is not None:
            val = [(self._dev(v[0]), self._dev(v[1], torch.int32)) for v in validation_data]
        unl_src = xu if pool is None else pool
        for epoch in range(1, epochs + 1):
            begin = time.time()
            # model m: the draws of MRGAN._fit, from rngs[m]
            inds, unl = zip(*[epoch_streams(rngs[m], n_lab, n_train, None if pool is None else pool.shape[1]) for m in range(G)])
            idx_lab = self._dev(np.stack(inds), torch.int32)
            lab_stream = self._dev(np.stack([yl[m][inds[m]] for m in range(G)]), torch.int32)
            idx_unl = self._dev(np.stack([u[0] for u in unl]), torch.int32)
            idx_unl2 = self._dev(np.stack([u[1] for u in unl]), torch.int32)
            dargs = E.Engine.disc_group_args(xl, lab_stream, unl_src, None, idx_lab, idx_unl, stream_mode=1)
            gargs = E.Engine.gen_group_args(unl_src, None, idx_unl2, stream_mode=1)
            self.engine.set_iterations(self.iterations, 0)
            for _ in range(nb):                                    # mr_gan.py:204-213
                self.engine.train_pair_group(dargs, gargs)
            self.iterations += 2 * nb
            rec = dict(epoch=epoch, loss_lab=[], loss_unl=[], train_err=[], loss_gen=[], test_err=[])
            for m in range(G):                                     # metrics and evaluation: model by model
                self.engine.select_model(m)
                met = self.engine.read_metrics(reset=True)
                for k, v in zip(('loss_lab', 'loss_unl', 'train_err', 'loss_gen'), met[:4]):
                    rec[k].append(v / nb)
                test_err = float('nan')
                if val is not None:
                    nte = (val[m][0].shape[0] // B) * B            # mr_gan.py:221-223: mean over whole test batches
                    if nte > 0:
                        test_err = self.engine.eval_error(val[m][0][:nte], val[m][1][:nte])
                rec['test_err'].append(test_err)
            self.engine.select_model(0)
            rec['time'] = time.time() - begin
            self.history.append(rec)
            if verbose:
                for m in range(G):                                 # mr_gan.py:227, once per model
                    print(('Model %d: ' % m) + EPOCH_LINE % (epoch, rec['time'], rec['loss_lab'][m], rec['loss_unl'][m], rec['train_err'][m],
                                                             rec['test_err'][m]))
                sys.stdout.flush()
        return self.history

    def predict_logits(self, m, X):
        with self._on_stream():
            self.engine.select_model(m)
            return self.engine.predict_logits(self._dev(X)).cpu().numpy()

    def saliency(self, m, X, y=None, objective='xent', heatmap=True, **kw):
        """MRGAN.saliency of model m (kw: method, draws, sigma, baseline, times_input)"""
        E.saliency_objective(objective)                            # (unknown ones are refused before the selection moves)
        E.attribution_plan(kw.get('method', 'gradient'), kw.get('draws'), kw.get('sigma'), kw.get('baseline'),
                           kw.get('times_input', False), d_in=self.input_dim)
        self.engine.select_model(m)
        return MRGAN.saliency(self, X, y, objective, heatmap, **kw)

    def evaluate(self, Xs, ys):
        """[test error of model m over (Xs[m], ys[m])], model by model"""
        errs = []
        with self._on_stream():
            for m in range(self.models):
                self.engine.select_model(m)
                errs.append(self.engine.eval_error(self._dev(Xs[m]), self._dev(ys[m], torch.int32)))
        return errs
