"""Shared builders for the parity tests: one seeded problem, run through the CPU oracle.

Conventions the HIP path and these tests share (documented in DESIGN.md):
  * layer noise and z come from the device generator restated in oracle.device_normal, keyed by
    (seed, site, segment, sub-step) where sub-step = Keras `iterations` before the call;
  * D-step segments: 0 labeled, 1 unlabeled, 2 generated;  G-step segments: 0 generated, 1 real.
"""
import numpy as np

from oracle import mrgan_oracle as O

SEED = 0x5EED5EED


def planted(n, d, seed):
    """n rows of six planted classes (y = arange(n) % 6): class centres 2 N(0, 1), unit noise -> (X float32 [n, d], y int32)"""
    rng = np.random.default_rng(seed)
    y = (np.arange(n) % 6).astype(np.int32)
    centres = 2.0 * rng.standard_normal((6, d)).astype(np.float32)
    return centres[y] + rng.standard_normal((n, d)).astype(np.float32), y


def layer_dims(D, d_hidden=O.D_HIDDEN):
    return (D,) + tuple(d_hidden)


def noise_set(seed, seg, step, B, D, row0=0, dtype=np.float64, d_hidden=O.D_HIDDEN, normal=O.device_normal):
    """the five GaussianNoise draws of one segment; `normal` = the restated generator (tests.gaussian_noise has the other one)"""
    dims = layer_dims(D, d_hidden)
    return [normal(seed, l, seg, step, B, dims[l], row0=row0, dtype=dtype) for l in range(5)]


def draw_z(seed, step, B, row0=0, dtype=np.float64, nz=O.NOISE_SIZE, normal=O.device_normal):
    return normal(seed, O.SITE_Z, 0, step, B, nz, row0=row0, dtype=dtype)


class Case(object):
    """A reproducible training problem + its oracle trajectory.

    normal: the generator that layer noise and device-drawn z come from (the oracle and the mirror take both as inputs).
    K: a problem with K classes.  The six-class draws stay what they are (golden files and measured bounds rest on them), so
    the weights (last dense from O.init_params(K=K)) and the labels are drawn again from a stream of their own, with class 8
    and class K-1 present in every batch."""

    def __init__(self, D=16, B=50, steps=3, seed=7, noise_seed=SEED, dtype=np.float64, device_z=False,
                 d_hidden=O.D_HIDDEN, g_hidden=O.G_HIDDEN, normal=O.device_normal, K=None):
        rng = np.random.default_rng(seed)
        self.D, self.B, self.steps, self.noise_seed, self.normal = D, B, steps, noise_seed, normal
        self.d_hidden, self.g_hidden = tuple(d_hidden), tuple(g_hidden)
        g, d = O.init_params(D, seed=seed, dtype=dtype, g_hidden=self.g_hidden, d_hidden=self.d_hidden)
        # non-trivial biases / BN affine so every path carries signal
        g = [p + 0.05 * rng.standard_normal(p.shape).astype(dtype) for p in g]
        d = [p + 0.05 * rng.standard_normal(p.shape).astype(dtype) for p in d]
        self.g0, self.d0 = [p.copy() for p in g], [p.copy() for p in d]
        self.x_lab = rng.standard_normal((steps, B, D)).astype(np.float32)
        self.labels = rng.integers(0, O.NUM_CLASSES, (steps, B)).astype(np.int32)
        self.x_unl = rng.standard_normal((steps, B, D)).astype(np.float32)
        self.x_unl2 = rng.standard_normal((steps, B, D)).astype(np.float32)
        self.z1 = None if device_z else rng.standard_normal((steps, B, O.NOISE_SIZE)).astype(np.float32)
        self.z2 = None if device_z else rng.standard_normal((steps, B, O.NOISE_SIZE)).astype(np.float32)
        self.probe = rng.standard_normal((64, D)).astype(np.float32)
        self.dtype = dtype
        self.K = O.NUM_CLASSES if K is None else K
        if K is not None:
            rng = np.random.default_rng(seed + 1000 * K)
            g, d = O.init_params(D, seed=seed, dtype=dtype, g_hidden=self.g_hidden, d_hidden=self.d_hidden, K=K)
            self.g0 = [p + 0.05 * rng.standard_normal(p.shape).astype(dtype) for p in g]
            self.d0 = [p + 0.05 * rng.standard_normal(p.shape).astype(dtype) for p in d]
            self.labels = rng.integers(0, K, (steps, B)).astype(np.int32)
            self.labels[:, 0], self.labels[:, B - 1] = 8, K - 1
            assert self.d0[-2].shape[1] == K and (self.labels >= 8).any() and (self.labels == K - 1).any()

    def _draws(self, z, it, rows, row0, segs):
        """(row slice, z, one noise_set per segment) of a sub-step at Keras iteration `it`, optionally of a row shard"""
        nB = rows or self.B
        sl = slice(row0, row0 + nB)
        z = z[sl] if z is not None else draw_z(self.noise_seed, it, nB, row0, normal=self.normal)
        return sl, np.asarray(z, self.dtype), [noise_set(self.noise_seed, seg, it, nB, self.D, row0, self.dtype, self.d_hidden, self.normal)
                                               for seg in range(segs)]

    def disc_inputs(self, t, it, rows=None, row0=0):
        """numpy inputs of D sub-step t executed at Keras iteration `it` (optionally a row shard)."""
        sl, z, (n_lab, n_unl, n_fake) = self._draws(None if self.z1 is None else self.z1[t], it, rows, row0, 3)
        return dict(x_lab=self.x_lab[t][sl].astype(self.dtype), labels=self.labels[t][sl],
                    x_unl=self.x_unl[t][sl].astype(self.dtype), z=z, n_lab=n_lab, n_unl=n_unl, n_fake=n_fake)

    def gen_inputs(self, t, it, rows=None, row0=0):
        sl, z, (n_fake, n_real) = self._draws(None if self.z2 is None else self.z2[t], it, rows, row0, 2)
        return dict(x_unl=self.x_unl2[t][sl].astype(self.dtype), z=z, n_fake=n_fake, n_real=n_real)

    def run_oracle(self, mirror=False, quantize=None):
        """trajectory through the fp64 restatement, or (mirror=True) through the engine-dataflow mirror with the engine's
        storage roundings (quantize = None | 'bf16' | 'fp8')"""
        orc = O.MRGANMirror(self.g0, self.d0, quantize=quantize) if mirror else O.MRGANOracle(self.g0, self.d0)
        out = dict(disc=[], gen=[], logits0=orc.predict_logits(self.probe.astype(self.dtype)))
        for t in range(self.steps):
            out['disc'].append(orc.disc_step(**self.disc_inputs(t, orc.adam.iterations)))
            out['gen'].append(orc.gen_step(**self.gen_inputs(t, orc.adam.iterations)))
        out['logits'] = orc.predict_logits(self.probe.astype(self.dtype))
        out['g'], out['d'] = orc.g, orc.d
        out['oracle'] = orc
        return out


def rel_err(a, ref):
    """scale-relative error: max |a - ref| / max |ref|"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(a - ref)) / (np.max(np.abs(ref)) + 1e-300))


def update_rel_err(w, w_ref, w0):
    """error of a weight tensor relative to the size of the update that produced it"""
    w, w_ref, w0 = [np.asarray(x, np.float64) for x in (w, w_ref, w0)]
    return float(np.linalg.norm(w - w_ref) / (np.linalg.norm(w_ref - w0) + 1e-300))


def frob_rel_err(a, ref):
    """Frobenius-relative error ||a - ref|| / ||ref||"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(a - ref) / (np.linalg.norm(ref) + 1e-300))


def cosine(a, ref):
    a, ref = np.asarray(a, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    return float(a @ ref / (np.linalg.norm(a) * np.linalg.norm(ref) + 1e-300))


# ---------------------------------------------------------------------------------------------------------
# layouts the GEMM epilogues write (csrc/gemm.h), restated for the kernel-level tests
# ---------------------------------------------------------------------------------------------------------
def _mask_pos(rows):
    """row -> (32-row block, lane half, bit) of the lane-native relu mask: a 32x32 accumulator holds row
    (r & 3) + 8 (r >> 2) + 4 half in register r, and bit r of the word of (block, column, half) is that element"""
    rows = np.asarray(rows)
    rr = rows & 31
    return rows >> 5, (rr >> 2) & 1, (rr & 3) | ((rr >> 3) << 2)


def mask_decode(words, m, n):
    """uint16 words [ceil(m / 32) or more][ldm][2] -> bool [m][n]"""
    words = np.asarray(words)
    blk, half, bit = _mask_pos(np.arange(m))
    w = words[blk[:, None], np.arange(n)[None, :], half[:, None]].astype(np.uint32)
    return ((w >> bit[:, None].astype(np.uint32)) & 1).astype(bool)


def mask_encode(bits, ldm):
    """bool [m][n] -> uint16 words [ceil(m / 32)][ldm][2], zero where no element of `bits` lives"""
    bits = np.asarray(bits, dtype=bool)
    m, n = bits.shape
    blk, half, bit = _mask_pos(np.arange(m))
    words = np.zeros(((m + 31) // 32, ldm, 2), dtype=np.uint32)
    np.bitwise_or.at(words, (blk[:, None], np.arange(n)[None, :], half[:, None]), bits.astype(np.uint32) << bit[:, None].astype(np.uint32))
    return words.astype(np.uint16)


def colsum_rows(m, nbatch):
    """partial-sum row of every (batch, row): the sums have a fixed granularity of 64 rows, [batch * tiles_m + row / 64][ldcs]
    with tiles_m = ceil(m / 64) -> (tiles_m, int array [nbatch][m])"""
    tiles_m = (m + 63) // 64
    return tiles_m, np.arange(nbatch)[:, None] * tiles_m + (np.arange(m) // 64)[None, :]


def colsum_groups(v):
    """[nbatch][m][n] -> the column sums over 64-row groups in the layout above, [nbatch * tiles_m][n] (same dtype)"""
    v = np.asarray(v)
    nbatch, m, n = v.shape
    tiles_m, prow = colsum_rows(m, nbatch)
    out = np.zeros((nbatch * tiles_m, n), dtype=v.dtype)
    np.add.at(out, prow.ravel(), v.reshape(nbatch * m, n))
    return out


# ---------------------------------------------------------------------------------------------------------
# pieces the kernel-level test files share (test_gemm_kernels.py, test_fp8_kernels.py).  torch is imported inside them: this
# module is also loaded by worker processes that must stay numpy-only (oracle_fit_job)
# ---------------------------------------------------------------------------------------------------------
DEV = "cuda:0"
SENT = -768.0                    # sentinel of every output buffer: exact in bf16, far outside the value range


def _rng(*key):
    return np.random.default_rng([int(k) & 0xFFFFFFFF for k in key])


def _embed(x, rows, ld, dtype, fill=float("nan")):
    """[nb][m][n] -> buffer [nb][rows][ld] of `dtype`, everything outside [m][n] holding `fill`"""
    import torch
    nb, m, n = x.shape
    t = torch.full((nb, rows, ld), fill, dtype=dtype, device=DEV)
    t[:, :m, :n] = x.to(dtype)
    return t


def _usage(err, bound):
    """largest err / bound and where (0 / 0 = 0, x / 0 = inf, NaN = inf)"""
    import torch
    inf = torch.full_like(err, float("inf"))
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, inf, torch.zeros_like(err)))
    ratio = torch.where(torch.isnan(err), inf, ratio)
    i = int(torch.argmax(ratio))
    return float(ratio.reshape(-1)[i]), tuple(int(v) for v in np.unravel_index(i, tuple(ratio.shape)))


def _assert_close(label, got, ref, bound, acc_bound=None):
    err = (got - ref).abs()
    use, at = _usage(err, bound)
    msg = "%s: usage %.3f at %s (got %r want %r bound %.3g)" % (label, use, at, float(got[at]), float(ref[at]), float(bound[at]))
    if acc_bound is not None:
        msg += " | accumulation term used %.4f" % _usage(err, acc_bound)[0]
    print(msg)
    assert use <= 1.0, msg
    return use


def _assert_sentinel(label, buf, inside, value=SENT):
    """every element of `buf` outside the boolean region `inside` still holds the sentinel"""
    import torch
    bad = (buf != value) & ~inside
    if bool(bad.any()):
        at = tuple(int(v[0]) for v in torch.nonzero(bad, as_tuple=True))
        raise AssertionError("%s: sentinel overwritten at %s (%d elements), holds %r" % (label, at, int(bad.sum()), float(buf[at])))


def oracle_logmel(contacts, sr=48000, n_mels=128):
    """CPU stand-in for the GPU front end of dataset() (the suite runs without a GPU; tests/test_gpu_parity.py holds the HIP
    kernel to it)"""
    from oracle.melspec_oracle import log_melspectrogram
    return [log_melspectrogram(np.asarray(c, dtype=np.float64), sr=sr, n_mels=n_mels).astype(np.float32).flatten() for c in contacts]


def write_fake_mreo(tmp, ft=4, cm=0.2, objects=2, trials=3):
    """a synthetic MREO-format pickle per material under `tmp` (processdata.py:23-34)"""
    import os
    import pickle
    from mr_gan_amd.data import MATERIALS
    rng = np.random.default_rng(0)
    for m, material in enumerate(MATERIALS):
        allData = {}
        for o in range(objects):
            d = {k: [] for k in ('forceTime', 'force0', 'force1', 'pressureTime', 'pressure0', 'pressure1',
                                 'temperatureTime', 'temperature', 'contactTime', 'contact')}
            for t in range(trials):
                n = int(100 * ft)
                d['force0'].append((rng.standard_normal(n) + 10 * m).tolist())
                d['force1'].append((rng.standard_normal(n) + 20 * m).tolist())
                d['temperature'].append((rng.standard_normal(n) + 30 * m).tolist())
                d['contact'].append(rng.standard_normal(int(48000 * cm)).tolist())
            allData['%s_obj%d' % (material, o)] = d
        with open(os.path.join(tmp, 'processed_0.1sbefore_%s_times_%.2f_%.2f.pkl' % (material, ft, cm)), 'wb') as f:
            pickle.dump(allData, f, 2)          # protocol 2 = what Python-2 cPickle.HIGHEST_PROTOCOL wrote


def stub_training(job, datasets, device):
    """CPU stand-in for scheduler.train_job: a deterministic 'test error' from the job's rows (and the worker's pid, so
    tests can see that several processes took part)."""
    import os
    X, y = datasets[job['dataset']]
    tr, te = job['train_idx'], job['test_idx']
    val = float(np.mean(X[tr]) - np.mean(X[te]) + 0.01 * job.get('percentlabeled', 0) + np.mean(y[te]))
    if job.get('explode'):
        raise ValueError("stub failure requested")
    if job.get('sleep'):
        import time
        time.sleep(job['sleep'])
    return (val, os.getpid(), device)


def oracle_fit(g0, d0, x_labeled, y_labeled, x_train, x_test, y_test, batch, epochs, seed, rng_seed, dtype=np.float32, quantize=None, log=None):
    """The epoch loop of mr_gan.py:183-230 through the CPU oracle, driven by the SAME streams as MRGAN.fit on the engine:
    index streams from `rng` in the order MRGAN._fit draws them (mr_gan.py:189-195), z and layer noise from the restated
    device generator keyed by (seed, site, segment, Keras iteration).  Returns the final whole-test-set error (mr_gan.py:230)."""
    from threadpoolctl import threadpool_limits
    # batch-50 products: OpenBLAS with many threads is pathologically slow on them (X^T dY at 50 x 1200 x 1000: 19 ms with 8
    # threads, 0.5 ms with 4), so the loop runs on 4 BLAS threads
    with threadpool_limits(limits=4):
        return _oracle_fit(g0, d0, x_labeled, y_labeled, x_train, x_test, y_test, batch, epochs, seed, np.random.RandomState(rng_seed), dtype,
                           quantize, log)


def _oracle_fit(g0, d0, x_labeled, y_labeled, x_train, x_test, y_test, batch, epochs, seed, rng, dtype, quantize, log):
    orc = O.MRGANMirror(g0, d0, quantize=quantize) if quantize else O.MRGANOracle([p.astype(dtype) for p in g0], [p.astype(dtype) for p in d0])
    xl, xu = x_labeled.astype(dtype), x_train.astype(dtype)
    yl = np.asarray(y_labeled).astype(np.int64)
    n_train, n_lab, D = xu.shape[0], xl.shape[0], xu.shape[1]
    nb = n_train // batch
    it = 0
    for epoch in range(epochs):
        inds = O.tiled_permutation(rng.permutation, n_lab, n_train)
        unl = [rng.permutation(n_train) for _ in range(3)]
        for t in range(nb):
            sl = slice(t * batch, (t + 1) * batch)
            ns = lambda seg, k: noise_set(seed, seg, k, batch, D, 0, dtype)
            orc.disc_step(xl[inds[sl]], yl[inds[sl]], xu[unl[0][sl]], draw_z(seed, it, batch, dtype=dtype), ns(0, it), ns(1, it), ns(2, it))
            orc.gen_step(xu[unl[1][sl]], draw_z(seed, it + 1, batch, dtype=dtype), ns(0, it + 1), ns(1, it + 1))
            it += 2
        if log is not None:
            log.append(float(orc.test_error(x_test.astype(dtype), y_test)))
    return float(orc.test_error(x_test.astype(dtype), y_test))


def oracle_fit_job(kw):
    """oracle_fit in a worker process (multiprocessing 'spawn'): the worker imports numpy only -- with torch's and
    scikit-learn's OpenMP pools loaded beside OpenBLAS these batch-50 products run ~80x slower (120 ms per forward, measured)."""
    log = []
    err = oracle_fit(log=log, **kw)
    return err, log


def run_oracle_fits(jobs, workers=2):
    """[kwargs of oracle_fit] -> [(final error, per-epoch errors)], each in a clean worker process with 4 BLAS threads"""
    import multiprocessing as mp
    import os
    old = {k: os.environ.get(k) for k in ("OPENBLAS_NUM_THREADS", "OMP_NUM_THREADS")}
    os.environ["OPENBLAS_NUM_THREADS"] = "4"
    os.environ["OMP_NUM_THREADS"] = "4"
    try:
        with mp.get_context("spawn").Pool(min(workers, len(jobs))) as pool:
            asyncs = [pool.apply_async(oracle_fit_job, (j,)) for j in jobs]
            return asyncs, pool, [a.get(timeout=600) for a in asyncs]
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
