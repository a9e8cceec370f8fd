"""Autoencoder pre-stage of the reference (others/mr_gan_autoencoder.py:109-140) on the HIP engine: the dimensionality
reduction of the raw contact-microphone vector.  A dense autoencoder D -> n0 -> n1 -> n2 -> n1 -> n0 -> D (relu x 5, linear
output) is fitted with loss = 'mse' and Keras' default Adam at batch 32; encoder.predict then replaces X_train / X_test and the
unchanged GAN trains on the n2-wide codes.

With the reference's three encoderNodes this is the six-layer dense stack the engine already runs as its discriminator; a
handle created with FLAG_AUTOENCODER stores the last layer at full width and trains through mrgan_ae_step
(include/mrgan_abi.h): the stage / dense / dX / dW / Adam kernels of the supervised step with the reconstruction head.  There
is no CPU path."""
import ctypes as C

import numpy as np

from mr_gan_amd import engine as E
from mr_gan_amd.data import prologue, resolve_num_classes, train_test_sets
from mr_gan_amd import model as M
from mr_gan_amd.model import MRGAN, Front
from mr_gan_amd.mr_gan import _run_lines, _test_error_line, print_lines

AE_LR, AE_BETA_1 = 0.001, 0.9              # Keras-2.0.9 Adam defaults (others/mr_gan_autoencoder.py:123 optimizer='adam')


def encoder_widths(encoder_nodes):
    """the five hidden widths n0 n1 n2 n1 n0 of others/mr_gan_autoencoder.py:110-118 for three encoder nodes"""
    nodes = [int(n) for n in encoder_nodes]
    if len(nodes) != 3:
        raise ValueError("encoder_nodes must have length 3, got %d: the engine's dense stack has six layers "
                         "(D -> n0 -> n1 -> n2 -> n1 -> n0 -> D)" % len(nodes))
    return (nodes[0], nodes[1], nodes[2], nodes[1], nodes[0])


class Autoencoder(Front):
    """autoencoder / encoder of others/mr_gan_autoencoder.py:109-127 on one MI355X: compile(loss='mse', optimizer='adam'),
    fit(X, X), encoder.predict.  dtype: 'float32' or 'bfloat16'."""

    nets = (E.NET_D,)

    def __init__(self, d_in, encoder_nodes=(128, 64, 16), batch_size=32, dtype='float32', seed=None, device='cuda:0',
                 lr=AE_LR, beta_1=AE_BETA_1, init_weights=True):
        widths = encoder_widths(encoder_nodes)                     # (checked before anything touches the device)
        self.code_dim = widths[2]
        Front.__init__(self, d_in, batch_size, dtype, seed, device, 'irwin-hall', init_weights, widths, fp8=False,
                       flags=E.FLAG_AUTOENCODER, sigma=(C.c_float * 5)(), lr=lr, beta1=beta_1)

    def get_weights(self):
        return self.engine.get_weights(E.NET_D)

    def set_weights(self, weights):
        self.engine.set_weights(E.NET_D, weights)

    def train_on_batch(self, x):
        """one batch of at most batch_size rows -> its mse"""
        import torch
        B, n = self.batch_size, len(x)
        with self._on_stream():
            xb = torch.zeros((B, self.input_dim), device=self.device)
            xb[:n] = self._dev(x)
            self._hold = a = E.Engine.ae_args(xb, rows_valid=0 if n == B else n)
            return self.engine.ae_step(a)

    def fit(self, X, epochs=100, validation_data=None, rng=None, verbose=0):
        """Keras fit(X, X, batch_size, shuffle=True): model.ae_epochs; rng: the source of the permutations (default
        RandomState(seed)); validation_data: rows whose mse is each epoch's val_loss -> history (loss, val_loss per epoch)"""
        with self._on_stream():
            M.ae_epochs(self.engine, self._dev, X, rng or np.random.RandomState(self.seed), epochs, self.history, validation_data, verbose)
            self.stream.synchronize()
        return self.history

    def encode(self, X):
        """encoder.predict(X) -> codes [n, n2] float32"""
        with self._on_stream():
            return self.engine.ae_encode(self._dev(X)).cpu().numpy()

    def reconstruct(self, X):
        """autoencoder.predict(X) -> [n, D] float32"""
        with self._on_stream():
            return self.engine.ae_reconstruct(self._dev(X), want_mse=False)[0].cpu().numpy()

    def evaluate(self, X):
        """autoencoder.evaluate(X, X) -> mse over all elements"""
        with self._on_stream():
            return self.engine.ae_reconstruct(self._dev(X), want_out=False)[1]


def gan_on_codes(make_codes, X, y, percentlabeled, percentunlabeled, epochs, trainTestSets, verbose, batch_size, dtype, seed, device, noise,
                 num_classes):
    """what mr_gan_autoencoder and mr_gan_pca (pca.py) share: split and standard-scale (the scaler fitted on the training rows),
    replace both sets by make_codes(X_train, X_test, rs) -> (codes of X_train, codes of X_test), not rescaled, print their
    shapes, then the unchanged GAN training of mr_gan() on the codes -> the test ACCURACY over the whole test set"""
    rs = np.random.RandomState(seed if seed is not None else np.random.randint(1 << 31))
    num_classes = resolve_num_classes(num_classes)
    sets = train_test_sets(X, y, trainTestSets, rs, num_classes)

    def codes(X_train, X_test):
        out = make_codes(X_train, X_test, rs)
        print_lines([(np.shape(out[0]), np.shape(out[1]))], verbose)
        return out
    x_labeled, y_labeled, x_unlabeled, X_train, X_test, y_test, lines = prologue(sets, percentlabeled, percentunlabeled, rs, num_classes,
                                                                                 transform=codes)
    print_lines(_run_lines(lines, epochs, batch_size, X_train, X_test), verbose)
    model = MRGAN(X_train.shape[1], batch_size=batch_size, dtype=dtype, seed=int(rs.randint(1 << 31)), device=device, noise=noise,
                  num_classes=num_classes)
    hist = model.fit(x_labeled, y_labeled, X_train, epochs=epochs, verbose=1 if verbose else 0,
                     validation_data=(X_test, y_test), x_unlabeled_pool=x_unlabeled, rng=rs)
    testerror = model.evaluate(X_test, y_test)
    print_lines(_test_error_line(testerror, [rec['test_err'] for rec in hist]), verbose)
    model.close()
    return 1.0 - testerror


def mr_gan_autoencoder(X, y, percentlabeled=50, percentunlabeled=None, epochs=100, trainTestSets=None, encoderNodes=(128, 64, 16),
                       ae_epochs=100, verbose=False, batch_size=50, ae_batch_size=32, dtype='float32', seed=None, device='cuda:0',
                       noise='irwin-hall', num_classes=None):
    """mr_gan() of others/mr_gan_autoencoder.py: split and standard-scale (the scaler fitted on the training rows), fit the
    autoencoder on X_train for ae_epochs epochs at batch ae_batch_size with X_test as validation data, replace both sets by
    their codes (not rescaled: the reference does not), then the unchanged GAN training of mr_gan() on the codes.
    Returns the test ACCURACY over the whole test set, as the reference's function does (others/mr_gan_autoencoder.py:212,
    :285) -- mr_gan() returns the test error."""
    E.noise_flags(noise)                                           # an unknown value fails before any data is touched
    encoder_widths(encoderNodes)

    def codes(X_train, X_test, rs):                                # others/mr_gan_autoencoder.py:109-140
        ae = Autoencoder(X_train.shape[1], encoder_nodes=encoderNodes, batch_size=ae_batch_size, dtype=dtype,
                         seed=int(rs.randint(1 << 31)), device=device)
        ae.fit(X_train, epochs=ae_epochs, validation_data=X_test, verbose=1 if verbose else 0)
        out = ae.encode(X_train), ae.encode(X_test)
        ae.close()
        return out
    return gan_on_codes(codes, X, y, percentlabeled, percentunlabeled, epochs, trainTestSets, verbose, batch_size, dtype, seed, device, noise,
                        num_classes)
