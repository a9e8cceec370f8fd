"""The numpy restatement of the true-Gaussian generator (tests/gaussian_noise.py) on its own: these tests pin the
definition the device is held to in tests/test_gaussian_noise_gpu.py, with the same thresholds."""
import numpy as np
import pytest

from tests import gaussian_noise as G
from tests.helpers import SEED


def test_distribution_of_the_restatement():
    G.check_distribution(G.gaussian_normal(SEED, 1, 1, 3, 2048, 512))


@pytest.mark.parametrize("key", [(0, 0, 0), (4, 2, 11), (16, 0, 5), (2, 1, 1000)])
def test_other_keys_are_normal_too(key):
    x = G.gaussian_normal(SEED, key[0], key[1], key[2], 2048, 512)
    m, s, k = G.moments(x)
    assert abs(m) < 5e-3 and abs(s - 1) < 5e-3 and abs(k) < 0.02, (m, s, k)        # the bounds of check_distribution, same n
    assert G.ks_distance(x) < 1.95e-3


def test_uniforms_are_exact_in_float32_and_inside_their_intervals():
    u1, u2 = G.gaussian_uniforms(SEED, 3, 2, 7, 512, 256)
    for u in (u1, u2):
        np.testing.assert_array_equal(u.astype(np.float32).astype(np.float64), u)
        np.testing.assert_array_equal(np.rint(u * 2.0 ** 24), u * 2.0 ** 24)
    assert u1.min() >= 2.0 ** -24 and u1.max() <= 1.0 - 2.0 ** -24          # ln u1 finite and negative
    assert u2.min() >= 0.0 and u2.max() <= 1.0 - 2.0 ** -24
    assert (np.rint(u1 * 2.0 ** 24).astype(np.int64) & 1).all()               # odd numerators: u1 is never 0


def test_support_bound():
    assert abs(G.SUPPORT - np.sqrt(-2.0 * np.log(2.0 ** -24))) < 1e-12 and G.SUPPORT < 5.77
    x = G.gaussian_normal(SEED, 1, 1, 3, 2048, 512)
    assert np.abs(x).max() <= G.SUPPORT


@pytest.mark.parametrize("row0", [36, 48, 2])
def test_a_shard_draws_what_the_full_batch_draws(row0):
    full = G.gaussian_normal(SEED, 2, 1, 9, 120, 96)
    np.testing.assert_array_equal(G.gaussian_normal(SEED, 2, 1, 9, 70, 96, row0=row0), full[row0:row0 + 70])
    # (an odd first row is consistent too in the restatement -- rows are indexed globally; the DEVICE draws whole pairs and
    #  takes even first rows only)
    np.testing.assert_array_equal(G.gaussian_normal(SEED, 2, 1, 9, 33, 96, row0=37), full[37:70])


def test_pairs_share_radius_and_angle():
    x = G.gaussian_normal(SEED, 0, 0, 0, 64, 48)
    u1, _ = G.gaussian_uniforms(SEED, 0, 0, 0, 64, 48)
    np.testing.assert_array_equal(u1[0::2], u1[1::2])
    np.testing.assert_allclose(x[0::2] ** 2 + x[1::2] ** 2, -2.0 * np.log(u1[0::2]), rtol=1e-12)


def test_stream_differs_from_the_default_generator_and_between_keys():
    from oracle import mrgan_oracle as O
    a = G.gaussian_normal(SEED, 1, 1, 3, 64, 64)
    assert np.abs(a - O.device_normal(SEED, 1, 1, 3, 64, 64)).max() > 1.0
    assert abs(np.corrcoef(a.ravel(), G.gaussian_normal(SEED, 1, 1, 4, 64, 64).ravel())[0, 1]) < 0.06
    assert abs(np.corrcoef(a.ravel(), G.gaussian_normal(SEED + 1, 1, 1, 3, 64, 64).ravel())[0, 1]) < 0.06


def test_twins_follow_the_helpers_conventions():
    from oracle import mrgan_oracle as O
    ns = G.noise_set(SEED, 2, 5, 50, 72)
    assert [n.shape for n in ns] == [(50, 72), (50, 1000), (50, 500), (50, 250), (50, 250)]
    np.testing.assert_array_equal(ns[3], G.gaussian_normal(SEED, 3, 2, 5, 50, 250))
    np.testing.assert_array_equal(G.draw_z(SEED, 4, 50), G.gaussian_normal(SEED, O.SITE_Z, 0, 4, 50, O.NOISE_SIZE))
    c = G.GaussCase(D=16, B=50, steps=1, device_z=True)
    np.testing.assert_array_equal(c.disc_inputs(0, 0)['z'], G.draw_z(SEED, 0, 50))
    np.testing.assert_array_equal(c.gen_inputs(0, 1, rows=24, row0=24)['n_real'][1], G.gaussian_normal(SEED, 1, 1, 1, 24, 1000, row0=24))


def test_noise_keyword_is_validated_without_a_device():
    from mr_gan_amd import engine as E
    assert E.noise_flags('irwin-hall') == 0 and E.noise_flags('gaussian') == E.FLAG_GAUSS_NOISE == 16
    with pytest.raises(ValueError):
        E.noise_flags('normal')
    from mr_gan_amd import dist
    assert dist.dp_flags(noise='gaussian') == dist.dp_flags() | E.FLAG_GAUSS_NOISE
    with pytest.raises(ValueError):
        dist.dp_flags(noise='box-muller')


def test_command_line_passes_noise_through_the_job_dicts():
    """--noise gaussian reaches every job dict (scheduler.train_job hands them to mr_gan()); the default adds nothing"""
    import importlib
    M = importlib.import_module('mr_gan_amd.mr_gan')
    seen = []

    class Sched(object):
        def __init__(self, **kw):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

        def put_dataset(self, X, y):
            return 0

        def run(self, jobs):
            seen.extend(jobs)
            return [0.0] * len(jobs)

    rs = np.random.RandomState(0)
    data = lambda **kw: (rs.randn(60, 4), np.repeat(np.arange(6), 10))
    M.main(['--tables', '6', '--gpus', '1', '--noise', 'gaussian'], dataset_fn=data, scheduler_factory=Sched)
    assert seen and all(j['noise'] == 'gaussian' for j in seen)
    del seen[:]
    M.main(['--tables', '6', '--gpus', '1'], dataset_fn=data, scheduler_factory=Sched)
    assert seen and all('noise' not in j for j in seen)
    with pytest.raises(SystemExit):
        M.main(['--tables', '6', '--noise', 'cauchy'], dataset_fn=data, scheduler_factory=Sched)
