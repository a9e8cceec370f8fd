"""More than eight classes, host side: the data helpers keep class order and counts, mr_gan / mr_nn take the class count."""
import inspect

import numpy as np

from mr_gan_amd import data


def test_synthetic_blobs_and_select_labeled_at_ten_classes():
    K = 10
    X, y = data.synthetic_blobs(n=400, d=12, num_classes=K, seed=3)
    assert X.shape == (400, 12) and sorted(set(y.tolist())) == list(range(K))
    assert [int(np.sum(y == j)) for j in range(K)] == [40] * K
    xl, yl, xu = data.select_labeled(X, y, 7, 5, num_classes=K)
    assert xl.shape == (7 * K, 12) and xu.shape == (12 * K, 12)
    np.testing.assert_array_equal(yl, np.repeat(np.arange(K), 7))                  # classes in order, 7 rows each
    for j in range(K):
        np.testing.assert_array_equal(xl[7 * j:7 * (j + 1)], X[y == j][:7])        # the first rows of each class
        np.testing.assert_array_equal(xu[12 * j:12 * (j + 1)], X[y == j][:12])
    # the default stays the reference's six materials: classes 6 .. 9 are left out
    xl6, yl6, _ = data.select_labeled(X, y, 7)
    assert xl6.shape == (42, 12) and yl6.max() == 5


def test_mr_gan_and_mr_nn_take_the_class_count():
    from mr_gan_amd.mr_gan import mr_gan
    from mr_gan_amd.mr_nn import mr_nn
    for fn in (mr_gan, mr_nn):
        p = inspect.signature(fn).parameters
        assert "num_classes" in p and p["num_classes"].default is None, fn.__name__
    assert data.resolve_num_classes(None) == len(data.MATERIALS) == 6
    assert data.resolve_num_classes(10) == 10
