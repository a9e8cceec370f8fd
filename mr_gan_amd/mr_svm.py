"""SVM baseline of the reference on the same harness (mr_svm.py:77-116 and its --tables 2 4 loops, :119-166):
RBF-kernel SVC (C = 1) trained on the labeled subset only.  By default on scikit-learn / CPU as in the reference;
--backend hip fits and scores with mr_gan_amd.svm.RBFSVM (csrc/svm.hip: Gram matrix, SMO solver and vote on the GPU).

    python -m mr_gan_amd.mr_svm --tables 2 4 [-v] [--backend {sklearn,hip}]

Shares dataset(), the data prologue and the modality names with mr_gan_amd.mr_gan; prints the reference's lines
(mr_svm.py prints only the averages for table 2 and one line per object for table 4)."""
import argparse
import functools
import itertools
import sys

import numpy as np

from mr_gan_amd.data import prologue, resolve_num_classes, train_test_sets
from mr_gan_amd.mr_gan import MODALITIES, dataset, print_lines
from mr_gan_amd.svm import RBFSVM


SVC_GAMMA = 'auto'
BACKENDS = ('sklearn', 'hip')


def mr_svm(X, y, percentlabeled=50, trainTestSets=None, verbose=False, seed=None, backend='sklearn'):
    if backend not in BACKENDS:
        raise ValueError("backend must be one of %s, got %r" % (BACKENDS, backend))
    rs = np.random.RandomState(seed if seed is not None else np.random.randint(1 << 31))     # mr_svm.py:79 is unseeded
    num_classes = resolve_num_classes(None)
    sets = train_test_sets(X, y, trainTestSets, rs, num_classes)   # mr_svm.py:82-89
    x_labeled, y_labeled, _, _, X_test, y_test, lines = prologue(sets, percentlabeled, None, rs, num_classes)
    print_lines(lines, verbose)
    # mr_svm.py:106 is SVC(kernel='rbf', C=1.0) under the scikit-learn of 2017 (Keras 2.0.9 era, README.md:43-48), whose default
    # kernel width was gamma='auto' = 1 / n_features.  scikit-learn >= 0.22 defaults to 'scale' (1 / (n_features * X.var())),
    # which differs on the small standardised labeled subset: pass the reference's value explicitly.
    if backend == 'hip':
        svm = RBFSVM(C=1.0, gamma=SVC_GAMMA)         # the same C and kernel width; no CPU fallback behind it
    else:
        from sklearn.svm import SVC
        svm = SVC(kernel='rbf', C=1.0, gamma=SVC_GAMMA)
    svm.fit(x_labeled, y_labeled)
    testerror = 1.0 - svm.score(X_test, y_test)                    # mr_svm.py:110
    if verbose:
        print_lines([('Test error:', testerror, 1.0 - np.mean(svm.predict(X_test) == y_test))])
    return testerror


def baseline_tables(tables, fn, dataset_fn, verbose=False, folds_fn=None):
    """The --tables 2 4 loops shared by mr_svm.py:126-166 and mr_nn.py:128-168 (identical up to the function called).
    folds_fn (mr_nn --group-folds): table 2 hands the six folds of a (modality, percentage) to
    folds_fn(sets, percentlabeled=, verbose=) -> their test errors in fold order, instead of calling fn once per fold."""
    from sklearn.model_selection import StratifiedKFold
    if '2' in tables:
        print('\n', '-' * 25, 'Testing various amounts of labeled training data', '-' * 25)
        print('-' * 100)
        for modality in [2, 5]:
            print('-' * 25, MODALITIES[modality], 'modality', '-' * 25)
            X, y = dataset_fn(modalities=modality)
            for percent in [1, 2, 4, 8, 16, 50, 100]:
                print('-' * 15, 'Percentage of training data labeled: %d%%' % percent, '-' * 15)
                errors = []
                skf = StratifiedKFold(n_splits=6, shuffle=True)
                sets = [[X[trainIdx], X[testIdx], y[trainIdx], y[testIdx]] for trainIdx, testIdx in skf.split(X, y)]
                if folds_fn is not None:
                    errors = list(folds_fn(sets, percentlabeled=percent, verbose=verbose))
                    sys.stdout.flush()
                for s in sets if folds_fn is None else []:
                    errors.append(fn(None, None, percentlabeled=percent, trainTestSets=s, verbose=verbose))
                    sys.stdout.flush()
                print('Average error:', np.mean(errors), 'Average accuracy:', np.mean(1.0 - np.array(errors)))
                sys.stdout.flush()
    if '4' in tables:
        print('\n', '-' * 25, 'Testing generalization with leave-one-object-out validation', '-' * 25)
        print('-' * 100)
        for modality in [2, 5]:
            print('-' * 25, MODALITIES[modality], 'modality', '-' * 25)
            objects = dataset_fn(modalities=modality, leaveObjectOut=True)
            for percent in [1, 4, 16, 50, 100]:
                print('-' * 15, 'Percentage of training data labeled: %d%%' % percent, '-' * 15)
                errors = []
                for objName, objData in objects.items():
                    Xtest, ytest = np.array(objData['x']), np.array(objData['y'])
                    Xtrain = np.array(list(itertools.chain.from_iterable([d['x'] for n, d in objects.items() if n != objName])))
                    ytrain = np.array(list(itertools.chain.from_iterable([d['y'] for n, d in objects.items() if n != objName])))
                    errors.append(fn(None, None, percentlabeled=percent, trainTestSets=[Xtrain, Xtest, ytrain, ytest], verbose=verbose))
                    print(objName, 'Test error:', errors[-1], 'Test accuracy:', 1.0 - errors[-1])
                    sys.stdout.flush()
                print('Average leave-one-object-out error:', np.mean(errors), 'Average accuracy:', np.mean(1.0 - np.array(errors)))
                sys.stdout.flush()


def main(argv=None, dataset_fn=dataset, fn=mr_svm):
    parser = argparse.ArgumentParser(description='RBF-SVM baseline for material recognition on haptic data.')
    parser.add_argument('-t', '--tables', nargs='+', help='[Required] Tables to recompute', required=True)
    parser.add_argument('-v', '--verbose', help='Verbose', action='store_true')
    parser.add_argument('--backend', choices=BACKENDS, default='sklearn',
                        help="'sklearn': scikit-learn on the CPU, as in the reference (default); 'hip': RBFSVM on the GPU")
    args = parser.parse_args(argv)
    if args.backend != 'sklearn':
        fn = functools.partial(fn, backend=args.backend)
    baseline_tables(args.tables, fn, dataset_fn, args.verbose)


if __name__ == '__main__':
    main()
