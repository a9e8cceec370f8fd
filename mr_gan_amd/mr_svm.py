"""SVM baseline of the reference on the same harness (mr_svm.py:77-116 and its --tables 2 4 loops, :119-166):
RBF-kernel SVC (C = 1) trained on the labeled subset only.  By default on scikit-learn / CPU as in the reference;
--backend hip fits and scores with mr_gan_amd.svm.RBFSVM (csrc/svm.hip: Gram matrix, SMO solver and vote on the GPU).

    python -m mr_gan_amd.mr_svm --tables 2 4 [-v] [--backend {sklearn,hip}] [--group-folds]
                                [--classifier {svc-rbf,svc-linear,nu-rbf,nu-linear}] [--pca N]

--pca N puts N principal components of the scaled sets in front of the classifier (others/wganlpctsemi.py:129-139 pcaScale), on
either backend (hip: mr_gan_amd.pca.PCA, fitted on each fold's training rows).

--classifier picks another libsvm classifier of the reference's wider grid (others/wganlpctsemi.py:205-208): SVC or NuSVC
(nu = 0.5) with the RBF or the linear kernel, on either backend (hip: mr_gan_amd.svm.KernelSVM).

--group-folds (with --backend hip) fits and scores the six folds of each table-2 cell, and consecutive runs of twelve objects of
each table-4 cell, as ONE RBFSVMGroup (grouped launches over ragged problems) and prints the same lines.  The flag serves
--classifier svc-rbf; the other classifiers are grouped through mr_svm_folds(..., classifier=) (one KernelSVMGroup), e.g.
main(argv, folds_fn=functools.partial(mr_svm_folds, classifier='nu-linear')).

Shares dataset(), the data prologue and the modality names with mr_gan_amd.mr_gan; prints the reference's lines
(mr_svm.py prints only the averages for table 2 and one line per object for table 4)."""
import argparse
import functools
import itertools
import sys

import numpy as np

from mr_gan_amd.data import prologue, resolve_num_classes, train_test_sets
from mr_gan_amd.mr_gan import MODALITIES, dataset, print_lines
from mr_gan_amd.pca import pca_transform_hook
from mr_gan_amd.svm import KernelSVM, KernelSVMGroup, RBFSVM, RBFSVMGroup


SVC_GAMMA = 'auto'
BACKENDS = ('sklearn', 'hip')
# kernels 0 - 3 of the reference's wider SVM grid (others/wganlpctsemi.py:205-208) -> (kernel, nu); NuSVC's nu is scikit-learn's default
NU = 0.5
CLASSIFIERS = {'svc-rbf': ('rbf', None), 'svc-linear': ('linear', None), 'nu-rbf': ('rbf', NU), 'nu-linear': ('linear', NU)}


def mr_svm(X, y, percentlabeled=50, trainTestSets=None, verbose=False, seed=None, backend='sklearn', classifier='svc-rbf', pca=0):
    """pca > 0: the classifier sees that many principal components of the standard-scaled sets, fitted on the training rows
    (others/wganlpctsemi.py:129-139 pcaScale, whose SVM grid takes PCA in {0, 10}), computed by the chosen backend"""
    if backend not in BACKENDS:
        raise ValueError("backend must be one of %s, got %r" % (BACKENDS, backend))
    if classifier not in CLASSIFIERS:
        raise ValueError("classifier must be one of %s, got %r" % (sorted(CLASSIFIERS), classifier))
    kernel, nu = CLASSIFIERS[classifier]
    transform = pca_transform_hook(pca, backend)
    rs = np.random.RandomState(seed if seed is not None else np.random.randint(1 << 31))     # mr_svm.py:79 is unseeded
    num_classes = resolve_num_classes(None)
    sets = train_test_sets(X, y, trainTestSets, rs, num_classes)   # mr_svm.py:82-89
    x_labeled, y_labeled, _, _, X_test, y_test, lines = prologue(sets, percentlabeled, None, rs, num_classes, transform=transform)
    print_lines(lines, verbose)
    # mr_svm.py:106 is SVC(kernel='rbf', C=1.0) under the scikit-learn of 2017 (Keras 2.0.9 era, README.md:43-48), whose default
    # kernel width was gamma='auto' = 1 / n_features.  scikit-learn >= 0.22 defaults to 'scale' (1 / (n_features * X.var())),
    # which differs on the small standardised labeled subset: pass the reference's value explicitly.
    if backend == 'hip' and classifier == 'svc-rbf':
        svm = RBFSVM(C=1.0, gamma=SVC_GAMMA)         # the same C and kernel width; no CPU fallback behind it
    elif backend == 'hip':
        svm = KernelSVM(kernel=kernel, nu=nu, C=1.0, gamma=SVC_GAMMA)
    elif nu is None:
        from sklearn.svm import SVC
        svm = SVC(kernel=kernel, C=1.0, gamma=SVC_GAMMA)
    else:
        from sklearn.svm import NuSVC
        svm = NuSVC(kernel=kernel, nu=nu, gamma=SVC_GAMMA)
    svm.fit(x_labeled, y_labeled)
    testerror = 1.0 - svm.score(X_test, y_test)                    # mr_svm.py:110
    if verbose:
        print_lines([('Test error:', testerror, 1.0 - np.mean(svm.predict(X_test) == y_test))])
    return testerror


def mr_svm_folds(sets, percentlabeled=50, verbose=False, seed=None, classifier='svc-rbf', pca=0):
    """mr_svm(backend='hip') of every [X_train, X_test, y_train, y_test] of `sets` (the folds of a table-2 cell, the objects of a
    table-4 cell) as one RBFSVMGroup -- for another classifier of CLASSIFIERS one KernelSVMGroup -> their test errors.  Fold f
    runs mr_svm()'s prologue from RandomState(seed + f), the rule of mr_nn_folds: the errors are those of
    mr_svm(None, None, trainTestSets=sets[f], seed=seed + f, backend='hip', classifier=classifier, pca=pca); pca > 0 is one device
    PCA fit per fold, in turn, inside the fold's prologue."""
    if classifier not in CLASSIFIERS:
        raise ValueError("classifier must be one of %s, got %r" % (sorted(CLASSIFIERS), classifier))
    kernel, nu = CLASSIFIERS[classifier]
    transform = pca_transform_hook(pca, 'hip')
    base = int(seed if seed is not None else np.random.randint(1 << 30))
    num_classes = resolve_num_classes(None)
    folds = []
    for f, s in enumerate(sets):
        folds.append(prologue(s, percentlabeled, None, np.random.RandomState(base + f), num_classes, transform=transform))
        print_lines(folds[-1][-1], verbose)
    x_labeled, y_labeled, _, _, X_test, y_test, _ = zip(*folds)
    if classifier == 'svc-rbf':
        group = RBFSVMGroup(C=1.0, gamma=SVC_GAMMA)
    else:
        group = KernelSVMGroup(kernel=kernel, nu=nu, C=1.0, gamma=SVC_GAMMA)
    group.fit(x_labeled, y_labeled)
    errors = [1.0 - s for s in group.score(X_test, y_test)]
    if verbose:
        for e, lab, yt in zip(errors, group.predict(X_test), y_test):
            print_lines([('Test error:', e, 1.0 - np.mean(lab == yt))])
    return errors


OBJECT_GROUP = 12              # table 4: consecutive runs of this many objects of a cell are one group


def baseline_tables(tables, fn, dataset_fn, verbose=False, folds_fn=None, objects_fn=None):
    """The --tables 2 4 loops shared by mr_svm.py:126-166 and mr_nn.py:128-168 (identical up to the function called).
    folds_fn (mr_nn / mr_svm --group-folds): table 2 hands the six folds of a (modality, percentage) to
    folds_fn(sets, percentlabeled=, verbose=) -> their test errors in fold order, instead of calling fn once per fold.
    objects_fn (mr_svm --group-folds), the same signature: table 4 hands it consecutive runs of OBJECT_GROUP leave-one-out sets
    of a cell; the per-object lines keep their order and format."""
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
                errors, names, pending = [], list(objects), []
                for k, (objName, objData) in enumerate(objects.items()):
                    Xtest, ytest = np.array(objData['x']), np.array(objData['y'])
                    Xtrain = np.array(list(itertools.chain.from_iterable([d['x'] for n, d in objects.items() if n != objName])))
                    ytrain = np.array(list(itertools.chain.from_iterable([d['y'] for n, d in objects.items() if n != objName])))
                    pending.append([Xtrain, Xtest, ytrain, ytest])
                    if objects_fn is not None and len(pending) < OBJECT_GROUP and k + 1 < len(names):
                        continue
                    if objects_fn is not None:
                        new = list(objects_fn(pending, percentlabeled=percent, verbose=verbose))
                    else:
                        new = [fn(None, None, percentlabeled=percent, trainTestSets=pending[0], verbose=verbose)]
                    for name, e in zip(names[len(errors):], new):
                        print(name, 'Test error:', e, 'Test accuracy:', 1.0 - e)
                    errors += new
                    pending = []
                    sys.stdout.flush()
                print('Average leave-one-object-out error:', np.mean(errors), 'Average accuracy:', np.mean(1.0 - np.array(errors)))
                sys.stdout.flush()


def main(argv=None, dataset_fn=dataset, fn=mr_svm, folds_fn=None):
    parser = argparse.ArgumentParser(description='RBF-SVM baseline for material recognition on haptic data.')
    parser.add_argument('-t', '--tables', nargs='+', help='[Required] Tables to recompute', required=True)
    parser.add_argument('-v', '--verbose', help='Verbose', action='store_true')
    parser.add_argument('--backend', choices=BACKENDS, default='sklearn',
                        help="'sklearn': scikit-learn on the CPU, as in the reference (default); 'hip': RBFSVM on the GPU")
    parser.add_argument('--group-folds', action='store_true',
                        help='with --backend hip: fit and score the six folds of a table-2 cell, and runs of twelve objects of a '
                             'table-4 cell, as one RBFSVMGroup (one launch set)')
    parser.add_argument('--classifier', choices=sorted(CLASSIFIERS), default='svc-rbf',
                        help="the libsvm classifier of the reference's grid (others/wganlpctsemi.py:205-208): SVC (C = 1) or NuSVC "
                             "(nu = 0.5) with the RBF or the linear kernel; default svc-rbf, the baseline of mr_svm.py")
    parser.add_argument('--pca', type=int, default=0, metavar='N',
                        help="fit the classifier on N principal components of the scaled sets (others/wganlpctsemi.py pcaScale; its grid "
                             "takes 0 and 10), computed by the chosen backend; default 0: no PCA")
    args = parser.parse_args(argv)
    if args.pca < 0:
        parser.error('--pca takes a non-negative component count')
    if args.group_folds and args.backend != 'hip':
        parser.error('--group-folds needs --backend hip')
    if args.group_folds and args.classifier != 'svc-rbf':
        parser.error('--group-folds serves --classifier svc-rbf only; the other classifiers are grouped through mr_svm_folds(classifier=)')
    if args.backend != 'sklearn':
        fn = functools.partial(fn, backend=args.backend)
    if args.classifier != 'svc-rbf':
        fn = functools.partial(fn, classifier=args.classifier)
    if args.group_folds and folds_fn is None:
        folds_fn = mr_svm_folds
    if args.pca:
        fn = functools.partial(fn, pca=args.pca)
        folds_fn = functools.partial(folds_fn, pca=args.pca) if folds_fn is not None else None
    hook = folds_fn if args.group_folds else None
    baseline_tables(args.tables, fn, dataset_fn, args.verbose, folds_fn=hook, objects_fn=hook)


if __name__ == '__main__':
    main()
