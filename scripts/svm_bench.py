"""Seconds per fit and per score of the SVM baseline at the surrogate's shape -- synthetic_mreo(): d = 1200, 7200 rows, 6000 of
them the training fold, 1200 the test fold -- with 60, 960 and 6000 labeled rows (1 %, 16 % and 100 % of table 2), on the GPU
through mr_gan_amd.svm.RBFSVM and on this machine's CPU through scikit-learn's SVC (libsvm, one thread), side by side.

The RBFSVM time is split into its three stages with device events around each (gram / solve inside fit, predict = the chunked
cross-Gram + decide launches of score, host-to-device copies of the chunks included); fit and score are also timed as a whole with
the host clock around calls that end in a device-to-host copy (they include the host sort, the upload and the download).  Every
size is warmed up once, then repeated; the medians are reported, with the per-pair SMO iteration counts of both sides and the
test error of both.

    python scripts/svm_bench.py [--labeled 60 960 6000] [--repeats 5] [--sklearn-repeats 3]
                                [--classifier {svc-rbf,svc-linear,nu-rbf,nu-linear}]
Prints one JSON line per size.  --classifier takes another libsvm classifier of mr_svm's grid through mr_gan_amd.svm.KernelSVM, the
same stages, against the matching SVC / NuSVC (profiles/svm_kinds_bench.txt); svc-rbf, the default, is RBFSVM as before.

    python scripts/svm_bench.py --group [G] [--labeled 60 960 6000] [--repeats 5]          (G = 6 where not given)
times G fits and scores through one RBFSVMGroup (grouped launches) against the same G problems through G RBFSVM objects one
after the other, in the same process and by the same scheme (warm-up, medians, stages in passes of their own; scikit-learn is not
run).  Problem f takes its training fold from np.arange(len(y)) % 6 != f % 6, so the problems hold different rows.  One JSON
line per size with both totals, the per-stage times and their ratios single / grouped (profiles/svm_group_bench.txt).  With
--classifier KIND the two sides are one KernelSVMGroup and G KernelSVM objects of that kind (profiles/svm_kind_group_bench.txt)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mr_gan_amd import KernelSVM, KernelSVMGroup, RBFSVM, RBFSVMGroup, synthetic_mreo  # noqa: E402
from mr_gan_amd.mr_svm import CLASSIFIERS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--labeled", type=int, nargs="+", default=[60, 960, 6000])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sklearn-repeats", type=int, default=3, help="repeats of the CPU side (1 at 6000 rows: one fit is tens of seconds)")
    ap.add_argument("--d", type=int, default=1200)
    ap.add_argument("--group", type=int, nargs="?", const=6, default=None,
                    help="time G problems through RBFSVMGroup against G RBFSVM objects instead (G = 6 where not given); with "
                         "--classifier, through KernelSVMGroup against G KernelSVM objects")
    ap.add_argument("--classifier", choices=sorted(CLASSIFIERS), default='svc-rbf')
    args = ap.parse_args()
    if args.group is not None and args.group < 1:
        ap.error("--group needs at least one problem")
    if not torch.cuda.is_available():
        raise SystemExit("svm_bench needs a GPU: nothing is measured without one")
    from sklearn import preprocessing
    from sklearn.svm import SVC, NuSVC
    kernel, nu = CLASSIFIERS[args.classifier]
    X, y, _ = synthetic_mreo(d=args.d)
    if args.group is not None:
        folds = []
        for f in range(args.group):
            tr = np.arange(len(y)) % 6 != f % 6
            sc = preprocessing.StandardScaler()
            folds.append((sc.fit_transform(X[tr]), y[tr], sc.transform(X[~tr]), y[~tr]))
        for n in args.labeled:
            per = n // 6
            probs = [(np.concatenate([a[ya == c][:per] for c in range(6)]), np.repeat(np.arange(6), per), xt, yt) for a, ya, xt, yt in folds]
            if args.classifier == 'svc-rbf':
                print(json.dumps(measure_group(args, probs)))
            else:
                print(json.dumps(dict(measure_group(args, probs, lambda: KernelSVMGroup(kernel=kernel, nu=nu, C=1.0, gamma='auto'),
                                                    lambda: KernelSVM(kernel=kernel, nu=nu, C=1.0, gamma='auto')), classifier=args.classifier)))
            sys.stdout.flush()
        return
    tr = np.arange(len(y)) % 6 != 0
    sc = preprocessing.StandardScaler()
    a, xt = sc.fit_transform(X[tr]), sc.transform(X[~tr])
    ya, yt = y[tr], y[~tr]
    for n in args.labeled:
        per = n // 6
        xl = np.concatenate([a[ya == c][:per] for c in range(6)])
        yl = np.repeat(np.arange(6), per)
        if args.classifier == 'svc-rbf':
            print(json.dumps(measure(args, SVC, xl, yl, xt, yt)))
        else:
            make_hip = lambda: KernelSVM(kernel=kernel, nu=nu, C=1.0, gamma='auto')
            make_sk = (lambda: SVC(kernel=kernel, C=1.0, gamma='auto')) if nu is None else (lambda: NuSVC(kernel=kernel, nu=nu, gamma='auto'))
            print(json.dumps(dict(measure(args, SVC, xl, yl, xt, yt, make_hip, make_sk), classifier=args.classifier)))
        sys.stdout.flush()


def measure(args, SVC, xl, yl, xt, yt, make_hip=None, make_sk=None):
    n, d = xl.shape
    clf = RBFSVM(C=1.0, gamma='auto') if make_hip is None else make_hip()
    clf.fit(xl, yl).score(xt, yt)                       # warm-up: code objects, allocator
    fit_s, score_s, stages = [], [], dict(gram=[], solve=[], predict=[])
    for rep in range(args.repeats):
        clf.time_stages = False
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        clf.fit(xl, yl)
        t1 = time.perf_counter()
        acc = clf.score(xt, yt)
        t2 = time.perf_counter()
        fit_s.append(t1 - t0)
        score_s.append(t2 - t1)
        clf.time_stages = True                          # a pass of its own: the events synchronise between the stages
        clf.fit(xl, yl)
        clf.score(xt, yt)
        for k in stages:
            stages[k].append(clf.times_[k])
    reps = 1 if n > 2000 else args.sklearn_repeats
    sk_fit, sk_score = [], []
    for rep in range(reps):
        svc = SVC(kernel='rbf', C=1.0, gamma='auto') if make_sk is None else make_sk()
        t0 = time.perf_counter()
        svc.fit(xl, yl)
        t1 = time.perf_counter()
        sk_acc = svc.score(xt, yt)
        t2 = time.perf_counter()
        sk_fit.append(t1 - t0)
        sk_score.append(t2 - t1)
    med = lambda v: round(float(np.median(v)), 6)
    return dict(labeled=n, d=d, test_rows=len(yt), repeats=args.repeats, sklearn_repeats=reps,
                hip_fit_s=med(fit_s), hip_score_s=med(score_s), hip_fit_all=[round(v, 6) for v in fit_s],
                hip_gram_s=med(stages['gram']), hip_solve_s=med(stages['solve']), hip_predict_s=med(stages['predict']),
                sklearn_fit_s=med(sk_fit), sklearn_score_s=med(sk_score),
                fit_ratio_sklearn_over_hip=round(float(np.median(sk_fit) / np.median(fit_s)), 2),
                score_ratio_sklearn_over_hip=round(float(np.median(sk_score) / np.median(score_s)), 2),
                hip_iterations=clf.n_iter_.tolist(), sklearn_iterations=np.asarray(svc.n_iter_).tolist(),
                hip_test_error=round(1.0 - acc, 6), sklearn_test_error=round(1.0 - sk_acc, 6),
                gram_gflop=round(2e-9 * n * n * d, 2))


def measure_group(args, probs, make_group=None, make_single=None):
    G = len(probs)
    xs, ys, xts, yts = [list(v) for v in zip(*probs)]
    group = RBFSVMGroup(C=1.0, gamma='auto') if make_group is None else make_group()
    singles = [RBFSVM(C=1.0, gamma='auto') if make_single is None else make_single() for _ in range(G)]
    group.fit(xs, ys).score(xts, yts)                   # warm-up of both sides: code objects, allocator
    for clf, x, y_, xt, yt in zip(singles, xs, ys, xts, yts):
        clf.fit(x, y_).score(xt, yt)
    keys = ('gram', 'solve', 'predict')
    t = dict(group_fit=[], group_score=[], single_fit=[], single_score=[])
    st = {side + k: [] for side in ('group_', 'single_') for k in keys}
    for rep in range(args.repeats):                     # the two sides alternate inside every repeat
        group.time_stages = False
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        group.fit(xs, ys)
        t1 = time.perf_counter()
        g_acc = group.score(xts, yts)
        t2 = time.perf_counter()
        t['group_fit'].append(t1 - t0)
        t['group_score'].append(t2 - t1)
        fit_s = score_s = 0.0
        s_acc = []
        for clf, x, y_, xt, yt in zip(singles, xs, ys, xts, yts):
            clf.time_stages = False
            t0 = time.perf_counter()
            clf.fit(x, y_)
            t1 = time.perf_counter()
            s_acc.append(clf.score(xt, yt))
            t2 = time.perf_counter()
            fit_s += t1 - t0
            score_s += t2 - t1
        t['single_fit'].append(fit_s)
        t['single_score'].append(score_s)
        group.time_stages = True                        # passes of their own: the events synchronise between the stages
        group.fit(xs, ys)
        group.score(xts, yts)
        tot = dict.fromkeys(keys, 0.0)
        for clf, x, y_, xt, yt in zip(singles, xs, ys, xts, yts):
            clf.time_stages = True
            clf.fit(x, y_)
            clf.score(xt, yt)
            for k in keys:
                tot[k] += clf.times_[k]
        for k in keys:
            st['group_' + k].append(group.times_[k])
            st['single_' + k].append(tot[k])
    if g_acc != s_acc or any(group[p].n_iter_.tobytes() != singles[p].n_iter_.tobytes() for p in range(G)):
        raise SystemExit("svm_bench: the grouped and the single results differ")
    med = lambda v: round(float(np.median(v)), 6)
    out = dict(labeled=len(ys[0]), d=xs[0].shape[1], group=G, test_rows=[len(v) for v in yts], repeats=args.repeats)
    for k, v in list(t.items()) + list(st.items()):
        out[k + '_s'] = med(v)
    for k in ('fit', 'score') + keys:
        out[k + '_ratio_single_over_group'] = round(float(np.median((t if k in ('fit', 'score') else st)['single_' + k])
                                                          / np.median((t if k in ('fit', 'score') else st)['group_' + k])), 2)
    most = max(1, max(int(group[p].n_iter_.max()) for p in range(G)))      # a nu start point can be optimal: 0 updates
    out.update(iterations_max_per_problem=[int(group[p].n_iter_.max()) for p in range(G)],
               group_solve_us_per_update_of_slowest_pair=round(1e6 * float(np.median(st['group_solve'])) / most, 3),
               single_solve_us_per_update_of_slowest_pairs=round(1e6 * float(np.median(st['single_solve']))
                                                                 / max(1, sum(int(c.n_iter_.max()) for c in singles)), 3),
               gram_mbytes_group=round(sum(4e-6 * len(v) ** 2 for v in ys), 1), test_error=[round(1.0 - a, 6) for a in g_acc])
    return out


if __name__ == "__main__":
    main()
