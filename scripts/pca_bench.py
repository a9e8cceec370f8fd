"""Seconds per fit and per transform of the PCA pre-stage at the surrogate's shape -- synthetic_mreo(): d = 1200, 7200 rows, 6000 of
them the training fold, 1200 the test fold, standard-scaled as the prologue does -- with 10 and 16 components, on the GPU
through mr_gan_amd.pca.PCA and on this machine's CPU through scikit-learn's PCA(svd_solver='full') and 'auto' (which, above
1000 features, is the randomized solver), side by side.

The PCA time is split into its stages with device events around each in passes of their own (mean / covariance / eig inside fit,
transform = the chunked projection of the test rows, host-to-device copies included), with the products the block iteration
took; fit and transform are also timed as a whole with the host clock around calls that end in a device-to-host copy.  Every
size is warmed up once, then repeated; medians and the spread (min, max) are reported.

Beside the covariance launch, the same product by the linear Gram kernel (mrgan_svm_kernel_matrix, LINEAR) on a pre-transposed
centred copy [d, n] -- m = n = 1200, reduction length 6000 -- is timed by device events, alternating with mrgan_pca_covariance:
the covariance kernel exists because it needs no transposed copy (the copy's own time is reported too).

    python scripts/pca_bench.py [--components 10 16] [--repeats 7] [--sklearn-repeats 3]
Prints one JSON line per component count and one for the covariance comparison (profiles/pca_bench.txt)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mr_gan_amd import PCA, synthetic_mreo  # noqa: E402
from mr_gan_amd import engine as E  # noqa: E402

med = lambda v: round(float(np.median(v)), 6)
spread = lambda v: [round(float(min(v)), 6), round(float(max(v)), 6)]


def events(fn, device):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(torch.cuda.current_stream(device))
    fn()
    b.record(torch.cuda.current_stream(device))
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def measure(args, k, a, xt):
    from sklearn import decomposition
    pca = PCA(k)
    pca.fit(a).transform(xt)                            # warm-up: code objects, allocator
    fit_s, tr_s, stages = [], [], dict(mean=[], covariance=[], eig=[], transform=[])
    for rep in range(args.repeats):
        pca.time_stages = False
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pca.fit(a)
        t1 = time.perf_counter()
        z = pca.transform(xt)
        t2 = time.perf_counter()
        fit_s.append(t1 - t0)
        tr_s.append(t2 - t1)
        pca.time_stages = True                          # a pass of its own: the events synchronise between the stages
        pca.fit(a)
        pca.transform(xt)
        for key in stages:
            stages[key].append(pca.times_[key])
    out = dict(components=k, rows=a.shape[0], d=a.shape[1], test_rows=xt.shape[0], repeats=args.repeats, products=pca.n_iter_,
               max_residual_over_lambda1=float(pca.residuals_.max() / pca.explained_variance_[0]),
               hip_fit_s=med(fit_s), hip_fit_spread=spread(fit_s), hip_transform_s=med(tr_s), hip_transform_spread=spread(tr_s),
               covariance_gflop=round(2e-9 * a.shape[0] * a.shape[1] ** 2, 2))
    for key, v in stages.items():
        out['hip_%s_s' % key] = med(v)
        out['hip_%s_spread' % key] = spread(v)
    for solver in ('full', 'auto'):
        f, t = [], []
        for rep in range(args.sklearn_repeats):
            sk = decomposition.PCA(n_components=k, svd_solver=solver, random_state=0)
            t0 = time.perf_counter()
            sk.fit(a)
            t1 = time.perf_counter()
            zs = sk.transform(xt)
            t2 = time.perf_counter()
            f.append(t1 - t0)
            t.append(t2 - t1)
        out['sklearn_%s_fit_s' % solver], out['sklearn_%s_transform_s' % solver] = med(f), med(t)
        out['fit_ratio_sklearn_%s_over_hip' % solver] = round(float(np.median(f) / np.median(fit_s)), 2)
        # agreement of the codes up to the components' signs (the randomized solver is approximate)
        out['sklearn_%s_max_code_diff' % solver] = float(np.abs(np.abs(zs) - np.abs(z)).max())
    return out


def covariance_comparison(args, a):
    """mrgan_pca_covariance against the linear Gram kernel on a pre-transposed centred copy: the same product"""
    pca = PCA(1)
    dev = pca.device
    x = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    n, d = x.shape
    mean = pca.mean_dev(x)
    cov = torch.empty((d, d), dtype=torch.float32, device=dev)
    gram = torch.empty((d, d), dtype=torch.float32, device=dev)
    xt = torch.empty((d, n), dtype=torch.float32, device=dev)
    transpose = lambda: xt.copy_((x - mean).t())
    linear = lambda: pca._call("mrgan_svm_kernel_matrix", E.SVM_KERNEL_LINEAR, xt.data_ptr(), xt.stride(0), d, xt.data_ptr(), xt.stride(0), d, n,
                               1.0, gram.data_ptr(), gram.stride(0))
    ours = lambda: pca.covariance_dev(x, mean, out=cov)
    for warm in (transpose, linear, ours):
        warm()
    t_cov, t_lin, t_tr = [], [], []
    for rep in range(args.repeats):                     # the two alternate inside every repeat
        t_cov.append(events(ours, dev))
        t_lin.append(events(linear, dev))
        t_tr.append(events(transpose, dev))
    diff = float((cov - gram / (n - 1)).abs().max())
    gflop = 2e-9 * n * d * d
    return dict(comparison='covariance', rows=n, d=d, repeats=args.repeats, gflop_full_product=round(gflop, 2),
                pca_covariance_s=med(t_cov), pca_covariance_spread=spread(t_cov),
                linear_gram_s=med(t_lin), linear_gram_spread=spread(t_lin), transposed_copy_s=med(t_tr),
                pca_covariance_tflops_of_full_product=round(gflop * 1e-3 / np.median(t_cov), 2),
                linear_gram_tflops=round(gflop * 1e-3 / np.median(t_lin), 2),
                ratio_linear_gram_over_pca_covariance=round(float(np.median(t_lin) / np.median(t_cov)), 3),
                max_abs_difference=diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--components", type=int, nargs="+", default=[10, 16])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sklearn-repeats", type=int, default=3)
    ap.add_argument("--d", type=int, default=1200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pca_bench needs a GPU: nothing is measured without one")
    from sklearn import preprocessing
    X, y, _ = synthetic_mreo(d=args.d)
    tr = np.arange(len(y)) % 6 != 0
    sc = preprocessing.StandardScaler()
    a, xt = sc.fit_transform(X[tr]), sc.transform(X[~tr])
    for k in args.components:
        print(json.dumps(measure(args, k, a, xt)))
        sys.stdout.flush()
    print(json.dumps(covariance_comparison(args, a)))


if __name__ == "__main__":
    main()
