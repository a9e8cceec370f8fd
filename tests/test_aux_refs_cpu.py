"""tests/aux_refs.py against the pinned oracle (oracle/mrgan_oracle.py) on one small seeded Case, to 1e-12: the kernel-level
tests of the non-GEMM kernels rest on the oracle, not on a third unpinned restatement."""
import numpy as np

from oracle import mrgan_oracle as O
from tests import aux_refs as R
from tests.helpers import Case

TOL = 1e-12


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert np.max(np.abs(a - b)) <= TOL * max(1.0, float(np.max(np.abs(b)))), float(np.max(np.abs(a - b)))


CASE = Case(D=16, B=50, steps=1, d_hidden=(48, 40, 32, 24, 24), g_hidden=(40, 40))


def _features():
    inp = CASE.disc_inputs(0, 0)
    out = {}
    for name, x, nz in (("lab", inp['x_lab'], inp['n_lab']), ("unl", inp['x_unl'], inp['n_unl'])):
        out[name] = O.disc_forward(CASE.d0, x, nz)
    xg, _ = O.gen_forward(CASE.g0, inp['z'])
    out["fake"] = O.disc_forward(CASE.d0, xg, inp['n_fake'])
    return inp, out


def test_head_reference_reproduces_oracle_losses_and_last_dense_gradients():
    inp, fw = _features()
    B, W6, b6 = CASE.B, CASE.d0[-2], CASE.d0[-1]
    labels = inp['labels']
    rows = {}
    for name, kind in (("lab", R.LAB), ("unl", R.UNL), ("fake", R.FAKE)):
        logits, feat, _ = fw[name]
        _close(feat @ W6 + b6, logits)
        rows[name] = R.head_rows(logits, kind, labels, 1.0 / B, O.UNLABELED_WEIGHT)
    loss_lab, loss_unl, err = O.disc_losses(fw["lab"][0], labels, fw["unl"][0], fw["fake"][0])
    _close(rows["lab"][0].sum() / B, loss_lab)
    _close((rows["unl"][1].sum() + rows["fake"][1].sum()) / B, loss_unl)
    _close(rows["lab"][2].sum() / B, err)
    for name, want in zip(("lab", "unl", "fake"), O.disc_loss_grads(fw["lab"][0], labels, fw["unl"][0], fw["fake"][0])):
        _close(rows[name][3], want)
        logits, feat, cache = fw[name]
        grads, _ = O.disc_backward(CASE.d0, cache, dlogits=want)
        dw6, db6, dpre, dbf = R.head_backward(feat, W6, rows[name][3])
        _close(dw6, grads[-2])
        _close(db6, grads[-1])
        _close(dbf, grads[-3])                               # bias gradient of the feature layer = column sums of dL/d(pre5)
        _close(cache['ins'][4].T @ dpre, grads[-4])
    # the supervised baseline's loss, and a first-index argmax on an exact tie
    logits = fw["lab"][0]
    loss, e, dl = O.mse_loss_grad(logits, labels)
    r = R.head_rows(logits, R.MSE, labels, 1.0 / B)
    _close(r[0].sum() / B, loss); _close(r[2].sum() / B, e); _close(r[3], dl)
    short = labels.copy()
    short[40:] = -1
    r = R.head_rows(logits, R.MSE, short, 1.0 / 40)
    loss, e, dl = O.mse_loss_grad(logits[:40], labels[:40])
    _close(r[0].sum() / 40, loss); _close(r[2].sum() / 40, e); _close(r[3][:40], dl)
    assert not r[3][40:].any() and not r[0][40:].any() and not r[2][40:].any()
    tie = np.array([[1.0, 3.0, 3.0, 0.0]])
    assert R.head_rows(tie, R.EVAL, [1], 1.0)[2][0] == 0.0 and R.head_rows(tie, R.EVAL, [2], 1.0)[2][0] == 1.0


def test_head_case_seeds_leave_no_row_undecided():
    """The train error of the kernel-level head tests leaves out rows whose two largest reference logits are closer than twice the
    logit bound (cap 1 %: no row at these sizes).  The reference side needs no GPU: every case of tests/test_aux_kernels.py is
    drawn here, and a case that names a label must have rows on which the two identical W6 columns tie for the maximum."""
    from tests import test_aux_kernels as T
    ties = 0
    for case in T.HEAD_CASES + T.WIDE_CASES:
        und, labelled, tie = T._head_inputs(**case)[-1]
        assert und <= 0.01 * labelled, (case, und, labelled)
        if labelled:
            assert tie > 0, case
        ties += tie
    assert ties > 100


def test_adam_reference_reproduces_oracle_adam():
    rng = np.random.default_rng(3)
    adam = O.Adam(CASE.g0, CASE.d0)
    params = [p.copy() for p in CASE.d0]
    mine = [(p.copy(), np.zeros_like(p), np.zeros_like(p)) for p in CASE.d0]
    for it in range(3):
        grads = [rng.standard_normal(p.shape) * 10.0 ** rng.integers(-6, 1) for p in params]
        lr_t = R.adam_lr_t(adam.lr, adam.b1, adam.b2, adam.iterations)
        _close(lr_t, adam.lr_t())
        adam.apply(params, grads, 'd')
        mine = [R.adam(p, m, v, g, lr_t, adam.b1, adam.b2, adam.eps) for (p, m, v), g in zip(mine, grads)]
        for (p, m, v), po, mo, vo in zip(mine, params, adam.md, adam.vd):
            _close(p, po); _close(m, mo); _close(v, vo)
    assert adam.iterations == 3


def test_fm_reference_reproduces_oracle_feature_matching():
    _, fw = _features()
    f_fake, f_real = fw["fake"][1], fw["unl"][1]
    loss, gj = R.fm(f_fake.sum(axis=0), f_real.sum(axis=0), CASE.B)
    _close(loss, O.fm_loss(f_fake, f_real))
    _close(np.broadcast_to(gj, f_fake.shape), O.fm_loss_grad(f_fake, f_real))
    _close(R.fm(f_fake.sum(axis=0), f_real.sum(axis=0), CASE.B, 0.5)[1], 0.5 * gj)


def test_batchnorm_reference_reproduces_oracle_generator_layer():
    inp, _ = _features()
    g, B = CASE.g0, CASE.B
    W1, b1, gamma, beta, W2, b2, W3, b3 = g
    x, c = O.gen_forward(g, inp['z'])
    h1 = c['h1']
    mean, var, rstd = R.bn_stats(h1.sum(axis=0), (h1 * h1).sum(axis=0), B, O.BN_EPS)
    _close(mean, c['mu']); _close(var, c['var']); _close(rstd, c['rstd'])
    _close(R.bn_apply(h1, mean, rstd, gamma, beta), c['hbn'])
    dx = np.random.default_rng(5).standard_normal(x.shape)
    grads = O.gen_backward(g, c, dx)
    dhbn = ((dx @ W3.T) * O.sigmoid(c['pre2'])) @ W2.T
    dpre1, dbeta, dgamma = R.bn_bwd(dhbn, h1, mean, rstd, gamma, B)
    _close(dgamma, grads[2]); _close(dbeta, grads[3])
    _close(c['z'].T @ dpre1, grads[0]); _close(dpre1.sum(axis=0), grads[1])
    # the same from the column sums a shard is handed
    _close(R.bn_bwd(dhbn, h1, mean, rstd, gamma, B, dhbn.sum(axis=0), (dhbn * c['xhat']).sum(axis=0))[0], dpre1)
    # a constant column: the clamp keeps the variance at zero, rstd = 1 / sqrt(eps), output = beta
    m, v, r = R.bn_stats(np.array([0.3 * 7]), np.array([0.09 * 7 - 1e-9]), 7, 2e-5)
    assert v[0] == 0.0 and r[0] == 1.0 / np.sqrt(2e-5)
