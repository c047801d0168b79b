"""Writes tests/golden/zv_kat.npz: the known-answer fixture of the zero-variance control variates (tests/test_zv_host.py, tests/test_gpu_zv.py).

Not run by the tests.  Needs mpmath (the tests do not).

  value, grad   one chain's saved values and gradlogtarget, n = 400 x D = 4, on the standardised swiss logistic regression (lambda = 100).
                The history comes from a NumPy MALA written out below (doc/examples/swiss/MALA/analytical.jl's target, MALA.jl's proposal
                x + h / 2 grad + sqrt(h) N(0, I)), NOT from the project's kernels or the CPU oracle: the fixture tests the estimator, any
                plausible history serves, and this one can be regenerated without building anything.  h = 0.1, 200 burn-in steps, seed below.
  a1, a2        the order-1 (4 x 4) and order-2 (14 x 4) coefficients of stats/variance/zv.jl for that history: centred cross-products and
                the solve  S_ff a = -S_fx  at 40 significant digits (mpmath), rounded to double.
  accept        the acceptance rate of the 400 saved transitions (a record).
"""
from pathlib import Path

import mpmath as mp
import numpy as np

HERE = Path(__file__).resolve().parent


def swiss():
    raw = np.load(HERE / "swiss.npz")
    X = raw["measurements"]
    X = (X - X.mean(axis=0)) / X.std(axis=0, ddof=1)
    return X, raw["status"].astype(np.float64)


def logtarget_and_grad(b, X, y, lam):
    xb = X @ b
    lt = float(xb @ y - np.sum(np.log1p(np.exp(xb))) - b @ b / (2.0 * lam))
    g = X.T @ (y - 1.0 / (1.0 + np.exp(-xb))) - b / lam
    return lt, g


def mala(X, y, lam, h, x0, burnin, n, rng):
    x = x0.copy()
    lt, g = logtarget_and_grad(x, X, y, lam)
    value, grad, acc = np.empty((n, x.size)), np.empty((n, x.size)), 0
    for t in range(burnin + n):
        mean = x + 0.5 * h * g
        prop = mean + np.sqrt(h) * rng.standard_normal(x.size)
        ltp, gp = logtarget_and_grad(prop, X, y, lam)
        back = prop + 0.5 * h * gp
        ratio = ltp - lt - np.sum((x - back) ** 2) / (2.0 * h) + np.sum((prop - mean) ** 2) / (2.0 * h)
        ok = np.log(rng.random()) < ratio
        if ok:
            x, lt, g = prop, ltp, gp
        if t >= burnin:
            value[t - burnin], grad[t - burnin] = x, g
            acc += bool(ok)
    return value, grad, acc / n


def controls(x, g, order):
    """zv.jl:24, 61-70 on exact (mpmath) numbers: rows of control variates."""
    n, d = len(x), len(x[0])
    rows = []
    for t in range(n):
        z = [-g[t][i] / 2 for i in range(d)]
        f = list(z)
        if order == 2:
            f += [2 * z[i] * x[t][i] - 1 for i in range(d)]
            f += [x[t][i] * z[j] + x[t][j] * z[i] for i in range(d - 1) for j in range(i + 1, d)]
        rows.append(f)
    return rows


def solve_exact(value, grad, order):
    mp.mp.dps = 40
    x = [[mp.mpf(float(v)) for v in row] for row in value]
    g = [[mp.mpf(float(v)) for v in row] for row in grad]
    f = controls(x, g, order)
    n, d, k = len(x), len(x[0]), len(f[0])
    fm = [mp.fsum(f[t][a] for t in range(n)) / n for a in range(k)]
    xm = [mp.fsum(x[t][i] for t in range(n)) / n for i in range(d)]
    sff = mp.matrix(k, k)
    sfx = mp.matrix(k, d)
    for a in range(k):
        for b in range(a, k):
            sff[a, b] = sff[b, a] = mp.fsum((f[t][a] - fm[a]) * (f[t][b] - fm[b]) for t in range(n))
        for i in range(d):
            sfx[a, i] = mp.fsum((f[t][a] - fm[a]) * (x[t][i] - xm[i]) for t in range(n))
    cols = [mp.lu_solve(sff, -sfx[:, i]) for i in range(d)]
    return np.array([[float(cols[i][a]) for i in range(d)] for a in range(k)])


def main():
    X, y = swiss()
    rng = np.random.default_rng(20131023)
    value, grad, acc = mala(X, y, 100.0, 0.1, np.array([5.1, -0.9, 8.2, -4.5]), 200, 400, rng)
    a1, a2 = solve_exact(value, grad, 1), solve_exact(value, grad, 2)
    np.savez(HERE / "zv_kat.npz", value=value, grad=grad, a1=a1, a2=a2, accept=np.float64(acc))
    print(f"zv_kat.npz: n = {value.shape[0]}, D = {value.shape[1]}, acceptance {acc:.3f}, max|a1| = {np.abs(a1).max():.3g}, max|a2| = {np.abs(a2).max():.3g}")


if __name__ == "__main__":
    main()
