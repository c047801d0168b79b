"""The derived-quantity closures of the tests (klara_desc.derived_src): C text for klara_user_derived, each with the number of outputs it writes.  The same
text goes to the run-time compiler (the device) and to gcc (tests/derived_ref.py, the reference)."""
import numpy as np

# (a) a contrast and a product: out = {x0 - x1, x0 * x1}
SRC_A = r"""
KLARA_USER_FN void klara_user_derived(const double* x, int D, const double* data, long long ndata, double* out, int K)
{
    out[0] = x[0] - x[1];
    out[1] = x[0] * x[1];
}
"""
K_A = 2

# (b) the sum of all D coordinates and the sum of their squares: reads the whole row
SRC_B = r"""
KLARA_USER_FN void klara_user_derived(const double* x, int D, const double* data, long long ndata, double* out, int K)
{
    double s = 0.0, q = 0.0;
    for (int i = 0; i < KLARA_D; ++i) { s = s + x[i]; q = q + x[i] * x[i]; }
    out[0] = s;
    out[1] = q;
}
"""
K_B = 2

# (c) the predictive probability at a new covariate row (the data block): 1 / (1 + exp(-sum_j data_j x_j))
SRC_C = r"""
KLARA_USER_FN void klara_user_derived(const double* x, int D, const double* data, long long ndata, double* out, int K)
{
    double eta = 0.0;
    for (int j = 0; j < KLARA_D; ++j) eta = eta + data[j] * x[j];
    out[0] = 1.0 / (1.0 + kd_exp(-eta));
}
"""
K_C = 1

# (d) NaN wherever x0 < 0
SRC_D = r"""
KLARA_USER_FN void klara_user_derived(const double* x, int D, const double* data, long long ndata, double* out, int K)
{
    out[0] = x[0] < 0.0 ? __builtin_nan("") : x[0];
}
"""
K_D = 1

# (e) any number of outputs (KLARA_K): out[k] = x[k mod D] * x[(k + 1) mod D] + k
SRC_E = r"""
KLARA_USER_FN void klara_user_derived(const double* x, int D, const double* data, long long ndata, double* out, int K)
{
    for (int k = 0; k < KLARA_K; ++k) out[k] = x[k % KLARA_D] * x[(k + 1) % KLARA_D] + (double)k;
}
"""

SRC_NO_FUNCTION = r"""
KLARA_USER_FN void some_other_name(const double* x, int D, const double* data, long long ndata, double* out, int K) { out[0] = x[0]; }
"""

# the error is on the text's line 5
SRC_SYNTAX_ERROR = r"""
KLARA_USER_FN void klara_user_derived(const double* x, int D, const double* data, long long ndata, double* out, int K)
{
    out[0] = x[0];
    out[1] = x[0] +* ;
}
"""
SYNTAX_ERROR_LINE = 5


def history(ncols, N, D, seed=0, scale=1.0):
    """(ncols, N, D) doubles as the device keeps a value history: column t, chain c, D values contiguous"""
    rng = np.random.default_rng([20261020, seed, ncols, N, D])
    return np.ascontiguousarray(scale * rng.standard_normal((ncols, N, D)))


def half_negative_history(ncols, N, D, seed=0):
    """closure (d)'s input: the chains of even index never see a negative x0, those of odd index see one in their second saved step at the latest"""
    h = history(ncols, N, D, seed)
    h[:, 0::2, 0] = np.abs(h[:, 0::2, 0])
    h[min(1, ncols - 1), 1::2, 0] = -np.abs(h[min(1, ncols - 1), 1::2, 0]) - 0.5
    return h


def covariate_row(D):
    """the data block of closure (c): an intercept and D - 1 covariates"""
    return np.concatenate([[1.0], np.linspace(-0.75, 0.5, D - 1)]) if D > 1 else np.ones(1)
