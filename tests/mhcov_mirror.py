"""An independent NumPy restatement of random-walk Metropolis with a full proposal covariance, MH(Σ) — test infrastructure only.

iterate!(job, MH, Multivariate) of src/samplers/iterate/MH.jl:72-124 (symmetric normalised branch) with the proposal of MH(σ::Matrix), samplers/MH.jl:63-66:
x' ~ MvNormal(x, Σ), drawn as x + L z with L = cholesky(Σ).  Nothing is shared with tests/mhcov_ref.py, the oracle or the kernels: the draws come from
tests/numpy_mirror.py's own Philox4x32-10 and Box-Muller (libm, not the library's table-driven functions), the log-target is a NumPy closure, L z is
NumPy's matrix-vector product (its own summation order) and log is libm's.  So the states agree with the reference to rounding (1e-12 over 40 transitions)
while the accept decisions must be identical.
"""
import math

import numpy as np

import numpy_mirror as M


class MhCovChain:
    def __init__(self, lt, x0, seed, chain_id, factor):
        self.ltf, self.seed, self.cid = lt, int(seed), int(chain_id)
        self.x = np.array(x0, dtype=float)
        self.D = self.x.size
        self.L = np.tril(np.asarray(factor, dtype=float))
        self.lt = float(lt(self.x))                                  # initialize!: MH.jl:72-85
        assert math.isfinite(self.lt), "Log-target not finite: initial value out of support"
        self.count = 0
        self.accepts = []

    def step(self):
        t = self.count
        self.count += 1
        z = M.normals(self.seed, self.cid, t, self.D)
        xp = self.x + self.L @ z                                     # :79, MvNormal(x, Σ)
        ltp = float(self.ltf(xp))                                    # :81
        ratio = ltp - self.lt                                        # :83
        acc = ratio > 0 or ratio > math.log(M.accept_uniform(self.seed, self.cid, t, self.D))      # :97
        if acc:
            self.x, self.lt = xp, ltp                                # :98-100
        self.accepts.append(bool(acc))
        return acc

    def run(self, n):
        for _ in range(n):
            self.step()
