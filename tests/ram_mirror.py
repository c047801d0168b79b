"""An independent NumPy restatement of the RAM sampler, written from the Julia sources — test infrastructure only.

iterate!(job, RAM, Multivariate) of src/samplers/iterate/RAM.jl:65-130 and the sampler state of src/samplers/RAM.jl:147-163, 201-211, taken
literally: `S * (eye + z z' / dot(z, z) * eta * (min(1, exp(ratio)) - targetrate)) * S'` and numpy.linalg.cholesky for
`ctranspose(chol(Hermitian(SST)))`, `count^(-gamma)` as a power.  None of the library's deviations R1-R4 is taken
over, and no code is shared with oracle/klara_oracle.c ko_ram or the kernels.  The draws are the job's Philox stream, read through the oracle library's
ko_transition_normals (D normals and the accept uniform of a transition).
"""
import ctypes as C
import math

import numpy as np

import oracle_ffi as O


def draws(seed, chain, t, D):
    z = np.zeros(D); u = C.c_double(0.0)
    O.load().ko_transition_normals(int(seed), int(chain), int(t), int(D), z.ctypes.data, C.byref(u))
    return z, u.value


class RamChain:
    def __init__(self, lt, x0, seed, chain_id, S0, targetrate=0.234, gamma=0.7):
        self.ltf, self.seed, self.cid = lt, int(seed), int(chain_id)
        self.x = np.array(x0, dtype=float)
        self.D = self.x.size
        self.lt = float(lt(self.x))                                  # initialize!: RAM.jl:117-130
        assert math.isfinite(self.lt), "Log-target not finite: initial value out of support"
        self.S = np.tril(np.array(S0, dtype=float))                  # sampler_state: copy(sampler.S0), :155-162
        self.targetrate, self.gamma = float(targetrate), float(gamma)
        self.count = 0
        self.accepts, self.last = [], None

    def step(self):
        t = self.count
        self.count += 1                                              # iterate/RAM.jl:66
        z, u = draws(self.seed, self.cid, t, self.D)                 # :72
        xp = self.x + self.S @ z                                     # :73
        ltp = float(self.ltf(xp))                                    # :75
        ratio = ltp - self.lt                                        # :77
        acc = bool(ratio > 0 or ratio > math.log(u))                 # :79
        if acc:                                                      # :80-82
            self.x, self.lt = xp, ltp
        eta = min(1.0, self.D * self.count ** (-self.gamma))         # :123
        with np.errstate(over="ignore"):
            M = np.outer(z, z) / np.dot(z, z) * eta * (min(1.0, float(np.exp(ratio))) - self.targetrate)     # :124-127
        SST = self.S @ (np.eye(self.D) + M) @ self.S.T               # :128
        self.last = (self.S.copy(), z, M)
        self.S = np.linalg.cholesky(0.5 * (SST + SST.T))             # :129 ctranspose(chol(Hermitian(SST)))
        self.accepts.append(acc)
        return acc

    def run(self, n):
        for _ in range(n):
            self.step()
