"""An independent NumPy restatement of the SMMALA sampler, written from the Julia sources — test infrastructure only.

iterate!(job, SMMALA, Multivariate) of src/samplers/iterate/SMMALA.jl:107-221 and the initial sampler state of src/samplers/SMMALA.jl:139-181,
with numpy.linalg for inv / logdet / the factorisation, the metric of doc/examples/swiss/SMMALA/analytical.jl:20-23, and the stream,
the log-target and the gradient of tests/numpy_mirror.py.  It shares no code with oracle/klara_oracle.c ko_smmala or the kernels.  The one
deviation it takes over from the library is the one that changes the draws (SMMALA deviation 1): the proposal
factor is C = L^-T with G = L L' (numpy.linalg.cholesky) instead of chol(inv(G))'.  Everything else — logdet(step * inv(G)),
dot(d, G d) / step — is the Julia expression.
"""
import math

import numpy as np

import numpy_mirror as M


def logistic_tensor(X, lam):
    """ptensorlogtarget of swiss/SMMALA/analytical.jl:20-23: (X' .* (r (1 - r))') X + I / lambda"""
    X = np.asarray(X, float)

    def tensor(p):
        r = 1.0 / (1.0 + np.exp(-(X @ p)))
        return (X.T * (r * (1.0 - r))) @ X + np.eye(X.shape[1]) / lam

    return tensor


class SmmalaChain(M.Chain):
    """numpy_mirror.Chain with the SMMALA sampler: tensor(x) is the metric (the parameter's tensorlogtarget).  (The base class's run loop
    and its tuning block — MALA's, as iterate/SMMALA.jl:196-220 — call _mala, which takes the SMMALA transition here.)"""

    def __init__(self, lt, grad, tensor, x0, seed, chain_id, *, driftstep=1.0, **kw):
        super().__init__("mala", lt, grad, x0, seed, chain_id, driftstep=driftstep, **kw)
        self.tensorf = tensor
        self.G = tensor(self.x)                                   # SMMALA.jl:164-181: tensor, its inverse, the first term, the factor
        self.invG = np.linalg.inv(self.G)
        self.first = self.invG @ self.g
        self.C = np.linalg.inv(np.linalg.cholesky(self.G)).T      # deviation 1: C = L^-T (the reference: chol(inv(G))')

    def _cnt(self):
        return (self.tuner == "vanilla" and self.verbose) or self.tuner == "rate"    # iterate/SMMALA.jl:108

    def propose(self, t, h):
        """one transition with step h; returns the accept flag (the state is updated on acceptance)"""
        mu = self.x + 0.5 * h * self.first                                               # :112
        xp = mu + math.sqrt(h) * (self.C @ M.normals(self.seed, self.cid, t, self.D))   # :113
        ltp, gp, Gp = self.ltf(xp), self.gradf(xp), self.tensorf(xp)                    # :115
        ratio = ltp - self.lt                                                            # :121
        ratio += 0.5 * (np.linalg.slogdet(h * self.invG)[1] + float((xp - mu) @ (self.G @ (xp - mu))) / h)    # :123-131
        try:
            Lp = np.linalg.cholesky(Gp)
        except np.linalg.LinAlgError:                                                    # deviation 4: not positive definite -> reject
            return False
        invGp = np.linalg.inv(Gp)                                                        # :133
        firstp = invGp @ gp                                                              # :135
        mup = xp + 0.5 * h * firstp                                                      # :137
        ratio -= 0.5 * (np.linalg.slogdet(h * invGp)[1] + float((self.x - mup) @ (Gp @ (self.x - mup))) / h)  # :139-147
        acc = ratio > 0 or ratio > math.log(M.accept_uniform(self.seed, self.cid, t, self.D))   # :149
        if acc:                                                                          # :150-176
            self.x, self.g, self.lt, self.G, self.invG, self.first = xp, gp, ltp, Gp, invGp, firstp
            self.C = np.linalg.inv(Lp).T
        return acc

    def _mala(self, t):
        return self.propose(t, self.step)


def run_pooled(chains, n, *, tuner, targetrate=None, score_k=7.0, period=100, burnin=0, verbose=False):
    """the pooled tuner (klara_tuner_mode POOLED): one step for all chains, the rate pooled over them; returns the accept rows"""
    step = chains[0].step
    accepted, proposed, totproposed = 0, 0, period
    cnt = (tuner == "vanilla" and verbose) or tuner == "rate"
    rows = []
    for _ in range(n):
        t = chains[0].t
        if cnt:
            proposed += 1
        row = []
        for c in chains:
            acc = c.propose(t, step)
            row.append(acc)
            i = t + 1
            if i > c.burnin and (i - c.burnin - 1) % c.thinning == 0 and i <= c.nsteps:
                c.saved.append(c.x.copy())
            c.t += 1
        if cnt:
            accepted += sum(row)
            if totproposed <= burnin and proposed % period == 0:
                rate = accepted / (proposed * len(chains))
                if tuner == "rate":
                    step *= 2.0 / (1.0 + math.exp(-score_k * (rate - targetrate)))
                totproposed += proposed
                accepted = proposed = 0
        rows.append(row)
    for c in chains:
        c.step = step
    return np.array(rows, dtype=np.uint8)
