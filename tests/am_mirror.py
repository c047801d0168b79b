"""An independent NumPy restatement of the AM sampler, written from the Julia sources — test infrastructure only.

iterate!(job, AM, Multivariate) of src/samplers/iterate/AM.jl:77-152, the sampler state of src/samplers/AM.jl:215-251, covariance! of
src/stats/covariance.jl:6-19 and recursive_mean! of src/stats/mean.jl:5, taken literally: a full matrix C, the three `ger!` updates,
`Hermitian(C)`, `MixtureModel([MvNormal(x, corescale * C), MvNormal(x, sqrtminorscale)], [1 - c, c])` with numpy.linalg.cholesky where the
MvNormal constructor factors its covariance (it raises where that throws), the mixture's logpdf by log-sum-exp at both centres, and the ratio
`(r - q(x -> x')) + q(x' -> x)` of :100-106.  None of the library's deviations A1-A5 is taken over, and no code is shared
with oracle/klara_oracle.c ko_am or the kernels.  The draws are the job's Philox stream, read through the oracle library: ko_transition_normals (D normals
and the accept uniform of a transition) and ko_stream_block, whose words (z, w) of the accept block choose the mixture component.
"""
import ctypes as C
import math

import numpy as np

import oracle_ffi as O

LOG2PI = math.log(2.0 * math.pi)


def draws(seed, chain, t, D):
    z = np.zeros(D); u = C.c_double(0.0)
    O.load().ko_transition_normals(int(seed), int(chain), int(t), int(D), z.ctypes.data, C.byref(u))
    return z, u.value


def selector(seed, chain, t, D):
    """the 52-bit uniform (m + 1/2) 2^-52 of words (z, w) of block slot ceil(D / 2): m = z's 32 bits over w's upper 20"""
    w = (C.c_uint32 * 4)()
    f = O.load().ko_stream_block
    f.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32)]
    f.restype = None
    f(int(seed), int(chain), int(t), (int(D) + 1) // 2, w)
    m = (int(w[2]) << 20) | (int(w[3]) >> 12)
    return (2 * m + 1) * 2.0 ** -53


def mvnormal_logpdf(mean, L, x):
    """logpdf(MvNormal(mean, Sigma), x) with Sigma = L L'"""
    y = np.linalg.solve(L, x - mean)
    return -0.5 * (mean.size * LOG2PI + 2.0 * float(np.sum(np.log(np.diag(L))))) - 0.5 * float(y @ y)


def mixture_logpdf(mean, L, sqrtminor, w, x):
    """logpdf(MixtureModel([MvNormal(mean, L L'), MvNormal(mean, sqrtminor)], w), x): log-sum-exp over the components of positive weight"""
    lp = []
    if w[0] > 0:
        lp.append(mvnormal_logpdf(mean, L, x) + math.log(w[0]))
    if w[1] > 0:
        lp.append(mvnormal_logpdf(mean, sqrtminor * np.eye(mean.size), x) + math.log(w[1]))
    m = max(lp)
    return m + math.log(sum(math.exp(v - m) for v in lp))


class AmChain:
    def __init__(self, lt, x0, seed, chain_id, C0, corescale=1.0, minorscale=1.0, c=0.05, t0=10):
        self.ltf, self.seed, self.cid = lt, int(seed), int(chain_id)
        self.x = np.array(x0, dtype=float)
        self.D = self.x.size
        self.lt = float(lt(self.x))                                  # initialize!: AM.jl:160-173
        assert math.isfinite(self.lt), "Log-target not finite: initial value out of support"
        self.C = np.array(C0, dtype=float)                           # sampler_state: copy(sampler.C0), AM.jl:238-246
        self.corescale, self.t0 = float(corescale), int(t0)
        self.sqrtminor = math.sqrt(minorscale)                       # :235
        self.w = [1 - c, c]                                          # :236
        self.lastmean = self.x.copy(); self.secondlastmean = self.x.copy()
        self.count = 0
        self.accepts, self.plain_accepts, self.q = [], [], []        # q: (logpdf at x' centred x, logpdf at x centred x') beyond t0

    def step(self):
        t = self.count
        self.count += 1                                              # iterate/AM.jl:78
        z, u = draws(self.seed, self.cid, t, self.D)
        L = None
        if self.count <= self.t0:                                    # :84-85 set_normal!
            xp = self.x + self.sqrtminor * z                         # :96
        else:
            k = self.count - 2                                       # :87-89 covariance!
            Cn = (k - 1) * self.C                                    # covariance.jl:14
            Cn = Cn + np.outer(self.x, self.x)                       # :15
            Cn = Cn + np.outer(-(k + 1) * self.lastmean, self.lastmean)          # :16
            Cn = Cn + np.outer(k * self.secondlastmean, self.secondlastmean)     # :17
            Cn = Cn / k                                              # :18
            self.C = np.triu(Cn) + np.triu(Cn, 1).T                  # :91 Hermitian(C): the upper triangle
            L = np.linalg.cholesky(self.corescale * self.C)          # :93 set_gmm!: MvNormal(x, corescale * C) factors its covariance — or throws
            core = selector(self.seed, self.cid, t, self.D) < self.w[0]          # rand(MixtureModel): the component, then its draw
            xp = self.x + (L @ z if core else self.sqrtminor * z)    # :96
        ltp = float(self.ltf(xp))                                    # :98
        r = ltp - self.lt                                            # :100
        ratio = r
        if L is not None:                                            # :102-106: the same C at both centres
            q1 = mixture_logpdf(self.x, L, self.sqrtminor, self.w, xp)
            q2 = mixture_logpdf(xp, L, self.sqrtminor, self.w, self.x)
            self.q.append((q1, q2))
            ratio = (r - q1) + q2
        logu = math.log(u)
        acc = bool(ratio > 0 or ratio > logu)                        # :108
        self.plain_accepts.append(bool(r > 0 or r > logu))           # what the test gives on r alone (A1)
        if acc:                                                      # :109-110
            self.x, self.lt = xp, ltp
        self.secondlastmean = self.lastmean.copy()                   # :134
        self.lastmean = ((self.count - 1) * self.lastmean + self.x) / self.count      # :135, mean.jl:5
        self.accepts.append(acc)
        return acc

    def run(self, n):
        for _ in range(n):
            self.step()
