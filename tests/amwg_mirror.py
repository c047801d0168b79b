"""An independent NumPy restatement of the AMWG sampler with the Roberts-Rosenthal tuner — test infrastructure only.

The algorithm iterate!(job, MuvAMWG, Multivariate) of src/samplers/iterate/AMWG.jl:82-171 intends (the candidate replaces
coordinate i of the CURRENT state), with tune_state / rate! / set_batch! / set_delta! / tune! of src/tuners/RobertsRosenthalMCTuner.jl:76-108 taken
literally: `totproposed` starts at the period and grows by the period at every event, batch = totproposed / period, δ = min(0.01, batch^-0.5) as a
power, the rate accepted / proposed with `proposed` counted up to the period.  Nothing is shared with tests/amwg_ref.py, the oracle or the kernels: the
draws come from tests/numpy_mirror.py's own Philox4x32-10 and Box-Muller (libm, not the library's table-driven functions), the log-target is a NumPy
closure, log / exp / sqrt are libm's.  So the states agree with the reference to rounding (1e-12 over 60 transitions) while the accept decisions —
the coordinate masks — must be identical.
"""
import math

import numpy as np

import numpy_mirror as M


def uniforms(seed, chain, t, D):
    """u_i: 44 bits of block slot ceil(D/2) + (i >> 1) of the transition — words (x, y) for even i, words (z, w) for odd i"""
    s0 = (D + 1) // 2
    out = []
    for i in range(D):
        b = M.stream_block(seed, chain, t, s0 + (i >> 1))
        out.append(M.u44(b[2], b[3]) if i & 1 else M.u44(b[0], b[1]))
    return out


class AmwgChain:
    def __init__(self, lt, x0, seed, chain_id, logsigma0, targetrate=0.44, period=50):
        self.ltf, self.seed, self.cid = lt, int(seed), int(chain_id)
        self.x = np.array(x0, dtype=float)
        self.D = self.x.size
        self.lt = float(lt(self.x))                                  # initialize!: AMWG.jl:153-164
        assert math.isfinite(self.lt), "Log-target not finite: initial value out of support"
        self.logsigma = np.array(np.broadcast_to(np.asarray(logsigma0, dtype=float), (self.D,)))      # tuner_state: copy of logσ0, AMWG.jl:165-166
        self.targetrate, self.period = float(targetrate), int(period)
        self.accepted = [0] * self.D; self.proposed = 0; self.totproposed = self.period               # AMWG.jl:166
        self.count = 0
        self.masks, self.rates, self.deltas = [], [], []

    def step(self):
        t = self.count
        self.count += 1
        z = M.normals(self.seed, self.cid, t, self.D)
        u = uniforms(self.seed, self.cid, t, self.D)
        self.proposed += 1                                           # iterate/AMWG.jl:83
        tuning = self.proposed == self.period                        # :85 (mod(proposed, period) == 0 with proposed cleared at every event)
        if tuning:
            batch = self.totproposed / self.period                   # set_batch!, RobertsRosenthalMCTuner.jl:99
            delta = min(0.01, batch ** -0.5)                         # set_delta!, :101
            self.deltas.append(delta)
        mask = 0
        for i in range(self.D):
            xp = self.x.copy()
            xp[i] = self.x[i] + math.sqrt(math.exp(self.logsigma[i])) * z[i]      # :96
            ltp = float(self.ltf(xp))                                # :97 (W1)
            ratio = ltp - self.lt                                    # :99
            if ratio > 0 or ratio > math.log(u[i]):                  # :117
                self.x, self.lt = xp, ltp
                self.accepted[i] += 1
                mask |= 1 << i
            if tuning:                                               # :148-165
                rate = self.accepted[i] / self.proposed              # rate!, RobertsRosenthalMCTuner.jl:80
                self.rates.append(rate)
                self.logsigma[i] += -delta if rate < self.targetrate else delta      # tune!, RobertsRosenthalMCTuner.jl:104-108
                self.accepted[i] = 0
        if tuning:
            self.totproposed += self.proposed; self.proposed = 0     # :168-170
        self.masks.append(mask)
        return mask

    def run(self, n):
        for _ in range(n):
            self.step()
