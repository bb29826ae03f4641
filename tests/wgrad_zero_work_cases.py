"""Cases of tests/test_wgrad_zero_work_gpu.py: the shapes at which k_wgrad's skip of the zero stretches of U (kernels_wgrad.h,
wg_zero_stretches) and its flush can go wrong.  Built from seeds alone; a case is a dict as in nlml_truth.py (id, sweep, kidx, Q, D, R,
pts, th) plus `fails`: the patients whose factorisation fails by construction (status < 0).

  edges_Q5 / edges_Q1   one ragged call at D = 3: n = 64 (one tile, diagonal only), n = 65 (a padding row block), n = 130 with the
                        output counts (1, 64, 65) (column segments that start and end on tile edges, an output of one observation),
                        and a patient without noise on duplicated times (every retry meets a zero pivot: status -1)
  flush_D24             n = 192, D = 24: 8 observations per output, so every 16-row group flushes twice and meets three outputs
  pf2_D2                n = 256, D = 2 alone in its call: 10 tiles, the launch of few large patients (PF = 2) by default
"""
import numpy as np

from medgp_amd import synth


def _patient(g, counts):
    """observations grouped by output, `counts[d]` of output d, sorted by time inside an output (the loader's order)"""
    m = np.repeat(np.arange(len(counts)), counts).astype(np.int32)
    t = g.uniform(0.0, 200.0, size=m.shape[0]).astype(np.float32)
    for d in range(len(counts)):
        idx = np.where(m == d)[0]
        t[idx] = np.sort(t[idx])
    return m, t, g.standard_normal(m.shape[0]).astype(np.float32)


def _singular(n):
    """one output, every time stamp three times: without noise K is singular whatever the jitter adds"""
    t = np.repeat(np.arange(1, n // 3 + 2), 3)[:n].astype(np.float32)
    return np.zeros(n, np.int32), t, np.ones(n, np.float32)


def cases():
    out = []
    for Q in (5, 1):
        g = np.random.Generator(np.random.Philox(key=[20261019, Q]))
        D, R = 3, 2
        pts = [_patient(g, [22, 21, 21]), _patient(g, [22, 22, 21]), _patient(g, [1, 64, 65]), _singular(70)]
        th = [synth.theta(4801, 10 * Q + p, 7, Q, D, R) for p in range(4)]
        th[3][:D] = -80.0
        out.append(dict(id=f"edges_Q{Q}", sweep="wgrad_zero_work", kidx=7, Q=Q, D=D, R=R, pts=pts, th=th, fails=[3]))
    g = np.random.Generator(np.random.Philox(key=[20261019, 24]))
    out.append(dict(id="flush_D24", sweep="wgrad_zero_work", kidx=7, Q=5, D=24, R=8, pts=[_patient(g, [8] * 24)],
                    th=[synth.theta(4802, 0, 7, 5, 24, 8)], fails=[]))
    g = np.random.Generator(np.random.Philox(key=[20261019, 2]))
    out.append(dict(id="pf2_D2", sweep="wgrad_zero_work", kidx=7, Q=5, D=2, R=2, pts=[_patient(g, [128, 128])],
                    th=[synth.theta(4803, 0, 7, 5, 2, 2)], fails=[]))
    return out
