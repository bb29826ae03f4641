"""The inference entry points share one set of grow-only device buffers (medgp_capi.hip: DevBuf, enum BufId): a sequence of calls
of different kinds and sizes on ONE context must give, call by call, the bits of the same call on a fresh context -- nothing a
call leaves in a shared buffer, and no buffer another call has outgrown or replaced, may show -- and a warm context allocates
nothing."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import medgp_amd
from medgp_amd import synth

FAM = (7, 2, 2, 2)   # LMC-SM, Q = 2, D = 2, R = 2
NS = (40, 130)       # two size classes


def _data():
    pts = [synth.patient(11, p, FAM[2], n, interleave=(p == 1)) for p, n in enumerate(NS)]
    th = np.stack([synth.theta(11, p, *FAM) for p in range(len(NS))])
    return pts, th


def _points(seed, m):
    g = np.random.default_rng(seed)
    return ([g.integers(0, FAM[2], size=m).astype(np.int32) for _ in NS], [g.uniform(0.0, 200.0, size=m).astype(np.float32) for _ in NS])


def make_ctx(pts):
    ctx = medgp_amd.Context(*FAM)
    ctx.reserve(len(pts), max(NS), len(pts))
    for s, (m, t, y) in enumerate(pts):
        ctx.set_patient(s, m, t, y)
    return ctx


def _flat(x):
    """every array of a (nested) result, in order"""
    if isinstance(x, np.ndarray):
        return [x]
    if isinstance(x, (list, tuple)):
        return [a for y in x for a in _flat(y)]
    return [] if x is None else [np.atleast_1d(np.asarray(x))]


def _calls(th):
    slots = np.arange(len(NS))
    g = np.random.default_rng(5)
    m5, t5 = _points(1, 5)
    m200, t200 = _points(2, 200)
    m70, t70 = _points(3, 70)
    prefix = [g.integers(0, n + 1, size=200).astype(np.int32) for n in NS]
    y2 = [g.normal(size=200).astype(np.float32) for _ in NS]
    eps = [g.normal(size=(70, 2)) for _ in NS]
    groups = []
    for n in NS:   # never held out, a singleton, an empty group (id 1), groups of 2 .. 64 and (N = 130) one of more than 64
        gid = np.where(np.arange(n) % 3 == 0, 2, 3 + np.arange(n) % 4).astype(np.int32)
        gid[:3] = (-1, 0, -1)
        if n > 100:
            gid[30:100] = 7
        groups.append(gid)
    posterior = lambda c: c.posterior(slots, th, m5, t5)
    return [("posterior", posterior),
            ("forecast", lambda c: c.forecast(slots, th, m200, t200, prefix, y2)),
            ("joint", lambda c: c.posterior_joint(slots, th, m70, t70, eps)),
            ("loo", lambda c: c.loo(slots, th, groups)),
            ("fit_predict", lambda c: c.fit_predict_batch(slots, th, [m[0] for m in m5], [t[0] for t in t5])),
            ("posterior again", posterior)]


def test_call_sequence_on_one_context_matches_fresh_contexts_bit_for_bit_and_warm_calls_allocate_nothing():
    pts, th = _data()
    calls = _calls(th)
    ctx = make_ctx(pts)
    got = [f(ctx) for _, f in calls]
    assert len(ctx.last_plan()) == 2, ctx.last_plan()   # two size classes
    for (name, f), mine in zip(calls, got):
        fresh = make_ctx(pts)
        ref = f(fresh)
        fresh.close()
        a, b = _flat(mine), _flat(ref)
        assert len(a) == len(b) and len(a) >= 3, name
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and x.shape == y.shape, name
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), name
        assert any(np.isfinite(x).any() for x in a if x.dtype.kind == "f"), name
    # every patient was factored in every call
    for (name, _), mine in zip(calls, got):
        st = mine[2] if name == "fit_predict" else mine[1]
        assert np.all(np.asarray(st) == 0), (name, st)
    warm = ctx.alloc_stats()[1]
    again = [f(ctx) for _, f in calls]
    assert ctx.alloc_stats()[1] == warm   # warm buffers allocate nothing
    for (name, _), x, y in zip(calls, got, again):
        assert all(np.array_equal(p.view(np.uint8), q.view(np.uint8)) for p, q in zip(_flat(x), _flat(y))), name
    ctx.close()
