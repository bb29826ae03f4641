"""medgp_amd.warp on the CPU: the map and its inverse, the packed optimiser vector, the prior, the start from the sample skewness and
the probability integral transform."""
import numpy as np

from medgp_amd import warp


def _psi(g, D):
    return np.stack([g.uniform(-0.5, 0.5, D), g.uniform(-1.0, 1.0, D), g.uniform(-0.7, 0.7, D)], axis=1)


def test_forward_inverse_round_trip_and_jacobian():
    g = np.random.default_rng(1)
    D = 4
    psi, kind = _psi(g, D), np.array([1, 0, 1, 1])
    m = g.integers(0, D, 200)
    y = 3.0 * g.standard_normal(200)
    z = warp.forward(y, psi, kind, m)
    assert np.array_equal(z[m == 1], y[m == 1])                       # NONE: exactly y
    back = warp.inverse(z, psi, kind, m)
    assert np.all(np.abs(back - y) <= 1e-13 * (1 + np.abs(y)))
    assert np.all(np.abs(warp.forward(y, warp.identity(D), None, m) - y) <= 4e-16 * (1 + np.abs(y)))
    h = 1e-6
    fd = (warp.forward(y + h, psi, kind, m) - warp.forward(y - h, psi, kind, m)) / (2 * h)
    assert np.all(fd > 0)                                             # monotone
    assert np.all(np.abs(np.log(fd) - warp.log_jacobian(y, psi, kind, m)) <= 1e-7)
    assert not np.any(warp.log_jacobian(y, psi, kind, m)[m == 1])
    assert np.all(np.abs(warp.log_jacobian(y, warp.identity(D), None, m)) <= 1e-14)


def test_pack_unpack():
    g = np.random.default_rng(2)
    nb, H, D = 3, 7, 4
    th, psi, kind = g.standard_normal((nb, H)), np.stack([_psi(g, D) for _ in range(nb)]), np.array([1, 0, 1, 0])
    x = warp.pack(th, psi, kind)
    assert x.shape == (nb, H + 3 * 2)
    th2, psi2 = warp.unpack(x, H, D, kind)
    assert np.array_equal(th2, th) and np.array_equal(psi2[:, [0, 2]], psi[:, [0, 2]]) and not np.any(psi2[:, [1, 3]])
    xa = warp.pack(th, psi)
    tha, psia = warp.unpack(xa, H, D)
    assert xa.shape == (nb, H + 3 * D) and np.array_equal(tha, th) and np.array_equal(psia, psi)
    try:
        warp.unpack(x, H, D)
    except ValueError:
        pass
    else:
        raise AssertionError("a vector of the wrong length was accepted")


def test_prior_grad_against_differences():
    g = np.random.default_rng(3)
    psi = np.stack([_psi(g, 3) for _ in range(2)])
    for mean, sd in ((0.0, 1.0), (np.array([0.1, -0.2, 0.0]), np.array([0.5, 1.0, 0.3]))):
        v, gr = warp.prior_grad(psi, mean, sd)
        assert v.shape == (2,) and gr.shape == psi.shape
        h = 1e-6
        for idx in np.ndindex(psi.shape):
            e = np.zeros_like(psi)
            e[idx] = h
            fd = (warp.prior_grad(psi + e, mean, sd)[0][idx[0]] - warp.prior_grad(psi - e, mean, sd)[0][idx[0]]) / (2 * h)
            assert abs(fd - gr[idx]) <= 1e-8 * (1 + abs(gr[idx]))
    assert np.array_equal(warp.prior_grad(psi)[1], psi)               # N(0, 1): the gradient is psi itself


def test_init_from_moments_has_the_sign_of_the_skew():
    g = np.random.default_rng(4)
    z = g.standard_normal(4000)
    m = np.repeat(np.arange(4), 1000)
    y = z.copy()
    y[m == 0] = np.sinh(np.arcsinh(z[m == 0]) + 0.8)                  # right-skewed
    y[m == 1] = np.sinh(np.arcsinh(z[m == 1]) - 0.8)                  # left-skewed
    y[m == 3] = 1.0                                                    # no spread
    psi = warp.init_from_moments(y, m, 5)
    assert psi.shape == (5, 3) and psi[0, 1] > 0.1 and psi[1, 1] < -0.1 and abs(psi[2, 1]) < 0.1
    assert not np.any(psi[3]) and not np.any(psi[4]) and not np.any(psi[:, [0, 2]]) and np.all(np.abs(psi[:, 1]) <= 1)


def test_pit_of_the_median_is_one_half_and_moments_of_the_identity():
    g = np.random.default_rng(5)
    D = 3
    psi, kind = _psi(g, D), np.array([1, 1, 0])
    m2 = g.integers(0, D, 50)
    zmean, zvar = g.standard_normal(50), g.uniform(0.2, 2.0, 50)
    med = warp.inverse(zmean, psi, kind, m2)
    assert np.all(np.abs(warp.pit(med, zmean, zvar, psi, kind, m2) - 0.5) <= 1e-12)
    lo = warp.inverse(zmean - 1.959963984540054 * np.sqrt(zvar), psi, kind, m2)
    assert np.all(np.abs(warp.pit(lo, zmean, zvar, psi, kind, m2) - 0.025) <= 1e-12)
    mean, var = warp.moments(zmean, zvar, warp.identity(D), None, m2)
    assert np.all(np.abs(mean - zmean) <= 1e-12) and np.all(np.abs(var - zvar) <= 1e-12 * (1 + zvar))
