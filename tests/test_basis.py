"""medgp_amd.basis on hand-checked inputs: the column builders, Design for observations and test points alike, effect against its
closed form, conditioning.  No GPU."""
import math

import numpy as np
import pytest

from medgp_amd import basis as B

META = np.array([0, 1, 0, 1, 1], np.int32)
TIME = np.array([0.0, 10.0, 20.0, 30.0, 40.0])


def test_builders_on_hand_checked_inputs():
    assert np.array_equal(B.intercept(2)(META, TIME), [[1, 0], [0, 1], [1, 0], [0, 1], [0, 1]])
    assert np.array_equal(B.linear(2, 20.0, 10.0)(META, TIME), [[-2, 0], [0, -1], [0, 0], [0, 1], [0, 2]])
    assert np.array_equal(B.step(10.0, 30.0)(META, TIME).ravel(), [0, 1, 1, 0, 0])          # on <= t < off
    assert np.array_equal(B.step(10.0)(META, TIME).ravel(), [0, 1, 1, 1, 1])                # no end
    assert np.array_equal(B.step(10.0, 30.0, covariates=[0])(META, TIME).ravel(), [0, 0, 1, 0, 0])
    assert np.array_equal(B.ramp(10.0, 30.0)(META, TIME).ravel(), [0, 0, 0.5, 1, 1])
    assert np.array_equal(B.ramp(10.0, 30.0, covariates=[1])(META, TIME).ravel(), [0, 0, 0, 1, 1])
    h = B.harmonic(40.0)(META, TIME)
    assert h.shape == (5, 2) and np.allclose(h[:, 0], [1, 0, -1, 0, 1], atol=1e-15) and np.allclose(h[:, 1], [0, 1, 0, -1, 0], atol=1e-15)
    assert not B.harmonic(40.0, covariates=[1])(META, TIME)[[0, 2]].any()
    d = B.dose([5.0, 25.0], [2.0, 0.5])(META, TIME).ravel()
    assert np.array_equal(d, [0, 2, 2, 0.5, 0.5])
    assert np.array_equal(B.dose([5.0, 25.0], [2.0, 0.5], covariates=[0])(META, TIME).ravel(), [0, 0, 2, 0, 0])
    assert np.array_equal(B.step(10.0)(None, TIME).ravel(), [0, 1, 1, 1, 1])                # SE / SM: no covariates
    with pytest.raises(ValueError):
        B.ramp(5.0, 5.0)
    with pytest.raises(ValueError):
        B.linear(1, 0.0, 0.0)
    with pytest.raises(ValueError):
        B.dose([1.0, 1.0], [1.0, 2.0])


def test_design_gives_the_same_columns_for_observations_and_test_points():
    des = B.Design([B.intercept(2), B.linear(2, 20.0, 10.0), B.step(10.0, 30.0, [1]), B.harmonic(24.0)])
    assert des.p == 7 and des.names == ["intercept0", "intercept1", "slope0", "slope1", "step[10,30)@1", "cos24", "sin24"]
    H = des.design(META, TIME)
    assert H.shape == (5, 7) and H.flags["C_CONTIGUOUS"] and H.dtype == np.float64
    # the rows of a point do not depend on which other points are asked for, nor on their order
    perm = np.array([3, 0, 4, 2, 1])
    assert np.array_equal(des.design(META[perm], TIME[perm]), H[perm])
    assert np.array_equal(des.design(META[1:2], TIME[1:2]), H[1:2])
    assert np.array_equal(des.contrast("slope1"), [0, 0, 0, 1, 0, 0, 0])
    with pytest.raises(ValueError):
        B.Design([B.intercept(33), B.linear(33, 0.0, 1.0)])       # 66 columns


def test_effect_against_its_closed_form():
    beta, cov = np.array([1.0, -2.0, 0.5]), np.array([[4.0, 1.0, 0.0], [1.0, 9.0, 0.0], [0.0, 0.0, 0.25]])
    est, sd, z, pr = B.effect(beta, cov, [0, 0, 1])
    assert (est, sd, z) == (0.5, 0.5, 1.0) and abs(pr - 0.8413447460685429) <= 1e-15
    est, sd, z, pr = B.effect(beta, cov, [1, -1, 0])             # a difference: var = 4 + 9 - 2
    assert est == 3.0 and abs(sd - math.sqrt(11.0)) <= 1e-15 and abs(z - 3.0 / math.sqrt(11.0)) <= 1e-15
    assert abs(pr - 0.5 * (1 + math.erf(3.0 / math.sqrt(22.0)))) <= 1e-15
    assert B.effect(beta, np.zeros((3, 3)), [0, 1, 0]) == (-2.0, 0.0, -math.inf, 0.0)          # FIXED: no spread
    b0, lam = B.flat_prior(3)
    assert not b0.any() and not lam.any() and np.array_equal(B.normal_prior(2, sd=0.5)[1], [4.0, 4.0])


def test_conditioning_flags_a_duplicated_column():
    g = np.random.default_rng(7)
    H = g.standard_normal((40, 5))
    assert 1.0 <= B.conditioning(H) < 10.0
    assert B.conditioning(H * np.array([1e6, 1, 1e-6, 1, 1])) == pytest.approx(B.conditioning(H), rel=1e-9)   # column scales do not matter
    assert B.conditioning(np.concatenate([H, H[:, 2:3]], axis=1)) == math.inf
    assert B.conditioning(np.concatenate([H, H[:, 2:3] + 1e-7 * H[:, 1:2]], axis=1)) > 1e6
    # uncentred time beside an intercept: the docstring's warning
    t = np.linspace(1000.0, 1200.0, 50)
    assert B.conditioning(np.stack([np.ones(50), t], axis=1)) > 10 * B.conditioning(np.stack([np.ones(50), (t - 1100.0) / 60.0], axis=1))
    assert B.conditioning(np.zeros((4, 2))) == math.inf and B.conditioning(g.standard_normal((3, 5))) == math.inf
