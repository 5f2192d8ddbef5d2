"""samplers.linear_alphas_cumprod (host code, no GPU): the linear-beta training table against its closed form, and that a sampler's schedule takes it.

With beta_s = b0 + d s (d = (b1 - b0) / (n - 1)) the product prod_{s <= t} (1 - beta_s) = d^(t+1) prod_{s <= t} (x - s), x = (1 - b0) / d, is
d^(t+1) Gamma(x + 1) / Gamma(x - t): evaluated through lgamma in float64 (x ~ 9e4, so the logarithms are ~ 1e6 and their difference is good to
~ 1e-9), against a table stored in fp32 (2^-24 relative)."""
import math

import numpy as np
import pytest

from tinyfusers_amd.variants import samplers as S


@pytest.mark.parametrize("b0,b1,n", [(0.00085, 0.0120, 1000), (0.0001, 0.02, 1000), (0.00085, 0.0120, 10)])
def test_linear_table_matches_its_closed_form(b0, b1, n):
    a = S.linear_alphas_cumprod(b0, b1, n)
    assert a.dtype == np.float32 and a.shape == (n,)
    d = (b1 - b0) / (n - 1)
    x = (1.0 - b0) / d
    t = np.arange(n)
    closed = np.exp([(i + 1) * math.log(d) + math.lgamma(x + 1.0) - math.lgamma(x - i) for i in t])
    np.testing.assert_allclose(a.astype(np.float64), closed, rtol=2e-7, atol=0)
    assert a[0] == np.float32(1.0 - b0) and (np.diff(a) < 0).all()


def test_linear_table_is_not_the_default_one():
    lin, dflt = S.linear_alphas_cumprod(), S.get_alphas_cumprod()
    assert lin.shape == dflt.shape == (1000,)
    # the same first and last beta, but evenly spaced betas are larger in between: the linear table falls faster (0.0016 against 0.0047 at the end)
    assert lin[0] == pytest.approx(dflt[0], rel=1e-6) and (lin[1:] < dflt[1:]).all()
    assert lin[-1] == pytest.approx(0.00158, abs=1e-5) and dflt[-1] == pytest.approx(0.00466, abs=1e-5)


def test_a_schedule_takes_the_linear_table():
    lin = S.linear_alphas_cumprod()
    smp = S.make("dpmpp2m")
    got, dflt = smp.schedule(steps=4, alphas_cumprod=lin), smp.schedule(steps=4)
    assert list(got.timesteps) == list(dflt.timesteps)
    assert np.array_equal(got.alphas, lin.astype(np.float64)[list(got.timesteps)]) and not np.allclose(got.coeffs, dflt.coeffs)
