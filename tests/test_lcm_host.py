"""Host checks (no GPU) of the LCM sampler of tinyfusers_amd/variants/samplers.py and of compile(..., cfg=False)'s refusals
(variants/inputs.py): the walk against its formula, the n = 4 table against pinned values, every table against a float64 loop written from
the scheduler's formulas, the image-to-image suffix, and the variance recursion that guards the sign and scale of c_n."""
import types

import numpy as np
import pytest

from tinyfusers_amd.variants import inputs as I
from tinyfusers_amd.variants import samplers as S


def _formula(n, original=50):
    k = 1000 // original
    return [k * (original - int(np.floor(i * original / n))) - 1 for i in range(n)]


@pytest.mark.parametrize("n", [1, 2, 4, 8, 50])
def test_default_timesteps_are_the_formula(n):
    sch = S.LCM().schedule(n)
    assert sch.timesteps == _formula(n) == [999 - 20 * ((50 * i) // n) for i in range(n)]
    assert S._check_timesteps(sch.timesteps) == sch.timesteps                  # the existing checks pass
    S._abar(np.concatenate([sch.alphas, [1.0]]))
    assert sch.alphas_prev[-1] == 1.0 and np.array_equal(sch.alphas_prev[:-1], sch.alphas[1:])
    assert np.array_equal(sch.alphas, S.get_alphas_cumprod()[sch.timesteps].astype(np.float64))


def test_pinned_walks_and_step_count_limits():
    assert S.LCM().schedule(4).timesteps == [999, 759, 499, 259]
    assert S.LCM().schedule(8).timesteps == [999, 879, 759, 639, 499, 379, 259, 139]
    assert S.LCM().schedule(1).timesteps == [999]
    assert S.LCM().schedule().timesteps == [999, 759, 499, 259]                # default_steps = 4
    assert S.LCM(original_steps=25).schedule(5).timesteps == _formula(5, 25)
    for bad in (0, 51, -1):
        with pytest.raises(ValueError):
            S.LCM().schedule(bad)
    with pytest.raises(ValueError):
        S.LCM(original_steps=25).schedule(26)
    for kw in (dict(original_steps=0), dict(timestep_scaling=0.0), dict(sigma_data=float("nan"))):
        with pytest.raises(ValueError):
            S.LCM(**kw)
    # an explicit walk is taken as it is, under the existing checks
    assert S.LCM().schedule(timesteps=[901, 601, 301, 1]).timesteps == [901, 601, 301, 1]
    for bad in ([500, 500, 1], [1, 500], [1000, 10], []):
        with pytest.raises(ValueError):
            S.LCM().schedule(timesteps=bad)


def test_n4_table_is_the_pinned_one():
    c = S.LCM().schedule(4).coeffs
    assert c.shape == (4, 4) and c.dtype == np.float64
    np.testing.assert_allclose(c[:, 1], [0.228501327, 0.526943562, 0.811773044, 0.999999981], rtol=0, atol=1e-9)
    np.testing.assert_allclose(c[:, 3], [0.973543601, 0.849900277, 0.583973046, 0.0], rtol=0, atol=1e-9)
    assert np.all(c[:, 2] == 0.0) and c[3, 3] == 0.0
    assert abs(c[0, 0] - 5.72e-10) < 1e-11 and abs(c[3, 0] - 3.73e-8) < 1e-9 and np.all(np.diff(c[:, 0]) > 0)


@pytest.mark.parametrize("kw", [dict(steps=1), dict(steps=2), dict(steps=4), dict(steps=8), dict(timesteps=[901, 601, 301, 1])])
def test_every_table_is_the_scheduler_formulas_in_float64(kw):
    """Luo et al. 2023 / the public LCM scheduler: scaled = t * timestep_scaling, c_skip = sigma_data^2 / (scaled^2 + sigma_data^2),
    c_out = scaled / sqrt(scaled^2 + sigma_data^2), denoised = c_out x0 + c_skip x, prev = sqrt(a_prev) denoised + sqrt(1 - a_prev) noise,
    and prev = denoised at the last step."""
    for lcm in (S.LCM(), S.LCM(timestep_scaling=7.0, sigma_data=0.3)):
        sch = lcm.schedule(**kw)
        ac = S.get_alphas_cumprod().astype(np.float64)
        rng = np.random.default_rng(len(sch.timesteps))
        n = len(sch.timesteps)
        for i, t in enumerate(sch.timesteps):
            x, x0, xp, z = rng.standard_normal((4, 64))
            scaled = float(t) * lcm.timestep_scaling
            c_skip = lcm.sigma_data ** 2 / (scaled ** 2 + lcm.sigma_data ** 2)
            c_out = scaled / (scaled ** 2 + lcm.sigma_data ** 2) ** 0.5
            denoised = c_out * x0 + c_skip * x
            if i == n - 1:
                ref = denoised
            else:
                a_prev = ac[sch.timesteps[i + 1]]
                ref = np.sqrt(a_prev) * denoised + np.sqrt(1.0 - a_prev) * z
            c_x, c_0, c_1, c_n = sch.coeffs[i]
            got = c_x * x + c_0 * x0 + c_1 * xp + c_n * z
            assert np.all(np.abs(got - ref) <= 1e-12 * (1.0 + np.abs(ref))), (i, float(np.max(np.abs(got - ref))))
        assert sch.coeffs[-1, 3] == 0.0 and np.all(sch.coeffs[:-1, 3] > 0) and np.isfinite(sch.coeffs).all()


def test_strength_keeps_the_last_steps_of_the_walk():
    full, half = S.LCM().schedule(8), S.LCM().schedule(8, strength=0.5)
    assert half.timesteps == full.timesteps[4:] == [499, 379, 259, 139]
    assert np.array_equal(half.alphas, full.alphas[4:]) and np.array_equal(half.alphas_prev, full.alphas_prev[4:])
    assert np.array_equal(half.coeffs, full.coeffs[4:])             # the row depends on its own timestep and a_s alone
    assert len(S.LCM().schedule(4, strength=0.1).timesteps) == 1


def test_make_and_the_other_samplers_are_untouched():
    lcm = S.make("lcm")
    assert isinstance(lcm, S.LCM) and lcm.stochastic is True and lcm.name == "lcm" and lcm.default_steps == 4
    assert (lcm.original_steps, lcm.timestep_scaling, lcm.sigma_data) == (50, 10.0, 0.5)
    with pytest.raises(ValueError, match="lcm"):
        S.make("unipc")
    assert S.Schedule._fields == ("sampler", "timesteps", "alphas", "alphas_prev", "coeffs")
    # the two hooks leave the existing tables and walks bit-identical to their table functions on the reference's walk
    ac = S.get_alphas_cumprod().astype(np.float64)
    for kind, fn, n in ((S.DDIM(0.3), lambda a: S.ddim_coefficients(a, 0.3), 50), (S.EulerAncestral(), S.euler_ancestral_coefficients, 30),
                        (S.DPMSolverPP2M(), S.dpmpp_2m_coefficients, 20)):
        sch = kind.schedule(n)
        ts = list(range(1, 1000, 1000 // n))[::-1]
        assert sch.timesteps == ts and np.array_equal(sch.coeffs, fn(np.concatenate([ac[ts], [1.0]])))


def test_variance_recursion_guards_the_noise_coefficient():
    """tests/test_gpu_samplers.py::test_ancestral_noise_is_fresh_every_step on the host with numpy noise: data N(0, s2) with the exact Gaussian
    denoiser makes the update x' = m_i x + c_n z, so the sample variance follows var' = m_i^2 var + c_n^2 exactly when z is fresh and c_n has the
    table's scale (a wrong sign convention or a squared c_n shows at once); c_n^2 itself is the noise of level a_s, 1 - a_s."""
    s2, n = 0.5, 1 << 18
    sch = S.LCM().schedule(8)
    rng = np.random.default_rng(8)
    x = rng.standard_normal(n)
    var = float(x.var())
    for i in range(len(sch.timesteps)):
        a_t = sch.alphas[i]
        sig2 = (1 - a_t) / a_t
        shrink = s2 / (s2 + sig2) / np.sqrt(a_t)
        x0 = x * shrink
        c_x, c_0, c_1, c_n = sch.coeffs[i]
        assert c_1 == 0.0 and c_n >= 0.0
        x = c_x * x + c_0 * x0 + c_n * rng.standard_normal(n)
        m = c_x + c_0 * shrink
        var = m * m * var + c_n * c_n
        assert abs(float(x.var()) / var - 1) < 0.015, (i, float(x.var()), var)
        assert abs(c_n * c_n - (1.0 - sch.alphas_prev[i])) < 1e-12                 # the noise of level a_s, not more, not less


# ---- compile(..., cfg=False): the refusals of variants/inputs.py, before any device work -------------------------------------------------
class _Untouchable:
    """A latent that fails the test when anything reads it."""
    def __getattr__(self, name):
        raise AssertionError(f"check_compile touched latent.{name}")


def _config(cfg_parallel=False, dtype="fp16", parallel_branches=False):
    return types.SimpleNamespace(cfg_parallel=cfg_parallel, dtype=dtype, parallel_branches=parallel_branches, is_bf16=lambda: dtype == "bf16")


def test_check_compile_refusals_of_the_guidance_free_step():
    sch = S.LCM().schedule(4)
    lat = _Untouchable()
    with pytest.raises(ValueError, match="cfg=False needs a sampler schedule"):
        I.check_compile(4, False, _config(), lat, None, False, None, False, cfg=False)
    with pytest.raises(ValueError, match="concat='edit'"):
        I.check_compile(8, False, _config(), lat, sch, False, "edit", False, cfg=False)
    with pytest.raises(S.UnsupportedSamplerConfig, match="TF_CFG_PARALLEL"):
        I.check_compile(4, False, _config(cfg_parallel=True), lat, sch, False, None, False, cfg=False)
    with pytest.raises(S.UnsupportedSamplerConfig, match="fp8"):
        I.check_compile(4, False, _config(dtype="fp8"), lat, sch, False, None, False, cfg=False)
    # what it composes with passes: plain, inpaint, the bf16 step, a ControlNet, the inpainting checkpoint
    lat4 = types.SimpleNamespace(shape=(2, 4, 16, 16))
    I.check_compile(4, False, _config(), lat, sch, False, None, False, cfg=False)
    I.check_compile(4, False, _config(), lat, sch, True, None, False, cfg=False)
    I.check_compile(4, False, _config(dtype="bf16"), lat, sch, False, None, False, cfg=False)
    I.check_compile(4, True, _config(), lat, sch, True, None, True, cfg=False)
    I.check_compile(9, False, _config(), lat4, sch, False, "inpaint", False, cfg=False)
    # the existing refusals still speak for a cfg=False model
    with pytest.raises(ValueError, match="attach_control"):
        I.check_compile(4, False, _config(), lat, sch, False, None, True, cfg=False)
    with pytest.raises(ValueError, match="in_channels=9"):
        I.check_compile(9, False, _config(), lat, sch, False, None, False, cfg=False)


def test_check_compile_default_is_the_cfg_step_as_before():
    sch = S.DPMSolverPP2M().schedule(10)
    lat = _Untouchable()
    I.check_compile(4, False, _config(), lat, None, False, None, False)                     # the DDIM step(): no sampler needed
    I.check_compile(4, False, _config(dtype="fp8"), lat, sch, False, None, False)            # fp8 with a sampler
    I.check_compile(4, False, _config(cfg_parallel=True), lat, None, False, None, False)     # the two-chain DDIM step
    I.check_compile(8, False, _config(), types.SimpleNamespace(shape=(1, 4, 8, 8)), sch, False, "edit", False, cfg=True)
    with pytest.raises(S.UnsupportedSamplerConfig):
        I.check_compile(4, False, _config(cfg_parallel=True), lat, sch, False, None, False)
    with pytest.raises(ValueError, match="inpaint=True needs a sampler"):
        I.check_compile(4, False, _config(), lat, None, True, None, False)
    with pytest.raises(TypeError):
        I.check_compile(4, False, _config(), lat, "lcm", False, None, False)
