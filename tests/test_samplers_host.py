"""Host checks of tinyfusers_amd/variants/samplers.py (no GPU): every coefficient table against an independent restatement of its
sampler, the order of accuracy of DDIM and DPM-Solver++(2M) on Gaussian data, schedule validation, and the numpy Philox4x32-10 the GPU
tests use as the reference of the device generator (csrc/sampler.hip) against the Random123 known-answer vectors."""
import numpy as np
import pytest

from tinyfusers_amd.variants import samplers as S

# ---- numpy restatement of the device generator (tests/test_gpu_samplers.py imports these) -------------------------------------------
_M0, _M1, _W0, _W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al. 2011).  ctr: (..., 4) uint32, key: (2,) uint32 -> (..., 4) uint32."""
    c = np.array(ctr, dtype=np.uint32, copy=True)
    k0, k1 = np.uint32(key[0]), np.uint32(key[1])
    mask = np.uint64(0xFFFFFFFF)
    with np.errstate(over="ignore"):
        for r in range(10):
            if r:
                k0, k1 = np.uint32(k0 + _W0), np.uint32(k1 + _W1)
            p0 = c[..., 0].astype(np.uint64) * _M0
            p1 = c[..., 2].astype(np.uint64) * _M1
            hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & mask).astype(np.uint32)
            hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & mask).astype(np.uint32)
            c = np.stack([hi1 ^ c[..., 1] ^ k0, lo1, hi0 ^ c[..., 3] ^ k1, lo0], axis=-1)
    return c


def randn_ref(seed, image, n_img, step, tag):
    """float64 N(0,1) of one image as the device draws it: counter (q, image, step, tag), key = the 64-bit seed, counter q -> elements
    4q .. 4q+3, u = ((bits >> 8) + 0.5) 2^-24, Box-Muller on (u0, u1) and (u2, u3)."""
    nq = (n_img + 3) // 4
    ctr = np.zeros((nq, 4), np.uint32)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = np.arange(nq, dtype=np.uint32), image, step, tag
    bits = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    u = ((bits >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    r01, r23 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    z = np.stack([r01 * np.cos(2 * np.pi * u[:, 1]), r01 * np.sin(2 * np.pi * u[:, 1]),
                  r23 * np.cos(2 * np.pi * u[:, 3]), r23 * np.sin(2 * np.pi * u[:, 3])], axis=1)
    return z.reshape(-1)[:n_img]


def apply(row, x, x0, x0_prev, z):
    c_x, c_0, c_1, c_n = row
    return c_x * x + c_0 * x0 + c_1 * x0_prev + c_n * z


# ---- 1. each table against an independent restatement ------------------------------------------------------------------------------
def _close(got, ref):
    assert np.all(np.abs(got - ref) <= 1e-12 * (1.0 + np.abs(ref))), float(np.max(np.abs(got - ref) / (1.0 + np.abs(ref))))


def test_ddim0_is_the_reference_update_at_every_step():
    """variants/sd.py:14-25: pred_x0 = (x - sqrt(1-a_t) e) / sqrt(a_t), x_prev = sqrt(a_prev) pred_x0 + sqrt(1-a_prev) e."""
    sch = S.DDIM().schedule(50)
    assert sch.timesteps == list(range(1, 1000, 20))[::-1]
    ac = S.get_alphas_cumprod()
    assert np.array_equal(sch.alphas, ac[sch.timesteps].astype(np.float64)) and sch.alphas_prev[-1] == 1.0
    assert np.array_equal(sch.alphas_prev[:-1], sch.alphas[1:])
    rng = np.random.default_rng(0)
    for i, (a_t, a_p) in enumerate(zip(sch.alphas, sch.alphas_prev)):
        x, e, xp, z = rng.standard_normal((4, 256))
        x0 = (x - np.sqrt(1 - a_t) * e) / np.sqrt(a_t)
        ref = np.sqrt(a_p) * x0 + np.sqrt(1 - a_p) * e
        assert sch.coeffs[i, 2] == 0.0 and sch.coeffs[i, 3] == 0.0
        _close(apply(sch.coeffs[i], x, x0, xp, z), ref)


@pytest.mark.parametrize("eta", [0.3, 1.0])
def test_ddim_eta_is_eq12_with_eq16_sigma(eta):
    """Song et al. 2021 eq. 12: x_{t-1} = sqrt(a_{t-1}) x0 + sqrt(1 - a_{t-1} - sigma^2) e + sigma z, eq. 16:
    sigma = eta sqrt((1 - a_{t-1}) / (1 - a_t)) sqrt(1 - a_t / a_{t-1})."""
    sch = S.DDIM(eta).schedule(50)
    rng = np.random.default_rng(1)
    assert np.all(sch.coeffs[:-1, 3] > 0) and sch.coeffs[-1, 3] == 0.0
    for i, (a_t, a_p) in enumerate(zip(sch.alphas, sch.alphas_prev)):
        x, e, xp, z = rng.standard_normal((4, 256))
        x0 = (x - np.sqrt(1 - a_t) * e) / np.sqrt(a_t)
        sigma = eta * np.sqrt((1 - a_p) / (1 - a_t) * (1 - a_t / a_p))
        ref = np.sqrt(a_p) * x0 + np.sqrt(max(1 - a_p - sigma ** 2, 0.0)) * e + sigma * z
        _close(apply(sch.coeffs[i], x, x0, xp, z), ref)


@pytest.mark.parametrize("eta", [1.0, 0.5])
def test_euler_ancestral_is_k_diffusion_in_sigma_form(eta):
    """k-diffusion sample_euler_ancestral on x_k = x / sqrt(a), sigma = sqrt((1 - a) / a), denoised = x0; back to VP by sqrt(a_s)."""
    sch = S.EulerAncestral(eta).schedule(30)
    rng = np.random.default_rng(2)
    for i, (a_t, a_p) in enumerate(zip(sch.alphas, sch.alphas_prev)):
        x, e, xp, z = rng.standard_normal((4, 256))
        x0 = (x - np.sqrt(1 - a_t) * e) / np.sqrt(a_t)
        s_from, s_to = np.sqrt((1 - a_t) / a_t), np.sqrt((1 - a_p) / a_p)
        s_up = min(s_to, eta * (s_to ** 2 * (s_from ** 2 - s_to ** 2) / s_from ** 2) ** 0.5)
        s_down = (s_to ** 2 - s_up ** 2) ** 0.5
        xk = x / np.sqrt(a_t)
        d = (xk - x0) / s_from
        xk = xk + d * (s_down - s_from) + z * s_up
        _close(apply(sch.coeffs[i], x, x0, xp, z), xk * np.sqrt(a_p))


def test_dpmpp_2m_is_algorithm_2_in_lambda_form():
    """DPM-Solver++ (Lu et al. 2022) Algorithm 2: lambda = log(alpha / sigma), h_i = lambda_i - lambda_{i-1}, r_i = h_{i-1} / h_i,
    D = (1 + 1/(2 r)) x0_i - 1/(2 r) x0_{i-1}, x_i = (sigma_i / sigma_{i-1}) x - alpha_i (e^{-h_i} - 1) D; first order on the first step and
    on the last (into sigma = 0, where x = x0)."""
    sch = S.DPMSolverPP2M().schedule(20)
    rng = np.random.default_rng(3)
    n = len(sch.timesteps)
    assert sch.coeffs[0, 2] == 0.0 and sch.coeffs[-1].tolist() == [0.0, 1.0, 0.0, 0.0] and np.all(sch.coeffs[1:-1, 2] != 0)
    assert np.all(sch.coeffs[:, 3] == 0.0)
    lam = lambda a: np.log(np.sqrt(a) / np.sqrt(1 - a)) if a < 1 else np.inf
    x = rng.standard_normal(256)
    x0_prev, h_prev = None, None
    for i, (a_t, a_p) in enumerate(zip(sch.alphas, sch.alphas_prev)):
        e = rng.standard_normal(256)
        x0 = (x - np.sqrt(1 - a_t) * e) / np.sqrt(a_t)
        if a_p == 1.0:
            ref = x0
        else:
            h = lam(a_p) - lam(a_t)
            D = x0 if x0_prev is None else (1 + 1 / (2 * (h_prev / h))) * x0 - 1 / (2 * (h_prev / h)) * x0_prev
            ref = np.sqrt(1 - a_p) / np.sqrt(1 - a_t) * x - np.sqrt(a_p) * (np.exp(-h) - 1) * D
            h_prev = h
        got = apply(sch.coeffs[i], x, x0, x0_prev if x0_prev is not None else np.zeros(256), np.zeros(256))
        _close(got, ref)
        x, x0_prev = ref, x0
    assert i == n - 1


# ---- 2. order of accuracy on Gaussian data ----------------------------------------------------------------------------------------
def _gaussian_error(table_fn, n, s2=0.5):
    """Data N(0, s2): exact denoiser D(x_k, sigma) = x_k s2 / (s2 + sigma^2); the probability-flow ODE scales x_k by
    sqrt(s2 + sigma^2) / sqrt(s2 + sigma_0^2).  Error in x_k at the last (nonzero) sigma of t = linspace(999, 1, n + 1)."""
    ac = S.get_alphas_cumprod().astype(np.float64)
    a = np.interp(np.linspace(999, 1, n + 1), np.arange(1000), ac)
    C = table_fn(a)
    assert C.shape == (n, 4)
    sig = np.sqrt((1 - a) / a)
    xk0 = np.array([1.0, -0.7, 2.3])
    x, xp = xk0 * np.sqrt(a[0]), np.zeros(3)
    for i in range(n):
        x0 = x / np.sqrt(a[i]) * s2 / (s2 + sig[i] ** 2)
        x = C[i, 0] * x + C[i, 1] * x0 + C[i, 2] * xp
        xp = x0
    exact = xk0 * np.sqrt(s2 + sig[-1] ** 2) / np.sqrt(s2 + sig[0] ** 2)
    return float(np.max(np.abs(x / np.sqrt(a[-1]) - exact)))


def test_order_of_accuracy_on_gaussian_data():
    ns = (20, 40, 80, 160)
    ddim = [_gaussian_error(S.ddim_coefficients, n) for n in ns]
    dpm = [_gaussian_error(S.dpmpp_2m_coefficients, n) for n in ns]
    r_ddim = [ddim[i] / ddim[i + 1] for i in (1, 2)]
    r_dpm = [dpm[i] / dpm[i + 1] for i in (1, 2)]
    print("error ratios per doubling, n = 40 -> 80 -> 160: DDIM", r_ddim, "DPM++2M", r_dpm)
    assert all(1.8 <= r <= 2.2 for r in r_ddim), r_ddim          # first order
    assert all(r >= 2.8 for r in r_dpm), r_dpm                    # second order (approaching 4)
    assert all(p < d for p, d in zip(dpm, ddim)), (dpm, ddim)


# ---- 3. the numpy Philox against the Random123 known-answer vectors -------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,want", [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_numpy_philox_known_answers(ctr, key, want):
    got = philox4x32_10(np.array([ctr], np.uint32), key)[0]
    assert " ".join(f"{int(v):08x}" for v in got) == want


def test_randn_ref_is_standard_normal():
    z = randn_ref(7, 0, 1 << 18, 0, 0)
    assert abs(z.mean()) < 1e-2 and abs(z.var() - 1) < 1e-2
    assert not np.array_equal(z[:64], randn_ref(7, 1, 64, 0, 0)) and not np.array_equal(z[:64], randn_ref(7, 0, 64, 0, 1))
    assert np.array_equal(randn_ref(7, 0, 10, 0, 0), z[:10])


# ---- 4. validation, finiteness -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [S.DDIM(), S.DDIM(1.0), S.DDIM(2.5), S.EulerAncestral(), S.EulerAncestral(0.5), S.DPMSolverPP2M()])
def test_every_coefficient_is_finite_for_every_step_count(kind):
    for steps in range(1, 1001):
        sch = kind.schedule(steps)
        n = len(sch.timesteps)
        assert sch.coeffs.shape == (n, 4) and sch.coeffs.dtype == np.float64
        assert np.isfinite(sch.coeffs).all(), (kind, steps)
        assert sch.alphas_prev[-1] == 1.0
        # into a_s = 1 every sampler lands on the data prediction
        np.testing.assert_allclose(sch.coeffs[-1], [0.0, 1.0, 0.0, 0.0], atol=1e-12)


def test_schedule_validation():
    with pytest.raises(ValueError):
        S.DDIM().schedule(0)
    with pytest.raises(ValueError):
        S.DDIM(-0.1)
    with pytest.raises(ValueError):
        S.EulerAncestral(float("nan"))
    for bad in ([500, 500, 1], [1, 500], [1000, 10], [10, -1], [], [5.5, 1]):
        with pytest.raises(ValueError):
            S.DPMSolverPP2M().schedule(timesteps=bad)
    with pytest.raises(ValueError):
        S.ddim_coefficients([0.5, 0.4])                            # alpha-bar must increase along the walk
    with pytest.raises(ValueError):
        S.dpmpp_2m_coefficients([0.5])
    sch = S.DPMSolverPP2M().schedule(timesteps=[999, 500, 0])
    assert sch.timesteps == [999, 500, 0] and sch.coeffs.shape == (3, 4)
    assert S.DPMSolverPP2M().schedule().timesteps == S.default_timesteps(20)
    assert S.make("ddim-eta", 0.5).eta == 0.5 and isinstance(S.make("dpmpp2m"), S.DPMSolverPP2M)
    with pytest.raises(ValueError):
        S.make("unipc")
