"""Samplers beyond the reference's sigma = 0 DDIM update (variants/sd.py:14-25), all in ONE update form.

For step i (alpha-bar a_t -> a_s), in VP coordinates, with e the CFG-combined UNet output (variants/sd.py:44):

    x0  = (x - sqrt(1 - a_t) e) / sqrt(a_t)                 data prediction (variants/sd.py:20)
    x'  = c_x x + c_0 x0 + c_1 x0_prev + c_n z              z ~ N(0, 1) from the device's counter-based RNG
    x0_prev <- x0

Every sampler is a table of [c_x, c_0, c_1, c_n] per step, computed here in float64 from the alpha-bar sequence and uploaded
once; the device kernel (tf_cfg_sampler_step_*, csrc/sampler.hip) is the same for all of them.

  * DDIM(eta)          -- Song et al. 2021, eq. 12 with sigma from eq. 16; eta = 0 is the reference's update.
  * EulerAncestral(eta) -- k-diffusion's sample_euler_ancestral (sigma_up / sigma_down) with sigma = sqrt((1 - a) / a), x_k = x / sqrt(a).
  * DPMSolverPP2M()    -- Lu et al. 2022, DPM-Solver++ Algorithm 2 (multistep, lambda = log(alpha / sigma)); the first step and a
                          step into sigma = 0 (a_s = 1, lambda = inf) are first order.
  * LCM()              -- Luo et al. 2023, latent consistency models, multistep consistency sampling (Algorithm 3): the boundary-scaled
                          x0 prediction is re-noised to the next level at every step.  Its scalings depend on the timestep, not on
                          alpha-bar alone, and it walks its own timesteps (``Sampler.walk`` / ``Sampler.table`` are the two hooks).

``Sampler.schedule(steps)`` walks the reference's timesteps (example/sd1.py:54-57: range(1, 1000, 1000 // steps), high to low, a_prev = 1
after the last step) and returns a ``Schedule`` that ``StableDiffusion.compile(..., sampler=...)`` captures; ``schedule(steps, strength=s)``
is the image-to-image suffix of that walk.
"""
import math
from collections import namedtuple

import numpy as np

N_TRAIN = 1000

Schedule = namedtuple("Schedule", ["sampler", "timesteps", "alphas", "alphas_prev", "coeffs"])
Schedule.__doc__ = """timesteps (int, walk order, high to low), alphas / alphas_prev (float64 alpha-bar before / after each step, the last
alphas_prev = 1), coeffs ((n, 4) float64 [c_x, c_0, c_1, c_n] per step), sampler (the object that made it)."""


class UnsupportedSamplerConfig(RuntimeError):
    """A sampler cannot run in this step configuration (config.cfg_parallel, or a model compiled without / with another sampler)."""


def _abar(alphas_cumprod):
    a = np.asarray(alphas_cumprod, dtype=np.float64).reshape(-1)
    if a.size < 2:
        raise ValueError("samplers: an alpha-bar sequence needs at least two values (one step)")
    if not np.all(np.isfinite(a)) or np.any(a <= 0.0) or np.any(a > 1.0):
        raise ValueError("samplers: alpha-bar values must lie in (0, 1]")
    if np.any(np.diff(a) <= 0.0):
        raise ValueError("samplers: alpha-bar must increase strictly along the walk (timesteps strictly decreasing)")
    return a


def _check_eta(eta):
    eta = float(eta)
    if not np.isfinite(eta) or eta < 0.0:
        raise ValueError(f"samplers: eta must be finite and >= 0, got {eta}")
    return eta


def ddim_coefficients(alphas_cumprod, eta=0.0):
    """(n, 4) float64 table of DDIM(eta) for the n steps of an alpha-bar sequence a_0 < a_1 < ... < a_n (walk order).
    sigma_i = eta sqrt((1 - a_s) / (1 - a_t)) sqrt(1 - a_t / a_s)  (eq. 16);  x' = sqrt(a_s) x0 + sqrt(1 - a_s - sigma^2) e + sigma z  (eq. 12),
    with e = (x - sqrt(a_t) x0) / sqrt(1 - a_t)."""
    a, eta = _abar(alphas_cumprod), _check_eta(eta)
    a_t, a_s = a[:-1], a[1:]
    sigma = eta * np.sqrt((1.0 - a_s) / (1.0 - a_t)) * np.sqrt(1.0 - a_t / a_s)
    sigma = np.minimum(sigma, np.sqrt(1.0 - a_s))           # eta > 1 cannot take more noise than the target level holds
    c_x = np.sqrt(np.maximum(1.0 - a_s - sigma * sigma, 0.0)) / np.sqrt(1.0 - a_t)
    c_0 = np.sqrt(a_s) - np.sqrt(a_t) * c_x
    return np.stack([c_x, c_0, np.zeros_like(c_x), sigma], axis=1)


def euler_ancestral_coefficients(alphas_cumprod, eta=1.0):
    """(n, 4) float64 table of Euler-ancestral (k-diffusion) in VP coordinates.  sigma = sqrt((1 - a) / a), x_k = x / sqrt(a), D = x0:
    sigma_up = min(sigma_s, eta sqrt(sigma_s^2 (sigma_t^2 - sigma_s^2) / sigma_t^2)), sigma_down = sqrt(sigma_s^2 - sigma_up^2),
    x_k' = D + (sigma_down / sigma_t)(x_k - D) + sigma_up z, and x' = sqrt(a_s) x_k'."""
    a, eta = _abar(alphas_cumprod), _check_eta(eta)
    a_t, a_s = a[:-1], a[1:]
    sig_t, sig_s = np.sqrt((1.0 - a_t) / a_t), np.sqrt((1.0 - a_s) / a_s)
    sig_up = np.minimum(sig_s, eta * np.sqrt(sig_s ** 2 * (sig_t ** 2 - sig_s ** 2) / sig_t ** 2))
    sig_down = np.sqrt(np.maximum(sig_s ** 2 - sig_up ** 2, 0.0))
    ratio = sig_down / sig_t
    c_x = np.sqrt(a_s) / np.sqrt(a_t) * ratio
    c_0 = np.sqrt(a_s) * (1.0 - ratio)
    return np.stack([c_x, c_0, np.zeros_like(c_x), np.sqrt(a_s) * sig_up], axis=1)


def dpmpp_2m_coefficients(alphas_cumprod):
    """(n, 4) float64 table of DPM-Solver++(2M).  alpha = sqrt(a), sigma = sqrt(1 - a), lambda = log(alpha / sigma), h = lambda_s - lambda_t:
    x' = (sigma_s / sigma_t) x - alpha_s (e^-h - 1) D,  D = (1 + 1/(2r)) x0 - 1/(2r) x0_prev,  r = h_prev / h.
    First order (D = x0) on the first step and on a step into sigma_s = 0, where x' = x0."""
    a = _abar(alphas_cumprod)
    n = a.size - 1
    al, sg = np.sqrt(a), np.sqrt(1.0 - a)
    out = np.zeros((n, 4))
    h_prev = None
    for i in range(n):
        if sg[i + 1] == 0.0:                                       # into sigma = 0: lambda = inf, x' = x0
            out[i] = (0.0, 1.0, 0.0, 0.0)
            continue
        lam_t, lam_s = np.log(al[i] / sg[i]), np.log(al[i + 1] / sg[i + 1])
        h = lam_s - lam_t
        one_m = -np.expm1(-h)                                      # 1 - e^-h
        c_x = sg[i + 1] / sg[i]
        if h_prev is None:
            out[i] = (c_x, al[i + 1] * one_m, 0.0, 0.0)
        else:
            k = h / (2.0 * h_prev)                                 # 1 / (2r)
            out[i] = (c_x, al[i + 1] * one_m * (1.0 + k), -al[i + 1] * one_m * k, 0.0)
        h_prev = h
    return out


def lcm_timesteps(steps, original_steps=50):
    """The walk of the multistep consistency sampler: ``steps`` of the ``original_steps`` timesteps the model was distilled on, k = N_TRAIN //
    original_steps apart: t_i = k (original_steps - floor(i original_steps / steps)) - 1 -- with the defaults 999 - 20 floor(50 i / steps)."""
    steps, original_steps = int(steps), int(original_steps)
    if not 1 <= original_steps <= N_TRAIN:
        raise ValueError(f"samplers: original_steps must lie in [1, {N_TRAIN}], got {original_steps}")
    if not 1 <= steps <= original_steps:
        raise ValueError(f"samplers: an LCM walk takes 1 to original_steps = {original_steps} steps, got {steps}")
    k = N_TRAIN // original_steps
    return [k * (original_steps - (i * original_steps) // steps) - 1 for i in range(steps)]


def lcm_coefficients(alphas_cumprod, timesteps, timestep_scaling=10.0, sigma_data=0.5):
    """(n, 4) float64 table of the multistep consistency sampler for the n steps of an alpha-bar sequence (walk order) at ``timesteps``.
    With s = timestep_scaling t and sd = sigma_data: c_skip = sd^2 / (s^2 + sd^2), c_out = s / sqrt(s^2 + sd^2) (the boundary condition
    f(x, 0) = x), denoised = c_skip x + c_out x0, x' = sqrt(a_s) denoised + sqrt(1 - a_s) z -- fresh noise at every step but the last."""
    a = _abar(alphas_cumprod)
    t = np.asarray(timesteps, dtype=np.float64).reshape(-1)
    if t.size != a.size - 1:
        raise ValueError(f"samplers: {t.size} timesteps for the {a.size - 1} steps of the alpha-bar sequence")
    timestep_scaling, sigma_data = float(timestep_scaling), float(sigma_data)
    if not (np.isfinite(timestep_scaling) and timestep_scaling > 0.0 and np.isfinite(sigma_data) and sigma_data > 0.0):
        raise ValueError(f"samplers: timestep_scaling and sigma_data must be finite and > 0, got {timestep_scaling}, {sigma_data}")
    s, sd2 = timestep_scaling * t, sigma_data * sigma_data
    c_skip, c_out = sd2 / (s * s + sd2), s / np.sqrt(s * s + sd2)
    a_s = a[1:]
    return np.stack([np.sqrt(a_s) * c_skip, np.sqrt(a_s) * c_out, np.zeros_like(a_s), np.sqrt(1.0 - a_s)], axis=1)


def get_alphas_cumprod(beta_start=0.00085, beta_end=0.0120, n_training_steps=N_TRAIN):
    """variants/sd.py:61-65 (host fp32: a 1000-entry table, not device work)."""
    betas = np.linspace(beta_start ** 0.5, beta_end ** 0.5, n_training_steps, dtype=np.float32) ** 2
    alphas = 1.0 - betas
    return np.cumprod(alphas, axis=0)


def linear_alphas_cumprod(beta_start=0.00085, beta_end=0.0120, n_training_steps=N_TRAIN):
    """The LINEAR-beta training table (betas evenly spaced from beta_start to beta_end, where get_alphas_cumprod spaces their square roots): what the
    AnimateDiff motion modules were trained with.  To be handed to ``schedule(alphas_cumprod=)``; the default table stays get_alphas_cumprod's.  Host
    float64 products, returned as fp32 like the default table."""
    betas = np.linspace(beta_start, beta_end, n_training_steps, dtype=np.float64)
    return np.cumprod(1.0 - betas, axis=0).astype(np.float32)


def default_timesteps(steps):
    """example/sd1.py:54: range(1, 1000, 1000 // steps), walked high to low."""
    steps = int(steps)
    if steps < 1:
        raise ValueError(f"samplers: steps must be >= 1, got {steps}")
    return list(range(1, N_TRAIN, max(1, N_TRAIN // steps)))[::-1]


def _check_strength(strength):
    s = float(strength)
    if not 0.0 < s <= 1.0:                                         # (False for nan)
        raise ValueError(f"samplers: strength must lie in (0, 1], got {strength}")
    return s


def _check_timesteps(timesteps):
    ts = [int(t) for t in timesteps]
    if any(float(t) != float(u) for t, u in zip(ts, timesteps)):
        raise ValueError("samplers: timesteps must be integers")
    if not ts:
        raise ValueError("samplers: at least one timestep")
    if ts[0] > N_TRAIN - 1 or ts[-1] < 0:
        raise ValueError(f"samplers: timesteps must lie in [0, {N_TRAIN - 1}]")
    if any(b >= a for a, b in zip(ts, ts[1:])):
        raise ValueError("samplers: timesteps must decrease strictly (walk order, high to low)")
    return ts


class Sampler:
    name = "sampler"
    default_steps = 50
    stochastic = False

    def coefficients(self, alphas_cumprod):
        raise NotImplementedError

    def walk(self, steps):
        """The timesteps this sampler walks by default for ``steps`` steps (high to low): example/sd1.py:54's."""
        return default_timesteps(steps)

    def table(self, alphas_cumprod, timesteps):
        """The coefficient table of the kept walk: ``coefficients`` of its alpha-bar sequence; a sampler whose update depends on the timestep
        itself (LCM) reads ``timesteps`` too."""
        return self.coefficients(alphas_cumprod)

    def schedule(self, steps=None, timesteps=None, alphas_cumprod=None, strength=1.0):
        """The walk: timesteps (default ``walk(steps)``: example/sd1.py:54-57's, LCM its own), the alpha-bar pairs (a_prev = 1 after the last step) and the
        coefficient table.  ``alphas_cumprod``: the 1000-entry training table (default variants/sd.py:61-65's, fp32 like the reference's).
        ``strength`` in (0, 1]: image-to-image (SDEdit) keeps the last max(1, floor(n strength)) steps of the n-step walk, and the table is
        built on that truncated walk (DPM-Solver++(2M)'s first kept step is first order).  An img2img run starts at level ``alphas[0]``."""
        strength = _check_strength(strength)
        if timesteps is None:
            timesteps = self.walk(self.default_steps if steps is None else steps)
        elif steps is not None and int(steps) != len(timesteps):
            raise ValueError("samplers: pass steps or timesteps, not both")
        ts = _check_timesteps(timesteps)
        ac = np.asarray(get_alphas_cumprod() if alphas_cumprod is None else alphas_cumprod, dtype=np.float64)
        walk = np.concatenate([ac[ts], [1.0]])
        first = len(ts) - max(1, math.floor(len(ts) * strength))
        ts, walk = ts[first:], walk[first:]
        return Schedule(self, ts, walk[:-1].copy(), walk[1:].copy(), self.table(walk, ts))

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{k}={v}' for k, v in vars(self).items())})"


class DDIM(Sampler):
    name = "ddim"

    def __init__(self, eta=0.0):
        self.eta = _check_eta(eta)
        self.stochastic = self.eta > 0.0

    def coefficients(self, alphas_cumprod):
        return ddim_coefficients(alphas_cumprod, self.eta)


class EulerAncestral(Sampler):
    name = "euler-a"

    def __init__(self, eta=1.0):
        self.eta = _check_eta(eta)
        self.stochastic = self.eta > 0.0

    def coefficients(self, alphas_cumprod):
        return euler_ancestral_coefficients(alphas_cumprod, self.eta)


class DPMSolverPP2M(Sampler):
    name = "dpmpp2m"
    default_steps = 20

    def coefficients(self, alphas_cumprod):
        return dpmpp_2m_coefficients(alphas_cumprod)


class LCM(Sampler):
    name = "lcm"
    default_steps = 4
    stochastic = True

    def __init__(self, original_steps=50, timestep_scaling=10.0, sigma_data=0.5):
        self.original_steps = int(original_steps)
        self.timestep_scaling, self.sigma_data = float(timestep_scaling), float(sigma_data)
        lcm_timesteps(1, self.original_steps)                           # (checks original_steps)
        lcm_coefficients([0.5, 1.0], [1], self.timestep_scaling, self.sigma_data)     # (checks the two scalings)

    def walk(self, steps):
        return lcm_timesteps(steps, self.original_steps)

    def coefficients(self, alphas_cumprod, timesteps):
        return lcm_coefficients(alphas_cumprod, timesteps, self.timestep_scaling, self.sigma_data)

    def table(self, alphas_cumprod, timesteps):
        return self.coefficients(alphas_cumprod, timesteps)


def make(name, eta=None):
    """example/sd1.py's --sampler names: ddim, ddim-eta, dpmpp2m, euler-a, lcm."""
    if name == "ddim":
        return DDIM(0.0 if eta is None else eta)
    if name == "ddim-eta":
        return DDIM(1.0 if eta is None else eta)
    if name == "euler-a":
        return EulerAncestral(1.0 if eta is None else eta)
    if name == "dpmpp2m":
        return DPMSolverPP2M()
    if name == "lcm":
        return LCM()
    raise ValueError(f"unknown sampler {name!r} (ddim, ddim-eta, dpmpp2m, euler-a, lcm)")
