"""FreeU (Si et al. 2023, as diffusers' apply_freeu / fourier_filter state it) on the host -- TEST INFRASTRUCTURE for csrc/freeu.hip,
UNetModel.__call__(freeu=) and StableDiffusion.compile(..., freeu=True).  numpy and torch on the CPU only.

(a) fourier_filter / apply_freeu: the FFT restatement in float64 (torch.fft): fftn over (H, W), fftshift, the 2 x 2 box
    [H//2-1 : H//2+1, W//2-1 : W//2+1] times s, un-shift, ifftn, real part; h[:, :C/2] *= b.
(b) closed_form: with a = 2 pi i / H, b = 2 pi j / W and t = (1, cos a, sin a, cos b, sin b, cos(a+b), sin(a+b)),
    y = x + (s - 1) / (H W) sum_q S_q t_q, S_q = sum_ij x t_q -- the four bins (u, v) in {0, -1}^2 of the box written out (H, W >= 2).
(c) emulate: the kernel's own fp32 arithmetic in numpy -- twiddles rounded to fp32 from float64 sincospi; thread pg of 32 walks the pixels pg,
    pg + 32, ... with one fma per sum (a plain add for S_0); the 32 partials are added in ascending pg; the apply is S_0, six fmas, and
    fma(g, c, x), g = (s - 1) / (H W) in fp32.  An fma is float32(float64 product + float64 addend): the product is exact, and the second
    rounding differs from one rounding only at ties of the first.
(d) BUDGET per element of the float64 reference y:  tol = half_ulp(|y| + A) + A,
      half_ulp(v): half the spacing of the storage type at v (tests/aux/norm_planted.py's), the store rounding at the largest magnitude the
          unrounded result can have;
      A = 2^-22 (|y| + K |s - 1| m):  the fp32 arithmetic.  |y| 2^-22 covers the last fma's rounding (2^-24 |y|) with room; m = mean_ij |x| of
          the plane is the size of the correction's terms -- each S_q / (H W) is at most m, its rounding error a few 2^-24 m sqrt-ish in H W.
    K is fixed by the EMULATION, never by a device: the smallest integer for which the emulation's largest error is at most A / 2 on every case
    of CASES x SCALES x both storage types (so the device gets twice the emulation's error, and no more).  Measured with emulate() below as
    max over elements of (2 err / 2^-22 - |y|) / (|s - 1| m), the K a case needs (tests/test_freeu_host.py prints them per case):
        largest:  3.20  (B, H, W, C) = (3, 12, 12, 328) float16, s = 0.9        -> K_FREEU = 4      (3.20 <= 4)
        by scale: 2.37 at s = 0.2, 3.20 at s = 0.9, 2.82 at s = -0.5; s = 1 is exact (the kernel copies).
(e) unet_forward(..., freeu=, control=): oracle.unet_forward with a ControlNet's residuals (tests/aux/controlnet_oracle.py::unet_forward) and
    FreeU in front of the concats of output_blocks[0 : 2n], n = num_res_blocks + 1: stage k = block // n, the skip filtered AFTER the control
    residual is added.  freeu=None, control=None: oracle.unet_forward exactly.

PLANTED PLANES.  Seeded noise alone lets a kernel that uses its neighbour's sums pass, so every (image, channel) plane is a sum of a DC offset,
components at (u, v) in {0, +-1}^2 with distinct amplitudes and phases, components at frequency 2 and at Nyquist (which the filter must pass
unchanged), and noise; amplitudes and phases differ between adjacent channels and between images.  mutants() restates what a subtly wrong kernel
computes (a lost pixel tail, swapped axes, the neighbouring channel's or the next image's sums, the sine terms dropped): every one exceeds the
budget by two orders of magnitude or more on every case it can show on (the sines of a 2 x 2 plane are all zero).
"""
import math

import numpy as np
import torch

from oracle import ops
from oracle.unet import SD15, _graph

F32, F64 = np.float32, np.float64
K_FREEU = 4.0
CASES_HW = ((2, 2), (4, 4), (8, 8), (16, 16), (12, 12), (5, 7), (3, 8), (6, 4))
CASES_C = (8, 72, 328)                  # one vector, a ragged slab (9 vectors: a full 8-vector slab and one more), more than one slab
CASES_B = (1, 3)
SCALES = (0.2, 0.9, -0.5, 1.0)
PG = 32                                 # pixel groups of a block (csrc/freeu.hip: FU_PG)


# ---- storage types ---------------------------------------------------------------------------------------------------------------------------
def round16(x, dtype):
    """fp32 -> (uint16 bit patterns, the float64 values they hold), round to nearest even."""
    x = np.ascontiguousarray(x, dtype=F32)
    if dtype == "bf16":
        u = x.view(np.uint32)
        bits = ((u + (((u >> 16) & 1) + np.uint32(0x7FFF))) >> 16).astype(np.uint16)
        return bits, (bits.astype(np.uint32) << 16).view(F32).astype(F64)
    h = x.astype(np.float16)
    return h.view(np.uint16), h.astype(F64)


def from16(bits, dtype):
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    return ((bits.astype(np.uint32) << 16).view(F32) if dtype == "bf16" else bits.view(np.float16)).astype(F64)


def half_ulp(v, dtype):
    """half the spacing of the storage type at magnitude v (float64); fp16 floors at its subnormal spacing."""
    v = np.abs(np.asarray(v, F64))
    e = np.where(v > 0, np.frexp(v)[1] - 1, -1000)
    return np.ldexp(1.0, np.maximum(e - 11, -25)) if dtype == "fp16" else np.ldexp(1.0, np.maximum(e - 8, -140))


# ---- (a) the FFT restatement ---------------------------------------------------------------------------------------------------------------------
def fourier_filter(x, scale, threshold=1):
    """diffusers' fourier_filter in float64: x (B, C, H, W) -> the same shape."""
    x = torch.as_tensor(np.asarray(x, F64)) if not torch.is_tensor(x) else x.to(torch.float64)
    B, C, H, W = x.shape
    f = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones((B, C, H, W), dtype=torch.float64)
    crow, ccol = H // 2, W // 2
    mask[..., crow - threshold:crow + threshold, ccol - threshold:ccol + threshold] = scale
    return torch.fft.ifftn(torch.fft.ifftshift(f * mask, dim=(-2, -1)), dim=(-2, -1)).real


def apply_freeu(stage, hidden, skip, s1, s2, b1, b2):
    """diffusers' apply_freeu: stage 0 / 1 -> (hidden with its first half of the channels times b, the filtered skip); other stages untouched."""
    if stage not in (0, 1):
        return hidden, skip
    s, b = (s1, b1) if stage == 0 else (s2, b2)
    hidden = hidden.clone()
    hidden[:, :hidden.shape[1] // 2] = hidden[:, :hidden.shape[1] // 2] * b
    return hidden, fourier_filter(skip, s).to(skip.dtype)


# ---- (b) the closed form --------------------------------------------------------------------------------------------------------------------------
def _sincospi(a):
    """(sin, cos)(pi a) in float64 with the exact values at multiples of 1/2 (what sincospi returns)."""
    r = np.mod(np.asarray(a, F64), 2.0)
    s, c = np.sin(np.pi * r), np.cos(np.pi * r)
    s = np.where((r == 0) | (r == 1), 0.0, np.where(r == 0.5, 1.0, np.where(r == 1.5, -1.0, s)))
    c = np.where((r == 0.5) | (r == 1.5), 0.0, np.where(r == 0, 1.0, np.where(r == 1, -1.0, c)))
    return s, c


def twiddles(H, W, dt=F64):
    """t (7, H, W): (1, cos a, sin a, cos b, sin b, cos(a+b), sin(a+b)); dt = float32: the kernel's -- the four tables rounded to fp32, the two
    products as it forms them."""
    si, ci = _sincospi(2.0 * np.arange(H) / H)
    sj, cj = _sincospi(2.0 * np.arange(W) / W)
    si, ci, sj, cj = (v.astype(dt) for v in (si, ci, sj, cj))
    ci, si, cj, sj = ci[:, None], si[:, None], cj[None, :], sj[None, :]
    if dt == F32:
        cc, ss = _fma(ci, cj, -(si * sj)), _fma(si, cj, ci * sj)
    else:
        cc, ss = ci * cj - si * sj, si * cj + ci * sj
    one = np.ones((H, W), dt)
    return np.stack([one, ci * one, si * one, cj * one, sj * one, cc, ss]).astype(dt)


def closed_form(x, scale):
    """x (B, C, H, W) float64 -> y: the input plus the rank-4 correction from seven real sums per plane."""
    x = np.asarray(x, F64)
    B, C, H, W = x.shape
    if H < 2 or W < 2:
        raise ValueError(f"closed_form: the 2 x 2 box needs H >= 2 and W >= 2, got {x.shape}")
    t = twiddles(H, W)
    S = np.einsum("bchw,qhw->bcq", x, t)
    return x + (scale - 1.0) / (H * W) * np.einsum("bcq,qhw->bchw", S, t)


# ---- (c) the kernel's fp32 arithmetic ----------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def emulate_sums(x, t):
    """S (B, C, 7) fp32 as the kernel forms them: x (B, C, H, W) fp32 values, t = twiddles(H, W, float32)."""
    B, C, H, W = x.shape
    n = H * W
    m = -(-n // PG)
    xp = np.zeros((B, C, m * PG), F32); xp[..., :n] = x.reshape(B, C, n)              # fma(0, t, acc) = acc: the padding adds nothing
    tp = np.zeros((7, m * PG), F32); tp[:, :n] = t.reshape(7, n)
    xp, tp = xp.reshape(B, C, m, PG), tp.reshape(7, m, PG)
    acc = np.zeros((B, C, 7, PG), F32)
    for k in range(m):
        acc[:, :, 0] = acc[:, :, 0] + xp[:, :, k]
        for q in range(1, 7):
            acc[:, :, q] = _fma(xp[:, :, k], tp[q, k], acc[:, :, q])
    S = acc[..., 0].copy()
    for g in range(1, PG):
        S = S + acc[..., g]
    return S


def emulate(x, scale, dtype):
    """-> (the fp32 values in front of the store, the stored bit patterns).  scale 1: the copy."""
    x = np.ascontiguousarray(x, dtype=F32)
    B, C, H, W = x.shape
    if F32(scale) == F32(1.0):
        return x.copy(), round16(x, dtype)[0]
    t = twiddles(H, W, F32)
    S = emulate_sums(x, t)
    c = np.broadcast_to(S[:, :, 0, None, None], x.shape).astype(F32)
    for q in range(1, 7):
        c = _fma(S[:, :, q, None, None], t[q], c)
    g = F32(F32(scale) - F32(1.0)) / F32(H * W)
    y = _fma(g, c, x)
    return y, round16(y, dtype)[0]


# ---- (d) the budget -----------------------------------------------------------------------------------------------------------------------------------
def plane_mean_abs(x):
    return np.abs(np.asarray(x, F64)).mean(axis=(2, 3), keepdims=True)


def budget(y, x, scale, dtype, K=K_FREEU):
    """(tol, A) per element of the float64 reference y of the (rounded) input x (module docstring)."""
    A = 2.0 ** -22 * (np.abs(y) + K * abs(float(scale) - 1.0) * plane_mean_abs(x))
    return half_ulp(np.abs(y) + A, dtype) + A, A


def k_needed(err, y, x, scale):
    """the K at which the largest fp32 error `err` of a case equals A / 2 (0 where A / 2 holds it at K = 0)."""
    u = abs(float(scale) - 1.0) * plane_mean_abs(x)
    if float(scale) == 1.0:
        assert np.all(err <= 1e-13), "scale 1 is a copy: only the FFT restatement's own float64 rounding is left"
        return 0.0
    return float(np.max((2.0 * err / 2.0 ** -22 - np.abs(y)) / u).clip(0))


# ---- planted planes --------------------------------------------------------------------------------------------------------------------------------------
def planted(B, C, H, W, dtype, seed=0):
    """-> (uint16 bit patterns (B, C, H, W), the float64 values they hold)."""
    rng = np.random.default_rng([seed, B, C, H, W])
    i, j = np.arange(H)[:, None] / H, np.arange(W)[None, :] / W
    b, c = np.arange(B)[:, None, None, None], np.arange(C)[None, :, None, None]
    x = 0.75 * (1 + (c + 2 * b) % 4) * np.where((c + b) % 2, -1.0, 1.0)                    # DC: differs between neighbours in sign and size
    k = 0
    for u in (-1, 0, 1):
        for v in (-1, 0, 1):
            if (u, v) == (0, 0):
                continue
            k += 1
            amp = (0.5 + 0.3 * k) * (1 + ((3 * c + 5 * b + k) % 7) / 3.0)
            ph = 0.7 * k + 0.9 * c + 1.3 * b
            x = x + amp * np.cos(2 * np.pi * (u * i + v * j)[None, None] + ph)
    x = x + (1.0 + (c % 3)) * np.cos(2 * np.pi * (2 * i + 0 * j)[None, None] + 0.4 * c)     # frequency 2 on each axis: passes unchanged (H, W > 4)
    x = x + (0.8 + (b % 2)) * np.cos(2 * np.pi * (0 * i + 2 * j)[None, None] + 0.6 * c + 0.2)
    x = x + (0.6 + ((c + b) % 5) / 4.0) * np.where((np.arange(H)[:, None] + np.arange(W)[None, :]) % 2, -1.0, 1.0)   # Nyquist on both axes
    x = x + 0.25 * rng.standard_normal((B, C, H, W))
    return round16(x.astype(F32), dtype)


def mutants(x, scale):
    """name -> what a subtly wrong kernel would write for x (B, C, H, W) float64."""
    B, C, H, W = x.shape
    t = twiddles(H, W)
    g = (scale - 1.0) / (H * W)
    S = np.einsum("bchw,qhw->bcq", x, t)
    out = {}
    xt = x.copy().reshape(B, C, -1); xt[..., -1] = 0                                      # the last pixel never summed
    out["lost pixel tail"] = x + g * np.einsum("bcq,qhw->bchw", np.einsum("bcp,qp->bcq", xt, t.reshape(7, -1)), t)
    if C > 1:
        out["neighbour's sums"] = x + g * np.einsum("bcq,qhw->bchw", np.roll(S, 1, axis=1), t)
    if B > 1:
        out["next image's sums"] = x + g * np.einsum("bcq,qhw->bchw", np.roll(S, 1, axis=0), t)
    ts = t[[0, 3, 4, 1, 2, 5, 6]]                                                         # the two axes' tables swapped in the apply
    if H == W:
        out["swapped axes"] = x + g * np.einsum("bcq,qhw->bchw", S, ts)
    else:
        out["swapped axes"] = x + g * np.einsum("bcq,qhw->bchw", np.einsum("bchw,qwh->bcq", x, twiddles(W, H)), t)
    out["sine terms dropped"] = x + g * np.einsum("bcq,qhw->bchw", S[..., [0, 1, 3, 5]], t[[0, 1, 3, 5]])
    return out


# ---- (e) the UNet --------------------------------------------------------------------------------------------------------------------------------------
def stage_map(cfg):
    """[(stage, output block, backbone channels, skip channels, latent size divisor)] of the 2n FreeU blocks, from the oracle's graph."""
    inp, _, out = _graph(cfg)
    n = cfg.num_res_blocks + 1
    outc = lambda b: b[-1][2] if b[-1][0] in ("conv", "res") else b[-1][1]
    skips = [outc(b) for b in inp]
    rows, ch, nlev = [], outc(inp[-1]), len(cfg.channel_mult)
    for i in range(2 * n):
        sk = skips.pop()
        assert out[i][0][1] == ch + sk
        rows.append((i // n, i, ch, sk, 2 ** (nlev - 1 - i // n)))
        ch = out[i][0][2]
    return rows


def unet_forward(x, timesteps, context, W, cfg=SD15, head_merge="reference_exact", control=None, freeu=None):
    """oracle.unet_forward; control: the (scaled) residuals of a ControlNet, mid += r[-1] and cat(x, saved.pop() + r.pop()); freeu = (s1, s2, b1,
    b2): apply_freeu in front of the concat of output block i < 2n with stage i // n, on the skip as the concat would have read it."""
    from controlnet_oracle import _embed_time, _run
    W = {k: ops.as_t(v) for k, v in W.items()}
    x, context = ops.as_t(x), ops.as_t(context)
    emb = _embed_time(timesteps, W, cfg)
    inp, mid, out = _graph(cfg)
    r = [ops.as_t(v) for v in control] if control is not None else None
    n = cfg.num_res_blocks + 1
    saved = []
    for i, b in enumerate(inp):
        for j, l in enumerate(b):
            x = _run(x, l, f"input_blocks.{i}.{j}", emb, context, W, cfg, head_merge)
        saved.append(x)
    for j, l in enumerate(mid):
        x = _run(x, l, f"middle_block.{j}", emb, context, W, cfg, head_merge)
    if r is not None:
        assert len(r) == len(saved) + 1, (len(r), len(saved))
        x = x + r.pop()
    for i, b in enumerate(out):
        skip = saved.pop() + r.pop() if r is not None else saved.pop()
        if freeu is not None:
            x, skip = apply_freeu(i // n, x, skip, *freeu)
        x = torch.cat((x, skip), dim=1)
        for j, l in enumerate(b):
            x = _run(x, l, f"output_blocks.{i}.{j}", emb, context, W, cfg, head_merge)
    x = ops.silu(ops.group_norm_affine(x, cfg.num_groups, W["out.0.weight"], W["out.0.bias"]))
    return ops.conv2d_bias(x, W["out.2.weight"], W["out.2.bias"], (1, 1))


def cases():
    """every (B, H, W, C) of the table."""
    return [(B, H, W, C) for (H, W) in CASES_HW for C in CASES_C for B in CASES_B]


assert math.isclose(K_FREEU, round(K_FREEU))
