"""The two sampler entries perturbed-attention guidance adds to csrc/sampler.hip, in float16 and bfloat16, at the sizes
tests/test_gpu_elementwise_planted.py walks its step kernel over (elementwise_planted.DDIM_CASES: one pixel, odd planes, one block, and 526336
elements -- past one trip of the tail's capped grid):

  * tf_latent_stack3_*: the latent alone into three guidance groups (k_latent_stack<T, 3> with no conditioning channels) -- every group the
    round-to-nearest-even of the fp32 latent, bit for bit, groups 0 and 1 also bit for bit what tf_cfg_duplicate_* writes; guard words untouched.
  * tf_cfg3_sampler_step_masked_*: the three-group combine, the sampler update and the inpainting blend (k_sampler_step<T, 3, true>) against
    float64 under that file's kind of budget, tol = A = K_DDIM 2^-22 scale (fp32 outputs), the scale its DDIM one extended term by term to
    this update (every fp32 product-sum is bounded by the sum of the magnitudes that enter it):
        E     = |e0| + g_T (|e2| + |e1|) + g_I (|e1| + |e0|)                      e = e0 + g_T (e2 - e1) + g_I (e1 - e0)
        X0    = (|x| + sqrt(1 - a_t) E) / sqrt(a_t)                               x0 = (x - sqrt(1 - a_t) e) / sqrt(a_t)
        scale = 1 + m (|c_x| |x| + |c_0| X0 + |c_1| |h| + |c_n| |z|) + (1 - m) (sqrt(a_s) |x0_init| + sqrt(1 - a_s) |z2|)
    (x0 itself, the history output, is held to K_DDIM 2^-22 (1 + X0)), plus what the device's fp32 normals may differ from the float64 ones by,
    2e-6 (1 + |z|) per draw -- the figure tests/test_gpu_img2img.py holds the kept pixels to -- times the factor the draw enters with.  Mask 1
    everywhere gives tf_cfg3_sampler_step_*'s bits, mask 0 on the last row x0_init exactly, and the entry refuses a missing pointer."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "aux"))

import elementwise_planted as P  # noqa: E402
from test_samplers_host import randn_ref  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 0x243F6A8885A308D3
G, S_T = 7.5, 3.0                       # the CFG scale and a PAG scale: g_I = g, g_T = g + s_t
Z_TOL = 2e-6                            # device fp32 normal against the float64 one, per (1 + |z|): tests/test_gpu_img2img.py's kept-pixel gate
GUARD, FILL = 64, 0x3A55


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T
    T.ensure_init(0)
    return T


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("B,C,H,W", P.DDIM_CASES)
def test_three_groups_of_the_latent_alone(tf, B, C, H, W, dtype):
    from tinyfusers_amd.native import hip, lib
    from tinyfusers_amd.storage.tensor import bfloat16
    dt = bfloat16 if dtype == "bf16" else np.float16
    rng = np.random.default_rng([7, B, C, H, W])
    lat = (rng.standard_normal((B, C, H, W)) * rng.choice([1e-3, 1.0, 40.0], (B, C, H, W))).astype(np.float32)
    want = P.to_bits(np.ascontiguousarray(lat.transpose(0, 2, 3, 1)), dtype).reshape(-1)          # NHWC, rounded to nearest even
    n = want.size
    d_lat = tf.DeviceArray.from_numpy(lat, np.float32, "row")
    raw = tf.DeviceArray.from_numpy(np.full(3 * n + GUARD, FILL, np.uint16), np.uint16, "row")
    getattr(hip, "tf_latent_stack3_" + ("bf16" if dtype == "bf16" else "f16"))(raw.ptr, d_lat.ptr, B, C, H, W, None)
    got = raw.numpy()
    assert (got[3 * n:] == FILL).all(), "guard words behind the three groups overwritten"
    for g in range(3):
        assert np.array_equal(got[g * n:(g + 1) * n], want), f"group {g}"
    pair = tf.DeviceArray.empty((2 * B, C, H, W), dt, "nhwc")
    getattr(hip, "tf_cfg_duplicate_" + ("bf16" if dtype == "bf16" else "f16"))(pair.ptr, d_lat.ptr, B, C, H, W, None)
    hip.tf_stream_sync(None)
    two = tf.DeviceArray(pair.ptr, (2 * n,), np.uint16, "row", base=pair).numpy()
    assert np.array_equal(two, got[:2 * n])
    # the argument rule: cfg_duplicate's
    entry = getattr(lib, "tf_latent_stack3_" + ("bf16" if dtype == "bf16" else "f16"))
    before = raw.numpy().copy()
    for bad in ((None, d_lat.ptr, B, C, H, W), (raw.ptr, None, B, C, H, W), (raw.ptr, d_lat.ptr, 0, C, H, W), (raw.ptr, d_lat.ptr, B, 0, H, W), (raw.ptr, d_lat.ptr, B, C, -1, W)):
        assert entry(*bad, None) == P.TF_E_ARG and b"tf_latent_stack3" in lib.tf_last_error()
    assert entry(raw.ptr, d_lat.ptr, B, C, 0, W, None) == 0                                     # nothing to do is no error
    assert np.array_equal(raw.numpy(), before)


def _ref(x, e3, hist, x0i, m, a_t, a_s, g_t, g_i, row, z, z2):
    """float64 update and its budgets (module docstring)."""
    b = x.shape[0]
    e0, e1, e2 = e3[:b], e3[b:2 * b], e3[2 * b:]
    a_t, a_s = np.float64(np.float32(a_t)), np.float64(np.float32(a_s))
    c_x, c_0, c_1, c_n = (np.float64(np.float32(c)) for c in row)
    e = e0 + g_t * (e2 - e1) + g_i * (e1 - e0)
    x0 = (x - np.sqrt(1 - a_t) * e) / np.sqrt(a_t)
    xn = c_x * x + c_0 * x0 + (c_1 * hist if c_1 != 0 else 0.0) + c_n * z
    known = np.sqrt(a_s) * x0i + np.sqrt(1 - a_s) * z2
    E = np.abs(e0) + g_t * (np.abs(e2) + np.abs(e1)) + g_i * (np.abs(e1) + np.abs(e0))
    X0 = (np.abs(x) + np.sqrt(1 - a_t) * E) / np.sqrt(a_t)
    scale = 1 + m * (abs(c_x) * np.abs(x) + abs(c_0) * X0 + abs(c_1) * np.abs(hist) + abs(c_n) * np.abs(z)) + (1 - m) * (np.sqrt(a_s) * np.abs(x0i) + np.sqrt(1 - a_s) * np.abs(z2))
    A = P.K_DDIM * 2.0 ** -22 * scale + Z_TOL * (m * abs(c_n) * (1 + np.abs(z)) + (1 - m) * np.sqrt(1 - a_s) * (1 + np.abs(z2)))
    return m * xn + (1 - m) * known, x0, A, P.K_DDIM * 2.0 ** -22 * (1 + X0)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("B,C,H,W", P.DDIM_CASES)
def test_the_masked_three_group_tail_matches_float64(tf, B, C, H, W, dtype):
    from tinyfusers_amd.native import hip, lib
    from tinyfusers_amd.storage.tensor import bfloat16
    from tinyfusers_amd.variants import samplers as S
    dt = bfloat16 if dtype == "bf16" else np.float16
    sfx = "bf16" if dtype == "bf16" else "f32"
    masked, plain = getattr(hip, "tf_cfg3_sampler_step_masked_" + sfx), getattr(hip, "tf_cfg3_sampler_step_" + sfx)
    n_img, offset = C * H * W, 5
    rng = np.random.default_rng([9, B, C, H, W])
    x, hist, x0i = (rng.standard_normal((B, C, H, W)).astype(np.float32) for _ in range(3))
    m = rng.random((B, 1, H, W)).astype(np.float32)                   # fractional, with exact 0 and 1 pixels
    m.reshape(B, -1)[:, 0::5], m.reshape(B, -1)[:, 1::5] = 0.0, 1.0
    d_eps = tf.DeviceArray.from_numpy(rng.standard_normal((3 * B, C, H, W)), dt, "nhwc")
    e3 = d_eps.numpy().astype(np.float64)                             # the values the kernel reads
    sp, edit = tf.DeviceArray.zeros((8,), np.float32, "row"), tf.DeviceArray.zeros((4,), np.float32, "row")
    hip.tf_set_step_params(edit.ptr, G, 0.0, 0.0, 0.0, None)
    d_x0i = tf.DeviceArray.from_numpy(x0i, np.float32, "row")
    lo, hi = SEED & 0xFFFFFFFF, SEED >> 32
    for name in ("dpmpp2m", "euler-a"):
        sch = S.make(name).schedule(25, strength=0.8)
        i = 9
        table = sch.coeffs.copy()
        table[i, 2] = table[i, 2] or 0.25                              # the history is read
        assert (table[i, 3] != 0) == (name == "euler-a")               # the tag-1 noise: drawn for euler-a, not for DPM++2M
        d_tab = tf.DeviceArray.from_numpy(table.astype(np.float32), np.float32, "row")

        def run(row, mask, with_mask=True):
            lat, h = tf.DeviceArray.from_numpy(x, np.float32, "row"), tf.DeviceArray.from_numpy(hist, np.float32, "row")
            dm = tf.DeviceArray.from_numpy(mask, np.float32, "row")
            hip.tf_set_sampler_params(sp.ptr, float(sch.timesteps[row]), float(sch.alphas[row]), float(sch.alphas_prev[row]), G + S_T, row, lo, hi, offset, None, None, 0, None)
            if with_mask:
                masked(lat.ptr, d_eps.ptr, h.ptr, sp.ptr, d_tab.ptr, len(table), edit.ptr, d_x0i.ptr, dm.ptr, B, C, H, W, None)
            else:
                plain(lat.ptr, d_eps.ptr, h.ptr, sp.ptr, d_tab.ptr, len(table), edit.ptr, B, C, H, W, None)
            return lat.numpy(), h.numpy()

        z, z2 = (np.stack([randn_ref(SEED, offset + b, n_img, i, tag).reshape(C, H, W) for b in range(B)]) for tag in (1, 2))
        ref, ref_x0, A, A0 = _ref(x.astype(np.float64), e3, hist.astype(np.float64), x0i.astype(np.float64), m.astype(np.float64), sch.alphas[i], sch.alphas_prev[i],
                                  np.float64(np.float32(G + S_T)), G, table[i], z, z2)
        got, got_h = run(i, m)
        err, err0 = np.abs(got - ref), np.abs(got_h - ref_x0)
        print(f"\nmasked three-group tail {name} {dtype} {(B, C, H, W)}: worst err / budget latent {float((err / A).max()):.3f}, x0 {float((err0 / A0).max()):.3f}")
        assert np.isfinite(got).all() and (err <= A).all() and (err0 <= A0).all(), (float((err / A).max()), float((err0 / A0).max()))
        # mask 1 everywhere: the unmasked three-group update, bit for bit
        ones = np.ones_like(m)
        a, ah = run(i, ones)
        b_, bh = run(i, ones, with_mask=False)
        assert np.array_equal(a, b_) and np.array_equal(ah, bh)
        # the last row (a_s = 1) with mask 0: x0_init exactly
        last = len(table) - 1
        assert sch.alphas_prev[last] == 1.0
        fin, _ = run(last, np.zeros_like(m))
        assert np.array_equal(fin, x0i)
    # the entry's own pointers: edit_params, x0_init and mask all set
    raw = getattr(lib, "tf_cfg3_sampler_step_masked_" + sfx)
    lat = tf.DeviceArray.from_numpy(x, np.float32, "row")
    dm = tf.DeviceArray.from_numpy(m, np.float32, "row")
    args = [lat.ptr, d_eps.ptr, lat.ptr, sp.ptr, d_tab.ptr, len(table), edit.ptr, d_x0i.ptr, dm.ptr]
    for k in (0, 1, 2, 3, 4, 6, 7, 8):
        bad = list(args)
        bad[k] = None
        assert raw(*bad, B, C, H, W, None) == P.TF_E_ARG and b"tf_cfg3_sampler_step_masked" in lib.tf_last_error(), k
    assert raw(*args[:5], 0, *args[6:], B, C, H, W, None) == P.TF_E_ARG
    assert np.array_equal(lat.numpy(), x)
