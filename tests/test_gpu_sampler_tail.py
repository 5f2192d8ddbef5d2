"""tf_sampler_tail_f32 / tf_sampler_tail_bf16 (csrc/sampler.hip): the closing launch of the captured step stated by `groups` and `flags` (bit 0
v-prediction, bit 1 the masked blend, bit 2 CFG rescale), at elementwise_planted.DDIM_CASES plus (2, 3, 5, 7), whose 105 elements per image are no
multiple of the Philox quad nor of the 8-element chunks of the statistics sweeps.  Guard words stand behind both outputs of every launch.

Budgets are tests/test_gpu_pag_step_kernels.py's construction with its constants (K_DDIM 2^-22 scale for the fp32 outputs, Z_TOL per draw), the
magnitudes from tests/aux/sd2_ref.py::tail: E term by term through the combine, X0 = sqrt(a_t) |x| + sqrt(1 - a_t) E for v.  With bit 2, E becomes
(phi f + 1 - phi) E and the relative error of f enters on top, DERIVED from the summation the kernel runs, not fitted:

    each sum of squared deviations adds, per thread, the n_t = 8 ceil(ceil(n_img / 8) / 1024) elements of its chunks one after the other, then 6
    butterfly levels across the wave, then the 16 wave partials one after the other: no term passes through more than D = n_t + 22 additions, and
    it enters as fl(fl(e - m)^2), three roundings.  All terms are >= 0, so rel(sum) <= (D + 3) u, u = 2^-24.  f = sqrt(q_t / q_e): HALF of the two
    sums' bounds after the square root, (D + 3) u together, plus 2 u for the division and the root.  The fp32 mean m' the deviations are taken
    from differs from the mean by at most (D + 2) u (mean |e - pivot| + |mean|), which adds (m' - m)^2 / var to a sum's relative error (two-pass:
    quadratic in u, also at |mean| = 8 std -- where a one-pass sum of squares would lose 64 (D + 3) u and fail this budget).  The device's e
    differs from the float64 one by at most 4 u E per element (the roundings of the combine), which moves std(e) by at most 4 u rms(E): relative
    4 u rms(E) / std(e), computed from the data in float64.  e_t is read, not computed: exact."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "aux"))

import elementwise_planted as P  # noqa: E402
import sd2_ref as R  # noqa: E402
from test_gpu_pag_step_kernels import Z_TOL  # noqa: E402
from test_samplers_host import randn_ref  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 0x243F6A8885A308D3
CASES = P.DDIM_CASES + [(2, 3, 5, 7)]
G, G_I = 7.5, 1.5
GUARD, FILL = 64, np.float32(-1234.5)
VPRED, MASKED, RESCALE = 1, 2, 4
U = 2.0 ** -24
_NORMALS = {}


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T
    T.ensure_init(0)
    return T


class Rig:
    """One problem: x, history, mask, x0_init, `groups` guidance groups in the 16-bit type, a schedule row; ``run`` launches an entry on guarded
    copies of x and the history and hands back (latent, history)."""

    def __init__(self, tf, shape, dtype, groups, name="dpmpp2m", eps=None, seed=0, offset=5, g=G):
        from tinyfusers_amd.native import hip
        from tinyfusers_amd.storage.tensor import bfloat16
        from tinyfusers_amd.variants import samplers as S
        self.tf, self.hip, self.shape, self.groups, self.dtype, self.offset, self.g = tf, hip, shape, groups, dtype, offset, g
        B, C, H, W = shape
        self.sfx = "bf16" if dtype == "bf16" else "f32"
        rng = np.random.default_rng([seed, B, C, H, W, groups])
        self.x, self.hist, self.x0i = (rng.standard_normal(shape).astype(np.float32) for _ in range(3))
        self.m = rng.random((B, 1, H, W)).astype(np.float32)
        self.m.reshape(B, -1)[:, 0::5], self.m.reshape(B, -1)[:, 1::5] = 0.0, 1.0
        if eps is None:
            eps = rng.standard_normal((groups * B, C, H, W)) * rng.choice([1e-3, 1.0, 40.0], (groups * B, C, H, W))
        self.d_eps = tf.DeviceArray.from_numpy(np.asarray(eps, np.float64), bfloat16 if dtype == "bf16" else np.float16, "nhwc")
        e = self.d_eps.numpy().astype(np.float64)                       # the values the kernel reads
        self.e = [e[k * B:(k + 1) * B] for k in range(groups)]
        self.sch = S.make(name).schedule(25, strength=0.8)
        self.row = 9
        self.table = self.sch.coeffs.copy()
        self.table[self.row, 2] = self.table[self.row, 2] or 0.25      # the history is read
        self.d_tab = tf.DeviceArray.from_numpy(self.table.astype(np.float32), np.float32, "row")
        self.sp, self.edit, self.phi = (tf.DeviceArray.zeros((n,), np.float32, "row") for n in (8, 4, 4))
        hip.tf_set_step_params(self.edit.ptr, G_I, 0.0, 0.0, 0.0, None)
        self.d_x0i, self.d_m = tf.DeviceArray.from_numpy(self.x0i, np.float32, "row"), tf.DeviceArray.from_numpy(self.m, np.float32, "row")
        self.set_row(self.row)

    def set_row(self, row, offset=None):
        lo, hi = SEED & 0xFFFFFFFF, SEED >> 32
        self.hip.tf_set_sampler_params(self.sp.ptr, float(self.sch.timesteps[row]), float(self.sch.alphas[row]), float(self.sch.alphas_prev[row]), self.g, row, lo, hi,
                                       self.offset if offset is None else offset, None, None, 0, None)

    def guarded(self, a):
        return self.tf.DeviceArray.from_numpy(np.concatenate([a.reshape(-1), np.full(GUARD, FILL, np.float32)]), np.float32, "row")

    def finish(self, lat, h):
        n = int(np.prod(self.shape))
        a, b = lat.numpy(), h.numpy()
        assert (a[n:] == FILL).all() and (b[n:] == FILL).all(), "guard words behind an output overwritten"
        return a[:n].reshape(self.shape), b[:n].reshape(self.shape)

    def tail(self, flags, phi=None, groups=None, eps=None):
        groups = self.groups if groups is None else groups
        lat, h = self.guarded(self.x), self.guarded(self.hist)
        if phi is not None:
            self.hip.tf_set_step_params(self.phi.ptr, float(phi), 0.0, 0.0, 0.0, None)
        masked = bool(flags & MASKED)
        getattr(self.hip, "tf_sampler_tail_" + self.sfx)(lat.ptr, (self.d_eps if eps is None else eps).ptr, h.ptr, self.sp.ptr, self.d_tab.ptr, len(self.table),
                                                         self.edit.ptr if groups == 3 else None, self.d_x0i.ptr if masked else None, self.d_m.ptr if masked else None,
                                                         self.phi.ptr if flags & RESCALE else None, *self.shape, groups, flags, None)
        return self.finish(lat, h)

    def old(self, masked, groups=None, eps=None):
        """The matching entry from before tf_sampler_tail_*."""
        groups = self.groups if groups is None else groups
        lat, h = self.guarded(self.x), self.guarded(self.hist)
        head = (lat.ptr, (self.d_eps if eps is None else eps).ptr, h.ptr, self.sp.ptr, self.d_tab.ptr, len(self.table))
        mk = (self.d_x0i.ptr, self.d_m.ptr)
        if groups == 1:
            getattr(self.hip, "tf_sampler_step1_" + self.sfx)(*head, *(mk if masked else (None, None)), *self.shape, None)
        elif groups == 2:
            getattr(self.hip, "tf_cfg_sampler_step_" + ("masked_" if masked else "") + self.sfx)(*head, *(mk if masked else ()), *self.shape, None)
        else:
            getattr(self.hip, "tf_cfg3_sampler_step_" + ("masked_" if masked else "") + self.sfx)(*head, self.edit.ptr, *(mk if masked else ()), *self.shape, None)
        return self.finish(lat, h)

    def normals(self, tag, offset=None):
        B, C, H, W = self.shape
        off = self.offset if offset is None else offset
        key = (B, C, H, W, off, self.row, tag)
        if key not in _NORMALS:                                           # (computed once per problem size: the big case draws 2^19 host normals)
            _NORMALS[key] = np.stack([randn_ref(SEED, off + b, C * H * W, self.row, tag).reshape(C, H, W) for b in range(B)])
        return _NORMALS[key]

    def reference(self, flags, phi=None):
        """(float64 result of sd2_ref.tail, latent budget, x0 budget) by the module docstring."""
        masked, cn = bool(flags & MASKED), self.table[self.row, 3]
        z = self.normals(1) if cn != 0 else np.zeros(self.shape)
        z2 = self.normals(2) if masked else np.zeros(self.shape)
        g = np.float64(np.float32(self.g))
        r = R.tail(self.x.astype(np.float64), self.e, self.hist.astype(np.float64), self.sch.alphas[self.row], self.sch.alphas_prev[self.row], g, self.table[self.row], z=z,
                   g_i=np.float64(np.float32(G_I)), phi=None if phi is None else np.float64(np.float32(phi)), vpred=bool(flags & VPRED),
                   x0_init=self.x0i.astype(np.float64) if masked else None, mask=self.m.astype(np.float64) if masked else None, z2=z2)
        a_t, a_s = np.float64(np.float32(self.sch.alphas[self.row])), np.float64(np.float32(self.sch.alphas_prev[self.row]))
        m = self.m.astype(np.float64) if masked else 1.0
        A = P.K_DDIM * 2.0 ** -22 * (1 + r["mag"]) + Z_TOL * (m * abs(cn) * (1 + np.abs(z)) + ((1 - m) * np.sqrt(1 - a_s) * (1 + np.abs(z2)) if masked else 0.0))
        A0 = P.K_DDIM * 2.0 ** -22 * (1 + r["X0"])
        if phi is not None:
            rel_f = self.rel_f(g)
            de = phi * r["f"] * np.abs(R.combine(self.e, g, G_I)[0]) * rel_f * (np.sqrt(1 - a_t) if flags & VPRED else np.sqrt(1 - a_t) / np.sqrt(a_t))
            A, A0 = A + m * abs(self.table[self.row, 1]) * de, A0 + de
            r["rel_f"] = rel_f
        return r, A, A0

    def rel_f(self, g):
        """The derived bound on f's relative error, per image (B, 1, 1, 1)."""
        B, n_img = self.shape[0], int(np.prod(self.shape[1:]))
        n_t = 8 * -(-(-(-n_img // 8)) // 1024)
        D = n_t + 22
        e, E, e_t = R.combine(self.e, g, G_I)
        out = []
        for b in range(B):
            eb, tb, Eb = e[b].reshape(-1), e_t[b].reshape(-1), E[b].reshape(-1)
            mean_terms = 0.0
            for v in (eb, tb):
                var = v.var()
                if var > 0:
                    mean_terms += ((D + 2) * U * (np.abs(v - v[0]).mean() + abs(v.mean()))) ** 2 / var
            se = eb.std()
            out.append((D + 3) * U + 2 * U + 0.5 * mean_terms + (4 * U * np.sqrt((Eb ** 2).mean()) / se if se > 0 else 0.0))
        return np.asarray(out).reshape(B, 1, 1, 1)


def _check(tag, got, got_h, r, A, A0):
    err, err0 = np.abs(got - r["latent"]), np.abs(got_h - r["x0"])
    print(f"\n{tag}: worst err / budget latent {float((err / A).max()):.3f}, x0 {float((err0 / A0).max()):.3f}" + (f", rel_f bound {float(r['rel_f'].max()):.2e}" if "rel_f" in r else ""))
    assert np.isfinite(got).all() and np.isfinite(got_h).all() and (err <= A).all() and (err0 <= A0).all(), (tag, float((err / A).max()), float((err0 / A0).max()))


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("B,C,H,W", CASES)
def test_flags_0_and_2_return_the_bits_of_the_existing_entries(tf, B, C, H, W, dtype):
    for groups in (1, 2, 3):
        for name in ("dpmpp2m", "euler-a"):
            rig = Rig(tf, (B, C, H, W), dtype, groups, name)
            for masked in (False, True):
                a, ah = rig.tail(MASKED if masked else 0)
                b, bh = rig.old(masked)
                assert np.array_equal(a, b) and np.array_equal(ah, bh), (groups, name, masked)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("B,C,H,W", CASES)
def test_v_prediction_matches_float64(tf, B, C, H, W, dtype):
    for groups in (1, 2, 3):
        for name in ("dpmpp2m", "euler-a"):
            rig = Rig(tf, (B, C, H, W), dtype, groups, name)
            for flags in (VPRED, VPRED | MASKED):
                got, got_h = rig.tail(flags)
                _check(f"v groups {groups} flags {flags} {name} {dtype} {(B, C, H, W)}", got, got_h, *rig.reference(flags))
            eps_form, _ = rig.tail(0)
            assert not np.array_equal(eps_form, rig.tail(VPRED)[0])                       # the bit is read


def _planted_mean(shape, groups, rng):
    """Every group = mean + noise with |mean| = 8 std, per image: means of both signs, deviations of three magnitudes."""
    B = shape[0]
    std = rng.choice([0.05, 1.0, 4.0], (groups * B, 1, 1, 1))
    return 8 * std * rng.choice([-1.0, 1.0], (groups * B, 1, 1, 1)) + std * rng.standard_normal((groups * B,) + tuple(shape[1:]))


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("B,C,H,W", CASES)
def test_cfg_rescale_matches_float64(tf, B, C, H, W, dtype):
    for groups in (2, 3):
        for kind in ("random", "planted-mean"):
            eps = _planted_mean((B, C, H, W), groups, np.random.default_rng([3, B, H, groups])) if kind == "planted-mean" else None
            rig = Rig(tf, (B, C, H, W), dtype, groups, "euler-a" if groups == 2 else "dpmpp2m", eps=eps)
            for flags, phi in ((RESCALE, 0.7), (RESCALE | VPRED, 0.7), (RESCALE | MASKED, 1.0), (RESCALE | VPRED | MASKED, 0.3)):
                got, got_h = rig.tail(flags, phi)
                _check(f"rescale {kind} groups {groups} flags {flags} phi {phi} {dtype} {(B, C, H, W)}", got, got_h, *rig.reference(flags, phi))
            if C * H * W > 4:
                assert not np.array_equal(rig.tail(RESCALE, 0.7)[0], rig.tail(0)[0])      # the word is read


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("B,C,H,W", [(2, 4, 8, 8), (2, 4, 257, 256)])
def test_cfg_rescale_exact_case(tf, B, C, H, W, dtype):
    """e_u = 0, e_t = +-1 in equal numbers per image, guidance 2, phi = 1: e = 2 e_t, f = 1/2, e' = e_t exactly -- the single-group update on e_t."""
    from tinyfusers_amd.storage.tensor import bfloat16
    dt = bfloat16 if dtype == "bf16" else np.float16
    rng = np.random.default_rng([5, H])
    et = np.ones((B, C * H * W)); et[:, :C * H * W // 2] = -1.0
    et = np.stack([rng.permutation(v) for v in et]).reshape(B, C, H, W)
    for name in ("dpmpp2m", "euler-a"):
        rig = Rig(tf, (B, C, H, W), dtype, 2, name, eps=np.concatenate([np.zeros_like(et), et]), g=2.0)
        one = tf.DeviceArray.from_numpy(et, dt, "nhwc")
        for extra in (0, VPRED, MASKED, VPRED | MASKED):
            a, ah = rig.tail(RESCALE | extra, 1.0)
            b, bh = rig.tail(extra, groups=1, eps=one)
            assert np.array_equal(a, b) and np.array_equal(ah, bh), (name, extra)
        c, ch = rig.tail(RESCALE, 1.0)
        d, dh = rig.old(False, groups=1, eps=one)                                         # tf_sampler_step1_* itself
        assert np.array_equal(c, d) and np.array_equal(ch, dh)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("B,C,H,W", CASES)
def test_phi_zero_is_the_call_without_the_bit_and_constant_images_have_f_one(tf, B, C, H, W, dtype):
    for groups in (2, 3):
        rig = Rig(tf, (B, C, H, W), dtype, groups, "euler-a")
        for extra in (0, VPRED, MASKED, VPRED | MASKED):
            a, ah = rig.tail(RESCALE | extra, 0.0)
            b, bh = rig.tail(extra)
            assert np.array_equal(a, b) and np.array_equal(ah, bh), (groups, extra)
        # every group constant per image (another constant per group and image): e is constant, f = 1, nothing non-finite
        vals = np.random.default_rng([8, groups]).choice([-3.0, -0.37, 0.11, 1.0, 25.0], (groups * B, 1, 1, 1))
        crig = Rig(tf, (B, C, H, W), dtype, groups, "dpmpp2m", eps=np.broadcast_to(vals, (groups * B, C, H, W)))
        for flags in (RESCALE, RESCALE | VPRED | MASKED):
            got, got_h = crig.tail(flags, 0.7)
            r, A, A0 = crig.reference(flags, 0.7)
            assert np.all(r["f"] == 1)
            _check(f"constant groups {groups} flags {flags} {dtype} {(B, C, H, W)}", got, got_h, r, A, A0)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_an_images_result_does_not_depend_on_the_batch(tf, dtype):
    for groups in (2, 3):
        rig = Rig(tf, (3, 4, 5, 7), dtype, groups, "euler-a")
        for flags in (RESCALE, RESCALE | VPRED | MASKED):
            all3, all3h = rig.tail(flags, 0.7)
            solo = Rig(tf, (1, 4, 5, 7), dtype, groups, "euler-a", eps=np.concatenate([e[1:2] for e in rig.e]))
            solo.x, solo.hist, solo.x0i, solo.m = rig.x[1:2], rig.hist[1:2], rig.x0i[1:2], rig.m[1:2]
            solo.d_x0i, solo.d_m = tf.DeviceArray.from_numpy(solo.x0i, np.float32, "row"), tf.DeviceArray.from_numpy(solo.m, np.float32, "row")
            solo.set_row(solo.row, offset=rig.offset + 1)                                 # image_offset + 1: the same global image
            one, oneh = solo.tail(flags, 0.7)
            assert np.array_equal(one[0], all3[1]) and np.array_equal(oneh[0], all3h[1]), (groups, flags)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_argument_rule(tf, dtype):
    from tinyfusers_amd.native import lib
    sfx = "bf16" if dtype == "bf16" else "f32"
    rig = Rig(tf, (2, 4, 8, 8), dtype, 3)
    raw = getattr(lib, "tf_sampler_tail_" + sfx)
    lat, h = rig.guarded(rig.x), rig.guarded(rig.hist)
    P_ = dict(latent=lat.ptr, eps=rig.d_eps.ptr, hist=h.ptr, sp=rig.sp.ptr, tab=rig.d_tab.ptr, edit=rig.edit.ptr, x0i=rig.d_x0i.ptr, mask=rig.d_m.ptr, phi=rig.phi.ptr)

    def call(groups, flags, rows=len(rig.table), shape=(2, 4, 8, 8), **over):
        p = dict(P_, **over)
        masked, resc = bool(flags & MASKED), bool(flags & RESCALE)
        args = [p["latent"], p["eps"], p["hist"], p["sp"], p["tab"], rows, p.get("edit_", p["edit"] if groups == 3 else None), p.get("x0i_", p["x0i"] if masked else None),
                p.get("mask_", p["mask"] if masked else None), p.get("phi_", p["phi"] if resc else None), *shape, groups, flags, None]
        return raw(*args)

    def refused(rc, word=None):
        msg = lib.tf_last_error()
        assert rc == P.TF_E_ARG and b"tf_sampler_tail_" + sfx.encode() in msg and (word is None or word in msg), (rc, msg)
    for k in ("latent", "eps", "hist", "sp", "tab"):                                      # the pointers every form needs
        refused(call(2, 0, **{k: None}))
    refused(call(2, 0, rows=0)); refused(call(2, 0, shape=(0, 4, 8, 8))); refused(call(2, 0, shape=(2, 4, 8, 0)))
    for groups in (0, 4, -1):
        refused(call(groups, 0, edit_=None), b"groups")
    refused(call(2, 8), b"flags"); refused(call(2, 0x10 | VPRED), b"flags")
    # x0_init and mask both set iff bit 1
    refused(call(2, MASKED, x0i_=None), b"x0_init and mask"); refused(call(2, MASKED, mask_=None), b"x0_init and mask"); refused(call(2, MASKED, x0i_=None, mask_=None), b"x0_init and mask")
    refused(call(2, 0, x0i_=P_["x0i"]), b"x0_init and mask"); refused(call(2, VPRED, mask_=P_["mask"]), b"x0_init and mask"); refused(call(1, 0, x0i_=P_["x0i"], mask_=P_["mask"]), b"x0_init and mask")
    # edit_params set iff groups == 3
    refused(call(3, 0, edit_=None), b"edit_params"); refused(call(2, 0, edit_=P_["edit"]), b"edit_params"); refused(call(1, VPRED, edit_=P_["edit"]), b"edit_params")
    # rescale set iff bit 2; bit 2 needs groups >= 2
    refused(call(2, RESCALE, phi_=None), b"rescale"); refused(call(3, RESCALE | VPRED, phi_=None), b"rescale"); refused(call(2, 0, phi_=P_["phi"]), b"rescale")
    refused(call(1, RESCALE), b"groups >= 2"); refused(call(1, RESCALE | VPRED | MASKED), b"groups >= 2")
    a, b = rig.finish(lat, h)
    assert np.array_equal(a, rig.x) and np.array_equal(b, rig.hist)                       # nothing was launched
    for groups, flags in ((1, 0), (1, VPRED | MASKED), (2, RESCALE | MASKED), (3, RESCALE | VPRED), (3, MASKED)):
        assert call(groups, flags) == 0, (groups, flags, lib.tf_last_error())
    rig.hip.tf_stream_sync(None)
