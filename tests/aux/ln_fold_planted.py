"""Planted row statistics for the LayerNorm fold of the GEMM families -- tf_linear_ln_16 on k_igemm (deep / wide / all-8 ring), k_igemm_pp,
k_gemm_c4, k_gemm_c8 and k_gemm_ar, and tf_ln_fold_weights_16 (k_ln_fold) -- their float64 answers, a numpy emulation of the kernels' fp32
arithmetic, the error budgets, the wrong answers a slipped kernel would give, and the case tables (host code, numpy only).
tests/test_ln_fold_planted_host.py checks every claim made here on the CPU; tests/test_gpu_ln_fold_planted.py walks the tables on the device.

INPUTS.  Row m of x holds mu_m + sigma_m z, z standardised per row, rounded to the storage type.  sigma_m = 2^((3 m + 1) mod 5 - 2) in [1/4, 4]
and mu_m = sigma_m R k_m / 16.  An integer k in [-16, 16] \\ {0} gives 5 x 32 = 160 (mu, sigma) pairs, fewer than the 513 consecutive rows that must
all differ (a 192- or 256-row tile, its other half, the same place of the next tile), so the third coprime factor goes into k itself:
k_m = s (a + j / 8), s a the 32 signed integers 1 .. 16 walked with stride 7, j = (3 m + 2) mod 7.  (e, s a, j) has period 5 x 32 x 7 = 1120 and
is one-to-one inside it: rows m != m' with |m - m'| < 1120 never share (mu, sigma); 1 <= |k| <= 16.75, so no row has |mu| < sigma R / 16.
const_rows(M) (three rows per case) are constant, sigma = 0 and |mu| = R x CONST_MU (values with a full mantissa, so that the fp32 sums
round): their variance is exactly 0, so the clamp of the single-pass variance and eps are all that stand between them and a NaN.  Weights: seeded normal K^-0.5, rounded; gamma and beta of norm_planted.affine
(multiples of 1 / 8); bias multiples of 1 / 8; the residual seeded normal, rounded.  With GEGLU the weight is made in the packed row order the
entry takes (16-row value | gate blocks: ff/nn.py pack_geglu) and the reference undoes it (unpack_geglu).

REFERENCE of tf_linear_ln_16: its contract is on the FOLDED operands it is given, so  y = rstd_m (x_m . w'_n - mean_m sum_k w'_nk) + bias'_n  in
float64, w' and bias' the 16-bit arrays of the fold (on the device: downloaded), mean and the biased variance in float64 from the rounded x,
rstd = (var + eps)^-1/2 with the fp32 eps passed; GEGLU a gelu_tanh(g) in float64; then the residual.
REFERENCE of tf_ln_fold_weights_16: w' == round16(w gamma) bit for bit (the product of two 16-bit values is exact in fp32: one rounding);
|colsum - sum_k w'| <= K_SUM 2^-24 sqrt(K) sum_k |w'|;  |bias' - (w . beta + bias)| <= half_ulp + K_SUM 2^-24 sqrt(K) (sum_k |w beta| + |bias|).

BUDGET per element:  tol = half_ulp(|y| + A) + A  [+ half_ulp(|y - r| + A) with a residual r: the short-K kernels round the accumulator to
16 bits before they add it, so every family is allowed two roundings],
    A = K_ACC 2^-24 sqrt(K) rstd_m (sum_k |x_mk w'_nk| + |mean_m| sum_k |w'_nk|)  +  K_STAT 2^-24 sqrt(K) (1 + mean_m^2 / var_m) |y - bias'_n|
(var_m + eps as the divisor in constant rows).  The second term is the single-pass variance E[x^2] - mean^2 from fp32 sums: it grows as R^2.
GEGLU: A_a and A_g go through y = a gelu(g) as  A = A_a |gelu(g)| + |a| (A_g |gelu'(g)| + K_ACT 2^-22 (1 + |gelu(g)|)), K_ACT of elementwise_planted.
The constants come from the EMULATION (emulate_fold), never from a device: fp32 lane sums by dot2 pairs over the K tiles and the kernels' xor
trees (8 lanes a row: the ring's loader waves, c4 / c8 with their partner half; 4 lanes: ping-pong, ar), fp32 accumulation per 16-deep k-step,
mean = s / K, rstd = rsqrt(max(q / K - mean^2, 0) + eps) moved +-1 fp32 step, the fold rstd (acc - mean colsum) + bias' fused and unfused (the
library is built with -ffp-contract=fast), GEGLU by elementwise_planted.emulate_act.  K_ACC is the smallest integer for which the emulation
GIVEN float64 statistics stays within A / 2 of its first term alone on every case, K_STAT then the smallest for which the whole emulation
stays within A / 2: the device gets twice the emulation's error and no more.  Measured, max |emulation - reference| / (A / 2 at K_* = 1) over
all cases, both lane forms and both storage types (the host test prints them per case):
    accumulation and fold on float64 statistics   0.25  (27600, 2432, 64) float16, residual   -> K_ACC = 1  (the smallest positive integer)
    with the fp32 single-pass statistics          0.30  (27600, 2432, 64) float16, residual   -> K_STAT = 1 (K_STAT = 0 fails: 1.55 there)
    k_ln_fold: colsum 0.015 (333, 520) float16, bias' 0.070 (6, 64) float16                  -> K_SUM = 1
The budget is a bound (sqrt(K) sum |terms|), so the integer floor leaves the emulation at a third of A / 2.  The emulation's largest absolute
error at R = 16 outside the constant rows is 1.3e-3 (a GEGLU output, (293, 96, 320) float16); in a constant row rstd = eps^-1/2 = 316 multiplies the
accumulation's error, which the first term of A carries through rstd_m.  Every mutant moves at least one element of every row tile it touches by
more than 8 tol (MUTANT_FACTOR).  A mutant that cannot show in a case is left out of that case and the host test's table says so: the stale
chunk without a forced tile, and the unclamped variance in bfloat16 (8-bit mantissas: the fp32 sums of squares are exact, never negative).

THE R LIMIT.  cancellation_limit(dtype) walks R = 16, 32, 64, ... at (64, 64, 320) with the R_MAIN constants until the emulation exceeds A / 2 or
the type can no longer hold the rows (spacing at R sigma above sigma / 4).  Measured: float16 meets A / 2 at every plantable R, the last being
R = 256 (0.29 of A / 2); bfloat16 at its plantable limit R = 32 (0.11 of A / 2).  The budget's R^2 term is a bound, not an estimate: the
emulation's error grows more slowly than it."""
import collections
import functools

import numpy as np

from norm_planted import MANTISSA, SENTINEL, _pair_tree, affine, fma, half_ulp, round16  # noqa: F401
from elementwise_planted import K_ACT, act64, emulate_act

F32, F64 = np.float32, np.float64
EPS = float(F32(1e-5))
U = 2.0 ** -24
R_MAIN = 16
K_ACC, K_STAT, K_SUM = 1, 1, 1
R_LIMIT = {"fp16": 256, "bf16": 32}        # cancellation_limit(): the last R the emulation meets (the host test asserts the table)
GUARD = 64
DTYPES = ("fp16", "bf16")
MUTANT_FACTOR = 8.0
UNSUPPORTED, E_ARG = 10002, 10001

# tf_gemm_debug bits and the `variant` column of tf_prof_dump / the tuning table
BIT_DEEP, BIT_WIDE, BIT_ALL8, BIT_PP, BIT_C4, BIT_C8, BIT_AR, BIT_PP3, BIT_PATCH = 8, 16, 256, 512, 1024, 16384, 32768, 2048, 128
BIT_M_FASTEST, BIT_PP_PHASES = 64, 8192
VARIANT_OF_BIT = {BIT_DEEP: 0, BIT_WIDE: 1, BIT_PATCH: 2, BIT_ALL8: 3, BIT_PP: 4, BIT_C4: 5, BIT_PP3: 6, BIT_C8: 7, BIT_AR: 8}
LANES_OF_VARIANT = {0: 8, 1: 8, 3: 8, 4: 4, 5: 8, 7: 8, 8: 4}

# family: the kernel's name in the tables; (M, N, K): N the OUTPUT width (GEGLU: the weight has 2 N packed rows); act 1 = GEGLU; res: a residual;
# (bm, bn, dbg): tf_gemm_force_config's tile and tf_gemm_debug's bits, bm = 0: unforced; R: |mu| / sigma of the planted rows
Case = collections.namedtuple("Case", "family M N K act res bm bn dbg R")


# ---- planted parameters -------------------------------------------------------------------------------------------------------------------------
def check_plantable(R, dtype):
    assert R >= 1 and R == 2 ** int(round(np.log2(R))), f"R = {R} is not a power of two"
    assert R * 2.0 ** -MANTISSA[dtype] <= 0.25, f"cannot plant R = {R} in {dtype}: the spacing at R sigma exceeds sigma / 4"


def max_plantable(dtype):
    return 2 ** (MANTISSA[dtype] - 2)


CONST_MU = (0.9713, 0.8371, 0.6127)         # |mu| / R of the constant rows: values with a full mantissa, so that the fp32 sums round


def const_rows(M):
    return sorted({3 % M, M // 2 + 1, M - 1})


def row_params(M, R):
    """(mu, sigma) of rows 0 .. M - 1 (float64); sigma = 0 in const_rows(M)."""
    m = np.arange(M, dtype=np.int64)
    sigma = np.exp2(((3 * m + 1) % 5 - 2).astype(F64))
    a = (7 * m + 3) % 32
    k = np.where(a >= 16, 1.0, -1.0) * (np.where(a >= 16, a - 15, 16 - a) + ((3 * m + 2) % 7) / 8.0)
    mu = sigma * R * k / 16.0
    c = const_rows(M)
    mu[c] = np.sign(k[c]) * R * np.asarray(CONST_MU[:len(c)])
    sigma[c] = 0.0
    return mu, sigma


def rows_distinct(mu, sigma, reach=512):
    """no two rows at most `reach` apart share (mu, sigma)."""
    pair = mu + 1j * sigma
    return all((pair[d:] != pair[:-d]).all() for d in range(1, min(reach, len(mu) - 1) + 1))


@functools.lru_cache(maxsize=4)
def x_input(M, K, dtype, R=R_MAIN):
    check_plantable(R, dtype)
    mu, sigma = row_params(M, R)
    z = np.random.default_rng([31, M, K]).standard_normal((M, K), dtype=F32).astype(F64)
    z -= z.mean(axis=1, keepdims=True)
    z /= np.sqrt((z * z).mean(axis=1, keepdims=True))
    x = round16(mu[:, None] + sigma[:, None] * z, dtype)
    for v in (x, mu, sigma):
        v.setflags(write=False)
    return x, mu, sigma


@functools.lru_cache(maxsize=8)
def weights(Np, K, dtype):
    """(w, bias) of Np (packed) rows: what the fold is given."""
    w = round16(np.random.default_rng([37, Np, K]).standard_normal((Np, K)) * K ** -0.5, dtype)
    bias = (((11 * np.arange(Np, dtype=np.int64) + 5) % 61 - 30) / 8.0).astype(F32)
    w.setflags(write=False)
    bias.setflags(write=False)
    return w, bias


@functools.lru_cache(maxsize=2)
def residual(M, N, dtype):
    r = round16(np.random.default_rng([41, M, N]).standard_normal((M, N), dtype=F32), dtype)
    r.setflags(write=False)
    return r


def packed_width(c):
    return 2 * c.N if c.act else c.N


def unpack_geglu(Np):
    """(value, gate) packed row indices of output columns 0 .. Np / 2 - 1: 16-row blocks v0 g0 v1 g1 ..."""
    n = np.arange(Np // 2)
    v = (n // 16) * 32 + n % 16
    return v, v + 16


def colsums_differ(cs):
    """column sums differ between neighbouring quads and between columns 16 and 64 apart (the lane maps of the epilogues)."""
    n = np.arange(len(cs))
    x16 = np.where((n ^ 16) < len(cs), n ^ 16, n - 16 if len(cs) > 16 else n)
    return all(len(cs) <= d or (cs[d:] != cs[:-d]).all() for d in (4, 16, 64)) and (len(cs) <= 16 or (cs != cs[x16]).all())


# ---- the weight fold ------------------------------------------------------------------------------------------------------------------------------
def fold64(w, bias, gamma, beta, dtype):
    """(w' exactly as the kernel must store it, float64 colsum of it, float64 bias' before the store, and the budgets of the two sums)."""
    wf = round16(w * gamma[None, :], dtype)                    # fp32 product of two 16-bit values: exact
    cs = wf.astype(F64).sum(axis=1)
    terms = w.astype(F64) * beta.astype(F64)[None, :]
    b0 = bias.astype(F64) if bias is not None else np.zeros(len(w))
    bf = terms.sum(axis=1) + b0
    rk = np.sqrt(w.shape[1])
    cs_tol = K_SUM * U * rk * np.abs(wf).astype(F64).sum(axis=1)
    a = K_SUM * U * rk * (np.abs(terms).sum(axis=1) + np.abs(b0))
    return wf, cs, bf, cs_tol, half_ulp(np.abs(bf) + a, dtype) + a, a


def fold_host(w, bias, gamma, beta, dtype):
    """what a correct fold hands to tf_linear_ln_16: (w', bias' rounded, colsum fp32) -- the host test's stand-in for the device's arrays."""
    wf, cs, bf, _, _, _ = fold64(w, bias, gamma, beta, dtype)
    return wf, round16(bf, dtype), cs.astype(F32)


def emulate_fold_weights(w, bias, gamma, beta, dtype):
    """k_ln_fold in fp32: lane l adds its vectors k = 8 l + 512 t element by element, then wave_sum's tree (halves first).  -> (colsum, bias' before the store)"""
    Np, K = w.shape
    T = -(-K // 512)
    wf = np.zeros((Np, T * 512), F32)
    wb = np.zeros((Np, T * 512), F32)
    wf[:, :K] = round16(w * gamma[None, :], dtype)
    wb[:, :K] = w
    bt = np.zeros(T * 512, F32)
    bt[:K] = beta
    cs, bs = np.zeros((Np, 64), F32), np.zeros((Np, 64), F32)
    for t in range(T):
        for j in range(8):
            col = t * 512 + np.arange(64) * 8 + j
            cs = cs + wf[:, col]
            bs = fma(bt[col][None, :], wb[:, col], bs)
    return _pair_tree(cs, ascending=False), (_pair_tree(bs, ascending=False) + (bias if bias is not None else F32(0))).astype(F32)


FOLD_CASES = [(1, 8), (6, 64), (70, 1280), (333, 520)]        # (N, K), each with and without a bias


# ---- float64 reference, budget, mutants -------------------------------------------------------------------------------------------------------------
def gelu_prime64(g):
    u = 2.0 * np.sqrt(2.0 / np.pi) * (g + 0.044715 * g ** 3)
    s = 1.0 / (1.0 + np.exp(-u))
    return s + g * s * (1.0 - s) * 2.0 * np.sqrt(2.0 / np.pi) * (1.0 + 3 * 0.044715 * g * g)


class Problem:
    """One launch's operands and everything the float64 answer needs that is cheap (per row / per column); the M x N work is done a block of rows
    at a time (blocks()) and never kept: block(sl) -> (y, tol, A), mutants(sl) -> name -> wrong y."""

    def __init__(self, case, dtype, wf=None, bf=None, eps=EPS):
        c = self.case = case
        self.dtype, self.eps = dtype, eps
        Np = self.Np = packed_width(c)
        self.x, self.mu, self.sigma = x_input(c.M, c.K, dtype, c.R)
        self.w, self.bias = weights(Np, c.K, dtype)
        self.gamma, self.beta = affine(c.K)
        self.res = residual(c.M, c.N, dtype) if c.res else None
        self.set_folded(*(fold_host(self.w, self.bias, self.gamma, self.beta, dtype)[:2] if wf is None else (wf, bf)))
        x64 = self.x.astype(F64)
        self.mean = x64.mean(axis=1)
        self.var = ((x64 - self.mean[:, None]) ** 2).mean(axis=1)
        self.vdiv = np.where(self.var > 0, self.var, self.var + eps)
        self.const = np.zeros(c.M, bool)
        self.const[const_rows(c.M)] = True
        self._alt = None

    def set_folded(self, wf, bf):
        self.wf, self.bf = np.ascontiguousarray(wf, F32).reshape(self.Np, self.case.K), np.ascontiguousarray(bf, F32).reshape(self.Np)
        self.wf64 = self.wf.astype(F64)
        self.S, self.absS = self.wf64.sum(axis=1), np.abs(self.wf64).sum(axis=1)

    def blocks(self, elems=1 << 22):
        step = max(64, elems // self.Np)
        return [slice(lo, min(self.case.M, lo + step)) for lo in range(0, self.case.M, step)]

    def finish(self, lin, sl):
        """packed float64 pre-activation (rows sl) -> the output: GEGLU, residual."""
        if self.case.act:
            v, g = unpack_geglu(self.Np)
            with np.errstate(all="ignore"):
                lin = lin[:, v] * act64("gelu", lin[:, g])
        return lin + self.res[sl] if self.res is not None else lin

    def gemm(self, sl):
        return self.x[sl].astype(F64) @ self.wf64.T

    def block(self, sl, G=None, k_acc=K_ACC, k_stat=K_STAT):
        c = self.case
        G = self.gemm(sl) if G is None else G
        absG = np.abs(self.x[sl]).astype(F64) @ np.abs(self.wf64).T
        mean, rstd = self.mean[sl, None], 1.0 / np.sqrt(self.var[sl, None] + self.eps)
        fold = rstd * (G - mean * self.S[None, :])
        lin = fold + self.bf[None, :]
        rk = np.sqrt(c.K)
        A = k_acc * U * rk * rstd * (absG + np.abs(mean) * self.absS[None, :]) + k_stat * U * rk * (1.0 + mean * mean / self.vdiv[sl, None]) * np.abs(fold)
        if c.act:
            v, g = unpack_geglu(self.Np)
            gg = act64("gelu", lin[:, g])
            A = A[:, v] * np.abs(gg) + np.abs(lin[:, v]) * (A[:, g] * np.abs(gelu_prime64(lin[:, g])) + K_ACT * 2.0 ** -22 * (1.0 + np.abs(gg)))
            y0 = lin[:, v] * gg
        else:
            y0 = lin
        tol = half_ulp(np.abs(y0) + A, self.dtype) + A
        if self.res is not None:
            y = y0 + self.res[sl]
            tol = half_ulp(np.abs(y) + A, self.dtype) + A + half_ulp(np.abs(y0) + A, self.dtype)
        else:
            y = y0
        return y, tol, A

    # -- mutants: one slip each, in float64.  alt(): per-row statistics and per-column vectors of every slip, made once
    def alt(self):
        if self._alt is not None:
            return self._alt
        c, M, K = self.case, self.case.M, self.case.K
        m = np.arange(M)
        x64 = self.x.astype(F64)
        every = np.ones(M, bool)
        out = {}

        def other_row(idx, name):
            ok = (idx >= 0) & (idx < M)
            j = np.where(ok, idx, m)
            out[name] = dict(mean=self.mean[j], var=self.var[j], rows=ok)
        other_row(m ^ 16, "statistics of row m ^ 16")
        other_row(m ^ 64, "statistics of row m ^ 64")
        if c.bm:
            other_row(m - c.bm, "statistics of row m - bm (the stale chunk)")

        def partial_sums(keep, name):
            xs = x64[:, keep]
            mean = xs.sum(axis=1) / K
            out[name] = dict(mean=mean, var=np.maximum((xs * xs).sum(axis=1) / K - mean * mean, 0.0), rows=every)
        k = np.arange(K)
        partial_sums(k % 64 < 32, "the partner K half not added")
        partial_sums(k < K - 64, "the last K tile missing from the sums")
        partial_sums(k >= 64, "the first K tile missing from the sums")
        n = np.arange(self.Np)
        out["colsum[n + 4]"] = dict(S=self.S[(n + 4) % self.Np], rows=every)
        out["colsum[n ^ 16]"] = dict(S=self.S[np.where((n ^ 16) < self.Np, n ^ 16, n)], rows=every)
        # the clamp: in float64 the single-pass variance of a constant row is 0 with or without it, and so is x . w' - mean colsum -- the slip shows
        # only where the fp32 sums leave the variance below -eps (a NaN).  The mutant takes the emulation's fp32 single-pass variance, unclamped, in
        # the constant rows where it is that low (float16 at K >= 128; bfloat16 squares have 16 bits: its fp32 sums are exact, and it never applies)
        rows = np.nonzero(self.const)[0]
        v32 = np.zeros(M)
        v32[rows] = np.minimum(emulate_stats(self.x[rows], 8)[2], emulate_stats(self.x[rows], 4)[2])      # (either lane form)
        neg = self.const & (v32 < -self.eps)
        if neg.any():
            out["the variance without the clamp"] = dict(var=np.where(neg, v32, self.var), rows=neg)
        out["eps left out"] = dict(eps=0.0, rows=self.const)
        out["mean but no rstd"] = dict(rstd=np.ones(M), rows=np.abs(1.0 / np.sqrt(self.var + self.eps) - 1.0) > 0.25)
        out["the unfolded bias in place of bias'"] = dict(bf=self.bias.astype(F64), rows=every)
        self._alt = out
        return out

    def not_applicable(self):
        return [nm for nm in MUTANTS if nm not in self.alt()]

    def mutants(self, sl, G=None):
        G = self.gemm(sl) if G is None else G
        res = {}
        for name, a in self.alt().items():
            mean = a.get("mean", self.mean)[sl, None]
            with np.errstate(all="ignore"):
                rstd = a["rstd"][sl, None] if "rstd" in a else 1.0 / np.sqrt(a.get("var", self.var)[sl, None] + a.get("eps", self.eps))
                lin = rstd * (G - mean * a.get("S", self.S)[None, :]) + a.get("bf", self.bf)[None, :]
                res[name] = self.finish(lin, sl)
        return res


MUTANTS = ["statistics of row m ^ 16", "statistics of row m ^ 64", "statistics of row m - bm (the stale chunk)", "the partner K half not added",
           "the last K tile missing from the sums", "the first K tile missing from the sums", "colsum[n + 4]", "colsum[n ^ 16]",
           "the variance without the clamp", "eps left out", "mean but no rstd", "the unfolded bias in place of bias'"]


def mutants(case, dtype, sl=None):
    """name -> the wrong (rows sl, N) answer of every slip that applies to the case (host folded operands)."""
    return Problem(case, dtype).mutants(slice(0, case.M) if sl is None else sl)


def beyond(got, want, tol):
    """|got - want| / tol with a non-finite value counting as infinitely far."""
    with np.errstate(all="ignore"):
        r = np.abs(got - want) / tol
    return np.where(np.isfinite(r), r, np.inf)


LARGEST = {"fp16": 65504.0, "bf16": float(np.finfo(np.float32).max)}


def matches(got, ym, tol, dtype):
    """does the output equal the mutant ym, element by element?  Within tol and the rounding of the mutant's own value; a non-finite output matches a
    mutant value that is non-finite or beyond the storage type."""
    with np.errstate(all="ignore"):
        out_of_type = ~np.isfinite(ym) | (np.abs(ym) >= LARGEST[dtype])
        near = np.abs(got - ym) <= tol + half_ulp(np.where(out_of_type, 0.0, ym), dtype)
    return np.where(np.isfinite(got), near & ~out_of_type, out_of_type)


def check_output(pb, got, k_acc=K_ACC, k_stat=K_STAT):
    """The GPU test's comparison (host code: the host test feeds it mutants as "device output").  got (M, N) float32.  -> (worst |err| / tol,
    the largest share of A an error uses beyond the store rounding tol - A, report): report is None where every element is within tol, else the text of the failure -- the first bad (row, column), the row's planted
    (mu, sigma), its tile, the mutants the output matches there and the mutants it matches everywhere."""
    c = pb.case
    worst, of_a, first, everywhere, there = 0.0, 0.0, None, None, []
    for sl in pb.blocks():
        G = pb.gemm(sl)
        y, tol, A = pb.block(sl, G, k_acc, k_stat)
        assert np.abs(y).max() < 1000, "a reference value comes near the sentinel"
        r = beyond(got[sl], y, tol)
        worst = max(worst, float(r.max()))
        with np.errstate(all="ignore"):
            of_a = max(of_a, float(np.nanmax((np.abs(got[sl] - y) - (tol - A)) / A)))
        if r.max() <= 1.0 and first is None:
            continue
        mut = pb.mutants(sl, G)
        match = {nm: matches(got[sl], ym, tol, pb.dtype) for nm, ym in mut.items()}
        if everywhere is None:
            everywhere = set(match)
        everywhere &= {nm for nm, ok in match.items() if ok.all()}
        if first is None:
            i, j = np.argwhere(r > 1.0)[0]
            first = (sl.start + int(i), int(j), float(got[sl][i, j]), float(y[i, j]), float(tol[i, j]))
            there = [nm for nm, ok in match.items() if ok[i, j]]
    if first is None:
        return worst, of_a, None
    m, n, g, y, t = first
    bm = c.bm or 1
    return worst, of_a, (f"{c} {pb.dtype}: y[{m}, {n}] = {g!r}, float64 {y!r}, tol {t:.3g} ({worst:.3g} x tol at worst); row planted (mu, sigma) = "
                   f"({pb.mu[m]!r}, {pb.sigma[m]!r}); row tile {m // bm} (row {m % bm} of it), column {n}; mutants matched there: {there or 'none'}; "
                   f"mutants matched everywhere: {sorted(everywhere) or 'none'}")


# ---- emulation of the kernels' fp32 arithmetic ---------------------------------------------------------------------------------------------------
def step32(v, n):
    return v if n == 0 else np.nextafter(v, F32(np.inf if n > 0 else -np.inf))


def emulate_stats(x, lanes, eps=EPS, fused=False, ulp=0):
    """(mean, rstd, unclamped variance) fp32 of rows x (rows, K) float32: `lanes` lanes share a row, each adds its 16-byte chunks (8 lanes: chunk c of
    every K tile; 4 lanes: chunks c and c + 4) two elements at a time (dot2_stats), then the xor tree; sk_mean_rstd's arithmetic."""
    rows, K = x.shape
    xt = x.reshape(rows, K // 64, 8, 4, 2).astype(F64)
    s, q = np.zeros((rows, lanes), F32), np.zeros((rows, lanes), F32)
    for t in range(K // 64):
        for h in range(8 // lanes):
            for e in range(4):
                p = xt[:, t, h * lanes:(h + 1) * lanes, e]
                s = (s + p[..., 0] + p[..., 1]).astype(F32)
                q = (q + p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]).astype(F32)
    s, q = _pair_tree(s), _pair_tree(q)
    invK = F32(1.0) / F32(K)
    mean = (s * invK).astype(F32)
    raw = fma(-mean, mean, (q * invK).astype(F32)) if fused else ((q * invK).astype(F32) - (mean * mean).astype(F32)).astype(F32)
    arg = (np.maximum(raw, F32(0)) + F32(eps)).astype(F32)
    rstd = step32((1.0 / np.sqrt(arg.astype(F64))).astype(F32), ulp)
    return mean, rstd, raw


ARITH = ((False, 0), (True, 0), (True, 1), (False, -1))      # (the two product-sums fused?, rsqrt / exp / rcp moved by that many fp32 steps)


def emulate_fold(pb, sl, lanes=8, fused=False, ulp=0, exact_stats=False, colsum=None):
    """The kernel's fp32 result in front of the store and the residual, rows sl: (rows, N) float32."""
    c = pb.case
    x = pb.x[sl]
    acc = np.zeros((x.shape[0], pb.Np), F32)
    for k0 in range(0, c.K, 16):                               # one MFMA k-step: 16 exact products added to the fp32 accumulator
        acc = (acc + x[:, k0:k0 + 16].astype(F64) @ pb.wf64[:, k0:k0 + 16].T).astype(F32)
    if exact_stats:
        mean, rstd = pb.mean[sl].astype(F32), (1.0 / np.sqrt(pb.var[sl] + pb.eps)).astype(F32)
    else:
        mean, rstd, _ = emulate_stats(x, lanes, pb.eps, fused, ulp)
    cs = (pb.S.astype(F32) if colsum is None else colsum)[None, :]
    inner = fma(-mean[:, None], cs, acc) if fused else (acc - (mean[:, None] * cs).astype(F32)).astype(F32)
    lin = ((rstd[:, None] * inner).astype(F32) + pb.bf[None, :]).astype(F32)
    if not c.act:
        return lin
    v, g = unpack_geglu(pb.Np)
    with np.errstate(all="ignore"):
        return (lin[:, v] * emulate_act("gelu", lin[:, g], ulp, ulp, fused)).astype(F32)


def emulation_ratios(pb, blocks=None, budgets=((1, 1), (K_ACC, K_STAT))):
    """(largest |emulation on float64 statistics - reference| / (A / 2 of the first term at K_ACC = 1), [largest |emulation - reference| / (A / 2)
    for every (k_acc, k_stat) of `budgets`], largest absolute error outside the constant rows) over both lane forms and ARITH; the colsum is the
    emulated fp32 one of k_ln_fold."""
    cs32 = emulate_fold_weights(pb.w, pb.bias, pb.gamma, pb.beta, pb.dtype)[0]
    ra, ab, rs = 0.0, 0.0, [0.0] * len(budgets)
    for sl in (pb.blocks(1 << 20) if blocks is None else blocks):
        G = pb.gemm(sl)
        r = pb.res[sl] if pb.res is not None else 0.0
        y = pb.block(sl, G)[0] - r
        A0 = pb.block(sl, G, 1, 0)[2]
        As = [pb.block(sl, G, ka, ks)[2] for ka, ks in budgets]
        for fused, ulp in ARITH:
            ra = max(ra, float((np.abs(emulate_fold(pb, sl, 8, fused, ulp, True) - y) / (A0 / 2)).max()))
            for lanes in (8, 4):
                e = np.abs(emulate_fold(pb, sl, lanes, fused, ulp, False, cs32) - y)
                rs = [max(v, float((e / (A / 2)).max())) for v, A in zip(rs, As)]
                ab = max(ab, float(e[~pb.const[sl]].max()))
    return ra, rs, ab


CANCELLATION_SHAPE = (64, 64, 320)


def cancellation_ratio(R, dtype):
    return emulation_ratios(Problem(Case("limit", *CANCELLATION_SHAPE, 0, False, 0, 0, 0, R), dtype))[1][1]


@functools.lru_cache(maxsize=None)
def cancellation_limit(dtype):
    """(the largest power-of-two R >= R_MAIN the emulation still meets A / 2 at, its ratio there, the ratio one step above or None where the type
    cannot hold the next R)."""
    R = R_MAIN
    ratio = cancellation_ratio(R, dtype)
    assert ratio <= 1.0
    while 2 * R <= max_plantable(dtype):
        nxt = cancellation_ratio(2 * R, dtype)
        if nxt > 1.0:
            return R, ratio, nxt
        R, ratio = 2 * R, nxt
    return R, ratio, None


# ---- the case tables ------------------------------------------------------------------------------------------------------------------------------
RING_TILES = [(64, 64), (128, 64), (64, 128), (128, 128), (256, 128), (64, 160), (128, 160)]
LONG_K_TILE = {BIT_DEEP: (256, 128), BIT_WIDE: (128, 128), BIT_ALL8: (128, 128)}      # K = 192 and 1280 (3 and 20 K tiles) on one tile per ring form
PP_TILES = [(256, 128), (256, 160), (256, 256), (192, 128), (192, 160)]


def ring_form(bm, bn, bit):
    """igemm_ring_form of gemm_common.h for channel counts on the 64 grid: the variant a tile runs when `bit` asks (the GPU test holds
    tf_gemm_ring_form against it)."""
    if bm == 256:
        return 0
    if bit == BIT_ALL8:
        return 3
    return 1 if bit == BIT_WIDE and not (bm == 128 and bn == 160) else 0


def _cases():
    out = []
    for bit in (BIT_DEEP, BIT_WIDE, BIT_ALL8):
        for bm, bn in RING_TILES:
            if ring_form(bm, bn, bit) != VARIANT_OF_BIT[bit]:
                continue                                       # the tile has no such ring
            ks = (64, 320) + ((192, 1280) if LONG_K_TILE[bit] == (bm, bn) else ())
            for K in ks:                                       # K = 64: m-fastest tile order, no residual; the others n-fastest with a residual
                out.append(Case("ring", 2 * bm + 37, bn + 36, K, 0, K != 64, bm, bn, bit | (BIT_M_FASTEST if K == 64 else 0), R_MAIN))
    out.append(Case("ring", 2 * 64 + 37, (128 + 32) // 2, 320, 1, False, 64, 128, BIT_ALL8, R_MAIN))      # GEGLU on the all-8 ring (a row of the tuning table)
    for bm, bn in PP_TILES:
        for K in (64, 320, 1280):
            out.append(Case("pp", 2 * bm + 37, bn + 36, K, 0, K == 320, bm, bn, BIT_PP, R_MAIN))
        if bn % 64 == 0:
            out.append(Case("pp", 2 * bm + 37, (bn + 32) // 2, 320, 1, False, bm, bn, BIT_PP, R_MAIN))
    out.append(Case("pp", 2 * 256 + 37, 128 + 36, 320, 0, True, 256, 128, BIT_PP | BIT_PP_PHASES, R_MAIN))
    for fam, bm, bit in (("c4", 128, BIT_C4), ("c8", 256, BIT_C8)):
        for order in (0, BIT_M_FASTEST):
            for K in (64, 128, 320, 1280):
                for res in (False, True):
                    out.append(Case(fam, 2 * bm + 37, 168, K, 0, res, bm, 128, bit | order, R_MAIN))
            out.append(Case(fam, 2 * bm + 37, 96, 320, 1, False, bm, 128, bit | order, R_MAIN))
    for K in (256, 320):
        out.append(Case("ar", 293, 168, K, 0, False, 128, 128, BIT_AR, R_MAIN))
        out.append(Case("ar", 293, 96, K, 1, False, 128, 128, BIT_AR, R_MAIN))
    out.append(Case("unforced", 300, 128, 64, 0, True, 0, 0, 0, R_MAIN))
    out.append(Case("unforced", 154, 64, 128, 1, False, 0, 0, 0, R_MAIN))
    return out


CASES = _cases()
# the chunked tile walk of k_gemm_c4 / k_gemm_c8 (n-fastest order): the smallest M for which shortk_chunk gives chunks of 2 and 4 on 256 CUs, packed
# N = 2432 = 19 column tiles (chunks straddle row blocks).  Every row block has statistics of its own here.
CHUNK_CASES = [Case(fam, M, 1216 if act else 2432, 64, act, not act, bm, 128, bit, R_MAIN)
               for M, act in ((27600, 0), (55200, 1)) for fam, bm, bit in (("c4", 128, BIT_C4), ("c8", 256, BIT_C8))]


def shortk_chunk(c, cus=256):
    """shortk_chunk of gemm_shortk.h: consecutive tiles a block of k_gemm_c4 / k_gemm_c8 walks with the fold (n-fastest order) on `cus` CUs."""
    if c.dbg & BIT_M_FASTEST:
        return 1
    tiles = -(-c.M // c.bm) * -(-packed_width(c) // c.bn)
    floor_ = (8 if c.family == "c4" else 4) * cus
    return 4 if tiles // 4 >= floor_ else 2 if tiles // 2 >= floor_ else 1


R_LIMIT_CASES = [Case("ring", 165, 100, 320, 0, False, 64, 64, BIT_DEEP, 0), Case("pp", 421, 164, 320, 0, False, 192, 128, BIT_PP, 0),
                 Case("c4", 293, 168, 320, 0, False, 128, 128, BIT_C4, 0), Case("c8", 549, 168, 320, 0, False, 256, 128, BIT_C8, 0),
                 Case("ar", 293, 168, 320, 0, False, 128, 128, BIT_AR, 0)]      # R = 0: the GPU test puts R_LIMIT[dtype] in


def family_bit(c):
    bits = [b for b in VARIANT_OF_BIT if c.dbg & b]
    return max(bits) if bits else 0


def predict_form(c):
    """the (bm, bn, splitk, variant) tf_prof_dump must show: the tile and family asked for, never split (None: the dispatcher's choice)."""
    return (c.bm, c.bn, 1, VARIANT_OF_BIT[family_bit(c)]) if c.bm else None


def tune_form(c):
    """(variant, bm, bn, act, order) as a row of the tuning table states it."""
    return (VARIANT_OF_BIT[family_bit(c)], c.bm, c.bn, c.act, 1 if c.dbg & BIT_M_FASTEST else 0)


def data_key(c):
    return (c.M, c.N, c.K, c.act, c.res, c.R)


def case_id(c):
    return f"{c.family}-{c.M}x{c.N}x{c.K}-a{c.act}r{int(c.res)}-{c.bm}x{c.bn}-d{c.dbg}"


# (what, M, N, K, act, bm, bn, dbg, colsum given, status, a word of the error text)
REFUSALS = [
    ("K off the 64 grid", 77, 64, 96, 0, 0, 0, 0, True, E_ARG, b"multiple of 64"),
    ("K below 64", 77, 64, 32, 0, 0, 0, 0, True, E_ARG, b"multiple of 64"),
    ("N off the 4 grid", 77, 6, 64, 0, 0, 0, 0, True, E_ARG, b"multiple of 4"),
    ("GEGLU with N off the 16 grid", 77, 24, 64, 1, 0, 0, 0, True, E_ARG, b"16 for GEGLU"),
    ("null colsum", 77, 64, 64, 0, 0, 0, 0, False, E_ARG, b"null tensor"),
    ("the ping-pong patch kernel cannot take the fold", 77, 64, 64, 0, 192, 128, BIT_PP3, True, UNSUPPORTED, b"ping-pong patch kernel"),
    ("the patch kernel cannot take the fold", 77, 64, 64, 0, 64, 128, BIT_PATCH, True, UNSUPPORTED, b"the patch kernel"),
]
