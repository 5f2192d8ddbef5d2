"""The expected value of a LoRA merge, in numpy float64, and the synthetic adapters of tests/test_lora_host.py and tests/test_gpu_lora.py.

    W' = W.reshape(N, Kd) + sum_i s_i up_i @ down_i

evaluated in float64 on the values the device holds (16-bit values widened exactly), with conv tensors flattened in the KRSC order the device
stores (storage/tensor.py: logical (K, C, R, S), stored (K, R, S, C)).  TEST INFRASTRUCTURE: nothing in the product imports this."""
import numpy as np


def stored(w):
    """Logical weight -> the (N, Kd) row matrix the device stores: a Linear's (out, in) as it is, a conv's (K, C, R, S) as (K, R S C)."""
    w = np.asarray(w)
    if w.ndim == 4:
        w = w.transpose(0, 2, 3, 1)
    return np.ascontiguousarray(w).reshape(w.shape[0], -1)


def logical(m, shape):
    """The inverse of ``stored`` for a weight of logical ``shape``."""
    if len(shape) == 4:
        k, c, r, s = shape
        return np.ascontiguousarray(np.asarray(m).reshape(k, r, s, c).transpose(0, 3, 1, 2))
    return np.asarray(m).reshape(shape)


def to16(x, dtype):
    """float array -> the float64 values of its rounding to fp16 / bf16 (round to nearest even)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dtype == "bf16":
        u = x.view(np.uint32)
        r = ((u + (((u >> 16) & 1) + np.uint32(0x7FFF))) >> 16).astype(np.uint32) << 16
        return r.view(np.float32).astype(np.float64)
    return x.astype(np.float16).astype(np.float64)


def merge_ref(w, adapters):
    """w: logical weight; adapters: [(s_i, up_i (N, r[, 1, 1]), down_i (r, in...))] logical arrays -> (W' (N, Kd) float64, S (N, Kd) float64), S =
    |base| + sum_i |s_i| sum_j |up| |down|: the magnitude the fp32 chain's rounding errors scale with."""
    ref = stored(w).astype(np.float64)
    mag = np.abs(ref)
    for s, up, down in adapters:
        u = np.asarray(up, np.float64).reshape(up.shape[0], -1)
        d = stored(down).astype(np.float64)
        ref = ref + np.float64(s) * (u @ d)
        mag = mag + abs(np.float64(s)) * (np.abs(u) @ np.abs(d))
    return ref, mag


def merge_bound(ref, mag, ranks, dtype):
    """|got - ref| <= rel |ref| + n 2^-24 S + 2^-24: rel = one unit in the last place of the 16-bit type (2^-10 fp16, 2^-7 bf16; covers the double
    rounding fp32 -> 16 bit), n = sum Rp_i + 2 adapters + 1 the length of the fp32 chain (Rp_i: the rank padded to 32), 2^-24 for results in
    fp16's subnormal range."""
    rel = 2.0 ** -7 if dtype == "bf16" else 2.0 ** -10
    n = sum((r + 31) // 32 * 32 for r in ranks) + 2 * len(ranks) + 1
    return rel * np.abs(ref) + n * 2.0 ** -24 * mag + 2.0 ** -24


def scale(weight, alpha, rank):
    """s_i as set_adapters computes it: float64, rounded to fp32 once."""
    return np.float32(np.float64(weight) * np.float64(alpha) / np.float64(rank))


def make_adapter(weights, rank, seed, frac=0.05, dtype=np.float16, exact=True):
    """A kohya-format adapter over ``weights`` ({kohya module name: logical base weight}): up (N, r[, 1, 1]) and down (r, in...) ~ N(0, 1) in fp16,
    alpha (fp32) per module such that ||(alpha / r) up down||_F = frac ||W||_F.  exact=False: ||up down||_F by its expectation sqrt(N Kd r)
    instead of the float64 product (the SD-1.5 shapes, where the size only has to be about right)."""
    rng = np.random.default_rng(seed)
    out = {}
    for name in sorted(weights):
        w = np.asarray(weights[name], np.float32)
        n = w.shape[0]
        up = rng.standard_normal((n, rank)).astype(np.float16)
        down = rng.standard_normal((rank,) + tuple(w.shape[1:])).astype(np.float16)
        norm = np.linalg.norm(up.astype(np.float32) @ stored(down).astype(np.float32)) if exact else np.sqrt(float(w.size) * rank)
        alpha = np.float32(rank * frac * np.linalg.norm(w) / norm)
        out[name + ".lora_up.weight"] = (up.reshape(n, rank, 1, 1) if w.ndim == 4 else up).astype(dtype)
        out[name + ".lora_down.weight"] = down.astype(dtype)
        out[name + ".alpha"] = np.asarray(alpha, np.float32)
    return out


def merged_state(state, paths, adapters, dtype="fp16"):
    """state: {LDM name: array}; paths: {kohya module name: LDM module path (``<path>.weight`` is a key of state)}; adapters: [(weight, kohya-format
    dict)] -> a copy of ``state`` (float32) in which every touched weight is the float64 merge of the 16-bit values, rounded to the 16-bit type:
    what an oracle is fed to restate a model with the adapters merged in."""
    out = {k: np.asarray(v, np.float32) for k, v in state.items()}
    touched = sorted({k.split(".")[0] for _, a in adapters for k in a})
    for mod in touched:
        key = paths[mod] + ".weight"
        w = to16(state[key], dtype)
        entries = []
        for weight, a in adapters:
            if mod + ".lora_up.weight" in a and weight != 0:
                up, down = to16(a[mod + ".lora_up.weight"], dtype), to16(a[mod + ".lora_down.weight"], dtype)
                entries.append((scale(weight, float(a[mod + ".alpha"]), down.shape[0]), up, down))
        if entries:
            ref, _ = merge_ref(w, entries)
            out[key] = logical(to16(ref, dtype), w.shape).astype(np.float32)
    return out
