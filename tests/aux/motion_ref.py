"""AnimateDiff motion modules on the host -- TEST INFRASTRUCTURE for vision/motion.py, UNetModel.__call__(motion=) and
StableDiffusion.compile(..., motion=True).  torch on the CPU only; written from the formulas of the published architecture, not from the library.

(a) motion_module_forward(x, W, F): one module in float64.  x (G F, C, h, w), the frames of a video adjacent; W: the module's tensors by their
    names below ``temporal_transformer.``:
        t   = proj_in(GroupNorm32(x, eps 1e-6))           statistics per image of the (G F) batch; tokens (G F, P, C), P = h w
        t   = t + to_out_i(Attn_i(LayerNorm_i(t) + pe_i[:F]))      i = 0, 1
        t   = t + ff.net.2(GEGLU(ff_norm(t)))
        out = x + scale proj_out(t)
    Attn = softmax_f'(q k^T / sqrt(C / heads)) v over the F frames of the same video and pixel, ``heads`` = 8.  GEGLU is a gelu(gate) with the
    project's GELU (oracle.ops.gelu: the tanh form every GEGLU of the library computes; it is within 5e-4 |a| of the erf form).
    The keyword arguments are the knobs of the sensitivity checks: ``heads`` and ``gn_eps`` state what a wrong device path would compute.
(b) unet_forward_motion: oracle.unet_forward's walk (fp32, the oracle's own pieces, as tests/aux/freeu_ref.py composes them) with the modules at
    their slots: behind everything else of input_blocks[1 + i (n + 1) + j], between the middle block's transformer and its second ResBlock,
    in output_blocks[i (n + 1) + j] in front of an Upsample.  ``motion`` = ({file prefix: {name: array}}, F, scale); None: oracle.unet_forward.
(c) module_inputs / eps_case: the inputs the GPU tests and the host sensitivity checks share.
"""
import math

import numpy as np
import torch

from oracle import ops
from oracle.unet import SD15, _graph

F64 = torch.float64
T = "transformer_blocks.0."


def t64(x):
    return x.to(F64) if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64)))


def _layer_norm(x, g, b, eps=1e-5):
    mu = x.mean(dim=-1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def _group_norm(x, groups, g, b, eps):
    n, c, h, w = x.shape
    xg = x.reshape(n, groups, -1)
    mu = xg.mean(dim=-1, keepdim=True)
    var = ((xg - mu) ** 2).mean(dim=-1, keepdim=True)
    return ((xg - mu) / torch.sqrt(var + eps)).reshape(n, c, h, w) * g.reshape(1, c, 1, 1) + b.reshape(1, c, 1, 1)


def temporal_attention(t, W, p, G, F, heads):
    """t (G F, P, C) -> softmax over the frames of one (video, pixel, head): (G F, P, C), heads merged the LDM way."""
    n, P, C = t.shape
    d = C // heads
    pe = t64(W[p + "pos_encoder.pe"])[0, :F]                                     # (F, C)
    y = (t.reshape(G, F, P, C) + pe[None, :, None, :])
    q, k, v = (y @ t64(W[p + f"to_{m}.weight"]).t() for m in "qkv")              # (G, F, P, C)
    q, k, v = (z.reshape(G, F, P, heads, d).permute(0, 2, 3, 1, 4) for z in (q, k, v))       # (G, P, heads, F, d)
    a = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d), dim=-1) @ v        # (G, P, heads, F, d)
    return a.permute(0, 3, 1, 2, 4).reshape(n, P, C)


def motion_module_forward(x, W, F, heads=8, gn_eps=1e-6, scale=1.0):
    x = t64(x)
    n, C, h, w = x.shape
    assert n % F == 0 and C % heads == 0, (x.shape, F, heads)
    G = n // F
    W = {k: t64(v) for k, v in W.items()}
    t = _group_norm(x, 32, W["norm.weight"], W["norm.bias"], gn_eps)
    t = t.reshape(n, C, h * w).permute(0, 2, 1)
    t = t @ W["proj_in.weight"].reshape(C, C).t() + W["proj_in.bias"]
    for i in (0, 1):
        p = f"{T}attention_blocks.{i}."
        y = _layer_norm(t, W[f"{T}norms.{i}.weight"], W[f"{T}norms.{i}.bias"])
        a = temporal_attention(y, W, p, G, F, heads)
        t = t + a @ W[p + "to_out.0.weight"].t() + W[p + "to_out.0.bias"]
    y = _layer_norm(t, W[T + "ff_norm.weight"], W[T + "ff_norm.bias"])
    y = y @ W[T + "ff.net.0.proj.weight"].t() + W[T + "ff.net.0.proj.bias"]
    a, gate = torch.chunk(y, 2, dim=-1)
    y = a * (0.5 * gate * (1.0 + torch.tanh(gate * 0.7978845608 * (1.0 + 0.044715 * gate * gate))))
    t = t + y @ W[T + "ff.net.2.weight"].t() + W[T + "ff.net.2.bias"]
    o = t @ W["proj_out.weight"].reshape(C, C).t() + W["proj_out.bias"]
    return x + scale * o.permute(0, 2, 1).reshape(n, C, h, w)


# ---- the file's names ----------------------------------------------------------------------------------------------------------------------------
def slot_names(cfg, mid=False):
    """[(file prefix, LDM slot)] in execution order, from the oracle's graph: down_blocks.i.motion_modules.j <-> input_blocks[1 + i (n + 1) + j],
    up_blocks.i.motion_modules.j <-> output_blocks[i (n + 1) + j]."""
    n, nlev = cfg.num_res_blocks, len(cfg.channel_mult)
    rows = [(f"down_blocks.{i}.motion_modules.{j}", f"input_blocks.{1 + i * (n + 1) + j}") for i in range(nlev) for j in range(n)]
    if mid:
        rows.append(("mid_block.motion_modules.0", "middle_block"))
    return rows + [(f"up_blocks.{i}.motion_modules.{j}", f"output_blocks.{i * (n + 1) + j}") for i in range(nlev) for j in range(n + 1)]


def split_modules(state):
    """A file's dict in the AnimateDiff spelling -> {file prefix: {name below temporal_transformer.: array}}."""
    out = {}
    for k, v in state.items():
        prefix, rel = k.split(".temporal_transformer.")
        out.setdefault(prefix, {})[rel] = v
    return out


def to_diffusers(state):
    """The same tensors under diffusers' MotionAdapter names."""
    out = {}
    for k, v in state.items():
        k = k.replace(".temporal_transformer.", ".")
        for a, b in ((".attention_blocks.0.", ".attn1."), (".attention_blocks.1.", ".attn2."), (".norms.0.", ".norm1."), (".norms.1.", ".norm2."),
                     (".ff_norm.", ".norm3."), (".pos_encoder.", ".pos_embed.")):
            k = k.replace(a, b)
        out[k] = v
    return out


# ---- (b) the UNet ------------------------------------------------------------------------------------------------------------------------------------
def unet_forward_motion(x, timesteps, context, W, cfg=SD15, head_merge="reference_exact", motion=None):
    from controlnet_oracle import _embed_time, _run
    W = {k: ops.as_t(v) for k, v in W.items()}
    x, context = ops.as_t(x), ops.as_t(context)
    emb = _embed_time(timesteps, W, cfg)
    inp, mid, out = _graph(cfg)
    mods, frames, scale = motion if motion is not None else ({}, 1, 1.0)
    at = {slot: mods[prefix] for prefix, slot in slot_names(cfg, "mid_block.motion_modules.0" in mods)} if mods else {}

    def mm(x, slot):
        return motion_module_forward(x, at[slot], frames, scale=scale).to(torch.float32) if slot in at else x

    saved = []
    for i, b in enumerate(inp):
        for j, l in enumerate(b):
            x = _run(x, l, f"input_blocks.{i}.{j}", emb, context, W, cfg, head_merge)
        x = mm(x, f"input_blocks.{i}")
        saved.append(x)                                              # (the module's output is what the skip concat reads)
    for j, l in enumerate(mid):
        if j == len(mid) - 1:
            x = mm(x, "middle_block")
        x = _run(x, l, f"middle_block.{j}", emb, context, W, cfg, head_merge)
    for i, b in enumerate(out):
        x = torch.cat((x, saved.pop()), dim=1)
        done = False
        for j, l in enumerate(b):
            if l[0] == "up":
                x, done = mm(x, f"output_blocks.{i}"), True
            x = _run(x, l, f"output_blocks.{i}.{j}", emb, context, W, cfg, head_merge)
        if not done:
            x = mm(x, f"output_blocks.{i}")
    x = ops.silu(ops.group_norm_affine(x, cfg.num_groups, W["out.0.weight"], W["out.0.bias"]))
    return ops.conv2d_bias(x, W["out.2.weight"], W["out.2.bias"], (1, 1))


# ---- (c) shared inputs ---------------------------------------------------------------------------------------------------------------------------------
MODULE_CASES = ((64, 3, 2, 3, 2, 32), (128, 16, 1, 2, 2, 32), (320, 16, 2, 2, 2, 32), (64, 24, 1, 1, 1, 32), (64, 32, 1, 1, 1, 32))   # (C, F, V, h, w, max_len)
RTOL, ATOL = 1e-2, 1.5e-2          # tests/test_gpu_model.py's bound on SpatialTransformer; bf16: x 8


def round16(x, dtype):
    """float array -> the float32 values the storage type holds (round to nearest even)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dtype == "bf16":
        u = x.view(np.uint32)
        bits = ((u + (((u >> 16) & 1) + np.uint32(0x7FFF))) >> 16).astype(np.uint32) << 16
        return bits.view(np.float32)
    return x.astype(np.float16).astype(np.float32)


def module_weights(C, max_len, seed=7):
    """One module's tensors (names below temporal_transformer.), fp16 values as float32, proj_out not zero."""
    from tinyfusers_amd.storage.synth import synth_motion_state_dict
    from tinyfusers_amd.vision.unet import UNetConfig
    cfg = UNetConfig(model_channels=C, channel_mult=(1,), num_res_blocks=1, attention_levels=(), n_heads=8, context_dim=64)
    mods = split_modules(synth_motion_state_dict(cfg, seed, max_len))
    return {k: v.astype(np.float32) for k, v in mods["down_blocks.0.motion_modules.0"].items()}


def module_input(C, F, V, h, w, seed=11):
    from tinyfusers_amd.storage.synth import synth_normal
    return synth_normal(seed, f"motion.x.{C}.{F}.{V}.{h}.{w}", (V * F, C, h, w)).astype(np.float16).astype(np.float32)


EPS_CASE = (64, 4, 1, 4, 4, 32)    # (C, F, V, h, w, max_len) of the GroupNorm eps case


def eps_case_input():
    """The eps case: per-group variance near 1e-5 (std 3.2e-3 around per-channel offsets of the same size), so that eps 1e-5 against 1e-6 changes
    the normalised values by tens of percent: 1 / sqrt(1e-5 + 1e-5) against 1 / sqrt(1e-5 + 1e-6)."""
    from tinyfusers_amd.storage.synth import synth_normal
    C, F, V, h, w, _ = EPS_CASE
    x = synth_normal(13, "motion.eps.x", (V * F, C, h, w)) * np.float32(3.2e-3)
    return x.astype(np.float16).astype(np.float32)
