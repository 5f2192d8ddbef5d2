"""CPU restatement (fp32, torch-CPU) of a ControlNet and of the UNet forward that takes its residuals -- TEST INFRASTRUCTURE, composed from
oracle.unet (_graph, resblock, spatial_transformer) and oracle.ops the way oracle.unet_forward is.

The published ControlNet for SD-1.x (Zhang et al. 2023, cldm.py of the public repository): a copy of the UNet's time_embed, input_blocks and
middle_block reading conv_in(x) + hint_stem(hint); a 1x1 "zero" convolution on every input block's output and on the middle block's; the
controlled UNet computes mid += r[-1] and cat(x, saved.pop() + r.pop()).  Weights: a flat dict keyed by the LDM names relative to the model root."""
from typing import Dict

import torch

from oracle import ops
from oracle.unet import SD15, UNetConfig, _graph, resblock, spatial_transformer, unet_param_shapes

# (cin, cout, stride) of the hint stem's 3x3 convolutions, indices 0, 2, ..., 14 of input_hint_block (SiLU at the odd ones); None: the hint's
# channels / the model's width
HINT_PLAN = ((None, 16, 1), (16, 16, 1), (16, 32, 2), (32, 32, 1), (32, 96, 2), (96, 96, 1), (96, 256, 2), (256, None, 1))


def controlnet_param_shapes(cfg: UNetConfig = SD15, hint_channels=3) -> Dict[str, tuple]:
    """Every weight / bias leaf of the ControlNet with its shape, in the checkpoint's names (without the ``control_model.`` prefix)."""
    inp, _, _ = _graph(cfg)
    P = {k: v for k, v in unet_param_shapes(cfg).items() if k.startswith(("time_embed.", "input_blocks.", "middle_block."))}
    P["input_blocks.0.0.weight"] = (cfg.model_channels, 4, 3, 3)               # the latent alone, whatever the UNet's in_channels
    for i, (ci, co, _) in enumerate(HINT_PLAN):
        ci, co = ci or hint_channels, co or cfg.model_channels
        P[f"input_hint_block.{2 * i}.weight"] = (co, ci, 3, 3)
        P[f"input_hint_block.{2 * i}.bias"] = (co,)
    chans = [b[-1][2] if b[-1][0] in ("conv", "res") else b[-1][1] for b in inp]       # what each input block puts out
    for i, c in enumerate(chans):
        P[f"zero_convs.{i}.0.weight"] = (c, c, 1, 1)
        P[f"zero_convs.{i}.0.bias"] = (c,)
    P["middle_block_out.0.weight"] = (chans[-1], chans[-1], 1, 1)
    P["middle_block_out.0.bias"] = (chans[-1],)
    return P


def hint_embedding(hint, W):
    """input_hint_block: conv, SiLU, conv, ..., conv (no SiLU behind the last).  hint (b, 3, 8h, 8w) in [0, 1] -> (b, model_channels, h, w)."""
    x = ops.as_t(hint)
    for i, (_, _, st) in enumerate(HINT_PLAN):
        x = ops.conv2d_bias(x, W[f"input_hint_block.{2 * i}.weight"], W[f"input_hint_block.{2 * i}.bias"], (1, 1), (st, st))
        if i != len(HINT_PLAN) - 1:
            x = ops.silu(x)
    return x


def _embed_time(timesteps, W, cfg):
    t_emb = ops.timestep_embedding(timesteps, cfg.model_channels)
    emb = ops.linear(t_emb, W["time_embed.0.weight"], W["time_embed.0.bias"])
    return ops.linear(ops.silu(emb), W["time_embed.2.weight"], W["time_embed.2.bias"])


def _run(x, l, p, emb, context, W, cfg, head_merge):
    if l[0] == "conv": return ops.conv2d_bias(x, W[p + ".weight"], W[p + ".bias"], (1, 1))
    if l[0] == "res": return resblock(x, emb, W, p, cfg)
    if l[0] == "st": return spatial_transformer(x, context, W, p, cfg.n_heads, cfg, head_merge)
    if l[0] == "down": return ops.conv2d_bias(x, W[p + ".op.weight"], W[p + ".op.bias"], (1, 1), (2, 2))
    if l[0] == "up": return ops.conv2d_bias(ops.upsample_nearest2x(x), W[p + ".conv.weight"], W[p + ".conv.bias"], (1, 1))
    raise ValueError(l)


def controlnet_forward(x, hint, timesteps, context, W, cfg=SD15, head_merge="reference_exact", hint_emb=None):
    """The len(input_blocks) + 1 residuals: zero_convs[i](input block i's output), then middle_block_out(the middle block's output).
    h = conv_in(x) + hint_stem(hint); a single hint is broadcast over the batch of x."""
    W = {k: ops.as_t(v) for k, v in W.items()}
    x, context = ops.as_t(x), ops.as_t(context)
    emb = _embed_time(timesteps, W, cfg)
    guided = hint_embedding(hint, W) if hint_emb is None else ops.as_t(hint_emb)
    inp, mid, _ = _graph(cfg)
    outs = []
    for i, b in enumerate(inp):
        for j, l in enumerate(b):
            x = _run(x, l, f"input_blocks.{i}.{j}", emb, context, W, cfg, head_merge)
        if i == 0:
            x = x + guided
        outs.append(ops.conv2d_bias(x, W[f"zero_convs.{i}.0.weight"], W[f"zero_convs.{i}.0.bias"]))
    for j, l in enumerate(mid):
        x = _run(x, l, f"middle_block.{j}", emb, context, W, cfg, head_merge)
    outs.append(ops.conv2d_bias(x, W["middle_block_out.0.weight"], W["middle_block_out.0.bias"]))
    return outs


def unet_forward(x, timesteps, context, W, cfg=SD15, head_merge="reference_exact", control=None):
    """oracle.unet_forward with the residuals of a ControlNet: mid += r[-1], cat(x, saved.pop() + r.pop()).  control: the list
    controlnet_forward returns (already scaled), or None."""
    W = {k: ops.as_t(v) for k, v in W.items()}
    x, context = ops.as_t(x), ops.as_t(context)
    emb = _embed_time(timesteps, W, cfg)
    inp, mid, out = _graph(cfg)
    r = [ops.as_t(v) for v in control] if control is not None else None
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
        x = torch.cat((x, saved.pop() + r.pop() if r is not None else saved.pop()), dim=1)
        for j, l in enumerate(b):
            x = _run(x, l, f"output_blocks.{i}.{j}", emb, context, W, cfg, head_merge)
    x = ops.silu(ops.group_norm_affine(x, cfg.num_groups, W["out.0.weight"], W["out.0.bias"]))
    return ops.conv2d_bias(x, W["out.2.weight"], W["out.2.bias"], (1, 1))
