"""CPU restatement (fp32, torch-CPU) of perturbed-attention guidance -- TEST INFRASTRUCTURE, composed from oracle.unet's own pieces (_graph,
resblock, cross_attention, feed_forward) and oracle.ops the way tests/aux/ip_adapter_ref.py composes its forward.

Published form (Ahn et al. 2024; diffusers' PAGIdentitySelfAttnProcessor): the perturbed branch runs the UNet on the conditional inputs, and in the
self-attention (attn1) of the selected SpatialTransformers the softmax is replaced by the identity, attn1(x) = to_out(to_v(x)); cross-attention,
the FeedForward and every other layer are untouched.  The combine: e = e_u + g (e_c - e_u) + s_t (e_c - e_p) with classifier-free guidance,
e = e_c + s_t (e_c - e_p) without, s_t = max(0, s - a (1000 - t))."""
import numpy as np
import torch

from oracle import ops
from oracle.unet import SD15, UNetConfig, _graph, cross_attention, feed_forward, resblock

SD15_LAYERS = ["input_blocks.1", "input_blocks.2", "input_blocks.4", "input_blocks.5", "input_blocks.7", "input_blocks.8", "middle_block",
               "output_blocks.3", "output_blocks.4", "output_blocks.5", "output_blocks.6", "output_blocks.7", "output_blocks.8", "output_blocks.9",
               "output_blocks.10", "output_blocks.11"]


def layers(cfg: UNetConfig = SD15):
    """The blocks that hold a SpatialTransformer, in execution order (input blocks, middle block, output blocks), from the oracle's block lists."""
    inp, mid, out = _graph(cfg)
    found = [f"input_blocks.{i}" for i, b in enumerate(inp) if any(l[0] == "st" for l in b)]
    found += ["middle_block"] if any(l[0] == "st" for l in mid) else []
    return found + [f"output_blocks.{i}" for i, b in enumerate(out) if any(l[0] == "st" for l in b)]


def identity_self_attention(x, W, p, n_heads, head_merge="reference_exact"):
    """oracle.unet.cross_attention's self-attention with the identity in place of softmax(q k^T): o = v per (batch, head), merged as it merges."""
    v = ops.linear(x, W[p + ".to_v.weight"])
    b, d = x.shape[0], v.shape[-1] // n_heads
    o = v.reshape(b, -1, n_heads, d).permute(0, 2, 1, 3)
    o = o.reshape(b, -1, n_heads * d) if head_merge == "reference_exact" else o.permute(0, 2, 1, 3).reshape(b, -1, n_heads * d)
    return ops.linear(o, W[p + ".to_out.0.weight"], W[p + ".to_out.0.bias"])


def _spatial_transformer(x, context, W, p, n_heads, cfg, head_merge, perturbed):
    b, c, h, w = x.shape
    x_in = x
    x = ops.group_norm_affine(x, cfg.num_groups, W[p + ".norm.weight"], W[p + ".norm.bias"])
    x = ops.conv2d_bias(x, W[p + ".proj_in.weight"], W[p + ".proj_in.bias"])
    x = x.reshape(b, c, h * w).permute(0, 2, 1)
    t = p + ".transformer_blocks.0"
    n1 = ops.layer_norm(x, W[t + ".norm1.weight"], W[t + ".norm1.bias"])
    x = (identity_self_attention(n1, W, t + ".attn1", n_heads, head_merge) if perturbed else cross_attention(n1, None, W, t + ".attn1", n_heads, head_merge)) + x
    x = cross_attention(ops.layer_norm(x, W[t + ".norm2.weight"], W[t + ".norm2.bias"]), context, W, t + ".attn2", n_heads, head_merge) + x
    x = feed_forward(ops.layer_norm(x, W[t + ".norm3.weight"], W[t + ".norm3.bias"]), W, t + ".ff") + x
    x = x.permute(0, 2, 1).reshape(b, c, h, w)
    return ops.conv2d_bias(x, W[p + ".proj_out.weight"], W[p + ".proj_out.bias"]) + x_in


def unet_forward(x, timesteps, context, W, perturb=(), cfg=SD15, head_merge="reference_exact"):
    """oracle.unet_forward with the identity self-attention in the SpatialTransformers of the blocks named in ``perturb`` (names of ``layers``);
    perturb = (): oracle.unet_forward itself."""
    unknown = set(perturb) - set(layers(cfg))
    assert not unknown, unknown
    W = {k: ops.as_t(v) for k, v in W.items()}
    x, context = ops.as_t(x), ops.as_t(context)
    t_emb = ops.timestep_embedding(timesteps, cfg.model_channels)
    emb = ops.linear(t_emb, W["time_embed.0.weight"], W["time_embed.0.bias"])
    emb = ops.linear(ops.silu(emb), W["time_embed.2.weight"], W["time_embed.2.bias"])
    inp, mid, out = _graph(cfg)

    def run(x, l, p, block):
        if l[0] == "conv": return ops.conv2d_bias(x, W[p + ".weight"], W[p + ".bias"], (1, 1))
        if l[0] == "res": return resblock(x, emb, W, p, cfg)
        if l[0] == "st": return _spatial_transformer(x, context, W, p, cfg.n_heads, cfg, head_merge, block in perturb)
        if l[0] == "down": return ops.conv2d_bias(x, W[p + ".op.weight"], W[p + ".op.bias"], (1, 1), (2, 2))
        if l[0] == "up": return ops.conv2d_bias(ops.upsample_nearest2x(x), W[p + ".conv.weight"], W[p + ".conv.bias"], (1, 1))
        raise ValueError(l)

    saved = []
    for i, b in enumerate(inp):
        for j, l in enumerate(b):
            x = run(x, l, f"input_blocks.{i}.{j}", f"input_blocks.{i}")
        saved.append(x)
    for j, l in enumerate(mid):
        x = run(x, l, f"middle_block.{j}", "middle_block")
    for i, b in enumerate(out):
        x = torch.cat((x, saved.pop()), dim=1)
        for j, l in enumerate(b):
            x = run(x, l, f"output_blocks.{i}.{j}", f"output_blocks.{i}")
    x = ops.silu(ops.group_norm_affine(x, cfg.num_groups, W["out.0.weight"], W["out.0.bias"]))
    return ops.conv2d_bias(x, W["out.2.weight"], W["out.2.bias"], (1, 1))


def scale_at(s, a, t):
    """s_t = max(0, s - a (1000 - t))."""
    return max(0.0, float(s) - float(a) * (1000.0 - float(t)))


def combine(e_u, e_p, e_c, g, s_t):
    """The float64 combine; e_u None: without classifier-free guidance."""
    e_p, e_c = np.asarray(e_p, np.float64), np.asarray(e_c, np.float64)
    if e_u is None:
        return e_c + s_t * (e_c - e_p)
    e_u = np.asarray(e_u, np.float64)
    return e_u + g * (e_c - e_u) + s_t * (e_c - e_p)
