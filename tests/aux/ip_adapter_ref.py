"""CPU restatement (fp32, torch-CPU) of an IP-Adapter (ip-adapter_sd15) and of the UNet forward with decoupled cross-attention -- TEST
INFRASTRUCTURE, composed from oracle.unet's own pieces (_graph, resblock, feed_forward, cross_attention's op sequence) and oracle.ops the way
tests/aux/controlnet_oracle.py composes its forward.

Published form (Ye et al. 2023; ip_adapter.py / attention_processor.py of the public repository): image tokens = LayerNorm(Linear(embeds)
.reshape(N, T, ctx)); in every cross-attention, out = to_out(attn(q, k, v) + s attn(q, to_k_ip(tokens), to_v_ip(tokens))), the same q.  Weights:
the flat dict of the file -- image_proj.{proj,norm}.{weight,bias}, ip_adapter.{n}.to_{k,v}_ip.weight with n odd in the order DOWN, UP, MID."""
import numpy as np
import torch

from oracle import ops
from oracle.unet import SD15, UNetConfig, _graph, feed_forward, resblock

SD15_PATHS = [(1, "input_blocks.1.1"), (3, "input_blocks.2.1"), (5, "input_blocks.4.1"), (7, "input_blocks.5.1"), (9, "input_blocks.7.1"),
              (11, "input_blocks.8.1"), (13, "output_blocks.3.1"), (15, "output_blocks.4.1"), (17, "output_blocks.5.1"), (19, "output_blocks.6.1"),
              (21, "output_blocks.7.1"), (23, "output_blocks.8.1"), (25, "output_blocks.9.1"), (27, "output_blocks.10.1"), (29, "output_blocks.11.1"),
              (31, "middle_block.1")]


def paths(cfg: UNetConfig = SD15):
    """[(n, module path)] from the oracle's block lists: input blocks, output blocks, then the middle block."""
    inp, mid, out = _graph(cfg)
    found = [f"{part}.{i}.{j}" for part, blocks in (("input_blocks", inp), ("output_blocks", out)) for i, b in enumerate(blocks) for j, l in enumerate(b) if l[0] == "st"]
    found += [f"middle_block.{j}" for j, l in enumerate(mid) if l[0] == "st"]
    return [(2 * k + 1, p) for k, p in enumerate(found)]


def adapter_param_shapes(cfg: UNetConfig = SD15, tokens=4, embed_dim=1024):
    inp, mid, out = _graph(cfg)
    width = {f"{part}.{i}.{j}": l[1] for part, blocks in (("input_blocks", inp), ("output_blocks", out)) for i, b in enumerate(blocks) for j, l in enumerate(b) if l[0] == "st"}
    width.update({f"middle_block.{j}": l[1] for j, l in enumerate(mid) if l[0] == "st"})
    c = cfg.context_dim
    P = {"image_proj.proj.weight": (tokens * c, embed_dim), "image_proj.proj.bias": (tokens * c,), "image_proj.norm.weight": (c,), "image_proj.norm.bias": (c,)}
    for n, p in paths(cfg):
        P[f"ip_adapter.{n}.to_k_ip.weight"] = P[f"ip_adapter.{n}.to_v_ip.weight"] = (width[p], c)
    return P


def image_tokens(embeds, A, ctx):
    """(N, E) -> (N, T, ctx)."""
    x = ops.linear(ops.as_t(embeds), ops.as_t(A["image_proj.proj.weight"]), ops.as_t(A["image_proj.proj.bias"]))
    return ops.layer_norm(x.reshape(x.shape[0], -1, ctx), ops.as_t(A["image_proj.norm.weight"]), ops.as_t(A["image_proj.norm.bias"]))


def context_kv(tokens, A, cfg=SD15):
    """The row-concatenated K_ip | V_ip projection of every block in adapter order: (N, T, kv_n)."""
    t = ops.as_t(tokens)
    return torch.cat([ops.linear(t, ops.as_t(A[f"ip_adapter.{n}.to_{kv}_ip.weight"])) for n, _ in paths(cfg) for kv in "kv"], dim=-1)


def _cross_attention_ip(x, context, W, p, n_heads, head_merge, tokens, wk, wv, s):
    """oracle.unet.cross_attention with the second term: the same q against the image tokens, added before to_out."""
    q = ops.linear(x, W[p + ".to_q.weight"])
    b, d = x.shape[0], q.shape[-1] // n_heads
    heads = lambda y: y.reshape(b, -1, n_heads, d).permute(0, 2, 1, 3)
    o = ops.scaled_dot_product_attention(heads(q), heads(ops.linear(context, W[p + ".to_k.weight"])), heads(ops.linear(context, W[p + ".to_v.weight"])))
    o = o + s * ops.scaled_dot_product_attention(heads(q), heads(ops.linear(tokens, wk)), heads(ops.linear(tokens, wv)))
    o = o.reshape(b, -1, n_heads * d) if head_merge == "reference_exact" else o.permute(0, 2, 1, 3).reshape(b, -1, n_heads * d)
    return ops.linear(o, W[p + ".to_out.0.weight"], W[p + ".to_out.0.bias"])


def _spatial_transformer_ip(x, context, W, p, n_heads, cfg, head_merge, tokens, wk, wv, s):
    from oracle.unet import cross_attention
    b, c, h, w = x.shape
    x_in = x
    x = ops.group_norm_affine(x, cfg.num_groups, W[p + ".norm.weight"], W[p + ".norm.bias"])
    x = ops.conv2d_bias(x, W[p + ".proj_in.weight"], W[p + ".proj_in.bias"])
    x = x.reshape(b, c, h * w).permute(0, 2, 1)
    t = p + ".transformer_blocks.0"
    x = cross_attention(ops.layer_norm(x, W[t + ".norm1.weight"], W[t + ".norm1.bias"]), None, W, t + ".attn1", n_heads, head_merge) + x
    x = _cross_attention_ip(ops.layer_norm(x, W[t + ".norm2.weight"], W[t + ".norm2.bias"]), context, W, t + ".attn2", n_heads, head_merge, tokens, wk, wv, s) + x
    x = feed_forward(ops.layer_norm(x, W[t + ".norm3.weight"], W[t + ".norm3.bias"]), W, t + ".ff") + x
    x = x.permute(0, 2, 1).reshape(b, c, h, w)
    return ops.conv2d_bias(x, W[p + ".proj_out.weight"], W[p + ".proj_out.bias"]) + x_in


def unet_forward(x, timesteps, context, W, A, tokens, scale=1.0, cfg=SD15, head_merge="reference_exact"):
    """oracle.unet_forward with the adapter A acting in every cross-attention.  tokens (b, T, ctx): the image tokens of every row of x; scale: one
    float or one per cross-attention in adapter order."""
    W = {k: ops.as_t(v) for k, v in W.items()}
    A = {k: ops.as_t(v) for k, v in A.items()}
    x, context, tokens = ops.as_t(x), ops.as_t(context), ops.as_t(tokens)
    table = paths(cfg)
    s = dict(zip((p for _, p in table), np.broadcast_to(np.asarray(scale, np.float32), (len(table),)).tolist()))
    idx = {p: n for n, p in table}
    t_emb = ops.timestep_embedding(timesteps, cfg.model_channels)
    emb = ops.linear(t_emb, W["time_embed.0.weight"], W["time_embed.0.bias"])
    emb = ops.linear(ops.silu(emb), W["time_embed.2.weight"], W["time_embed.2.bias"])
    inp, mid, out = _graph(cfg)

    def run(x, l, p):
        if l[0] == "conv": return ops.conv2d_bias(x, W[p + ".weight"], W[p + ".bias"], (1, 1))
        if l[0] == "res": return resblock(x, emb, W, p, cfg)
        if l[0] == "st":
            return _spatial_transformer_ip(x, context, W, p, cfg.n_heads, cfg, head_merge, tokens, A[f"ip_adapter.{idx[p]}.to_k_ip.weight"],
                                           A[f"ip_adapter.{idx[p]}.to_v_ip.weight"], s[p])
        if l[0] == "down": return ops.conv2d_bias(x, W[p + ".op.weight"], W[p + ".op.bias"], (1, 1), (2, 2))
        if l[0] == "up": return ops.conv2d_bias(ops.upsample_nearest2x(x), W[p + ".conv.weight"], W[p + ".conv.bias"], (1, 1))
        raise ValueError(l)

    saved = []
    for i, b in enumerate(inp):
        for j, l in enumerate(b):
            x = run(x, l, f"input_blocks.{i}.{j}")
        saved.append(x)
    for j, l in enumerate(mid):
        x = run(x, l, f"middle_block.{j}")
    for i, b in enumerate(out):
        x = torch.cat((x, saved.pop()), dim=1)
        for j, l in enumerate(b):
            x = run(x, l, f"output_blocks.{i}.{j}")
    x = ops.silu(ops.group_norm_affine(x, cfg.num_groups, W["out.0.weight"], W["out.0.bias"]))
    return ops.conv2d_bias(x, W["out.2.weight"], W["out.2.bias"], (1, 1))
