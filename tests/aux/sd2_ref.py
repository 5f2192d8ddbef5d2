"""CPU references of the SD-2.x path (tests/test_sd2_host.py, tests/test_gpu_sampler_tail.py, tests/test_gpu_sd2.py):

  * ``tail``: the float64 restatement of tf_sampler_tail_* (csrc/sampler.hip) -- combine, CFG rescale, eps / v, update, blend -- with the magnitudes
    the tests' budgets are built from;
  * ``unet_forward``: oracle/unet.py's UNet walk with a head count per SpatialTransformer (channels // d_head), assembled from the oracle's own
    block functions, which take the head count as an argument;
  * ``text_tower``: transformers.CLIPTextModel (hidden_act "gelu", layers - 1 layers) in float64 on the OpenCLIP weights renamed: its
    last_hidden_state is the penultimate resblock's output through the final LayerNorm."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


# ---- the tail --------------------------------------------------------------------------------------------------------------------------
def combine(groups, g, g_i=None):
    """(e, E, e_t): the combined output of 1, 2 or 3 guidance groups (float64 arrays), the sum of the magnitudes that enter it, the text group."""
    a = [np.abs(x) for x in groups]
    if len(groups) == 1:
        return groups[0], a[0], groups[0]
    if len(groups) == 2:
        u, c = groups
        return u + g * (c - u), a[0] + abs(g) * (a[1] + a[0]), c
    e0, e1, e2 = groups
    return e0 + g * (e2 - e1) + g_i * (e1 - e0), a[0] + abs(g) * (a[2] + a[1]) + abs(g_i) * (a[1] + a[0]), e2


def rescale_factor(e, e_t):
    """f per image (B, 1, 1, 1): std(e_t) / std(e) over the image's elements, 1 where std(e) == 0 (the 1 / (n - 1) of both cancels)."""
    b = e.shape[0]
    se, st = e.reshape(b, -1).std(axis=1), e_t.reshape(b, -1).std(axis=1)
    f = np.where(se > 0, st / np.where(se > 0, se, 1.0), 1.0)
    return f.reshape((b,) + (1,) * (e.ndim - 1))


def tail(x, groups, hist, a_t, a_s, g, row, z=0.0, g_i=None, phi=None, vpred=False, x0_init=None, mask=None, z2=0.0):
    """float64 tf_sampler_tail_*.  x, hist, groups[k], x0_init (B,C,H,W); mask (B,1,H,W); a_t, a_s, g, g_i, phi and the row as the fp32 values the
    device reads; z / z2 the tag-1 / tag-2 normals.  -> dict: latent, x0, f, e (the output the update ran on), E (its magnitude bound)."""
    a_t, a_s = np.float64(np.float32(a_t)), np.float64(np.float32(a_s))
    c_x, c_0, c_1, c_n = (np.float64(np.float32(c)) for c in row)
    e, E, e_t = combine(groups, g, g_i)
    f = np.ones((x.shape[0], 1, 1, 1))
    if phi is not None:
        f = rescale_factor(e, e_t)
        e, E = phi * (e * f) + (1 - phi) * e, (phi * f + (1 - phi)) * E
    s1, r = np.sqrt(1 - a_t), np.sqrt(a_t)
    x0 = r * x - s1 * e if vpred else (x - s1 * e) / r
    X0 = r * np.abs(x) + s1 * E if vpred else (np.abs(x) + s1 * E) / r
    xn = c_x * x + c_0 * x0 + (c_1 * hist if c_1 != 0 else 0.0) + c_n * z
    mag = abs(c_x) * np.abs(x) + abs(c_0) * X0 + abs(c_1) * np.abs(hist) + abs(c_n) * np.abs(z)
    if mask is not None:
        known = np.sqrt(a_s) * x0_init + np.sqrt(1 - a_s) * z2
        xn = mask * xn + (1 - mask) * known
        mag = mask * mag + (1 - mask) * (np.sqrt(a_s) * np.abs(x0_init) + np.sqrt(1 - a_s) * np.abs(z2))
    return dict(latent=xn, x0=x0, f=f, e=e, E=E, X0=X0, mag=mag)


# ---- the UNet with a head count per level --------------------------------------------------------------------------------------------------
def oracle_cfg(cfg):
    """oracle.UNetConfig of a tinyfusers_amd UNetConfig (its n_heads is not used: ``unet_forward`` hands every block its own count)."""
    import oracle
    return oracle.UNetConfig(in_channels=cfg.in_channels, out_channels=cfg.out_channels, model_channels=cfg.model_channels, channel_mult=cfg.channel_mult,
                             num_res_blocks=cfg.num_res_blocks, attention_levels=cfg.attention_levels, n_heads=1, context_dim=cfg.context_dim)


def unet_forward(x, timesteps, context, W, cfg, head_merge="reference_exact", perturb=()):
    """oracle.unet_forward (vision/unet.py:51-76) for a configuration with d_head: SpatialTransformer at ch channels runs ch // d_head heads.
    perturb: blocks ("middle_block", "input_blocks.1", ...) whose self-attention is the identity (tests/aux/pag_ref.py's transformer)."""
    import torch
    from oracle import ops
    from oracle import unet as U
    import pag_ref
    ocfg = oracle_cfg(cfg)
    W = {k: ops.as_t(v) for k, v in W.items()}
    x, context = ops.as_t(x), ops.as_t(context)
    t_emb = ops.timestep_embedding(timesteps, ocfg.model_channels)
    emb = ops.linear(t_emb, W["time_embed.0.weight"], W["time_embed.0.bias"])
    emb = ops.linear(ops.silu(emb), W["time_embed.2.weight"], W["time_embed.2.bias"])
    inp, mid, out = U._graph(ocfg)

    def run(x, l, p):
        if l[0] == "conv": return ops.conv2d_bias(x, W[p + ".weight"], W[p + ".bias"], (1, 1))
        if l[0] == "res": return U.resblock(x, emb, W, p, ocfg)
        if l[0] == "st":
            heads = l[1] // cfg.d_head if cfg.d_head else cfg.n_heads
            if p.rsplit(".", 1)[0] in perturb:
                return pag_ref._spatial_transformer(x, context, W, p, heads, ocfg, head_merge, True)
            return U.spatial_transformer(x, context, W, p, heads, ocfg, head_merge)
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
    x = ops.silu(ops.group_norm_affine(x, ocfg.num_groups, W["out.0.weight"], W["out.0.bias"]))
    return ops.conv2d_bias(x, W["out.2.weight"], W["out.2.bias"], (1, 1))


def unet_shapes(cfg):
    import oracle
    return oracle.unet_param_shapes(oracle_cfg(cfg))


def trajectory(W, cfg, contexts, lat0, sch, g, vpred=False, phi=None, g_i=None, noise=None, x0_init=None, mask=None, noise2=None, perturb=None):
    """The sampled trajectory in float64 around the oracle's forward: ``contexts`` one (B, T, D) array per guidance group, ``perturb`` None or one
    tuple of perturbed blocks per group, noise(i) / noise2(i) the tag-1 / tag-2 normals of step i (None: not drawn); g (and g_i) may be callables
    of the timestep."""
    x, xp = lat0.astype(np.float64), np.zeros(lat0.shape)
    G = len(contexts)
    val = lambda v, t: v(t) if callable(v) else v
    for i, t in enumerate(sch.timesteps):
        x32, tt = x.astype(np.float32), np.array([t], np.float32)
        outs = [unet_forward(x32, tt, contexts[k], W, cfg, perturb=perturb[k] if perturb else ()).numpy().astype(np.float64) for k in range(G)]
        r = tail(x, outs, xp, sch.alphas[i], sch.alphas_prev[i], val(g, t), sch.coeffs[i], z=noise(i) if noise else 0.0, g_i=val(g_i, t),
                 phi=phi, vpred=vpred, x0_init=x0_init, mask=mask, z2=noise2(i) if noise2 else 0.0)
        x, xp = r["latent"], r["x0"]
    return x


# ---- the OpenCLIP text tower ---------------------------------------------------------------------------------------------------------------
def ldm_to_hf(state, layers):
    """An OpenCLIP text tower's tensors (names below cond_stage_model.model.) under transformers' CLIPTextModel names, for its first ``layers``
    resblocks: in_proj_weight / in_proj_bias split into q | k | v (rows 0:W, W:2W, 2W:3W)."""
    w = int(np.shape(state["token_embedding.weight"])[1])
    out = {"embeddings.token_embedding.weight": state["token_embedding.weight"], "embeddings.position_embedding.weight": state["positional_embedding"],
           "final_layer_norm.weight": state["ln_final.weight"], "final_layer_norm.bias": state["ln_final.bias"]}
    for i in range(layers):
        s, d = f"transformer.resblocks.{i}.", f"encoder.layers.{i}."
        for k, name in enumerate(("q_proj", "k_proj", "v_proj")):
            out[d + f"self_attn.{name}.weight"] = state[s + "attn.in_proj_weight"][k * w:(k + 1) * w]
            out[d + f"self_attn.{name}.bias"] = state[s + "attn.in_proj_bias"][k * w:(k + 1) * w]
        for a, b in (("attn.out_proj", "self_attn.out_proj"), ("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"), ("mlp.c_fc", "mlp.fc1"), ("mlp.c_proj", "mlp.fc2")):
            out[d + b + ".weight"], out[d + b + ".bias"] = state[s + a + ".weight"], state[s + a + ".bias"]
    return out


def text_tower(state, cfg, ids):
    """(B, T, width) float64: CLIPTextModel over layers - 1 layers with the exact GELU, causal mask, no padding mask."""
    import torch
    from transformers import CLIPTextConfig, CLIPTextModel
    hcfg = CLIPTextConfig(vocab_size=cfg.vocab, hidden_size=cfg.width, intermediate_size=cfg.mlp, num_hidden_layers=cfg.layers - 1, num_attention_heads=cfg.heads,
                          max_position_embeddings=cfg.positions, hidden_act="gelu", layer_norm_eps=cfg.eps, bos_token_id=0, pad_token_id=1, eos_token_id=2)
    model = CLIPTextModel(hcfg).double().eval()
    own = model.state_dict()
    prefix = next(k for k in own if k.endswith("embeddings.token_embedding.weight"))[:-len("embeddings.token_embedding.weight")]
    hf = {prefix + k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in ldm_to_hf(state, cfg.layers - 1).items()}
    missing = [k for k in own if k not in hf and not k.endswith("position_ids")]
    assert not missing, missing
    model.load_state_dict(hf, strict=False)
    with torch.no_grad():
        return model(input_ids=torch.from_numpy(np.asarray(ids, np.int64))).last_hidden_state.numpy()
