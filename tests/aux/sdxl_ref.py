"""CPU references of the SDXL path (tests/test_sdxl_host.py, tests/test_gpu_sdxl.py), assembled from the oracle's block functions the way
tests/aux/sd2_ref.py is:

  * ``graph`` / ``unet_shapes``: the UNet plan with a transformer depth per level and ``label_emb``, stated here from the published SDXL plan
    (not read off the package under test);
  * ``adm_vector``: y = [pooled | Fourier(original h, w, crop top, left, target h, w)] in float64 numpy, from the definition;
  * ``unet_forward``: oracle/unet.py's walk with a loop over ``basic_transformer_block`` for depth, a head count per transformer and
    emb = time_embed(t) + label_emb(y), one row per image;
  * ``trajectory``: the sampled trajectory around it with sd2_ref's float64 tail;
  * ``clip_l_hidden`` / ``big_g``: transformers.CLIPTextModel(output_hidden_states=True).hidden_states[-2] and CLIPTextModelWithProjection in float64 on
    renamed weights."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sd2_ref  # noqa: E402


# ---- the plan --------------------------------------------------------------------------------------------------------------------------------
def graph(cfg):
    """(input_blocks, middle, output_blocks): lists of ('conv', cin, cout) | ('res', cin, cout) | ('st', ch, depth) | ('down', ch) | ('up', ch) --
    oracle/unet.py::_graph with cfg.transformer_depth[level] blocks per transformer (none at depth 0), the middle block at the last level's depth."""
    mc, td = cfg.model_channels, cfg.transformer_depth
    inp, chans, ch, nlev = [[("conv", cfg.in_channels, mc)]], [mc], mc, len(cfg.channel_mult)
    for lev, mult in enumerate(cfg.channel_mult):
        for _ in range(cfg.num_res_blocks):
            blk = [("res", ch, mc * mult)]
            ch = mc * mult
            if td[lev]:
                blk.append(("st", ch, td[lev]))
            inp.append(blk); chans.append(ch)
        if lev != nlev - 1:
            inp.append([("down", ch)]); chans.append(ch)
    mid = [("res", ch, ch), ("st", ch, td[-1]), ("res", ch, ch)]
    out = []
    for lev in reversed(range(nlev)):
        mult = cfg.channel_mult[lev]
        for i in range(cfg.num_res_blocks + 1):
            blk = [("res", ch + chans.pop(), mc * mult)]
            ch = mc * mult
            if td[lev]:
                blk.append(("st", ch, td[lev]))
            if lev > 0 and i == cfg.num_res_blocks:
                blk.append(("up", ch))
            out.append(blk)
    return inp, mid, out


def unet_shapes(cfg):
    """name -> shape of every tensor of the UNet, LDM names (oracle/unet.py::unet_param_shapes with depth and label_emb)."""
    P, emb, cd = {}, 4 * cfg.model_channels, cfg.context_dim

    def lin(p, i, o, bias=True):
        P[p + ".weight"] = (o, i)
        if bias:
            P[p + ".bias"] = (o,)

    def conv(p, i, o, k):
        P[p + ".weight"], P[p + ".bias"] = (o, i, k, k), (o,)

    def norm(p, c):
        P[p + ".weight"], P[p + ".bias"] = (c,), (c,)

    def block(p, b):
        for j, l in enumerate(b):
            q = f"{p}.{j}"
            if l[0] == "conv":
                conv(q, l[1], l[2], 3)
            elif l[0] == "res":
                i, o = l[1], l[2]
                norm(q + ".in_layers.0", i); conv(q + ".in_layers.2", i, o, 3); lin(q + ".emb_layers.1", emb, o)
                norm(q + ".out_layers.0", o); conv(q + ".out_layers.3", o, o, 3)
                if i != o:
                    conv(q + ".skip_connection", i, o, 1)
            elif l[0] == "st":
                c = l[1]
                norm(q + ".norm", c); conv(q + ".proj_in", c, c, 1); conv(q + ".proj_out", c, c, 1)
                for d in range(l[2]):
                    t = f"{q}.transformer_blocks.{d}"
                    for a, kd in (("attn1", c), ("attn2", cd)):
                        lin(f"{t}.{a}.to_q", c, c, False); lin(f"{t}.{a}.to_k", kd, c, False); lin(f"{t}.{a}.to_v", kd, c, False); lin(f"{t}.{a}.to_out.0", c, c)
                    lin(t + ".ff.net.0.proj", c, 8 * c); lin(t + ".ff.net.2", 4 * c, c)
                    norm(t + ".norm1", c); norm(t + ".norm2", c); norm(t + ".norm3", c)
            elif l[0] == "down":
                conv(q + ".op", l[1], l[1], 3)
            elif l[0] == "up":
                conv(q + ".conv", l[1], l[1], 3)

    lin("time_embed.0", cfg.model_channels, emb); lin("time_embed.2", emb, emb)
    lin("label_emb.0.0", cfg.adm_in_channels, emb); lin("label_emb.0.2", emb, emb)
    inp, mid, out = graph(cfg)
    for i, b in enumerate(inp):
        block(f"input_blocks.{i}", b)
    block("middle_block", mid)
    for i, b in enumerate(out):
        block(f"output_blocks.{i}", b)
    norm("out.0", cfg.model_channels); conv("out.2", cfg.model_channels, cfg.out_channels, 3)
    return P


# ---- the vector conditioning -------------------------------------------------------------------------------------------------------------------
def fourier(t, dim, max_period=10000.0):
    """[cos(t f_i) | sin(t f_i)], f_i = max_period^(-i / (dim / 2)), i < dim / 2: float64, t of any shape -> (..., dim)."""
    half = dim // 2
    f = np.exp(-np.log(np.float64(max_period)) * np.arange(half, dtype=np.float64) / half)
    a = np.asarray(t, np.float64)[..., None] * f
    return np.concatenate((np.cos(a), np.sin(a)), axis=-1)


def adm_vector(pooled, ids, dim):
    """y (R, P + 6 dim) = [pooled | emb(ids[:, 0]) | .. | emb(ids[:, 5])] in float64; ids (R, 6) = original h, w, crop top, left, target h, w."""
    pooled, ids = np.asarray(pooled, np.float64), np.asarray(ids, np.float64)
    assert ids.shape == (pooled.shape[0], 6), ids.shape
    return np.concatenate([pooled] + [fourier(ids[:, k], dim) for k in range(6)], axis=1)


def pooled_index(ids):
    """OpenCLIP's pooling position per prompt: the first position of the highest token id (the end-of-text token has the highest id of the vocabulary)."""
    ids = np.asarray(ids)
    return np.array([int(np.flatnonzero(row == row.max())[0]) for row in ids])


# ---- the UNet --------------------------------------------------------------------------------------------------------------------------------
def unet_forward(x, timesteps, context, y, W, cfg, head_merge="reference_exact"):
    """The SDXL UNet: x (B, C, H, W), context (B, T, D), y (B, adm) one vector per image.  W: torch fp32 tensors by LDM name."""
    import torch
    from oracle import ops
    from oracle import unet as U
    ocfg = sd2_ref.oracle_cfg(cfg)
    W = {k: ops.as_t(v) for k, v in W.items()}
    x, context = ops.as_t(x), ops.as_t(context)
    t_emb = ops.timestep_embedding(timesteps, ocfg.model_channels)
    emb = ops.linear(t_emb, W["time_embed.0.weight"], W["time_embed.0.bias"])
    emb = ops.linear(ops.silu(emb), W["time_embed.2.weight"], W["time_embed.2.bias"])
    ye = ops.linear(ops.as_t(np.asarray(y, np.float32)), W["label_emb.0.0.weight"], W["label_emb.0.0.bias"])
    ye = ops.linear(ops.silu(ye), W["label_emb.0.2.weight"], W["label_emb.0.2.bias"])
    emb = emb + ye                                          # (1, E) + (B, E): one row per image
    inp, mid, out = graph(cfg)

    def st(x, p, ch, depth):
        b, c, h, w = x.shape
        x_in = x
        x = ops.group_norm_affine(x, ocfg.num_groups, W[p + ".norm.weight"], W[p + ".norm.bias"])
        x = ops.conv2d_bias(x, W[p + ".proj_in.weight"], W[p + ".proj_in.bias"])
        x = x.reshape(b, c, h * w).permute(0, 2, 1)
        for d in range(depth):
            x = U.basic_transformer_block(x, context, W, f"{p}.transformer_blocks.{d}", ch // cfg.d_head, head_merge)
        x = x.permute(0, 2, 1).reshape(b, c, h, w)
        return ops.conv2d_bias(x, W[p + ".proj_out.weight"], W[p + ".proj_out.bias"]) + x_in

    def run(x, l, p):
        if l[0] == "conv": return ops.conv2d_bias(x, W[p + ".weight"], W[p + ".bias"], (1, 1))
        if l[0] == "res": return U.resblock(x, emb, W, p, ocfg)
        if l[0] == "st": return st(x, p, l[1], l[2])
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


def trajectory(W, cfg, contexts, ys, lat0, sch, g, vpred=False, phi=None, x0_init=None, mask=None, noise2=None):
    """sd2_ref.trajectory with a vector per guidance group: contexts[k] (B, T, D) and ys[k] (B, adm), unconditional group first; vpred, phi, x0_init,
    mask and noise2 (the tag-2 normals of step i) as sd2_ref.tail takes them."""
    x, xp = lat0.astype(np.float64), np.zeros(lat0.shape)
    for i, t in enumerate(sch.timesteps):
        x32, tt = x.astype(np.float32), np.array([t], np.float32)
        outs = [unet_forward(x32, tt, contexts[k], ys[k], W, cfg).numpy().astype(np.float64) for k in range(len(contexts))]
        r = sd2_ref.tail(x, outs, xp, sch.alphas[i], sch.alphas_prev[i], g, sch.coeffs[i], phi=phi, vpred=vpred, x0_init=x0_init, mask=mask,
                         z2=noise2(i) if noise2 else 0.0)
        x, xp = r["latent"], r["x0"]
    return x


# ---- what the earlier configurations computed before SDXL ----------------------------------------------------------------------------------------
def parent_recipe(name, steps=2, guidance=7.5, seed=0x243F6A8885A308D3):
    """The latent after a ``steps``-step DPM++2M run of configuration ``name`` ("TINY", "TINY_V2") with synthetic weights, B = 2 at 16 x 16, through
    compile / start / run -- on whichever tinyfusers_amd is importable (the tree's, or the parent commit's when the golden file is made).  The GEMM
    tiles come from the cost model alone (tf_gemm_autotune(0)): a timed choice could differ between two processes."""
    import tinyfusers_amd.storage.tensor as T
    from tinyfusers_amd.native import hip
    from tinyfusers_amd.storage.state import param_shapes, update_state
    from tinyfusers_amd.storage.synth import synth_normal, synth_state_dict
    from tinyfusers_amd.variants import samplers as S
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision import unet as U
    T.ensure_init(0)
    cfg = getattr(U, name)
    hip.tf_gemm_autotune(0)
    try:
        sd = StableDiffusion(cfg)
        update_state(sd.model.diffusion_model, synth_state_dict(param_shapes(sd.model.diffusion_model), 5), "")
        ctx = T.DeviceArray.from_numpy(synth_normal(5, "c", (2, 13, cfg.context_dim)).astype(np.float16))
        unc = T.DeviceArray.from_numpy(synth_normal(5, "u", (2, 13, cfg.context_dim)).astype(np.float16))
        lat = sd.latent_from_numpy(np.zeros((2, 4, 16, 16), np.float32))
        sd.compile(unc, ctx, lat, sampler=S.DPMSolverPP2M().schedule(steps))
        sd.start(seed=seed)
        sd.run(guidance); sd.synchronize()
        return lat.numpy().copy()
    finally:
        hip.tf_gemm_autotune(int(os.environ.get("TF_GEMM_AUTOTUNE") or 1))      # (what tinyfusers_amd.native set at import)


# ---- the text towers ---------------------------------------------------------------------------------------------------------------------------
def _hf_text(kind, state, width, layers, heads, mlp, vocab, positions, act, ids, projection=None):
    import torch
    import transformers
    hcfg = transformers.CLIPTextConfig(vocab_size=vocab, hidden_size=width, intermediate_size=mlp, num_hidden_layers=layers, num_attention_heads=heads,
                                       max_position_embeddings=positions, hidden_act=act, layer_norm_eps=1e-5, bos_token_id=0, pad_token_id=1, eos_token_id=2,
                                       projection_dim=projection or width)
    model = getattr(transformers, kind)(hcfg).double().eval()
    own = model.state_dict()
    anchor = next(k for k in own if k.endswith("embeddings.token_embedding.weight"))
    prefix = anchor[:-len("embeddings.token_embedding.weight")]
    hf = {(k if k == "text_projection.weight" else prefix + k): torch.from_numpy(np.asarray(v, np.float64)) for k, v in state.items()}
    missing = [k for k in own if k not in hf and not k.endswith("position_ids")]
    assert not missing, missing
    model.load_state_dict(hf, strict=False)
    with torch.no_grad():
        return model(input_ids=torch.from_numpy(np.asarray(ids, np.int64)), output_hidden_states=True)


def clip_l_hidden(state, ids, width, layers, heads, mlp, vocab, positions=77):
    """(B, T, width) float64: hidden_states[-2] of transformers.CLIPTextModel (quick_gelu) on a CLIPTextTransformer's tensors -- the output of encoder
    layer ``layers - 1``, before the final LayerNorm.  ``state``: names below ``text_model.``, which are transformers' own."""
    return _hf_text("CLIPTextModel", state, width, layers, heads, mlp, vocab, positions, "quick_gelu", ids).hidden_states[-2].numpy()


def big_g(state, cfg, ids):
    """(hidden_states[-2] (B, T, W), text_embeds (B, W)) of transformers.CLIPTextModelWithProjection (exact GELU, every layer) on an OpenCLIP tower's
    tensors renamed by sd2_ref.ldm_to_hf; its Linear holds text_projection transposed (OpenCLIP multiplies by the bare matrix)."""
    hf = sd2_ref.ldm_to_hf(state, cfg.layers)
    hf["text_projection.weight"] = np.asarray(state["text_projection"]).T
    out = _hf_text("CLIPTextModelWithProjection", hf, cfg.width, cfg.layers, cfg.heads, cfg.mlp, cfg.vocab, cfg.positions, "gelu", ids, projection=cfg.width)
    return out.hidden_states[-2].numpy(), out.text_embeds.numpy()
