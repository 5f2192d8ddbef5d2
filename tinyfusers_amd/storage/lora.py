"""LoRA adapters for the SD-1.x models: reading adapter files, naming the targets, deciding the scales, and the device-side merge.

The reference has no adapters (its weights come from update_state alone, storage/state.py:4-23); nothing here is ported.  An adapter of a
weight W (N, Kd) -- a Linear's (out, in), or a conv's KRSC storage (K, R S C) -- is a pair up (N, r), down (r, Kd) and a number alpha; the
merged weight is W' = round16(W + sum_i s_i up_i down_i), s_i = weight_i alpha_i / r_i, computed by ONE launch of tf_lora_merge_16 per
module (csrc/lora.hip) from the pristine base weight into a fresh buffer.  Swapping ``module.weight`` for the merged handle is all the rest
of the package needs: every derived buffer (LayerNorm folds, GEGLU packs, the FF2 x proj_out product, the 1x1-skip fold, the batched
time-embedding GEMV and K|V GEMM, the e4m3 packs) is keyed by ``DeviceArray.wkey`` and follows by itself.

Nothing here needs a device to be imported, to parse a file or to name the targets.

File formats (``parse_lora``):
  * kohya: ``<module>.lora_down.weight`` (r, in...), ``<module>.lora_up.weight`` (out, r[, 1, 1]), optional ``<module>.alpha`` (default: r);
    <module> = ``lora_unet_...`` / ``lora_te_...`` (diffusers module path with '.' -> '_');
  * PEFT / diffusers: ``unet.<dotted module>.lora_A.weight`` (= down) / ``.lora_B.weight`` (= up), optional ``.alpha``, and
    ``text_encoder.<dotted module>.lora_A/B.weight``; the dotted path with '.' -> '_' is the kohya name.
Tensors of any float type are cast to the step's 16-bit type (config.is_bf16()): for an fp32 (or fp16 -> bf16) file that is a ROUNDING of the
adapter's values, once, when it is loaded.
"""
from collections import namedtuple

import numpy as np

MAX_RANK = 256          # ranks above this are refused
MAX_ADAPTERS = 8        # adapters of one tf_lora_merge_16 launch, i.e. active on any one module

LoraWeights = namedtuple("LoraWeights", ["up", "down_t", "alpha", "rank"])
LoraWeights.__doc__ = """One module's adapter on the host, in the kernel's operand layout: up (N, Rp) and down_t (Kd, Rp), both contiguous along the
rank, the rank zero-padded to Rp (a multiple of 32); float16 arrays, or float32 arrays of bfloat16-representable values in the bf16 step."""

_UNSUPPORTED = (("hada_", "LoHa (Hadamard-product) adapters"), ("lokr_", "LoKr (Kronecker-product) adapters"), ("dora_scale", "DoRA (weight-decomposed) adapters"),
                ("lora_mid", "Tucker-decomposed conv adapters (lora_mid)"))


# ---- targets: generated from the module tree ------------------------------------------------------------------------------------------------
def _resnet(names, kohya, path, block):
    from ..vision.conv2d import Conv2d
    names[kohya + "_conv1"] = path + ".in_layers.2"
    names[kohya + "_time_emb_proj"] = path + ".emb_layers.1"
    names[kohya + "_conv2"] = path + ".out_layers.3"
    if isinstance(block.skip_connection, Conv2d):          # (an identity skip has no conv_shortcut)
        names[kohya + "_conv_shortcut"] = path + ".skip_connection"


def _transformer(names, kohya, path, st):
    names[kohya + "_proj_in"] = path + ".proj_in"
    names[kohya + "_proj_out"] = path + ".proj_out"
    for b in range(len(st.transformer_blocks)):
        k, p = f"{kohya}_transformer_blocks_{b}", f"{path}.transformer_blocks.{b}"
        for attn in ("attn1", "attn2"):
            for proj in ("to_q", "to_k", "to_v"):
                names[f"{k}_{attn}_{proj}"] = f"{p}.{attn}.{proj}"
            names[f"{k}_{attn}_to_out_0"] = f"{p}.{attn}.to_out.0"
        names[k + "_ff_net_0_proj"] = p + ".ff.net.0.proj"
        names[k + "_ff_net_2"] = p + ".ff.net.2"


def unet_target_paths(unet):
    """kohya name -> dotted path below the UNet, by a walk over its block plan (vision/unet.py): with nrb = cfg.num_res_blocks, diffusers'
    down_blocks_{l}_{resnets,attentions}_{j} is input_blocks[1 + l (nrb + 1) + j][0 | 1], down_blocks_{l}_downsamplers_0_conv is
    input_blocks[(l + 1)(nrb + 1)][0].op, mid_block_resnets_{0,1} / attentions_0 are middle_block[0, 2] / [1], up_blocks_{u}_{resnets,attentions}_{j}
    is output_blocks[u (nrb + 1) + j][0 | 1] and up_blocks_{u}_upsamplers_0_conv the last element of output_blocks[u (nrb + 1) + nrb], .conv."""
    from ..attention.attention import SpatialTransformer
    from ..vision.resnet import ResBlock
    from ..vision.unet import Downsample, Upsample
    cfg = unet.cfg
    nrb, nlev = cfg.num_res_blocks, len(cfg.channel_mult)
    names = {"lora_unet_conv_in": "input_blocks.0.0", "lora_unet_conv_out": "out.2"}

    def block(kohya_level, j, path, blk):
        assert isinstance(blk[0], ResBlock), path
        _resnet(names, f"{kohya_level}_resnets_{j}", path + ".0", blk[0])
        if len(blk) > 1 and isinstance(blk[1], SpatialTransformer):
            _transformer(names, f"{kohya_level}_attentions_{j}", path + ".1", blk[1])

    for lev in range(nlev):
        for j in range(nrb):
            i = 1 + lev * (nrb + 1) + j
            block(f"lora_unet_down_blocks_{lev}", j, f"input_blocks.{i}", unet.input_blocks[i])
        i = (lev + 1) * (nrb + 1)
        if i < len(unet.input_blocks) and isinstance(unet.input_blocks[i][0], Downsample):
            names[f"lora_unet_down_blocks_{lev}_downsamplers_0_conv"] = f"input_blocks.{i}.0.op"
    mid = unet.middle_block
    _resnet(names, "lora_unet_mid_block_resnets_0", "middle_block.0", mid[0])
    _transformer(names, "lora_unet_mid_block_attentions_0", "middle_block.1", mid[1])
    _resnet(names, "lora_unet_mid_block_resnets_1", "middle_block.2", mid[2])
    for u in range(nlev):
        for j in range(nrb + 1):
            i = u * (nrb + 1) + j
            blk = unet.output_blocks[i]
            block(f"lora_unet_up_blocks_{u}", j, f"output_blocks.{i}", blk)
            if isinstance(blk[-1], Upsample):
                names[f"lora_unet_up_blocks_{u}_upsamplers_0_conv"] = f"output_blocks.{i}.{len(blk) - 1}.conv"
    return names


def text_target_paths(text_model):
    """kohya name -> dotted path below the CLIP text model (vae/encoder.py::CLIPTextTransformer)."""
    names = {}
    for i in range(len(text_model.encoder.layers)):
        for kohya, path in (("self_attn_q_proj", "self_attn.q_proj"), ("self_attn_k_proj", "self_attn.k_proj"), ("self_attn_v_proj", "self_attn.v_proj"),
                            ("self_attn_out_proj", "self_attn.out_proj"), ("mlp_fc1", "mlp.fc1"), ("mlp_fc2", "mlp.fc2")):
            names[f"lora_te_text_model_encoder_layers_{i}_{kohya}"] = f"encoder.layers.{i}.{path}"
    return names


def lora_target_paths(sd):
    """kohya name -> the LDM checkpoint path of the module (param_shapes(sd) lists ``<path>.weight``) for every target of a StableDiffusion."""
    paths = {k: "model.diffusion_model." + p for k, p in unet_target_paths(sd.model.diffusion_model).items()}
    if hasattr(sd.cond_stage_model, "transformer"):          # the SD-1.x CLIP text encoder; the OpenCLIP tower of SD-2.x has no lora_te_* targets
        paths.update({k: "cond_stage_model.transformer.text_model." + p for k, p in text_target_paths(sd.cond_stage_model.transformer.text_model).items()})
    return paths


def _resolve(root, path):
    node = root
    for part in path.split("."):
        if isinstance(node, dict):
            node = node[part]
        elif isinstance(node, (list, tuple)) and not hasattr(node, "_fields"):
            node = node[int(part)]
        else:
            node = getattr(node, part)
    return node


def lora_targets(sd):
    """kohya name -> module (a Linear or a Conv2d) for every adapter target of a StableDiffusion: generated from the UNet's block plan and the
    CLIP text model, never parsed out of the underscore names.  The ControlNet and the VAE are not targets."""
    return {k: _resolve(sd, p) for k, p in lora_target_paths(sd).items()}


def weight_shape(module):
    """The logical weight shape of a target: (out, in) of a Linear, (K, C, R, S) of a Conv2d."""
    from .state import _leaf_shape
    return tuple(int(v) for v in _leaf_shape(module, "weight"))


# ---- parsing --------------------------------------------------------------------------------------------------------------------------------
def _to_numpy(v):
    if hasattr(v, "detach"):
        v = v.detach().cpu()
        if str(v.dtype) == "torch.bfloat16":
            v = v.float()
        v = v.numpy()
    return np.asarray(v)


def _split_key(key):
    """(kohya module name, 'down' | 'up' | 'alpha') of one key of an adapter file, or None where the key is not an adapter tensor's."""
    for suffix, what in ((".lora_down.weight", "down"), (".lora_up.weight", "up"), (".lora_A.weight", "down"), (".lora_B.weight", "up"), (".alpha", "alpha")):
        if key.endswith(suffix):
            mod = key[:-len(suffix)]
            break
    else:
        return None
    if mod.startswith("unet."):
        mod = "lora_unet_" + mod[len("unet."):].replace(".", "_")
    elif mod.startswith("text_encoder."):
        mod = "lora_te_" + mod[len("text_encoder."):].replace(".", "_")
    return mod, what


def parse_lora(src):
    """A path (.safetensors, torch-zip .ckpt / .pt) or a dict of arrays -> ({kohya module name: {'down', 'up', 'alpha', 'keys'}}, [keys that are not
    adapter tensors]).  Refuses, by name and with the reason, what this package does not merge: LoHa, LoKr, DoRA, Tucker convs and the old
    diffusers attention-processor files."""
    if isinstance(src, dict):
        tensors = src
    else:
        from .unpicker import load_checkpoint
        tensors = load_checkpoint(str(src))
    mods, other = {}, []
    for key in tensors:
        for mark, why in _UNSUPPORTED:
            if mark in key:
                raise ValueError(f"load_lora: {key}: {why} are not supported (plain LoRA / LoCon pairs lora_down, lora_up, alpha only)")
        if ".processor." in key and "_lora." in key:
            raise ValueError(f"load_lora: {key}: the old diffusers attention-processor format (*.processor.*_lora.*) is not supported -- "
                             "convert the file to kohya or PEFT keys")
        sk = _split_key(key)
        if sk is None:
            other.append(key)
            continue
        mod, what = sk
        m = mods.setdefault(mod, {"keys": {}})
        if what in m:
            raise ValueError(f"load_lora: {key}: a second {what} tensor for {mod} (also {m['keys'][what]})")
        m[what], m["keys"][what] = _to_numpy(tensors[key]), key
    return mods, other


def _cast16(x, bf16):
    """Float array -> the step's 16-bit type on the host: float16, or float32 values rounded to bfloat16 (round to nearest even)."""
    x = np.asarray(x, dtype=np.float32)
    if bf16:
        from .tensor import bf16_bits_to_f32, f32_to_bf16_bits
        return bf16_bits_to_f32(f32_to_bf16_bits(x)).reshape(x.shape)
    with np.errstate(over="ignore"):
        return x.astype(np.float16)


def pad_rank(r):
    return (int(r) + 31) // 32 * 32


def operand_layout(up, down, shape, bf16=False):
    """The kernel's operands of one pair: up (N, r[, 1, 1]) and down (r, in...) as logical (file) arrays for a module whose weight has the logical
    ``shape`` -> (up (N, Rp), down_t (Kd, Rp)) in the 16-bit type.  A conv's down (r, C, R, S) is flattened in the order the device stores the
    conv's own weight, KRSC: (r, R S C)."""
    r = down.shape[0]
    rp = pad_rank(r)
    if down.ndim == 4:
        down = down.transpose(0, 2, 3, 1)                  # the NHWC rule of storage/tensor.py: (r, C, R, S) -> (r, R, S, C)
    down = np.ascontiguousarray(down).reshape(r, -1)
    n, kd = int(shape[0]), int(np.prod(shape[1:]))
    up_p = np.zeros((n, rp), np.float32)
    up_p[:, :r] = np.asarray(up, np.float32).reshape(n, r)
    dn_p = np.zeros((kd, rp), np.float32)
    dn_p[:, :r] = np.asarray(down, np.float32).T
    return _cast16(up_p, bf16), _cast16(dn_p, bf16)


def check_lora(mods, other, shapes, strict=True, bf16=False, has_text_encoder=True):
    """Check parsed adapter tensors against the targets' weight shapes ({kohya name: logical shape}) -> {kohya name: LoraWeights}.  Every failure
    is a ValueError naming the key, raised before anything is uploaded.  Keys that match no target raise (listing the first five), or with
    strict=False print ``skipped: <key>`` lines, as update_state does."""
    unmatched = list(other)
    out = {}
    for mod, m in mods.items():
        keys = m["keys"]
        if mod not in shapes:
            unmatched += list(keys.values())
            continue
        for need in ("down", "up"):
            if need not in m:
                raise ValueError(f"load_lora: {next(iter(keys.values()))}: {mod} has no lora_{need} tensor")
        up, down, shape = m["up"], m["down"], tuple(shapes[mod])
        for what in ("down", "up"):
            if m[what].dtype.kind != "f":
                raise ValueError(f"load_lora: {keys[what]}: not a float tensor ({m[what].dtype})")
        if down.ndim not in (2, 4) or up.ndim not in (2, 4):
            raise ValueError(f"load_lora: {keys['down']}: adapter tensors are 2-D (Linear) or 4-D (conv), got {down.shape} and {up.shape}")
        rank = int(down.shape[0])
        if rank < 1 or rank > MAX_RANK:
            raise ValueError(f"load_lora: {keys['down']}: rank {rank} is outside 1..{MAX_RANK}")
        if up.ndim == 4 and tuple(up.shape[2:]) != (1, 1):
            raise ValueError(f"load_lora: {keys['up']}: the lora_up of a conv must be 1x1, got {tuple(up.shape)}")
        if up.shape[0] != shape[0]:
            raise ValueError(f"load_lora: {keys['up']}: {up.shape[0]} output rows, the module has {shape[0]} (weight {shape})")
        if up.shape[1] != rank:
            raise ValueError(f"load_lora: {keys['up']}: shape {tuple(up.shape)} does not match the rank {rank} of {keys['down']}")
        side = tuple(shape[1:])
        ok = tuple(down.shape[1:]) == side or (len(side) == 3 and side[1:] == (1, 1) and tuple(down.shape[1:]) == side[:1]) \
            or (len(side) == 1 and tuple(down.shape[1:]) == side + (1, 1))
        if not ok:
            raise ValueError(f"load_lora: {keys['down']}: input side {tuple(down.shape[1:])} does not match the module's {side} (weight {shape})")
        for what in ("down", "up"):
            if not np.isfinite(m[what]).all():
                raise ValueError(f"load_lora: {keys[what]}: a value is not finite")
        alpha = float(rank)
        if "alpha" in m:
            a = np.asarray(m["alpha"], dtype=np.float64).reshape(-1)
            if a.size != 1 or not np.isfinite(a[0]):
                raise ValueError(f"load_lora: {keys['alpha']}: alpha must be one finite number, got {m['alpha']!r}")
            alpha = float(a[0])
        up16, dn16 = operand_layout(up.reshape(up.shape[0], rank), down.reshape(rank, *side), shape, bf16)
        for arr, what in ((up16, "up"), (dn16, "down")):
            if not np.isfinite(arr).all():
                raise ValueError(f"load_lora: {keys[what]}: a value is not finite after the cast to the 16-bit type")
        out[mod] = LoraWeights(up16, dn16, alpha, rank)
    if unmatched:
        if strict:
            te = [k for k in unmatched if (_split_key(k) or ("",))[0].startswith("lora_te_")]
            why = " (this model has no text encoder)" if te and not has_text_encoder else ""
            raise ValueError(f"load_lora: {len(unmatched)} key(s) match no target of this model{why}: {', '.join(unmatched[:5])}"
                             + (" ..." if len(unmatched) > 5 else "") + " -- strict=False skips them")
        for k in unmatched:
            print(f"skipped: {k}")
    return out


# ---- which adapter enters which module, and how strongly -----------------------------------------------------------------------------------------
def is_text_target(kohya_name):
    return kohya_name.startswith("lora_te_")


def plan_adapters(loaded, names, weights=1.0, text_encoder_weights=None):
    """The pure part of set_adapters.  loaded: {adapter name: {kohya module name: anything with .alpha and .rank}}; names: the adapters to
    activate, in launch order; weights: one float or one per name (the UNet side); text_encoder_weights: likewise, default = weights.
    -> ({kohya module name: [(adapter name, s_i)]}, {adapter name: (weight, text_encoder_weight)}), s_i = weight alpha / rank computed in float64
    and rounded to fp32 once; adapters whose weight on that side is 0 do not appear.  ValueError: unknown or repeated names, weights that are not
    finite or not one per name, more than 8 adapters on one module."""
    names = list(names)
    for n in names:
        if n not in loaded:
            raise ValueError(f"set_adapters: unknown adapter {n!r} (loaded: {sorted(loaded)})")
    if len(set(names)) != len(names):
        raise ValueError(f"set_adapters: an adapter is named twice: {names}")

    def per_name(w, what):
        a = np.asarray(w, dtype=np.float64)
        if a.ndim == 0:
            a = np.full((len(names),), float(a))
        if a.ndim != 1 or a.shape[0] != len(names):
            raise ValueError(f"set_adapters: {what} takes one float or one per name ({len(names)}), got shape {a.shape}")
        if not np.isfinite(a).all():
            raise ValueError(f"set_adapters: {what}={w} is not finite")
        return a
    wu = per_name(weights, "weights")
    wt = wu if text_encoder_weights is None else per_name(text_encoder_weights, "text_encoder_weights")
    plan = {}
    for n, u, t in zip(names, wu, wt):
        for mod, lw in loaded[n].items():
            w = t if is_text_target(mod) else u
            if w == 0.0:
                continue
            with np.errstate(over="ignore"):
                s = np.float32(np.float64(w) * np.float64(lw.alpha) / np.float64(lw.rank))
            if not np.isfinite(s):
                raise ValueError(f"set_adapters: the scale of {n!r} on {mod} is not finite in fp32 (weight {w}, alpha {lw.alpha}, rank {lw.rank})")
            if s == 0.0:
                continue
            plan.setdefault(mod, []).append((n, s))
    for mod, entries in plan.items():
        if len(entries) > MAX_ADAPTERS:
            raise ValueError(f"set_adapters: {len(entries)} adapters on {mod}, at most {MAX_ADAPTERS} merge in one launch")
    return plan, {n: (float(u), float(t)) for n, u, t in zip(names, wu, wt)}


class LoraRegistry:
    """Per model: the loaded adapters, and per touched module the pristine base handle and the merged handle now installed.  ``apply`` installs a
    plan through ``merge(base handle, [(adapter's per-module data, s_i)]) -> new handle``; a module no entry touches gets its base handle -- the
    same object -- back, so an empty plan restores the model bit for bit with no arithmetic."""

    def __init__(self):
        self.loaded = {}        # adapter name -> {kohya module name: per-module data (.alpha, .rank; on the device: .up, .down_t)}
        self.active = {}        # adapter name -> (weight, text_encoder_weight)
        self.base = {}          # kohya module name -> base handle
        self.merged = {}        # kohya module name -> merged handle now installed
        self.plan = {}

    def apply(self, plan, targets, merge):
        """-> (changed?, the handles taken out of the modules: keep them referenced until nothing queued or captured reads them)."""
        retired, changed = [], False
        sig = lambda entries: [(n, float(s)) for n, s in entries or ()]
        for mod in sorted(set(plan) | set(self.base)):
            module = targets[mod]
            cur = module.weight
            if mod in self.base and cur is not self.base[mod] and cur is not self.merged.get(mod):
                self.base[mod] = cur                        # someone installed a new weight (update_state) in between: it is the base now
                self.merged.pop(mod, None)
            elif mod not in self.base:
                self.base[mod] = cur
            entries = plan.get(mod)
            if entries:
                if cur is self.merged.get(mod) and sig(entries) == sig(self.plan.get(mod)):
                    continue                                # the same adapters at the same scales over the same base: nothing to do
                new = merge(self.base[mod], [(self.loaded[n][mod], s) for n, s in entries])
                if cur is not self.base[mod]:
                    retired.append(cur)
                self.merged[mod] = module.weight = new
                changed = True
            else:
                if cur is not self.base[mod]:
                    retired.append(cur)
                    module.weight = self.base[mod]
                    changed = True
                self.merged.pop(mod, None)
                del self.base[mod]
        self.plan = {m: list(e) for m, e in plan.items()}
        return changed, retired


# ---- the device side ------------------------------------------------------------------------------------------------------------------------------
DeviceLora = namedtuple("DeviceLora", ["up", "down_t", "alpha", "rank", "rp"])


def upload(weights, bf16):
    """{kohya name: LoraWeights} -> {kohya name: DeviceLora}: up / down_t as device arrays of the step's 16-bit type."""
    from .tensor import DeviceArray, bfloat16
    dt = bfloat16 if bf16 else np.float16
    return {k: DeviceLora(DeviceArray.from_numpy(w.up, dt, "row"), DeviceArray.from_numpy(w.down_t, dt, "row"), w.alpha, w.rank, w.up.shape[1])
            for k, w in weights.items()}


def merge_device(base, entries):
    """One tf_lora_merge_16 launch on the current stream: base (a Linear's (out, in) or a conv's KRSC-stored weight) and [(DeviceLora, s_i)] -> a fresh
    DeviceArray of base's shape, type and layout."""
    import ctypes
    from ..native import LoraEntry, hip
    from .tensor import DeviceArray, _sh, dtag
    n, kd = base.shape[0], base.size // base.shape[0]
    if not 1 <= len(entries) <= MAX_ADAPTERS:
        raise ValueError(f"merge_device: {len(entries)} adapters (1..{MAX_ADAPTERS})")
    table = (LoraEntry * len(entries))()
    for e, (lw, s) in zip(table, entries):
        if dtag(lw.up.dtype) != dtag(base.dtype) or base.dtype.itemsize != 2:
            raise ValueError(f"merge_device: the adapter was loaded as {lw.up.dtype}, the weight is {base.dtype} -- load it under the dtype the model runs in")
        if lw.up.shape != (n, lw.rp) or lw.down_t.shape != (kd, lw.rp):
            raise ValueError(f"merge_device: adapter operands {lw.up.shape}, {lw.down_t.shape} do not fit the weight ({n}, {kd})")
        e.up, e.down_t, e.rp, e.scale = lw.up.ptr, lw.down_t.ptr, lw.rp, float(s)
    dst = DeviceArray.empty(base.shape, base.dtype, base.layout)
    hip.tf_lora_merge_16(dtag(base.dtype), dst.ptr, base.ptr, ctypes.cast(table, ctypes.c_void_p), len(entries), n, kd, _sh())
    dst._base = (base, [lw for lw, _ in entries])           # (referenced while the launch is queued)
    return dst
