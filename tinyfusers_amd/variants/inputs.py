"""Argument checks of the StableDiffusion sampler object (variants/sd.py) that need no model state: each takes what it checks and, for
the words of its message, the method or argument it serves; each returns the checked value or raises.  The module does not import the
native library, so nothing here can launch or write -- sd.py's ``compile`` and ``start`` run these first and touch the device afterwards."""
import numpy as np

from ..storage.tensor import DeviceArray
from .samplers import Schedule, UnsupportedSamplerConfig

CONCAT_CHANNELS = {"inpaint": 5, "edit": 4}        # conditioning channels behind the 4 latent ones: [mask | masked-image latent], [image latent]


def repaint_mask(mask, who, latent_ok=False):
    """An image-resolution mask (B,H,W) -- bool, uint8 or float; >= 0.5 (uint8: nonzero) means repaint -- as a bool array.  With ``latent_ok`` a
    float (B,1,h,w) array is a latent mask already and comes back as fp32 (4-D) once its values are checked to lie in [0, 1]."""
    m = np.asarray(mask)
    if m.dtype != np.bool_ and m.dtype != np.uint8 and m.dtype.kind != "f":
        raise TypeError(f"StableDiffusion.{who}: bool, uint8 or float masks, got {m.dtype}")
    if m.dtype.kind == "f" and not (np.isfinite(m).all() and (m >= 0).all() and (m <= 1).all()):
        raise ValueError(f"StableDiffusion.{who}: float mask values must lie in [0, 1]")
    if latent_ok and m.ndim == 4:
        if m.shape[1] != 1 or m.dtype.kind != "f":
            raise ValueError(f"StableDiffusion.{who}: a latent-size mask is float (B,1,h,w), got {m.dtype} {m.shape}")
        return np.ascontiguousarray(m, dtype=np.float32)
    if m.ndim != 3 or m.shape[0] < 1 or m.shape[1] < 8 or m.shape[2] < 8 or m.shape[1] % 8 or m.shape[2] % 8:
        raise ValueError(f"StableDiffusion.{who}: takes (B,H,W) with H and W multiples of 8"
                         + (" (or a float (B,1,h,w) latent mask)" if latent_ok else "") + f", got {m.shape}")
    return (m != 0) if m.dtype == np.uint8 else (m >= 0.5)


def u8_image(image, rule, hw=None, batches=None):
    """A uint8 (B,H,W,3) image batch, host (comes back contiguous) or device, with -- where given -- the size ``hw`` and a batch in ``batches``:
    -> (image, its shape), or ValueError(``rule``, got <dtype> <shape>)."""
    if not isinstance(image, DeviceArray):
        image = np.ascontiguousarray(image)
    ish = tuple(int(v) for v in image.shape)
    if np.dtype(image.dtype) != np.uint8 or len(ish) != 4 or ish[3] != 3 or (hw is not None and ish[1:3] != tuple(hw)) \
            or (batches is not None and ish[0] not in batches):
        raise ValueError(f"{rule}, got {np.dtype(image.dtype)} {ish}")
    return image, ish


def fp32_nchw(x, shape, name):
    """start()'s array arguments that are copied as they are: a device array must be fp32 NCHW of exactly ``shape`` and comes back itself; anything
    else becomes a contiguous fp32 host array, which must have that shape."""
    if isinstance(x, DeviceArray):
        if x.shape != shape or x.dtype != np.float32 or x.layout != "row":
            raise ValueError(f"StableDiffusion.start: a device {name} must be an fp32 NCHW {shape} array, got {x}")
        return x
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.shape != shape:
        raise ValueError(f"StableDiffusion.start: {name} must have the shape {shape}, got {x.shape}")
    return x


def control_scales(control_scale, n_res):
    """start(control_scale=) -> the 16 fp32 words of the scale buffer (one per residual; 16: whole 4-word writes): all ones when not given."""
    scales = np.ones((16,), np.float32)
    if control_scale is not None:
        sc = np.asarray(control_scale, dtype=np.float32)
        if sc.ndim > 1 or (sc.ndim == 1 and sc.shape[0] != n_res):
            raise ValueError(f"StableDiffusion.start: control_scale= takes one float or {n_res} (one per residual), got shape {sc.shape}")
        if not np.isfinite(sc).all():
            raise ValueError(f"StableDiffusion.start: control_scale={control_scale}")
        scales[:n_res] = sc
    return scales


def ip_scales(ip_scale, n_attn, who="start"):
    """ip_scale= -> the fp32 words of the adapter's scale buffer (one per cross-attention in adapter order, padded to whole 4-word writes): all
    ones when not given."""
    scales = np.ones(((n_attn + 3) // 4 * 4,), np.float32)
    if ip_scale is not None:
        sc = np.asarray(ip_scale, dtype=np.float32)
        if sc.ndim > 1 or (sc.ndim == 1 and sc.shape[0] != n_attn):
            raise ValueError(f"StableDiffusion.{who}: ip_scale takes one float or {n_attn} (one per cross-attention), got shape {sc.shape}")
        if not np.isfinite(sc).all():
            raise ValueError(f"StableDiffusion.{who}: ip_scale={ip_scale}")
        scales[:n_attn] = sc
    return scales


def freeu_scales(values, who="set_freeu"):
    """(s1, s2, b1, b2) -> the 4 fp32 words of the FreeU scale buffer (one whole 4-word write): four finite floats, anything else raises."""
    try:
        sc = np.asarray(values, dtype=np.float32)
    except (TypeError, ValueError):
        sc = None
    if sc is None or sc.shape != (4,) or not np.isfinite(sc).all():
        raise ValueError(f"StableDiffusion.{who}: FreeU takes four finite floats (s1, s2, b1, b2), got {values!r}")
    return np.ascontiguousarray(sc)


PAG_WORDS = 16            # vision/unet.py::PAG_WORDS: the flag array of perturbed-attention guidance, one 64-byte write


def pag_layer_words(layers, table, who="set_pag"):
    """set_pag's ``layers`` -> the PAG_WORDS fp32 flag words (1 = this SpatialTransformer's self-attention is perturbed).  ``table``: the UNet's
    vision/unet.py::pag_layers paths in execution order.  A layer is an index into the table, an LDM path ("input_blocks.4", "middle_block",
    "output_blocks.7"; a trailing ".1" -- the transformer's place inside its block -- is accepted), one of the shorthands "down" / "mid" / "up" /
    "all", or a list of any of these (an empty list: no layer).  Everything is checked before the words are returned: an unknown name, or an index
    or a block without a transformer, raises ValueError."""
    def refuse(item):
        raise ValueError(f"StableDiffusion.{who}: pag layer {item!r} names no SpatialTransformer of this UNet (an index below {len(table)}, one of "
                         f"{', '.join(table)}, or 'down' / 'mid' / 'up' / 'all')")
    groups = {"down": "input_blocks.", "mid": "middle_block", "up": "output_blocks.", "all": ""}
    items = list(layers) if isinstance(layers, (list, tuple)) else [layers]
    words = np.zeros((PAG_WORDS,), np.float32)
    for item in items:
        if isinstance(item, (bool, np.bool_)):
            refuse(item)
        if isinstance(item, (int, np.integer)):
            if not 0 <= int(item) < len(table):
                refuse(item)
            words[int(item)] = 1.0
        elif isinstance(item, str) and item in groups:
            words[[i for i, p in enumerate(table) if p.startswith(groups[item])]] = 1.0
        elif isinstance(item, str):
            path = item if item in table or not item.endswith(".1") else item[:-2]
            if path not in table:
                refuse(item)
            words[table.index(path)] = 1.0
        else:
            refuse(item)
    return words


def pag_values(scale, adaptive, who="set_pag"):
    """(scale, adaptive scale) of perturbed-attention guidance as two finite floats >= 0, or ValueError."""
    try:
        s, a = float(scale), float(adaptive)
    except (TypeError, ValueError):
        s = a = float("nan")
    if not (np.isfinite(s) and np.isfinite(a) and s >= 0 and a >= 0):
        raise ValueError(f"StableDiffusion.{who}: the PAG scale and adaptive scale are finite floats >= 0, got {scale!r}, {adaptive!r}")
    return s, a


def pag_scale_at(scale, adaptive, timestep):
    """s_t = max(0, s - a (1000 - t)): the perturbed-attention guidance scale at a timestep, as diffusers' PAG pipelines state it."""
    return max(0.0, float(scale) - float(adaptive) * (1000.0 - float(timestep)))


def pag_guidance_words(guidance, s_t, cfg=True):
    """The two scalars the existing tails read, from the CFG scale g and s_t: (the parameter block's guidance word, the edit word or None).
    With CFG the groups are [uncond ; perturbed ; cond] and the three-group tail's e0 + g_T (e2 - e1) + g_I (e1 - e0) at g_T = g + s_t, g_I = g is
    e_u + g (e_c - e_u) + s_t (e_c - e_p); without, [perturbed ; cond] and the pair tail's e_p + (1 + s_t)(e_c - e_p) is e_c + s_t (e_c - e_p)."""
    return (float(guidance) + float(s_t), float(guidance)) if cfg else (1.0 + float(s_t), None)


def ip_embeds(x, batch, width):
    """start(ip_image_embeds=): a host float (B, E) array (or one row for every image) -> fp32 (B, E)."""
    if isinstance(x, DeviceArray):
        raise TypeError("StableDiffusion.start: ip_image_embeds= takes a host array")
    e = np.ascontiguousarray(x, dtype=np.float32)
    if e.ndim != 2 or e.shape[0] not in (1, batch) or e.shape[1] != width:
        raise ValueError(f"StableDiffusion.start: ip_image_embeds must be float {(batch, width)} (or one row for all) for the compiled latent and the attached adapter, got {e.shape}")
    if not np.isfinite(e).all():
        raise ValueError("StableDiffusion.start: ip_image_embeds holds non-finite values")
    return np.ascontiguousarray(np.broadcast_to(e, (batch, width)))


def cfg_rescale_phi(phi, who="set_cfg_rescale"):
    """CFG rescale's phi as a float in [0, 1], or ValueError."""
    try:
        v = float(phi)
    except (TypeError, ValueError):
        v = float("nan")
    if not 0.0 <= v <= 1.0:
        raise ValueError(f"StableDiffusion.{who}: the CFG rescale factor phi is a float in [0, 1], got {phi!r}")
    return v


def adm_pooled(x, batch, width, name):
    """start(pooled= / uncond_pooled=): a host float (B, P) array (or one row for every image) -> fp32 (B, P)."""
    if isinstance(x, DeviceArray):
        raise TypeError(f"StableDiffusion.start: {name}= takes a host array")
    e = np.ascontiguousarray(x, dtype=np.float32)
    if e.ndim != 2 or e.shape[0] not in (1, batch) or e.shape[1] != width:
        raise ValueError(f"StableDiffusion.start: {name} must be float {(batch, width)} (or one row for all) for the compiled latent and this UNet, got {e.shape}")
    if not np.isfinite(e).all():
        raise ValueError(f"StableDiffusion.start: {name} holds non-finite values")
    return np.ascontiguousarray(np.broadcast_to(e, (batch, width)))


def adm_ids(x, batch, name="uncond_size_ids"):
    """The six size ids [original h, w, crop top, left, target h, w] per image: a host (B, 6) array (or one row for all) -> fp32 (B, 6), finite and >= 0."""
    e = np.ascontiguousarray(x, dtype=np.float32)
    if e.ndim == 1:
        e = e[None]
    if e.ndim != 2 or e.shape[0] not in (1, batch) or e.shape[1] != 6:
        raise ValueError(f"StableDiffusion.start: {name} must be {(batch, 6)} (or one row for all): original h, w, crop top, left, target h, w; got {e.shape}")
    if not (np.isfinite(e).all() and (e >= 0).all()):
        raise ValueError(f"StableDiffusion.start: {name} holds negative or non-finite values")
    return np.ascontiguousarray(np.broadcast_to(e, (batch, 6)))


def adm_size_ids(original_size, crop_top_left, target_size, batch, height, width):
    """start(original_size=, crop_top_left=, target_size=) -> fp32 (B, 6) [original h, w, crop top, left, target h, w]: each an (h, w) pair or a
    (B, 2) array with a pair per image; None: the image size (height, width), (0, 0) and the image size."""
    cols = []
    for name, v, default in (("original_size", original_size, (height, width)), ("crop_top_left", crop_top_left, (0, 0)), ("target_size", target_size, (height, width))):
        e = np.asarray(default if v is None else v, dtype=np.float32)
        if e.ndim == 1:
            e = e[None]
        if e.ndim != 2 or e.shape[0] not in (1, batch) or e.shape[1] != 2:
            raise ValueError(f"StableDiffusion.start: {name} takes an (h, w) pair or a {(batch, 2)} array, got shape {np.shape(v)}")
        cols.append(np.broadcast_to(e, (batch, 2)))
    return adm_ids(np.concatenate(cols, axis=1), batch, "original_size / crop_top_left / target_size")


MOTION_MAX_FRAMES = 32            # tf_sdpa_temporal_16's F (vision/motion.py::MAX_FRAMES)
DUAL_HEAD_SIZES = (40, 80, 160)     # the head sizes tf_sdpa_dual_16 (an IP-Adapter's cross-attention) has instances for


def check_compile(cin, has_control_net, config, latent, sampler, inpaint, concat, control, cfg=True, ip_adapter=False, has_ip_adapter=False,
                  freeu=False, freeu_plan=(), pag=False, pag_table=(), prediction="eps", cfg_rescale=False, head_sizes=(), adm=False, motion=False,
                  has_motion=False, frames=None, motion_max_len=0):
    """compile()'s refusals, before any device work: ``cin`` the UNet's in_channels, ``config`` the package's config module, ``freeu_plan`` the
    UNet's vision/unet.py::freeu_stages rows (stage, block, backbone channels, skip channels, latent size divisor), ``pag_table`` its
    vision/unet.py::pag_layers paths, ``head_sizes`` its vision/unet.py::head_sizes (read for ip_adapter=True), ``adm`` whether the UNet is
    vector-conditioned (UNetConfig.adm_in_channels: SDXL), ``has_motion`` whether a MotionAdapter is attached and ``motion_max_len`` the frames its
    positional tables hold (read for motion=True)."""
    def refuse(exc, text):
        raise exc(f"StableDiffusion.compile: {text}")
    if motion:   # the video step runs cfg=True / False, every sampler, prediction="v", cfg_rescale=True, img2img starts, bf16, LoRA; the rest is refused by name
        if adm:
            refuse(UnsupportedSamplerConfig, "motion=True on an SDXL model is not supported (the motion modules of AnimateDiff-SDXL have another block plan)")
        if not has_motion:
            refuse(ValueError, "motion=True needs an adapter: attach_motion(MotionAdapter.load(cfg, FILE)) first")
        if sampler is None:
            refuse(ValueError, "motion=True needs a sampler schedule (sampler=<Schedule>)")
        for flag, name in ((control, "control=True (a ControlNet under the motion modules)"), (ip_adapter, "ip_adapter=True"), (concat is not None, f"concat={concat!r}"),
                           (pag, "pag=True"), (freeu, "freeu=True"), (inpaint, "inpaint=True")):
            if flag:
                refuse(UnsupportedSamplerConfig, f"motion=True and {name} together are not supported")
        if config.dtype == "fp8":
            refuse(UnsupportedSamplerConfig, "motion=True runs in the fp16 and the bf16 step, not under the fp8 policy (config.set_dtype('fp8'))")
        if config.cfg_parallel:
            refuse(UnsupportedSamplerConfig, "a model with motion modules has no two-chain CFG form (TF_CFG_PARALLEL)")
        top = min(MOTION_MAX_FRAMES, int(motion_max_len))
        if isinstance(frames, bool) or not isinstance(frames, (int, np.integer)) or not 1 <= int(frames) <= top:
            refuse(ValueError, f"motion=True needs frames=F with 1 <= F <= {top} (the adapter's positional tables hold {motion_max_len} frames, the temporal "
                               f"attention launch takes {MOTION_MAX_FRAMES}), got frames={frames!r}")
        if latent.shape[0] % int(frames):
            refuse(ValueError, f"motion=True: the latent holds videos x frames images in (video, frame) order, a batch of {latent.shape[0]} is no multiple of frames={frames}")
    elif frames is not None:
        refuse(ValueError, f"frames={frames!r} belongs to motion=True")
    if adm:      # SDXL runs cfg=True / False, every sampler, img2img, inpaint=True, prediction="v", cfg_rescale=True, bf16; the rest is refused by name
        if sampler is None:
            refuse(UnsupportedSamplerConfig, "an SDXL model needs a sampler schedule (sampler=<Schedule>): its time-embedding rows depend on start(pooled=) and are built there")
        for flag, name in ((control, "control=True (an SDXL ControlNet)"), (ip_adapter, "ip_adapter=True (an SDXL IP-Adapter)"), (concat is not None, f"concat={concat!r}"),
                           (pag, "pag=True"), (freeu, "freeu=True")):
            if flag:
                refuse(UnsupportedSamplerConfig, f"{name} on an SDXL model is not supported")
        if config.dtype == "fp8":
            refuse(UnsupportedSamplerConfig, "an SDXL model runs in the fp16 and the bf16 step, not under the fp8 policy (config.set_dtype('fp8'))")
        if config.cfg_parallel:
            refuse(UnsupportedSamplerConfig, "an SDXL model has no two-chain CFG form (TF_CFG_PARALLEL)")
    if prediction not in ("eps", "v"):
        refuse(ValueError, f"prediction= takes 'eps' or 'v', got {prediction!r}")
    if prediction == "v" or cfg_rescale:
        what = "prediction='v'" if prediction == "v" else "cfg_rescale=True"
        if sampler is None:
            refuse(ValueError, f"{what} needs a sampler schedule (sampler=<Schedule>): the reference-shaped step() keeps its eps-prediction DDIM form")
        if config.cfg_parallel:
            refuse(UnsupportedSamplerConfig, f"{what} has no two-chain CFG form (TF_CFG_PARALLEL)")
    if cfg_rescale:
        if concat == "edit":
            refuse(ValueError, "cfg_rescale=True and concat='edit' together are not supported (CFG rescale is defined against ONE text group; the InstructPix2Pix "
                               "combine has two guidance scales)")
        if not cfg and not pag:
            refuse(ValueError, "cfg_rescale=True needs a guidance pair or triple to rescale against: cfg=True, or pag=True (cfg=False alone has one group and no guidance)")
    if pag:
        if sampler is None:
            refuse(ValueError, "pag=True needs a sampler schedule (sampler=<Schedule>)")
        if concat == "edit":
            refuse(ValueError, "pag=True and concat='edit' together are not supported (InstructPix2Pix runs three guidance groups already: the perturbed one would be a fourth)")
        if config.cfg_parallel:
            refuse(UnsupportedSamplerConfig, "perturbed-attention guidance has no two-chain CFG form (TF_CFG_PARALLEL)")
        if config.dtype == "fp8":
            refuse(UnsupportedSamplerConfig, "pag=True runs in the fp16 and the bf16 step, not under the fp8 policy (config.set_dtype('fp8'))")
        if len(pag_table) > PAG_WORDS:
            refuse(ValueError, f"pag=True: this UNet has {len(pag_table)} SpatialTransformers, the flag array holds {PAG_WORDS}")
    if freeu:
        if sampler is None:
            refuse(ValueError, "freeu=True needs a sampler schedule (sampler=<Schedule>)")
        if config.cfg_parallel:
            refuse(UnsupportedSamplerConfig, "a FreeU model has no two-chain CFG form (TF_CFG_PARALLEL)")
        if config.dtype == "fp8":
            refuse(UnsupportedSamplerConfig, "freeu=True runs in the fp16 and the bf16 step, not under the fp8 policy (config.set_dtype('fp8'))")
        for stage, block, ch, cskip, div in freeu_plan:
            h, w = (int(latent.shape[2]) // div, int(latent.shape[3]) // div) if latent is not None else (2, 2)
            if ch % 16 or cskip % 8 or h < 2 or w < 2:
                refuse(ValueError, f"freeu=True: output block {block} (stage {stage + 1}) concatenates a backbone of {ch} channels and a skip of {cskip} at "
                                   f"{h} x {w} -- the FreeU kernels need backbone channels in multiples of 16, skip channels in multiples of 8 and planes of at least 2 x 2")
    if ip_adapter:
        if not has_ip_adapter:
            refuse(ValueError, "ip_adapter=True needs an adapter: attach_ip_adapter(IPAdapter.load(unet, FILE)) first")
        if sampler is None:
            refuse(ValueError, "ip_adapter=True needs a sampler schedule (sampler=<Schedule>)")
        if concat == "edit":
            refuse(ValueError, "ip_adapter=True and concat='edit' together are not supported (the adapter's unconditional convention is defined for two guidance groups, InstructPix2Pix runs three)")
        if config.cfg_parallel:
            refuse(UnsupportedSamplerConfig, "an adapted model has no two-chain CFG form (TF_CFG_PARALLEL)")
        if config.dtype == "fp8":
            refuse(UnsupportedSamplerConfig, "ip_adapter=True runs in the fp16 and the bf16 step, not under the fp8 policy (config.set_dtype('fp8'))")
        bad = [hs for hs in head_sizes if hs not in DUAL_HEAD_SIZES]
        if bad:
            refuse(UnsupportedSamplerConfig, f"ip_adapter=True: this UNet's cross-attentions have head size {bad[0]}, the dual launch (tf_sdpa_dual_16) has "
                                             f"instances for {', '.join(str(v) for v in DUAL_HEAD_SIZES)} (SD-1.x); an IP-Adapter on SD-2.x is not supported")
    if not cfg:
        if sampler is None:
            refuse(ValueError, "cfg=False needs a sampler schedule (sampler=<Schedule>): the reference-shaped step() keeps its CFG form")
        if concat == "edit":
            refuse(ValueError, "cfg=False and concat='edit' together are not supported (the InstructPix2Pix update is defined by its three guidance branches)")
        if config.cfg_parallel:
            refuse(UnsupportedSamplerConfig, "cfg=False has one guidance branch, so no two-chain CFG form (TF_CFG_PARALLEL)")
        if config.dtype == "fp8":
            refuse(UnsupportedSamplerConfig, "cfg=False runs in the fp16 and the bf16 step, not under the fp8 policy (config.set_dtype('fp8'))")
    if concat not in (None, "inpaint", "edit"):
        refuse(ValueError, f"concat= takes None, 'inpaint' or 'edit', got {concat!r}")
    if control:
        if not has_control_net:
            refuse(ValueError, "control=True needs a ControlNet: attach_control(ControlNet(cfg)) first")
        if sampler is None:
            refuse(ValueError, "control=True needs a sampler schedule (sampler=<Schedule>)")
        if concat is not None:
            refuse(ValueError, f"control=True and concat={concat!r} together (a ControlNet on a concat-conditioned model) are not supported")
        if config.cfg_parallel:
            refuse(UnsupportedSamplerConfig, "a controlled model has no two-chain CFG form (TF_CFG_PARALLEL)")
        if config.dtype == "fp8":
            refuse(UnsupportedSamplerConfig, "control=True runs in the fp16 and the bf16 step, not under the fp8 policy (config.set_dtype('fp8'))")
    if concat is None and cin != 4:
        refuse(ValueError, f"a UNet with in_channels={cin} is concat-conditioned: pass concat='inpaint' (9 channels) or concat='edit' (8)")
    if concat is not None:
        if sampler is None:
            refuse(ValueError, f"concat={concat!r} needs a sampler schedule (sampler=<Schedule>)")
        if cin != 4 + CONCAT_CHANNELS[concat]:
            refuse(ValueError, f"concat={concat!r} needs a UNet with in_channels={4 + CONCAT_CHANNELS[concat]}, this one has {cin}")
        if inpaint:
            refuse(ValueError, "concat= and inpaint=True together (the latent blend on top of a concat-conditioned model) are not supported")
        if config.cfg_parallel:
            refuse(UnsupportedSamplerConfig, "a concat-conditioned model has no two-chain CFG form (TF_CFG_PARALLEL)")
        if latent.shape[1] != 4:
            refuse(ValueError, f"the latent of a concat-conditioned model has 4 channels, got {latent.shape}")
    if config.is_bf16() and (config.parallel_branches or config.cfg_parallel):
        refuse(RuntimeError, "the bfloat16 step has no parallel-branch / two-chain CFG form (TF_PARALLEL_BRANCHES / TF_CFG_PARALLEL are fp16-only experiments)")
    if inpaint and sampler is None:
        refuse(ValueError, "inpaint=True needs a sampler schedule (sampler=<Schedule>)")
    if sampler is not None:
        if not isinstance(sampler, Schedule):
            refuse(TypeError, "sampler= takes a Schedule (e.g. DPMSolverPP2M().schedule(20))")
        if config.cfg_parallel:
            refuse(UnsupportedSamplerConfig, "a sampler schedule has no two-chain CFG form (TF_CFG_PARALLEL is an fp16-only experiment)")
