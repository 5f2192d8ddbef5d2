"""StableDiffusion sampler object -- mirrors tinyfusers/variants/sd.py:7-65.

Same call surface: ``sd(unconditional_context, context, latent, timestep, alphas, alphas_prev, guidance)``
returns x_{t-1}.  Differences, all MI355X-first:
  * no host round trip / device syncs per step (variants/sd.py:34-41); CFG duplicate, CFG combine and the DDIM
    update are two tiny kernels; the latent state stays fp32 NCHW on the device;
  * batch generalised from the reference's hard-coded 1 (D8) to [uncond x B ; cond x B];
  * ``compile()`` captures the whole step (one launch per fused op) into one HIP graph replayed per step.
Beyond the UNet denoising path the next rows are built too: first_stage_model (VAE decode side, 8(f1))
and cond_stage_model.transformer.text_model (CLIP text encoder, 8(f2)), under the reference's attribute names so that
update_state walks the same LDM checkpoint keys.  The encoder side of first_stage_model feeds image-to-image and inpainting
(``encode_image``, ``start(init_image= / init_latent=, mask=)``, ``compile(..., inpaint=True)``) and the conditioning of the
concat-conditioned checkpoints: the SD-1.5 inpainting UNet (SD15_INPAINT, 9 input channels) and InstructPix2Pix (SD15_EDIT, 8 input channels)
run through ``compile(..., concat="inpaint" | "edit")`` and ``start(cond_image= / cond_mask= / cond_latent=, image_guidance=)``.
A ControlNet (vision/controlnet.py; ``attach_control``, ``compile(..., control=True)``, ``start(control_image= / control_hint=, control_scale=)``)
runs inside the same captured step: its residuals enter the UNet's skip connections through one launch (tf_control_add_16).
LoRA adapters (storage/lora.py; ``load_lora``, ``set_adapters``, ``adapters``, ``unload_lora``) are merged on the device into fresh weight buffers
(tf_lora_merge_16, one launch per touched module, from the kept base weight); a compiled model re-captures its step.
``compile(..., cfg=False)`` is the guidance-free step of few-step samplers (samplers.LCM with an LCM-LoRA): ONE guidance group -- the UNet runs
on B images against the context alone, between tf_latent_stack1_* and tf_sampler_step1_* (csrc/sampler.hip).
``compile(..., freeu=True)`` is FreeU inside the captured step (csrc/freeu.hip; ``set_freeu``, ``start(freeu=)``): Fourier-filtered skips and a
scaled backbone in front of the concats of the first two decoder stages, four device scalars that change without a re-capture.
``compile(..., pag=True)`` is perturbed-attention guidance inside the captured step (csrc/sdpa_pag.hip; ``set_pag``, ``start(pag=)``): one more
guidance group whose self-attentions are the identity in the selected transformers, combined by the tails that exist.
``StableDiffusion(SDXL)`` is the SDXL base model: a UNet with vector conditioning (``start(pooled=, original_size=, crop_top_left=, target_size=)``
-- everything that depends on it is computed in ``start``, the captured step gains no launch), two text towers under ``conditioner.embedders``
(``encode_prompt``), the SD-1.5 VAE tree at ``latent_scale`` 0.13025.
``compile(..., motion=True, frames=F)`` is the AnimateDiff video step (vision/motion.py; ``attach_motion``, ``set_motion_scale``, ``start(motion_scale=)``): the
latent holds V videos of F frames, every motion module runs inside the one graph, the strength of their residual branch changes without a re-capture.

How the object is laid out.  Everything ``compile`` / ``start`` / ``set_context`` / ``set_adapters`` keep on the model is declared, with its
"not compiled" value, in ``_reset_state``: ``__init__`` runs all of it, ``compile`` the per-compile part, so a re-compile with other flags drops the
buffers of the modes it no longer uses and nothing probes for a name.  ``compile`` is refuse -> reset / remember -> allocate the mode buffers ->
hoist -> warm up -> capture; ``start`` checks all three argument groups (control, conditioning, latent) and only then writes; ``step`` and
``step_sampler`` share ``_advance``.  The argument checks that need no model state live in variants/inputs.py, which cannot reach the device.
"""
import ctypes
from collections import namedtuple

import numpy as np

from .. import config
from ..native import hip
from ..storage.tensor import Branch, DeviceArray, Stream, _sh, asarray, bfloat16, dtag, pool, use_stream
from ..vision.unet import SD15, SD15_EDIT, SD15_INPAINT, SD21, SD21_INPAINT, SDXL, StepParams, UNetModel, freeu_stages, head_sizes, pag_layers
from . import inputs
from .samplers import UnsupportedSamplerConfig, get_alphas_cumprod  # noqa: F401  (get_alphas_cumprod: variants/sd.py:61-65, re-exported)


def _seed_words(seed):
    """A seed (any int; taken mod 2^64) -> the two 32-bit key words of the device generator."""
    seed = int(seed) % (1 << 64)
    return seed & 0xFFFFFFFF, seed >> 32


def _scalar(v):
    return float(np.asarray(v.numpy() if isinstance(v, DeviceArray) else v, dtype=np.float32).reshape(-1)[0])


def _step_dtype():
    """The 16-bit type of the step's activations (config.is_bf16())."""
    return bfloat16 if config.is_bf16() else np.float16


def _entry16(stem, other):
    """The library entry ``<stem>_bf16`` in the bfloat16 step, else ``<stem>_<other>`` (its float16 twin: "f16", or "f32" where the entry is
    named after the fp32 latent it updates)."""
    return getattr(hip, f"{stem}_{'bf16' if config.is_bf16() else other}")


class StableDiffusion:
    def __init__(self, cfg=SD15, init=False):
        self.alphas_cumprod = get_alphas_cumprod()
        self.model = namedtuple("DiffusionModel", ["diffusion_model"])(diffusion_model=UNetModel(cfg, init=init))
        from ..vae.vae import AutoencoderKL
        sd15 = any(cfg is c for c in (SD15, SD15_INPAINT, SD15_EDIT))        # the three SD-1.5 checkpoints share the VAE and the text encoder
        sd21 = any(cfg is c for c in (SD21, SD21_INPAINT))                   # SD-2.x: the same VAE (architecture and 0.18215), the OpenCLIP ViT-H text tower
        sdxl = cfg is SDXL                                                   # SDXL base: the same VAE architecture at another latent scale, two text towers
        self.latent_scale = 0.13025 if sdxl else 0.18215                     # decode divides by it, encode_image and the inpainting conditioning multiply
        self.first_stage_model = AutoencoderKL(init=init, init_encoder=False) if sd15 or sd21 or sdxl else None   # text-to-image uses the decode side only: the encoder stays an empty tree until update_state fills it (encode_image needs it)
        self.cond_stage_model = None
        if sd15:                         # variants/sd.py:12: cond_stage_model.transformer.text_model
            from ..vae.encoder import CLIPTextTransformer
            self.cond_stage_model = namedtuple("CondStageModel", ["transformer"])(
                transformer=namedtuple("Transformer", ["text_model"])(text_model=CLIPTextTransformer(init=init)))
        if sd21:                         # an LDM v2 checkpoint's cond_stage_model.model.* (vae/open_clip_text.py); built empty: update_state fills it
            from ..vae.open_clip_text import OpenClipText
            self.cond_stage_model = OpenClipText()
        self.conditioner = None
        if sdxl:                         # an SGM checkpoint's conditioner.embedders.0.transformer.text_model.* (CLIP-L, tapped behind layer 11 of 12) and
            from ..vae.encoder import CLIPTextTransformer          # conditioner.embedders.1.model.* (OpenCLIP bigG: penultimate output, pooled vector)
            from ..vae.open_clip_text import BIG_G_TEXT, OpenClipText
            clip_l = namedtuple("Embedder0", ["transformer"])(transformer=namedtuple("Transformer", ["text_model"])(text_model=CLIPTextTransformer(init=init, tap=11)))
            self.conditioner = namedtuple("Conditioner", ["embedders"])(embedders=[clip_l, OpenClipText(BIG_G_TEXT, tap="penultimate_raw", pooled=True)])
        self.control_model = None        # a ControlNet (vision/controlnet.py), under the LDM checkpoint's name: attach_control sets it
        self._ip_model = None            # an IPAdapter (storage/ip_adapter.py): attach_ip_adapter sets it (private: no checkpoint of the model names it)
        self._clip_vision = None         # a ClipVision (vae/clip_vision.py): attach_clip_vision sets it; start(ip_image=) runs it
        self._motion_model = None        # a MotionAdapter (vision/motion.py): attach_motion sets it (private: no checkpoint of the model names it)
        self._reset_state(everything=True)

    def _reset_state(self, everything=False):
        """Every attribute compile / start / set_context / set_adapters keep on the model, at its "not compiled" value.  ``compile`` runs the
        per-compile part, which lets go of the previous compile's buffers; the graph, its blocks and ``_keep`` are not touched there -- ``_capture``
        releases them in the order set_adapters relies on -- nor are the parameter block (a DDIM re-compile keeps its own) and the adapters."""
        if everything:
            self._params = None                  # StepParams: the 4 step scalars; a sampler's block adds row, seed, image offset
            self._graph = self._graph_blocks = self._keep = None     # the captured step, the pool blocks it owns, what its nodes reference
            self._lora = None                    # storage/lora.py::LoraRegistry, made by the first load_lora
        self._compile_args = None                # compile's arguments (set_adapters captures the step again)
        self._needs_start = False                # set_adapters re-captured: the previous start's state did not survive
        self._stream = None                      # the sampler stream; None: never compiled
        self._latent = self._unc = self._ctx = self._ctx2 = None     # the caller's latent and contexts; the private stacked context
        self._sched, self._inpaint, self._concat, self._control, self._groups = None, False, None, False, 2      # the mode
        self._cfg = True                         # cfg=False: no unconditional group (one group; with pag=True [perturbed ; cond])
        self._pag, self._pag_flags, self._pag_scale, self._pag_edit_g = False, None, (3.0, 0.0), None     # pag=True: the 16 layer words; (scale, adaptive scale); the g the edit word holds
        self._coeffs = self._x0_hist = None      # sampler: coefficient table, fp32 x0 history
        self._x0_init = self._mask = None        # inpaint=True: the clean latent and the (B,1,h,w) mask
        self._cond = self._edit = None           # concat=: the conditioning channels; [0] g_I of the three-branch update
        self._hint_emb = self._control_scales = None                 # control=True
        self._freeu, self._freeu_scales = False, None                # freeu=True: the device fp32 words [s1, s2, b1, b2]
        self._vpred, self._rescale, self._rescale_phi = False, False, None     # prediction="v"; cfg_rescale=True: the device fp32 word phi (in a 4-word block)
        self._ip, self._ip_model_compiled, self._ip_kv, self._ip_scales, self._ip_keep = False, None, None, None, None     # the adapter the step captured, ip_adapter=True: image-token K|V (G B, T, kv_n), the scales
        self._motion, self._motion_compiled, self._frames, self._ctx_vid = False, None, None, None     # motion=True: the adapter the step captured, F, the per-video stacked context
        self._seed, self._image_offset, self._cursor = (0, 0), 0, 0  # what start() sets, step_sampler advances
        # a UNet with label_emb (SDXL): y (G B, adm) and label_emb(y) (G B, E), private buffers start(pooled=) fills; the schedule's table of
        # time-embedding rows (S G B, N) built there, and the serial that keys it (a new start invalidates the rows of the previous one)
        self._adm, self._adm_y, self._y_emb, self._adm_table, self._adm_serial, self._adm_keep = False, None, None, None, 0, None
        self._kv_all = self._kv_key = self._ckv_all = self._emb_cur = self._emb_key = self._keep_row = None     # hoisted K|V and time-embedding row
        self._emb_rows = {}
        self._ctx_tmp = self._kv_tmp = self._start_keep = self._cond_keep = self._control_keep = self._ip_tower_keep = None   # referenced until their kernels have run

    def attach_control(self, net):
        """Give the model a ControlNet (vision/controlnet.py) built for the UNet's configuration: ``compile(..., control=True)`` then captures
        the controlled step.  update_state(sd, W) fills it from the checkpoint's ``control_model.*`` tensors."""
        from dataclasses import replace
        from ..vision.controlnet import ControlNet
        if not isinstance(net, ControlNet):
            raise TypeError(f"StableDiffusion.attach_control: takes a ControlNet, got {type(net).__name__}")
        if replace(net.cfg, in_channels=4) != replace(self.model.diffusion_model.cfg, in_channels=4):
            raise ValueError(f"StableDiffusion.attach_control: the ControlNet was built for {net.cfg}, the UNet is {self.model.diffusion_model.cfg}")
        self.control_model = net
        return self

    def attach_ip_adapter(self, adapter):
        """Give the model an IPAdapter (storage/ip_adapter.py) built for its UNet: ``compile(..., ip_adapter=True)`` then captures the step whose
        cross-attentions are the dual launches.  The adapter acts on the UNet only; a ControlNet's cross-attentions stay plain."""
        from ..storage.ip_adapter import IPAdapter, adapter_paths
        if not isinstance(adapter, IPAdapter):
            raise TypeError(f"StableDiffusion.attach_ip_adapter: takes an IPAdapter, got {type(adapter).__name__}")
        table = adapter_paths(self.model.diffusion_model)
        if adapter.paths != [(n, p) for n, p, _ in table] or adapter.context_dim != self.model.diffusion_model.cfg.context_dim \
                or [p.to_k_ip.out_features for p in adapter.ip_adapter.values()] != [st.proj_in._shape[0] for _, _, st in table]:
            raise ValueError("StableDiffusion.attach_ip_adapter: the adapter was built for another UNet configuration")
        if self._clip_vision is not None:
            self._check_tower_fits(self._clip_vision, adapter, "attach_ip_adapter")
        self._ip_model = adapter
        return self

    @staticmethod
    def _check_tower_fits(tower, adapter, who):
        if tower.cfg.projection != adapter.embed_dim:
            raise ValueError(f"StableDiffusion.{who}: the CLIP vision tower projects to {tower.cfg.projection} values, the IP-Adapter's image "
                             f"projection reads {adapter.embed_dim}")

    def attach_clip_vision(self, tower):
        """Give the model a CLIP image tower (vae/clip_vision.py::ClipVision): ``start(ip_image=)`` then turns a picture into the image embeddings
        on the device.  Its projection width must be the attached adapter's embedding width (checked here and in attach_ip_adapter, whichever
        comes second).  Nothing is captured again: the tower runs in start(), outside the step's graph."""
        from ..vae.clip_vision import ClipVision
        if not isinstance(tower, ClipVision):
            raise TypeError(f"StableDiffusion.attach_clip_vision: takes a ClipVision, got {type(tower).__name__}")
        if self._ip_model is not None:
            self._check_tower_fits(tower, self._ip_model, "attach_clip_vision")
        self._clip_vision = tower
        return self

    def attach_motion(self, adapter):
        """Give the model AnimateDiff motion modules (vision/motion.py::MotionAdapter) built for its UNet's configuration: ``compile(..., motion=True,
        frames=F)`` then captures the video step.  The adapter never touches the UNet's weights; a step compiled with motion=False does not see it."""
        from ..vision.motion import MotionAdapter
        if not isinstance(adapter, MotionAdapter):
            raise TypeError(f"StableDiffusion.attach_motion: takes a MotionAdapter, got {type(adapter).__name__}")
        if adapter.cfg != self.model.diffusion_model.cfg:
            raise ValueError(f"StableDiffusion.attach_motion: the adapter was built for {adapter.cfg}, the UNet is {self.model.diffusion_model.cfg}")
        self._motion_model = adapter
        return self

    def detach_motion(self):
        """Forget the motion modules.  A step compiled with motion=True keeps running on the modules it captured until the next compile."""
        self._motion_model = None
        return self

    def detach_ip_adapter(self):
        """Forget the adapter.  A step compiled with ip_adapter=True keeps running on the weights it captured until the next compile."""
        self._ip_model = None
        return self

    # -- reference surface -------------------------------------------------------------------------
    def get_model_output(self, unconditional_context, context, latent, timestep, unconditional_guidance_scale, params=None):
        """variants/sd.py:27-46.  Returns the raw UNet output for [uncond x B ; cond x B] (2B,4,H,W) -- the CFG
        combine is fused with the DDIM update in __call__ (use cfg_combine() to get e_t on its own)."""
        b, c, h, w = latent.shape
        x2 = self._cfg_duplicate(latent)
        ctx = self._stack_context(unconditional_context, context)
        sp = params if params is not None else self._step_params().set(_scalar(timestep), 1.0, 1.0, _scalar(unconditional_guidance_scale))
        return self.model.diffusion_model(x2, sp, ctx)

    def get_x_prev_and_pred_x0(self, x, e_t, a_t, a_prev):
        """variants/sd.py:14-25 on host arrays (kept for API parity / tests; the device path is tf_cfg_ddim_step_f32)."""
        x, e_t = np.asarray(x, dtype=np.float32), np.asarray(e_t, dtype=np.float32)
        a_t, a_prev = np.float32(_scalar(a_t)), np.float32(_scalar(a_prev))
        sqrt_one_minus_at = np.sqrt(1 - a_t)
        pred_x0 = (x - sqrt_one_minus_at * e_t) / np.sqrt(a_t)
        dir_xt = np.sqrt(1.0 - a_prev) * e_t
        return np.sqrt(a_prev) * pred_x0 + dir_xt, pred_x0

    def __call__(self, unconditional_context, context, latent, timestep, alphas, alphas_prev, guidance):
        """variants/sd.py:56-59: one denoising step; latent (B,4,H,W) fp32 device array -> new latent."""
        sp = self._step_params().set(_scalar(timestep), _scalar(alphas), _scalar(alphas_prev), _scalar(guidance))
        out = self.get_model_output(unconditional_context, context, latent, timestep, guidance, params=sp)
        b, c, h, w = latent.shape
        x_prev = DeviceArray.empty(latent.shape, np.float32, "row")
        hip.tf_memcpy_async(x_prev.ptr, latent.ptr, latent.nbytes, 3, _sh())
        _entry16("tf_cfg_ddim_step", "f32")(x_prev.ptr, out.ptr, sp.dev.ptr, b, c, h, w, _sh())
        return x_prev

    def decode(self, x):
        """variants/sd.py:48-54: post_quant_conv(x / 0.18215) -> Decoder -> (x+1)/2 -> clip -> uint8 (H, W, 3).
        x: fp32 NCHW latent (1,4,h,w) on the device.  Returns a host uint8 array."""
        b, c, h, w = x.shape
        assert b == 1, "decode: batch 1 (the reference reshapes to (3,512,512), variants/sd.py:52)"
        z16 = DeviceArray.empty((b, c, h, w), np.float16, "row")
        hip.tf_scale_cast_f32_to_f16(z16.ptr, x.ptr, 1.0 / self.latent_scale, x.size, _sh())
        z = DeviceArray.empty((b, c, h, w), np.float16, "nhwc")
        hip.tf_nchw_to_nhwc_f16(z.ptr, z16.ptr, b, c, h, w, _sh())
        y = self.first_stage_model.decoder(self.first_stage_model.post_quant_conv(z))      # (1,3,8h,8w) NHWC
        n = y.size
        out = DeviceArray.empty((n,), np.uint8, "row")
        hip.tf_image_to_u8(out.ptr, y.ptr, n, _sh())
        hip.tf_stream_sync(_sh())
        host = np.empty((y.shape[2], y.shape[3], y.shape[1]), dtype=np.uint8)
        hip.tf_memcpy(host.ctypes.data, out.ptr, n, 2)
        return host

    @staticmethod
    def encoder_size_error(h, w):
        """Why the VAE encoder cannot take an (h, w) image, or None: three stride-2 levels need multiples of 8, and the reference-exact
        AttnBlock at the latent resolution (config.head_merge) runs the fused SDPA kernel with head size w / 8 (a multiple of 8 in [8, 160])."""
        if h < 8 or w < 8 or h % 8 or w % 8:
            return f"the image size {h}x{w} must be a positive multiple of 8 in both dimensions"
        if config.head_merge == "reference_exact" and (w % 64 or w > 1280):
            return f"the width {w} must be a multiple of 64 up to 1280 (the encoder's reference-exact AttnBlock runs a head size of width / 8)"
        return None

    def encode_prompt(self, ids_l, ids_g):
        """SDXL: (B, T) token ids of the two tokenizers (host arrays) -> (context (B, T, 2048), pooled (B, 1280)) on the device: CLIP-L's layer-11 output
        and OpenCLIP bigG's penultimate output, neither through its final LayerNorm, side by side; the pooled vector from bigG's last layer."""
        if self.conditioner is None:
            raise RuntimeError("StableDiffusion.encode_prompt: this model has no conditioner (the SDXL configuration only)")
        if tuple(np.shape(ids_l)) != tuple(np.shape(ids_g)) or np.ndim(ids_l) != 2:
            raise ValueError(f"StableDiffusion.encode_prompt: both towers take (B, T) token ids of one shape, got {np.shape(ids_l)} and {np.shape(ids_g)}")
        a = self.conditioner.embedders[0].transformer.text_model(ids_l)
        g, pooled = self.conditioner.embedders[1](ids_g)
        (b, t, wa), wg = a.shape, g.shape[2]
        ctx = DeviceArray.empty((b, t, wa + wg), a.dtype, "row")
        hip.tf_memcpy_2d_async(ctx.ptr, (wa + wg) * 2, a.ptr, wa * 2, wa * 2, b * t, _sh())
        hip.tf_memcpy_2d_async(ctx.ptr + wa * 2, (wa + wg) * 2, g.ptr, wg * 2, wg * 2, b * t, _sh())
        ctx._base = (a, g)                                               # (referenced until the copies have run)
        return ctx, pooled

    def encode_image(self, images):
        """vae/vae.py:12-15 for image-to-image: uint8 (B,H,W,3) images (host or device) -> x0 = 0.18215 x means, a device fp32 NCHW latent
        (B,4,H/8,W/8) -- the inverse of decode's 1/0.18215 (variants/sd.py:49).  uint8 -> x/127.5 - 1 (tf_image_from_u8_f16) -> Encoder +
        quant_conv, means only (AutoencoderKL.encode) -> tf_means_to_latent_f32.  Asynchronous, on the current stream."""
        fsm = self._encoder_side("encode_image")
        images, (b, h, w, _) = inputs.u8_image(images, "StableDiffusion.encode_image: takes uint8 (B,H,W,3) images")
        why = self.encoder_size_error(h, w)
        if b < 1 or why:
            raise ValueError(f"StableDiffusion.encode_image: {why or 'an empty batch'}")
        means, keep = self._encode_u8(fsm, images)                       # (B,4,H/8,W/8) fp16 NHWC
        x0 = DeviceArray.empty(means.shape, np.float32, "row")
        if self.latent_scale == 0.18215:
            hip.tf_means_to_latent_f32(x0.ptr, means.ptr, b, means.shape[2], means.shape[3], _sh())
        else:                            # the same kernel and product at the model's scale (SDXL: 0.13025)
            hip.tf_means_to_cond_f32(x0.ptr, means.ptr, b, means.shape[2], means.shape[3], self.latent_scale, 0, 4, _sh())
        x0._base = keep                                                  # (referenced until the kernels have run)
        return x0

    @staticmethod
    def _encode_u8(fsm, image, m8=None):
        """A checked uint8 (B,H,W,3) image, host or device -> x / 127.5 - 1 in fp16 NHWC (tf_image_from_u8_f16; with ``m8``, a host uint8 (B,H,W)
        mask, tf_image_from_u8_masked_f16 sets the pixels where it is 1 to 0) -> the means of ``fsm.encode``, on the current stream.  Returns
        (means, what must stay referenced until the kernels have run)."""
        dev = image if isinstance(image, DeviceArray) else DeviceArray.from_numpy(image, np.uint8, "row")
        b, h, w, _ = dev.shape
        x = DeviceArray.empty((b, 3, h, w), np.float16, "nhwc")          # NHWC: the (B,H,W,3) element order of the uint8 image
        if m8 is None:
            dm8 = None
            hip.tf_image_from_u8_f16(x.ptr, dev.ptr, x.size, _sh())
        else:
            dm8 = DeviceArray.from_numpy(m8, np.uint8, "row")
            hip.tf_image_from_u8_masked_f16(x.ptr, dev.ptr, dm8.ptr, b, h, w, _sh())
        means = fsm.encode(x)
        return means, (dev, x, dm8, means)

    def _encoder_side(self, who):
        """first_stage_model with a filled encoder, or the RuntimeError ``who`` raises."""
        fsm = self.first_stage_model
        if fsm is None:
            raise RuntimeError(f"StableDiffusion.{who}: this model has no first_stage_model (SD-1.5, SD-2.x and SDXL configurations only)")
        enc = fsm.encoder
        if any(m.weight is None for m in (enc.conv_in, enc.conv_out, fsm.quant_conv)):
            raise RuntimeError(f"StableDiffusion.{who}: the VAE encoder has no weights -- it is built empty; fill it with update_state "
                               "from an LDM checkpoint (or synth_state_dict(param_shapes(model)))")
        return fsm

    @staticmethod
    def latent_mask(mask):
        """Host helper: an inpainting mask at image resolution (B,H,W) -- bool, uint8 or float, >= 0.5 (uint8: nonzero) means repaint -- to the
        latent mask (B,1,H/8,W/8) fp32 the masked step reads, by the maximum over each 8x8 block (a latent pixel is repainted when any of its
        image pixels is).  A float (B,1,h,w) array is a latent mask already: it passes through once its values are checked to lie in [0, 1]."""
        rep = inputs.repaint_mask(mask, "latent_mask", latent_ok=True)
        if rep.ndim == 4:
            return rep
        b, h, w = rep.shape
        return rep.reshape(b, 1, h // 8, 8, w // 8, 8).any(axis=(3, 5)).astype(np.float32)

    @staticmethod
    def concat_mask_u8(mask):
        """Host helper: an inpainting mask at image resolution (B,H,W) -- bool, uint8 or float, latent_mask's repaint convention (>= 0.5, uint8:
        nonzero) -- binarised to uint8 (B,H,W), 1 = repaint: what tf_image_from_u8_masked_f16 reads to blank the masked image."""
        return np.ascontiguousarray(inputs.repaint_mask(mask, "concat_mask"), dtype=np.uint8)

    @staticmethod
    def concat_mask(mask):
        """Host helper: the mask channel of the SD-1.5 inpainting UNet, (B,1,H/8,W/8) fp32, from an image-resolution mask (B,H,W) (bool, uint8
        or float; latent_mask's repaint convention).  The mask is binarised at image resolution, then latent pixel [i, j] takes image pixel
        [8i, 8j]: the nearest-neighbour resize the inpainting weights were trained and are sampled with.  Deliberately NOT latent_mask's
        maximum over each 8x8 block -- that rule serves the latent blend, where a latent pixel is repainted when any of its image pixels is;
        here the channel is an input of the network and has to look like what it saw in training."""
        return StableDiffusion.concat_mask_u8(mask)[:, None, ::8, ::8].astype(np.float32)

    # -- helpers ---------------------------------------------------------------------------------
    def _step_params(self):
        if self._params is None:
            self._params = StepParams()
        return self._params

    @staticmethod
    def _cfg_duplicate(latent):
        """variants/sd.py:31: the latent for both halves of the CFG pair, in the step's 16-bit type (NHWC)."""
        b, c, h, w = latent.shape
        x2 = DeviceArray.empty((2 * b, c, h, w), _step_dtype(), "nhwc")
        _entry16("tf_cfg_duplicate", "f16")(x2.ptr, latent.ptr, b, c, h, w, _sh())
        return x2

    def _latent_stack1(self):
        """variants/sd.py:31 for the guidance-free step (cfg=False): the latent once -- with the conditioning channels of concat="inpaint" behind
        it -- NHWC in the step's 16-bit type."""
        b, c, h, w = self._latent.shape
        cc = self._cond.shape[1] if self._cond is not None else 0
        x = DeviceArray.empty((b, c + cc, h, w), _step_dtype(), "nhwc")
        _entry16("tf_latent_stack1", "f16")(x.ptr, self._latent.ptr, self._cond.ptr if cc else None, b, c, cc, h, w, _sh())
        return x

    def _latent_stack3(self):
        """variants/sd.py:31 for the three guidance groups of pag=True on a 4-channel UNet: the latent three times, NHWC in the step's 16-bit type."""
        b, c, h, w = self._latent.shape
        x = DeviceArray.empty((3 * b, c, h, w), _step_dtype(), "nhwc")
        _entry16("tf_latent_stack3", "f16")(x.ptr, self._latent.ptr, b, c, h, w, _sh())
        return x

    def _cond_groups(self):
        """How many of the last guidance groups read the conditional inputs: the conditional group, and in front of it pag=True's perturbed one."""
        return 2 if self._pag else 1

    def _cfg_concat(self):
        """variants/sd.py:31 for a concat-conditioned UNet: [latent | cond] for every guidance group, NHWC in the step's 16-bit type; an edit
        model's first group (bit 0 of drop_bits) reads zeros in place of the conditioning."""
        b, c, h, w = self._latent.shape
        cc = self._cond.shape[1]
        x = DeviceArray.empty((self._groups * b, c + cc, h, w), _step_dtype(), "nhwc")
        _entry16("tf_cfg_concat", "f16")(x.ptr, self._latent.ptr, self._cond.ptr, b, c, cc, h, w, self._groups, 0b001 if self._concat == "edit" else 0, _sh())
        return x

    @staticmethod
    def _stack_context(unconditional_context, context, groups=2, cond_groups=1):
        """[unc ; ctx], or for the three guidance branches of an edit model [unc ; unc ; ctx]; one group (cfg=False): ctx alone, unc is not read.
        cond_groups = 2 (pag=True): the last TWO groups read ctx -- [unc ; ctx ; ctx], or [ctx ; ctx] without CFG: the perturbed group runs on the
        conditional inputs."""
        b, t, d = context.shape
        ctx = DeviceArray.empty((groups * b, t, d), context.dtype, "row")
        for g in range(groups):
            src = context if g >= groups - cond_groups else unconditional_context
            hip.tf_memcpy_async(ctx.ptr + g * context.nbytes, src.ptr, context.nbytes, 3, _sh())
        if config.is_bf16():
            from ..ff.linear import to_bf16
            ctx = to_bf16(ctx)                                 # (the bfloat16 step takes fp16 or bfloat16 contexts)
        return ctx

    @staticmethod
    def latent_from_numpy(x):
        """(B,4,H,W) host array -> fp32 NCHW device latent (the sampler state)."""
        return DeviceArray.from_numpy(np.ascontiguousarray(x, dtype=np.float32), np.float32, "row")

    def set_latent(self, x):
        """Start a new image: host noise (B,4,H,W) -> the latent buffer the compiled step updates in place.  Ordered after
        every step already queued (the sampler stream is drained first)."""
        self._require_compiled("set_latent")
        self.synchronize()
        self._latent.copy_from_numpy(x)
        self._needs_start = False
        return self._latent

    @staticmethod
    def randn_latent(shape, seed, image_offset=0):
        """A device fp32 NCHW latent (B,C,H,W) of N(0,1) noise drawn on the device (tf_randn_f32, tag 0): image b is global image
        image_offset + b of ``seed``, whatever the batch it is drawn in (a rank of dist.shard_range reproduces a single-GPU run's images)."""
        b = int(shape[0])
        out = DeviceArray.empty(tuple(shape), np.float32, "row")
        lo, hi = _seed_words(seed)
        hip.tf_randn_f32(out.ptr, b, out.size // b if b else 0, lo, hi, int(image_offset), 0, 0, _sh())
        return out

    # -- whole-step HIP graph ------------------------------------------------------------------------
    def compile(self, unconditional_context, context, latent, stream=None, warmup=2, timesteps=None, sampler=None, inpaint=False, concat=None, control=False,
                cfg=True, ip_adapter=False, freeu=False, pag=False, prediction="eps", cfg_rescale=False, motion=False, frames=None):
        """Capture one denoising step for these (static) buffers into a HIP graph.  Afterwards
        ``step(timestep, a_t, a_prev, guidance)`` updates ``latent`` in place with one graph launch.

        Step-invariant work stays out of the captured step (config.hoist_step_invariants): the cross-attention K|V projection of the
        context runs here and in ``set_context`` -- it depends on the context alone -- and the time-embedding row of a timestep (the MLP
        of unet.py:54-56 + the 22 ResBlock projections of resnet.py:28) is computed once per distinct timestep, kept in a table, and
        handed to the replay by the launch that sets the step scalars.  ``timesteps``: the schedule, to fill the table up front.

        The captured step reads PRIVATE buffers (the stacked context and, hoisted, its K|V projection): ``set_context`` is the only supported
        way to change the prompts of a compiled sampler -- writing into the arrays handed to ``compile`` (or into ``_ctx2``) changes nothing the
        cross-attention reads.  The hoisted tables are keyed by ``weights_key()``: eager steps (``step(..., eager=True)``) follow weights replaced
        after ``compile``; the captured graph holds the addresses of the weights it was captured with, so a new weight set needs ``compile`` again.

        ``sampler``: a ``Schedule`` (variants/samplers.py, e.g. ``DPMSolverPP2M().schedule(20)``).  The captured step then ends in the fused
        sampler update (tf_cfg_sampler_step_*) instead of the DDIM one, its coefficient table is uploaded once, the model owns an fp32 x0 history,
        and the sampler is driven by ``start`` / ``run`` / ``step_sampler``; ``step`` is refused.  Without one, nothing changes.

        ``inpaint=True`` (with a sampler only): the model owns private fp32 ``x0_init`` (the clean latent) and ``mask`` (B,1,H,W) buffers, the
        mask all ones, and the captured step ends in the masked update (tf_cfg_sampler_step_masked_*), which keeps the region where the mask is
        0 on the noised trajectory of x0_init.  ``start(init_image= / init_latent=, mask=)`` fills them.

        ``concat="inpaint" | "edit"`` (with a sampler only): a concat-conditioned UNet -- SD15_INPAINT, in_channels 9, reads [latent(4) | mask(1) |
        0.18215 x means of the masked image(4)]; SD15_EDIT (InstructPix2Pix), in_channels 8, reads [latent(4) | unscaled means of the image to
        edit(4)].  The model owns a private fp32 conditioning buffer (B, 5 | 4, h, w), zero until ``start(cond_image= / cond_latent=)`` fills it, and
        the captured step opens with tf_cfg_concat_* in place of tf_cfg_duplicate_* (the same launch count).  "inpaint" runs the two CFG groups with
        the conditioning in both and ends in tf_cfg_sampler_step_*; "edit" runs three groups [x|0, unc ; x|c, unc ; x|c, ctx] and ends in
        tf_cfg3_sampler_step_*: e = e0 + g_T (e2 - e1) + g_I (e1 - e0), g_T the guidance of step_sampler / run and g_I the image guidance (1.5 until
        ``start(image_guidance=)`` sets it).  A model whose in_channels is not 4 compiles with the matching ``concat`` only.

        ``control=True`` (with a sampler and an attached ControlNet, ``attach_control``): the captured step runs the UNet's encoder, the ControlNet on
        the same stacked latent, and one launch (tf_control_add_16) that adds the 13 residuals to the skip tensors and the middle output, scaled by a
        device fp32 array -- all inside the one graph.  The model owns a private hint embedding (G B, model_channels, h, w), zero until
        ``start(control_image= / control_hint=)`` fills it, the scales (all ones until ``start(control_scale=)``), and the ControlNet's hoisted K|V
        projection; its time-embedding row travels behind the UNet's in the one buffer the parameter launch copies.  Combines with ``inpaint=True``
        (the latent blend lives in the sampler tail); not with ``concat=``, TF_CFG_PARALLEL or the fp8 policy.

        ``cfg=False`` (with a sampler only): the guidance-free step of a consistency model (samplers.LCM with an LCM-LoRA merged in), which samples at
        guidance 1 where e = e_u + 1 (e_c - e_u) = e_c.  ONE guidance group: the captured step opens with tf_latent_stack1_* (the conditioning channels
        of concat="inpaint" behind the latent), runs the UNet -- and a ControlNet, its hint embedding one group -- on B images against ``context`` alone,
        hoisted K|V included, and ends in tf_sampler_step1_* (its masked form for inpaint=True): the launch count of the CFG step, half the rows in every
        launch.  ``unconditional_context`` may be None here and in ``set_context`` (it is ignored if given); ``run`` / ``step_sampler`` take guidance
        None or 1.0 and raise ValueError for anything else.  Not with concat="edit", TF_CFG_PARALLEL or the fp8 policy.  cfg=True with an LCM schedule
        runs the two-branch step with that table (LCM-LoRA at guidance 1-2).

        ``ip_adapter=True`` (with a sampler and an attached IPAdapter, ``attach_ip_adapter``): every cross-attention of the UNet becomes the dual
        launch (tf_sdpa_dual_16) -- the same number of graph nodes.  The model owns the image tokens' K|V (G B, T, kv_n), zero until
        ``start(ip_image_embeds=)`` projects it (outside the graph, as the text K|V is), and a device fp32 array with one strength per
        cross-attention, all ones; ``set_ip_scale`` changes them without a re-capture, and at 0 the step computes what the un-adapted step
        computes.  Combines with cfg=False, inpaint=True, concat="inpaint", control=True, LoRA, bf16; not with concat="edit", TF_CFG_PARALLEL or
        the fp8 policy.  (The warm-up steps run every dual instance once before the capture: its first launch sets a function attribute.)

        ``freeu=True`` (with a sampler only): FreeU (Si et al. 2023, as diffusers' ``enable_freeu`` states it) inside the captured step -- in front
        of the concats of the first two decoder stages one launch (tf_freeu_skip_16) puts the 2 (num_res_blocks + 1) skip tensors through the
        Fourier filter, behind the encoder and behind tf_control_add_16 where there is one, and one launch per block (tf_freeu_backbone_16) scales
        the first half of the backbone's channels.  The model owns the device fp32 words [s1, s2, b1, b2], all ones; ``set_freeu`` and
        ``start(freeu=)`` change them without a re-capture.  At all ones both kernels copy their input's bits, yet the step is NOT bit for bit
        the freeu=False step: the tensors FreeU makes carry no GroupNorm statistics, so those concats' GroupNorms compute their own (two passes
        over the stored 16-bit values) where the plain step merges the fp32 partials its producing convolutions emitted -- the same numbers up
        to fp32 summation order and the 16-bit rounding of the producer's output.  Combines with cfg=False, inpaint=True, both concat= modes,
        control=True, ip_adapter=True, LoRA, bf16; not with TF_CFG_PARALLEL or the fp8 policy.

        ``pag=True`` (with a sampler only): perturbed-attention guidance (Ahn et al. 2024, as diffusers' PAG pipelines state it).  One more
        guidance group, the perturbed one, runs the UNet on the conditional inputs (the prompt's context, an IP-Adapter's image tokens, the
        concat="inpaint" channels, the control hint) with the self-attention of the selected SpatialTransformers replaced by the identity,
        attn1(x) = to_out(to_v(norm1(x))): the groups are [uncond ; perturbed ; cond] (three) and, with cfg=False, [perturbed ; cond] (two).  Every
        self-attention of the UNet becomes tf_sdpa_pag_16 -- one launch either way, the same number of graph nodes as the step without PAG --
        which reads its layer's word of a 16-word device array when it runs; a ControlNet runs all groups unperturbed.  The combine is
        e = e_u + g (e_c - e_u) + s_t (e_c - e_p) (cfg=False: e_c + s_t (e_c - e_p)), s_t = max(0, s - a (1000 - t)), through the tails that
        exist: the three-group expression at g_I = g, g_T = g + s_t, the pair expression at guidance 1 + s_t -- the scale travels in the guidance
        word of the parameter launch and in the edit word, so a replay has no launch more.  ``set_pag`` / ``start(pag=)`` change scale, layers and
        adaptive scale without a re-capture; after compile they are 3.0, "mid" and 0.  With no layer selected e_p is e_c bit for bit; at scale 0
        the step is the pag=False step up to the tail's rounding.  Combines with cfg=False, inpaint=True, concat="inpaint", control=True,
        ip_adapter=True, freeu=True, LoRA, bf16; not with concat="edit" (a fourth group), TF_CFG_PARALLEL or the fp8 policy.  The UNet's head sizes
        must be among 40, 64, 80, 128 and 160 (the LDS-DMA attention families; SD-1.5: 40, 80, 160).

        ``prediction="v"`` (with a sampler only): the UNet's output is v (Salimans & Ho 2022) as the SD-2.x 768-v checkpoints predict it; the tail's x0
        line becomes x0 = sqrt(a_t) x - sqrt(1 - a_t) v and nothing else changes (the coefficient tables are in x0 form).  Combines with everything that
        has a sampler.  ``cfg_rescale=True`` (with a sampler and a guidance pair or triple: cfg=True or pag=True; not concat="edit"): CFG rescale (Lin et
        al. 2023; diffusers' ``guidance_rescale``) -- per image the combined output is scaled to the standard deviation of the text group's, e' = phi e
        std(e_t) / std(e) + (1 - phi) e, inside the step's last launch (tf_sampler_tail_*, csrc/sampler.hip: one block per image, two-pass statistics in
        a fixed order), so the step keeps its number of graph nodes.  The model owns the device word phi, 0.7 after compile (the paper's suggestion, not
        tuned here); ``set_cfg_rescale`` and ``start(cfg_rescale=)`` change it without a re-capture, and at 0 the step computes the cfg_rescale=False
        step's bits.  With the defaults the tail is the entry it always was.  Neither runs under TF_CFG_PARALLEL.

        ``motion=True, frames=F`` (with a sampler and an attached MotionAdapter, ``attach_motion``): the video step of AnimateDiff.  The latent is
        (V F, 4, h, w), V videos of F frames in (video, frame) order, 1 <= F <= min(32, the adapter's max_len); every motion module runs at its slot of
        the UNet (vision/unet.py::UNetModel._with_motion) on G V videos, G the guidance groups -- nine launches per module, the temporal attention
        (tf_sdpa_temporal_16) among them, all inside the one graph; the positional tables pe W^T are built here, outside it.  The context has V F rows,
        or V rows -- one prompt per video: its K|V is projected once per video in the hoist and the projected rows are replicated to the video's
        frames (DESIGN 4.3 states the memory this costs).  ``set_motion_scale`` / ``start(motion_scale=)`` change the strength of the modules'
        residual branch without a re-capture; it is 1 after compile.  Combines with cfg=False, every sampler, prediction="v", cfg_rescale=True,
        image-to-image starts (an init_latent of V F frames), bf16 and LoRA on the UNet's own weights; not with control=True, ip_adapter=True, concat=,
        pag=True, freeu=True, inpaint=True, the fp8 policy, TF_CFG_PARALLEL or an SDXL model, each refused by name.  With motion=False an attached
        adapter changes nothing: the image step's bits and launches.

        The arguments are remembered: ``set_adapters`` (LoRA) on a compiled model swaps weight handles and calls ``compile`` again with the same ones."""
        inputs.check_compile(self.model.diffusion_model.cfg.in_channels, self.control_model is not None, config, latent, sampler, inpaint, concat, control, cfg,
                             ip_adapter=ip_adapter, has_ip_adapter=self._ip_model is not None, freeu=freeu,
                             freeu_plan=freeu_stages(self.model.diffusion_model.cfg) if freeu else (), pag=pag,
                             pag_table=pag_layers(self.model.diffusion_model.cfg) if pag else (), prediction=prediction, cfg_rescale=cfg_rescale,
                             head_sizes=head_sizes(self.model.diffusion_model.cfg) if ip_adapter else (),
                             adm=bool(self.model.diffusion_model.cfg.adm_in_channels), motion=bool(motion), has_motion=self._motion_model is not None,
                             frames=frames, motion_max_len=self._motion_model.max_len if self._motion_model is not None else 0)
        if motion and context.shape[0] not in (latent.shape[0], latent.shape[0] // int(frames)):
            raise ValueError(f"StableDiffusion.compile: motion=True takes one context row per frame ({latent.shape[0]}) or per video ({latent.shape[0] // int(frames)}), "
                             f"got {context.shape[0]}")
        if (ip_adapter or pag) and warmup < 1:
            raise ValueError(f"StableDiffusion.compile: {'ip_adapter' if ip_adapter else 'pag'}=True needs warmup >= 1 (the first launch of an attention instance cannot be captured)")
        if sampler is not None:
            timesteps = sampler.timesteps
        self._reset_state()
        self._compile_args = dict(unconditional_context=unconditional_context, context=context, latent=latent, warmup=warmup, timesteps=timesteps,
                                  sampler=sampler, inpaint=inpaint, concat=concat, control=control, cfg=cfg, ip_adapter=ip_adapter, freeu=freeu, pag=pag,
                                  prediction=prediction, cfg_rescale=cfg_rescale, motion=motion, frames=frames)
        self._stream = stream or Stream()
        self._latent, self._unc, self._ctx = latent, unconditional_context, context
        self._sched, self._inpaint, self._concat, self._control = sampler, bool(inpaint), concat, bool(control)
        self._cfg, self._pag = bool(cfg), bool(pag)
        self._groups = 3 if concat == "edit" else (2 if cfg else 1) + (1 if pag else 0)
        self._ip = bool(ip_adapter)
        self._freeu = bool(freeu)
        self._vpred, self._rescale = prediction == "v", bool(cfg_rescale)
        self._adm = bool(self.model.diffusion_model.cfg.adm_in_channels)
        self._ip_model_compiled = self._ip_model if self._ip else None
        self._motion, self._frames = bool(motion), int(frames) if motion else None
        self._motion_compiled = self._motion_model if self._motion else None
        if sampler is not None:
            with use_stream(self._stream):
                self._alloc_sampler_buffers()
        sp = self._step_params()
        with use_stream(self._stream):
            self._hoist(sp, timesteps)
            self._warm_up(sp, warmup)
            self._capture(sp)
        return self

    def _alloc_sampler_buffers(self):
        """What a sampler schedule and its modes (inpaint, concat, control) own, on the current stream."""
        b, _, h, w = shape = self._latent.shape
        self._params = StepParams(DeviceArray.zeros((8,), np.float32, "row"))      # the sampler block: the 4 step scalars + row, seed, image offset
        self._coeffs = DeviceArray.from_numpy(np.asarray(self._sched.coeffs, np.float32), np.float32, "row")
        self._x0_hist = DeviceArray.zeros(shape, np.float32, "row")
        if self._inpaint:
            self._x0_init = DeviceArray.zeros(shape, np.float32, "row")
            self._mask = DeviceArray.from_numpy(np.ones((b, 1, h, w), np.float32), np.float32, "row")
        if self._concat is not None:
            self._cond = DeviceArray.zeros((b, inputs.CONCAT_CHANNELS[self._concat], h, w), np.float32, "row")
        if self._concat is not None or self._groups == 3:
            self._edit = DeviceArray.zeros((4,), np.float32, "row")      # [0] g_I, the image guidance of the three-branch update (pag=True: the CFG scale g)
            hip.tf_set_step_params(self._edit.ptr, 1.5, 0.0, 0.0, 0.0, _sh())
        if self._control:
            self._hint_emb = DeviceArray.zeros((self._groups * b, self.control_model.cfg.model_channels, h, w), _step_dtype(), "nhwc")
            self._control_scales = DeviceArray.from_numpy(np.ones((16,), np.float32), np.float32, "row")     # one per residual; 16: whole 4-word writes
        if self._freeu:
            self._freeu_scales = DeviceArray.from_numpy(np.ones((4,), np.float32), np.float32, "row")      # [s1, s2, b1, b2]: one 4-word write
        if self._rescale:
            self._rescale_phi = DeviceArray.from_numpy(np.asarray([0.7, 0.0, 0.0, 0.0], np.float32), np.float32, "row")       # [0] phi: one 4-word write
        if self._pag:
            self._pag_flags = DeviceArray.from_numpy(inputs.pag_layer_words("mid", pag_layers(self.model.diffusion_model.cfg)), np.float32, "row")
        if self._adm:                        # y = 0 until start(pooled=) writes it: the warm-up steps and the capture read these buffers
            ucfg = self.model.diffusion_model.cfg
            self._adm_y = DeviceArray.zeros((self._groups * b, ucfg.adm_in_channels), _step_dtype(), "row")
            self._y_emb = DeviceArray.empty((self._groups * b, 4 * ucfg.model_channels), _step_dtype(), "row")
        if self._ip:
            ad = self._ip_model_compiled
            self._ip_kv = DeviceArray.zeros((self._groups * b, ad.num_tokens, ad.kv_layout()[1]), _step_dtype(), "row")
            self._ip_scales = DeviceArray.from_numpy(inputs.ip_scales(None, len(ad.paths)), np.float32, "row")

    def _hoist(self, sp, timesteps):
        """The private stacked context and -- config.hoist_step_invariants -- what depends on it or on the timestep alone: the K|V projections and
        the buffer ``_emb_cur`` the captured step reads its time-embedding row from, with the rows of ``timesteps`` computed up front."""
        self._ctx2 = self._frame_context(self._stack_context(self._unc, self._ctx, self._groups, self._cond_groups()))
        if self._adm:
            self._refresh_y_emb()
        if self._motion:                     # the positional tables pe W^T and the live last launches: built once, outside the captured step
            self._motion_compiled.set_scale(1.0)
            self._motion_compiled.prepare(self._frames)
        if not config.hoist_step_invariants or config.cfg_parallel:
            return
        self._kv_all, self._kv_key = self._context_kv(), self._weights_key()
        if self._control:
            self._ckv_all = self.control_model.context_kv(self._ctx2)
        row = self._time_row(sp.set(981.0))
        self._emb_cur = DeviceArray.empty(row.shape, row.dtype, "row")       # what the captured step reads (fp16, or bfloat16 bits in the bf16 step)
        assert self._emb_cur.nbytes % 16 == 0
        hip.tf_memcpy_async(self._emb_cur.ptr, row.ptr, row.nbytes, 3, _sh())   # (the warm-up steps run at t = 981)
        self._keep_row = row
        if self._adm:
            return                           # the schedule's rows depend on y: start() builds them all in one pass (_build_adm_table)
        for t in (timesteps if timesteps is not None else ()):
            self._emb_row(float(t))

    def _per_frame(self, a):
        """(R, ...) rows, one per (group, video) -> (R F, ...): every row F times, adjacent -- the (group, video, frame) order of the stacked latent."""
        f, per = self._frames, a.nbytes // a.shape[0]
        out = DeviceArray.empty((a.shape[0] * f,) + a.shape[1:], a.dtype, a.layout)
        for r in range(a.shape[0]):
            for k in range(f):
                hip.tf_memcpy_async(out.ptr + (r * f + k) * per, a.ptr + r * per, per, 3, _sh())
        out._base = a                        # (referenced until the copies have run)
        return out

    def _frame_context(self, stacked):
        """The stacked context the UNet reads, one row per image.  motion=True with one prompt per video: the per-video stack is kept (``_ctx_vid``:
        what the hoisted K|V is projected from) and its rows are replicated to the video's frames."""
        self._ctx_vid = None
        if not self._motion or stacked.shape[0] == self._groups * self._latent.shape[0]:
            return stacked
        self._ctx_vid = stacked
        return self._per_frame(stacked)

    def _context_kv(self):
        """The UNet's hoisted K|V projection of the stacked context; one prompt per video: projected once per video, the rows replicated to its frames."""
        if self._ctx_vid is None:
            return self.model.diffusion_model.context_kv(self._ctx2)
        return self._per_frame(self.model.diffusion_model.context_kv(self._ctx_vid))

    def _warm_up(self, sp, warmup):
        """``warmup`` eager steps at t = 981 on a latent that is put back afterwards: they warm the pool and build the lazily packed weights."""
        latent = self._latent
        saved = DeviceArray.empty(latent.shape, np.float32, "row")
        hip.tf_memcpy_async(saved.ptr, latent.ptr, latent.nbytes, 3, _sh())
        for _ in range(warmup):
            if self._sched is not None:
                hip.tf_set_sampler_params(sp.dev.ptr, 981.0, 0.5, 0.6, 7.5, 0, 0, 0, 0, None, None, 0, _sh())
            else:
                sp.set(981.0, 0.5, 0.6, 7.5)
            self._eager_step(sp)
        hip.tf_memcpy_async(latent.ptr, saved.ptr, latent.nbytes, 3, _sh())
        self._stream.synchronize()

    def _capture(self, sp):
        """Capture one ``_eager_step`` on the (drained) sampler stream into the graph ``step`` replays."""
        if self._graph_blocks:          # a previous graph of this model: its buffers go back to the pool
            hip.tf_graph_destroy(self._graph)
            pool().disown(self._graph_blocks)
            self._graph, self._graph_blocks = None, None
        pool().begin_capture()
        g, ok = ctypes.c_void_p(), False
        try:
            hip.tf_graph_begin_capture(self._stream.handle)
            self._eager_step(sp)
            hip.tf_graph_end_capture(self._stream.handle, ctypes.byref(g))
            ok = True
        finally:
            blocks = pool().end_capture()    # every block the captured step touches now belongs to the graph
            if not ok:
                # an op raised inside the capture (pool frozen, untuned shape, ...): leave capture mode so that the stream
                # stays usable, and give the blocks back -- there is no graph to own them
                hip.tf_graph_abort_capture(self._stream.handle)
                self._keep = None
                pool().disown(blocks)
        self._graph, self._graph_blocks = g, blocks

    def _eager_step(self, sp):
        """One step, launch by launch -- what ``_capture`` records: the stacked input, the UNet, the tail that updates the latent."""
        x2 = self._latent_stack1() if self._groups == 1 else self._cfg_concat() if self._concat else self._latent_stack3() if self._groups == 3 \
            else self._cfg_duplicate(self._latent)
        outs = self._unet_two_chains(x2, sp) if config.cfg_parallel else (self._unet(x2, sp),)
        self._tail(sp, *outs[:2])
        self._keep = (x2,) + outs       # graph nodes reference these blocks: keep them out of the pool

    def _unet(self, x2, sp):
        """The UNet's output for the stacked input: plain, from the hoisted row and K|V, or controlled."""
        unet, cn, row, ctx = self.model.diffusion_model, self.control_model, self._emb_cur, self._ctx2
        ip = (self._ip_model_compiled, self._ip_kv, self._ip_scales) if self._ip else None
        b = self._latent.shape[0]
        pag = (self._pag_flags, ((self._groups - 2) * b, (self._groups - 1) * b)) if self._pag else None      # the group in front of the conditional one
        if self._motion:                     # (refused together with control / ip / freeu / pag: the plain call with the modules in)
            return unet(x2, sp, ctx, shared=None if row is None else (None, row, self._kv_all), motion=(self._motion_compiled, self._frames))
        if not self._control:
            return unet(x2, sp, ctx, shared=None if row is None else (None, row, self._kv_all), ip=ip, freeu=self._freeu_scales, pag=pag,
                        y_emb=self._y_emb if row is None else None)     # (step() has put this timestep's row -- SDXL: one per image -- into _emb_cur)
        # the UNet's encoder, then the ControlNet on the same stacked latent, then the seam (UNetModel.__call__ calls `residuals` behind its
        # middle block); each model reads its own view of the hoisted row [UNet's | ControlNet's]
        shared_u = shared_c = None
        if row is not None:
            nu = row.shape[1] - cn._prepare()["emb_w"].shape[0]
            shared_u = (None, row.view((1, nu), "row"), self._kv_all)
            shared_c = (None, row.view((1, row.shape[1] - nu), "row", nu), self._ckv_all)
        residuals = lambda: cn(x2, self._hint_emb, sp, ctx, shared=shared_c)
        return unet(x2, sp, ctx, shared=shared_u, control=(residuals, self._control_scales), ip=ip, freeu=self._freeu_scales, pag=pag)

    def _unet_two_chains(self, x2, sp):
        """config.cfg_parallel: the unconditional and the conditional half of the CFG pair (variants/sd.py:31-32) as two independent UNet chains: one
        runs as a side branch of the step (its own stream / graph branch), so the launch gaps and partly filled grids of one chain are covered by
        the other; what both share (time embedding, context K|V) is computed once in front of the fork.  -> (out_u, out_c, the shared arrays...)."""
        unet, b = self.model.diffusion_model, self._latent.shape[0]
        emb, emb_all, kv_all = unet.step_shared(sp, self._ctx2)
        half = lambda a, i: a.view((b,) + a.shape[1:], a.layout, i * b * (a.size // a.shape[0])) if a is not None else None
        br = Branch()
        with br:
            out_u = unet(half(x2, 0), sp, None, shared=(emb, emb_all, half(kv_all, 0)))
        out_c = unet(half(x2, 1), sp, None, shared=(emb, emb_all, half(kv_all, 1)))
        br.join()
        return out_u, out_c, emb, emb_all, kv_all

    def _tail(self, sp, out, out_c=None):
        """The step's last launch, by mode: CFG combine + the DDIM update (from two chains: tf_cfg_ddim_step2_f32), or the sampler update of the
        schedule's row -- three-branch for an edit model and for pag=True with CFG, masked for inpaint=True, single-branch (tf_sampler_step1_*, both
        forms) for cfg=False without PAG; pag=True with cfg=False ends in the pair's tails on [perturbed ; cond]."""
        lat, (b, c, h, w) = self._latent, self._latent.shape
        if out_c is not None:
            return hip.tf_cfg_ddim_step2_f32(lat.ptr, out.ptr, out_c.ptr, sp.dev.ptr, b, c, h, w, _sh())
        if self._sched is None:
            return _entry16("tf_cfg_ddim_step", "f32")(lat.ptr, out.ptr, sp.dev.ptr, b, c, h, w, _sh())
        if self._vpred or self._rescale:          # the one entry that states every form (csrc/sampler.hip): flags bit 0 v, bit 1 masked, bit 2 rescale
            ptr = lambda a: a.ptr if a is not None else None
            flags = (1 if self._vpred else 0) | (2 if self._inpaint else 0) | (4 if self._rescale else 0)
            return _entry16("tf_sampler_tail", "f32")(lat.ptr, out.ptr, self._x0_hist.ptr, sp.dev.ptr, self._coeffs.ptr, len(self._sched.timesteps),
                                                      self._edit.ptr if self._groups == 3 else None, ptr(self._x0_init), ptr(self._mask), ptr(self._rescale_phi),
                                                      b, c, h, w, self._groups, flags, _sh())
        if self._groups == 1:
            extra = (self._x0_init.ptr, self._mask.ptr) if self._inpaint else (None, None)
            return _entry16("tf_sampler_step1", "f32")(lat.ptr, out.ptr, self._x0_hist.ptr, sp.dev.ptr, self._coeffs.ptr, len(self._sched.timesteps), *extra, b, c, h, w, _sh())
        stem, extra = ("tf_cfg3_sampler_step_masked", (self._edit.ptr, self._x0_init.ptr, self._mask.ptr)) if self._groups == 3 and self._inpaint else \
                      ("tf_cfg3_sampler_step", (self._edit.ptr,)) if self._groups == 3 else \
                      ("tf_cfg_sampler_step_masked", (self._x0_init.ptr, self._mask.ptr)) if self._inpaint else ("tf_cfg_sampler_step", ())
        _entry16(stem, "f32")(lat.ptr, out.ptr, self._x0_hist.ptr, sp.dev.ptr, self._coeffs.ptr, len(self._sched.timesteps), *extra, b, c, h, w, _sh())

    def _advance(self, timestep, eager, set_params):
        """What ``step`` and ``step_sampler`` share, on the sampler stream: the parameter launch ``set_params(dst, src, nbytes)`` -- hoisted, it also
        copies this timestep's cached row (src) into ``_emb_cur`` (dst); (None, None, 0) otherwise -- then one graph replay, or the eager step.
        The stream switch is un-ordered on purpose: an event edge between two graph launches costs 0.2 ms per step (measured, tools/ab3.sh), and
        consecutive steps are ordered by the stream itself."""
        with use_stream(self._stream, ordered=False):
            if self._emb_cur is not None:
                row = self._hoisted_row(timestep)
                set_params(self._emb_cur.ptr, row.ptr, row.nbytes)
            else:
                set_params(None, None, 0)
            if eager or self._graph is None:
                self._eager_step(self._params)
            else:
                hip.tf_graph_launch(self._graph, self._stream.handle)

    def step(self, timestep, a_t, a_prev, guidance, eager=False):
        """One denoising step on the sampler stream, asynchronous (``_advance``).  Work on other streams that touches the latent goes through
        set_latent() / synchronize().
        After a ``set_adapters`` that changed a weight of a compiled model, ``set_latent`` must come first (UnsupportedSamplerConfig otherwise)."""
        self._require_compiled("step")
        if self._sched is not None:
            raise UnsupportedSamplerConfig("StableDiffusion.step: this model was compiled with a sampler schedule -- drive it with start() / run() / step_sampler()")
        self._require_started("step")
        sp = self._params

        def set_params(dst, src, nbytes):
            if dst is None:
                sp.set(timestep, a_t, a_prev, guidance)
            else:
                hip.tf_set_step_params_copy(sp.dev.ptr, float(timestep), float(a_t), float(a_prev), float(guidance), dst, src, nbytes, _sh())
        self._advance(timestep, eager, set_params)

    def _hoisted_row(self, timestep):
        """The cached time-embedding row of this timestep for the replay's parameter launch; refreshes the hoisted K|V first if a weight changed."""
        key = self._weights_key()
        if self._kv_all is not None and self._kv_key != key:
            # a to_k / to_v (or any hoisted) weight was replaced since compile(): the K|V projection the graph reads is stale -- refresh it in place
            self._kv_tmp, self._kv_key = self._refresh_kv(), key
        return self._emb_row(float(timestep), key)     # (computed on this stream the first time a timestep is seen)

    # -- sampler schedules (compile(..., sampler=Schedule)) -----------------------------------------------------------------------
    def _require_compiled(self, what):
        if self._stream is None:
            raise RuntimeError(f"StableDiffusion.{what}: compile() first -- this model has no compiled step, sampler stream or latent yet")

    def _require_started(self, what):
        if self._needs_start:
            raise UnsupportedSamplerConfig(f"StableDiffusion.{what}: set_adapters captured the step again and the previous start's state (latent, mask, "
                                           "conditioning, hint, cursor) did not survive -- call start() (or set_latent(), for the DDIM step) first")

    def _require_sampler(self, what):
        if self._sched is None:
            raise UnsupportedSamplerConfig(f"StableDiffusion.{what}: compile(..., sampler=<Schedule>) first (this model "
                                           + ("was never compiled)" if self._stream is None else "runs the DDIM step())"))
        return self._sched

    def start(self, seed=None, noise=None, image_offset=0, init_image=None, init_latent=None, mask=None, cond_image=None, cond_mask=None,
              cond_latent=None, image_guidance=None, control_image=None, control_hint=None, control_scale=None, ip_image_embeds=None, ip_image=None,
              ip_scale=None, freeu=None, pag=None, cfg_rescale=None, pooled=None, uncond_pooled=None, original_size=None, crop_top_left=None,
              target_size=None, uncond_size_ids=None, motion_scale=None):
        """A new image batch for the compiled sampler: sets the latent in place and rewinds the schedule.  ``seed``: the initial latent is
        drawn on the device (tag 0; image b is global image image_offset + b), and the ancestral noise of every step comes from the same seed
        (tag 1); ``noise``: a host (B,C,H,W) array for the initial latent instead (the ancestral noise then uses ``seed``, default 0).
        Ordered after every step already queued.

        Image-to-image: ``init_image`` (uint8 (B,H,W,3), encoded by ``encode_image``) or ``init_latent`` (x0, fp32 (B,C,H,W), host or device)
        sets latent = sqrt(a) x0 + sqrt(1 - a) z at the schedule's start level a = alphas[0] (Sampler.schedule(..., strength=)), z the tag-0
        noise of ``seed`` -- the noise a text-to-image start from that seed draws.  Inpainting (a model compiled with inpaint=True, which
        requires an init): ``mask`` -- a latent_mask() input, or a device fp32 (B,1,h,w) array; 1 = repaint -- is written into the model's mask
        buffer (all ones without one) and x0 into its x0_init buffer.

        A concat-conditioned model (compile(..., concat=)) needs its conditioning at every start, orthogonally to the arguments above (image-to-image
        on an inpainting checkpoint works).  ``cond_image`` (uint8 (B,H,W,3), host or device) goes through the VAE encoder on the device: "edit"
        keeps the unscaled means of the image; "inpaint" needs ``cond_mask`` too (a concat_mask() input, host (B,H,W); 1 = repaint) and writes
        [concat_mask | 0.18215 x means of the image with the masked pixels set to 0].  ``cond_latent``: the fp32 (B, 5 | 4, h, w) conditioning itself,
        host or device, copied as it is.  ``image_guidance`` ("edit" only): g_I of the three-branch update, kept until the next value.  Every
        argument is checked before anything is written.

        A controlled model (compile(..., control=True)) needs its hint at every start: ``control_image`` (uint8 (B | 1, 8h, 8w, 3), host or device;
        x / 255 on the device) or ``control_hint`` (a host float (B | 1, 3, 8h, 8w) array in [0, 1]) goes through the ControlNet's hint stem once,
        here; a single hint serves every image.  ``control_scale``: the strength of the 13 residuals, one float or one per residual (12 skip
        connections in input-block order, then the middle block); 1 when not given.  Hint and scales follow a new start without a recompile.

        An adapted model (compile(..., ip_adapter=True)) needs its image prompt at every start: ``ip_image_embeds``, a host float (B | 1, E) array of
        CLIP image embeddings.  The conditional group reads the adapter's tokens of the embeddings, the unconditional group its tokens of zeros (the
        published convention); the image tokens' K|V is projected here, outside the graph.  ``ip_scale``: one float or one per cross-attention (adapter
        order: down, up, mid); 1 when not given.  ``ip_image`` (uint8 (B | 1, S, S, 3), host or device, S the tower's image size: 224 for ViT-H; resized
        and cropped by the caller) instead of ``ip_image_embeds``: the attached CLIP vision tower (``attach_clip_vision``) computes the embeddings on
        the device, ordered into the sampler stream; [0 | embeddings] for the CFG pair is built there too.  Without a tower it is refused.

        A FreeU model (compile(..., freeu=True)): ``freeu=(s1, s2, b1, b2)`` writes the four scalars as ``set_freeu`` does; without it they keep
        their values.

        A PAG model (compile(..., pag=True)): ``pag=(scale, layers)`` or ``(scale, layers, adaptive)`` sets what ``set_pag`` sets; without it they
        keep their values.

        A rescaled model (compile(..., cfg_rescale=True)): ``cfg_rescale=phi`` writes the word ``set_cfg_rescale`` writes; without it phi keeps its
        value.

        A vector-conditioned model (UNetConfig.adm_in_channels: SDXL) needs ``pooled`` at every start: the pooled text vector, a host float (B | 1, P)
        array (``encode_prompt``'s second result).  ``uncond_pooled``: the unconditional group's (zeros when not given).  ``original_size``,
        ``crop_top_left``, ``target_size``: (h, w) pairs in pixels, or (B, 2) arrays with a pair per image; when not given the latent's size x 8,
        (0, 0) and the latent's size x 8.  ``uncond_size_ids``: the unconditional group's six ids (B | 1, 6) [original h, w, crop top, left, target
        h, w]; the conditional ones when not given.  y = [pooled | Fourier(ids)] (tf_adm_vector_16), label_emb(y) and the time-embedding rows of
        the whole schedule -- one per step and image -- are computed here: the replay's parameter launch copies G B rows where it copied one.
        On any other model these arguments raise.

        A video model (compile(..., motion=True)): the latent is V F frames in (video, frame) order -- ``init_latent`` likewise; ``motion_scale`` (one
        float, or one per motion module in execution order) writes what ``set_motion_scale`` writes; without it the scale keeps its value."""
        self._require_sampler("start")
        ms = self._check_motion_scale(motion_scale, "start")
        adm = self._check_adm(pooled, uncond_pooled, original_size, crop_top_left, target_size, uncond_size_ids)
        phi = self._check_cfg_rescale(cfg_rescale, "start")
        pg = self._check_pag(pag, "start")
        fu = self._check_freeu(freeu, "start")
        ipa = self._check_ip(ip_image_embeds, ip_image, ip_scale)
        ctrl = self._check_control(control_image, control_hint, control_scale)
        cond = self._check_cond(cond_image, cond_mask, cond_latent, image_guidance)
        latent = self._check_latent(seed, noise, image_offset, init_image, init_latent, mask)
        self._write_latent(*latent)                # every check has passed: from here on the model changes
        if cond is not None:
            self._write_cond(*cond)
        if ctrl is not None:
            self._write_control(*ctrl)
        if ipa is not None:
            self._write_ip(*ipa)
        if fu is not None:
            self._write_freeu(fu)
        if pg is not None:
            self._write_pag(*pg)
        if phi is not None:
            self._write_cfg_rescale(phi)
        if adm is not None:
            self._write_adm(*adm)
        if ms is not None:
            self._write_motion_scale(ms)
        return self._latent

    def _check_motion_scale(self, value, who):
        """The motion scale checked against the compiled model before anything changes: None when not given, else one float per module."""
        if value is None:
            return None
        if not self._motion:
            raise ValueError(f"StableDiffusion.{who}: " + ("motion_scale= needs" if who == "start" else "needs") + " a model compiled with motion=True")
        return self._motion_compiled.scales(value)

    def _write_motion_scale(self, scales):
        """Rewrite every module's live last-launch weight and bias, round16(s base), on the sampler stream behind every step already queued: one
        elementwise launch per tensor, outside the graph, which reads the live copies (the bfloat16 step forms the products on the host: drained first)."""
        if config.is_bf16():
            self.synchronize()
        with use_stream(self._stream, ordered=False):
            self._motion_compiled.set_scale(scales)

    def set_motion_scale(self, scale=1.0):
        """The strength of the motion modules' residual branch, out = x_in + s proj_out(x), from the next step on: one finite float, or one per module
        in execution order (input blocks, middle block, output blocks), checked before anything is written.  The captured step reads private live
        copies of each module's last weight and bias, which this rewrites from the kept fp32 base: nothing is captured again.  0 switches the modules'
        contribution off (the step is then the image step up to the path the GroupNorm statistics take); 1 after compile."""
        self._require_sampler("set_motion_scale")
        self._write_motion_scale(self._check_motion_scale(scale, "set_motion_scale"))

    def _check_adm(self, pooled, uncond_pooled, original_size, crop_top_left, target_size, uncond_size_ids):
        """start()'s vector-conditioning arguments, checked against the compiled model before anything changes: None for a model without label_emb,
        else (pooled (R, P) fp32, size ids (R, 6) fp32) for the R = G B rows of the stacked batch, unconditional group first."""
        given = [n for n, v in (("pooled", pooled), ("uncond_pooled", uncond_pooled), ("original_size", original_size), ("crop_top_left", crop_top_left),
                                ("target_size", target_size), ("uncond_size_ids", uncond_size_ids)) if v is not None]
        if not self._adm:
            if given:
                raise UnsupportedSamplerConfig(f"StableDiffusion.start: {given[0]}= needs a vector-conditioned UNet (UNetConfig.adm_in_channels: SDXL); this model has none")
            return None
        if pooled is None:
            raise UnsupportedSamplerConfig("StableDiffusion.start: a vector-conditioned model (SDXL) reads its pooled text vector at every start -- pass pooled= "
                                           "(encode_prompt's second result)")
        ucfg = self.model.diffusion_model.cfg
        (b, _, h, w), p = self._latent.shape, ucfg.adm_in_channels - 6 * ucfg.adm_time_dim
        pc = inputs.adm_pooled(pooled, b, p, "pooled")
        pu = inputs.adm_pooled(uncond_pooled, b, p, "uncond_pooled") if uncond_pooled is not None else np.zeros_like(pc)
        ic = inputs.adm_size_ids(original_size, crop_top_left, target_size, b, 8 * h, 8 * w)
        iu = inputs.adm_ids(uncond_size_ids, b) if uncond_size_ids is not None else ic
        lead = self._groups - 1              # [uncond ; cond], or cond alone (cfg=False)
        return np.concatenate([pu] * lead + [pc]), np.concatenate([iu] * lead + [ic])

    def _write_adm(self, pooled, ids):
        """y = [pooled | Fourier(ids)] into the model's buffer, then everything that depends on it, on the sampler stream behind every step already
        queued.  The serial makes the rows of the previous start stale."""
        self.synchronize()
        ucfg = self.model.diffusion_model.cfg
        with use_stream(self._stream):
            dp, di = DeviceArray.from_numpy(pooled, _step_dtype(), "row"), DeviceArray.from_numpy(ids, np.float32, "row")
            hip.tf_adm_vector_16(dtag(self._adm_y.dtype), self._adm_y.ptr, dp.ptr, di.ptr, pooled.shape[0], pooled.shape[1], ucfg.adm_time_dim, 10000.0, _sh())
            self._adm_keep = (dp, di)                                    # (referenced until the kernel has run)
            self._adm_serial += 1
            self._refresh_y_emb()
            self._build_adm_table()

    def _refresh_y_emb(self):
        """label_emb(y) into the buffer an un-hoisted step reads (and the rows are built from), on the current stream."""
        y_emb = self.model.diffusion_model.label_embedding(self._adm_y)
        hip.tf_memcpy_async(self._y_emb.ptr, y_emb.ptr, y_emb.nbytes, 3, _sh())
        self._adm_keep = (self._adm_keep, y_emb)

    def _build_adm_table(self):
        """The whole schedule's time-embedding rows in one pass (UNetModel.time_embedding_table), keyed by the weights and this start's serial:
        row block s is what the parameter launch of step s copies into ``_emb_cur``."""
        if self._emb_cur is None:
            return                                                       # (not hoisted: the step computes its rows from _y_emb)
        ts = [float(t) for t in self._sched.timesteps]
        table = self.model.diffusion_model.time_embedding_table(ts, self._y_emb)
        r, n = self._emb_cur.shape
        assert table.shape == (len(ts) * r, n), (table.shape, len(ts), r, n)
        self._adm_table, self._emb_key = table, self._weights_key()
        self._emb_rows = {t: table.view((r, n), "row", i * r * n) for i, t in enumerate(ts)}

    def _check_cfg_rescale(self, phi, who):
        """phi checked against the compiled model before anything changes: None when not given, else the float in [0, 1]."""
        if phi is None:
            return None
        if not self._rescale:
            raise ValueError(f"StableDiffusion.{who}: " + ("cfg_rescale= needs" if who == "start" else "needs") + " a model compiled with cfg_rescale=True")
        return inputs.cfg_rescale_phi(phi, who)

    def _write_cfg_rescale(self, phi):
        with use_stream(self._stream, ordered=False):                    # stream-ordered: the value travels as a kernel argument
            hip.tf_set_step_params(self._rescale_phi.ptr, float(phi), 0.0, 0.0, 0.0, _sh())

    def set_cfg_rescale(self, phi=0.7):
        """CFG rescale's phi from the next step on: 0 <= phi <= 1, checked before anything is written; 0 is the un-rescaled step, 0.7 the paper's
        suggestion.  The captured step reads the word from the device: nothing is captured again."""
        self._require_sampler("set_cfg_rescale")
        self._write_cfg_rescale(self._check_cfg_rescale(phi, "set_cfg_rescale"))

    def _check_pag(self, pag, who):
        """(scale, layers[, adaptive]) checked against the compiled model before anything changes: None when not given, else (the 16 fp32 layer
        words, (scale, adaptive scale))."""
        if pag is None:
            return None
        if not self._pag:
            raise ValueError(f"StableDiffusion.{who}: " + ("pag= needs" if who == "start" else "needs") + " a model compiled with pag=True")
        if not isinstance(pag, (tuple, list)) or len(pag) not in (2, 3):
            raise ValueError(f"StableDiffusion.{who}: pag takes (scale, layers) or (scale, layers, adaptive), got {pag!r}")
        values = inputs.pag_values(pag[0], pag[2] if len(pag) == 3 else 0.0, who)
        return inputs.pag_layer_words(pag[1], pag_layers(self.model.diffusion_model.cfg), who), values

    def _write_pag(self, words, values):
        """The layer words -- one 64-byte write, four 4-word parameter launches on the sampler stream, behind every step already queued -- and the
        scales, which stay on the host: step_sampler folds them into the guidance word of its parameter launch."""
        with use_stream(self._stream, ordered=False):                    # stream-ordered: the values travel as kernel arguments
            for q in range(4):
                hip.tf_set_step_params(self._pag_flags.ptr + 16 * q, *(float(v) for v in words[4 * q:4 * q + 4]), _sh())
        self._pag_scale = values

    def set_pag(self, scale=3.0, layers="mid", adaptive=0.0):
        """Perturbed-attention guidance from the next step on.  ``scale``: s; ``adaptive``: a of s_t = max(0, s - a (1000 - t)); ``layers``: the
        SpatialTransformers whose self-attention the perturbed group replaces by the identity -- indices in execution order (SD-1.5: input_blocks
        0-5, middle_block 6, output_blocks 7-15), LDM paths ("input_blocks.4", "middle_block", "output_blocks.7"), the shorthands "down", "mid",
        "up", "all", or a list of any of these ([]: none, then e_p = e_c).  All of it is checked before anything is written.  The captured step
        reads the layer words from the device and the scale from the words its parameter launch carries: nothing is captured again."""
        self._require_sampler("set_pag")
        self._write_pag(*self._check_pag((scale, layers, adaptive), "set_pag"))

    def _check_freeu(self, values, who):
        """(s1, s2, b1, b2) checked against the compiled model before anything changes: None when not given, else the 4 fp32 words."""
        if values is None:
            return None
        if not self._freeu:
            raise ValueError(f"StableDiffusion.{who}: " + ("freeu= needs" if who == "start" else "needs") + " a model compiled with freeu=True")
        return inputs.freeu_scales(values, who)

    def _write_freeu(self, scales):
        with use_stream(self._stream, ordered=False):                    # stream-ordered: the values travel as kernel arguments
            hip.tf_set_step_params(self._freeu_scales.ptr, *(float(v) for v in scales), _sh())

    def set_freeu(self, s1=1.0, s2=1.0, b1=1.0, b2=1.0):
        """FreeU's four scalars from the next step on -- s1, s2: the Fourier filter's scale on the skips of decoder stage 1 and 2; b1, b2: the
        factor on the first half of the backbone's channels there -- four finite floats, checked before anything is written.  The captured step
        reads them from the device, so nothing is captured again.  All ones: the un-FreeU'd model's result up to the GroupNorm statistics path
        (``compile``).  The values usually quoted for SD-1.5 are s1 = 0.9, s2 = 0.2, b1 = 1.5, b2 = 1.6 (the authors' suggestion, not tuned here)."""
        self._require_sampler("set_freeu")
        self._write_freeu(self._check_freeu((s1, s2, b1, b2), "set_freeu"))

    def _check_ip(self, ip_image_embeds, ip_image, ip_scale):
        """start()'s adapter arguments, checked against the compiled model before anything changes: None for a model without ip_adapter=True,
        else (fp32 (B, E) embeddings, the fp32 scale words)."""
        if not self._ip:
            if any(v is not None for v in (ip_image_embeds, ip_image, ip_scale)):
                raise ValueError("StableDiffusion.start: ip_image_embeds=, ip_image= and ip_scale= need a model compiled with ip_adapter=True")
            return None
        if ip_image is not None and ip_image_embeds is not None:
            raise ValueError("StableDiffusion.start: pass ip_image= or ip_image_embeds=, not both")
        ad, b = self._ip_model_compiled, self._latent.shape[0]
        if ip_image is not None:
            tower = self._clip_vision
            if tower is None:
                raise UnsupportedSamplerConfig("StableDiffusion.start: ip_image= needs a CLIP vision tower -- attach_clip_vision(ClipVision.load(FILE)) first, "
                                               "or compute the image embeddings elsewhere and pass ip_image_embeds=")
            self._check_tower_fits(tower, ad, "start")
            if dtag(tower.dtype) != dtag(_step_dtype()):
                raise ValueError("StableDiffusion.start: the CLIP vision tower's weights and the step hold different 16-bit types (load both under one config.dtype)")
            s = tower.cfg.image
            rule = f"StableDiffusion.start: ip_image must be uint8 {(b, s, s, 3)} (or one image for all) for the compiled latent and the attached tower"
            return inputs.u8_image(ip_image, rule, (s, s), (1, b))[0], inputs.ip_scales(ip_scale, len(ad.paths))
        if ip_image_embeds is None:
            raise ValueError("StableDiffusion.start: a model compiled with ip_adapter=True reads its image prompt at every step -- pass ip_image_embeds= or ip_image=")
        return inputs.ip_embeds(ip_image_embeds, b, ad.embed_dim), inputs.ip_scales(ip_scale, len(ad.paths))

    def _write_ip_scales(self, scales):
        for q in range(len(scales) // 4):                                # stream-ordered: the values travel as kernel arguments
            hip.tf_set_step_params(self._ip_scales.ptr + 16 * q, *(float(v) for v in scales[4 * q:4 * q + 4]), _sh())

    def _write_ip(self, embeds, scales):
        """The scales and the image tokens' K|V of every guidance group, on the sampler stream behind every step already queued: [tokens(0) |
        tokens(embeds)] for the CFG pair, tokens(embeds) alone for cfg=False.  ``embeds``: the checked fp32 host (B, E) array, or the checked uint8
        image batch (B | 1, S, S, 3), host or device, which the attached tower turns into the embeddings here."""
        if isinstance(embeds, DeviceArray):
            hip.tf_stream_sync(_sh())                                  # (made on the caller's stream)
        self.synchronize()
        ad, b = self._ip_model_compiled, self._latent.shape[0]
        with use_stream(self._stream):
            self._write_ip_scales(scales)
            if embeds.dtype == np.uint8:
                dev = self._ip_rows_from_images(embeds, b, ad.embed_dim)
            else:
                cg = self._cond_groups()
                dev = DeviceArray.from_numpy(np.concatenate([np.zeros_like(embeds)] * (self._groups - cg) + [embeds] * cg), _step_dtype(), "row")
            tokens = ad.tokens(dev)
            kv = ad.context_kv(tokens)
            assert kv.shape == self._ip_kv.shape and kv.dtype == self._ip_kv.dtype, (kv.shape, self._ip_kv.shape)
            hip.tf_memcpy_async(self._ip_kv.ptr, kv.ptr, kv.nbytes, 3, _sh())
            self._ip_keep = (dev, tokens, kv)                            # (referenced until the kernels have run)

    def _ip_rows_from_images(self, images, b, e):
        """(G B, E) device rows [0 | tower(images)] (the tower's rows alone for cfg=False): a memset and a copy.  One image for every latent is
        copied B times in front of the tower, so it runs the very launches B copies handed in by the caller run -- the GEMMs pick their tiles by the
        row count, and the result must not depend on who made the copies (the tower streams its weights once per call whatever the batch)."""
        if images.shape[0] != b:
            if isinstance(images, DeviceArray):
                one, images = images, DeviceArray.empty((b,) + images.shape[1:], np.uint8, "row")
                for k in range(b):
                    hip.tf_memcpy_async(images.ptr + k * one.nbytes, one.ptr, one.nbytes, 3, _sh())
            else:
                images = np.ascontiguousarray(np.repeat(images, b, axis=0))
        emb = self._clip_vision(images)
        per = e * emb.dtype.itemsize
        dev = DeviceArray.empty((self._groups * b, e), emb.dtype, "row")
        lead = (self._groups - self._cond_groups()) * b
        if lead:
            hip.tf_memset_async(dev.ptr, 0, lead * per, _sh())
        for g in range(self._cond_groups()):                               # (pag=True: the perturbed group reads the image prompt too)
            hip.tf_memcpy_async(dev.ptr + (lead + g * b) * per, emb.ptr, b * per, 3, _sh())
        self._ip_tower_keep = (images, emb)
        return dev

    def set_ip_scale(self, ip_scale):
        """The adapter's strength -- one float or one per cross-attention -- from the next step on: the captured step reads the values from the
        device, so nothing is captured again."""
        self._require_sampler("set_ip_scale")
        if not self._ip:
            raise ValueError("StableDiffusion.set_ip_scale: needs a model compiled with ip_adapter=True")
        scales = inputs.ip_scales(ip_scale, len(self._ip_model_compiled.paths), "set_ip_scale")
        with use_stream(self._stream, ordered=False):
            self._write_ip_scales(scales)

    def _check_control(self, control_image, control_hint, control_scale):
        """start()'s ControlNet arguments, checked against the compiled model before anything changes: None for a model without control=True, else
        (device or host uint8 image or None, host float hint or None, the 16 fp32 scale words)."""
        if not self._control:
            if any(v is not None for v in (control_image, control_hint, control_scale)):
                raise ValueError("StableDiffusion.start: control_image=, control_hint= and control_scale= need a model compiled with control=True")
            return None
        if control_image is None and control_hint is None:
            raise ValueError("StableDiffusion.start: a model compiled with control=True reads its hint at every step -- pass control_image= or control_hint=")
        if control_image is not None and control_hint is not None:
            raise ValueError("StableDiffusion.start: pass control_image= or control_hint=, not both")
        b, _, h, w = self._latent.shape
        scales = inputs.control_scales(control_scale, len(self.control_model.input_blocks) + 1)
        if control_image is not None:
            rule = f"StableDiffusion.start: control_image must be uint8 {(b, 8 * h, 8 * w, 3)} (or one image for all) for the compiled latent"
            return inputs.u8_image(control_image, rule, (8 * h, 8 * w), (1, b))[0], None, scales
        if isinstance(control_hint, DeviceArray):
            raise TypeError("StableDiffusion.start: control_hint= takes a host array (a device image goes through control_image=)")
        hint = np.ascontiguousarray(control_hint, dtype=np.float32)
        if hint.ndim != 4 or hint.shape[0] not in (1, b) or hint.shape[1:] != (3, 8 * h, 8 * w):
            raise ValueError(f"StableDiffusion.start: control_hint must be float {(b, 3, 8 * h, 8 * w)} (or one hint for all) for the compiled latent, got {hint.shape}")
        if not (np.isfinite(hint).all() and (hint >= 0).all() and (hint <= 1).all()):
            raise ValueError("StableDiffusion.start: control_hint values must lie in [0, 1]")
        return None, hint, scales

    def _write_control(self, image, hint, scales):
        """Fill the scales and the hint embedding of every guidance group on the sampler stream, behind every step already queued."""
        if isinstance(image, DeviceArray):
            hip.tf_stream_sync(_sh())                                  # (made on the caller's stream)
        self.synchronize()
        b, _, h, w = self._latent.shape
        dt = self._hint_emb.dtype
        with use_stream(self._stream):
            for q in range(4):                                           # stream-ordered: the values travel as kernel arguments
                hip.tf_set_step_params(self._control_scales.ptr + 16 * q, *(float(v) for v in scales[4 * q:4 * q + 4]), _sh())
            if image is not None:
                dev = image if isinstance(image, DeviceArray) else DeviceArray.from_numpy(image, np.uint8, "row")
                x = DeviceArray.empty((dev.shape[0], 3, 8 * h, 8 * w), dt, "nhwc")     # NHWC: the (B,H,W,3) element order of the uint8 image
                hip.tf_hint_from_u8_16(dtag(dt), x.ptr, dev.ptr, x.size, _sh())
            else:
                dev, x = None, DeviceArray.from_numpy(hint, dt, "nhwc")
            emb = self.control_model.hint_embedding(x)
            per = emb.nbytes // emb.shape[0]
            assert emb.shape[1:] == self._hint_emb.shape[1:], (emb.shape, self._hint_emb.shape)
            for g in range(self._groups):
                if emb.shape[0] == b:
                    hip.tf_memcpy_async(self._hint_emb.ptr + g * b * per, emb.ptr, b * per, 3, _sh())
                else:                                                    # one hint for every image
                    for k in range(b):
                        hip.tf_memcpy_async(self._hint_emb.ptr + (g * b + k) * per, emb.ptr, per, 3, _sh())
            self._control_keep = (dev, x, emb)                           # (referenced until the kernels have run)

    def _check_latent(self, seed, noise, image_offset, init_image, init_latent, mask):
        """start()'s latent arguments -- text-to-image, image-to-image, the latent-blend inpainting buffers -- checked against the compiled model
        before anything changes: (seed words, image offset, host noise or None, checked init_image or None, x0 as a device or fp32 host array or
        None, the inpainting mask as a device or fp32 host array or None)."""
        init = init_image if init_image is not None else init_latent
        if init_image is not None and init_latent is not None:
            raise ValueError("StableDiffusion.start: pass init_image= or init_latent=, not both")
        if init is not None and (noise is not None or seed is None):
            raise ValueError("StableDiffusion.start: an image-to-image start takes its noise from seed= (and no noise= array)")
        if seed is None and noise is None:
            raise ValueError("StableDiffusion.start: pass seed= (device noise) or noise= (a host array)")
        if int(image_offset) < 0:
            raise ValueError(f"StableDiffusion.start: image_offset must be >= 0, got {image_offset}")
        if mask is not None and not self._inpaint:
            raise ValueError("StableDiffusion.start: mask= needs a model compiled with inpaint=True")
        if self._inpaint and init is None:
            raise ValueError("StableDiffusion.start: an inpainting model starts from init_image= or init_latent=")
        shape = self._latent.shape
        if noise is not None:
            noise = np.asarray(noise)
            if noise.shape != shape:
                raise ValueError(f"StableDiffusion.start: noise must have the latent's shape {shape}, got {noise.shape}")
        if init_image is not None:
            init_image = self._check_encodable(init_image, "init_image")
        elif init_latent is not None:
            init_latent = inputs.fp32_nchw(init_latent, shape, "init_latent")
        if self._inpaint:
            if mask is None:
                mask = np.ones(self._mask.shape, np.float32)
            else:        # a device fp32 (B,1,h,w) array as it is; anything else through latent_mask
                mask = inputs.fp32_nchw(mask if isinstance(mask, DeviceArray) else self.latent_mask(mask), self._mask.shape, "mask (at latent size)")
        return _seed_words(0 if seed is None else seed), int(image_offset), noise, init_image, init_latent, mask

    def _check_encodable(self, image, name):
        """start()'s images that go through the VAE encoder: uint8, host or device, of the compiled latent's batch and 8x its size, on a model whose
        encoder holds weights and can take that size.  -> the image (host: contiguous)."""
        b, _, h, w = self._latent.shape
        rule = f"StableDiffusion.start: {name} must be uint8 {(b, 8 * h, 8 * w, 3)} for the compiled latent"
        image, _ = inputs.u8_image(image, rule, (8 * h, 8 * w), (b,))
        self._encoder_side("start")
        why = self.encoder_size_error(8 * h, 8 * w)
        if why:
            raise ValueError(f"StableDiffusion.start: {name}: {why}")
        return image

    def _write_latent(self, seed, image_offset, noise, init_image, x0, mask):
        """Rewind the schedule and set the latent (and the inpainting buffers) on the sampler stream, behind every step already queued."""
        self._seed, self._image_offset, self._cursor = seed, image_offset, 0
        self._needs_start = False
        b = self._latent.shape[0]
        if init_image is None and x0 is None:
            if noise is not None:
                self.set_latent(noise)
                return
            self.synchronize()
            with use_stream(self._stream):
                hip.tf_randn_f32(self._latent.ptr, b, self._latent.size // b, seed[0], seed[1], image_offset, 0, 0, _sh())
            return
        for made_by_caller in (mask, x0):
            if isinstance(made_by_caller, DeviceArray):
                hip.tf_stream_sync(_sh())                              # (made on the caller's stream)
        self.synchronize()
        with use_stream(self._stream):
            if init_image is not None:
                x0 = self.encode_image(init_image)
            elif not isinstance(x0, DeviceArray):
                x0 = DeviceArray.from_numpy(x0, np.float32, "row")
            if self._inpaint:
                hip.tf_memcpy_async(self._x0_init.ptr, x0.ptr, x0.nbytes, 3, _sh())
                if isinstance(mask, DeviceArray):
                    hip.tf_memcpy_async(self._mask.ptr, mask.ptr, mask.nbytes, 3, _sh())
                else:
                    self._mask.copy_from_numpy(mask)
            hip.tf_noise_to_level_f32(self._latent.ptr, x0.ptr, b, self._latent.size // b, float(self._sched.alphas[0]), seed[0], seed[1], image_offset, _sh())
            self._start_keep = x0                                       # (referenced until the kernels have run)

    def _check_cond(self, cond_image, cond_mask, cond_latent, image_guidance):
        """start()'s conditioning arguments, checked against the compiled model before anything changes: None for a model without concat=, else
        (image or None, uint8 image-size mask or None, latent mask or None, cond_latent or None, g_I or None), host arrays converted."""
        concat = self._concat
        if concat is None:
            if any(v is not None for v in (cond_image, cond_mask, cond_latent, image_guidance)):
                raise ValueError("StableDiffusion.start: cond_image=, cond_mask=, cond_latent= and image_guidance= need a model compiled with concat=")
            return None
        if cond_image is None and cond_latent is None:
            raise ValueError(f"StableDiffusion.start: a model compiled with concat={concat!r} reads its conditioning channels at every step -- pass "
                             "cond_image=" + (" and cond_mask=" if concat == "inpaint" else "") + ", or cond_latent=")
        if cond_image is not None and cond_latent is not None:
            raise ValueError("StableDiffusion.start: pass cond_image= or cond_latent=, not both")
        if image_guidance is not None:
            if concat != "edit":
                raise ValueError("StableDiffusion.start: image_guidance= belongs to a model compiled with concat='edit'")
            image_guidance = float(image_guidance)
            if not np.isfinite(image_guidance):
                raise ValueError(f"StableDiffusion.start: image_guidance={image_guidance}")
        if cond_mask is not None and (concat != "inpaint" or cond_image is None):
            raise ValueError("StableDiffusion.start: cond_mask= goes with cond_image= on a model compiled with concat='inpaint' (a cond_latent carries its mask channel)")
        if cond_latent is not None:
            return None, None, None, inputs.fp32_nchw(cond_latent, self._cond.shape, "cond_latent"), image_guidance
        self._encoder_side("start")                # (a model without an encoder says so before the image is looked at)
        cond_image = self._check_encodable(cond_image, "cond_image")
        m8 = lat_mask = None
        if concat == "inpaint":
            if cond_mask is None:
                raise ValueError("StableDiffusion.start: an inpainting checkpoint's cond_image= needs cond_mask= (the region to repaint)")
            m8 = self.concat_mask_u8(cond_mask)
            if m8.shape != cond_image.shape[:3]:
                raise ValueError(f"StableDiffusion.start: cond_mask is {m8.shape}, the cond_image needs {tuple(cond_image.shape[:3])}")
            lat_mask = self.concat_mask(m8)
        return cond_image, m8, lat_mask, None, image_guidance

    def _write_cond(self, image, m8, lat_mask, cond_latent, image_guidance):
        """Fill the conditioning buffer (and g_I) on the sampler stream, behind every step already queued."""
        if isinstance(image, DeviceArray) or isinstance(cond_latent, DeviceArray):
            hip.tf_stream_sync(_sh())                                  # (made on the caller's stream)
        self.synchronize()
        b, cc, h, w = self._cond.shape
        with use_stream(self._stream):
            if image_guidance is not None:
                hip.tf_set_step_params(self._edit.ptr, image_guidance, 0.0, 0.0, 0.0, _sh())
            if isinstance(cond_latent, DeviceArray):
                hip.tf_memcpy_async(self._cond.ptr, cond_latent.ptr, cond_latent.nbytes, 3, _sh())
                self._cond_keep = cond_latent
                return
            if cond_latent is not None:
                self._cond.copy_from_numpy(cond_latent)
                return
            if m8 is None:                                                   # edit: the unscaled mode of the posterior
                means, self._cond_keep = self._encode_u8(self.first_stage_model, image)
                hip.tf_means_to_cond_f32(self._cond.ptr, means.ptr, b, h, w, 1.0, 0, cc, _sh())
                return
            dlm = DeviceArray.from_numpy(lat_mask, np.float32, "row")
            means, keep = self._encode_u8(self.first_stage_model, image, m8)
            hip.tf_memcpy_2d_async(self._cond.ptr, cc * h * w * 4, dlm.ptr, h * w * 4, h * w * 4, b, _sh())     # channel 0: the latent mask
            hip.tf_means_to_cond_f32(self._cond.ptr, means.ptr, b, h, w, self.latent_scale, 1, cc, _sh())
            self._cond_keep = keep + (dlm,)                                  # (referenced until the kernels have run)

    def _guidance(self, guidance, what):
        """The guidance scale of ``run`` / ``step_sampler`` as a float; a model compiled with cfg=False takes None or 1.0 only."""
        if self._cfg:
            if guidance is None:
                raise TypeError(f"StableDiffusion.{what}: a model compiled with cfg=True needs its guidance scale")
            return float(guidance)
        if guidance is not None and float(guidance) != 1.0:
            raise ValueError(f"StableDiffusion.{what}: this model was compiled with cfg=False and has no guidance branch -- guidance is None or 1.0, got {guidance}")
        return 1.0

    def step_sampler(self, i, guidance=None, eager=False):
        """Step i of the compiled schedule (asynchronous, on the sampler stream): one parameter launch (timestep scalars, schedule row, seed and
        -- hoisted -- the cached time-embedding row) and one graph replay, the same launches as ``step``.  ``guidance``: the CFG scale; a model
        compiled with cfg=False takes None or 1.0."""
        sched = self._require_sampler("step_sampler")
        guidance = self._guidance(guidance, "step_sampler")
        self._require_started("step_sampler")
        n = len(sched.timesteps)
        i = int(i)
        if not 0 <= i < n:
            raise IndexError(f"StableDiffusion.step_sampler: step {i} outside the schedule's {n} steps")
        t = sched.timesteps[i]
        word, edit = (guidance, None) if not self._pag else inputs.pag_guidance_words(guidance, inputs.pag_scale_at(*self._pag_scale, t), self._cfg)

        def set_params(dst, src, nbytes):
            if edit is not None and edit != self._pag_edit_g:            # pag=True with CFG: g_I = g, written when the CFG scale changes, not per step
                hip.tf_set_step_params(self._edit.ptr, edit, 0.0, 0.0, 0.0, _sh())
                self._pag_edit_g = edit
            hip.tf_set_sampler_params(self._params.dev.ptr, float(t), float(sched.alphas[i]), float(sched.alphas_prev[i]), word, i, self._seed[0], self._seed[1],
                                      self._image_offset, dst, src, nbytes, _sh())
        self._advance(t, eager, set_params)
        self._cursor = i + 1

    def run(self, guidance=None, eager=False):
        """Every remaining step of the schedule (all of them after ``start``); returns the latent (asynchronous: synchronize() to read it)."""
        sched = self._require_sampler("run")
        guidance = self._guidance(guidance, "run")
        self._require_started("run")
        for i in range(self._cursor, len(sched.timesteps)):
            self.step_sampler(i, guidance, eager=eager)
        return self._latent

    def _emb_row(self, t, key=None):
        """The cached time-embedding row of timestep t (keyed by the weights it was computed from; at most 1024 rows are kept)."""
        key = self._weights_key() if key is None else key
        if self._emb_key != key:
            self._emb_rows, self._emb_key = {}, key
            if self._adm:                    # a weight was replaced since start(): label_emb(y) and the schedule's rows again, from the kept y
                self._refresh_y_emb()
                self._build_adm_table()
        row = self._emb_rows.get(t)
        if row is None:
            if len(self._emb_rows) >= 1024:
                self._emb_rows.clear()
            tmp = StepParams().set(t)
            row = self._emb_rows[t] = self._time_row(tmp)
            row._base = (row._base, tmp)
        return row

    def _weights_key(self):
        """weights_key() of everything the hoisted tables were computed from: the UNet and, in a controlled model, the ControlNet."""
        key = self.model.diffusion_model.weights_key()
        if self._adm:
            key = key + (("adm", self._adm_serial),)     # the conditioning serial: start(pooled=) makes every cached row stale
        return key + self.control_model.weights_key() if self._control else key

    def _time_row(self, params):
        """The hoisted time-embedding row of one timestep: the UNet's, and behind it in the same buffer a controlled model's ControlNet's -- one
        copy in the parameter launch hands both to the replay."""
        row = self.model.diffusion_model.time_embedding_all(params, self._y_emb if self._adm else None)[1]
        if not self._control:
            return row
        crow = self.control_model.time_embedding_all(params)[1]
        both = DeviceArray.empty((1, row.shape[1] + crow.shape[1]), row.dtype, "row")
        hip.tf_memcpy_async(both.ptr, row.ptr, row.nbytes, 3, _sh())
        hip.tf_memcpy_async(both.ptr + row.nbytes, crow.ptr, crow.nbytes, 3, _sh())
        both._base = (row, crow)
        return both

    def _refresh_kv(self):
        """Recompute the hoisted K|V projections of the stacked context into the buffers the captured step reads; returns what must stay referenced
        until the copies have run."""
        kv = self._context_kv()
        hip.tf_memcpy_async(self._kv_all.ptr, kv.ptr, kv.nbytes, 3, _sh())
        ckv = None
        if self._ckv_all is not None:
            ckv = self.control_model.context_kv(self._ctx2)
            hip.tf_memcpy_async(self._ckv_all.ptr, ckv.ptr, ckv.nbytes, 3, _sh())
        return kv, ckv

    def set_context(self, unconditional_context, context):
        """New prompts for the compiled step: refresh the stacked context in place (the captured graph reads these buffers) and the
        cross-attention K|V projection that was hoisted out of the step.  Ordered on the sampler stream.  A model compiled with cfg=False reads
        ``context`` alone: ``unconditional_context`` may be None."""
        self._require_compiled("set_context")
        with use_stream(self._stream):
            new = self._frame_context(self._stack_context(unconditional_context, context, self._groups, self._cond_groups()))       # (in the step's 16-bit type)
            assert new.nbytes == self._ctx2.nbytes, "set_context: the contexts must have the shape the step was compiled for"
            hip.tf_memcpy_async(self._ctx2.ptr, new.ptr, new.nbytes, 3, _sh())
            self._ctx_tmp = new                                    # (referenced until the copy has run)
            if self._kv_all is not None:
                self._kv_tmp, self._kv_key = self._refresh_kv(), self._weights_key()   # (referenced until the copies have run)
        self._unc, self._ctx = unconditional_context, context

    def synchronize(self):
        self._require_compiled("synchronize")
        self._stream.synchronize()

    # -- LoRA adapters (storage/lora.py) ---------------------------------------------------------------------------------------------------------
    def load_lora(self, src, name=None, strict=True):
        """Read a LoRA adapter -- a path (.safetensors, torch-zip .ckpt / .pt) or a dict of arrays, kohya or PEFT / diffusers keys (storage/lora.py) --
        check every tensor against this model's targets (ValueError naming the key; nothing is uploaded before all of it passed) and upload its
        operands in the step's 16-bit type (config.is_bf16(); an fp32 file is ROUNDED to it).  Nothing is merged yet: ``set_adapters`` does that.
        ``name``: the adapter's name (default: the file's base name, or "lora<n>").  Keys that match no target raise, or with strict=False print
        ``skipped: <key>``; a model without a text encoder has no ``lora_te_*`` targets.  Returns the name."""
        import os
        from ..storage import lora as L
        if self.model.diffusion_model.cfg.adm_in_channels:
            raise UnsupportedSamplerConfig("StableDiffusion.load_lora: LoRA adapters on an SDXL model are not supported (their targets name two text towers and "
                                           "transformers of depth 2 and 10; nothing is loaded)")
        reg = self._lora if self._lora is not None else L.LoraRegistry()
        if name is None:
            name = os.path.splitext(os.path.basename(str(src)))[0] if not isinstance(src, dict) else f"lora{len(reg.loaded)}"
        if name in reg.loaded:
            raise ValueError(f"StableDiffusion.load_lora: an adapter named {name!r} is loaded already (unload_lora it first, or pass name=)")
        mods, other = L.parse_lora(src)
        shapes = {k: L.weight_shape(m) for k, m in L.lora_targets(self).items()}
        weights = L.check_lora(mods, other, shapes, strict=strict, bf16=config.is_bf16(), has_text_encoder=hasattr(self.cond_stage_model, "transformer"))
        reg.loaded[name] = L.upload(weights, config.is_bf16())
        self._lora = reg
        return name

    def set_adapters(self, names, weights=1.0, text_encoder_weights=None):
        """Activate the loaded adapters ``names`` (a list; empty: none) at ``weights`` (one float, or one per name; ``text_encoder_weights`` likewise for
        the ``lora_te_*`` targets, default: the UNet weight).  Every module an adapter with a non-zero weight touches gets a fresh weight
        W' = round16(W + sum_i s_i up_i down_i), s_i = weight_i alpha_i / rank_i (float64, rounded to fp32 once), by one tf_lora_merge_16 launch from
        the kept BASE weight -- at most 8 adapters per module; a module no active adapter touches gets its base handle, the same object, back:
        ``set_adapters([])`` restores the model bit for bit.  A weight installed by update_state in between becomes the new base.

        A compiled model captures its step again: the sampler stream is drained and ``compile`` -- which destroys the old graph before it captures the
        new one -- is called with the arguments it was given, before any replaced buffer is released.  The previous ``start``'s state (latent, mask, conditioning, hint, cursor) does not
        survive: ``step_sampler`` / ``run`` / ``step`` raise UnsupportedSamplerConfig until ``start`` (or ``set_latent``, for the DDIM ``step``)
        has been called again.  A model that was never compiled only swaps handles.  Contexts encoded before a text-encoder adapter changed are
        not re-encoded: encode the prompts again and hand them to ``set_context``."""
        from ..storage import lora as L
        if isinstance(names, str):
            raise TypeError("StableDiffusion.set_adapters: names is a list of adapter names")
        reg = self._lora if self._lora is not None else L.LoraRegistry()
        plan, active = L.plan_adapters(reg.loaded, names, weights, text_encoder_weights)
        compiled = self._graph is not None and self._compile_args is not None
        if compiled:
            self.synchronize()
        hip.tf_stream_sync(_sh())
        changed, retired = reg.apply(plan, L.lora_targets(self), L.merge_device)
        reg.active = active
        self._lora = reg
        if changed:
            hip.tf_stream_sync(_sh())                                    # the merges have run: the adapters' and the retired buffers may go
            if compiled:
                # compile destroys the previous graph itself, behind its warm-up steps: the arrays the old capture left referenced (_keep) are
                # let go while the graph still owns their blocks, and only then do the blocks go back to the pool -- once
                self.compile(stream=self._stream, **self._compile_args)
                self._needs_start = True
        del retired
        return self

    def adapters(self):
        """{name: (weight, text_encoder_weight)} of the adapters now merged in (set_adapters' order)."""
        return dict(self._lora.active) if self._lora is not None else {}

    def unload_lora(self, name):
        """Forget a loaded adapter and release its device buffers; an adapter that is active (``adapters()``) is refused -- set_adapters without it first."""
        reg = self._lora
        if reg is None or name not in reg.loaded:
            raise ValueError(f"StableDiffusion.unload_lora: unknown adapter {name!r}")
        if name in reg.active:
            raise ValueError(f"StableDiffusion.unload_lora: {name!r} is active -- set_adapters([...]) without it first")
        del reg.loaded[name]
