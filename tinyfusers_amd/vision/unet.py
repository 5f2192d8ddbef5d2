"""UNetModel / Upsample / Downsample / timestep_embedding -- mirrors tinyfusers/vision/unet.py:9-97.

Same module tree and attribute names as the reference (they are the LDM checkpoint keys that update_state
walks), generated from a channel plan so that a down-scaled graph can be built for tests; the default plan
is exactly the SD-1.x one hard-coded in vision/unet.py:12-49.

Step-level batching that the reference does not do (results unchanged):
  * the 22 ResBlock ``emb_layers`` Linear(SiLU(emb)) run as ONE weight-streaming GEMV over a device-side
    concatenated weight at the top of the step;
  * the 32 cross-attention to_k / to_v projections of the context run as ONE GEMM (N = sum 2C) -- every
    layer then reads its K|V column slice through SDPA strides;
  * the channel concat of :72 is never materialised (GroupNorm / conv read both tensors), the nearest-2x
    upsample of :81-83 is folded into the following conv's gather.

The encoder half (block plan, batched projections, the walk over input_blocks and middle_block) lives in ``encoder_plan`` / ``StepModel``: a
ControlNet (vision/controlnet.py) is a second copy of it, and ``UNetModel.__call__(control=...)`` takes its residuals in (``control_add``).
``UNetModel.__call__(freeu=...)`` is FreeU in front of the concats of the first two decoder stages (``freeu_stages``, ``freeu_skips``,
``freeu_backbone``).  ``UNetModel.__call__(pag=...)`` is perturbed-attention guidance: one batch range of every selected SpatialTransformer's
self-attention takes the identity (``pag_layers``; attention/sdpa.py::sdpa_pag_strided).  ``UNetModel.__call__(motion=(adapter, F))`` runs AnimateDiff
motion modules (vision/motion.py) at their slots of the walk (``_with_motion``).
"""
import ctypes
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import numpy as np

from ..attention.attention import SpatialTransformer, _concat_rows
from ..ff.group_norm import GroupNorm
from ..ff.linear import Linear, RowSlice, gemv_f16, gemv_rows, linear_f16
from ..native import ControlEntry, FreeuEntry, hip
from .. import config
from ..storage.tensor import Branch, DeviceArray, Tensor, _sh, asarray, bfloat16, dtag, is_bfloat16
from .conv2d import Conv2d
from .motion import MotionModule
from .resnet import ResBlock


@dataclass(frozen=True)
class UNetConfig:
    in_channels: int = 4
    out_channels: int = 4
    model_channels: int = 320
    channel_mult: Tuple[int, ...] = (1, 2, 4, 4)
    num_res_blocks: int = 2
    attention_levels: Tuple[int, ...] = (0, 1, 2)
    n_heads: int = 8
    context_dim: int = 768
    d_head: Optional[int] = None      # SD-2.x: a fixed head size, the head count follows the channels (``heads_at``); n_heads is then unused
    transformer_depth: Optional[Tuple[int, ...]] = None      # SDXL: BasicTransformerBlocks per SpatialTransformer, one entry per level (0: none there); None: 1 on attention_levels (``depth_at``)
    adm_in_channels: Optional[int] = None                    # SDXL: the width of the vector conditioning y; emb = time_embed(t) + label_emb(y)
    adm_time_dim: int = 256                                  # SDXL: the Fourier width of each of the six size ids inside y


SD15 = UNetConfig()
SD15_INPAINT = replace(SD15, in_channels=9)   # sd-v1-5-inpainting: [latent(4) | mask(1) | latent of the masked image(4)]
SD15_EDIT = replace(SD15, in_channels=8)      # InstructPix2Pix: [latent(4) | latent of the image to edit(4)]
TINY = UNetConfig(model_channels=64, channel_mult=(1, 2, 2), attention_levels=(0, 1), n_heads=2, context_dim=64)
SD21 = replace(SD15, d_head=64, context_dim=1024)     # Stable Diffusion 2.0 / 2.1 (512-base, 768-v): 5 / 10 / 20 / 20 heads of 64, OpenCLIP ViT-H context
SD21_INPAINT = replace(SD21, in_channels=9)           # 512-inpainting-ema: SD15_INPAINT's channels
TINY_V2 = UNetConfig(model_channels=64, channel_mult=(1, 2, 2), attention_levels=(0, 1), d_head=64, context_dim=128)     # 1 / 2 / 2 heads of 64
# SDXL base: three levels with 0 / 2 / 10 transformer blocks (10 in the middle block), 5 / 10 / 20 heads of 64, the 2048-wide context of two text
# towers, y = [pooled (1280) | Fourier(original h, w, crop top, left, target h, w) (6 x 256)]
SDXL = UNetConfig(channel_mult=(1, 2, 4), transformer_depth=(0, 2, 10), d_head=64, context_dim=2048, adm_in_channels=2816)
TINY_XL = UNetConfig(model_channels=64, channel_mult=(1, 2, 2), transformer_depth=(0, 1, 2), d_head=64, context_dim=128, adm_in_channels=64 + 6 * 32, adm_time_dim=32)


def heads_at(cfg, ch):
    """(head count, head size) of a SpatialTransformer at ``ch`` channels: cfg.n_heads heads of ch // n_heads (SD-1.x), or -- cfg.d_head set --
    ch // d_head heads of d_head (SD-2.x).  The one place the encoder plan, the decoder half and the compile checks take them from."""
    if cfg.d_head is None:
        return cfg.n_heads, ch // cfg.n_heads
    if cfg.d_head <= 0 or ch % cfg.d_head:
        raise ValueError(f"UNetConfig: d_head={cfg.d_head} does not divide the {ch} channels of a SpatialTransformer")
    return ch // cfg.d_head, cfg.d_head


def depth_at(cfg, lev):
    """BasicTransformerBlocks of a SpatialTransformer at level ``lev`` (0: the level has none); lev = "mid": of the middle block's.  The one place
    the plan is read from: cfg.transformer_depth where set (the middle block takes the last level's), else 1 on cfg.attention_levels and in the
    middle block -- the SD-1.x / SD-2.x plan."""
    td = cfg.transformer_depth
    if td is None:
        return 1 if lev == "mid" or lev in cfg.attention_levels else 0
    if len(td) != len(cfg.channel_mult) or min(td) < 0 or td[-1] < 1:
        raise ValueError(f"UNetConfig: transformer_depth={td} needs one entry >= 0 per level of channel_mult={cfg.channel_mult}, the last >= 1 (the middle block's)")
    return td[-1] if lev == "mid" else td[lev]


def head_sizes(cfg):
    """The head sizes of the UNet's SpatialTransformers, one per attention level, from the channel plan alone."""
    return sorted({heads_at(cfg, cfg.model_channels * cfg.channel_mult[lev])[1] for lev in range(len(cfg.channel_mult)) if depth_at(cfg, lev)}
                  | {heads_at(cfg, cfg.model_channels * cfg.channel_mult[-1])[1]})


class Upsample:
    def __init__(self, channels, init=True):
        self.conv = Conv2d(channels, channels, kernel_size=[3, 3], padding=[1, 1], init=init)

    def __call__(self, x, out_gn=0, out_norm=None):
        return self.conv(x, upsample=True, gn=out_gn, out_norm=out_norm)       # nearest-2x (unet.py:81-83) folded into the conv gather


class Downsample:
    def __init__(self, channels, init=True):
        self.op = Conv2d(channels, channels, stride=[2, 2], kernel_size=[3, 3], padding=[1, 1], init=init)

    def __call__(self, x, out_gn=0, out_norm=None):
        return self.op(x, gn=out_gn, out_norm=out_norm)


class StepParams:
    """Device-resident per-step scalars [timestep, a_t, a_prev, guidance] (fp32).  ``set`` is a 1-thread kernel
    whose arguments carry the values, so it is stream-ordered with the step graph that reads them.  ``StepParams(dev)`` wraps an existing
    device array that starts with these four words (a sampler's parameter block, a caller's timestep array) and writes nothing."""

    def __init__(self, dev=None):
        self.dev = dev
        if dev is None:
            self.dev = DeviceArray.empty((4,), np.float32, "row")
            self.set(0.0)

    def set(self, timestep, a_t=1.0, a_prev=1.0, guidance=1.0):
        hip.tf_set_step_params(self.dev.ptr, float(timestep), float(a_t), float(a_prev), float(guidance), _sh())
        return self


def _as_params(timesteps):
    if isinstance(timesteps, StepParams):
        return timesteps
    if isinstance(timesteps, DeviceArray):
        return StepParams(timesteps)
    t = float(np.asarray(timesteps, dtype=np.float32).reshape(-1)[0])
    return StepParams().set(t)


def timestep_embedding(timesteps, dim, max_period=10000):
    """unet.py:92-97: (1, dim) = [cos(t f), sin(t f)].  timesteps: host scalar/array, or StepParams / a device
    fp32 array whose element 0 is the timestep."""
    sp = _as_params(timesteps)
    if config.is_bf16():
        out = DeviceArray.empty((1, dim), bfloat16, "row")
        hip.tf_timestep_embedding_bf16(out.ptr, sp.dev.ptr, dim, float(max_period), _sh())
        out._base = sp
        return out
    out = DeviceArray.empty((1, dim), np.float16, "row")
    hip.tf_timestep_embedding_f16(out.ptr, sp.dev.ptr, dim, float(max_period), _sh())
    out._base = sp
    return out


def encoder_plan(cfg, in_channels, init=False):
    """The encoder half of vision/unet.py:12-37 from the channel plan: (time_embed, input_blocks, middle_block, chans) -- chans[i] = the channel
    count input block i saves for the skip concat.  Built once for the UNet and for a ControlNet (vision/controlnet.py), whose trunk is this."""
    mc, emb = cfg.model_channels, cfg.model_channels * 4
    cd = cfg.context_dim
    R = lambda i, o: ResBlock(i, emb, o, init=init)
    S = lambda c, d: SpatialTransformer(c, cd, *heads_at(cfg, c), init=init, depth=d)
    time_embed = [Linear(mc, emb, init=init), Tensor.silu, Linear(emb, emb, init=init)]
    input_blocks = [[Conv2d(in_channels, mc, kernel_size=[3, 3], padding=[1, 1], init=init)]]
    chans, ch, nlev = [mc], mc, len(cfg.channel_mult)
    for lev, mult in enumerate(cfg.channel_mult):
        for _ in range(cfg.num_res_blocks):
            blk = [R(ch, mc * mult)]
            ch = mc * mult
            if depth_at(cfg, lev):
                blk.append(S(ch, depth_at(cfg, lev)))
            input_blocks.append(blk)
            chans.append(ch)
        if lev != nlev - 1:
            input_blocks.append([Downsample(ch, init=init)])
            chans.append(ch)
    middle_block = [R(ch, ch), S(ch, depth_at(cfg, "mid")), R(ch, ch)]
    return time_embed, input_blocks, middle_block, chans


class StepModel:
    """What the UNet and a ControlNet share: the step-level batched projections (one GEMV for every ResBlock's time-embedding Linear, one GEMM
    for every cross-attention K|V) and the walk over the encoder half.  A subclass has cfg, time_embed, input_blocks, middle_block and, the
    UNet, output_blocks."""

    # -- step-level batched projections (built once per weight set, on the device)
    def _all(self, kind):
        blocks = [bb for b in self.input_blocks for bb in b] + list(self.middle_block) + [bb for b in getattr(self, "output_blocks", ()) for bb in b]
        return [bb for bb in blocks if isinstance(bb, kind)]

    def _prepare(self):
        res, sts = self._all(ResBlock), self._all(SpatialTransformer)
        blocks = [blk for s in sts for blk in s.transformer_blocks]          # every block of every transformer, in execution order
        key = tuple(r.emb_layers[1].weight.wkey for r in res) + tuple(r.emb_layers[1].bias.wkey for r in res) \
            + tuple(w.wkey for blk in blocks for w in (blk.attn2.to_k.weight, blk.attn2.to_v.weight))
        if self._batched is not None and self._batched["key"] == key:
            return self._batched
        emb_w = _concat_rows([r.emb_layers[1].weight for r in res])
        emb_b = _concat_rows([r.emb_layers[1].bias.view((r.emb_layers[1].bias.size, 1)) for r in res]).view((emb_w.shape[0],))
        emb_off, off = {}, 0
        for r in res:
            emb_off[id(r)] = (off, r.emb_layers[1].weight.shape[0]); off += r.emb_layers[1].weight.shape[0]
        kv_w, kv_off, off = None, {}, 0
        if blocks:
            ws = []
            for blk in blocks:                      # kv_off: per block (a transformer of depth d owns d consecutive column slices)
                a = blk.attn2
                ws += [a.to_k.weight, a.to_v.weight]
                kv_off[id(blk)] = off; off += 2 * a.to_k.weight.shape[0]
            kv_w = _concat_rows(ws)
        self._batched = dict(key=key, emb_w=emb_w, emb_b=emb_b, emb_off=emb_off, kv_w=kv_w, kv_off=kv_off, kv_n=off)
        return self._batched

    def time_embedding_all(self, timesteps, y_emb=None):
        """(emb, emb_all): the time-embedding chain of unet.py:54-56 and every ResBlock's Linear(SiLU(emb)) (resnet.py:28) as one row.  Both
        depend on the timestep alone -- not on the latent, the context or the batch -- so a sampler may compute the row of a timestep once
        and keep it (variants/sd.py here: StableDiffusion.compile(timesteps=...)).

        The rule of the row's shape, stated once.  A model WITHOUT ``label_emb`` (SD-1.x, SD-2.x, every ControlNet) has the (1, N) row above; its
        ResBlocks read it through a stride-0 per-image bias (one row for every image), and ``y_emb`` must be None.  A model WITH ``label_emb``
        (cfg.adm_in_channels: SDXL) computes emb = time_embed(t) + label_emb(y), and SiLU sits between that sum and the ResBlock projections, so
        the rows of two images (or of the unconditional and the conditional group) differ: ``y_emb`` = ``label_embedding(y)``, (R, E) with R the
        batch the UNet runs on, is required, emb is (R, E) and emb_all (R, N); ResBlock i reads columns [off_i, off_i + n_i) of image b's row
        through a per-image bias of stride N (ff/linear.py::RowSlice).  Both still depend on nothing but the timestep and y."""
        bt = self._prepare()
        t_emb = timestep_embedding(timesteps, self.cfg.model_channels)
        emb = self.time_embed[2](self.time_embed[0](t_emb), silu_input=True)          # Linear -> SiLU -> Linear
        if getattr(self, "label_emb", None) is None:
            if y_emb is not None:
                raise ValueError("time_embedding_all: y_emb= is for a model with label_emb (UNetConfig.adm_in_channels)")
            return emb, gemv_f16(emb, bt["emb_w"], bt["emb_b"], silu_input=True)      # every ResBlock's Linear(SiLU(emb))
        if y_emb is None:
            raise ValueError("time_embedding_all: a model with label_emb (UNetConfig.adm_in_channels) needs y_emb = label_embedding(y)")
        emb = self.emb_rows(emb, y_emb)                                               # (R, E): row r = emb + y_emb[r]
        return emb, gemv_rows(emb, bt["emb_w"], bt["emb_b"], silu_input=True)

    def label_embedding(self, y):
        """label_emb(y): y (R, adm_in_channels) in the step's 16-bit type -> (R, E), Linear -> SiLU -> Linear."""
        le = getattr(self, "label_emb", None)
        if le is None:
            raise ValueError("label_embedding: this model has no label_emb (UNetConfig.adm_in_channels is None)")
        if y.ndim != 2 or y.shape[1] != le[0][0].in_features:
            raise ValueError(f"label_embedding: y must be (R, {le[0][0].in_features}), got {y.shape}")
        return gemv_rows(gemv_rows(y, le[0][0].weight, le[0][0].bias), le[0][2].weight, le[0][2].bias, silu_input=True)

    @staticmethod
    def emb_rows(t_emb, y_emb):
        """(S R, E): row s R + r = t_emb[s] + y_emb[r] (tf_adm_emb_rows_16: fp32 add, one rounding)."""
        (s, e), r = t_emb.shape, y_emb.shape[0]
        assert y_emb.shape == (r, e) and dtag(y_emb.dtype) == dtag(t_emb.dtype), (t_emb.shape, y_emb.shape)
        out = DeviceArray.empty((s * r, e), t_emb.dtype, "row")
        hip.tf_adm_emb_rows_16(dtag(t_emb.dtype), out.ptr, t_emb.ptr, y_emb.ptr, s, r, e, _sh())
        return out

    def time_embedding_table(self, timesteps, y_emb):
        """(S R, N): ``time_embedding_all``'s emb_all for every timestep of a schedule, rows [s R, (s + 1) R) those of timesteps[s] -- the time MLP
        at M = S, ONE row build and ONE pass of the batched ResBlock projection at M = S R (the projection weight, 35 MB at SDXL, is read once
        per table, not once per timestep).  Every row holds the bits ``time_embedding_all`` gives it (the GEMV computes each row on its own)."""
        bt = self._prepare()
        mc, ts = self.cfg.model_channels, [float(t) for t in timesteps]
        t_sin = DeviceArray.empty((len(ts), mc), bfloat16 if config.is_bf16() else np.float16, "row")
        keep = []
        for i, t in enumerate(ts):
            row = timestep_embedding(t, mc)
            hip.tf_memcpy_async(t_sin.ptr + i * row.nbytes, row.ptr, row.nbytes, 3, _sh())
            keep.append(row)
        t_emb = gemv_rows(gemv_rows(t_sin, self.time_embed[0].weight, self.time_embed[0].bias), self.time_embed[2].weight, self.time_embed[2].bias, silu_input=True)
        out = gemv_rows(self.emb_rows(t_emb, y_emb), bt["emb_w"], bt["emb_b"], silu_input=True)
        out._base = (out._base, keep, t_sin, t_emb)
        return out

    def context_kv(self, context):
        """Every cross-attention's K|V projection of the (stacked) context as ONE GEMM (attention/attention.py:35-36 for all 16 blocks):
        depends on the context alone, so a sampler computes it when the context changes, not once per step."""
        bt = self._prepare()
        return linear_f16(context, bt["kv_w"]) if bt["kv_w"] is not None else None

    def weights_key(self):
        """Identity of everything time_embedding_all / context_kv depend on: a cached row is stale once any of these weights is replaced."""
        mlps = (self.time_embed[0], self.time_embed[2]) + ((self.label_emb[0][0], self.label_emb[0][2]) if getattr(self, "label_emb", None) is not None else ())
        return self._prepare()["key"] + tuple(m.weight.wkey for m in mlps) + tuple(m.bias.wkey for m in mlps)

    def step_shared(self, timesteps, context, y_emb=None):
        """What one denoising step computes ONCE for every sample: the time-embedding chain (the same timestep for the whole batch) and
        the cross-attention K|V projection of all contexts.  __call__ computes them itself unless handed the result (``shared``)."""
        emb, emb_all = self.time_embedding_all(timesteps, y_emb)
        return emb, emb_all, self.context_kv(context)

    def _shared(self, timesteps, context, shared, y_emb=None):
        """(emb, emb_all, kv_all, br) of one call: handed in (``shared``) or computed here; br is the open side branch the K|V projection runs
        on (config.parallel_branches), joined by the first SpatialTransformer."""
        bt = self._prepare()
        if shared is not None:
            return (*shared, None)                     # kv_all: this call's rows (b, tk, kv_n) of the step-level projection; emb may be None (emb_all is what the ResBlocks read)
        br = kv_all = None
        if config.parallel_branches and bt["kv_w"] is not None:
            br = Branch()                              # the context projection is independent of the time-embedding chain
            with br:
                kv_all = linear_f16(context, bt["kv_w"])      # (either element type since round 5)
        emb, emb_all = self.time_embedding_all(timesteps, y_emb)                     # Linear -> SiLU -> Linear, then every ResBlock's Linear(SiLU(emb))
        if br is None:
            kv_all = self.context_kv(context)                                         # every attn2's K|V of the context
        return emb, emb_all, kv_all, br

    def _runner(self, emb, emb_all, kv_all, context, ip=None, pag=None, frames=None):
        bt = self._prepare()
        # frames: F of ``UNetModel.__call__(motion=(adapter, F))`` -- what a MotionModule of the walked sequence is called with
        # pag = (flags, (b0, b1)): the device fp32 array with one word per SpatialTransformer in execution order, and the perturbed batch range
        pag_idx = {id(st): i for i, st in enumerate(self._all(SpatialTransformer))} if pag is not None else None
        # ip = (kv_ip_all (b, T, kv_n), {id(SpatialTransformer): (column offset, scale index)}, kv_n, scales): an IP-Adapter's image-token K|V
        # for every cross-attention and the device fp32 array of their strengths (UNetModel.__call__(ip=))

        def run(x, bb, nxt, force_gn=0, residual=None):
            # nxt = the module that reads this one's output as a single tensor (None across a concat): when it opens
            # with a GroupNorm, the statistics are produced by this module's last conv.  force_gn: the output (also) enters
            # an equal-split concat whose GroupNorm merges the two producers' partials (tf_group_norm_apply2_f16)
            gn = nxt.num_groups if isinstance(nxt, GroupNorm) else 32 if isinstance(nxt, (ResBlock, SpatialTransformer, MotionModule)) else force_gn
            # ... and where that conv runs split-K its reduce applies the norm too: (the GroupNorm module that opens nxt, silu)
            on = (nxt, True) if isinstance(nxt, GroupNorm) else (nxt.in_layers[0], True) if isinstance(nxt, ResBlock) \
                else (nxt.norm, False) if isinstance(nxt, (SpatialTransformer, MotionModule)) else None      # (a motion module opens with GroupNorm(32, eps 1e-6), no SiLU)
            if isinstance(bb, ResBlock):
                off, n = bt["emb_off"][id(bb)]
                if emb_all.shape[0] == 1:                      # one row for every image (time_embedding_all's rule)
                    return bb(x, emb, emb_out=emb_all.view((1, n), "row", off), out_gn=gn, out_norm=on)
                nb = (x[0] if isinstance(x, (tuple, list)) else x).shape[0]
                if emb_all.shape[0] != nb:
                    raise ValueError(f"UNet: {emb_all.shape[0]} time-embedding rows for a batch of {nb} (label_embedding(y) has one row per image)")
                return bb(x, emb, emb_out=RowSlice(emb_all, off, n), out_gn=gn, out_norm=on)
            if isinstance(bb, SpatialTransformer):
                c = bb.proj_in.weight.shape[0]
                bip = None
                if ip is not None:
                    off, idx = ip[1][id(bb)]
                    bip = (KVSlice(ip[0], off, c, ip[2]), ip[3].ptr + 4 * idx)
                bpag = (pag[0].ptr + 4 * pag_idx[id(bb)], pag[1]) if pag is not None else None
                kvs = [KVSlice(kv_all, bt["kv_off"][id(blk)], c, bt["kv_n"]) for blk in bb.transformer_blocks]      # each block its own K|V columns
                return bb(x, context, kv=kvs, out_gn=gn, out_norm=on, ip=bip, pag=bpag)
            if isinstance(bb, MotionModule):
                return bb(x, frames, out_gn=gn, out_norm=on)
            if isinstance(bb, (Downsample, Upsample)):
                return bb(x, out_gn=gn, out_norm=on)
            if isinstance(bb, Conv2d):
                if residual is not None:                       # a ControlNet's conv_in: + the hint embedding, in the conv's epilogue
                    return bb(x, residual=residual, gn=gn, out_norm=on)
                return bb(x, gn=gn, out_norm=on)               # conv_in: its output feeds the first ResBlock's GroupNorm and the last skip concat
            return bb(x)
        return run

    def _encode(self, run, x, br=None, concat_stats=True, residual=None, replaced=0, blocks=None):
        """input_blocks and middle_block over x: (the middle block's output, what every input block saves for the skip concats).  concat_stats:
        the saved tensors and the output enter the output path's concats as they are -- their producers emit the statistics those concats'
        GroupNorms merge (config.concat_stats).  residual: added to the first module's (conv_in's) output.  replaced: the last ``replaced`` saved
        tensors and the output are replaced before their concats read them (FreeU): their producers are not asked for concat statistics.  blocks:
        (input blocks, middle block) to walk in place of the model's own (``UNetModel._with_motion``: the same lists with the motion modules in)."""
        input_blocks, middle_block = (self.input_blocks, self.middle_block) if blocks is None else blocks
        saved_inputs = []
        joined = br is None
        seq = [bb for b in input_blocks for bb in b] + list(middle_block)
        ends = []                                   # indices after which the tensor is also saved for a skip concat
        i = 0
        for b in input_blocks:
            i += len(b)
            ends.append(i - 1)
        kept = set(ends[:len(ends) - replaced]) if replaced else set(ends)
        ends = set(ends)
        for i, bb in enumerate(seq):
            nxt = seq[i + 1] if i + 1 < len(seq) else None     # the middle block's output enters a concat
            if not joined and isinstance(bb, SpatialTransformer):
                br.join(); joined = True            # first consumer of kv_all
            # tensors saved for (or entering) the output path's concat carry 32-group statistics when the concat is an equal split
            want = concat_stats and config.concat_stats and (i in kept or (nxt is None and not replaced)) and x.size <= config.concat_stats_max_elems
            x = run(x, bb, nxt, force_gn=32 if want else 0, residual=residual if i == 0 else None)
            if i in ends:
                saved_inputs.append(x)
        if not joined:
            br.join()
        return x, saved_inputs


def control_add(skips, residuals, scales):
    """The seam of a controlled step: new_i = skip_i + s_i residual_i for every tensor of ``skips`` in ONE launch (tf_control_add_16; s: the
    device fp32 array ``scales``).  The new tensors carry no GroupNorm statistics (.gn) and no normalised twin (.normed): those of the skips
    describe the tensors before the add."""
    if len(residuals) != len(skips) or len(skips) > 16:
        raise ValueError(f"control_add: {len(residuals)} residuals for {len(skips)} skip tensors (at most 16)")
    if scales.dtype != np.float32 or scales.size < len(skips):
        raise ValueError(f"control_add: scales must hold {len(skips)} fp32 values, got {scales}")
    table, outs = (ControlEntry * len(skips))(), []
    for e, k, r in zip(table, skips, residuals):
        if r.shape != k.shape or r.layout != k.layout or dtag(r.dtype) != dtag(k.dtype) or k.dtype.itemsize != 2 or k.size % 8:
            raise ValueError(f"control_add: residual {r} does not match the skip tensor {k} (16-bit, a multiple of 8 elements)")
        o = DeviceArray.empty(k.shape, k.dtype, k.layout)
        e.dst, e.skip, e.residual, e.n = o.ptr, k.ptr, r.ptr, k.size
        o._base = (k, r)                                  # (referenced while the launch is queued)
        outs.append(o)
    hip.tf_control_add_16(dtag(skips[0].dtype), ctypes.cast(table, ctypes.c_void_p), len(skips), scales.ptr, _sh())
    return outs


PAG_WORDS = 16        # the flag array of perturbed-attention guidance: one fp32 word per SpatialTransformer, one 64-byte write


def pag_layers(cfg):
    """The LDM paths of the UNet's SpatialTransformers in execution order -- input blocks, middle block, output blocks: the order of the flag words of
    ``UNetModel.__call__(pag=)``.  SD-1.5: input_blocks 1, 2, 4, 5, 7, 8 (words 0-5), middle_block (6), output_blocks 3 .. 11 (7-15).  From the channel
    plan alone (encoder_plan's and UNetModel's walk), so that the layer names of ``set_pag`` are checked without a model."""
    nlev, paths, i = len(cfg.channel_mult), [], 1
    for lev in range(nlev):
        for _ in range(cfg.num_res_blocks):
            if depth_at(cfg, lev):
                paths.append(f"input_blocks.{i}")
            i += 1
        i += lev != nlev - 1                          # the Downsample block
    paths.append("middle_block")
    i = 0
    for lev in reversed(range(nlev)):
        for _ in range(cfg.num_res_blocks + 1):
            if depth_at(cfg, lev):
                paths.append(f"output_blocks.{i}")
            i += 1
    return paths


def freeu_stages(cfg):
    """FreeU's stage -> block map (diffusers' up_blocks[0] and up_blocks[1]): with n = num_res_blocks + 1, stage k is output_blocks[k n : (k + 1) n].
    -> [(stage, output block, backbone channels, skip channels, latent size divisor)] for the 2n blocks, in block order.  (The authors' LDM code
    keys on the backbone's channel count, 1280 / 640, which names other blocks; this follows diffusers.)"""
    mc, nlev, n = cfg.model_channels, len(cfg.channel_mult), cfg.num_res_blocks + 1
    if nlev < 2:
        raise ValueError(f"freeu_stages: FreeU needs two decoder stages, {cfg} has {nlev}")
    chans = [mc]                                    # what encoder_plan's input blocks save
    for lev, mult in enumerate(cfg.channel_mult):
        chans += [mc * mult] * cfg.num_res_blocks + ([mc * mult] if lev != nlev - 1 else [])
    ch, plan = chans[-1], []
    for k, lev in enumerate((nlev - 1, nlev - 2)):
        for i in range(n):
            plan.append((k, k * n + i, ch, chans.pop(), 2 ** lev))
            ch = mc * cfg.channel_mult[lev]
    return plan


def freeu_skips(skips, stages, scales):
    """new_i = fourier_filter(skip_i, threshold 1, scale s[stage_i]) for every tensor of ``skips`` in ONE launch (tf_freeu_skip_16; s: words 0 and
    1 of the device fp32 array ``scales`` = [s1, s2, b1, b2]).  The new tensors carry no GroupNorm statistics (.gn) and no normalised twin
    (.normed) -- control_add's rule: those of the skips describe the tensors before the filter."""
    if len(skips) != len(stages) or not 1 <= len(skips) <= 8:
        raise ValueError(f"freeu_skips: {len(stages)} stages for {len(skips)} skip tensors (1 to 8)")
    if scales.dtype != np.float32 or scales.size < 4:
        raise ValueError(f"freeu_skips: scales must hold the 4 fp32 values [s1, s2, b1, b2], got {scales}")
    table, outs = (FreeuEntry * len(skips))(), []
    for e, k, st in zip(table, skips, stages):
        if k.layout != "nhwc" or k.dtype.itemsize != 2 or dtag(k.dtype) != dtag(skips[0].dtype) or k.shape[1] % 8 or k.shape[2] < 2 or k.shape[3] < 2:
            raise ValueError(f"freeu_skips: the skip tensor {k} is not 16-bit NHWC with C a multiple of 8, H >= 2 and W >= 2")
        o = DeviceArray.empty(k.shape, k.dtype, k.layout)
        e.dst, e.src, e.scale_index = o.ptr, k.ptr, st
        e.B, e.C, e.H, e.W = k.shape
        o._base = k                                       # (referenced while the launch is queued)
        outs.append(o)
    hip.tf_freeu_skip_16(dtag(skips[0].dtype), ctypes.cast(table, ctypes.c_void_p), len(skips), scales.ptr, _sh())
    return outs


def freeu_backbone(x, stage, scales):
    """x[:, :C/2] *= b[stage] (word 2 + stage of ``scales``), in place: one launch over half the tensor (tf_freeu_backbone_16).  -> a new handle
    on the same memory without .gn / .normed, which describe the tensor before the scaling."""
    n, c, h, w = x.shape
    if x.layout != "nhwc" or x.dtype.itemsize != 2 or c % 16:
        raise ValueError(f"freeu_backbone: the backbone tensor {x} is not 16-bit NHWC with C a multiple of 16")
    hip.tf_freeu_backbone_16(dtag(x.dtype), x.ptr, x.ptr, n * h * w, c, scales.ptr, 2 + stage, _sh())
    return x.view(x.shape, x.layout)


class UNetModel(StepModel):
    def __init__(self, cfg: UNetConfig = SD15, init=False):
        self.cfg = cfg
        mc, emb = cfg.model_channels, cfg.model_channels * 4
        cd = cfg.context_dim
        R = lambda i, o: ResBlock(i, emb, o, init=init)
        S = lambda c, d: SpatialTransformer(c, cd, *heads_at(cfg, c), init=init, depth=d)
        self.time_embed, self.input_blocks, self.middle_block, chans = encoder_plan(cfg, cfg.in_channels, init)
        # SDXL: emb = time_embed(t) + label_emb(y); the tree spells the checkpoint's label_emb.0.0.* / label_emb.0.2.* (None: no such leaves)
        self.label_emb = [[Linear(cfg.adm_in_channels, emb, init=init), Tensor.silu, Linear(emb, emb, init=init)]] if cfg.adm_in_channels else None
        ch, nlev = chans[-1], len(cfg.channel_mult)
        self.output_blocks = []
        for lev in reversed(range(nlev)):
            mult = cfg.channel_mult[lev]
            for i in range(cfg.num_res_blocks + 1):
                blk = [R(ch + chans.pop(), mc * mult)]
                ch = mc * mult
                if depth_at(cfg, lev):
                    blk.append(S(ch, depth_at(cfg, lev)))
                if lev > 0 and i == cfg.num_res_blocks:
                    blk.append(Upsample(ch, init=init))
                self.output_blocks.append(blk)
        self.out = [GroupNorm(32, mc, init=init), Tensor.silu, Conv2d(mc, cfg.out_channels, kernel_size=[3, 3], padding=[1, 1], init=init)]
        self._batched = None

    def ip_slots(self, adapter):
        """{id(SpatialTransformer): (column offset in the adapter's K|V GEMM, index of its scale)} for ``adapter`` (storage/ip_adapter.py)."""
        from ..storage.ip_adapter import adapter_paths
        offs, _ = adapter.kv_layout()
        paths = adapter_paths(self)
        if [(n, p) for n, p, _ in paths] != adapter.paths:
            raise ValueError("UNetModel.ip_slots: the adapter was built for another UNet")
        return {id(st): (offs[k], k) for k, (_, _, st) in enumerate(paths)}

    def _with_motion(self, adapter):
        """(input_blocks, middle_block, output_blocks) with the adapter's modules at their slots -- new lists, the model's own stay as they are: behind
        everything else of an input block, between the middle block's transformer and its second ResBlock, behind the ResBlock / SpatialTransformer
        of an output block and in front of its Upsample."""
        if adapter.cfg != self.cfg:
            raise ValueError(f"UNetModel: the motion adapter was built for {adapter.cfg}, this UNet is {self.cfg}")
        mods = adapter.modules
        inp = [list(b) + ([mods[f"input_blocks.{i}"]] if f"input_blocks.{i}" in mods else []) for i, b in enumerate(self.input_blocks)]
        mid = list(self.middle_block)
        if "middle_block" in mods:
            mid.insert(len(mid) - 1, mods["middle_block"])
        out = []
        for i, b in enumerate(self.output_blocks):
            b, m = list(b), mods.get(f"output_blocks.{i}")
            if m is not None:
                b.insert(len(b) - 1 if isinstance(b[-1], Upsample) else len(b), m)
            out.append(b)
        return inp, mid, out

    def __call__(self, x, timesteps=None, context=None, shared=None, control=None, ip=None, freeu=None, pag=None, y_emb=None, motion=None):
        """y_emb: ``label_embedding(y)``, (batch, E), on a model with label_emb (SDXL) where ``shared`` does not hand the rows in.
        control = (residuals, scales): a ControlNet's len(input_blocks) + 1 residual tensors (or a callable that returns them, called behind
        the middle block) and the device fp32 array of their strengths.  Behind the middle block one launch (control_add) makes new skip tensors
        and a new middle output, skip_i + s_i residual_i, which carry no statistics: the output path's concat GroupNorms then compute theirs
        (ff/group_norm.py::_gn, the explicit path), and no producer is asked for concat statistics.  None: the step as it always was.
        ip = (adapter, kv_ip_all, scales): an IP-Adapter (storage/ip_adapter.py), its context_kv of the image tokens (b, T, kv_n) and a device fp32
        array with one strength per cross-attention in adapter order: every cross-attention becomes the dual launch.  None: the plain launches.
        freeu = a device fp32 array [s1, s2, b1, b2]: FreeU on the 2n blocks of the first two decoder stages (``freeu_stages``).  Behind the
        encoder -- and behind control_add, so the filter reads the skip as the concat would have read it -- one launch (``freeu_skips``) replaces
        their 2n skip tensors, and in front of each of those blocks one launch (``freeu_backbone``) scales the first half of x's channels.  What
        FreeU makes carries no statistics: those 2n concat GroupNorms compute theirs, the producers of what enters them are not asked for concat
        statistics, and the later blocks keep their apply-only concats.  None: the step as it always was, launch for launch.
        pag = (flags, (b0, b1)): perturbed-attention guidance -- flags a device fp32 array of PAG_WORDS words, one per SpatialTransformer in
        ``pag_layers`` order; the rows [b0, b1) of x are the perturbed guidance group: in every SpatialTransformer whose word is not zero their
        self-attention is the identity, attn1(x) = to_out(to_v(norm1(x))), inside the one attention launch (tf_sdpa_pag_16 in place of tf_sdpa_16).
        The words are read when the kernels run.  None: the plain launches.
        motion = (adapter, F): AnimateDiff motion modules (vision/motion.py::MotionAdapter) -- the batch is groups x videos x F images in (group, video,
        frame) order, and every module of the adapter runs at its slot (``_with_motion``) on batch / F videos of F frames.  A module's output is its
        block's output: the skip concats save it, and the block in front emits the statistics of the module's GroupNorm(32, eps 1e-6).  None: the
        sequence as it always was, launch for launch."""
        emb, emb_all, kv_all, br = self._shared(timesteps, context, shared, y_emb)
        frames, input_blocks, middle_block, output_blocks = None, self.input_blocks, self.middle_block, self.output_blocks
        if motion is not None:
            madapter, frames = motion[0], int(motion[1])
            if frames < 1 or x.shape[0] % frames or frames > madapter.max_len:
                raise ValueError(f"UNetModel: motion: a batch of {x.shape[0]} images does not hold videos of {frames} frames (1 .. {madapter.max_len}, frames of a video adjacent)")
            input_blocks, middle_block, output_blocks = self._with_motion(madapter)
        fu = freeu_stages(self.cfg) if freeu is not None else []
        if ip is not None:
            adapter, kv_ip, scales = ip
            if kv_ip.shape[0] != x.shape[0] or kv_ip.shape[2] != adapter.kv_layout()[1] or scales.dtype != np.float32 or scales.size < len(adapter.paths):
                raise ValueError(f"UNetModel: ip K|V {kv_ip.shape} / scales {scales.shape} do not fit a batch of {x.shape[0]} and {len(adapter.paths)} cross-attentions")
            ip = (kv_ip, self.ip_slots(adapter), adapter.kv_layout()[1], scales)
        if pag is not None:
            flags, (b0, b1) = pag
            n_st = len(self._all(SpatialTransformer))
            if flags.dtype != np.float32 or flags.size < n_st or n_st > PAG_WORDS or not 0 <= b0 <= b1 <= x.shape[0]:
                raise ValueError(f"UNetModel: pag flags {flags} / batch range [{b0}, {b1}) do not fit {n_st} SpatialTransformers (at most {PAG_WORDS}) and a batch of {x.shape[0]}")
            pag = (flags, (int(b0), int(b1)))
        run = self._runner(emb, emb_all, kv_all, context, ip, pag, frames)
        x, saved_inputs = self._encode(run, x, br, concat_stats=control is None, replaced=len(fu), blocks=(input_blocks, middle_block))
        if control is not None:
            residuals, scales = control
            *saved_inputs, x = control_add(saved_inputs + [x], residuals() if callable(residuals) else residuals, scales)
        if fu:
            saved_inputs[-len(fu):] = freeu_skips(saved_inputs[-len(fu):], [st for st, *_ in reversed(fu)], freeu)     # (popped from the end: block order reversed)
        for bi, b in enumerate(output_blocks):
            if bi < len(fu):
                x = freeu_backbone(x, fu[bi][0], freeu)
            x = (x, saved_inputs.pop())            # channel concat (unet.py:72), consumed un-materialised
            for j, bb in enumerate(b):
                last = bi == len(output_blocks) - 1 and j == len(b) - 1
                nxt = b[j + 1] if j + 1 < len(b) else (self.out[0] if last else None)
                cout = bb.conv.weight.shape[0] if isinstance(bb, Upsample) else (bb.out_layers[3].weight.shape[0] if isinstance(bb, ResBlock) else bb.proj_out.weight.shape[0])      # (SpatialTransformer and MotionModule: proj_out)
                # the output enters the next concat: emit its statistics in sub-groups as wide as the 32 groups of the saved partner
                # (32 sub-groups for an equal split, 64 for the 2:1 splits), so that the concat's GroupNorm is apply-only
                fg = 0
                if control is None and bi + 1 >= len(fu) and config.concat_stats and nxt is None and saved_inputs and saved_inputs[-1].size <= config.concat_stats_max_elems:
                    c2 = saved_inputs[-1].shape[1]
                    sub = c2 // 32
                    if c2 % 32 == 0 and sub >= 4 and cout % sub == 0 and ((cout + c2) // 32) % sub == 0 and cout // sub <= 256:
                        fg = cout // sub
                x = run(x, bb, nxt, force_gn=fg)
        return self.out[2](self.out[0](x, silu=True))


class KVSlice:
    """Column slice [off, off+2C) of the step-level (b, tk, kv_n) K|V projection."""
    __slots__ = ("arr", "off", "c", "ld")

    def __init__(self, arr, off, c, ld):
        self.arr, self.off, self.c, self.ld = arr, off, c, ld
