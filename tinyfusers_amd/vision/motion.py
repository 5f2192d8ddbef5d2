"""AnimateDiff motion modules (Guo et al. 2023): ``MotionModule`` is the public repository's VanillaTemporalModule / TemporalTransformer3DModel
with one transformer block and attention_blocks = (Temporal_Self, Temporal_Self); ``MotionAdapter`` holds one per slot of a UNet and reads them
from a motion-module file.  A module acts on the (G F, C, h, w) activation of G videos of F frames, frames of one video adjacent:

    x   = proj_in(GroupNorm32(x_in, eps 1e-6))                      per frame (the v2 / v3 "inflated" GroupNorm, diffusers' semantics)
    x   = x + to_out_i(Attn_i(LayerNorm_i(x) + pe_i[:F]))           i = 0, 1: over the F frames of one video and pixel, 8 heads of C / 8
    x   = x + ff(ff_norm(x))                                        GEGLU feed-forward
    out = x_in + s proj_out(x)                                      s: the motion scale, 1 unless ``set_scale`` says otherwise

Launches (9 library entries per module where the GroupNorm statistics came with x_in): GroupNorm inside the 1x1 proj_in; per attention
the LayerNorm-folded q|k|v GEMM on the raw tokens, ONE tf_sdpa_temporal_16 on the column views of that buffer with the fp32 tables pe W^T added
as the operands load -- (LN(x) + pe) W^T = LN(x) W^T + pe W^T --, to_out with the residual in its epilogue; the LayerNorm-folded GEGLU GEMM; and
ff.net[2] folded into proj_out (config.fold_proj_out; the plain pair otherwise) with the residual x_in and the consumer's GroupNorm statistics in
its epilogue.  The temporal launch always merges heads the LDM way, whatever config.head_merge says of the spatial attentions.

The last launch reads PRIVATE live copies of its weight and bias, round16(s base) from the kept fp32 base: ``set_scale`` rewrites them in place,
so a captured step follows the scale without a re-capture.

File names, stated from the published code (no such file exists on the development machines; tests write dicts with exactly these names): under
``<block>.motion_modules.<j>.temporal_transformer.`` -- norm, proj_in (a 2-D Linear weight), transformer_blocks.0.norms.{0,1},
transformer_blocks.0.attention_blocks.{0,1}.{to_q,to_k,to_v,to_out.0,pos_encoder.pe}, transformer_blocks.0.ff_norm, transformer_blocks.0.ff.net.{0.proj,2},
proj_out.  diffusers' MotionAdapter spelling (no ``temporal_transformer.``, attn1 / attn2, norm1 / norm2 / norm3, pos_embed) is accepted too."""
import os
import re

import numpy as np

from .. import config
from ..attention.attention import _concat_rows
from ..attention.sdpa import sdpa_temporal_strided
from ..ff.group_norm import GroupNorm
from ..ff.layer_norm import LayerNorm
from ..ff.linear import Linear, fold_layer_norm, linear_f16, linear_ln_f16
from ..ff.nn import FeedForward
from ..native import hip
from ..storage.state import update_state
from ..storage.tensor import DeviceArray, _sh, dtag, is_bfloat16
from .conv2d import Conv2d, _conv

HEADS = 8                  # temporal_attention_dim_div = 1: always 8 heads of C / 8, whatever the UNet's own head plan
MAX_FRAMES = 32            # tf_sdpa_temporal_16's F


def sinusoid_pe(max_len, channels):
    """The positional table a file without ``pe`` means: pe[:, 0::2] = sin(pos div), pe[:, 1::2] = cos(pos div), div = exp(-ln 1e4 (0, 2, ...) / C)."""
    pos = np.arange(max_len, dtype=np.float64)[:, None]
    div = np.exp(-np.log(10000.0) * np.arange(0, channels, 2, dtype=np.float64) / channels)
    pe = np.zeros((1, max_len, channels), np.float64)
    pe[0, :, 0::2], pe[0, :, 1::2] = np.sin(pos * div), np.cos(pos * div)
    return pe.astype(np.float32)


def motion_slots(cfg, mid=False):
    """[(file prefix, LDM slot, channels)] of the motion modules of a UNet configuration in execution order: down_blocks.i.motion_modules.j behind
    everything else of input_blocks[1 + i (n + 1) + j], mid_block.motion_modules.0 between the middle block's transformer and its second ResBlock
    (``mid``: v2 files), up_blocks.i.motion_modules.j in output_blocks[i (n + 1) + j] in front of an Upsample; n = num_res_blocks."""
    mc, n, nlev = cfg.model_channels, cfg.num_res_blocks, len(cfg.channel_mult)
    rows = [(f"down_blocks.{i}.motion_modules.{j}", f"input_blocks.{1 + i * (n + 1) + j}", mc * cfg.channel_mult[i]) for i in range(nlev) for j in range(n)]
    if mid:
        rows.append(("mid_block.motion_modules.0", "middle_block", mc * cfg.channel_mult[-1]))
    rows += [(f"up_blocks.{i}.motion_modules.{j}", f"output_blocks.{i * (n + 1) + j}", mc * cfg.channel_mult[nlev - 1 - i]) for i in range(nlev) for j in range(n + 1)]
    return rows


class _PosEncoder:
    def __init__(self, max_len, channels):
        self._state_leaves = {"pe": (1, max_len, channels)}
        self.pe = None


class _TemporalAttention:
    """One Temporal_Self attention: bias-free to_q / to_k / to_v, to_out.0 with bias, its own positional table."""

    def __init__(self, channels, max_len, init=True):
        self.to_q, self.to_k, self.to_v = (Linear(channels, channels, bias=False, init=init) for _ in range(3))
        self.to_out = [Linear(channels, channels, init=init)]
        self.pos_encoder = _PosEncoder(max_len, channels)
        self._fused = self._ln_fold = self._tabs = None

    def _fused_weights(self):
        key = (self.to_q.weight.wkey, self.to_k.weight.wkey, self.to_v.weight.wkey)
        if self._fused is None or self._fused[0] != key:
            self._fused = (key, _concat_rows([self.to_q.weight, self.to_k.weight, self.to_v.weight]))
        return self._fused[1]

    def _folded(self, ln):
        w = self._fused_weights()
        key = (w.wkey, ln.weight.wkey, ln.bias.wkey)
        if self._ln_fold is None or self._ln_fold[0] != key:
            self._ln_fold = (key, fold_layer_norm(w, None, ln))
        return self._ln_fold[1]

    def tables(self, F):
        """(pe_q, pe_k, pe_v): fp32 (F, C) device arrays pe[:F] W^T of the RAW weights, built once per weight set and F -- outside a captured step:
        the first eager call or ``MotionAdapter.prepare`` -- and kept.  float16: tf_linear_f32out_f16 (fp32 accumulators of 16-bit operands);
        bfloat16 has no such entry, its tables are the same products formed on the host in fp32 from the stored values."""
        pe = self.pos_encoder.pe
        ws = (self.to_q.weight, self.to_k.weight, self.to_v.weight)
        key = (pe.wkey,) + tuple(w.wkey for w in ws) + (F,)
        if self._tabs is None or self._tabs[0] != key:
            c = pe.shape[2]
            if not 1 <= F <= min(MAX_FRAMES, pe.shape[1]):
                raise ValueError(f"MotionModule: {F} frames: the positional table holds {pe.shape[1]} and the temporal attention launch takes 1 .. {MAX_FRAMES}")
            tabs = []
            if is_bfloat16(pe.dtype):
                rows = pe.numpy()[0, :F]
                tabs = [DeviceArray.from_numpy(np.ascontiguousarray(rows @ w.numpy().T, dtype=np.float32), np.float32, "row") for w in ws]
            else:
                for w in ws:
                    t = DeviceArray.empty((F, c), np.float32, "row")
                    hip.tf_linear_f32out_f16(t.ptr, pe.ptr, w.ptr, F, c, c, _sh())
                    tabs.append(t)
            self._tabs = (key, tuple(tabs))
        return self._tabs[1]

    def __call__(self, x, G, F, ln, residual):
        n, p, c = x.shape
        hs = c // HEADS
        if config.fuse_layer_norm and c % 64 == 0:
            qkv = linear_ln_f16(x, self._folded(ln), ln.eps)               # (G F, P, 3C): q | k | v of LN(x), no bias
        else:
            qkv = linear_f16(ln(x), self._fused_weights())
        o = DeviceArray.empty((n, p, c), x.dtype, "row")
        si, so = (3 * c * p, 3 * c, hs), (c * p, c, hs)                    # (frame, pixel, head) strides; o: the LDM head merge
        sdpa_temporal_strided(o, qkv, qkv.view(qkv.shape, "row", c), qkv.view(qkv.shape, "row", 2 * c), G, F, p, HEADS, hs, si, si, si, so, *self.tables(F))
        return self.to_out[0](o, residual=residual)


class _TemporalBlock:
    def __init__(self, channels, max_len, init=True):
        self.attention_blocks = [_TemporalAttention(channels, max_len, init=init) for _ in range(2)]
        self.norms = [LayerNorm(channels, init=init) for _ in range(2)]
        self.ff = FeedForward(channels, init=init)
        self.ff_norm = LayerNorm(channels, init=init)


class MotionModule:
    """One motion module; its attribute tree below ``temporal_transformer.`` spells the file's names (update_state fills it)."""

    def __init__(self, channels, max_len, init=True):
        if channels % (8 * HEADS) or not 8 <= channels // HEADS <= 160:
            raise ValueError(f"MotionModule: {channels} channels: {HEADS} heads need a head size that is a multiple of 8 in [8, 160]")
        self.channels, self.max_len = int(channels), int(max_len)
        self.norm = GroupNorm(32, channels, eps=1e-6, init=init)
        self.proj_in = Conv2d(channels, channels, kernel_size=[1, 1], init=init)       # (the file's 2-D Linear weight: the 1x1 conv's bytes)
        self.transformer_blocks = [_TemporalBlock(channels, max_len, init=init)]
        self.proj_out = Conv2d(channels, channels, kernel_size=[1, 1], init=init)
        self._scale, self._live = 1.0, None
        if init:
            for a in self.transformer_blocks[0].attention_blocks:
                a.pos_encoder.pe = DeviceArray.from_numpy(sinusoid_pe(max_len, channels), self.norm.weight.dtype, "row")

    def _folds(self):
        return config.fold_proj_out and config.dtype != "fp8"

    def _last(self):
        """(weight, bias) the last launch reads: private live copies round16(s base) of proj_out -- with ff.net[2] folded in front where
        config.fold_proj_out applies (SpatialTransformer._ff2_proj_out's fold, on the host in fp32) -- from the kept fp32 base.  Rebuilt when a
        weight below is replaced (a captured step then needs its capture again, as for any weight)."""
        ff2, po = self.transformer_blocks[0].ff.net[2], self.proj_out
        fold = self._folds()
        key = (ff2.weight.wkey, ff2.bias.wkey, po.weight.wkey, po.bias.wkey, fold)
        if self._live is None or self._live[0] != key:
            c = self.channels
            wp, bp = po.weight.numpy().reshape(c, -1), po.bias.numpy()
            if fold:
                w2, b2 = ff2.weight.numpy(), ff2.bias.numpy()
                wp, bp = np.concatenate((wp @ w2, wp), axis=1), wp @ b2 + bp
            wp, bp = np.ascontiguousarray(wp, dtype=np.float32), np.ascontiguousarray(bp, dtype=np.float32)
            dt = po.weight.dtype
            base = (wp, bp) if is_bfloat16(dt) else (DeviceArray.from_numpy(wp, np.float32, "row"), DeviceArray.from_numpy(bp, np.float32, "row"))
            live = (DeviceArray.empty((c, wp.shape[1], 1, 1), dt, "nhwc"), DeviceArray.empty((c,), dt, "row"))
            self._live = (key, base, live)
            self._write_live()
        return self._live[2]

    def _write_live(self):
        """live = round16(scale base): one fp32 multiply and one rounding per element.  float16: tf_scale_cast_f32_to_f16 on the current stream;
        bfloat16: the same product and rounding on the host (storage/tensor.py::f32_to_bf16_bits) and an upload -- outside any captured step."""
        _, base, live = self._live
        s = np.float32(self._scale)
        for b, l in zip(base, live):
            if isinstance(b, DeviceArray):
                hip.tf_scale_cast_f32_to_f16(l.ptr, b.ptr, float(s), b.size, _sh())
            else:
                hip.tf_stream_sync(_sh())
                l.copy_from_numpy((s * b).astype(np.float32).reshape(l.shape))

    def set_scale(self, s):
        """The strength of the residual branch, out = x_in + s proj_out(x), from the next launch on (stream-ordered on the current stream)."""
        s = float(s)
        if not np.isfinite(s):
            raise ValueError(f"MotionModule.set_scale: the motion scale is a finite float, got {s!r}")
        self._scale = s
        if self._live is not None:
            self._write_live()

    def prepare(self, F):
        """Everything derived from the weights that a captured step must find built: the positional tables of F frames and the live last launch."""
        for a in self.transformer_blocks[0].attention_blocks:
            a.tables(F)
        self._last()

    def __call__(self, x_in, F, out_gn=0, out_norm=None):
        """x_in: (G F, C, h, w) NHWC, the frames of a video adjacent.  out_gn / out_norm: the consumer's GroupNorm, as for SpatialTransformer."""
        n, c, h, w = x_in.shape
        if c != self.channels or F < 1 or n % F:
            raise ValueError(f"MotionModule: a batch of {n} images with {c} channels does not hold videos of {F} frames with {self.channels} channels")
        G, blk = n // F, self.transformer_blocks[0]
        x = self.proj_in(x_in, gn_in=(self.norm, False)).tokens()              # (G F, P, C)
        for attn, ln in zip(blk.attention_blocks, blk.norms):
            x = attn(x, G, F, ln, residual=x)
        wl, bl = self._last()
        fused_ln = config.fuse_layer_norm and c % 64 == 0
        if self._folds():
            hid = blk.ff.net[0](x, ln=blk.ff_norm) if fused_ln else blk.ff.net[0](blk.ff_norm(x))
            pair = (hid.image(n, hid.shape[-1], h, w), x.image(n, c, h, w))
            return _conv(pair, wl, bl, [0, 0], [1, 1], [1, 1], residual=x_in, gn=out_gn, out_norm=out_norm)
        x = blk.ff(x, residual=x, ln=blk.ff_norm) if fused_ln else blk.ff(blk.ff_norm(x), residual=x)
        return _conv(x.image(n, c, h, w), wl, bl, [0, 0], [1, 1], [1, 1], residual=x_in, gn=out_gn, out_norm=out_norm)


# ---- the file ---------------------------------------------------------------------------------------------------------------------------------
_DIFFUSERS = ((".attn1.", ".attention_blocks.0."), (".attn2.", ".attention_blocks.1."), (".norm1.", ".norms.0."), (".norm2.", ".norms.1."),
              (".norm3.", ".ff_norm."), (".pos_embed.", ".pos_encoder."))
_KEY = re.compile(r"^((?:down_blocks|up_blocks)\.\d+\.motion_modules\.\d+|mid_block\.motion_modules\.\d+)\.(.+)$")


def module_shapes(channels, max_len, pe=True):
    """name -> shape of one module's tensors, relative to ``temporal_transformer.``, as the AnimateDiff files spell them."""
    c, t = channels, "transformer_blocks.0."
    s = {"norm.weight": (c,), "norm.bias": (c,), "proj_in.weight": (c, c), "proj_in.bias": (c,), "proj_out.weight": (c, c), "proj_out.bias": (c,),
         t + "ff_norm.weight": (c,), t + "ff_norm.bias": (c,), t + "ff.net.0.proj.weight": (8 * c, c), t + "ff.net.0.proj.bias": (8 * c,),
         t + "ff.net.2.weight": (c, 4 * c), t + "ff.net.2.bias": (c,)}
    for i in (0, 1):
        a = f"{t}attention_blocks.{i}."
        s.update({f"{t}norms.{i}.weight": (c,), f"{t}norms.{i}.bias": (c,), a + "to_q.weight": (c, c), a + "to_k.weight": (c, c), a + "to_v.weight": (c, c),
                  a + "to_out.0.weight": (c, c), a + "to_out.0.bias": (c,)})
        if pe:
            s[a + "pos_encoder.pe"] = (1, max_len, c)
    return s


def canonical_name(key):
    """A file's key in either spelling -> (module prefix, name relative to temporal_transformer. in the AnimateDiff spelling), or None."""
    m = _KEY.match(key)
    if m is None:
        return None
    prefix, rest = m.groups()
    if rest.startswith("temporal_transformer."):
        rest = rest[len("temporal_transformer."):]
    rest = "." + rest
    for a, b in _DIFFUSERS:
        rest = rest.replace(a, b)
    return prefix, rest[1:]


def parse_motion_state(cfg, state):
    """Check a file's tensors against the UNet configuration, host code only: -> (max_len, mid, {module prefix: {name: array}}), the positional
    tables filled in with the sinusoid where the file has none.  Unknown, missing or mis-shaped tensors raise ValueError naming them; so does a
    module for a block the UNet does not have, or of another channel count."""
    mods, unknown = {}, []
    for key, v in state.items():
        cn = canonical_name(key)
        if cn is None:
            unknown.append(key)
            continue
        mods.setdefault(cn[0], {})[cn[1]] = np.asarray(v.numpy() if hasattr(v, "numpy") and not isinstance(v, np.ndarray) else v)
    if unknown:
        raise ValueError(f"MotionAdapter.load: the file holds tensors that name no motion module: {sorted(unknown)[:4]}")
    if not mods:
        raise ValueError("MotionAdapter.load: the file holds no motion module (no *.motion_modules.* tensor)")
    mid = any(p.startswith("mid_block.") for p in mods)
    plan = {p: c for p, _, c in motion_slots(cfg, mid)}
    for p in mods:
        if p not in plan:
            raise ValueError(f"MotionAdapter.load: the file has a module at {p}, this UNet configuration has no such block (its slots: {len(plan)} modules, "
                             f"{next(iter(plan))} ... {list(plan)[-1]})")
    for p in plan:
        if p not in mods:
            raise ValueError(f"MotionAdapter.load: the file lacks the module {p}.* (this UNet configuration has {len(plan)} slots)")
    has_pe = any(name.endswith(".pe") for m in mods.values() for name in m)
    max_len = MAX_FRAMES
    if has_pe:
        first = next(v for m in mods.values() for name, v in m.items() if name.endswith(".pe"))
        if first.ndim != 3 or first.shape[0] != 1 or first.shape[1] < 1:
            raise ValueError(f"MotionAdapter.load: a positional table pos_encoder.pe has shape {tuple(first.shape)}, not (1, max_len, C)")
        max_len = int(first.shape[1])
    for p, c in plan.items():
        want, have = module_shapes(c, max_len, has_pe), mods[p]
        gamma = have.get("norm.weight")
        if gamma is not None and gamma.ndim == 1 and gamma.shape[0] != c:
            raise ValueError(f"MotionAdapter.load: the module {p} has {gamma.shape[0]} channels (norm.weight), the UNet's block has {c}")
        for name, shape in want.items():
            if name not in have:
                raise ValueError(f"MotionAdapter.load: the file lacks {p}.temporal_transformer.{name}")
            got = tuple(have[name].shape)
            if name in ("proj_in.weight", "proj_out.weight") and got == shape + (1, 1):
                have[name] = have[name].reshape(shape)                       # (stored as a 1x1 conv: the same bytes)
            elif got != shape:
                raise ValueError(f"MotionAdapter.load: {p}.temporal_transformer.{name} has shape {got}, this UNet needs {shape}")
        extra = sorted(n for n in have if n not in want)
        if extra:
            raise ValueError(f"MotionAdapter.load: the file holds tensors a motion module has no place for: {[f'{p}.temporal_transformer.{n}' for n in extra[:4]]}")
        if not has_pe:
            for i in (0, 1):
                have[f"transformer_blocks.0.attention_blocks.{i}.pos_encoder.pe"] = sinusoid_pe(max_len, c)
    return max_len, mid, mods


class MotionAdapter:
    """The motion modules of one UNet configuration: ``modules`` maps an LDM slot ("input_blocks.4", "middle_block", "output_blocks.7") to its
    MotionModule, in execution order; ``UNetModel.__call__(motion=(adapter, F))`` runs them."""

    def __init__(self, cfg, max_len=MAX_FRAMES, mid=False, init=False):
        self.cfg, self.max_len, self.mid = cfg, int(max_len), bool(mid)
        self.plan = motion_slots(cfg, mid)
        self.modules = {slot: MotionModule(c, max_len, init=init) for _, slot, c in self.plan}

    @classmethod
    def load(cls, cfg, src):
        """``src``: a ``.ckpt`` / ``.pt`` / ``.safetensors`` file (storage/unpicker.py::load_checkpoint) or a dict of arrays.  Everything is checked
        on the host before anything is uploaded; the tensors are installed in the step's 16-bit type (config.is_bf16())."""
        if isinstance(src, (str, os.PathLike)):
            from ..storage.unpicker import load_checkpoint
            src = load_checkpoint(os.fspath(src))
        if not isinstance(src, dict):
            raise TypeError(f"MotionAdapter.load: takes a file name or a dict, got {type(src).__name__}")
        max_len, mid, mods = parse_motion_state(cfg, src)
        self = cls(cfg, max_len, mid)
        for prefix, slot, _ in self.plan:
            update_state(self.modules[slot], mods[prefix], "")
        return self

    def module_list(self):
        return list(self.modules.values())

    def prepare(self, F):
        """Build what a captured step of F frames must find built (the positional tables, the live last launches), on the current stream."""
        if not 1 <= int(F) <= min(MAX_FRAMES, self.max_len):
            raise ValueError(f"MotionAdapter: frames={F}: 1 <= F <= {min(MAX_FRAMES, self.max_len)} (the positional tables hold {self.max_len} frames, the "
                             f"temporal attention launch takes {MAX_FRAMES})")
        for m in self.modules.values():
            m.prepare(int(F))

    def scales(self, value):
        """One motion scale, or one per module in execution order -> the list of finite floats, or ValueError."""
        n = len(self.modules)
        try:
            sc = np.asarray(value, dtype=np.float64)
        except (TypeError, ValueError):
            sc = None
        if sc is None or sc.ndim > 1 or (sc.ndim == 1 and sc.shape[0] != n) or not np.isfinite(sc).all():
            raise ValueError(f"MotionAdapter: the motion scale is one finite float or {n} (one per module in execution order), got {value!r}")
        return [float(v) for v in np.broadcast_to(sc, (n,))]

    def set_scale(self, value):
        for m, s in zip(self.modules.values(), self.scales(value)):
            m.set_scale(s)
