"""The OpenCLIP ViT-H/14 text tower as Stable Diffusion 2.x uses it (LDM's ``FrozenOpenCLIPEmbedder(layer="penultimate")``): 77 token ids in, the
(B, T, 1024) context the SD-2.x UNet's cross-attention reads out.

It is the layer vae/clip_vision.py runs -- LayerNorm folded into the fused q|k|v GEMM, flash SDPA through strides (16 heads of 64: the LDS-DMA
kernel the SD-1.5 text encoder runs), out_proj + residual, LayerNorm folded into fc1, the exact GELU (tf_gelu_erf_16), fc2 + residual -- with the
causal mask of vae/encoder.py::CLIPTextTransformer, over ``layers - 1`` of the checkpoint's resblocks (the penultimate layer's output), then
``ln_final``.  The attribute tree spells the names of an LDM v2 checkpoint below ``cond_stage_model.model.``, so update_state on the whole
StableDiffusion walks them:

    token_embedding.weight (vocab, W)        positional_embedding (positions, W), a bare parameter
    transformer.resblocks.N.ln_1 / ln_2 .weight / .bias
    transformer.resblocks.N.attn.in_proj_weight (3W, W) / in_proj_bias (3W,): q | k | v rows in that order, installed as the fused operand
    transformer.resblocks.N.attn.out_proj, .mlp.c_fc, .mlp.c_proj .weight / .bias           ln_final.weight / .bias

The last resblock, ``text_projection``, ``logit_scale`` and ``attn_mask`` of a checkpoint have no slot here: they are read past and never run.

SDXL's second embedder (LDM's ``FrozenOpenCLIPEmbedder2(layer="penultimate", legacy=False)``, ViT-bigG/14: ``BIG_G_TEXT``) is
``OpenClipText(cfg, tap="penultimate_raw", pooled=True)``: every resblock runs, the context is the penultimate resblock's output WITHOUT ``ln_final``,
and the pooled vector is ``ln_final(last)[b, argmax(ids[b])] @ text_projection`` -- the row of the highest token id, OpenCLIP's rule for the
end-of-text token; ``text_projection`` is a bare (W, W) parameter used un-transposed.  Then the last resblock and ``text_projection`` do have slots."""
import os
from dataclasses import dataclass

import numpy as np

from ..attention.attention import CLIPAttention
from ..ff.embedding import Embedding, embedding
from ..ff.layer_norm import LayerNorm
from ..ff.linear import Linear, fold_layer_norm
from ..ff.nn import CLIPMLP
from ..native import hip
from ..storage.state import param_shapes as _param_shapes
from ..storage.state import update_state
from ..storage.tensor import DeviceArray, _sh, bfloat16, dtag, is_bfloat16

LDM_PREFIX = "cond_stage_model.model."


@dataclass(frozen=True)
class OpenClipTextConfig:
    width: int = 1024
    layers: int = 24          # the checkpoint's resblocks; layers - 1 of them run
    heads: int = 16
    mlp: int = 4096
    vocab: int = 49408
    positions: int = 77
    eps: float = 1e-5


VIT_H_TEXT = OpenClipTextConfig()
BIG_G_TEXT = OpenClipTextConfig(width=1280, layers=32, heads=20, mlp=5120)       # OpenCLIP ViT-bigG/14: SDXL's second text tower


def pooled_rows(input_ids):
    """The row of the (B T, W) token matrix the pooled vector is read from, per prompt: b T + argmax(ids[b]) -- the FIRST position of the highest
    id (numpy's and torch's argmax), which is the end-of-text token wherever it stands, padding behind it or not."""
    ids = np.asarray(input_ids)
    if ids.ndim != 2 or ids.dtype.kind not in "iu":
        raise ValueError(f"OpenClipText: the pooled vector needs (B, T) integer token ids on the host, got {ids.dtype} {ids.shape}")
    b, t = ids.shape
    return (np.arange(b) * t + ids.argmax(axis=1)).astype(np.int32)


class _Attention(CLIPAttention):
    """CLIPAttention over the checkpoint's fused in_proj: the (3W, W) weight and (3W,) bias ARE the q | k | v operand CLIPAttention concatenates
    from three Linears, so nothing is split or copied."""

    def __init__(self, width, heads):
        assert width % heads == 0, (width, heads)
        self.embed_dim, self.num_heads, self.head_dim = width, heads, width // heads
        self.in_proj_weight = self.in_proj_bias = None
        self.out_proj = Linear(width, width, init=False)
        self._state_leaves = {"in_proj_weight": (3 * width, width), "in_proj_bias": (3 * width,)}
        self._fused = None

    def _qkv(self, ln):
        w, b = self.in_proj_weight, self.in_proj_bias
        key = (w.wkey, b.wkey) + ((ln.weight.wkey, ln.bias.wkey) if ln is not None else ())
        if self._fused is None or self._fused[0] != key:
            self._fused = (key, fold_layer_norm(w, b, ln) if ln is not None else (w, b))
        return self._fused[1]


class _Mlp(CLIPMLP):
    """CLIPMLP with the exact GELU under OpenCLIP's names: c_fc, c_proj."""

    def __init__(self, width, hidden):
        self.act = "gelu"
        self.c_fc = Linear(width, hidden, init=False)
        self.c_proj = Linear(hidden, width, init=False)

    fc1 = property(lambda self: self.c_fc)
    fc2 = property(lambda self: self.c_proj)


class _ResBlock:
    def __init__(self, cfg):
        self.ln_1 = LayerNorm(cfg.width, eps=cfg.eps, init=False)
        self.attn = _Attention(cfg.width, cfg.heads)
        self.ln_2 = LayerNorm(cfg.width, eps=cfg.eps, init=False)
        self.mlp = _Mlp(cfg.width, cfg.mlp)

    def __call__(self, x, mask):
        x = self.attn(x, mask, residual=x, ln=self.ln_1)
        return self.mlp(x, residual=x, ln=self.ln_2)


class _Transformer:
    def __init__(self, cfg, every=False):
        self.resblocks = [_ResBlock(cfg) for _ in range(cfg.layers if every else cfg.layers - 1)]      # penultimate: the last resblock never runs (every: the pooled vector reads it)


class _Model:
    def __init__(self, cfg, pooled=False):
        self.token_embedding = Embedding(cfg.vocab, cfg.width, init=False)
        self.positional_embedding = None
        self._state_leaves = {"positional_embedding": (cfg.positions, cfg.width)}
        self.transformer = _Transformer(cfg, every=pooled)
        self.ln_final = LayerNorm(cfg.width, eps=cfg.eps, init=False)
        if pooled:
            self.text_projection = None
            self._state_leaves["text_projection"] = (cfg.width, cfg.width)


def config_from_state(state, heads=None):
    """The configuration a checkpoint's shapes state (names without prefix).  The head count is not in the file: ``heads`` None means width // 64,
    OpenCLIP's head size."""
    for key, nd in (("token_embedding.weight", 2), ("positional_embedding", 2), ("transformer.resblocks.0.mlp.c_fc.weight", 2)):
        if key not in state or np.ndim(state[key]) != nd:
            raise ValueError(f"OpenClipText.load: the file lacks {key}" if key not in state else f"OpenClipText.load: {key} has shape {tuple(np.shape(state[key]))}")
    vocab, width = (int(v) for v in np.shape(state["token_embedding.weight"]))
    layers = 0
    while f"transformer.resblocks.{layers}.mlp.c_fc.weight" in state:
        layers += 1
    heads = width // 64 if heads is None else int(heads)
    if layers < 2 or heads < 1 or width % heads:
        raise ValueError(f"OpenClipText.load: {layers} resblocks (at least 2: the penultimate one's output is the context), heads={heads} for width {width}")
    return OpenClipTextConfig(width=width, layers=layers, heads=heads, mlp=int(np.shape(state["transformer.resblocks.0.mlp.c_fc.weight"])[0]), vocab=vocab,
                              positions=int(np.shape(state["positional_embedding"])[0]))


def load_state(src):
    """name (without the LDM prefix) -> array of a file (load_checkpoint's formats) or a dict, flat or under "state_dict": the tensors below
    ``cond_stage_model.model.`` when the source has any, else those below ``model.``, else the source's own names."""
    if isinstance(src, (str, os.PathLike)):
        from ..storage.unpicker import load_checkpoint
        src = load_checkpoint(os.fspath(src))
    if not isinstance(src, dict):
        raise TypeError(f"OpenClipText.load: takes a file name or a dict, got {type(src).__name__}")
    if "state_dict" in src and isinstance(src["state_dict"], dict):
        src = src["state_dict"]
    for prefix in (LDM_PREFIX, "model."):
        if any(k.startswith(prefix) for k in src):
            return {k[len(prefix):]: v for k, v in src.items() if k.startswith(prefix)}
    return dict(src)


class OpenClipText:
    """``tower = OpenClipText.load(file | dict)`` (or built empty and filled by update_state under ``cond_stage_model``); ``tower(ids)``: (B, T <= 77)
    token ids, host or int32 device array -> the device (B, T, width) context in the 16-bit type the weights were installed in."""

    def __init__(self, cfg=VIT_H_TEXT, tap="penultimate", pooled=False):
        """tap: "penultimate" -- ln_final of the penultimate resblock's output, the SD-2.x context -- or "penultimate_raw", that output itself
        (SDXL).  pooled=True: ``tower(ids)`` returns (context, pooled (B, W)); the last resblock and text_projection are then part of the tree."""
        if cfg.layers < 2 or cfg.width % cfg.heads or cfg.width % 64 or cfg.width > 2560 or cfg.mlp % 8:
            raise ValueError(f"OpenClipText: unsupported configuration {cfg} (at least 2 layers, width a multiple of 64 and of heads, <= 2560)")
        if tap not in ("penultimate", "penultimate_raw"):
            raise ValueError(f"OpenClipText: tap= takes 'penultimate' or 'penultimate_raw', got {tap!r}")
        self.cfg = cfg
        self._tap, self._pooled, self._proj_t = tap, bool(pooled), None
        self.model = _Model(cfg, pooled=self._pooled)

    @classmethod
    def load(cls, src, heads=None):
        from .clip_vision import _host
        state = {k: _host(v) for k, v in load_state(src).items()}
        self = cls(config_from_state(state, heads))
        for key, shape in _param_shapes(self.model).items():
            if key not in state:
                raise ValueError(f"OpenClipText.load: the file lacks {key}")
            if tuple(state[key].shape) != tuple(shape):
                raise ValueError(f"OpenClipText.load: {key} has shape {tuple(state[key].shape)}, this tower needs {tuple(shape)}")
        update_state(self.model, state, "")
        return self

    @property
    def dtype(self):
        w = self.model.ln_final.weight
        if w is None:
            raise RuntimeError("OpenClipText: the tower has no weights yet (OpenClipText.load, or update_state on the model that holds it)")
        return w.dtype

    def embeddings(self, input_ids):
        """token rows + position rows: one gather launch in float16 (tf_embedding_f16 adds the position row); in bfloat16 the gather copies the
        rows' bits and one tf_add_16 launch per sequence adds the positions."""
        m, t = self.model, int(input_ids.shape[1])
        if t > self.cfg.positions:
            raise ValueError(f"OpenClipText: {t} tokens, the tower has {self.cfg.positions} positions")
        if not is_bfloat16(self.dtype):
            return embedding(m.token_embedding.weight, input_ids, m.positional_embedding)
        rows = embedding(m.token_embedding.weight, input_ids)                # (a 16-bit gather: the bits of the bfloat16 rows)
        b, _, d = rows.shape
        x = DeviceArray.empty((b, t, d), bfloat16, "row")
        for k in range(b):
            hip.tf_add_16(dtag(bfloat16), x.ptr + k * t * d * 2, rows.ptr + k * t * d * 2, m.positional_embedding.ptr, t * d, _sh())
        x._base = rows                                                       # (referenced until the adds have run)
        return x

    def __call__(self, input_ids):
        t = int(input_ids.shape[1])
        rows = pooled_rows(input_ids) if self._pooled else None                            # (checked before anything is launched)
        x = self.embeddings(input_ids)
        mask = np.triu(np.full((1, 1, t, t), float("-inf"), dtype=np.float32), k=1)       # the causal mask of vae/encoder.py:79
        blocks = self.model.transformer.resblocks
        for block in blocks[:self.cfg.layers - 1]:
            x = block(x, mask)
        ctx = self.model.ln_final(x) if self._tap == "penultimate" else x
        if not self._pooled:
            return ctx
        return ctx, self._pool(self.model.ln_final(blocks[-1](x, mask)), rows)

    def _pool(self, last, rows):
        """ln_final(last)[b, argmax(ids[b])] @ text_projection: one row gather (tf_gather_rows_16; the indices travel as a device int32 array) and one
        GEMV over the projection transposed once per weight (our Linear computes x W^T)."""
        b, t, w = last.shape
        proj = self.model.text_projection
        if self._proj_t is None or self._proj_t[0] != proj.wkey:
            pt = DeviceArray.empty((w, w), proj.dtype, "row")
            hip.tf_nhwc_to_nchw_f16(pt.ptr, proj.ptr, 1, w, 1, w, _sh())                  # (K, N) -> (N, K): a 2-byte transpose, either element type
            self._proj_t = (proj.wkey, pt)
        idx = DeviceArray.from_numpy(rows, np.int32, "row")
        picked = DeviceArray.empty((b, w), last.dtype, "row")
        hip.tf_gather_rows_16(picked.ptr, last.ptr, idx.ptr, b, w, b * t, _sh())
        from ..ff.linear import gemv_rows
        out = gemv_rows(picked, self._proj_t[1])
        out._base = (out._base, idx, picked, last)                                        # (referenced until the kernels have run)
        return out


def param_shapes(cfg, pooled=False):
    """name (below ``cond_stage_model.model.``) -> shape of every tensor the tower reads."""
    return _param_shapes(OpenClipText(cfg, pooled=pooled).model)


def synthetic_state(cfg, seed=0, prefix="", pooled=False):
    """Seeded weights in the checkpoint's names (fp16 values as fp32 arrays), the LAST resblock included as a file has it: what example/sd1.py and
    tools/sampler_bench.py run without a file.  Scaled so that activations stay of order one through the layers."""
    rng = np.random.default_rng(seed)
    shapes = dict(param_shapes(cfg, pooled))
    last = f"transformer.resblocks.{cfg.layers - 1}."
    shapes.update({k.replace("transformer.resblocks.0.", last): s for k, s in list(shapes.items()) if k.startswith("transformer.resblocks.0.")})
    out = {}
    for k, s in shapes.items():
        if k.endswith((".ln_1.weight", ".ln_2.weight", "ln_final.weight")):
            a = 1.0 + 0.05 * rng.standard_normal(s)
        elif k.endswith(("bias", "positional_embedding", "token_embedding.weight")):
            a = 0.05 * rng.standard_normal(s)
        elif k == "text_projection":
            a = rng.standard_normal(s) * (0.7 / np.sqrt(s[0]))
        else:
            a = rng.standard_normal(s) * (0.7 / np.sqrt(s[-1]))
        out[prefix + k] = a.astype(np.float16).astype(np.float32)
    return out
