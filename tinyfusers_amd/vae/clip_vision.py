"""The CLIP ViT image tower with projection (``CLIPVisionModelWithProjection``; ViT-H/14 is the IP-Adapter's image encoder): a uint8 picture in,
the projected image embedding out, all on the device.  It is the front end of ``StableDiffusion.start(ip_image=)`` (variants/sd.py).

A ViT encoder layer is the CLIP text tower's layer (vae/encoder.py: CLIPAttention, CLIPMLP) with other sizes, no mask and the exact GELU, so the
layers reuse those classes and their kernels: LayerNorm folded into the fused q|k|v GEMM, unmasked SDPA through strides (257 tokens, 16 heads of
80: the in-block split form), out_proj + residual, LayerNorm folded into fc1, tf_gelu_erf_16 in place, fc2 + residual.  What is the tower's own
lives in csrc/vit.hip: the input edge (tf_vit_patchify_u8_16: normalised patch matrix, the A operand of the patch-embedding GEMM), the token
assembly with the pre-LayerNorm (tf_vit_embed_ln_16) and the GELU.  The pooled head gathers the class rows with one strided copy, then
post_layernorm folded into the bias-free visual_projection (one tf_linear_ln_16 launch).

File format, as published (no image-encoder file exists on the development machines: the names are stated from the published format and pinned by
tests/test_clip_vision_host.py on files the test writes).  Flat ``.safetensors`` / torch-zip ``.bin`` / ``.pt``:
``vision_model.embeddings.class_embedding`` (D), ``vision_model.embeddings.patch_embedding.weight`` (D, 3, P, P; no bias),
``vision_model.embeddings.position_embedding.weight`` (T, D), ``vision_model.pre_layrnorm.{weight,bias}`` (the upstream spelling),
``vision_model.encoder.layers.{i}.{self_attn.{q,k,v,out}_proj, layer_norm1, layer_norm2, mlp.{fc1,fc2}}.{weight,bias}``,
``vision_model.post_layernorm.{weight,bias}``, ``visual_projection.weight`` (E, D).  ``vision_model.embeddings.position_ids`` is ignored; a
file with ``text_model.*`` keys (a whole CLIP model) is refused."""
import ctypes
import os
from dataclasses import dataclass

import numpy as np

from ..attention.attention import CLIPAttention
from ..ff.layer_norm import LayerNorm
from ..ff.linear import Linear, fold_layer_norm, linear_f16, linear_ln_f16
from ..ff.nn import CLIPMLP
from ..native import hip
from ..storage.state import update_state
from ..storage.tensor import DeviceArray, Stream, _sh, asarray, bfloat16, dtag, ensure_init, pool, use_stream

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
P_ = "vision_model."


@dataclass(frozen=True)
class ClipVisionConfig:
    image: int = 224
    patch: int = 14
    width: int = 1280
    heads: int = 16
    layers: int = 32
    mlp: int = 5120
    projection: int = 1024
    eps: float = 1e-5

    @property
    def tokens(self):
        return (self.image // self.patch) ** 2 + 1

    @property
    def kpad(self):
        """Columns of the patch matrix: 3 P^2 rounded up to whole 16-byte vectors (588 -> 592 for P = 14)."""
        return (3 * self.patch * self.patch + 7) // 8 * 8


VIT_H = ClipVisionConfig()


def norm_constants():
    """(scale3, shift3) of tf_vit_patchify_u8_16 for CLIP's mean / std: x_norm = u8 * scale + shift, rounded to fp32."""
    mean, std = np.asarray(CLIP_MEAN, np.float64), np.asarray(CLIP_STD, np.float64)
    return (1.0 / (255.0 * std)).astype(np.float32), (-mean / std).astype(np.float32)


def pack_patch_weight(w, kpad):
    """The (D, 3, P, P) conv weight of the file as the (D, kpad) GEMM weight the patch matrix multiplies: column ky 3P + kx 3 + c (the order of
    tf_vit_patchify_u8_16's columns), zero beyond 3 P^2.  Host code, done once per weight set."""
    w = np.asarray(w, np.float32)
    d, c, p, p2 = w.shape
    assert c == 3 and p == p2 and kpad % 8 == 0 and kpad >= 3 * p * p, (w.shape, kpad)
    out = np.zeros((d, kpad), np.float32)
    out[:, :3 * p * p] = w.transpose(0, 2, 3, 1).reshape(d, 3 * p * p)
    return out


def param_shapes(cfg):
    """name -> shape of every tensor of a ``CLIPVisionModelWithProjection`` file of that configuration."""
    d, s = cfg.width, {}
    s[P_ + "embeddings.class_embedding"] = (d,)
    s[P_ + "embeddings.patch_embedding.weight"] = (d, 3, cfg.patch, cfg.patch)
    s[P_ + "embeddings.position_embedding.weight"] = (cfg.tokens, d)
    for n in ("pre_layrnorm", "post_layernorm"):
        s[P_ + n + ".weight"] = s[P_ + n + ".bias"] = (d,)
    for i in range(cfg.layers):
        l = f"{P_}encoder.layers.{i}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            s[l + f"self_attn.{n}.weight"], s[l + f"self_attn.{n}.bias"] = (d, d), (d,)
        for n in ("layer_norm1", "layer_norm2"):
            s[l + n + ".weight"] = s[l + n + ".bias"] = (d,)
        s[l + "mlp.fc1.weight"], s[l + "mlp.fc1.bias"] = (cfg.mlp, d), (cfg.mlp,)
        s[l + "mlp.fc2.weight"], s[l + "mlp.fc2.bias"] = (d, cfg.mlp), (d,)
    s["visual_projection.weight"] = (cfg.projection, d)
    return s


def config_from_state(state, heads=None):
    """The configuration a file's shapes state.  The head count is not in the file: ``heads`` None means width // 80 for the ViT-H width 1280 and is
    an error otherwise.  Raises ValueError naming the key that does not fit."""
    def need(key, ndim):
        if key not in state:
            raise ValueError(f"ClipVision.load: the file lacks {key}")
        if np.ndim(state[key]) != ndim:
            raise ValueError(f"ClipVision.load: {key} has shape {tuple(np.shape(state[key]))}, expected {ndim} dimensions")
        return tuple(int(v) for v in np.shape(state[key]))
    pw = need(P_ + "embeddings.patch_embedding.weight", 4)
    if pw[1] != 3 or pw[2] != pw[3]:
        raise ValueError(f"ClipVision.load: {P_}embeddings.patch_embedding.weight has shape {pw}, expected (width, 3, P, P)")
    width, patch = pw[0], pw[2]
    pos = need(P_ + "embeddings.position_embedding.weight", 2)
    grid = int(round((pos[0] - 1) ** 0.5))
    if pos[0] < 2 or grid * grid + 1 != pos[0] or pos[1] != width:
        raise ValueError(f"ClipVision.load: {P_}embeddings.position_embedding.weight has shape {pos}: the token count must be (image / patch)^2 + 1 "
                         f"and the width {width}")
    layers = 0
    while f"{P_}encoder.layers.{layers}.mlp.fc1.weight" in state:
        layers += 1
    if layers == 0:
        raise ValueError(f"ClipVision.load: the file lacks {P_}encoder.layers.0.mlp.fc1.weight")
    mlp = need(f"{P_}encoder.layers.0.mlp.fc1.weight", 2)[0]
    proj = need("visual_projection.weight", 2)[0]
    if heads is None:
        if width != 1280:
            raise ValueError(f"ClipVision.load: the head count is not in the file and width {width} is not ViT-H's 1280 -- pass heads=")
        heads = width // 80
    if heads < 1 or width % heads:
        raise ValueError(f"ClipVision.load: heads={heads} does not divide the width {width}")
    return ClipVisionConfig(image=grid * patch, patch=patch, width=width, heads=int(heads), layers=layers, mlp=mlp, projection=proj)


def load_state(src):
    """name -> numpy array of an image-encoder file (``.safetensors`` / ``.bin`` / ``.pt`` through load_checkpoint) or of a dict (flat, or with the
    tensors under "state_dict"), without ``position_ids``; a file that holds a text tower is refused."""
    if isinstance(src, (str, os.PathLike)):
        from ..storage.unpicker import load_checkpoint
        src = load_checkpoint(os.fspath(src))
    if not isinstance(src, dict):
        raise TypeError(f"ClipVision.load: takes a file name or a dict, got {type(src).__name__}")
    if "state_dict" in src and isinstance(src["state_dict"], dict):
        src = src["state_dict"]
    text = sorted(k for k in src if k.startswith("text_model.") or k == "text_projection.weight")
    if text:
        raise ValueError(f"ClipVision.load: this file holds a CLIP text tower ({text[0]}, ...): pass the image encoder's file (CLIPVisionModelWithProjection)")
    return {k: _host(v) for k, v in src.items() if k != P_ + "embeddings.position_ids"}


def _host(v):
    """A file's tensor as a numpy array; a torch bfloat16 tensor (numpy has no such type) goes through float32, exactly."""
    if hasattr(v, "detach"):
        v = v.detach().cpu()
        v = (v.float() if str(v.dtype) == "torch.bfloat16" else v).numpy()
    return np.asarray(v)


def check_state(state, cfg):
    """Every tensor of a loaded file against ``param_shapes(cfg)``: a missing, mis-shaped or surplus key raises naming it.  Host code."""
    want = param_shapes(cfg)
    for key, shape in want.items():
        if key not in state:
            raise ValueError(f"ClipVision.load: the file lacks {key}")
        if tuple(state[key].shape) != shape:
            raise ValueError(f"ClipVision.load: {key} has shape {tuple(state[key].shape)}, this tower needs {shape}")
    extra = sorted(k for k in state if k not in want)
    if extra:
        raise ValueError(f"ClipVision.load: the file holds tensors this tower has no place for: {extra[:4]}")
    return state


class _Holder:
    """A ``weight`` slot update_state fills (the patch embedding's conv weight, the position table)."""

    def __init__(self):
        self.weight = None


class _Embeddings:
    def __init__(self):
        self.class_embedding = None          # (D,): not a weight / bias leaf -- ClipVision.load installs it
        self.patch_embedding = _Holder()     # (D, 3, P, P), stored KRSC; the GEMM reads the packed (D, kpad) copy (ClipVision._patch_weight)
        self.position_embedding = _Holder()  # (T, D)


class VisionEncoderLayer:
    def __init__(self, cfg):
        self.self_attn = CLIPAttention(init=False, embed_dim=cfg.width, num_heads=cfg.heads)
        self.layer_norm1 = LayerNorm(cfg.width, eps=cfg.eps, init=False)
        self.mlp = CLIPMLP(init=False, dim=cfg.width, hidden=cfg.mlp, act="gelu")
        self.layer_norm2 = LayerNorm(cfg.width, eps=cfg.eps, init=False)

    def __call__(self, x):
        x = self.self_attn(x, None, residual=x, ln=self.layer_norm1)
        return self.mlp(x, residual=x, ln=self.layer_norm2)


class _Encoder:
    def __init__(self, cfg):
        self.layers = [VisionEncoderLayer(cfg) for _ in range(cfg.layers)]


class _VisionModel:
    def __init__(self, cfg):
        self.embeddings = _Embeddings()
        self.pre_layrnorm = LayerNorm(cfg.width, eps=cfg.eps, init=False)
        self.encoder = _Encoder(cfg)
        self.post_layernorm = LayerNorm(cfg.width, eps=cfg.eps, init=False)


class ClipVision:
    """``tower = ClipVision.load(file | dict)``; ``tower(images)``: uint8 (N, S, S, 3) pictures, host or device, S = ``cfg.image`` -> the device
    (N, projection) image embeddings in the tower's 16-bit type (the package's config.dtype when the weights were loaded).  Resizing and cropping
    the picture to S x S (CLIP's preprocessing: bicubic resize of the short side, centre crop) is the caller's job; the normalisation is the tower's.

    The first call for a batch size runs launch by launch (twice: see __call__) -- it sets dynamic-LDS function attributes and autotunes GEMM shapes that are not in the
    table, neither of which can happen under capture -- and is then captured into a HIP graph that later calls replay (the pool discipline of
    StableDiffusion._capture: every block the captured tower touches belongs to the graph).  ``eager(images)`` always runs launch by launch.  The
    work runs on the tower's own stream, ordered behind the caller's current stream and in front of what the caller launches next."""

    def __init__(self, cfg=VIT_H):
        if cfg.image % cfg.patch or cfg.width % cfg.heads or cfg.width % 64 or cfg.width > 2560 or cfg.projection % 4:
            raise ValueError(f"ClipVision: unsupported configuration {cfg} (image a multiple of patch, width a multiple of 64 and of heads, <= 2560, "
                             "projection a multiple of 4)")
        self.cfg = cfg
        self.vision_model = _VisionModel(cfg)
        self.visual_projection = Linear(cfg.width, cfg.projection, bias=False, init=False)
        self._stream = None
        self._graphs = {}          # batch size -> (graph, its pool blocks, input buffer, output array)
        self._packed = self._head = None

    @classmethod
    def load(cls, src, heads=None):
        state = load_state(src)
        cfg = config_from_state(state, heads)
        self = cls(cfg)
        check_state(state, cfg)
        update_state(self, state, "")
        self.vision_model.embeddings.class_embedding = asarray(state[P_ + "embeddings.class_embedding"], self.dtype, "row")
        return self

    @property
    def dtype(self):
        w = self.visual_projection.weight
        if w is None:
            raise RuntimeError("ClipVision: the tower has no weights yet (ClipVision.load)")
        return w.dtype

    # -- derived weights, made once per weight set
    def _patch_weight(self):
        w = self.vision_model.embeddings.patch_embedding.weight
        if self._packed is None or self._packed[0] != w.wkey:
            self._packed = (w.wkey, DeviceArray.from_numpy(pack_patch_weight(w.numpy(), self.cfg.kpad), w.dtype, "row"))
        return self._packed[1]

    def _head_folded(self):
        ln, w = self.vision_model.post_layernorm, self.visual_projection.weight
        key = (w.wkey, ln.weight.wkey, ln.bias.wkey)
        if self._head is None or self._head[0] != key:
            self._head = (key, fold_layer_norm(w, None, ln))
        return self._head[1]

    # -- the tower, launch by launch, on the current stream
    def embeddings(self, img):
        """uint8 device (N, S, S, 3) -> (N, T, D): patch matrix, patch-embedding GEMM, then class row | patch rows + position rows + pre_layrnorm."""
        cfg, emb, dt = self.cfg, self.vision_model.embeddings, self.dtype
        if emb.class_embedding is None:
            raise RuntimeError("ClipVision: vision_model.embeddings.class_embedding is not set (ClipVision.load installs it)")
        n, g = img.shape[0], cfg.image // cfg.patch
        patches = DeviceArray.empty((n * g * g, cfg.kpad), dt, "row")
        scale, shift = norm_constants()
        hip.tf_vit_patchify_u8_16(dtag(dt), patches.ptr, img.ptr, n, cfg.image, cfg.patch, cfg.kpad, scale.ctypes.data_as(ctypes.c_void_p),
                                  shift.ctypes.data_as(ctypes.c_void_p), _sh())
        pe = linear_f16(patches, self._patch_weight())
        x = DeviceArray.empty((n, cfg.tokens, cfg.width), dt, "row")
        pre = self.vision_model.pre_layrnorm
        hip.tf_vit_embed_ln_16(dtag(dt), x.ptr, pe.ptr, emb.class_embedding.ptr, emb.position_embedding.weight.ptr, pre.weight.ptr, pre.bias.ptr,
                               n, cfg.tokens, cfg.width, float(cfg.eps), _sh())
        return x

    def hidden(self, img):
        x = self.embeddings(img)
        for layer in self.vision_model.encoder.layers:
            x = layer(x)
        return x

    def pooled(self, x):
        """(N, T, D) last hidden state -> (N, projection): the class rows gathered with one strided copy, then post_layernorm folded into the
        bias-free visual_projection (one tf_linear_ln_16 launch)."""
        cfg, n = self.cfg, x.shape[0]
        rows = DeviceArray.empty((n, cfg.width), x.dtype, "row")
        hip.tf_memcpy_2d_async(rows.ptr, cfg.width * 2, x.ptr, cfg.tokens * cfg.width * 2, cfg.width * 2, n, _sh())
        return linear_ln_f16(rows, self._head_folded(), self.vision_model.post_layernorm.eps)

    def _forward(self, img):
        return self.pooled(self.hidden(img))

    # -- public calls
    def check_images(self, images):
        from ..variants.inputs import u8_image
        s = self.cfg.image
        return u8_image(images, f"ClipVision: images must be uint8 (N, {s}, {s}, 3) with N >= 1 (resize and crop to {s} x {s} first)", (s, s))

    def _enter(self):
        ensure_init()
        if self._stream is None:
            self._stream = Stream()
        return use_stream(self._stream)

    @staticmethod
    def _fill(buf, images):
        if isinstance(images, DeviceArray):
            hip.tf_memcpy_async(buf.ptr, images.ptr, buf.nbytes, 3, _sh())
        else:
            buf.copy_from_numpy(images)
        return buf

    def eager(self, images):
        images, ish = self.check_images(images)
        if ish[0] < 1:
            raise ValueError("ClipVision: an empty image batch")
        with self._enter():
            img = self._fill(DeviceArray.empty(ish, np.uint8, "row"), images)
            return self._forward(img)

    def __call__(self, images):
        images, ish = self.check_images(images)
        n = ish[0]
        if n < 1:
            raise ValueError("ClipVision: an empty image batch")
        with self._enter():
            if n not in self._graphs:
                buf = self._fill(DeviceArray.empty(ish, np.uint8, "row"), images)
                # two eager passes, as StableDiffusion._warm_up has them: the first builds the lazily derived weights (packed patch weight, fused and
                # folded q|k|v / fc1 / head) -- persistent allocations that take blocks the pass itself has just freed -- tunes and sets attributes; the
                # second allocates and frees activations only, which is exactly what the frozen pool must hold for the capture
                self._forward(buf)
                first = self._forward(buf)
                res = DeviceArray.empty(first.shape, first.dtype, "row")
                hip.tf_memcpy_async(res.ptr, first.ptr, first.nbytes, 3, _sh())
                del first                                  # (back to the pool: the capture allocates exactly what the eager run freed)
                self._stream.synchronize()
                self._graphs[n] = self._capture(buf)
                return res
            graph, _, buf, out = self._graphs[n]
            self._fill(buf, images)
            hip.tf_graph_launch(graph, self._stream.handle)
            res = DeviceArray.empty(out.shape, out.dtype, "row")
            hip.tf_memcpy_async(res.ptr, out.ptr, out.nbytes, 3, _sh())
            return res

    def _capture(self, buf):
        pool().begin_capture()
        g, ok, out = ctypes.c_void_p(), False, None
        try:
            hip.tf_graph_begin_capture(self._stream.handle)
            out = self._forward(buf)
            hip.tf_graph_end_capture(self._stream.handle, ctypes.byref(g))
            ok = True
        finally:
            blocks = pool().end_capture()
            if not ok:
                hip.tf_graph_abort_capture(self._stream.handle)
                out = None                                 # (dropped while the pool still owns its block: released once, by disown)
                pool().disown(blocks)
        return g, blocks, buf, out

    def release_graphs(self):
        """Destroy the captured graphs and hand their blocks back to the pool (the next call of a batch size captures again)."""
        while self._graphs:
            g, blocks, buf, out = self._graphs.popitem()[1]
            hip.tf_graph_destroy(g)
            # the output block belongs to the graph: let go of it while the pool still owns it (its finalizer is then a no-op) and hand every
            # block back exactly once through disown -- the other order would put it on the free list twice
            del buf, out
            pool().disown(blocks)


def synthetic_state(cfg, seed=0, scale=None):
    """Seeded weights of a tower of that configuration in the file's names (fp16 values as fp32 arrays): what example/sd1.py and
    tools/sampler_bench.py run without a file.  The matrices are scaled so that activations stay of order one through the layers."""
    rng = np.random.default_rng(seed)
    out = {}
    for k, s in param_shapes(cfg).items():
        if k.endswith("norm.weight") or k.endswith("norm1.weight") or k.endswith("norm2.weight"):
            a = 1.0 + 0.05 * rng.standard_normal(s)
        elif k.endswith(".bias") or k.endswith("class_embedding") or k.endswith("position_embedding.weight"):
            a = 0.05 * rng.standard_normal(s)
        else:
            fan_in = int(np.prod(s[1:]))
            a = rng.standard_normal(s) * ((scale if scale is not None else 0.7) / np.sqrt(fan_in))
        out[k] = a.astype(np.float16).astype(np.float32)
    return out
