"""IP-Adapter for SD-1.5 (``ip-adapter_sd15``; Ye et al. 2023): image prompts through decoupled cross-attention.  The adapter never touches the
UNet's weights: it owns an image projection (Linear E -> T x context_dim, LayerNorm over each of the T tokens) and one ``(to_k_ip, to_v_ip)`` pair
of bias-free Linears per cross-attention; each cross-attention adds ``s softmax(q K_ip^T / sqrt d) V_ip`` to its output, inside its one attention
launch (tf_sdpa_dual_16, CrossAttention(..., ip=)).

File format, as published (no adapter file exists on the development machines: names and order are stated from the published format and pinned
by tests/test_ip_adapter_host.py on files the test writes).  Flat ``.safetensors``: ``image_proj.proj.{weight,bias}`` (T x ctx, E) / (T x ctx),
``image_proj.norm.{weight,bias}`` (ctx), ``ip_adapter.{n}.to_k_ip.weight`` / ``ip_adapter.{n}.to_v_ip.weight`` (C, ctx), n = 1, 3, ..., odd.  The
``.bin`` layout is a torch-zip holding the same names nested under ``"image_proj"`` and ``"ip_adapter"``.  The odd indices follow the diffusers
attention-processor order DOWN, UP, MID -- for SD-1.5 input_blocks 1, 2, 4, 5, 7, 8 -> 1 ... 11, output_blocks 3 ... 11 -> 13 ... 29, middle_block
-> 31 -- which is NOT the order StepModel._all walks (input, middle, output): ``adapter_paths`` builds the table from the module tree explicitly.
The "plus" (Resampler: ``image_proj.latents``) and FaceID families are refused by name."""
import os

import numpy as np

from ..ff.layer_norm import LayerNorm
from ..ff.linear import Linear, linear_f16
from .state import update_state

MAX_TOKENS = 64            # one key tile of the dual attention launch


class UnsupportedAdapter(ValueError):
    pass


def adapter_paths(unet):
    """[(n, module path, SpatialTransformer)] for every cross-attention of ``unet`` in the adapter's order: input blocks, output blocks, then the
    middle block; n = 1, 3, 5, ... ."""
    from ..attention.attention import SpatialTransformer
    found = []
    for part in ("input_blocks", "output_blocks"):
        for i, blk in enumerate(getattr(unet, part)):
            for j, bb in enumerate(blk):
                if isinstance(bb, SpatialTransformer):
                    found.append((f"{part}.{i}.{j}", bb))
    for j, bb in enumerate(unet.middle_block):
        if isinstance(bb, SpatialTransformer):
            found.append((f"middle_block.{j}", bb))
    return [(2 * k + 1, path, st) for k, (path, st) in enumerate(found)]


def _flat(obj):
    """The flat name -> array dict of either published layout."""
    if "image_proj" in obj and "ip_adapter" in obj and isinstance(obj["image_proj"], dict):
        flat = {f"image_proj.{k}": v for k, v in obj["image_proj"].items()}
        flat.update({f"ip_adapter.{k}": v for k, v in obj["ip_adapter"].items()})
        return flat
    return dict(obj)


def load_ip_adapter(src):
    """name -> numpy array of an ``ip-adapter_sd15`` file (``.safetensors`` flat, ``.bin`` / ``.pt`` torch-zip nested) or of a dict in either
    layout, through storage/unpicker.py::load_checkpoint.  Other adapter families raise UnsupportedAdapter naming the family."""
    if isinstance(src, (str, os.PathLike)):
        from .unpicker import load_checkpoint
        src = load_checkpoint(os.fspath(src))
    if not isinstance(src, dict):
        raise TypeError(f"load_ip_adapter: takes a file name or a dict, got {type(src).__name__}")
    flat = {k: np.asarray(v.numpy() if hasattr(v, "numpy") and not isinstance(v, np.ndarray) else v) for k, v in _flat(src).items()}
    names = set(flat)
    if any(k.startswith(("image_proj.latents", "image_proj.proj_in.", "image_proj.layers.")) for k in names):
        raise UnsupportedAdapter("load_ip_adapter: this is an IP-Adapter 'plus' file (Resampler image projection, image_proj.latents): the plus family is unsupported")
    if any("lora" in k or k.startswith(("image_proj.proj.0.", "image_proj.perceiver_resampler.")) for k in names):
        raise UnsupportedAdapter("load_ip_adapter: this is an IP-Adapter FaceID / full-face file (MLP image projection or LoRA weights): the FaceID family is unsupported")
    need = {"image_proj.proj.weight", "image_proj.proj.bias", "image_proj.norm.weight", "image_proj.norm.bias"}
    if not need <= names or not any(k.startswith("ip_adapter.") for k in names):
        raise UnsupportedAdapter(f"load_ip_adapter: not an ip-adapter_sd15 file: missing {sorted(need - names) or 'ip_adapter.*'}")
    return flat


class _Pair:
    def __init__(self, ctx, c):
        self.to_k_ip = Linear(ctx, c, bias=False, init=False)
        self.to_v_ip = Linear(ctx, c, bias=False, init=False)


class _ImageProj:
    def __init__(self, embed_dim, tokens, ctx):
        self.proj = Linear(embed_dim, tokens * ctx, init=False)
        self.norm = LayerNorm(ctx, init=False)


class IPAdapter:
    """The adapter's modules for one UNet: ``image_proj`` and ``ip_adapter[str(n)]`` pairs, named as the file names them (update_state fills
    them).  ``IPAdapter.load(unet, file | dict)`` reads T and E from the file and checks every shape against the UNet, naming the key."""

    def __init__(self, unet, num_tokens=4, embed_dim=1024):
        if not 1 <= int(num_tokens) <= MAX_TOKENS:
            raise UnsupportedAdapter(f"IPAdapter: {num_tokens} image tokens: the attention launch takes 1 .. {MAX_TOKENS}")
        self.num_tokens, self.embed_dim, self.context_dim = int(num_tokens), int(embed_dim), unet.cfg.context_dim
        self.image_proj = _ImageProj(self.embed_dim, self.num_tokens, self.context_dim)
        self.paths = [(n, path) for n, path, _ in adapter_paths(unet)]
        self.ip_adapter = {str(n): _Pair(self.context_dim, st.proj_in._shape[0])
                           for n, _, st in adapter_paths(unet)}
        self._kv = None

    def expected_shapes(self):
        t, e, c = self.num_tokens, self.embed_dim, self.context_dim
        shapes = {"image_proj.proj.weight": (t * c, e), "image_proj.proj.bias": (t * c,), "image_proj.norm.weight": (c,), "image_proj.norm.bias": (c,)}
        for n, pair in self.ip_adapter.items():
            shapes[f"ip_adapter.{n}.to_k_ip.weight"] = shapes[f"ip_adapter.{n}.to_v_ip.weight"] = (pair.to_k_ip.out_features, c)
        return shapes

    @staticmethod
    def token_count(unet, state):
        """(T, E) read from image_proj.proj.weight (T x context_dim, E)."""
        ctx, w = unet.cfg.context_dim, state["image_proj.proj.weight"]
        if w.ndim != 2 or w.shape[0] % ctx or w.shape[0] == 0:
            raise ValueError(f"IPAdapter.load: image_proj.proj.weight {tuple(w.shape)} is not (T x {ctx}, E) for this UNet's context width")
        return w.shape[0] // ctx, w.shape[1]

    def check(self, state):
        """Every tensor of a loaded file against this adapter's shapes -- a missing, mis-shaped or surplus key raises naming it.  Host code."""
        want = self.expected_shapes()
        for key, shape in want.items():
            if key not in state:
                raise ValueError(f"IPAdapter.load: the file lacks {key} (this UNet has {len(self.ip_adapter)} cross-attentions)")
            if tuple(state[key].shape) != shape:
                raise ValueError(f"IPAdapter.load: {key} has shape {tuple(state[key].shape)}, this UNet needs {shape}")
        extra = sorted(k for k in state if k not in want)
        if extra:
            raise ValueError(f"IPAdapter.load: the file holds tensors this UNet has no place for: {extra[:4]}")
        return state

    @classmethod
    def load(cls, unet, src):
        state = load_ip_adapter(src)
        self = cls(unet, *cls.token_count(unet, state))
        update_state(self, self.check(state), "")
        return self

    # -- device side, in the step's 16-bit type
    def tokens(self, embeds):
        """image embeddings (N, E) -> the image tokens (N, T, context_dim): Linear, then LayerNorm over each token."""
        n, e = embeds.shape
        assert e == self.embed_dim, (embeds.shape, self.embed_dim)
        x = self.image_proj.proj(embeds)
        return self.image_proj.norm(x.view((n, self.num_tokens, self.context_dim), "row"))

    def _prepare(self):
        from ..attention.attention import _concat_rows
        ws = [w for p in self.ip_adapter.values() for w in (p.to_k_ip.weight, p.to_v_ip.weight)]
        key = tuple(w.wkey for w in ws)
        if self._kv is None or self._kv[0] != key:
            offs, off = [], 0
            for p in self.ip_adapter.values():
                offs.append(off)
                off += 2 * p.to_k_ip.out_features
            self._kv = (key, _concat_rows(ws), offs, off)
        return self._kv

    def context_kv(self, tokens):
        """Every block's K_ip | V_ip of the image tokens as ONE GEMM over the row-concatenated weights (the twin of StepModel.context_kv):
        (N, T, kv_n); block k's columns start at ``kv_layout()[0][k]``."""
        return linear_f16(tokens, self._prepare()[1])

    def kv_layout(self):
        """(column offset of every block's k | v in adapter order, kv_n)."""
        _, _, offs, kv_n = self._prepare()
        return offs, kv_n
