"""CPU restatement of the CLIP ViT image tower with projection (``CLIPVisionModelWithProjection``) on the file's tensors, for the tests of
tinyfusers_amd/vae/clip_vision.py.  Host code: numpy + torch on the CPU; nothing of the product is imported.

What the tower adds to the text tower is restated in float64: the CLIP normalisation, the patch embedding as a STRIDED CONVOLUTION on the file's
(width, 3, P, P) weight (so a column-order mistake of the product's patch matrix / packed weight shows), the class row and position rows, every
LayerNorm, the exact GELU (the error function on double, in its erfc form: 1 + erf(x / sqrt 2) cancels in the negative tail, which is what the
kernel's erfc form avoids too) and the pooled head.  The attention and the Linears are the oracle's own pieces (oracle.clip.clip_attention, oracle.ops.linear), which
compute in float32, unmasked."""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import clip as OC  # noqa: E402
from oracle import ops  # noqa: E402

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
P_ = "vision_model."
TINY = dict(image=56, patch=14, width=320, heads=4, layers=2, mlp=1280, projection=32)
VIT_H = dict(image=224, patch=14, width=1280, heads=16, layers=32, mlp=5120, projection=1024)


def vision_param_shapes(cfg):
    d, s = cfg["width"], {}
    tokens = (cfg["image"] // cfg["patch"]) ** 2 + 1
    s[P_ + "embeddings.class_embedding"] = (d,)
    s[P_ + "embeddings.patch_embedding.weight"] = (d, 3, cfg["patch"], cfg["patch"])
    s[P_ + "embeddings.position_embedding.weight"] = (tokens, d)
    s[P_ + "pre_layrnorm.weight"] = s[P_ + "pre_layrnorm.bias"] = (d,)
    for i in range(cfg["layers"]):
        l = f"{P_}encoder.layers.{i}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            s[l + f"self_attn.{n}.weight"] = (d, d)
            s[l + f"self_attn.{n}.bias"] = (d,)
        for n in ("layer_norm1", "layer_norm2"):
            s[l + n + ".weight"] = s[l + n + ".bias"] = (d,)
        s[l + "mlp.fc1.weight"], s[l + "mlp.fc1.bias"] = (cfg["mlp"], d), (cfg["mlp"],)
        s[l + "mlp.fc2.weight"], s[l + "mlp.fc2.bias"] = (d, cfg["mlp"]), (d,)
    s[P_ + "post_layernorm.weight"] = s[P_ + "post_layernorm.bias"] = (d,)
    s["visual_projection.weight"] = (cfg["projection"], d)
    return s


def make_weights(cfg, seed=3):
    """Seeded fp16 tensors under the file's names: matrices at 0.7 / sqrt(fan in), LayerNorm weights around 1, biases and embeddings small."""
    rng = np.random.default_rng(seed)
    W = {}
    for k, s in vision_param_shapes(cfg).items():
        if "norm" in k and k.endswith(".weight"):
            a = 1.0 + 0.1 * rng.standard_normal(s)
        elif k.endswith(".bias") or "class_embedding" in k or "position_embedding" in k:
            a = 0.1 * rng.standard_normal(s)
        else:
            a = rng.standard_normal(s) * (0.7 / math.sqrt(int(np.prod(s[1:]))))
        W[k] = a.astype(np.float16)
    return W


def _d(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float64))


def layer_norm64(x, w, b, eps=1e-5):
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * _d(w) + _d(b)


def gelu64(x):
    x = x.double()
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))          # = 0.5 x (1 + erf(x / sqrt 2)), without its cancellation for x < 0


def normalise(images_u8):
    """uint8 (N, S, S, 3) -> float64 (N, 3, S, S): (x / 255 - mean) / std."""
    x = torch.as_tensor(np.asarray(images_u8)).double() / 255.0
    return ((x - _d(CLIP_MEAN)) / _d(CLIP_STD)).permute(0, 3, 1, 2).contiguous()


def patch_embed(images_u8, W, cfg):
    """(N, g^2, D): the stride-P, bias-free convolution of the normalised image with the file's weight, rows in (py, px) order."""
    y = torch.nn.functional.conv2d(normalise(images_u8), _d(W[P_ + "embeddings.patch_embedding.weight"]), stride=cfg["patch"])
    return y.flatten(2).transpose(1, 2)


def embeddings(images_u8, W, cfg):
    pe = patch_embed(images_u8, W, cfg)
    n = pe.shape[0]
    cls = _d(W[P_ + "embeddings.class_embedding"]).expand(n, 1, -1)
    x = torch.cat([cls, pe], dim=1) + _d(W[P_ + "embeddings.position_embedding.weight"])[None]
    return layer_norm64(x, W[P_ + "pre_layrnorm.weight"], W[P_ + "pre_layrnorm.bias"])


def encoder_layer(x, W, p, heads):
    h = layer_norm64(x, W[p + "layer_norm1.weight"], W[p + "layer_norm1.bias"])
    x = x.double() + OC.clip_attention(h, W, p + "self_attn.", None, heads).double()
    h = layer_norm64(x, W[p + "layer_norm2.weight"], W[p + "layer_norm2.bias"])
    h = gelu64(ops.linear(h, W[p + "mlp.fc1.weight"], W[p + "mlp.fc1.bias"]))
    return x + ops.linear(h, W[p + "mlp.fc2.weight"], W[p + "mlp.fc2.bias"]).double()


def hidden(images_u8, W, cfg):
    x = embeddings(images_u8, W, cfg)
    for i in range(cfg["layers"]):
        x = encoder_layer(x, W, f"{P_}encoder.layers.{i}.", cfg["heads"])
    return x


def pooled(x, W):
    h = layer_norm64(x[:, 0], W[P_ + "post_layernorm.weight"], W[P_ + "post_layernorm.bias"])
    return h @ _d(W["visual_projection.weight"]).t()


def forward(images_u8, W, cfg):
    """uint8 (N, S, S, 3) -> float64 (N, projection) image embeddings."""
    return pooled(hidden(images_u8, W, cfg), W)
