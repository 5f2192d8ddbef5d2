"""The reference's vae/encoder.py: the VAE Encoder (:12-34; nothing on the sampler's path uses it -- AutoencoderKL.__call__ does) and the CLIP
text encoder (:36-81: CLIPEncoder, CLIPEncoderLayer, CLIPTextEmbeddings, CLIPTextTransformer).

Produces the (B, 77, 768) contexts the UNet's cross-attention reads (example/sd1.py:46-49).  Per layer: 5 launches of
the UNet's own kernels -- LN1 folded into the fused q|k|v GEMM, causal SDPA (d = 64, LDS-DMA kernel), out_proj + residual,
LN2 folded into fc1, quick-GELU, fc2 + residual."""
import numpy as np

from ..attention.attention import CLIPAttention
from ..ff.embedding import Embedding, embedding
from ..ff.layer_norm import LayerNorm
from ..ff.nn import CLIPMLP
from ..native import hip
from ..storage.tensor import DeviceArray, _sh, bfloat16, dtag, is_bfloat16


ENCODER_WIDTHS = ((128, 128), (128, 256), (256, 512), (512, 512))     # (in, out) channels of encoder level 0 (image resolution) .. 3


class Encoder:
    """vae/encoder.py:12-34.  Attribute tree = checkpoint keys: ``conv_in``, ``down.<level>.block.<0..1>``, ``down.<level>.downsample.conv``
    (levels 0..2), ``mid``, ``norm_out``, ``conv_out``.  A level runs two ResnetBlocks and, except for the last, halves the resolution with a
    stride-2 3x3 conv whose padding is [0, 1, 0, 1] -- one pixel on the right and at the bottom only (the LDM form; the reference hands that
    list to its conv as ``padding``), here an explicit zero pad followed by an unpadded conv (vision/conv2d.py::pad_image).  The output has
    8 channels: means and log-variances of the latent."""

    def __init__(self, init=True):
        from ..ff.group_norm import GroupNorm
        from ..vision.conv2d import Conv2d
        from ..vision.resnet import ResnetBlock
        from .mid import Mid
        self.conv_in = Conv2d(3, 128, kernel_size=[3, 3], padding=[1, 1], init=init)
        self.down = []
        for i, (cin, cout) in enumerate(ENCODER_WIDTHS):
            level = {"block": [ResnetBlock(cin, cout, init=init), ResnetBlock(cout, cout, init=init)]}
            if i != len(ENCODER_WIDTHS) - 1:
                level["downsample"] = {"conv": Conv2d(cout, cout, kernel_size=[3, 3], stride=[2, 2], padding=[0, 1, 0, 1], init=init)}
            self.down.append(level)
        top = ENCODER_WIDTHS[-1][1]
        self.mid = Mid(top, init=init)
        self.norm_out = GroupNorm(32, top, init=init)
        self.conv_out = Conv2d(top, 8, kernel_size=[3, 3], padding=[1, 1], init=init)

    def __call__(self, x):
        x = self.conv_in(x)
        for level in self.down:
            for block in level["block"]:
                x = block(x)
            if "downsample" in level:
                x = level["downsample"]["conv"](x)
        x = self.mid(x)
        return self.conv_out(self.norm_out(x, silu=True))


class CLIPEncoderLayer:
    def __init__(self, init=True, width=768, heads=12, mlp=3072):
        self.self_attn = CLIPAttention(init=init, embed_dim=width, num_heads=heads)
        self.layer_norm1 = LayerNorm(width, init=init)
        self.mlp = CLIPMLP(init=init, dim=width, hidden=mlp)
        self.layer_norm2 = LayerNorm(width, init=init)

    def __call__(self, hidden_states, causal_attention_mask):
        hidden_states = self.self_attn(hidden_states, causal_attention_mask, residual=hidden_states, ln=self.layer_norm1)
        return self.mlp(hidden_states, residual=hidden_states, ln=self.layer_norm2)


class CLIPEncoder:
    def __init__(self, init=True, layers=12, width=768, heads=12, mlp=3072):
        self.layers = [CLIPEncoderLayer(init=init, width=width, heads=heads, mlp=mlp) for i in range(layers)]

    def __call__(self, hidden_states, causal_attention_mask, layers=None):
        """layers: run the first ``layers`` layers only (None: all of them)."""
        for l in self.layers[:layers]:
            hidden_states = l(hidden_states, causal_attention_mask)
        return hidden_states


class CLIPTextEmbeddings:
    def __init__(self, init=True, vocab=49408, width=768, positions=77):
        self.token_embedding = Embedding(vocab, width, init=init)
        self.position_embedding = Embedding(positions, width, init=init)

    def __call__(self, input_ids, position_ids=None):
        """position_ids: None or arange(T) (all the reference passes, vae/encoder.py:78): row i is added to token i."""
        if position_ids is not None:
            p = np.asarray(position_ids).reshape(-1)
            assert (p == np.arange(p.size)).all(), "position_ids must be arange(T)"
        w, pos = self.token_embedding.weight, self.position_embedding.weight
        if not is_bfloat16(w.dtype):
            return embedding(w, input_ids, pos)
        # bfloat16 weights (the SDXL towers under config.set_dtype("bf16")): the gather copies the rows' bits, one tf_add_16 per sequence adds the
        # positions -- vae/open_clip_text.py::OpenClipText.embeddings' form
        rows = embedding(w, input_ids)
        b, t, d = rows.shape
        x = DeviceArray.empty((b, t, d), bfloat16, "row")
        for k in range(b):
            hip.tf_add_16(dtag(bfloat16), x.ptr + k * t * d * 2, rows.ptr + k * t * d * 2, pos.ptr, t * d, _sh())
        x._base = rows                                                       # (referenced until the adds have run)
        return x


class CLIPTextTransformer:
    """tap = k: the output of encoder layer k (the first k layers run) WITHOUT final_layer_norm -- SDXL reads CLIP-L at k = 11 of 12, transformers'
    ``hidden_states[-2]``; None: every layer and the final LayerNorm, the SD-1.x context.  The shape arguments default to CLIP ViT-L/14's."""

    def __init__(self, init=True, tap=None, width=768, layers=12, heads=12, mlp=3072, vocab=49408, positions=77):
        if tap is not None and not 1 <= int(tap) <= layers:
            raise ValueError(f"CLIPTextTransformer: tap={tap!r} names no encoder layer (1 .. {layers}, or None)")
        self._tap = None if tap is None else int(tap)
        self.embeddings = CLIPTextEmbeddings(init=init, vocab=vocab, width=width, positions=positions)
        self.encoder = CLIPEncoder(init=init, layers=layers, width=width, heads=heads, mlp=mlp)
        self.final_layer_norm = LayerNorm(width, init=init)

    def __call__(self, input_ids):
        """input_ids: (B, T <= 77) integer token ids (host array or int32 DeviceArray) -> (B, T, 768) f16 context."""
        t = input_ids.shape[1]
        x = self.embeddings(input_ids)
        mask = np.triu(np.full((1, 1, t, t), float("-inf"), dtype=np.float32), k=1)       # vae/encoder.py:79
        if self._tap is not None:
            return self.encoder(x, mask, layers=self._tap)
        x = self.encoder(x, mask)
        return self.final_layer_norm(x)
