"""ControlNet for the SD-1.x UNet (Zhang et al. 2023; the ``control_model.*`` tensors of a control_*_sd15_* / control_v11*_sd15_* checkpoint).

A second copy of the UNet's encoder half -- time_embed, input_blocks and middle_block of vision/unet.py, built from the same plan and walked
by the same code -- that reads the latent plus an embedding of the hint image, and hands back one residual per skip connection and one for the
middle block's output, each through a 1x1 "zero" convolution.  UNetModel.__call__(control=...) adds them (vision/unet.py: control_add).
Attribute names are the LDM checkpoint's, so ``update_state(net, W, "control_model.")`` walks a real file.
"""
from ..native import hip
from ..storage.tensor import DeviceArray, Tensor, _sh, is_bfloat16
from .conv2d import Conv2d
from .unet import SD15, StepModel, UNetConfig, encoder_plan

# the hint stem: eight 3x3 convolutions (pad 1), three of them stride 2 -- an (8h, 8w) image comes down to the latent's (h, w).
# (cin, cout, stride); the last conv's cout is the model's width.  The same 16 / 32 / 96 / 256 plan for every configuration
_HINT_PLAN = ((None, 16, 1), (16, 16, 1), (16, 32, 2), (32, 32, 1), (32, 96, 2), (96, 96, 1), (96, 256, 2), (256, None, 1))


def _silu(x):
    out = DeviceArray.empty(x.shape, x.dtype, x.layout)
    (hip.tf_silu_bf16 if is_bfloat16(x.dtype) else hip.tf_silu_f16)(out.ptr, x.ptr, x.size, _sh())
    return out


class ControlNet(StepModel):
    def __init__(self, cfg: UNetConfig = SD15, hint_channels=3, init=False):
        self.cfg = cfg
        mc = cfg.model_channels
        self.time_embed, self.input_blocks, self.middle_block, chans = encoder_plan(cfg, 4, init)       # the latent alone: in_channels 4
        self.input_hint_block = []                       # convs at 0, 2, ..., 14; SiLU between them
        for ci, co, st in _HINT_PLAN:
            if self.input_hint_block:
                self.input_hint_block.append(Tensor.silu)
            self.input_hint_block.append(Conv2d(ci or hint_channels, co or mc, kernel_size=[3, 3], stride=[st, st], padding=[1, 1], init=init))
        self.zero_convs = [[Conv2d(c, c, kernel_size=[1, 1], init=init)] for c in chans]                # one per input block
        self.middle_block_out = [Conv2d(chans[-1], chans[-1], kernel_size=[1, 1], init=init)]
        self._batched = None

    def hint_embedding(self, hint):
        """hint: 16-bit NHWC (b, hint_channels, 8h, 8w) in [0, 1] -> the stem's (b, model_channels, h, w) output.  Depends on the hint alone: a
        sampler runs it once per image, outside the captured step (the first conv, Cin = 3, goes down the small-channel im2col path)."""
        x = hint
        for m in self.input_hint_block:
            x = m(x) if isinstance(m, Conv2d) else _silu(x)
        return x

    def __call__(self, x, hint_emb, timesteps=None, context=None, shared=None):
        """x: the NHWC latent the UNet reads (CFG-stacked); hint_emb: hint_embedding's output, one row per image of x.  Returns the
        len(input_blocks) + 1 residuals: zero conv i of input block i's output, then middle_block_out of the middle block's.
        h = conv_in(x) + hint_emb rides in the conv's epilogue.  ``shared`` as UNetModel's: (emb, this model's time-embedding row, this
        model's K|V projection of the context)."""
        emb, emb_all, kv_all, br = self._shared(timesteps, context, shared)
        run = self._runner(emb, emb_all, kv_all, context)
        h, saved = self._encode(run, x, br, concat_stats=False, residual=hint_emb)
        return [zc[0](s) for zc, s in zip(self.zero_convs, saved)] + [self.middle_block_out[0](h)]
