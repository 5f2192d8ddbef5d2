#!/usr/bin/env python3
"""Sampler driver -- mirrors example/sd1.py:34-79 of the reference: load weights, run the prompt's token ids through the
CLIP text encoder for the two contexts (:44-49), timesteps = range(1,1000,1000//steps), reversed loop, VAE decode.
No checkpoint or BPE vocabulary exists offline, so by default the weights are the seeded synthetic ones and
the "prompt" is a seeded list of token ids; ``--ckpt file.ckpt|file.safetensors`` reads real LDM weights through
storage/unpicker.py + update_state instead (example/sd1.py:40-41), ``--vocab bpe_simple_vocab_16e6.txt.gz --prompt "..."``
tokenizes a real prompt (tokenizer/clip.py).
BASELINE config 3: full 50-step sampler, batch 1, end-to-end img/s.

    python -m example.sd1 --steps 50 [--ckpt sd-v1-4.ckpt] [--out rendered.npy]
    python -m example.sd1 --steps 20 --sampler dpmpp2m          # DPM-Solver++(2M); also ddim, ddim-eta, euler-a (--eta)
    python -m example.sd1 --steps 20 --sampler dpmpp2m --init-image x.npy --strength 0.6 [--mask m.npy]   # img2img / inpainting
    python -m example.sd1 --steps 20 --sampler dpmpp2m --concat inpaint --cond-image x.npy --cond-mask m.npy   # the 9-channel inpainting UNet
    python -m example.sd1 --steps 20 --sampler dpmpp2m --concat edit --cond-image x.npy [--image-guidance 1.5]   # InstructPix2Pix (8 channels)
    python -m example.sd1 --steps 20 --sampler dpmpp2m --control-image edges.npy [--control-ckpt control_v11p_sd15_canny.safetensors] [--control-scale 1.0]   # ControlNet
    python -m example.sd1 --steps 20 --sampler dpmpp2m --lora style.safetensors:0.8 --lora lcm.safetensors:1:0   # LoRA adapters, FILE[:w[:w_te]], merged on the device
    python -m example.sd1 --steps 4 --sampler lcm --no-cfg --lora lcm.safetensors:1:0   # few-step sampling: the LCM sampler on the guidance-free single-branch step
    python -m example.sd1 --steps 20 --sampler dpmpp2m --freeu 0.9,0.2,1.5,1.6   # FreeU: s1,s2,b1,b2 (the values usually quoted for SD-1.5)
    python -m example.sd1 --steps 20 --sampler dpmpp2m --pag 3.0 --pag-layers mid   # perturbed-attention guidance next to CFG (with --no-cfg: instead of it)
    python -m example.sd1 --steps 20 --sampler dpmpp2m --ip-adapter ip-adapter_sd15.safetensors --ip-embeds e.npy [--ip-scale 0.6]   # IP-Adapter: an image prompt, as CLIP image embeddings (1, 1024)
    python -m example.sd1 --steps 20 --sampler dpmpp2m --ip-adapter ip-adapter_sd15.safetensors --ip-image x.npy [--clip-vision image_encoder.safetensors]   # ... or as the picture itself, uint8 (224, 224, 3): the CLIP ViT-H tower runs on the device
    python -m example.sd1 --sd2 --steps 20 --sampler dpmpp2m --prediction v --cfg-rescale 0.7   # Stable Diffusion 2.x: OpenCLIP context, heads of 64, v-prediction, CFG rescale
    python -m example.sd1 --ckpt v2-1_768-ema-pruned.safetensors --steps 20 --sampler dpmpp2m --prediction v --cfg-rescale 0.7   # ... from a checkpoint (768-v: --prediction v)
    python -m example.sd1 --sdxl --steps 20 --sampler dpmpp2m [--ckpt sd_xl_base_1.0.safetensors] [--size 1024]   # SDXL base: two text towers, pooled / size conditioning
    python -m example.sd1 --steps 20 --sampler dpmpp2m --motion [mm_sd_v15_v2.ckpt] --frames 16 [--motion-scale 1.0] [--size 512] --out frames.npy   # AnimateDiff: one 16-frame video, (F, H, W, 3) uint8
With --ckpt the configuration is read off the checkpoint: its conv_in (4, 9 or 8 input channels), and SD-2.x when the cross-attention keys read a
1024-wide context; --concat / --sd2 pick it on synthetic weights.  The parameterisation is NOT in the file: --prediction defaults to eps.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

def run_sdxl(ap, args):
    """--sdxl: text to image on the SDXL base model -- both towers, start(pooled=, original_size=, crop_top_left=, target_size=), the sampler, the VAE
    at latent_scale 0.13025.  Token ids stand in for the two tokenizers' output when there is no --vocab (both towers read CLIP's BPE; bigG pads with 0)."""
    import contextlib
    import io
    if not args.sampler:
        ap.error("--sdxl needs --sampler (the time-embedding rows of an SDXL model are built in start())")
    for flag, name in ((args.concat, "--concat"), (args.control_image, "--control-image"), (args.lora, "--lora"), (args.ip_adapter is not None, "--ip-adapter"),
                       (args.freeu is not None, "--freeu"), (args.pag is not None, "--pag"), (args.init_image, "--init-image"), (args.sd2, "--sd2")):
        if flag:
            ap.error(f"{name} with --sdxl is not supported by this example")
    if args.size < 64 or args.size % 64:
        ap.error(f"--size {args.size}: expected a positive multiple of 64")
    import tinyfusers_amd.storage.tensor as T
    from tinyfusers_amd.storage.state import param_shapes, update_state
    from tinyfusers_amd.storage.synth import synth_state_dict
    from tinyfusers_amd.variants.samplers import make
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vae.open_clip_text import synthetic_state
    from tinyfusers_amd.vision.unet import SDXL
    t0 = time.time()
    T.ensure_init(0)
    model = StableDiffusion(SDXL)
    big_g = "conditioner.embedders.1.model."
    if args.ckpt:
        from tinyfusers_amd.storage.unpicker import load_checkpoint
        state = load_checkpoint(args.ckpt)
        if "model.diffusion_model.label_emb.0.0.weight" not in state:
            sys.exit("--ckpt: the file holds no model.diffusion_model.label_emb.* tensors -- not an SDXL base checkpoint")
    else:
        state = synth_state_dict({k: v for k, v in param_shapes(model).items() if not k.startswith(big_g)}, 0)
        state.update(synthetic_state(model.conditioner.embedders[1].cfg, 0, big_g, pooled=True))
    with contextlib.redirect_stdout(io.StringIO()):
        update_state(model, state, "")
    del state
    print(f"weights installed in {time.time() - t0:.1f}s")
    if args.vocab:
        from tinyfusers_amd.tokenizer.clip import ClipTokenizer
        tok = ClipTokenizer(args.vocab)
        ids = [np.array([tok.encode(p, pad_id=pad)]) for p in (args.prompt, "") for pad in (None, 0)]
    else:
        rng = np.random.default_rng(args.seed)
        prompt = np.full((1, 77), 49407, dtype=np.int64); prompt[0, 0] = 49406; prompt[0, 1:10] = rng.integers(0, 49406, 9)
        empty = np.full((1, 77), 49407, dtype=np.int64); empty[0, 0] = 49406
        pg, eg = prompt.copy(), empty.copy()
        pg[0, 11:] = 0; eg[0, 2:] = 0
        ids = [prompt, pg, empty, eg]
    model.encode_prompt(ids[0], ids[1])                          # first call folds the LayerNorms / fuses q|k|v once
    T.hip.tf_stream_sync(None)
    t0 = time.perf_counter()
    context, pooled = model.encode_prompt(ids[0], ids[1])
    unc, unc_pooled = (None, None) if args.no_cfg else model.encode_prompt(ids[2], ids[3])
    T.hip.tf_stream_sync(None)
    print(f"context {context.shape}, pooled {pooled.shape}  ({1e3 * (time.perf_counter() - t0):.2f} ms for both towers" + ("" if args.no_cfg else ", two prompts") + ")")
    side = args.size // 8
    latent = model.latent_from_numpy(np.zeros((1, 4, side, side), np.float32))
    schedule = make(args.sampler, args.eta).schedule(args.steps)
    model.compile(unc, context, latent, sampler=schedule, cfg=not args.no_cfg, prediction=args.prediction, cfg_rescale=args.cfg_rescale is not None)
    if args.cfg_rescale is not None:
        model.set_cfg_rescale(args.cfg_rescale)
    times = []
    for n in range(args.images + 1):
        t0 = time.perf_counter()
        model.start(seed=args.seed, image_offset=n, pooled=pooled.numpy(), uncond_pooled=None if unc_pooled is None else unc_pooled.numpy(),
                    original_size=(args.size, args.size), crop_top_left=(0, 0), target_size=(args.size, args.size))
        model.synchronize()
        t1 = time.perf_counter()
        model.run(None if args.no_cfg else args.guidance)
        model.synchronize()
        t2 = time.perf_counter()
        assert np.isfinite(latent.numpy()).all(), f"image {n}: the sampler produced a non-finite latent"
        with T.use_stream(model._stream):
            x = model.decode(latent)
        t3 = time.perf_counter()
        times.append((t1 - t0, t2 - t1, t3 - t2))
        print(f"image {n}: start {1e3 * (t1 - t0):.1f} ms, {args.steps} steps {1e3 * (t2 - t1):.1f} ms, decode {1e3 * (t3 - t2):.1f} ms, image {x.shape} mean {x.mean():.1f}")
    st, s, d = (np.median([t[i] for t in times[1:]]) for i in range(3))
    print(f"end-to-end (start + sampler + VAE decode, batch 1): {1.0 / (st + s + d):.3f} img/s")
    if args.out:
        np.save(args.out, x)


def run_motion(ap, args):
    """--motion [FILE]: text to video with AnimateDiff motion modules on SD-1.5 -- one video of --frames frames under one prompt, the linear-beta
    schedule the motion modules were trained with, every frame decoded by the VAE; --out gets the (F, H, W, 3) uint8 frames."""
    import contextlib
    import io
    if not args.sampler:
        ap.error("--motion needs --sampler")
    for flag, name in ((args.concat, "--concat"), (args.control_image, "--control-image"), (args.ip_adapter is not None, "--ip-adapter"), (args.freeu is not None, "--freeu"),
                       (args.pag is not None, "--pag"), (args.init_image, "--init-image"), (args.sd2, "--sd2")):
        if flag:
            ap.error(f"{name} with --motion is not supported")
    if args.size < 64 or args.size % 64 or args.size > 1024:
        ap.error(f"--size {args.size}: expected a multiple of 64 up to 1024")
    import tinyfusers_amd.storage.tensor as T
    from tinyfusers_amd.storage.state import param_shapes, update_state
    from tinyfusers_amd.storage.synth import synth_motion_state_dict, synth_state_dict
    from tinyfusers_amd.variants.samplers import linear_alphas_cumprod, make
    from tinyfusers_amd.variants.sd import StableDiffusion
    from tinyfusers_amd.vision.motion import MotionAdapter
    from tinyfusers_amd.vision.unet import SD15
    t0 = time.time()
    T.ensure_init(0)
    model = StableDiffusion(SD15)
    if args.ckpt:
        from tinyfusers_amd.storage.unpicker import load_checkpoint
        state = load_checkpoint(args.ckpt)
    else:
        state = synth_state_dict(param_shapes(model), 0)
    with contextlib.redirect_stdout(io.StringIO()):
        update_state(model, state, "")
    del state
    adapter = MotionAdapter.load(SD15, args.motion or synth_motion_state_dict(SD15, 1, max_len=24))
    if not 1 <= args.frames <= min(32, adapter.max_len):
        ap.error(f"--frames {args.frames}: this motion module takes 1 .. {min(32, adapter.max_len)} frames")
    model.attach_motion(adapter)
    print(f"weights installed in {time.time() - t0:.1f}s: {len(adapter.modules)} motion modules, max_len {adapter.max_len}" + (", mid_block" if adapter.mid else ""))
    if args.lora:
        names = [model.load_lora(spec.split(":")[0], name=f"{i}") for i, spec in enumerate(args.lora)]
        model.set_adapters(names, [float(spec.split(":")[1]) if ":" in spec else 1.0 for spec in args.lora])
    if args.vocab:
        from tinyfusers_amd.tokenizer.clip import ClipTokenizer
        tok = ClipTokenizer(args.vocab)
        prompt, empty = np.array([tok.encode(args.prompt)]), np.array([tok.encode("")])
    else:
        rng = np.random.default_rng(args.seed)
        prompt = np.full((1, 77), 49407, dtype=np.int64); prompt[0, 0] = 49406; prompt[0, 1:10] = rng.integers(0, 49406, 9)
        empty = np.full((1, 77), 49407, dtype=np.int64); empty[0, 0] = 49406
    text_model = model.cond_stage_model.transformer.text_model
    context = text_model(prompt)                                 # ONE prompt for the video: compile broadcasts it to the frames
    unc = None if args.no_cfg else text_model(empty)
    side, f = args.size // 8, args.frames
    latent = model.latent_from_numpy(np.zeros((f, 4, side, side), np.float32))
    schedule = make(args.sampler, args.eta).schedule(args.steps, alphas_cumprod=linear_alphas_cumprod())
    model.compile(unc, context, latent, sampler=schedule, cfg=not args.no_cfg, prediction=args.prediction, cfg_rescale=args.cfg_rescale is not None,
                  motion=True, frames=f)
    if args.cfg_rescale is not None:
        model.set_cfg_rescale(args.cfg_rescale)
    if args.motion_scale is not None:
        model.set_motion_scale(args.motion_scale)
    times = []
    for n in range(args.images + 1):
        model.start(seed=args.seed, image_offset=n * f)
        model.synchronize()
        t0 = time.perf_counter()
        model.run(None if args.no_cfg else args.guidance)
        model.synchronize()
        t1 = time.perf_counter()
        assert np.isfinite(latent.numpy()).all(), f"video {n}: the sampler produced a non-finite latent"
        per = latent.size // f
        with T.use_stream(model._stream):
            frames = np.stack([model.decode(latent.view((1, 4, side, side), "row", k * per)) for k in range(f)])
        t2 = time.perf_counter()
        times.append((t1 - t0, t2 - t1))
        print(f"video {n}: {args.steps} steps {1e3 * (t1 - t0):.1f} ms ({args.steps / (t1 - t0):.1f} steps/s), decode of {f} frames {1e3 * (t2 - t1):.1f} ms, "
              f"frames {frames.shape} {frames.dtype} mean {frames.mean():.1f}")
    s, d = (np.median([t[i] for t in times[1:]]) for i in range(2)) if len(times) > 1 else times[0]
    print(f"end-to-end (sampler + VAE decode, one video of {f} frames): {f / (s + d):.3f} frames/s")
    if args.out:
        np.save(args.out, frames)
        print(f"wrote {frames.shape} {frames.dtype} to {args.out}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="Run the SD-1.x sampler on MI355X (synthetic weights)")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--guidance", type=float, default=7.5)
    ap.add_argument("--images", type=int, default=3, help="images to time after the first (compile + warm-up) one")
    ap.add_argument("--out", default="")
    ap.add_argument("--ckpt", default="", help="LDM checkpoint (.ckpt torch zip or .safetensors); default: synthetic weights")
    ap.add_argument("--vocab", default="", help="local bpe_simple_vocab_16e6.txt.gz for the prompt; default: seeded token ids")
    ap.add_argument("--prompt", default="a horse sized cat eating a bagel")
    ap.add_argument("--sampler", choices=["ddim", "ddim-eta", "dpmpp2m", "euler-a", "lcm"], default=None,
                    help="run a sampler schedule (variants/samplers.py) with device-side noise from --seed; default: the reference's DDIM loop")
    ap.add_argument("--no-cfg", action="store_true",
                    help="with --sampler: the guidance-free step (compile(..., cfg=False)): one guidance branch, --guidance is not used and the unconditional "
                         "prompt is not encoded -- how an LCM / LCM-LoRA samples (guidance 1)")
    ap.add_argument("--eta", type=float, default=None, help="noise scale of ddim-eta (default 1) and euler-a (default 1)")
    ap.add_argument("--init-image", default="", help="image-to-image from this (H,W,3) uint8 image: .npy, or .png / .jpg through PIL")
    ap.add_argument("--strength", type=float, default=None, help="with --init-image: the part of the schedule that runs, in (0, 1] (default 0.6)")
    ap.add_argument("--mask", default="", help="with --init-image: inpaint where this (H,W) mask is >= 0.5 (uint8: nonzero); .npy, .png or .jpg")
    ap.add_argument("--concat", choices=["inpaint", "edit"], default=None,
                    help="a concat-conditioned UNet on synthetic weights: the SD-1.5 inpainting checkpoint (9 input channels) or InstructPix2Pix (8); "
                         "with --ckpt the checkpoint decides")
    ap.add_argument("--cond-image", default="", help="the image a concat-conditioned UNet reads: the image to inpaint / to edit, (H,W,3) uint8; .npy, .png or .jpg")
    ap.add_argument("--cond-mask", default="", help="with an inpainting checkpoint: repaint where this (H,W) mask is >= 0.5 (uint8: nonzero)")
    ap.add_argument("--image-guidance", type=float, default=None, help="with an InstructPix2Pix checkpoint: the image guidance scale (default 1.5)")
    ap.add_argument("--control-image", default="", help="condition on this ControlNet hint (edges, depth, pose ...), one (H,W,3) uint8 image; .npy, .png or .jpg")
    ap.add_argument("--control-ckpt", default="", help="with --control-image: the ControlNet checkpoint (its control_model.* tensors); default: synthetic weights")
    ap.add_argument("--control-scale", type=float, default=None, help="with --control-image: the strength of the control residuals (default 1.0)")
    ap.add_argument("--lora", action="append", default=[], metavar="FILE[:w[:w_te]]",
                    help="merge this LoRA adapter (.safetensors / .ckpt / .pt; kohya or PEFT keys) at UNet weight w (default 1) and text-encoder weight w_te "
                         "(default w); repeatable")
    ap.add_argument("--ip-adapter", nargs="?", const="", default=None, metavar="FILE",
                    help="condition on an image prompt through an IP-Adapter (ip-adapter_sd15 .safetensors / .bin); without FILE: synthetic adapter weights")
    ap.add_argument("--ip-embeds", default="", help="with --ip-adapter: the CLIP image embeddings of the prompt image, a float (1, E) .npy (E = 1024 for ViT-H); "
                                                    "with synthetic adapter weights a seeded vector stands in when not given")
    ap.add_argument("--ip-image", default="", help="with --ip-adapter: the prompt image itself (.npy or an image file), uint8 (S, S, 3) ALREADY resized and centre-cropped to the "
                                                   "image tower's size (224 for ViT-H); the CLIP vision tower turns it into the embeddings on the device")
    ap.add_argument("--clip-vision", default="", help="with --ip-image: the CLIP image encoder's checkpoint (CLIPVisionModelWithProjection .safetensors / .bin); "
                                                      "default: synthetic ViT-H weights")
    ap.add_argument("--ip-scale", type=float, default=None, help="with --ip-adapter: the adapter's strength (default 1.0)")
    ap.add_argument("--freeu", default=None, metavar="S1,S2,B1,B2",
                    help="FreeU inside the captured step (needs --sampler): the Fourier filter's scale on the skips and the backbone factor of decoder stages 1 and 2; "
                         "0.9,0.2,1.5,1.6 are the values usually quoted for SD-1.5")
    ap.add_argument("--pag", type=float, default=None, metavar="SCALE",
                    help="perturbed-attention guidance inside the captured step (needs --sampler): one more guidance group whose self-attention is the identity "
                         "in the selected transformers; 3.0 is the scale usually quoted")
    ap.add_argument("--pag-layers", default="mid", help="with --pag: the transformers to perturb, comma-separated: down, mid, up, all, LDM paths (input_blocks.4, "
                                                        "middle_block, output_blocks.7) or indices in execution order (default: mid)")
    ap.add_argument("--pag-adaptive", type=float, default=0.0, metavar="A", help="with --pag: the adaptive scale a of s_t = max(0, s - a (1000 - t)) (default 0)")
    ap.add_argument("--sd2", action="store_true", help="the Stable Diffusion 2.x configuration on synthetic weights (heads of 64, 1024-wide OpenCLIP context); with --ckpt the checkpoint decides")
    ap.add_argument("--prediction", choices=["eps", "v"], default="eps",
                    help="what the UNet predicts (needs --sampler for v): the SD-2.x 768-v checkpoints predict v; a checkpoint file does not say, so the default is eps")
    ap.add_argument("--cfg-rescale", type=float, default=None, metavar="PHI",
                    help="CFG rescale inside the captured step (needs --sampler and a guidance pair): the factor phi in [0, 1]; 0.7 is the value usually quoted with v-prediction")
    ap.add_argument("--sdxl", action="store_true", help="the SDXL base configuration (needs --sampler): two text towers, pooled / size conditioning through start(); "
                                                         "--ckpt FILE: an SGM checkpoint (sd_xl_base_1.0), synthetic weights without one")
    ap.add_argument("--size", type=int, default=None, help="with --sdxl or --motion: the image's side in pixels, a multiple of 64 (default 1024 / 512)")
    ap.add_argument("--motion", nargs="?", const="", default=None, metavar="FILE",
                    help="text to video with AnimateDiff motion modules (needs --sampler): a motion-module file (mm_sd_v15*.ckpt / .safetensors, AnimateDiff or "
                         "diffusers names); without FILE: synthetic module weights.  --out then holds the (F, H, W, 3) uint8 frames")
    ap.add_argument("--frames", type=int, default=16, help="with --motion: the frames of the video, 1 .. min(32, the file's max_len) (default 16)")
    ap.add_argument("--motion-scale", type=float, default=None, help="with --motion: the strength of the modules' residual branch (default 1.0)")
    args = ap.parse_args()
    if args.size is None:
        args.size = 512 if args.motion is not None else 1024
    if args.sdxl:
        if args.motion is not None:
            ap.error("--motion with --sdxl is not supported")
        run_sdxl(ap, args)
        sys.exit(0)
    if args.motion is not None:
        run_motion(ap, args)
        sys.exit(0)
    if args.motion_scale is not None:
        ap.error("--motion-scale needs --motion")
    if (args.prediction == "v" or args.cfg_rescale is not None) and not args.sampler:
        ap.error("--prediction v and --cfg-rescale need --sampler")
    if args.cfg_rescale is not None and not 0.0 <= args.cfg_rescale <= 1.0:
        ap.error(f"--cfg-rescale {args.cfg_rescale}: expected a factor in [0, 1]")
    if args.cfg_rescale is not None and ((args.no_cfg and args.pag is None) or args.concat == "edit"):
        ap.error("--cfg-rescale needs a guidance pair or triple (not --no-cfg without --pag, not an InstructPix2Pix checkpoint)")
    if args.sd2 and (args.concat == "edit" or args.ip_adapter is not None):
        ap.error("--sd2 has no InstructPix2Pix configuration and no IP-Adapter")
    if args.pag is not None and not args.sampler:
        ap.error("--pag needs --sampler")
    pag_layers = [int(v) if v.lstrip("-").isdigit() else v for v in args.pag_layers.split(",") if v]
    freeu = None
    if args.freeu is not None:
        if not args.sampler:
            ap.error("--freeu needs --sampler")
        try:
            freeu = tuple(float(v) for v in args.freeu.split(","))
        except ValueError:
            freeu = ()
        if len(freeu) != 4 or not all(np.isfinite(freeu)):
            ap.error(f"--freeu {args.freeu}: expected four finite floats S1,S2,B1,B2")
    if (args.ip_embeds or args.ip_image or args.clip_vision or args.ip_scale is not None) and args.ip_adapter is None:
        ap.error("--ip-embeds, --ip-image, --clip-vision and --ip-scale need --ip-adapter")
    if args.ip_adapter is not None:
        if not args.sampler:
            ap.error("--ip-adapter needs --sampler")
        if args.ip_image and args.ip_embeds:
            ap.error("--ip-image and --ip-embeds: pass one of them")
        if args.clip_vision and not args.ip_image:
            ap.error("--clip-vision needs --ip-image")
        if args.ip_adapter and not (args.ip_embeds or args.ip_image):
            ap.error("--ip-adapter FILE needs --ip-embeds (the CLIP image embeddings of the prompt image) or --ip-image")
        if args.concat == "edit":
            ap.error("--ip-adapter on an InstructPix2Pix checkpoint is not supported")
    loras = []
    for spec in args.lora:
        parts = spec.split(":")
        cut = len(parts)
        while cut > 1 and len(parts) - cut < 2:
            try:
                float(parts[cut - 1])
            except ValueError:
                break
            cut -= 1
        try:
            ws = [float(v) for v in parts[cut:]]
        except ValueError:
            ws = None
        if ws is None or not parts[0]:
            ap.error(f"--lora {spec}: expected FILE[:w[:w_te]]")
        loras.append((":".join(parts[:cut]), ws[0] if ws else 1.0, ws[1] if len(ws) > 1 else (ws[0] if ws else 1.0)))
    if args.no_cfg and not args.sampler:
        ap.error("--no-cfg needs --sampler")
    if args.no_cfg and args.concat == "edit":
        ap.error("--no-cfg on an InstructPix2Pix checkpoint is not supported (its update is defined by three guidance branches)")
    if (args.control_ckpt or args.control_scale is not None) and not args.control_image:
        ap.error("--control-ckpt and --control-scale need --control-image")
    if args.control_image and not args.sampler:
        ap.error("--control-image needs --sampler")
    if (args.init_image or args.mask or args.strength is not None) and not args.sampler:
        ap.error("--init-image, --strength and --mask need --sampler")
    if (args.mask or args.strength is not None) and not args.init_image:
        ap.error("--strength and --mask need --init-image")

    def load_array(path, mode):
        """.npy as stored; .png / .jpg through PIL (imported only here), mode "RGB" or "L"."""
        if path.lower().endswith(".npy"):
            return np.load(path)
        from PIL import Image
        return np.asarray(Image.open(path).convert(mode))

    import tinyfusers_amd.storage.tensor as T
    from tinyfusers_amd.storage.state import param_shapes, update_state
    from tinyfusers_amd.storage.synth import synth_normal, synth_state_dict
    from tinyfusers_amd.variants.sd import StableDiffusion

    from tinyfusers_amd.vision.unet import SD15, SD15_EDIT, SD15_INPAINT, SD21, SD21_INPAINT

    t0 = time.time()
    import io, contextlib
    concat, sd2 = args.concat, args.sd2
    if args.ckpt:
        from tinyfusers_amd.storage.unpicker import load_checkpoint
        state = load_checkpoint(args.ckpt)                       # memory-mapped; update_state streams tensor by tensor
        cin = int(state["model.diffusion_model.input_blocks.0.0.weight"].shape[1])
        if cin not in (4, 9, 8):
            sys.exit(f"--ckpt: the UNet's conv_in reads {cin} channels; 4 (text-to-image), 9 (inpainting) and 8 (InstructPix2Pix) are supported")
        if concat and cin != {"inpaint": 9, "edit": 8}[concat]:
            sys.exit(f"--concat {concat} does not fit this checkpoint, whose conv_in reads {cin} channels")
        concat = {4: None, 9: "inpaint", 8: "edit"}[cin]
        to_k = state.get("model.diffusion_model.input_blocks.1.1.transformer_blocks.0.attn2.to_k.weight")
        sd2 = to_k is not None and int(to_k.shape[1]) == 1024      # the cross-attention reads the OpenCLIP ViT-H context: SD-2.x
        if sd2 and concat == "edit":
            sys.exit("--ckpt: an 8-channel UNet with a 1024-wide context is not a supported configuration")
        if sd2 and args.ip_adapter is not None:
            sys.exit("--ip-adapter on an SD-2.x checkpoint is not supported")
    if concat:
        what = "an inpainting checkpoint (9 input channels)" if concat == "inpaint" else "an InstructPix2Pix checkpoint (8 input channels)"
        if not args.sampler:
            ap.error(f"{what} runs with --sampler")
        if not args.cond_image or (concat == "inpaint" and not args.cond_mask):
            ap.error(f"{what} needs --cond-image" + (" and --cond-mask" if concat == "inpaint" else "") + ": its UNet reads them at every step")
        if args.no_cfg and concat == "edit":
            ap.error("--no-cfg on an InstructPix2Pix checkpoint is not supported (its update is defined by three guidance branches)")
        if args.mask:
            ap.error("--mask (the latent blend) on top of a concat-conditioned checkpoint is not supported; use --cond-mask")
    if concat and args.control_image:
        ap.error("--control-image on a concat-conditioned checkpoint is not supported")
    if (args.cond_image or args.cond_mask or args.image_guidance is not None) and not concat:
        ap.error("--cond-image, --cond-mask and --image-guidance need an inpainting or InstructPix2Pix checkpoint (--ckpt, or --concat on synthetic weights)")
    if (args.cond_mask and concat != "inpaint") or (args.image_guidance is not None and concat != "edit"):
        ap.error("--cond-mask goes with an inpainting checkpoint, --image-guidance with an InstructPix2Pix one")
    T.ensure_init(0)
    model = StableDiffusion({None: SD21, "inpaint": SD21_INPAINT}[concat] if sd2 else {None: SD15, "inpaint": SD15_INPAINT, "edit": SD15_EDIT}[concat])
    if not args.ckpt:
        state = synth_state_dict({k: v for k, v in param_shapes(model).items() if not k.startswith("cond_stage_model.model.")}, 0)   # UNet + VAE decoder + CLIP text encoder, by LDM name
        if sd2:                                                # the OpenCLIP tower's names are not synth_tensor's: its own seeded weights
            from tinyfusers_amd.vae.open_clip_text import LDM_PREFIX, synthetic_state
            state.update(synthetic_state(model.cond_stage_model.cfg, 0, LDM_PREFIX))
    with contextlib.redirect_stdout(io.StringIO()):
        update_state(model, state, "")
    del state
    if args.control_image:
        from tinyfusers_amd.vision.controlnet import ControlNet
        net = ControlNet(SD21 if sd2 else SD15)
        if args.control_ckpt:
            from tinyfusers_amd.storage.unpicker import load_checkpoint
            cstate = load_checkpoint(args.control_ckpt)
            if not any(k.startswith("control_model.") for k in cstate):
                sys.exit("--control-ckpt: the file holds no control_model.* tensors")
        else:
            cstate = synth_state_dict(param_shapes(net, "control_model"), 1)
        with contextlib.redirect_stdout(io.StringIO()):
            update_state(net, cstate, "control_model.")
        del cstate
        model.attach_control(net)
    if args.ip_adapter is not None:
        from tinyfusers_amd.storage.ip_adapter import IPAdapter
        if concat == "edit":
            sys.exit("--ip-adapter on an InstructPix2Pix checkpoint is not supported")
        unet = model.model.diffusion_model
        if args.ip_adapter:
            adapter = IPAdapter.load(unet, args.ip_adapter)
        else:
            adapter = IPAdapter(unet, 4, 1024)
            astate = {k: (synth_normal(2, k, shp, 0.03) + (1.0 if k == "image_proj.norm.weight" else 0.0)).astype(np.float16) for k, shp in adapter.expected_shapes().items()}
            with contextlib.redirect_stdout(io.StringIO()):
                update_state(adapter, astate, "")
        model.attach_ip_adapter(adapter)
        if args.ip_image:
            from dataclasses import replace
            from tinyfusers_amd.vae.clip_vision import VIT_H, ClipVision, synthetic_state
            with contextlib.redirect_stdout(io.StringIO()):
                tower = ClipVision.load(args.clip_vision or synthetic_state(replace(VIT_H, projection=adapter.embed_dim), 3))
            model.attach_clip_vision(tower)
    print(f"weights installed in {time.time() - t0:.1f}s")
    if loras:                                                    # before the prompts are encoded (text-encoder adapters) and before compile
        t0 = time.perf_counter()
        names = [model.load_lora(path, name=f"{i}:{os.path.basename(path)}") for i, (path, _, _) in enumerate(loras)]
        model.set_adapters(names, [w for _, w, _ in loras], [w for _, _, w in loras])
        T.hip.tf_stream_sync(None)
        print(f"LoRA: {', '.join(f'{n} at {w} / {wt}' for n, (w, wt) in model.adapters().items())} merged in {1e3 * (time.perf_counter() - t0):.1f} ms (load + merge)")
    # run through CLIP to get the contexts (example/sd1.py:44-49); token ids stand in for tokenizer.encode(prompt)
    if args.vocab:
        from tinyfusers_amd.tokenizer.clip import ClipTokenizer
        tokenizer = ClipTokenizer(args.vocab)
        pad = 0 if sd2 else None                               # SD-2.x pads with id 0 behind the end-of-text token
        prompt, empty = np.array([tokenizer.encode(args.prompt, pad_id=pad)]), np.array([tokenizer.encode("", pad_id=pad)])
    else:
        rng = np.random.default_rng(args.seed)
        n_words = 9
        prompt = np.full((1, 77), 49407, dtype=np.int64); prompt[0, 0] = 49406; prompt[0, 1:1 + n_words] = rng.integers(0, 49406, n_words)
        empty = np.full((1, 77), 49407, dtype=np.int64); empty[0, 0] = 49406
        if sd2:
            prompt[0, 2 + n_words:] = 0; empty[0, 2:] = 0
    text_model = model.cond_stage_model if sd2 else model.cond_stage_model.transformer.text_model
    text_model(prompt)                                           # first call folds the LayerNorms / fuses q|k|v once
    T.hip.tf_stream_sync(None)
    t0 = time.perf_counter()
    context = text_model(prompt)
    unconditional_context = None if args.no_cfg else text_model(empty)       # (the guidance-free step reads the prompt alone)
    T.hip.tf_stream_sync(None)
    print(f"CLIP context: {context.shape}, " + ("no unconditional context (--no-cfg)" if args.no_cfg else f"unconditional CLIP context: {unconditional_context.shape}")
          + f"  ({1e3 * (time.perf_counter() - t0):.2f} ms)")
    timesteps = list(range(1, 1000, 1000 // args.steps))
    alphas = model.alphas_cumprod[timesteps]
    alphas_prev = np.concatenate((np.array([1.0]), alphas[:-1])).astype(np.float32)
    init_image = mask = None
    lat_hw = (64, 64)
    if args.init_image:
        init_image = load_array(args.init_image, "RGB")
        if init_image.ndim == 3:
            init_image = init_image[None]
        if init_image.dtype != np.uint8 or init_image.ndim != 4 or init_image.shape[0] != 1 or init_image.shape[3] != 3:
            sys.exit(f"--init-image: expected one uint8 (H,W,3) image, got {init_image.dtype} {init_image.shape}")
        why = StableDiffusion.encoder_size_error(init_image.shape[1], init_image.shape[2])
        if why:
            sys.exit(f"--init-image: {why}")
        lat_hw = (init_image.shape[1] // 8, init_image.shape[2] // 8)
        if args.mask:
            mask = load_array(args.mask, "L")
            mask = StableDiffusion.latent_mask(mask[None] if mask.ndim == 2 else mask)
    cond_kw = {}
    if concat:
        cond_image = load_array(args.cond_image, "RGB")
        cond_image = cond_image[None] if cond_image.ndim == 3 else cond_image
        if cond_image.dtype != np.uint8 or cond_image.ndim != 4 or cond_image.shape[0] != 1 or cond_image.shape[3] != 3:
            sys.exit(f"--cond-image: expected one uint8 (H,W,3) image, got {cond_image.dtype} {cond_image.shape}")
        why = StableDiffusion.encoder_size_error(cond_image.shape[1], cond_image.shape[2])
        if why:
            sys.exit(f"--cond-image: {why}")
        if init_image is not None and init_image.shape != cond_image.shape:
            sys.exit(f"--init-image {init_image.shape} and --cond-image {cond_image.shape} differ in size")
        lat_hw = (cond_image.shape[1] // 8, cond_image.shape[2] // 8)
        cond_kw = {"cond_image": cond_image}
        if concat == "inpaint":
            cond_mask = load_array(args.cond_mask, "L")
            cond_kw["cond_mask"] = cond_mask[None] if cond_mask.ndim == 2 else cond_mask
        if args.image_guidance is not None:
            cond_kw["image_guidance"] = args.image_guidance
    if args.control_image:
        hint = load_array(args.control_image, "RGB")
        hint = hint[None] if hint.ndim == 3 else hint
        if hint.dtype != np.uint8 or hint.ndim != 4 or hint.shape[0] != 1 or hint.shape[3] != 3 or hint.shape[1] % 8 or hint.shape[2] % 8:
            sys.exit(f"--control-image: expected one uint8 (H,W,3) image with H and W multiples of 8, got {hint.dtype} {hint.shape}")
        if init_image is not None and init_image.shape != hint.shape:
            sys.exit(f"--init-image {init_image.shape} and --control-image {hint.shape} differ in size")
        lat_hw = (hint.shape[1] // 8, hint.shape[2] // 8)
        cond_kw = {"control_image": hint}
        if args.control_scale is not None:
            cond_kw["control_scale"] = args.control_scale
    if args.ip_adapter is not None and args.ip_image:
        ip_image = load_array(args.ip_image, "RGB")
        ip_image = ip_image[None] if ip_image.ndim == 3 else ip_image
        size = tower.cfg.image
        if ip_image.dtype != np.uint8 or ip_image.shape != (1, size, size, 3):
            sys.exit(f"--ip-image: expected one uint8 ({size}, {size}, 3) image (resize and centre-crop it first), got {ip_image.dtype} {ip_image.shape}")
        cond_kw = dict(cond_kw, ip_image=ip_image)
        if args.ip_scale is not None:
            cond_kw["ip_scale"] = args.ip_scale
    elif args.ip_adapter is not None:
        embeds = np.load(args.ip_embeds) if args.ip_embeds else synth_normal(args.seed, "sd.ip_embeds", (1, adapter.embed_dim))
        embeds = np.asarray(embeds, np.float32).reshape(1, -1) if np.asarray(embeds).ndim == 1 else np.asarray(embeds, np.float32)
        if embeds.shape != (1, adapter.embed_dim):
            sys.exit(f"--ip-embeds: expected one float (1, {adapter.embed_dim}) embedding for this adapter, got {embeds.shape}")
        cond_kw = dict(cond_kw, ip_image_embeds=embeds)
        if args.ip_scale is not None:
            cond_kw["ip_scale"] = args.ip_scale
    latent = model.latent_from_numpy(synth_normal(args.seed, "sd.latent", (1, 4) + lat_hw))
    if args.sampler:
        from tinyfusers_amd.variants.samplers import make
        strength = 1.0 if init_image is None else (0.6 if args.strength is None else args.strength)
        schedule = make(args.sampler, args.eta).schedule(args.steps, strength=strength)
        print(f"sampler {schedule.sampler}: {len(schedule.timesteps)} steps, timesteps {schedule.timesteps[0]} .. {schedule.timesteps[-1]}"
              + (f" (strength {strength}{', inpainting' if mask is not None else ''})" if init_image is not None else ""))
        model.compile(unconditional_context, context, latent, sampler=schedule, inpaint=mask is not None, concat=concat, control=bool(args.control_image),
                      cfg=not args.no_cfg, ip_adapter=args.ip_adapter is not None, freeu=freeu is not None, pag=args.pag is not None,
                      prediction=args.prediction, cfg_rescale=args.cfg_rescale is not None)
        if args.cfg_rescale is not None:
            model.set_cfg_rescale(args.cfg_rescale)              # one device word: it stays until the next set_cfg_rescale / start(cfg_rescale=)
        if args.pag is not None:
            model.set_pag(args.pag, pag_layers, args.pag_adaptive)   # 16 device words and two host scalars: they stay until the next set_pag / start(pag=)
        if freeu is not None:
            model.set_freeu(*freeu)                              # four device scalars: they stay until the next set_freeu / start(freeu=)
    else:
        model.compile(unconditional_context, context, latent)
    times = []
    for n in range(args.images + 1):
        enc = 0.0
        if init_image is not None:
            t0 = time.perf_counter()
            with T.use_stream(model._stream):
                x0 = model.encode_image(init_image)              # the VAE encoder: x0 = 0.18215 x its means
            model.synchronize()
            enc = time.perf_counter() - t0
            model.start(seed=args.seed, image_offset=n, init_latent=x0, mask=mask, **cond_kw)   # x0 noised to the schedule's start level
        elif args.sampler:
            model.start(seed=args.seed, image_offset=n, **cond_kw)   # image n of the seed: its latent and ancestral noise drawn on the device; a
            #                                                          concat-conditioned UNet's image (and mask) go through the VAE encoder here
        else:
            model.set_latent(synth_normal(args.seed + n, "sd.latent", (1, 4, 64, 64)))
        t0 = time.perf_counter()
        if args.sampler:
            model.run(None if args.no_cfg else args.guidance)
        else:
            for index, timestep in list(enumerate(timesteps))[::-1]:
                model.step(timestep, alphas[index], alphas_prev[index], args.guidance)
        model.synchronize()
        t1 = time.perf_counter()
        assert np.isfinite(latent.numpy()).all(), f"image {n}: the sampler produced a non-finite latent"
        with T.use_stream(model._stream):
            x = model.decode(latent)
        t2 = time.perf_counter()
        times.append((t1 - t0, t2 - t1, enc))
        steps = len(schedule.timesteps) if init_image is not None else args.steps
        print(f"image {n}: " + (f"encode {1e3 * enc:.1f} ms, " if init_image is not None else "")
              + f"{steps} steps {1e3 * (t1 - t0):.1f} ms ({steps / (t1 - t0):.1f} steps/s), decode {1e3 * (t2 - t1):.1f} ms, image {x.shape} mean {x.mean():.1f}")
    s, d, e = (np.median([t[i] for t in times[1:]]) for i in range(3))
    if init_image is not None:
        print(f"end-to-end (VAE encode + sampler + VAE decode, batch 1): {1.0 / (e + s + d):.3f} img/s  [encode {1e3 * e:.1f} ms + {steps} steps "
              f"{1e3 * s:.1f} ms + decode {1e3 * d:.1f} ms]")
    else:
        print(f"end-to-end (sampler + VAE decode, batch 1): {1.0 / (s + d):.3f} img/s  [{steps} steps {1e3 * s:.1f} ms + decode {1e3 * d:.1f} ms]")
    if args.out:
        np.save(args.out, x)
