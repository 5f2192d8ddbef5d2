"""GPU checks of the CLIP vision tower (vae/clip_vision.py) and of ``StableDiffusion.start(ip_image=)`` against the CPU restatement
tests/aux/clip_vision_ref.py.

The tiny tower is image 56 / patch 14 (17 tokens), width 320, 4 heads of 80, 2 layers, mlp 1280, projection 32 -- the E of the tiny adapter of
tests/test_gpu_ip_adapter.py, whose UNet, adapter and sampler helpers the end-to-end test reuses.  (a) - (c) are held to the project's forward gate,
rel-L2 <= 5e-3 and max |d| <= 1e-2 (1 + |ref|); in the bfloat16 step both bounds are 3e-2, the figure the existing bf16 tests use
(tests/test_gpu_samplers.py), against the restatement on bfloat16-rounded weights.  Every case prints its measured errors (pytest -s)."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "aux"))
import clip_vision_ref as R  # noqa: E402
import norm_planted as P  # noqa: E402
import test_gpu_ip_adapter as IP  # noqa: E402

DTYPES = ("fp16", "bf16")


@pytest.fixture(scope="module")
def tf():
    import tinyfusers_amd.storage.tensor as T_
    T_.ensure_init(0)
    return T_


@pytest.fixture
def step_dtype(request):
    """The package's 16-bit type for one test (weights are installed in it), put back afterwards."""
    from tinyfusers_amd import config
    config.set_dtype(request.param)
    try:
        yield request.param
    finally:
        config.set_dtype("fp16")


@functools.lru_cache(maxsize=None)
def _weights(name):
    cfg = dict(tiny=R.TINY, tall=dict(R.TINY, image=224, layers=1), wide=dict(R.VIT_H, layers=1, projection=64))[name]
    return cfg, R.make_weights(cfg, seed=3)


def _images(n, s, seed=7):
    return np.random.default_rng([seed, n, s]).integers(0, 256, (n, s, s, 3), dtype=np.uint8)


def _tower(name, tell_heads=True):
    from tinyfusers_amd.vae.clip_vision import ClipVision
    cfg, W = _weights(name)
    return ClipVision.load(W, heads=cfg["heads"] if tell_heads else None), cfg, W


def _ref_weights(W, dtype):
    return W if dtype == "fp16" else {k: P.round16(v.astype(np.float32), "bf16") for k, v in W.items()}


def _gate(got, ref, dtype, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    rel, mx = (5e-3, 1e-2) if dtype == "fp16" else (3e-2, 3e-2)
    rl2 = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    worst = float((np.abs(got - ref) / (1 + np.abs(ref))).max())
    print(f"\n{what} {dtype}: rel-L2 {rl2:.3e} (gate {rel}), max |d| / (1 + |ref|) {worst:.3e} (gate {mx}), max |ref| {np.abs(ref).max():.2f}")
    assert got.shape == ref.shape and np.isfinite(got).all() and rl2 <= rel and worst <= mx, (what, rl2, worst)


def _dev_u8(tf, img):
    return tf.DeviceArray.from_numpy(img, np.uint8, "row")


@pytest.mark.parametrize("step_dtype", DTYPES, indirect=True)
def test_tiny_tower_embeddings_and_output_match_the_restatement(tf, step_dtype):
    tower, cfg, W = _tower("tiny")
    Wr = _ref_weights(W, step_dtype)
    img = _images(2, 56)
    assert tf.dtag(tower.dtype) == (1 if step_dtype == "bf16" else 0)
    emb = tower.embeddings(_dev_u8(tf, img))
    assert emb.shape == (2, 17, 320)
    _gate(emb.numpy(), R.embeddings(img, Wr, cfg).numpy(), step_dtype, "(a) tiny embeddings (class | patches + positions, pre-LayerNorm)")
    out = tower.eager(img)
    assert out.shape == (2, 32)
    _gate(out.numpy(), R.forward(img, Wr, cfg).numpy(), step_dtype, "(a) tiny tower, projected embeddings")
    np.testing.assert_array_equal(tower.eager(_dev_u8(tf, img)).numpy(), out.numpy())       # a device image batch: the same bits
    one = tower.eager(img[1:])                                               # batch 1 (other GEMM tiles: close, not the same bits)
    _gate(one.numpy(), R.forward(img[1:], Wr, cfg).numpy(), step_dtype, "(a) tiny tower, batch 1")


@pytest.mark.parametrize("step_dtype", DTYPES, indirect=True)
def test_one_layer_at_257_tokens(tf, step_dtype):
    """(b) image 224: 256 patches + the class row -- the attention's last query block holds one row."""
    tower, cfg, W = _tower("tall")
    img = _images(2, 224)
    hid = tower.hidden(_dev_u8(tf, img))
    assert hid.shape == (2, 257, 320)
    _gate(hid.numpy(), R.hidden(img, _ref_weights(W, step_dtype), cfg).numpy(), step_dtype, "(b) one layer, 257 tokens, width 320")


@pytest.mark.parametrize("step_dtype", DTYPES, indirect=True)
def test_one_layer_at_vit_h_widths(tf, step_dtype):
    """(c) 1280 / 16 heads of 80 / 5120, 257 tokens, batch 1: the real GEMM and attention shapes (the split attention form)."""
    from tinyfusers_amd.attention.sdpa import sdpa_instance
    tower, cfg, W = _tower("wide", tell_heads=False)                               # width 1280: 16 heads without being told
    assert tower.cfg.heads == 16 and tower.cfg.tokens == 257 and tower.cfg.mlp == 5120
    assert sdpa_instance(tower.dtype, 1, 16, 257, 257, 80, 3 * 1280, 3 * 1280) == "split"
    img = _images(1, 224)
    hid = tower.hidden(_dev_u8(tf, img))
    Wr = _ref_weights(W, step_dtype)
    _gate(hid.numpy(), R.hidden(img, Wr, cfg).numpy(), step_dtype, "(c) one layer at ViT-H widths")
    _gate(tower.pooled(hid).numpy(), R.pooled(R.hidden(img, Wr, cfg), Wr).numpy(), step_dtype, "(c) pooled head at width 1280")


def test_graph_replay_equals_eager_bit_for_bit(tf):
    tower, cfg, W = _tower("tiny")
    a, b = _images(2, 56, 1), _images(2, 56, 2)
    first = tower(a).numpy()                                                 # eager, then captured
    assert list(tower._graphs) == [2]
    np.testing.assert_array_equal(first, tower.eager(a).numpy())
    np.testing.assert_array_equal(tower(a).numpy(), first)                   # replay
    rb = tower(_dev_u8(tf, b)).numpy()                                       # a second image through the same graph, from the device
    np.testing.assert_array_equal(rb, tower.eager(b).numpy())
    assert not np.array_equal(rb, first)
    np.testing.assert_array_equal(tower(a).numpy(), first)
    one = tower(a[:1]).numpy()                                               # another batch size: its own graph
    assert sorted(tower._graphs) == [1, 2]
    np.testing.assert_array_equal(tower(a[:1]).numpy(), one)
    np.testing.assert_array_equal(tower.eager(a[:1]).numpy(), one)
    for bad in (a.astype(np.float32), a[:, :28], a[..., :2]):
        with pytest.raises(ValueError, match="images must be uint8"):
            tower(bad)
    # release_graphs hands every block back exactly once: a result outlives the next call, and no block is on the free list twice
    tower.release_graphs()
    assert not tower._graphs
    r1 = tower(a)                                                            # eager, then captured again
    r2 = tower(b)                                                            # replay
    r3 = tower(a[:1])
    np.testing.assert_array_equal(r1.numpy(), first)
    np.testing.assert_array_equal(r2.numpy(), rb)
    np.testing.assert_array_equal(r3.numpy(), one)
    assert len({r1.ptr, r2.ptr, r3.ptr} | {g[3].ptr for g in tower._graphs.values()}) == 5
    tower.release_graphs()
    free = [p_ for lst in tf.pool().free_blocks.values() for p_ in lst]
    assert len(free) == len(set(free)), "a block is on the pool's free list twice"
    np.testing.assert_array_equal(r1.numpy(), first)


def test_first_call_captures_on_a_cold_pool(tf):
    """A fresh tower whose first call finds no spare block in the pool: the lazily derived weights (the folded head's is as large as the
    patch-embedding output of the tiny tower) take blocks the first eager pass has freed, and the capture must still find every block it needs."""
    pool = tf.pool()
    stash, pool.free_blocks = pool.free_blocks, {}
    try:
        tower = _tower("tiny")[0]
        a = _images(2, 56, 4)
        got = tower(a).numpy()
        assert list(tower._graphs) == [2]
        np.testing.assert_array_equal(tower(a).numpy(), got)
        np.testing.assert_array_equal(tower.eager(a).numpy(), got)
        tower.release_graphs()
    finally:
        for n, lst in stash.items():
            pool.free_blocks.setdefault(n, []).extend(lst)


def test_a_file_loaded_tower_equals_the_in_memory_one(tf, tmp_path):
    import torch
    from tinyfusers_amd.storage.unpicker import save_safetensors
    from tinyfusers_amd.vae.clip_vision import ClipVision
    cfg, W = _weights("tiny")
    img = _images(2, 56)
    want = _tower("tiny")[0].eager(img).numpy()
    flat, nested = str(tmp_path / "vit.safetensors"), str(tmp_path / "vit.bin")
    save_safetensors(flat, W)
    torch.save({"state_dict": {k: torch.from_numpy(v.copy()) for k, v in W.items()}}, nested)
    for src in (flat, nested):
        tower = ClipVision.load(src, heads=4)
        assert tower.cfg.image == 56 and tower.cfg.layers == 2 and tower.cfg.projection == 32
        np.testing.assert_array_equal(tower.eager(img).numpy(), want)


@pytest.mark.parametrize("name,cfg", (("dpmpp2m", True), ("lcm", False)))
def test_start_ip_image_is_start_ip_image_embeds_of_the_towers_output(tf, name, cfg):
    """(e) the final latent of start(ip_image=) equals, bit for bit, that of start(ip_image_embeds=tower(img)): the 16-bit embedding passes through
    fp32 on the host exactly.  One image for every latent equals B copies.  (g) without attach_clip_vision the old refusal stands."""
    from tinyfusers_amd.variants.samplers import UnsupportedSamplerConfig
    tower = _tower("tiny")[0]
    img = _images(IP.B, 56, 3)
    sch = IP._sched(name)
    sd, lat = IP._model(tf, sch, cfg=cfg)
    guidance = IP.G if cfg else None
    with pytest.raises(UnsupportedSamplerConfig, match="CLIP vision tower"):
        sd.start(seed=IP.SEED, ip_image=img)
    assert sd.attach_clip_vision(tower) is sd
    graph = sd._graph
    emb = tower(img).numpy()
    assert emb.shape == (IP.B, IP.E) and emb.dtype == np.float32
    _, want = IP._final(sd, lat, guidance=guidance, ip_image_embeds=emb)
    _, got = IP._final(sd, lat, guidance=guidance, ip_image=img)
    np.testing.assert_array_equal(got, want)
    _, got_dev = IP._final(sd, lat, guidance=guidance, ip_image=_dev_u8(tf, img))
    np.testing.assert_array_equal(got_dev, want)
    _, eager = IP._final(sd, lat, eager=True, guidance=guidance, ip_image=img)
    np.testing.assert_array_equal(eager, want)
    # one image for all == B copies of it; and it is another trajectory
    _, one = IP._final(sd, lat, guidance=guidance, ip_image=img[:1])
    _, copies = IP._final(sd, lat, guidance=guidance, ip_image=np.repeat(img[:1], IP.B, 0))
    np.testing.assert_array_equal(one, copies)
    _, one_dev = IP._final(sd, lat, guidance=guidance, ip_image=_dev_u8(tf, img[:1]))
    np.testing.assert_array_equal(one_dev, copies)
    assert float(np.abs(one - want).max()) > 1e-3 and sd._graph is graph     # (nothing was captured again)
    before = lat.numpy().copy()
    with pytest.raises(ValueError, match="not both"):
        sd.start(seed=IP.SEED + 1, ip_image=img, ip_image_embeds=emb)
    with pytest.raises(ValueError, match="ip_image must be uint8"):
        sd.start(seed=IP.SEED + 1, ip_image=img[:, :28])
    np.testing.assert_array_equal(lat.numpy(), before)                       # nothing was written


def test_attach_checks_the_widths(tf):
    from tinyfusers_amd.vae.clip_vision import ClipVision
    sd, _ = IP._model(tf, IP._sched())
    cfg, W = _weights("wide")                                                # projects to 64 values, the tiny adapter reads 32
    with pytest.raises(ValueError, match="64 values.*reads 32"):
        sd.attach_clip_vision(ClipVision.load(W))
    with pytest.raises(TypeError, match="ClipVision"):
        sd.attach_clip_vision(object())
