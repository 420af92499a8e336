"""Model configs of the BASELINE.json workloads and deterministic synthetic ("random-init") weights.

There are no checkpoints in this environment, so every BASELINE config runs on random-init weights
(SURVEY.md §8d).  The weights are a pure function of (parameter name, shape, seed) so that the CPU
oracle, the real reference (when present) and the MI355X executor can be handed bit-identical fp32
state dicts anywhere, without relying on module construction order.

Init law (documented gain-scaled variant of torch's default):
  * conv / linear weight  ~ N(0, gain^2 / fan_in),   gain = 1/sqrt(3)  (variance of torch's default
    kaiming_uniform(a=sqrt(5)) = U(-1/sqrt(fan_in), 1/sqrt(fan_in)))
  * conv / linear bias    ~ N(0, gain^2 / fan_in)
  * norm weight = 1 + 0.1*N(0,1), norm bias = 0.1*N(0,1)   (so the affine path is exercised)
numpy's PCG64 + ziggurat stream is platform-independent, unlike vectorised torch CPU randn.
"""
import zlib
from collections import OrderedDict

import numpy as np
import torch

from .backend.nn.layout import clip_param_shapes, flux_param_shapes, unet_param_shapes, vae_decoder_param_shapes, vae_encoder_param_shapes

# LDM-style unet_config dicts (parameter counts 859.52 M / 2567.46 M verified against
# the reference module's own parameter shapes, tests/golden/param_shapes.json, in tests/test_oracle_golden.py).
SD15_UNET_CONFIG = dict(
    in_channels=4, model_channels=320, out_channels=4, num_res_blocks=[2, 2, 2, 2], channel_mult=(1, 2, 4, 4),
    num_heads=8, use_spatial_transformer=True, transformer_depth=[1, 1, 1, 1, 1, 1, 0, 0],
    transformer_depth_middle=1, transformer_depth_output=[1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0],
    context_dim=768, use_linear_in_transformer=False)

SDXL_UNET_CONFIG = dict(
    in_channels=4, model_channels=320, out_channels=4, num_res_blocks=[2, 2, 2], channel_mult=(1, 2, 4),
    num_head_channels=64, use_spatial_transformer=True, transformer_depth=[0, 0, 2, 2, 10, 10],
    transformer_depth_middle=10, transformer_depth_output=[0, 0, 0, 2, 2, 2, 10, 10, 10],
    context_dim=2048, use_linear_in_transformer=True, adm_in_channels=2816, num_classes="sequential")

# Small configs with the same block grammar (used by the parity tests; finish in seconds on CPU).
TINY_SD15_UNET_CONFIG = dict(
    in_channels=4, model_channels=64, out_channels=4, num_res_blocks=[1, 1, 1], channel_mult=(1, 2, 2),
    num_heads=4, use_spatial_transformer=True, transformer_depth=[1, 1, 0],
    transformer_depth_middle=1, transformer_depth_output=[1, 1, 1, 1, 0, 0],
    context_dim=128, use_linear_in_transformer=False)
# transformer_depth_output is consumed with pop() from the END (unet.py:649): listed low-res-last.

# two heads per block at twice the width: heads of 64 and of 128.  Heads up to 64 wide are padded to 64 (backend/nn/unet.py _dpad), so the config
# above never meets the wider kernels SD1.5's 80- and 160-wide heads run on; this one does at its lower level (128 -> 160: native IP-Adapter's
# composite route)
TINY_SD15_WIDE_HEADS_UNET_CONFIG = dict(TINY_SD15_UNET_CONFIG, model_channels=128, num_heads=2)

TINY_SD15_INPAINT_UNET_CONFIG = dict(TINY_SD15_UNET_CONFIG, in_channels=9)  # 4 latent + 1 mask + 4 masked-image latent (sd-v1-5-inpainting)

TINY_SDXL_UNET_CONFIG = dict(
    in_channels=4, model_channels=64, out_channels=4, num_res_blocks=[1, 1], channel_mult=(1, 2),
    num_head_channels=64, use_spatial_transformer=True, transformer_depth=[0, 2],
    transformer_depth_middle=2, transformer_depth_output=[0, 0, 2, 2],
    context_dim=128, use_linear_in_transformer=True, adm_in_channels=192, num_classes="sequential")

SD15_VAE_CONFIG = dict(in_channels=3, out_channels=3, block_out_channels=(128, 256, 512, 512), layers_per_block=2,
                       latent_channels=4, scaling_factor=0.18215, shift_factor=0.0,
                       use_quant_conv=True, use_post_quant_conv=True)
SDXL_VAE_CONFIG = dict(SD15_VAE_CONFIG, scaling_factor=0.13025)
TINY_VAE_CONFIG = dict(in_channels=3, out_channels=3, block_out_channels=(64, 128), layers_per_block=1,
                       latent_channels=4, scaling_factor=0.18215, shift_factor=0.0,
                       use_quant_conv=True, use_post_quant_conv=True)

# Flux.1-dev VAE (backend/huggingface/black-forest-labs/FLUX.1-dev/vae/config.json): 16 latent channels, no quant convs, shift factor
FLUX_VAE_CONFIG = dict(in_channels=3, out_channels=3, block_out_channels=(128, 256, 512, 512), layers_per_block=2, latent_channels=16,
                       scaling_factor=0.3611, shift_factor=0.1159, use_quant_conv=False, use_post_quant_conv=False)
TINY_FLUX_VAE_CONFIG = dict(TINY_VAE_CONFIG, latent_channels=16, scaling_factor=0.3611, shift_factor=0.1159, use_quant_conv=False,
                            use_post_quant_conv=False)

# Flux.1-dev (backend/huggingface/black-forest-labs/FLUX.1-dev/transformer/config.json) and a tiny twin with the
# same head_dim 128 / axes_dim split (the RoPE table and attention tile shapes are the real ones)
FLUX_DEV_CONFIG = dict(in_channels=16, vec_in_dim=768, context_in_dim=4096, hidden_size=3072, mlp_ratio=4.0, num_heads=24, depth=19,
                       depth_single_blocks=38, axes_dim=[16, 56, 56], theta=10000, qkv_bias=True, guidance_embed=True)
TINY_FLUX_CONFIG = dict(in_channels=16, vec_in_dim=64, context_in_dim=128, hidden_size=256, mlp_ratio=4.0, num_heads=2, depth=2,
                        depth_single_blocks=2, axes_dim=[16, 56, 56], theta=10000, qkv_bias=True, guidance_embed=True)

SCHEDULE = dict(beta_schedule="linear", linear_start=0.00085, linear_end=0.012, timesteps=1000,
                prediction_type="epsilon")

DEFAULT_GAIN = 1.0 / np.sqrt(3.0)


def _is_norm(name, shape):
    if len(shape) != 1:
        return False
    parts = name.split(".")
    return any(p.startswith("norm") for p in parts) or parts[-2] == "0" and (
        "in_layers" in parts or "out_layers" in parts or parts[0] == "out")


def synth_tensor(name, shape, seed=0, gain=DEFAULT_GAIN):
    rng = np.random.Generator(np.random.PCG64([seed, zlib.crc32(name.encode())]))
    z = rng.standard_normal(shape, dtype=np.float32)
    if _is_norm(name, shape):
        if name.endswith((".weight", ".scale")):
            z = 1.0 + 0.1 * z
        else:
            z = 0.1 * z
    else:
        if name.endswith(".bias"):
            # the sibling weight's fan_in is not known from the bias alone; callers pass it via shape hints
            raise ValueError("bias needs fan_in; use synth_state_dict")
        fan_in = int(np.prod(shape[1:]))
        z *= gain / np.sqrt(fan_in)
    return torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32))


_BRANCH_OUT = (".out_layers.3.", ".to_out.0.", ".ff.net.2.", ".proj_out.", ".conv2.")


def synth_entry(shapes, name, seed=0, gain=DEFAULT_GAIN, residual_gain=1.0):
    """one tensor of `synth_state_dict(shapes, ...)`: a pure function of (name, shape, seed) -- and of the sibling weight's shape for a bias"""
    shape = shapes[name]
    if _is_norm(name, shape):
        return synth_tensor(name, shape, seed)
    if name.endswith(".bias"):
        wshape = shapes[name[:-5] + ".weight"]
        fan_in = int(np.prod(wshape[1:]))
        rng = np.random.Generator(np.random.PCG64([seed, zlib.crc32(name.encode())]))
        z = rng.standard_normal(shape, dtype=np.float32) * (gain / np.sqrt(fan_in))
        t = torch.from_numpy(z.astype(np.float32))
    else:
        t = synth_tensor(name, shape, seed, gain)
    if residual_gain != 1.0 and any(b in name for b in _BRANCH_OUT):
        t = t * residual_gain
    return t


def synth_state_dict(shapes, seed=0, gain=DEFAULT_GAIN, residual_gain=1.0):
    """fp32 CPU state dict for `shapes` (name -> shape).  `residual_gain` scales the last projection of
    every residual branch (documented knob to keep random-init nets well conditioned; 1.0 = off)."""
    return OrderedDict((name, synth_entry(shapes, name, seed, gain, residual_gain)) for name in shapes)


class LazySynthStateDict:
    """`synth_state_dict(shapes, seed)` as a read-only mapping that draws a tensor when it is asked for and keeps nothing: a 12 G-parameter
    network (Flux.1 at full depth: 48 GB as fp32) is loaded tensor by tensor without the state dict ever existing in host memory.  `dtype`:
    cast on the way out (round to nearest, what `module.to(dtype)` does to the fp32 tensor)."""

    def __init__(self, shapes, seed=0, dtype=None, **kw):
        self.shapes, self.seed, self.dtype, self.kw = shapes, seed, dtype, kw

    def __getitem__(self, name):
        t = synth_entry(self.shapes, name, self.seed, **self.kw)
        return t if self.dtype is None else t.to(self.dtype)

    def __contains__(self, name):
        return name in self.shapes

    def __iter__(self):
        return iter(self.shapes)

    def __len__(self):
        return len(self.shapes)

    def keys(self):
        return self.shapes.keys()

    def items(self):
        return ((k, self[k]) for k in self.shapes)


def synth_state_dict_threaded(shapes, seed=0, dtype=None, workers=None, **kw):
    """`synth_state_dict` drawn by a thread pool (numpy's generators release the GIL; every tensor is a pure function of its name, so the result does
    not depend on the schedule), each tensor cast to `dtype` as soon as it exists: Flux.1 at full depth is 24 GB of fp16 / bf16 in well under a minute
    on a many-core host instead of five minutes on one core, and the fp32 form never exists as a whole."""
    import os
    from concurrent.futures import ThreadPoolExecutor
    workers = workers or max(1, min(32, (os.cpu_count() or 2) - 1))

    def draw(name):
        t = synth_entry(shapes, name, seed, **kw)
        return t if dtype is None else t.to(dtype)

    names = list(shapes)
    with ThreadPoolExecutor(workers) as pool:
        return OrderedDict(zip(names, pool.map(draw, names)))


def synth_unet_state_dict(cfg, seed=0, **kw):
    return synth_state_dict(unet_param_shapes(cfg), seed=seed, **kw)


# the tiny SDXL-shaped UNet with transformers on TWO levels (SDXL has them at 1/2 and 1/4 of the latent): what ControlNet-LLLite needs to meet both
# of its conditioning depths (2 and 3).  The context is wider than the blocks' 128 channels: the reference's LLLite patch tells a self-attention
# from a cross-attention by comparing the widths of q's and k's inputs
TINY_SDXL_2LEVEL_UNET_CONFIG = dict(TINY_SDXL_UNET_CONFIG, num_res_blocks=[1, 1, 1], channel_mult=(1, 2, 2), transformer_depth=[0, 1, 1],
                                    transformer_depth_middle=1, transformer_depth_output=[0, 0, 1, 1, 1, 1], context_dim=192)

LLLITE_PROJECTIONS = ("attn1_to_q", "attn1_to_k", "attn1_to_v", "attn2_to_q")     # what the published SDXL files adapt


def lllite_param_shapes(cfg, projections=LLLITE_PROJECTIONS, hidden=64, embed=32):
    """name -> shape of a ControlNet-LLLite file (Linear modules) for every transformer block of the UNet `cfg`: a module per block and projection,
    its conditioning chain as deep as the block's level asks (a level at 1 / 2^i of the latent is 1 / 2^(i+3) of the control image: depth i + 1)"""
    from .backend.nn.layout import Down, SpatialT, unet_layout
    lay = unet_layout(cfg)
    levels, level, stack = {}, 0, []
    for blk in lay.input_blocks:
        for L in blk:
            if isinstance(L, Down):
                level += 1
            elif isinstance(L, SpatialT):
                levels[L.key] = (level, L)
        stack.append(level)
    for L in lay.middle:
        if isinstance(L, SpatialT):
            levels[L.key] = (level, L)
    for blk in lay.output_blocks:
        level = stack.pop()
        for L in blk:
            if isinstance(L, SpatialT):
                levels[L.key] = (level, L)
    shapes = OrderedDict()
    for key, (level, L) in levels.items():
        depth = level + 1
        if not 1 <= depth <= 3:
            raise ValueError(f"no LLLite conditioning depth for a transformer at level {level}")
        c = L.heads * L.dim_head
        half = embed // 2
        convs = {1: [(half, 3, 4), (embed, half, 2)], 2: [(half, 3, 4), (embed, half, 4)], 3: [(half, 3, 4), (half, half, 4), (embed, half, 2)]}[depth]
        for di in range(L.depth):
            for proj in projections:
                m = f"lllite_unet_{key.replace('.', '_')}_transformer_blocks_{di}_{proj}"
                for i, (co, ci, k) in enumerate(convs):
                    shapes[f"{m}.conditioning1.{2 * i}.weight"] = (co, ci, k, k)
                    shapes[f"{m}.conditioning1.{2 * i}.bias"] = (co,)
                for name, (o, i_) in (("down", (hidden, c)), ("mid", (hidden, embed + hidden)), ("up", (c, hidden))):
                    shapes[f"{m}.{name}.0.weight"] = (o, i_)
                    shapes[f"{m}.{name}.0.bias"] = (o,)
    return shapes


def synth_lllite_state_dict(cfg, seed=21, gain=1.0, up_gain=1.0, **kw):
    """seeded ControlNet-LLLite weights for the UNet `cfg`.  Training starts `up` at zero; here it is drawn like every other layer, times `up_gain`,
    so that a route that drops the adapters computes something else"""
    sd = synth_state_dict(lllite_param_shapes(cfg, **kw), seed=seed, gain=gain)
    if up_gain != 1.0:
        for k in sd:
            if ".up.0." in k:
                sd[k] = sd[k] * up_gain
    return sd


IPADAPTER_CLIP_DIM = 64      # width of the synthetic CLIP-vision embeddings the tiny IP-Adapter files take


def ipadapter_param_shapes(cfg, plus=False, clip_dim=IPADAPTER_CLIP_DIM, resampler_dim=128, depth=4):
    """-> {"image_proj": name -> shape, "ip_adapter": name -> shape} of an IP-Adapter file for the UNet `cfg`: the base image projection (4
    tokens) or, plus=True, the perceiver resampler (16 tokens, heads of 64), and a to_k_ip / to_v_ip pair per cross-attention, numbered 2n + 1 in
    the reference's order (backend/nn/ipadapter.attn2_order)"""
    from .backend.nn.ipadapter import attn2_order
    from .backend.nn.layout import SpatialT, unet_layout
    lay = unet_layout(cfg)
    ctx = cfg["context_dim"]
    proj = OrderedDict()
    if plus:
        proj["latents"] = (1, 16, resampler_dim)
        proj["proj_in.weight"], proj["proj_in.bias"] = (resampler_dim, clip_dim), (resampler_dim,)
        proj["proj_out.weight"], proj["proj_out.bias"] = (ctx, resampler_dim), (ctx,)
        proj["norm_out.weight"], proj["norm_out.bias"] = (ctx,), (ctx,)
        for i in range(depth):
            p = f"layers.{i}."
            for n in ("norm1", "norm2"):
                proj[p + f"0.{n}.weight"], proj[p + f"0.{n}.bias"] = (resampler_dim,), (resampler_dim,)
            proj[p + "0.to_q.weight"], proj[p + "0.to_kv.weight"] = (resampler_dim, resampler_dim), (2 * resampler_dim, resampler_dim)
            proj[p + "0.to_out.weight"] = (resampler_dim, resampler_dim)
            proj[p + "1.0.weight"], proj[p + "1.0.bias"] = (resampler_dim,), (resampler_dim,)
            proj[p + "1.1.weight"], proj[p + "1.3.weight"] = (4 * resampler_dim, resampler_dim), (resampler_dim, 4 * resampler_dim)
    else:
        proj["proj.weight"], proj["proj.bias"] = (4 * ctx, clip_dim), (4 * ctx,)
        proj["norm.weight"], proj["norm.bias"] = (ctx,), (ctx,)
    width = {f"{L.key}.transformer_blocks.{di}": L.heads * L.dim_head for L in lay.all_layers() if isinstance(L, SpatialT) for di in range(L.depth)}
    ip = OrderedDict()
    for n, (_, _, _, name) in enumerate(attn2_order(lay)):
        ip[f"{2 * n + 1}.to_k_ip.weight"] = ip[f"{2 * n + 1}.to_v_ip.weight"] = (width[name], ctx)
    return {"image_proj": proj, "ip_adapter": ip}


def synth_ipadapter_state_dict(cfg, plus=False, seed=31, gain=1.0, kv_gain=1.0, **kw):
    """seeded IP-Adapter weights for the UNet `cfg`, in the layout of a .bin file: {"image_proj": {...}, "ip_adapter": {...}}.  The resampler's
    LayerNorm in front of its feed-forward (`layers.N.1.0`) is drawn around 1 / 0 like every other norm; kv_gain scales to_k_ip / to_v_ip so that
    a route that drops the image tokens computes something visibly else."""
    shapes = ipadapter_param_shapes(cfg, plus=plus, **kw)
    proj = synth_state_dict(shapes["image_proj"], seed=seed, gain=gain)
    for k in proj:
        if k.endswith((".1.0.weight", ".1.0.bias")):
            proj[k] = synth_tensor("norm." + k, shapes["image_proj"][k], seed)
    ip = synth_state_dict(shapes["ip_adapter"], seed=seed + 1, gain=gain * kv_gain)
    return {"image_proj": proj, "ip_adapter": ip}


def synth_clip_vision_embeds(plus=False, seed=41, clip_dim=IPADAPTER_CLIP_DIM, tokens=257):
    """seeded stand-ins for the CLIP-vision outputs an IP-Adapter takes: (clip_embed, clip_embed_zeroed) -- image_embeds [1, D] and zeros for a base
    file; penultimate_hidden_states [1, 257, D] and those of a black image (a second draw) for a plus file"""
    g = torch.Generator().manual_seed(seed)
    if not plus:
        e = torch.randn(1, clip_dim, generator=g)
        return e, torch.zeros_like(e)
    return torch.randn(1, tokens, clip_dim, generator=g), torch.randn(1, tokens, clip_dim, generator=g) * 0.25


def synth_controlnet_state_dict(cfg, hint_channels=3, seed=6, zero_conv_gain=1.0, **kw):
    """cldm.ControlNet weights.  Real checkpoints start from ZERO 1x1 output convs; random ones (same init as every other conv) make the
    residuals non-trivial for parity tests."""
    from .backend.nn.layout import controlnet_param_shapes
    return synth_state_dict(controlnet_param_shapes(cfg, hint_channels), seed=seed, **kw)


def synth_control_lora_state_dict(cfg, hint_channels=3, rank=4, seed=13, delta_gain=0.5, skip_prefixes=("time_embed.",)):
    """A Control-LoRA file (patcher/controlnet.py:360-457): for the trunk's conv / linear weights a low-rank pair `<module>.up` / `<module>.down`
    that is ADDED to the UNet's own weight, everything else (norms, biases, hint block, zero convs) stored directly, plus the `lora_controlnet`
    marker.  Modules under `skip_prefixes` get no entry at all: they run on the UNet's weights unchanged."""
    from .backend.nn.layout import controlnet_param_shapes
    shapes = controlnet_param_shapes(cfg, hint_channels)
    direct = synth_state_dict(shapes, seed=seed)
    trunk = ("input_blocks.", "middle_block.", "time_embed.", "label_emb.")
    sd = OrderedDict()
    for name, shape in shapes.items():
        if name.startswith(skip_prefixes):
            continue
        if name.startswith(trunk) and name.endswith(".weight") and len(shape) >= 2:
            base = name[:-7]
            up_shape = (shape[0], rank) + (1,) * (len(shape) - 2)
            # up ~ N(0, 1/rank), down ~ N(0, (delta_gain * gain)^2 / fan_in)  =>  std(up @ down) = delta_gain * std(a synthetic weight)
            sd[base + ".up"] = synth_tensor(base + ".up", up_shape, seed, 1.0)
            sd[base + ".down"] = synth_tensor(base + ".down", (rank,) + tuple(shape[1:]), seed, delta_gain * DEFAULT_GAIN)
        else:
            sd[name] = direct[name]
    sd["lora_controlnet"] = torch.zeros(1)
    return sd


# an SD1.5-SHAPED small UNet (4 levels x 2 ResBlocks = 12 input blocks): T2I-Adapter features are placed by input-block index, so its tests
# need the real block grammar; channels 64 / 128 / 256 / 256
MINI_SD15_UNET_CONFIG = dict(
    in_channels=4, model_channels=64, out_channels=4, num_res_blocks=[2, 2, 2, 2], channel_mult=(1, 2, 4, 4), num_heads=4,
    use_spatial_transformer=True, transformer_depth=[1, 1, 1, 1, 1, 1, 0, 0], transformer_depth_middle=1,
    transformer_depth_output=[1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0], context_dim=128, use_linear_in_transformer=False)


def synth_t2i_adapter_state_dict(seed=11, **adapter_kw):
    from .backend.nn.cnets.t2i_adapter import adapter_param_shapes
    return synth_state_dict(OrderedDict(adapter_param_shapes(**adapter_kw)), seed=seed)


def synth_t2i_adapter_light_state_dict(seed=12, **adapter_kw):
    from .backend.nn.cnets.t2i_adapter import adapter_light_param_shapes
    return synth_state_dict(OrderedDict(adapter_light_param_shapes(**adapter_kw)), seed=seed)


def synth_flux_state_dict(cfg, seed=2, **kw):
    return synth_state_dict(flux_param_shapes(cfg), seed=seed, **kw)


def synth_vae_decoder_state_dict(cfg, seed=1, **kw):
    return synth_state_dict(vae_decoder_param_shapes(cfg), seed=seed, **kw)


def synth_vae_state_dict(cfg, seed=1, **kw):
    """decoder + encoder + quant convs; the decoder tensors equal synth_vae_decoder_state_dict's (pure function of the name)"""
    shapes = OrderedDict(vae_decoder_param_shapes(cfg))
    shapes.update(vae_encoder_param_shapes(cfg))
    return synth_state_dict(shapes, seed=seed, **kw)


# CLIP-L (SD1.x / SDXL first encoder) and OpenCLIP bigG (SDXL second encoder) text-model configs, and tiny twins with the
# real head width (64) for the parity tests
CLIP_L_CONFIG = dict(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, vocab_size=49408,
                     max_position_embeddings=77, hidden_act="quick_gelu")
CLIP_G_CONFIG = dict(hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=20, vocab_size=49408,
                     max_position_embeddings=77, hidden_act="gelu", add_text_projection=True)
TINY_CLIP_L_CONFIG = dict(hidden_size=128, intermediate_size=256, num_hidden_layers=3, num_attention_heads=2, vocab_size=1000,
                          max_position_embeddings=77, hidden_act="quick_gelu")
TINY_CLIP_G_CONFIG = dict(hidden_size=192, intermediate_size=320, num_hidden_layers=4, num_attention_heads=3, vocab_size=1000,
                          max_position_embeddings=77, hidden_act="gelu", add_text_projection=True)


def synth_clip_state_dict(cfg, seed=4, **kw):
    return synth_state_dict(clip_param_shapes(cfg), seed=seed, **kw)


# CLIP-vision towers (backend/nn/clip_vision.py): tiny twins with the three real head widths -- 64 (ViT-L/14, quick_gelu), 80 (ViT-H/14) and 104
# (ViT-bigG/14) -- at the real image / patch size; projection 64 = IPADAPTER_CLIP_DIM, so the tiny IP-Adapter files take their image_embeds
def _tiny_clip_vision(hidden, heads, act):
    return dict(hidden_size=hidden, intermediate_size=2 * hidden, num_hidden_layers=2, num_attention_heads=heads, hidden_act=act, projection_dim=64,
                image_size=224, patch_size=14, num_channels=3, layer_norm_eps=1e-5)


TINY_CLIP_VISION_CONFIGS = {"d64": _tiny_clip_vision(128, 2, "quick_gelu"), "d80": _tiny_clip_vision(320, 4, "gelu"), "d104": _tiny_clip_vision(832, 8, "gelu")}


def clip_vision_param_shapes(cfg):
    """transformers' CLIPVisionModelWithProjection keys: vision_model.* and visual_projection.weight"""
    c, f = cfg["hidden_size"], cfg["intermediate_size"]
    s = OrderedDict()
    p = "vision_model."
    s[p + "embeddings.class_embedding"] = (c,)
    s[p + "embeddings.patch_embedding.weight"] = (c, cfg.get("num_channels", 3), cfg.get("patch_size", 14), cfg.get("patch_size", 14))
    s[p + "embeddings.position_embedding.weight"] = ((cfg.get("image_size", 224) // cfg.get("patch_size", 14)) ** 2 + 1, c)
    s[p + "pre_layrnorm.weight"], s[p + "pre_layrnorm.bias"] = (c,), (c,)
    for i in range(cfg["num_hidden_layers"]):
        b = f"{p}encoder.layers.{i}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            s[b + f"self_attn.{n}.weight"], s[b + f"self_attn.{n}.bias"] = (c, c), (c,)
        for n in ("layer_norm1", "layer_norm2"):
            s[b + n + ".weight"], s[b + n + ".bias"] = (c,), (c,)
        s[b + "mlp.fc1.weight"], s[b + "mlp.fc1.bias"] = (f, c), (f,)
        s[b + "mlp.fc2.weight"], s[b + "mlp.fc2.bias"] = (c, f), (c,)
    s[p + "post_layernorm.weight"], s[p + "post_layernorm.bias"] = (c,), (c,)
    s["visual_projection.weight"] = (cfg["projection_dim"], c)
    return s


def synth_clip_vision_state_dict(cfg, seed=17, embed_gain=0.5, mlp_gain=(1.5, 4.0)):
    """random-init CLIP-vision tower, a pure function of (name, shape, seed): projections around the init law (N(0, 1) * DEFAULT_GAIN / sqrt(fan_in),
    biases on their weight's fan_in), every LayerNorm 1 + 0.1 N / 0.1 N, class and position embeddings N(0, embed_gain^2) -- of the order of the
    patch projection's output, so that leaving either out is visible.  mlp_gain = (fc1, fc2) factors on the MLP's two projections: at the init law's
    own gain the pre-activations are so small that erf-GELU and quick-GELU differ by 4 x the fp16 floor of the output; at (1.5, 4) they differ by 12 x"""
    shapes = clip_vision_param_shapes(cfg)
    sd = OrderedDict()
    for name, shape in shapes.items():
        z = torch.from_numpy(np.random.Generator(np.random.PCG64([seed, zlib.crc32(name.encode())])).standard_normal(shape, dtype=np.float32))
        if "norm" in name:
            z = 1.0 + 0.1 * z if name.endswith(".weight") else 0.1 * z
        elif "embeddings.class_embedding" in name or "position_embedding" in name:
            z = embed_gain * z
        else:
            wshape = shapes[name[:-5] + ".weight"] if name.endswith(".bias") else shape
            z = z * float((mlp_gain[0] if ".mlp.fc1." in name else mlp_gain[1] if ".mlp.fc2." in name else 1.0) * DEFAULT_GAIN / np.sqrt(int(np.prod(wshape[1:]))))
        sd[name] = z
    return sd


def openclip_keyed(sd, prefix="visual."):
    """a transformers-keyed CLIP-vision state dict in OpenCLIP's layout (what backend/patcher/clipvision.convert_to_transformers reads): q / k / v
    fused into attn.in_proj_*, ln_pre / ln_post, conv1, positional_embedding, proj = visual_projection.weight transposed"""
    top = {"vision_model.embeddings.class_embedding": "class_embedding", "vision_model.embeddings.patch_embedding.weight": "conv1.weight",
           "vision_model.embeddings.position_embedding.weight": "positional_embedding", "vision_model.post_layernorm.weight": "ln_post.weight",
           "vision_model.post_layernorm.bias": "ln_post.bias", "vision_model.pre_layrnorm.weight": "ln_pre.weight", "vision_model.pre_layrnorm.bias": "ln_pre.bias"}
    block = {"layer_norm1": "ln_1", "layer_norm2": "ln_2", "mlp.fc1": "mlp.c_fc", "mlp.fc2": "mlp.c_proj", "self_attn.out_proj": "attn.out_proj"}
    out = OrderedDict()
    for k, v in sd.items():
        if k in top:
            out[prefix + top[k]] = v
        elif k == "visual_projection.weight":
            out[prefix + "proj"] = v.t().contiguous()
        else:
            i, rest = k[len("vision_model.encoder.layers."):].split(".", 1)
            mod, leaf = rest.rsplit(".", 1)
            if mod == "self_attn.q_proj":
                b = f"vision_model.encoder.layers.{i}.self_attn."
                out[f"{prefix}transformer.resblocks.{i}.attn.in_proj_{leaf}"] = torch.cat([sd[f"{b}{p}_proj.{leaf}"] for p in "qkv"])
            elif mod in block:
                out[f"{prefix}transformer.resblocks.{i}.{block[mod]}.{leaf}"] = v
    return out


def synth_image(h, w, seed, batch=1):
    """uniform-random fp32 image [batch, h, w, 3] in [0, 1) (the reference's BHWC image tensors)"""
    return torch.from_numpy(np.random.Generator(np.random.PCG64([seed, 3])).random((batch, h, w, 3), dtype=np.float32))


# T5-XXL as Flux uses it (backend/huggingface/black-forest-labs/FLUX.1-dev/text_encoder_2/config.json): 24 layers, 64 heads of 64, gated tanh-GELU
T5_XXL_CONFIG = dict(d_model=4096, d_ff=10240, num_layers=24, num_heads=64, vocab_size=32128, dense_act_fn="gelu_pytorch_tanh", is_gated_act=True, model_type="t5")
TINY_T5_CONFIG = dict(d_model=128, d_ff=320, num_layers=3, num_heads=2, vocab_size=1000, dense_act_fn="gelu_pytorch_tanh", is_gated_act=True, model_type="t5")


def synth_t5_state_dict(cfg, seed=9):
    """random-init T5 encoder: N(0, 1) / sqrt(fan_in) projections, RMS-norm weights 1 + 0.1 N, token embeddings N(0, 1), bias table N(0, 0.5)"""
    from .backend.nn.layout import t5_param_shapes
    sd = OrderedDict()
    for name, shape in t5_param_shapes(cfg).items():
        rng = np.random.Generator(np.random.PCG64([seed, zlib.crc32(name.encode())]))
        if name == "logit_scale":
            sd[name] = torch.tensor(4.6055)
            continue
        z = torch.from_numpy(rng.standard_normal(shape, dtype=np.float32))
        if name.endswith("layer_norm.weight"):
            z = 1.0 + 0.1 * z
        elif name.endswith("relative_attention_bias.weight"):
            z = 0.5 * z
        elif name != "transformer.shared.weight":
            z = z / float(np.sqrt(shape[1]))
        sd[name] = z
    return sd


def synth_conditioning(batch, context_dim, adm_in_channels=None, tokens=77, seed=1234):
    """cond / uncond tensors of the shapes the text encoders would produce."""
    rng = np.random.Generator(np.random.PCG64([seed, 7]))
    c = torch.from_numpy(rng.standard_normal((batch, tokens, context_dim), dtype=np.float32))
    uc = torch.from_numpy(rng.standard_normal((batch, tokens, context_dim), dtype=np.float32))
    if adm_in_channels is None:
        return c, uc
    y = torch.from_numpy(rng.standard_normal((batch, adm_in_channels), dtype=np.float32))
    uy = torch.from_numpy(rng.standard_normal((batch, adm_in_channels), dtype=np.float32))
    return {"crossattn": c, "vector": y}, {"crossattn": uc, "vector": uy}


def synth_state_dict_device(shapes, seed, device, dtype=torch.float16, gain=DEFAULT_GAIN):
    """Same init law as `synth_state_dict`, drawn directly on the device (bench.py: 2.6 G parameters in seconds).
    Values differ from the numpy stream, so this is for throughput runs, not for parity fixtures."""
    g = torch.Generator(device=device).manual_seed(int(seed))
    sd = OrderedDict()
    for name, shape in shapes.items():
        z = torch.randn(shape, generator=g, device=device, dtype=torch.float32)
        if _is_norm(name, shape):
            z = 1.0 + 0.1 * z if name.endswith((".weight", ".scale")) else 0.1 * z
        else:
            wshape = shapes[name[:-5] + ".weight"] if name.endswith(".bias") else shape
            z = z * (gain / float(np.sqrt(int(np.prod(wshape[1:])))))
        sd[name] = z.to(dtype)
    return sd
