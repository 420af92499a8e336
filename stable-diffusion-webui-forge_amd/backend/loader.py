"""Single-file checkpoint -> native engine: counterpart of backend/loader.py (`preprocess_state_dict` :442,
`split_state_dict` :449, `forge_loader` :498) for the SD1.x / SD2.x / SDXL-base LDM layouts and Flux.1 (dev / schnell) transformers.

The reference delegates model-family detection to the `huggingface_guess` package (git lllyasviel/huggingface_guess@84826248,
`launch_utils.py:397-404`; absent here): `guess(sd)` reads the UNet hyper-parameters off the tensor shapes
(`detection.detect_unet_config`, the ComfyUI model-detection algorithm) and matches them against the known model list.
`detect_unet_config` below restates that published shape-reading algorithm for the LDM UNet; the head layout, which shapes
cannot reveal, follows the model list (context 768 -> SD1.x: 8 heads; 1024 -> SD2.x, 2048 / 1280 -> SDXL: 64 channels per head).
The native executor binds LDM parameter names directly, so no key conversion is needed for the UNet or the (LDM-layout) VAE of
a single-file checkpoint; a diffusers-keyed VAE goes through `misc.diffusers_state_dict.vae_from_diffusers` (the reference calls
`huggingface_guess.diffusers_convert.convert_vae_state_dict`, loader.py:58-59).  `detect_flux_config` restates the same package's Flux
branch.  Parity of these restatements is UNPINNED against the package itself (it is not in the image): they are anchored on the reference's
call sites, on its engines' use of the resulting configuration (diffusion_engine/flux.py:36-47), on the per-family configuration files
the reference ships under backend/huggingface/ (SD1.5, SD-inpainting, SDXL-base UNets; FLUX.1-dev / -schnell transformers and VAE) and
on round trips through the native parameter-shape tables (tests/test_loader_lora.py)."""
import torch

from .diffusion_engine.base import build_engine

UNET_PREFIX = "model.diffusion_model."
VAE_PREFIX = "first_stage_model."


def load_torch_file(path, device="cpu"):
    if isinstance(path, dict):
        return path
    if str(path).endswith((".safetensors", ".sft")):
        from safetensors.torch import load_file
        return load_file(path, device=str(device))
    if str(path).lower().endswith(".gguf"):      # utils.py:27-31: {name: GGUFTensor} (packed bytes, memory-mapped); dequantize_state_dict expands them
        from .gguf_file import load_gguf
        return load_gguf(path)
    sd = torch.load(path, map_location=device, weights_only=True)
    return sd.get("state_dict", sd)


def _is_gguf(v):
    from .gguf_file import GGUFTensor
    return isinstance(v, GGUFTensor)


def _is_packed(v):
    """a tensor the device expands: a GGUFTensor, or a PackedTensor (float8 / bitsandbytes 4-bit storage, backend/quant_state.py)"""
    from .quant_state import PackedTensor
    return _is_gguf(v) or isinstance(v, PackedTensor)


def _staged_parts(v):
    """-> [(name, flat uint8 host view)] of what one packed tensor sends to the device: its bytes, and for a bitsandbytes tensor its small side
    tensors (absmax and the tables) behind them.  Views only: nothing is copied here."""
    if _is_gguf(v):
        return [("data", v.data)]
    parts = [("data", v.data.numpy())]
    if v.state is not None:
        parts += [(name, t.view(torch.uint8).numpy()) for name in ("absmax", "code", "code2", "absmax2") for t in (getattr(v.state, name),) if t is not None]
    return parts


def _staged_layout(parts):
    """-> ([(name, offset, view)], total) for the parts of one tensor: every part at a 16-byte aligned offset of one staging segment; a tensor
    without side tensors takes exactly its own bytes"""
    layout, off, end = [], 0, 0
    for name, a in parts:
        layout.append((name, off, a))
        end = off + a.nbytes
        off = (end + 15) // 16 * 16
    return layout, end


@torch.inference_mode()
def dequantize_state_dict(sd, device="cuda", dtype=torch.bfloat16):
    """Materialise a state dict read from a GGUF file: every GGUFTensor is copied to the device as packed bytes and expanded there into a `dtype`
    (fp16 / bf16) tensor of its shape by the fmx_gguf_dequant kernels; ordinary tensors pass through untouched.  PackedTensor values (float8 and
    bitsandbytes NF4 / FP4 storage, backend/quant_state.py) take the same route through fmx_fp8_expand / fmx_bnb4_dequant; a bitsandbytes
    tensor's side tensors (absmax, tables) are staged behind its bytes, in the same copy.  The reference keeps the blocks and
    dequantises inside every forward (operations_gguf.py); here the weights become the resident 16-bit tensors the executors consume, once.

    Staging: two pinned host buffers of the largest tensor's packed size, used alternately, and one side stream.  Tensor i+1 is copied into its
    pinned buffer by the host and sent to the device while tensor i's kernel runs; an event per buffer keeps the host from overwriting bytes whose
    copy is still in flight.  The packed device copy is freed to the stream-ordered allocator as soon as its kernel is queued, so the extra device
    memory at any time is a couple of tensors' packed bytes, not the file's."""
    from .. import hipops
    if not any(_is_packed(v) for v in sd.values()):
        return sd
    # F32 / F16 / BF16 tensors of the file (norm scales, biases, tables) are ordinary tensors of their own type, as the reference keeps them:
    # consumers that want fp32 (the T5 bias table) get every stored bit; the executors cast the rest when they bind them
    plain = {0: torch.float32, 1: torch.float16, 30: torch.bfloat16}
    sd = {k: (torch.from_numpy(v.data.copy()).view(plain[v.qtype]).reshape(v.shape) if _is_gguf(v) and v.qtype in plain else v) for k, v in sd.items()}
    todo = [(k, v, *_staged_layout(_staged_parts(v))) for k, v in sd.items() if _is_packed(v)]      # views and offsets: no bytes are read yet
    if not todo:
        return sd
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("GGUF, float8 and bitsandbytes tensors are expanded on the GPU: device must be a cuda device")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    out = dict(sd)
    cap = max(n for _, _, _, n in todo)
    pinned = [torch.empty(cap, dtype=torch.uint8).pin_memory() for _ in range(2)]
    free = [None, None]                 # event: the buffer's last host-to-device copy has completed
    with torch.cuda.device(device):
        stream = torch.cuda.Stream(device)
        stream.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(stream):
            for i, (k, v, layout, n) in enumerate(todo):
                slot = i & 1
                if free[slot] is not None:
                    free[slot].synchronize()
                stage = pinned[slot][:n]
                for _, off, a in layout:
                    stage.numpy()[off:off + a.nbytes] = a                   # page-in + copy from the mapping: the file read
                raw = torch.empty(n, dtype=torch.uint8, device=device)
                raw.copy_(stage, non_blocking=True)
                free[slot] = torch.cuda.Event()
                free[slot].record(stream)
                if _is_gguf(v):
                    out[k] = hipops.gguf_dequant(raw, v.qtype, v.shape, dtype)
                elif v.state is None:
                    out[k] = hipops.fp8_expand(raw, v.scheme, v.shape, dtype)
                else:
                    dev = {name: raw[off:off + a.nbytes] for name, off, a in layout}
                    f32 = lambda t: t.view(torch.float32) if t is not None else None  # noqa: E731
                    state = v.state._replace(code=f32(dev["code"]), absmax=dev["absmax"] if v.state.nested else f32(dev["absmax"]),
                                             code2=f32(dev.get("code2")), absmax2=f32(dev.get("absmax2")))
                    out[k] = hipops.bnb4_dequant(dev["data"], state, dtype)
                    del dev, state
                del raw                                                     # allocated and freed on this stream: reusable by the next tensor
        torch.cuda.current_stream(device).wait_stream(stream)
        stream.synchronize()
    return out


# llama.cpp tensor names of a T5 encoder (the GGUF files city96 publishes) -> HF names: the key map of loader.py:185-199, applied the same way
# (every replacement, in this order, on every key)
T5_LLAMA_KEY_MAP = (("enc.", "encoder."), (".blk.", ".block."), ("token_embd", "shared"), ("output_norm", "final_layer_norm"),
                    ("attn_q", "layer.0.SelfAttention.q"), ("attn_k", "layer.0.SelfAttention.k"), ("attn_v", "layer.0.SelfAttention.v"),
                    ("attn_o", "layer.0.SelfAttention.o"), ("attn_norm", "layer.0.layer_norm"),
                    ("attn_rel_b", "layer.0.SelfAttention.relative_attention_bias"), ("ffn_up", "layer.1.DenseReluDense.wi_1"),
                    ("ffn_down", "layer.1.DenseReluDense.wo"), ("ffn_gate", "layer.1.DenseReluDense.wi_0"), ("ffn_norm", "layer.1.layer_norm"))
T5_PREFIX = "text_encoders.t5xxl.transformer."        # where a Flux checkpoint keeps its text encoders (huggingface_guess' Flux prefixes)
CLIP_L_PREFIX = "text_encoders.clip_l.transformer."


def t5_llama_key(k):
    for s, d in T5_LLAMA_KEY_MAP:
        k = k.replace(s, d)
    return k


def replace_state_dict(sd, asd):
    """loader.py:181-300 for the components that exist on the native path: merge an additional state dict (a VAE, a CLIP-L or a T5 file that comes
    beside a transformer-only checkpoint) into the checkpoint dict `sd` under the prefix the Flux layout keeps that component at, replacing
    what was there.  Recognised by the same probe keys as the reference: `decoder.conv_in.weight` (VAE), `enc.blk.0.attn_k.weight` (T5 in
    llama.cpp naming, renamed first), `encoder.block.0.layer.0.SelfAttention.k.weight` (T5, HF naming),
    `text_model.encoder.layers.0.layer_norm1.weight` (CLIP-L, 768 wide).  -> sd (modified in place)."""
    if "enc.blk.0.attn_k.weight" in asd:
        asd = {t5_llama_key(k): v for k, v in asd.items()}

    def put(prefix, part):
        for k in [k for k in sd if k.startswith(prefix)]:
            del sd[k]
        for k, v in part.items():
            sd[prefix + k] = v

    if "decoder.conv_in.weight" in asd:
        put("vae." if flux_prefix(sd) is not None else VAE_PREFIX, asd)
    elif "encoder.block.0.layer.0.SelfAttention.k.weight" in asd:
        put(T5_PREFIX, asd)
    elif "text_model.encoder.layers.0.layer_norm1.weight" in asd and asd["text_model.encoder.layers.0.layer_norm1.weight"].shape[0] == 768:
        put(CLIP_L_PREFIX, asd)
    else:
        raise NotImplementedError("additional state dict not recognised: expected a VAE (decoder.conv_in.weight), a CLIP-L "
                                  "(text_model.encoder.layers.0.layer_norm1.weight, 768 wide) or a T5 encoder (HF or llama.cpp names)")
    return sd


def preprocess_state_dict(sd):
    """loader.py:442-446: a bare UNet state dict gets the checkpoint prefix."""
    if not any(k.startswith("model.diffusion_model") for k in sd.keys()):
        sd = {f"model.diffusion_model.{k}": v for k, v in sd.items()}
    return sd


def _count(sd, fmt):
    n = 0
    while fmt.format(n) in sd:
        n += 1
    return n


def detect_unet_config(sd, prefix=UNET_PREFIX):
    """LDM UNet hyper-parameters from tensor shapes (see the module docstring)."""
    g = lambda k: sd[prefix + k]  # noqa: E731
    has = lambda k: (prefix + k) in sd  # noqa: E731
    mc = g("input_blocks.0.0.weight").shape[0]
    cfg = dict(in_channels=g("input_blocks.0.0.weight").shape[1], model_channels=mc, out_channels=g("out.2.weight").shape[0],
               use_spatial_transformer=True)
    if has("label_emb.0.0.weight"):
        cfg["adm_in_channels"] = g("label_emb.0.0.weight").shape[1]
        cfg["num_classes"] = "sequential"
    channel_mult, num_res_blocks, depth_in = [], [], []
    context_dim, use_linear = None, False

    def tdepth(block):
        nonlocal context_dim, use_linear
        d = 0
        while has(f"{block}.1.transformer_blocks.{d}.norm1.weight"):
            d += 1
        if d:
            context_dim = g(f"{block}.1.transformer_blocks.0.attn2.to_k.weight").shape[1]
            use_linear = g(f"{block}.1.proj_in.weight").dim() == 2
        return d

    i, res_in_level = 1, 0
    while has(f"input_blocks.{i}.0.in_layers.0.weight") or has(f"input_blocks.{i}.0.op.weight"):
        if has(f"input_blocks.{i}.0.op.weight"):
            num_res_blocks.append(res_in_level)
            res_in_level = 0
        else:
            out_ch = g(f"input_blocks.{i}.0.out_layers.3.weight").shape[0]
            if res_in_level == 0:
                channel_mult.append(out_ch // mc)
            res_in_level += 1
            depth_in.append(tdepth(f"input_blocks.{i}"))
        i += 1
    num_res_blocks.append(res_in_level)
    cfg["channel_mult"] = tuple(channel_mult)
    cfg["num_res_blocks"] = num_res_blocks
    cfg["transformer_depth"] = depth_in
    cfg["transformer_depth_middle"] = _count(sd, prefix + "middle_block.1.transformer_blocks.{}.norm1.weight") if has("middle_block.1.norm.weight") else -1
    if cfg["transformer_depth_middle"] > 0 and context_dim is None:
        context_dim = g("middle_block.1.transformer_blocks.0.attn2.to_k.weight").shape[1]
        use_linear = g("middle_block.1.proj_in.weight").dim() == 2
    depth_out = []
    o = 0
    while has(f"output_blocks.{o}.0.in_layers.0.weight"):
        depth_out.append(tdepth(f"output_blocks.{o}"))
        o += 1
    cfg["transformer_depth_output"] = depth_out[::-1]  # consumed with pop() from the end (unet.py:649)
    cfg["context_dim"] = context_dim
    cfg["use_linear_in_transformer"] = bool(use_linear)
    if context_dim == 768:
        cfg["num_heads"] = 8                 # SD1.x
    else:
        cfg["num_head_channels"] = 64        # SD2.x / SDXL / refiner
    return cfg


def detect_vae_config(vae_sd, **constants):
    """AutoencoderKL structure from an LDM-keyed VAE state dict (widths per level, ResBlocks per level, latent channels, quant convs); what no
    tensor carries (scaling / shift factor) comes in as `constants`."""
    n = _count(vae_sd, "decoder.up.{}.block.0.conv1.weight")
    return dict(in_channels=vae_sd["encoder.conv_in.weight"].shape[1] if "encoder.conv_in.weight" in vae_sd else 3,
                out_channels=vae_sd["decoder.conv_out.weight"].shape[0],
                block_out_channels=tuple(vae_sd[f"decoder.up.{l}.block.0.conv1.weight"].shape[0] for l in range(n)),
                layers_per_block=_count(vae_sd, "decoder.up.0.block.{}.conv1.weight") - 1, latent_channels=vae_sd["decoder.conv_in.weight"].shape[1],
                use_quant_conv="quant_conv.weight" in vae_sd, use_post_quant_conv="post_quant_conv.weight" in vae_sd, **constants)


def _vae_as_stored(vae, prefix):
    """VAEs stay as stored: the reference builds the VAE in its own type whatever the file's, so a float8 tensor is only cast (here: to its exact
    fp32 values, on the host, before any key conversion touches it); a bitsandbytes tensor has no meaning there and is refused by key."""
    from .quant_state import is_packed
    out = {}
    for k, v in vae.items():
        if is_packed(v):
            if not v.is_fp8:
                raise NotImplementedError(f"{prefix}{k}: bitsandbytes {v.scheme} storage is not served for a VAE")
            v = v.host_float()
        out[k] = v
    return out


def flux_prefix(sd):
    """-> key prefix of a Flux transformer inside `sd` ('model.diffusion_model.' in full checkpoints, '' in transformer-only files), or None."""
    for prefix in (UNET_PREFIX, ""):
        if prefix + "double_blocks.0.img_attn.norm.key_norm.scale" in sd:
            return prefix
    return None


def detect_flux_config(sd, prefix=UNET_PREFIX):
    """Flux hyper-parameters.  huggingface_guess (absent here) keys the family on `double_blocks.0.img_attn.norm.key_norm.scale`, counts the
    double / single blocks, reads `guidance_embed` off the presence of `guidance_in.in_layer.weight` and fills every other field with the
    Flux.1 constants; here the widths are read off the tensors instead (identical for Flux.1 files, and it keeps reduced-size twins
    loadable), head_dim is the norm scale's length, and the rotary split / theta -- which no tensor carries -- are Flux.1's."""
    g = lambda k: sd[prefix + k]  # noqa: E731
    hidden = g("img_in.weight").shape[0]
    head_dim = g("double_blocks.0.img_attn.norm.key_norm.scale").shape[0]
    if head_dim != 128:
        raise NotImplementedError(f"Flux head_dim {head_dim}: the rotary split [16, 56, 56] is defined for 128")
    return dict(in_channels=g("img_in.weight").shape[1] // 4, vec_in_dim=g("vector_in.in_layer.weight").shape[1],
                context_in_dim=g("txt_in.weight").shape[1], hidden_size=hidden, mlp_ratio=g("double_blocks.0.img_mlp.0.weight").shape[0] / hidden,
                num_heads=hidden // head_dim, depth=_count(sd, prefix + "double_blocks.{}.img_attn.qkv.weight"),
                depth_single_blocks=_count(sd, prefix + "single_blocks.{}.linear1.weight"), axes_dim=[16, 56, 56], theta=10000,
                qkv_bias=(prefix + "double_blocks.0.img_attn.qkv.bias") in sd, guidance_embed=(prefix + "guidance_in.in_layer.weight") in sd)


FLUX_VAE_PREFIXES = ("vae.", VAE_PREFIX)  # Forge's own Flux checkpoints store the VAE under 'vae.', converted LDM ones under 'first_stage_model.'


def split_flux_state_dict(sd):
    """Flux counterpart of split_state_dict: -> ({'transformer', 'vae'}, guess).  The compute type follows the stored tensors as the reference's
    loader does (bf16 files -> bf16, fp16 files -> fp16; fp32 files run in bf16, the reference's first choice for Flux; GGUF files and wrapped
    float8 / bitsandbytes nf4 / fp4 files (quant_state.wrap_quantized_state_dict, applied by forge_loader) -> bf16).  Raw float8 tensors are
    refused: only wrapped ones are accepted.  Shapes are all that is read here, so packed tensors need no expansion yet."""
    prefix = flux_prefix(sd)
    tr = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix) and not k.startswith(FLUX_VAE_PREFIXES + ("text_encoders.",))}
    vae = {}
    from .misc.diffusers_state_dict import vae_from_diffusers
    for vp in FLUX_VAE_PREFIXES:
        vae = {k[len(vp):]: v for k, v in sd.items() if k.startswith(vp)}
        if vae:
            vae = vae_from_diffusers(_vae_as_stored(vae, vp))
            break
    probe = tr["img_in.weight"]
    # a GGUF file runs in bf16, the reference's first choice for Flux; its tensors are expanded by dequantize_state_dict
    stored = torch.bfloat16 if _is_packed(probe) else probe.dtype
    if stored not in (torch.float16, torch.bfloat16, torch.float32):
        raise NotImplementedError(f"Flux state dict holds raw {stored} tensors: float8 and bitsandbytes nf4 / fp4 storage is loaded through forge_loader, "
                                  "which wraps such tensors first (quant_state.wrap_quantized_state_dict)")
    guess = {"flux_config": detect_flux_config(sd, prefix), "vae_config": detect_vae_config(vae, scaling_factor=0.3611, shift_factor=0.1159) if vae else None, "is_flux": True,
             "dtype": torch.float16 if stored == torch.float16 else torch.bfloat16,
             "ignored": sorted({k.split(".")[0] for k in sd if not k.startswith((prefix,) + FLUX_VAE_PREFIXES)} if prefix else set())}
    # text encoders that ride in the checkpoint dict (additional_state_dicts): handed out as state dicts for IntegratedT5 / IntegratedCLIP
    encoders = {name: {"transformer." + k[len(p):]: v for k, v in sd.items() if k.startswith(p)} for name, p in (("t5xxl", T5_PREFIX), ("clip_l", CLIP_L_PREFIX))}
    return {"transformer": tr, "vae": vae, "text_encoders": {n: e for n, e in encoders.items() if e}}, guess


def split_state_dict(sd):
    """loader.py:449-486 without the text encoders: -> ({'unet': ..., 'vae': ...}, guess dict).  A float8-stored checkpoint comes back with its
    UNet as the reference's fp8 storage leaves it (quant_state.mirror_fp8_storage), every tensor a PackedTensor for dequantize_state_dict to
    expand; bitsandbytes storage is not served for this family."""
    from .quant_state import is_packed, mirror_fp8_storage, wrap_quantized_state_dict
    sd = wrap_quantized_state_dict(preprocess_state_dict(load_torch_file(sd)))
    for k, v in sd.items():
        if is_packed(v) and not v.is_fp8:
            raise NotImplementedError(f"{k}: bitsandbytes {v.scheme} storage is loaded for Flux transformers and T5 encoders; SD / SDXL checkpoints are not served")
    unet = mirror_fp8_storage({k[len(UNET_PREFIX):]: v for k, v in sd.items() if k.startswith(UNET_PREFIX)}, "unet")
    vae = {k[len(VAE_PREFIX):]: v for k, v in sd.items() if k.startswith(VAE_PREFIX)}
    vae = {k: v for k, v in vae.items() if not k.startswith(("loss.", "model_ema."))}
    from .misc.diffusers_state_dict import vae_from_diffusers
    vae = vae_from_diffusers(_vae_as_stored(vae, VAE_PREFIX))   # loader.py:58-59
    unet_config = detect_unet_config(sd)
    is_sdxl = unet_config.get("adm_in_channels") is not None
    vae_config = detect_vae_config(vae, scaling_factor=0.13025 if is_sdxl else 0.18215, shift_factor=0.0) if vae else None
    # the prediction type is not in the tensor shapes: checkpoints mark it with a 'v_pred' key (and 'ztsnr' for a zero-terminal-SNR schedule,
    # loader.py:462); a yaml next to the file or the caller decides otherwise (loader.py:543-567) -> forge_loader(prediction_type=...)
    pred = "v_prediction" if "v_pred" in sd else "epsilon"
    # SD2.x-768 v-prediction checkpoints carry NO marker key.  huggingface_guess (the package the reference's loader.py:567 takes
    # model_type from; absent here, restated) tells them from SD2.x-base (epsilon) by a statistic of one trained tensor: the standard
    # deviation of output_blocks.11.1.transformer_blocks.0.norm1.bias exceeds 0.09 for the v-prediction models (SD2.x: context_dim
    # 1024, 4 input channels).  Loading such a file as epsilon produces garbage images silently, so the heuristic is applied and reported.
    pred_source = "marker key" if "v_pred" in sd else "default"
    probe = UNET_PREFIX + "output_blocks.11.1.transformer_blocks.0.norm1.bias"
    if pred == "epsilon" and unet_config.get("context_dim") == 1024 and unet_config.get("in_channels") == 4 and not is_sdxl and probe in sd:
        if float((sd[probe].host_float() if is_packed(sd[probe]) else sd[probe].float()).std(unbiased=False)) > 0.09:   # the population form, as huggingface_guess computes it
            pred, pred_source = "v_prediction", "SD2.x norm1.bias statistic (std > 0.09)"
    guess = {"unet_config": unet_config, "vae_config": vae_config, "is_sdxl": is_sdxl, "prediction_type": pred, "prediction_type_source": pred_source,
             "ztsnr": "ztsnr" in sd, "ignored": sorted({k.split(".")[0] for k in sd if not k.startswith((UNET_PREFIX, VAE_PREFIX))})}
    return {"unet": unet, "vae": vae}, guess


@torch.inference_mode()
def forge_loader(sd, loras=None, device="cuda", prediction_type=None, additional_state_dicts=None, dtype=None):
    """checkpoint path / state dict (+ optional [(lora_sd, strength)]) -> ForgeDiffusionEngine on the native executors.
    prediction_type: 'epsilon' | 'v_prediction' | 'edm' to override what the checkpoint's marker keys say (SD2.x-768, v-pred SDXL finetunes).
    additional_state_dicts: further files / dicts (VAE, CLIP-L, T5) merged into the checkpoint by replace_state_dict, as the reference's keyword
    (loader.py:449-452, :498): a Flux GGUF holds the transformer only.  dtype: compute type of a Flux transformer, overriding the stored one.
    `.gguf` inputs are dequantised on the device (dequantize_state_dict); the text encoders' state dicts are left on the engine as
    `engine.text_encoder_state_dicts` ({'t5xxl': ..., 'clip_l': ...}, keys as IntegratedT5 / IntegratedCLIP take them).
    float8 and bitsandbytes nf4 / fp4 storage (flux1-dev-fp8, t5xxl_fp8_e4m3fn, flux1-dev-bnb-nf4) takes the same device route: the tensors are
    wrapped (quant_state.wrap_quantized_state_dict), each component is brought to what the reference's storage type makes of it
    (quant_state.mirror_fp8_storage: per component, wider tensors of an fp8-majority component are rounded to fp8) and expanded once into 16-bit
    weights.  Served: Flux transformers (fp8, nf4, fp4), T5 (fp8, nf4, fp4) and CLIP-L (fp8) side files, SD / SDXL UNets (fp8)."""
    from .patcher.lora import merge_loras_into_state_dict
    from .quant_state import is_packed, mirror_fp8_storage, wrap_quantized_state_dict
    sd = load_torch_file(sd)
    if additional_state_dicts:
        sd = dict(sd)
        for asd in additional_state_dicts:
            replace_state_dict(sd, load_torch_file(asd))
    sd = wrap_quantized_state_dict(sd)
    if flux_prefix(sd) is not None:
        from .diffusion_engine.base import build_flux_engine
        from .patcher.lora import merge_loras_into_flux_state_dict
        parts, guess = split_flux_state_dict(sd)
        if dtype is not None:
            guess["dtype"] = dtype
        for k, v in parts["text_encoders"].get("clip_l", {}).items():
            if is_packed(v) and not v.is_fp8:
                raise NotImplementedError(f"{CLIP_L_PREFIX}{k[len('transformer.'):]}: bitsandbytes {v.scheme} storage is not served for CLIP-L")
        parts["transformer"] = mirror_fp8_storage(parts["transformer"], "flux")
        if "t5xxl" in parts["text_encoders"]:      # CLIP-L is built in its own type whatever the file's: its fp8 tensors are only expanded
            parts["text_encoders"]["t5xxl"] = mirror_fp8_storage(parts["text_encoders"]["t5xxl"], "t5")
        parts["transformer"] = dequantize_state_dict(parts["transformer"], device, guess["dtype"])
        parts["vae"] = dequantize_state_dict(parts["vae"], device, torch.float16)
        tsd, report = parts["transformer"], None
        if loras:   # native and diffusers-named Flux LoRAs (comfyui_lora_collection/lora.py:286-299, :342-347), merged offline like the UNet's
            tsd, report = merge_loras_into_flux_state_dict(tsd, guess["flux_config"], [(load_torch_file(l), s) for l, s in loras], device=device, dtype=guess["dtype"])
        engine = build_flux_engine(guess["flux_config"], tsd, device=device, vae_config=guess["vae_config"],
                                   vae_state_dict=parts["vae"] or None, dtype=guess["dtype"])
        engine.lora_report = report
        engine.model_guess = guess
        engine.text_encoder_state_dicts = {n: dequantize_state_dict(e, device, guess["dtype"]) for n, e in parts["text_encoders"].items()}
        return engine
    if any(_is_gguf(v) for v in sd.values()):
        raise NotImplementedError("GGUF checkpoints are loaded for Flux transformers (and their VAE / text encoder side files); "
                                  "SD / SDXL UNets in GGUF are not on the native path")
    parts, guess = split_state_dict(sd)
    if prediction_type is not None:
        guess["prediction_type"] = prediction_type
    unet_sd = dequantize_state_dict(parts["unet"], device, torch.float16)      # fp8 storage: expanded to the UNet's compute type (every code fits)
    report = None
    if loras:
        unet_sd, report = merge_loras_into_state_dict(unet_sd, guess["unet_config"], [(load_torch_file(l), s) for l, s in loras], device=device)
    engine = build_engine(guess["unet_config"], unet_sd, guess["vae_config"], parts["vae"] or None, device=device,
                          prediction_type=guess["prediction_type"], ztsnr=guess["ztsnr"])
    engine.lora_report = report
    engine.model_guess = guess
    return engine
