"""CPU: checkpoint splitting / model-family detection / LoRA key maps and patch parsing of forge_amd.backend.{loader,patcher.lora}
against fixtures produced by the REAL reference (oracle/make_golden.py gen_lora), against what the reference's own functions returned
(tests/golden/ref_lora_key_maps.json.gz) and against the configuration files it ships (tests/golden/hf_configs/; both by oracle/make_ref_fixtures.py)."""
import gzip
import hashlib
import json
import os

import pytest
import torch

import forge_amd  # noqa: F401
from forge_amd import synth
from forge_amd.backend import loader
from forge_amd.backend.misc.diffusers_state_dict import unet_to_diffusers
from forge_amd.backend.nn.layout import unet_param_shapes, vae_decoder_param_shapes, vae_encoder_param_shapes
from forge_amd.backend.patcher import lora as nlora
from conftest import GOLDEN, load_golden

HF_CONFIGS = os.path.join(GOLDEN, "hf_configs")   # backend/huggingface/ of the reference: the files the detection tests read


def _ref_key_maps():
    with gzip.open(os.path.join(GOLDEN, "ref_lora_key_maps.json.gz"), "rt") as f:
        return json.load(f)


def _meta_sd(shapes, prefix=""):
    return {prefix + k: torch.empty(v, device="meta") for k, v in shapes.items()}


SD21_UNET_CONFIG = dict(in_channels=4, model_channels=320, out_channels=4, num_res_blocks=[2, 2, 2, 2], channel_mult=(1, 2, 4, 4), num_head_channels=64,
                        use_spatial_transformer=True, transformer_depth=[1, 1, 1, 1, 1, 1, 0, 0], transformer_depth_middle=1,
                        transformer_depth_output=[1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0], context_dim=1024, use_linear_in_transformer=True)
SDXL_REFINER_UNET_CONFIG = dict(in_channels=4, model_channels=384, out_channels=4, num_res_blocks=[2, 2, 2, 2], channel_mult=(1, 2, 4, 4), num_head_channels=64,
                                use_spatial_transformer=True, transformer_depth=[0, 0, 4, 4, 4, 4, 0, 0], transformer_depth_middle=4,
                                transformer_depth_output=[0, 0, 0, 4, 4, 4, 4, 4, 4, 0, 0, 0], context_dim=1280, use_linear_in_transformer=True,
                                adm_in_channels=2560, num_classes="sequential")


@pytest.mark.parametrize("name,cfg", [("sd15", synth.SD15_UNET_CONFIG), ("sdxl", synth.SDXL_UNET_CONFIG), ("sd21", SD21_UNET_CONFIG),
                                      ("sdxl_refiner", SDXL_REFINER_UNET_CONFIG), ("sd15_inpaint", dict(synth.SD15_UNET_CONFIG, in_channels=9))])
def test_detect_unet_config_from_shapes(name, cfg):
    det = loader.detect_unet_config(_meta_sd(unet_param_shapes(cfg), loader.UNET_PREFIX))
    assert unet_param_shapes(det) == unet_param_shapes(cfg)
    for k in ("num_heads", "num_head_channels", "context_dim", "use_linear_in_transformer", "adm_in_channels"):
        assert det.get(k) == cfg.get(k), k


def test_split_state_dict_single_file_layout():
    cfg = synth.SDXL_UNET_CONFIG
    sd = _meta_sd(unet_param_shapes(cfg), loader.UNET_PREFIX)
    vshapes = dict(vae_decoder_param_shapes(synth.SDXL_VAE_CONFIG))
    vshapes.update(vae_encoder_param_shapes(synth.SDXL_VAE_CONFIG))
    sd.update(_meta_sd(vshapes, loader.VAE_PREFIX))
    sd["conditioner.embedders.0.transformer.text_model.embeddings.position_ids"] = torch.empty(1, 77, device="meta")
    sd["first_stage_model.loss.logvar"] = torch.empty(1, device="meta")
    parts, guess = loader.split_state_dict(sd)
    assert set(parts["unet"]) == set(unet_param_shapes(cfg))
    assert set(parts["vae"]) == set(vshapes)
    assert guess["is_sdxl"] and guess["vae_config"]["scaling_factor"] == 0.13025 and guess["ignored"] == ["conditioner"]
    assert guess["vae_config"] == synth.SDXL_VAE_CONFIG      # structure read off the tensors + the family's scaling constant
    assert guess["prediction_type"] == "epsilon" and not guess["ztsnr"]
    sd["v_pred"], sd["ztsnr"] = torch.empty(0, device="meta"), torch.empty(0, device="meta")   # marker keys of v-prediction / zero-terminal-SNR checkpoints
    _, guess_v = loader.split_state_dict(sd)
    assert guess_v["prediction_type"] == "v_prediction" and guess_v["ztsnr"]
    # a bare UNet state dict gets the checkpoint prefix (loader.py:442-446)
    bare = loader.preprocess_state_dict(_meta_sd(unet_param_shapes(synth.SD15_UNET_CONFIG)))
    assert all(k.startswith(loader.UNET_PREFIX) for k in bare)


def test_sd2_v_prediction_is_recognised_without_a_marker_key():
    """SD2.x-768 (v-prediction) and SD2.x-base (epsilon) share every tensor shape and carry no marker: the trained bias of
    output_blocks.11.1.transformer_blocks.0.norm1 decides (std > 0.09 -> v-prediction), as huggingface_guess does for the reference."""
    shapes = unet_param_shapes(SD21_UNET_CONFIG)
    probe = loader.UNET_PREFIX + "output_blocks.11.1.transformer_blocks.0.norm1.bias"
    assert probe[len(loader.UNET_PREFIX):] in shapes
    g = torch.Generator().manual_seed(0)
    for std, want in ((0.02, "epsilon"), (0.15, "v_prediction")):
        sd = _meta_sd(shapes, loader.UNET_PREFIX)
        sd[probe] = torch.randn(shapes[probe[len(loader.UNET_PREFIX):]], generator=g) * std
        _, guess = loader.split_state_dict(sd)
        assert guess["prediction_type"] == want, (std, guess["prediction_type"], guess["prediction_type_source"])
    # the statistic is an SD2.x rule: an SD1.5 UNet (context 768) with a wild bias stays epsilon
    s15 = unet_param_shapes(synth.SD15_UNET_CONFIG)
    sd = _meta_sd(s15, loader.UNET_PREFIX)
    sd[probe] = torch.randn(s15[probe[len(loader.UNET_PREFIX):]], generator=g)
    assert loader.split_state_dict(sd)[1]["prediction_type"] == "epsilon"


def _key_map(cfg):
    return nlora.model_lora_keys_unet(list(unet_param_shapes(cfg)), cfg)


def test_lora_key_map_matches_reference_fixture():
    g = load_golden("tiny_sd15_lora_merge.pt")
    km = _key_map(synth.TINY_SD15_UNET_CONFIG)
    txt = "\n".join(f"{a}\t{b}" for a, b in sorted(km.items()))
    assert len(km) == g["key_map_len"]
    assert hashlib.sha256(txt.encode()).hexdigest() == g["key_map_sha256"]


@pytest.mark.parametrize("cfg", [synth.SD15_UNET_CONFIG, synth.SDXL_UNET_CONFIG, synth.TINY_SDXL_UNET_CONFIG])
def test_lora_key_map_and_diffusers_names_vs_reference(cfg):
    """unet_to_diffusers and the LoRA key map against the reference's unet_to_diffusers / model_lora_keys_unet on the same configuration."""
    name = {id(synth.SD15_UNET_CONFIG): "sd15", id(synth.SDXL_UNET_CONFIG): "sdxl", id(synth.TINY_SDXL_UNET_CONFIG): "tiny_sdxl"}[id(cfg)]
    ref = _ref_key_maps()["unet"][name]
    assert ref["unet_to_diffusers"] == unet_to_diffusers(cfg)
    assert ref["model_lora_keys_unet"] == _key_map(cfg)


def test_load_lora_patch_parsing():
    from oracle.make_golden import synth_lora
    g = load_golden("tiny_sd15_lora_merge.pt")
    cfg = synth.TINY_SD15_UNET_CONFIG
    patch_dict, remaining = nlora.load_lora(synth_lora(cfg), _key_map(cfg))
    assert sorted(remaining) == g["remaining"]
    assert {k[len("diffusion_model."):] for k in patch_dict} == set(g["merged"])
    kinds = {k: v[0] for k, v in patch_dict.items()}
    assert kinds["diffusion_model.out.2.weight"] == "set" and kinds["diffusion_model.output_blocks.5.0.emb_layers.1.bias"] == "diff"
    assert patch_dict["diffusion_model.output_blocks.5.0.in_layers.2.weight"][1][3] is not None  # Tucker mid tensor kept


def test_lycoris_and_dora_merge_vs_reference():
    """LoHa (linear / Tucker conv), LoKr (full x low-rank, low-rank x 4-d), GLoRA (square / non-square), DoRA on LoRA / LoHa / LoKr (output- and
    input-axis norms), w_norm / b_norm: the native parser + merge against the reference's load_lora + merge_lora_to_weight (fp16 weights, fp32
    computation).  These branches are load-time weight algebra in torch, so they run on the CPU here as they do on the device."""
    from oracle.make_golden import synth_lycoris
    g = load_golden("tiny_sd15_lycoris_merge.pt")
    cfg = synth.TINY_SD15_UNET_CONFIG
    sd = {k: v.half() for k, v in synth.synth_unet_state_dict(cfg, seed=0).items()}
    patch_dict, remaining = nlora.load_lora(synth_lycoris(cfg), _key_map(cfg))
    assert sorted(remaining) == g["remaining"]
    assert {k[len("diffusion_model."):]: v[0] for k, v in patch_dict.items()} == g["kinds"]
    for mk, pv in patch_dict.items():
        k = mk[len("diffusion_model."):]
        got = nlora.merge_lora_to_weight([(g["strength"], pv, 1.0, None, None)], sd[k].clone(), key=k, device="cpu")
        want = g["merged_every_5th"][k]
        assert got.dtype == torch.float16
        err = (got.flatten()[::5].float() - want.float()).abs().max() / want.float().abs().max()
        assert err < 2e-3, (k, pv[0], float(err))  # one fp16 rounding of the result; the reference rounds W + delta the same way


def test_control_lora_weight_assembly_matches_the_oracle():
    """Host side of Control-LoRA (backend/patcher/controlnet.py control_lora_state_dict / load_controlnet) against oracle/controlnet.py, which is
    pinned to the reference's ControlLora (tests/golden/*_control_lora.pt)."""
    from forge_amd.backend.patcher import controlnet as pc
    from oracle import controlnet as ocn
    cfg = synth.TINY_SDXL_UNET_CONFIG
    unet_sd = synth.synth_unet_state_dict(cfg, seed=0)
    cl = synth.synth_control_lora_state_dict(cfg)
    trunk = {k: v for k, v in unet_sd.items() if k.startswith(("input_blocks.", "middle_block.", "time_embed.", "label_emb."))}
    got, want = pc.control_lora_state_dict(trunk, cl), ocn.control_lora_weights(unet_sd, cl)
    assert set(got) == set(want)
    for k in want:
        torch.testing.assert_close(got[k].float(), want[k], rtol=1e-6, atol=1e-7)
    obj = pc.load_controlnet(cl, device="cpu")
    assert isinstance(obj, pc.ControlLora) and obj.copy().control_weights is cl
    with pytest.raises(ValueError):
        pc.load_controlnet({"foo": torch.zeros(1)})


def _vae_ldm_to_diffusers_names(sd, n_levels):
    """Test-side inverse of vae_from_diffusers, written from the module structure of diffusers' AutoencoderKL (Encoder / Decoder with
    DownEncoderBlock2D / UpDecoderBlock2D / UNetMidBlock2D + Attention), not from the product's rules."""
    out = {}
    for k, v in sd.items():
        parts = k.split(".")
        if parts[1] in ("down", "up"):
            side, level = parts[0], int(parts[2])
            blk = f"{side}.{'down_blocks' if parts[1] == 'down' else 'up_blocks'}.{level if parts[1] == 'down' else n_levels - 1 - level}"
            if parts[3] == "block":
                tail = ".".join(parts[5:]).replace("nin_shortcut", "conv_shortcut")
                k2 = f"{blk}.resnets.{parts[4]}.{tail}"
            else:
                k2 = f"{blk}.{'downsamplers' if parts[3] == 'downsample' else 'upsamplers'}.0.conv.{parts[-1]}"
        elif parts[1] == "mid" and parts[2].startswith("block_"):
            k2 = f"{parts[0]}.mid_block.resnets.{int(parts[2][6:]) - 1}." + ".".join(parts[3:])
        elif parts[1] == "mid":
            name = {"norm": "group_norm", "q": "to_q", "k": "to_k", "v": "to_v", "proj_out": "to_out.0"}[parts[3]]
            k2 = f"{parts[0]}.mid_block.attentions.0.{name}.{parts[4]}"
            if parts[4] == "weight" and v.dim() == 4:
                v = v.reshape(v.shape[0], v.shape[1])   # diffusers' Attention uses Linear layers
        elif parts[1] == "norm_out":
            k2 = f"{parts[0]}.conv_norm_out.{parts[2]}"
        else:
            k2 = k
        out[k2] = v
    return out


def test_vae_keys_from_diffusers_round_trip():
    from forge_amd.backend.misc.diffusers_state_dict import vae_from_diffusers
    for cfg in (synth.TINY_VAE_CONFIG, synth.TINY_FLUX_VAE_CONFIG):
        ldm = synth.synth_vae_state_dict(cfg, seed=1)
        dif = _vae_ldm_to_diffusers_names(ldm, len(cfg["block_out_channels"]))
        assert "decoder.up_blocks.0.resnets.0.norm1.weight" in dif and "encoder.mid_block.attentions.0.to_q.weight" in dif   # loader.py:58 marker
        assert dif["decoder.mid_block.attentions.0.to_out.0.weight"].dim() == 2 and not any(".up." in k or ".down." in k for k in dif)
        back = vae_from_diffusers(dif)
        assert set(back) == set(ldm)
        for k in ldm:
            assert back[k].shape == ldm[k].shape and torch.equal(back[k], ldm[k]), k
        assert vae_from_diffusers(ldm) is ldm   # already LDM-keyed: untouched


def test_flux_checkpoint_detection_and_split():
    """loader: Flux transformer recognised by its marker key (with and without the checkpoint prefix), configuration read off the tensors,
    VAE found under 'vae.' (diffusers names converted), compute type following the stored tensors."""
    cfg = synth.TINY_FLUX_CONFIG
    tr = {k: v.to(torch.bfloat16) for k, v in synth.synth_flux_state_dict(cfg, seed=2).items()}
    vae = synth.synth_vae_state_dict(synth.TINY_FLUX_VAE_CONFIG, seed=1)
    ck = {"model.diffusion_model." + k: v for k, v in tr.items()}
    ck.update({"vae." + k: v for k, v in _vae_ldm_to_diffusers_names(vae, len(synth.TINY_FLUX_VAE_CONFIG["block_out_channels"])).items()})
    ck["text_encoders.clip_l.transformer.text_model.embeddings.position_embedding.weight"] = torch.zeros(77, 8)
    assert loader.flux_prefix(ck) == "model.diffusion_model." and loader.flux_prefix(tr) == "" and loader.flux_prefix(vae) is None
    parts, guess = loader.split_flux_state_dict(ck)
    assert guess["flux_config"] == cfg and guess["dtype"] == torch.bfloat16 and guess["ignored"] == ["text_encoders"]
    assert set(parts["transformer"]) == set(tr) and set(parts["vae"]) == set(vae)
    assert guess["vae_config"] == {**synth.TINY_FLUX_VAE_CONFIG, "block_out_channels": tuple(synth.TINY_FLUX_VAE_CONFIG["block_out_channels"])}
    full = loader.detect_vae_config({k: torch.empty(s, device="meta") for k, s in {**vae_decoder_param_shapes(synth.FLUX_VAE_CONFIG),
                                                                                  **vae_encoder_param_shapes(synth.FLUX_VAE_CONFIG)}.items()},
                                    scaling_factor=0.3611, shift_factor=0.1159)
    assert full == synth.FLUX_VAE_CONFIG
    parts2, guess2 = loader.split_flux_state_dict({k: v.half() for k, v in tr.items()})     # transformer-only file, fp16
    assert guess2["flux_config"] == cfg and guess2["dtype"] == torch.float16 and not parts2["vae"] and guess2["vae_config"] is None
    schnell = {k: v for k, v in tr.items() if not k.startswith("guidance_in.")}
    assert loader.detect_flux_config(schnell, "")["guidance_embed"] is False
    with pytest.raises(NotImplementedError):
        loader.split_flux_state_dict({k: v.to(torch.float8_e4m3fn) for k, v in tr.items()})


def test_flux_and_vae_detection_agree_with_the_configuration_files_the_reference_ships():
    """The reference builds Flux from backend/huggingface/black-forest-labs/FLUX.1-{dev,schnell}/{transformer,vae}/config.json (diffusers field
    names); what the loader reads off a full-size state dict must describe the same networks."""
    import json
    import os
    from forge_amd.backend.nn.layout import flux_param_shapes
    root = os.path.join(HF_CONFIGS, "black-forest-labs")
    for repo, guidance in (("FLUX.1-dev", True), ("FLUX.1-schnell", False)):
        want = json.load(open(os.path.join(root, repo, "transformer", "config.json")))
        cfg = dict(synth.FLUX_DEV_CONFIG, guidance_embed=guidance)
        sd = {k: torch.empty(s, device="meta") for k, s in flux_param_shapes(cfg).items()}
        got = loader.detect_flux_config(sd, "")
        assert got == cfg
        assert (got["hidden_size"] // got["num_heads"], got["num_heads"], got["depth"], got["depth_single_blocks"]) == (
            want["attention_head_dim"], want["num_attention_heads"], want["num_layers"], want["num_single_layers"])
        assert (got["in_channels"] * 4, got["context_in_dim"], got["vec_in_dim"], got["guidance_embed"]) == (
            want["in_channels"], want["joint_attention_dim"], want["pooled_projection_dim"], want["guidance_embeds"])
        vwant = json.load(open(os.path.join(root, repo, "vae", "config.json")))
        vshapes = {**vae_decoder_param_shapes(synth.FLUX_VAE_CONFIG), **vae_encoder_param_shapes(synth.FLUX_VAE_CONFIG)}
        vgot = loader.detect_vae_config({k: torch.empty(s, device="meta") for k, s in vshapes.items()}, scaling_factor=0.3611, shift_factor=0.1159)
        for k in ("block_out_channels", "layers_per_block", "latent_channels", "in_channels", "out_channels", "scaling_factor", "shift_factor",
                  "use_quant_conv", "use_post_quant_conv"):
            assert (tuple(vgot[k]) if k == "block_out_channels" else vgot[k]) == (tuple(vwant[k]) if k == "block_out_channels" else vwant[k]), k


@pytest.mark.parametrize("repo,base,override", [
    ("runwayml/stable-diffusion-v1-5", "SD15_UNET_CONFIG", {}),
    ("runwayml/stable-diffusion-inpainting", "SD15_UNET_CONFIG", {"in_channels": 9}),
    ("stabilityai/stable-diffusion-xl-base-1.0", "SDXL_UNET_CONFIG", {}),
])
def test_unet_detection_agrees_with_the_configuration_files_the_reference_ships(repo, base, override):
    """detect_unet_config on a full-size (meta) state dict vs backend/huggingface/<repo>/unet/config.json (diffusers field names: widths per
    level, ResBlocks per level, transformer depth per level, heads, context / label widths, linear vs conv projections)."""
    import json
    import os
    want = json.load(open(os.path.join(HF_CONFIGS, repo, "unet", "config.json")))
    cfg = dict(getattr(synth, base), **override)
    got = loader.detect_unet_config(_meta_sd(unet_param_shapes(cfg), loader.UNET_PREFIX))
    mc = got["model_channels"]
    widths = [mc * m for m in got["channel_mult"]]
    assert widths == want["block_out_channels"] and got["in_channels"] == want["in_channels"] and got["out_channels"] == want["out_channels"]
    nres = got["num_res_blocks"]
    assert set(nres) == {want["layers_per_block"]} and len(nres) == len(widths)
    assert got["context_dim"] == want["cross_attention_dim"] and got["use_linear_in_transformer"] == bool(want.get("use_linear_projection", False))
    assert got.get("adm_in_channels") == want.get("projection_class_embeddings_input_dim")
    # transformer depth of each level's first ResBlock position (0 where the diffusers block type has no cross-attention)
    depth_per_level = [got["transformer_depth"][sum(nres[:i])] for i in range(len(widths))]
    tl = want.get("transformer_layers_per_block", 1)
    tl = tl if isinstance(tl, list) else [tl] * len(widths)
    want_depth = [tl[i] if "CrossAttn" in t else 0 for i, t in enumerate(want["down_block_types"])]
    assert depth_per_level == want_depth
    # heads: diffusers' (misnamed) attention_head_dim holds the head COUNT per level
    heads = want["attention_head_dim"]
    heads = heads if isinstance(heads, list) else [heads] * len(widths)
    if "num_heads" in got:
        assert all(h == got["num_heads"] for h in heads)
    else:
        assert [w // got["num_head_channels"] for w in widths] == heads


def _ldm_config_from_diffusers(want):
    """Test-side mapping diffusers UNet2DConditionModel config -> the LDM constructor arguments (what huggingface_guess's model list encodes)."""
    widths, lpb = want["block_out_channels"], want["layers_per_block"]
    mc, n = widths[0], len(widths)
    tl = want.get("transformer_layers_per_block") or 1
    tl = tl if isinstance(tl, list) else [tl] * n
    per_level = [tl[i] if "CrossAttn" in t else 0 for i, t in enumerate(want["down_block_types"])]
    cfg = dict(in_channels=want["in_channels"], model_channels=mc, out_channels=want["out_channels"], num_res_blocks=[lpb] * n,
               channel_mult=tuple(w // mc for w in widths), use_spatial_transformer=True,
               transformer_depth=[d for d in per_level for _ in range(lpb)], transformer_depth_middle=tl[-1],
               transformer_depth_output=[d for d in per_level for _ in range(lpb + 1)], context_dim=want["cross_attention_dim"],
               use_linear_in_transformer=bool(want.get("use_linear_projection", False)), num_head_channels=64)
    if want.get("projection_class_embeddings_input_dim"):
        cfg.update(adm_in_channels=want["projection_class_embeddings_input_dim"], num_classes="sequential")
    return cfg


@pytest.mark.parametrize("repo", ["stabilityai/stable-diffusion-2-1", "stabilityai/stable-diffusion-xl-refiner-1.0", "stabilityai/stable-diffusion-xl-base-1.0"])
def test_unet_detection_round_trips_the_sd2_and_refiner_structures(repo):
    """SD2.1 (context 1024, linear projections, 64 channels per head, last level without attention) and the SDXL refiner (384-wide, four levels,
    attention only in the two middle ones, 2560-wide label input): shipped config -> LDM arguments -> parameter shapes -> detection."""
    import json
    import os
    want = json.load(open(os.path.join(HF_CONFIGS, repo, "unet", "config.json")))
    cfg = _ldm_config_from_diffusers(want)
    got = loader.detect_unet_config(_meta_sd(unet_param_shapes(cfg), loader.UNET_PREFIX))
    for k, v in cfg.items():
        assert got[k] == v, (k, got[k], v)
    assert [w // got["num_head_channels"] for w in want["block_out_channels"]] == want["attention_head_dim"]
    if "xl-base" in repo:
        assert {k: got[k] for k in synth.SDXL_UNET_CONFIG} == synth.SDXL_UNET_CONFIG


def test_family_constants_match_the_shipped_scheduler_and_vae_configs():
    """The constants no tensor carries -- noise schedule, VAE scaling / shift factors, the Flux time-shift parameters -- against the scheduler and
    VAE configuration files under backend/huggingface/."""
    import inspect
    import json
    import os
    from forge_amd.backend.modules.k_prediction import PredictionFlux
    hub = HF_CONFIGS
    load = lambda *p: json.load(open(os.path.join(hub, *p)))  # noqa: E731
    for repo in ("runwayml/stable-diffusion-v1-5", "stabilityai/stable-diffusion-xl-base-1.0"):
        sch = load(repo, "scheduler", "scheduler_config.json")
        # diffusers' "scaled_linear" is the LDM "linear" schedule (linspace of sqrt(beta)), k_prediction.py:20-25
        assert sch["beta_schedule"] == "scaled_linear" and synth.SCHEDULE["beta_schedule"] == "linear"
        assert (sch["beta_start"], sch["beta_end"], sch["num_train_timesteps"]) == (synth.SCHEDULE["linear_start"], synth.SCHEDULE["linear_end"],
                                                                                     synth.SCHEDULE["timesteps"])
    # the SD1.5 file predates the field: AutoencoderKL's default 0.18215 applies (backend/nn/vae.py:278)
    assert load("runwayml/stable-diffusion-v1-5", "vae", "config.json").get("scaling_factor", 0.18215) == synth.SD15_VAE_CONFIG["scaling_factor"] == 0.18215
    assert load("stabilityai/stable-diffusion-xl-base-1.0", "vae", "config.json")["scaling_factor"] == synth.SDXL_VAE_CONFIG["scaling_factor"]
    fl = load("black-forest-labs/FLUX.1-dev", "scheduler", "scheduler_config.json")
    d = {k: v.default for k, v in inspect.signature(PredictionFlux.__init__).parameters.items() if v.default is not inspect.Parameter.empty}
    assert (d["base_seq_len"], d["max_seq_len"], d["base_shift"], d["max_shift"]) == (fl["base_image_seq_len"], fl["max_image_seq_len"],
                                                                                      fl["base_shift"], fl["max_shift"])
    assert abs(PredictionFlux().mu - fl["max_shift"]) < 1e-12      # the engine's constant 4096-token image sits at the top of the shift range


def _norm_target(v):
    return v if isinstance(v, str) else (v[0], v[1], v[2].__name__ if len(v) > 2 else None)


def test_flux_lora_key_map_matches_reference_fixture():
    """Flux LoRA key map (VERDICT r4 missing 3): native, diffusers ('transformer.'), simpletuner LyCORIS ('lycoris_') and OneTrainer ('lora_transformer_')
    spellings, with the slice targets (q | k | v of a fused qkv; q | k | v | mlp of linear1) and the swap_scale_shift function target, against the map the
    reference builds (tests/golden/tiny_flux_lora_merge.pt, oracle/make_golden.py gen_flux_lora); the patch parser finds every entry of the synthetic LoRA."""
    from forge_amd.backend.nn.layout import flux_param_shapes
    from oracle.make_golden import synth_flux_lora
    g = load_golden("tiny_flux_lora_merge.pt")
    cfg = synth.TINY_FLUX_CONFIG
    km = nlora.model_lora_keys_flux(list(flux_param_shapes(cfg)), cfg)
    assert {k: _norm_target(v) for k, v in km.items()} == g["key_map_targets"]
    patch_dict, remaining = nlora.load_lora(synth_flux_lora(cfg), km)
    assert sorted(remaining) == g["remaining"] == []
    touched = {(t if isinstance(t, str) else t[0])[len("diffusion_model."):] for t in patch_dict}
    assert touched == set(g["merged"])


def test_flux_to_diffusers_vs_reference():
    """flux_to_diffusers against the reference's (function targets compared through their output on the fixture's test input)."""
    from forge_amd.backend.misc.diffusers_state_dict import flux_to_diffusers
    from oracle.make_ref_fixtures import TEST_INPUT, flux_target_record
    ref = _ref_key_maps()["flux_to_diffusers"]
    for name, cfg in (("tiny_flux", synth.TINY_FLUX_CONFIG), ("flux_dev", synth.FLUX_DEV_CONFIG)):
        ours, theirs = flux_to_diffusers(cfg, output_prefix="diffusion_model."), ref[name]
        assert set(ours) == set(theirs)
        for k in ours:
            a, b = ours[k], theirs[k]
            if isinstance(b, list) and len(b) > 2:
                assert a[0] == b[0] and a[1] is None and torch.equal(a[2](TEST_INPUT), torch.tensor(b[2], dtype=TEST_INPUT.dtype))
            else:
                assert flux_target_record(a) == b, k


def test_bias_diff_on_a_slice_target_is_reported_not_raised():
    """a diffusers-named Flux LoRA carrying `.diff_b` on to_q / proj_mlp (slice targets `(key, offset)`): the reference's
    `to_load[x][:-len(".weight")]` on the tuple yields a key no parameter has (lora.py:199-203), i.e. the bias diff patches nothing; the native parser must
    not raise (tuple + str) and reports the entry as unused."""
    import torch
    from forge_amd import synth
    from forge_amd.backend.patcher import lora as nlora
    from forge_amd.backend.nn.layout import flux_param_shapes
    cfg = synth.TINY_FLUX_CONFIG
    km = nlora.model_lora_keys_flux(list(flux_param_shapes(cfg)), cfg)
    hs = cfg["hidden_size"]
    x = "transformer.transformer_blocks.0.attn.to_q"
    assert isinstance(km[x], tuple)
    lo = {x + ".lora_up.weight": torch.randn(hs, 4), x + ".lora_down.weight": torch.randn(4, hs), x + ".diff_b": torch.randn(hs),
          "transformer.norm_out.linear.w_norm": torch.randn(2 * hs, hs), "transformer.norm_out.linear.b_norm": torch.randn(2 * hs)}
    patch, remaining = nlora.load_lora(lo, km)
    assert km[x] in patch and all(isinstance(k, (str, tuple)) for k in patch)
    assert x + ".diff_b" in remaining
    # a plain (string) target keeps its bias diff
    y = "lora_unet_img_in"
    patch2, rem2 = nlora.load_lora({y + ".diff": torch.randn(*flux_param_shapes(cfg)["img_in.weight"]), y + ".diff_b": torch.randn(hs)}, km)
    assert "diffusion_model.img_in.bias" in patch2 and not rem2
