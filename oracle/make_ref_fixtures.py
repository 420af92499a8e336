"""TEST INFRASTRUCTURE ONLY.  Records what the CPU tests used to read from the real reference at run time, so that they run on a clean checkout
anywhere (authoring container only, like oracle/make_golden.py):

    python -m oracle.make_ref_fixtures

writes under tests/golden/:
  hf_configs/<repo>/<part>/<file>.json   the diffusers configuration files the reference ships under backend/huggingface/ (settings only),
                                         for the model-family detection tests of tests/test_loader_lora.py
  ref_lora_key_maps.json.gz              the reference's unet_to_diffusers / model_lora_keys_unet for the SD1.5, SDXL and tiny SDXL UNets, and
                                         flux_to_diffusers for the tiny and full-size Flux configurations (function targets recorded as their
                                         output on TEST_INPUT)
  ref_masking_fill.pt                    modules/masking.py fill() on the PIL images of tests/test_masking_fill.py::_case
  ref_prompt_attention_random.json.gz    parse_prompt_attention of backend/text_processing/parsing.py on the random strings of
                                         tests/test_text_processing.py::random_prompts, in both modes
  ref_tiny_sd15_unet_fwd_fp16.pt         the reference UNet in its own fp16 mode (oracle/make_floor.py half_unet) on the input of
                                         tiny_sd15_unet_fwd.pt: the run the committed floor `tiny_sd15_unet_fwd.pt:eps` was measured on
"""
import gzip
import importlib
import importlib.util
import json
import os
import shutil
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import forge_amd  # noqa: E402,F401
from forge_amd import synth  # noqa: E402
from forge_amd.backend.nn.layout import unet_param_shapes  # noqa: E402
from oracle import ref_import  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
HF_CONFIGS = [
    "runwayml/stable-diffusion-v1-5/unet/config.json", "runwayml/stable-diffusion-v1-5/vae/config.json",
    "runwayml/stable-diffusion-v1-5/scheduler/scheduler_config.json",
    "runwayml/stable-diffusion-inpainting/unet/config.json",
    "stabilityai/stable-diffusion-xl-base-1.0/unet/config.json", "stabilityai/stable-diffusion-xl-base-1.0/vae/config.json",
    "stabilityai/stable-diffusion-xl-base-1.0/scheduler/scheduler_config.json",
    "stabilityai/stable-diffusion-2-1/unet/config.json",
    "stabilityai/stable-diffusion-xl-refiner-1.0/unet/config.json",
    "black-forest-labs/FLUX.1-dev/transformer/config.json", "black-forest-labs/FLUX.1-dev/vae/config.json",
    "black-forest-labs/FLUX.1-dev/scheduler/scheduler_config.json",
    "black-forest-labs/FLUX.1-schnell/transformer/config.json", "black-forest-labs/FLUX.1-schnell/vae/config.json",
]
UNET_KEY_MAP_CONFIGS = {"sd15": synth.SD15_UNET_CONFIG, "sdxl": synth.SDXL_UNET_CONFIG, "tiny_sdxl": synth.TINY_SDXL_UNET_CONFIG}
FLUX_KEY_MAP_CONFIGS = {"tiny_flux": synth.TINY_FLUX_CONFIG, "flux_dev": synth.FLUX_DEV_CONFIG}
TEST_INPUT = torch.arange(12.0).reshape(6, 2)     # what a function target of flux_to_diffusers is applied to


def flux_target_record(v):
    """str -> str; (key, slice) -> [key, slice]; (key, None, fn) -> [key, None, fn(TEST_INPUT)]"""
    if isinstance(v, str):
        return v
    if len(v) > 2:
        return [v[0], None, v[2](TEST_INPUT).tolist()]
    return [v[0], list(v[1]) if v[1] is not None else None]


def gen_hf_configs():
    hub = os.path.join(ref_import.REFERENCE_ROOT, "backend", "huggingface")
    for rel in HF_CONFIGS:
        dst = os.path.join(GOLD, "hf_configs", rel)
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        shutil.copyfile(os.path.join(hub, rel), dst)


def gen_key_maps():
    ref_import.load_reference()
    rl = importlib.import_module("backend.patcher.lora")
    cu = importlib.import_module("packages_3rdparty.comfyui_lora_collection.utils")
    out = {"unet": {}, "flux_to_diffusers": {}}
    for name, cfg in UNET_KEY_MAP_CONFIGS.items():
        rcfg = {k: (list(v) if isinstance(v, (list, tuple)) else v) for k, v in cfg.items()}
        keys = {"diffusion_model." + k: None for k in unet_param_shapes(cfg)}
        model = SimpleNamespace(state_dict=lambda: keys, diffusion_model=SimpleNamespace(config=rcfg), config=SimpleNamespace(huggingface_repo="sd"))
        out["unet"][name] = {"unet_to_diffusers": cu.unet_to_diffusers(dict(rcfg)), "model_lora_keys_unet": rl.model_lora_keys_unet(model, {})}
    for name, cfg in FLUX_KEY_MAP_CONFIGS.items():
        m = cu.flux_to_diffusers(dict(cfg), output_prefix="diffusion_model.")
        out["flux_to_diffusers"][name] = {k: flux_target_record(v) for k, v in m.items()}
    with gzip.open(os.path.join(GOLD, "ref_lora_key_maps.json.gz"), "wt") as f:
        json.dump(out, f, sort_keys=True)


def gen_masking_fill():
    from test_masking_fill import _case, _pil
    spec = importlib.util.spec_from_file_location("ref_masking", os.path.join(ref_import.REFERENCE_ROOT, "modules", "masking.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    img, mask = _case()
    outs = [torch.from_numpy(np.array(mod.fill(*_pil(img[i], mask)))) for i in range(img.shape[0])]
    torch.save({"filled_pil_u8": torch.stack(outs), "note": "modules/masking.py fill() on the PIL images of tests/test_masking_fill.py::_case, [B, H, W, 3]"},
               os.path.join(GOLD, "ref_masking_fill.pt"))


def gen_prompt_attention():
    from test_text_processing import random_prompts
    spec = importlib.util.spec_from_file_location("_ref_parsing", os.path.join(ref_import.REFERENCE_ROOT, "backend", "text_processing", "parsing.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    rows = [[s, mode, ref.parse_prompt_attention(s, mode)] for s in random_prompts() for mode in ("Original", "None")]
    with gzip.open(os.path.join(GOLD, "ref_prompt_attention_random.json.gz"), "wt") as f:
        json.dump(rows, f)


def gen_floor_fp16():
    from oracle.make_floor import half_unet
    g = torch.load(os.path.join(GOLD, "tiny_sd15_unet_fwd.pt"), map_location="cpu", weights_only=False)
    with torch.no_grad():
        eps16 = half_unet(synth.TINY_SD15_UNET_CONFIG)(g["x"], g["t"], context=g["ctx"], y=None, transformer_options={})
    torch.save({"eps": eps16.float(), "note": "reference UNet in fp16 (oracle/make_floor.py half_unet) on tiny_sd15_unet_fwd.pt's x / t / ctx"},
               os.path.join(GOLD, "ref_tiny_sd15_unet_fwd_fp16.pt"))


def main():
    if not ref_import.reference_available():
        raise SystemExit(f"reference not present at {ref_import.REFERENCE_ROOT}")
    gen_hf_configs()
    gen_key_maps()
    gen_masking_fill()
    gen_prompt_attention()
    gen_floor_fp16()
    print("wrote tests/golden/hf_configs/, ref_lora_key_maps.json.gz, ref_masking_fill.pt, ref_prompt_attention_random.json.gz, "
          "ref_tiny_sd15_unet_fwd_fp16.pt")


if __name__ == "__main__":
    main()
