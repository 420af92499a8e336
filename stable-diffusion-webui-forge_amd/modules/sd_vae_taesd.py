"""Mirror of modules/sd_vae_taesd.py:107-131 (`decoder_model`): which Tiny AutoEncoder serves the loaded engine, loaded once per file name from
<shared.models_path>/VAE-taesd and run by the native executor forge_amd.backend.nn.taesd.TAESDDecoder.

Unlike the reference (:99-104, :121) nothing is ever downloaded: a missing file is a FileNotFoundError that names the path.  `.pth` files are read with
torch.load(weights_only=True); a `.safetensors` file of the same stem is accepted too.  The encoder half (:134-158) is not built."""
import os

import torch

from . import shared

sd_vae_taesd_models = {}


def decoder_model_name(sd_model):
    """sd_vae_taesd.py:108-115: SD3 -> taesd3, any other non-legacy engine (Flux) -> taef1, SDXL -> taesdxl, else taesd"""
    if getattr(sd_model, "is_sd3", False):
        return "taesd3_decoder.pth"
    legacy = sd_model.is_webui_legacy_model() if hasattr(sd_model, "is_webui_legacy_model") else not getattr(sd_model, "is_flux", False)
    if not legacy:
        return "taef1_decoder.pth"
    if getattr(sd_model, "is_sdxl", False):
        return "taesdxl_decoder.pth"
    return "taesd_decoder.pth"


def _element_type(sd_model):
    """the reference runs TAESD in devices.dtype; here: bfloat16 beside a bfloat16 VAE executor, float16 otherwise"""
    vae = getattr(getattr(sd_model, "forge_objects", None), "vae", None)
    dt = getattr(getattr(vae, "first_stage_model", None), "dtype", None)
    return torch.bfloat16 if dt == torch.bfloat16 else torch.float16


def load_state_dict(path):
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path)
    return torch.load(path, map_location="cpu", weights_only=True)


def decoder_model():
    """-> TAESDDecoder for shared.sd_model (cached per file name)"""
    from ..backend.nn.taesd import TAESDDecoder
    sd_model = shared.sd_model
    if sd_model is None:
        raise RuntimeError("TAESD: no engine loaded (shared.sd_model is None)")
    model_name = decoder_model_name(sd_model)
    loaded_model = sd_vae_taesd_models.get(model_name)
    if loaded_model is None:
        model_path = os.path.join(shared.models_path, "VAE-taesd", model_name)
        if not os.path.exists(model_path):
            alt = model_path[:-len(".pth")] + ".safetensors"
            if not os.path.exists(alt):
                raise FileNotFoundError(f"TAESD model not found: {os.path.abspath(model_path)} (nothing is downloaded: put the file there, or set "
                                        f"forge_amd.modules.shared.models_path)")
            model_path = alt
        loaded_model = TAESDDecoder(load_state_dict(model_path), device=getattr(sd_model, "device", None) or "cuda", dtype=_element_type(sd_model))
        sd_vae_taesd_models[model_name] = loaded_model
    return loaded_model


def encoder_model():
    raise NotImplementedError('the TAESD encoder (modules/sd_vae_taesd.py:134-158, sd_vae_encode_method = "TAESD") is not built; use "Full"')
