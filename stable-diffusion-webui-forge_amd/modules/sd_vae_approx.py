"""Mirror of modules/sd_vae_approx.py:73-74 (`cheap_approximation`): a latent -> RGB linear map with the engine's `latent_rgb_factors`.
"Approx NN" (VAEApprox, :10-70: 7x7 / 5x5 convolutions on 8 to 32 channels) is not built; `model()` returns None, and callers fall back to the
cheap approximation exactly as the reference does when its `model()` returns None (modules/sd_samplers_common.py:50-52)."""
import torch

from . import shared
from .. import hipops as ops


def model():
    return None


def latent_rgb_factors(sd_model):
    """the [L][3] table of the engine's latent format (reference: shared.sd_model.model_config.latent_format.latent_rgb_factors, tables that live in
    huggingface_guess); also read from an attribute `latent_rgb_factors` of the engine itself.  None of them are shipped here."""
    fmt = getattr(getattr(sd_model, "model_config", None), "latent_format", None)
    fac = getattr(fmt, "latent_rgb_factors", None)
    return fac if fac is not None else getattr(sd_model, "latent_rgb_factors", None)


def cheap_approximation(sample):
    fac = latent_rgb_factors(shared.sd_model)
    if fac is None:
        raise NotImplementedError('"Approx cheap" / "Approx NN" previews need the engine\'s latent_rgb_factors ([latent channels][3]; set '
                                  '`engine.latent_rgb_factors`), which this engine does not carry; use show_progress_type = "TAESD"')
    lead = sample.shape[:-3]
    z = sample.reshape(-1, *sample.shape[-3:]).to(torch.float32).contiguous()
    return ops.latent_rgb(z, fac).reshape(*lead, 3, *sample.shape[-2:])
