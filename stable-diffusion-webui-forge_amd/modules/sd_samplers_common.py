"""Mirror of modules/sd_samplers_common.py for the path: `SamplerData` (:13-31), `InterruptedException` (:186),
`TorchHijack` (:214-235), `Sampler` base (:238-364: callback_state, launch_sampling, initialize), and the latent -> picture helpers behind
live previews and the VAE decode method (:36-93, :123-128)."""
import inspect
from collections import namedtuple

import numpy as np
import torch

from . import shared
from .. import k_diffusion  # noqa: F401
from ..k_diffusion import sampling as kd_sampling


class SamplerData(namedtuple("SamplerData", ["name", "constructor", "aliases", "options"])):
    def total_steps(self, steps):
        if self.options.get("second_order", False):
            steps = steps * 2
        return steps


class InterruptedException(BaseException):
    pass


def setup_img2img_steps(p, steps=None):
    """sd_samplers_common.py:24-33."""
    if getattr(shared.opts, "img2img_fix_steps", False) or steps is not None:
        requested_steps = (steps or p.steps)
        steps = int(requested_steps / min(p.denoising_strength, 0.999)) if p.denoising_strength > 0 else 0
        t_enc = requested_steps - 1
    else:
        steps = p.steps
        t_enc = int(min(p.denoising_strength, 0.999) * steps)
    return steps, t_enc


approximation_indexes = {"Full": 0, "Approx NN": 1, "Approx cheap": 2, "TAESD": 3}   # sd_samplers_common.py:36


def samples_to_images_tensor(sample, approximation=None, model=None):
    """sd_samplers_common.py:39-67: latents [B, L, h, w] -> RGB image tensors [B, 3, H, W] in about [-1, 1].  approximation None: the live-preview
    method (opts.show_progress_type; "Full" there means "Approx NN").  "Approx NN" (sd_vae_approx.VAEApprox) is not built and falls back to the
    cheap approximation, as the reference does when `sd_vae_approx.model()` returns None; `live_preview_fast_interrupt` is not mirrored."""
    from . import sd_vae_approx, sd_vae_taesd
    if approximation is None:
        approximation = approximation_indexes.get(shared.opts.show_progress_type, 0)
        if approximation == 0:
            approximation = 1
    if approximation in (1, 2):
        return sd_vae_approx.cheap_approximation(sample)
    if approximation == 3:
        # TAESD takes the RAW latent (no process_out) and returns about [0, 1] (:56-61)
        return sd_vae_taesd.decoder_model().decode(sample) * 2 - 1
    if model is None:
        model = shared.sd_model
    return model.decode_first_stage(sample)


def single_sample_to_image(sample, approximation=None):
    """sd_samplers_common.py:70-80: one latent [L, h, w] -> PIL.Image"""
    from PIL import Image
    x_sample = samples_to_images_tensor(sample.unsqueeze(0), approximation)[0] * 0.5 + 0.5
    x_sample = x_sample.float().cpu()
    x_sample.clamp_(0.0, 1.0)
    x_sample.mul_(255.)
    x_sample.round_()
    x_sample = x_sample.to(torch.uint8)
    x_sample = np.moveaxis(x_sample.numpy(), 0, 2)
    return Image.fromarray(x_sample)


def decode_first_stage(model, x):
    """sd_samplers_common.py:83-85: the decode of final images by opts.sd_vae_decode_method"""
    approx_index = approximation_indexes.get(shared.opts.sd_vae_decode_method, 0)
    return samples_to_images_tensor(x, approx_index, model)


def sample_to_image(samples, index=0, approximation=None):
    return single_sample_to_image(samples[index], approximation)      # :88-89


def preview_due():
    """the period rule of store_latent (:126): previews on, a positive period, and the sampling step a multiple of it.  Reads three attributes: with
    previews off nothing is launched and nothing synchronises"""
    opts = shared.opts
    return bool(opts.live_previews_enable) and opts.show_progress_every_n_steps > 0 and shared.state.sampling_step % opts.show_progress_every_n_steps == 0


def store_latent(decoded):
    """sd_samplers_common.py:123-128.  The preview is made right here, on the caller's stream and outside any captured graph: `decoded` may live in a
    graph's memory pool that the next replay overwrites."""
    shared.state.current_latent = decoded
    if preview_due():
        if not shared.parallel_processing_allowed:
            shared.state.assign_current_image(sample_to_image(decoded))


def images_tensor_to_samples(image, approximation=None, model=None):
    """sd_samplers_common.py:96-120 ("Full" VAE encode only; the TAESD encoder is not built): image [B,3,H,W] in [0, 1] -> latent, one image at a
    time as the reference does (each draws its own posterior noise from the CPU default generator, nn/vae.py:28)."""
    if approximation is None:
        approximation = approximation_indexes.get(getattr(shared.opts, "sd_vae_encode_method", "Full"), 0)
    if approximation == 3:
        raise NotImplementedError('sd_vae_encode_method = "TAESD": the TAESD encoder (modules/sd_vae_taesd.py:47-54, :134-158) is not built; use "Full"')
    model = model if model is not None else shared.sd_model
    image = image.to(model.device, dtype=torch.float32) * 2 - 1
    if len(image) > 1:
        return torch.stack([model.encode_first_stage(torch.unsqueeze(img, 0))[0] for img in image])
    return model.encode_first_stage(image)


class TorchHijack:
    """Replaces `torch` inside k_diffusion.sampling so that randn_like draws from the per-image generators (p.rng):
    images generated in a batch equal images generated individually (and independent of multi-GPU sharding)."""

    def __init__(self, p):
        self.rng = p.rng

    def __getattr__(self, item):
        if item == "randn_like":
            return self.randn_like
        if hasattr(torch, item):
            return getattr(torch, item)
        raise AttributeError(f"'{type(self).__name__}' object has no attribute '{item}'")

    def randn_like(self, x):
        return self.rng.next()


class Sampler:
    def __init__(self, funcname):
        self.funcname = funcname
        self.func = funcname
        self.extra_params = []
        self.stop_at = None
        self.eta = None
        self.config = None
        self.last_latent = None
        self.s_min_uncond = None
        self.s_churn, self.s_tmin, self.s_tmax, self.s_noise = 0.0, 0.0, float("inf"), 1.0
        self.eta_option_field = "eta_ancestral"
        self.eta_default = 1.0
        self.p = None
        self.model_wrap_cfg = None
        self.sampler_extra_args = None
        self.options = {}

    def callback_state(self, d):
        step = d["i"]
        if self.stop_at is not None and step > self.stop_at:
            raise InterruptedException
        shared.state.sampling_step = step

    def launch_sampling(self, steps, func):
        self.model_wrap_cfg.steps = steps
        self.model_wrap_cfg.total_steps = self.config.total_steps(steps)
        shared.state.sampling_steps = steps
        shared.state.sampling_step = 0
        try:
            return func()
        except RecursionError:
            return self.last_latent
        except InterruptedException:
            return self.last_latent

    def create_noise_sampler(self, x, sigmas, p):
        """sd_samplers_common.py:343-351: one Brownian path per image, seeded by the image's seed, so results do not depend on batch size."""
        if getattr(shared.opts, "no_dpmpp_sde_batch_determinism", False):
            return None
        sigma_min, sigma_max = sigmas[sigmas > 0].min(), sigmas.max()
        it = getattr(p, "iteration", 0)
        current_iter_seeds = p.all_seeds[it * p.batch_size:(it + 1) * p.batch_size]
        return kd_sampling.BrownianTreeNoiseSampler(x, sigma_min, sigma_max, seed=current_iter_seeds)

    def initialize(self, p):
        self.p = p
        self.model_wrap_cfg.p = p
        self.model_wrap_cfg.mask = getattr(p, "mask", None)
        self.model_wrap_cfg.nmask = getattr(p, "nmask", None)
        self.model_wrap_cfg.mask_noise_source = getattr(p, "mask_noise_source", None)
        self.model_wrap_cfg.step = 0
        self.eta = p.eta if getattr(p, "eta", None) is not None else getattr(shared.opts, self.eta_option_field, 0.0)
        self.s_min_uncond = getattr(p, "s_min_uncond", 0.0)
        kd_sampling.torch = TorchHijack(p)
        extra = {}
        params = inspect.signature(self.func).parameters
        for name in self.extra_params:
            if hasattr(p, name) and name in params:
                extra[name] = getattr(p, name)
        if "eta" in params:
            extra["eta"] = self.eta
        return extra
