"""Native Perturbed-Attention Guidance -- the patcher-level entry (reference: extensions-builtin/sd_forge_perturbed_attention/scripts/
forge_perturbed_attention.py, "PerturbedAttentionGuidance Integrated").

The reference installs a Python post-CFG function that runs the conditional batch a second time with the middle block's self-attention replaced
by `lambda q, k, v, to: v` and adds (cond_denoised - degraded) * scale to the CFG result.  Here the parameters travel as the model option "pag":
on a step inside the window KModel.denoise_cfg stacks [uncond ; cond ; cond] into ONE UNet forward (backend/nn/unet.py `pag_from`, hipops.
attn_value_rows) and the term joins the CFG combination (hipops.cfg_pag_combine) -- no Python hook, so the step stays on the captured graph, and
no second model call.  The scale is an argument of the combine launch, outside the graph: attenuation never re-captures.

What the reference keeps in class globals (scale, PAG_start / PAG_end, doPAG, evaluated by its on_cfg_denoiser callback) is the option's
parameters and one mutable number, the current scale: reset at sampling_prepare (the reference: process_before_every_sampling, so a hires second
pass starts at the full scale again), lowered after every application."""
from collections import namedtuple

PagParams = namedtuple("PagParams", ["scale", "attenuation", "start_step", "end_step"], defaults=(3.0, 0.0, 0.0, 1.0))

OPTION = "pag"
FEATURE = "Perturbed-Attention Guidance"


class PagOption:
    """model_options["pag"]: the job's parameters and the current (attenuated) scale.  Clones of the patcher that carries it share it, as they
    share every leaf of model_options: it is the state of one job."""
    __slots__ = ("params", "scale")

    def __init__(self, params):
        self.params = params
        self.scale = params.scale

    def reset(self):
        self.scale = self.params.scale

    def applied(self):
        """after every application (model call, so twice a step under a two-evaluation sampler): forge_perturbed_attention.py:81, repeated
        subtraction in Python floats"""
        self.scale -= self.params.scale * self.params.attenuation / 100.0

    def __repr__(self):
        return f"PagOption({self.params}, scale={self.scale})"


def patch_pag(unet_patcher, scale=3.0, attenuation=0.0, start_step=0.0, end_step=1.0):
    """-> a clone of `unet_patcher` that carries Perturbed-Attention Guidance (the reference UI's fields and defaults)"""
    from ..modules.k_model import KModelFlux
    if isinstance(unet_patcher.model, KModelFlux):
        raise NotImplementedError(f"{FEATURE}: UNet models only")
    m = unet_patcher.clone()
    m.model_options[OPTION] = PagOption(PagParams(float(scale), float(attenuation), float(start_step), float(end_step)))
    return m


def pag_active(sampling_step, total_sampling_steps, start, end):
    """The reference's window test (denoiser_callback): start <= sampling_step / (total_sampling_steps - 1) <= end.  A one-step job, where the
    reference would divide by zero, is at position 0.0."""
    pos = sampling_step / (total_sampling_steps - 1) if total_sampling_steps > 1 else 0.0
    return pos >= start and pos <= end


def options_for_step(model_options, sampling_step, total_sampling_steps):
    """model_options as the step should see them: unchanged on a step that applies the guidance (or without the option), else a copy without
    the option -- a scale <= 0 (forge_perturbed_attention.py:68) or a step outside the window is an ordinary step: no third group, the plain
    graph, no decrement.  The patcher's own dict is never written."""
    opt = model_options.get(OPTION)
    if opt is None or (opt.scale > 0.0 and pag_active(sampling_step, total_sampling_steps, opt.params.start_step, opt.params.end_step)):
        return model_options
    return {k: v for k, v in model_options.items() if k != OPTION}


def pag_for_call(model_options):
    """-> the PagOption a model call has to apply, or None"""
    opt = model_options.get(OPTION)
    return opt if opt is not None and opt.scale > 0.0 else None


def reset(unet_patcher):
    """sampling_prepare: every sampling pass starts at the full scale"""
    opt = unet_patcher.model_options.get(OPTION)
    if opt is not None:
        opt.reset()
