"""Native FreeU v2 -- the patcher-level entry (reference: extensions-builtin/sd_forge_freeu/scripts/forge_freeu.py).

The reference's `patch_freeu_v2` installs a Python `output_block_patch`; here the parameters travel as the plain transformer option
"freeu_v2", which the UNet executor reads on its fast path (backend/nn/unet.py, hipops.freeu): no Python hook, so the step stays on the
captured graph, and no FFT.  The step window the reference keeps in class globals (freeu_start / freeu_end, evaluated by its
on_cfg_denoiser callback) is part of the parameters; backend/sampling/sampling_function.py drops the option on steps outside it."""
from collections import namedtuple

FreeUParams = namedtuple("FreeUParams", ["b1", "b2", "s1", "s2", "start", "end"], defaults=(0.0, 1.0))

OPTION = "freeu_v2"
FEATURE = "FreeU"

# name -> (b1, b2, s1, s2, start, end): the presets the reference's UI offers
PRESETS = {
    "Forge default": FreeUParams(1.01, 1.02, 0.99, 0.95, 0.0, 1.0),
    "SD 1.4": FreeUParams(1.3, 1.4, 0.9, 0.2, 0.0, 1.0),
    "SD 1.5": FreeUParams(1.5, 1.6, 0.9, 0.2, 0.0, 1.0),
    "SD 2.1": FreeUParams(1.4, 1.6, 0.9, 0.2, 0.0, 1.0),
    "SDXL": FreeUParams(1.3, 1.4, 0.9, 0.2, 0.0, 1.0),
}


def patch_freeu_v2(unet_patcher, b1, b2, s1, s2, start=0.0, end=1.0):
    """-> a clone of `unet_patcher` that carries FreeU v2 (the reference function's name and argument order, plus the step window).
    b1 / s1 act on the output blocks whose backbone input has 4 x model_channels channels, b2 / s2 on those with 2 x model_channels."""
    m = unet_patcher.clone()
    m.set_transformer_option(OPTION, FreeUParams(float(b1), float(b2), float(s1), float(s2), float(start), float(end)))
    return m


def freeu_active(sampling_step, total_sampling_steps, start, end):
    """The reference's window test: start <= sampling_step / (total_sampling_steps - 1) <= end.  A one-step job, where the reference would
    divide by zero, is at position 0.0."""
    pos = sampling_step / (total_sampling_steps - 1) if total_sampling_steps > 1 else 0.0
    return start <= pos <= end


def options_for_step(model_options, sampling_step, total_sampling_steps):
    """model_options as the step should see them: unchanged inside the FreeU window (or without FreeU), else a copy whose
    transformer_options lack the option.  The patcher's own dicts are never written."""
    to = model_options.get("transformer_options") or {}
    fu = to.get(OPTION)
    if fu is None or freeu_active(sampling_step, total_sampling_steps, fu.start, fu.end):
        return model_options
    out = dict(model_options)
    out["transformer_options"] = {k: v for k, v in to.items() if k != OPTION}
    return out


def freeu_graph_key(freeu):
    """what native FreeU adds to a graph key: ("freeu", b1, b2, s1, s2)"""
    return ("freeu",) + tuple(float(v) for v in freeu[:4])
