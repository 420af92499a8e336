"""Native Dynamic Thresholding (CFG-Fix) -- the patcher-level entry (reference: extensions-builtin/sd_forge_dynamic_thresholding,
lib_dynamic_thresholding/dynthres.py and dynthres_core.py).

The reference installs a Python `sampler_cfg_function`: about 25 small launches per step, a full sort inside torch.quantile and a device read of
the timestep in the middle of the sampler loop; a step with such a function also leaves the fused denoise_cfg route.  Here the parameters
travel as the plain model option "dynthresh"; backend/sampling/sampling_function.py keeps the step on the route it would have taken, works the
schedule out on the host from the sigma values the samplers carry along, and replaces the CFG result by hipops.dynthresh of the two denoised
predictions (csrc/fmx_dynthresh.hip).  The reference forms `input - (input - denoised)` on the way into its function and `input - result` twice
on the way out, about an ulp of |x| each; the native route works on the denoised predictions directly."""
import math
from collections import namedtuple

import torch

OPTION = "dynthresh"

MODES = ["Constant", "Linear Down", "Cosine Down", "Half Cosine Down", "Linear Up", "Cosine Up", "Half Cosine Up", "Power Up", "Power Down",
         "Linear Repeating", "Cosine Repeating", "Sawtooth"]
STARTPOINTS = ["MEAN", "ZERO"]
VARIABILITIES = ["AD", "STD"]

# the twelve fields of the reference's UI with its defaults: the checkbox, then the argument order of DynamicThresholdingNode.patch
DynThreshParams = namedtuple("DynThreshParams", ["enabled", "mimic_scale", "threshold_percentile", "mimic_mode", "mimic_scale_min", "cfg_mode", "cfg_scale_min",
                                                 "sched_val", "separate_feature_channels", "scaling_startpoint", "variability_measure",
                                                 "interpolate_phi"],
                             defaults=(False, 7.0, 1.0, "Constant", 0.0, "Constant", 0.0, 1.0, "enable", "MEAN", "AD", 1.0))

MAX_STEPS = 999   # what DynamicThresholdingNode.patch hands to DynThresh


def interpret_scale(scale, mode, scale_min, step, sched_val, max_steps=MAX_STEPS):
    """dynthres_core.py:29-59: the scale of this step under one of the twelve schedules; host arithmetic in Python floats.  `frac` is
    step / (max_steps - 1), which reaches 999 / 998 at timestep 0 -- as in the reference."""
    if mode not in MODES:
        raise ValueError(f"unknown Dynamic Thresholding mode {mode!r}")
    scale -= scale_min
    frac = step / (max_steps - 1)
    if mode == "Linear Down":
        scale *= 1.0 - frac
    elif mode == "Half Cosine Down":
        scale *= math.cos(frac)
    elif mode == "Cosine Down":
        scale *= math.cos(frac * 1.5707)
    elif mode == "Linear Up":
        scale *= frac
    elif mode == "Half Cosine Up":
        scale *= 1.0 - math.cos(frac)
    elif mode == "Cosine Up":
        scale *= 1.0 - math.cos(frac * 1.5707)
    elif mode == "Power Up":
        scale *= math.pow(frac, sched_val)
    elif mode == "Power Down":
        scale *= 1.0 - math.pow(frac, sched_val)
    elif mode == "Linear Repeating":
        portion = (frac * sched_val) % 1.0
        scale *= (0.5 - portion) * 2 if portion < 0.5 else (portion - 0.5) * 2
    elif mode == "Cosine Repeating":
        scale *= math.cos(frac * 6.28318 * sched_val) * 0.5 + 0.5
    elif mode == "Sawtooth":
        scale *= (frac * sched_val) % 1.0
    return scale + scale_min


def scales_for_sigma(params, predictor, sigma_host, cond_scale):
    """-> (mimic, cfg) of the step whose sigmas are the HOST values `sigma_host` (k_model.host_sigmas): dynthres.py:41-43 takes
    step = 999 - predictor.timestep(sigma)[0] -- the table index for the UNet models, sigma itself for Flux -- without the reference's
    `.item()` on a device tensor."""
    time_step = predictor.timestep(torch.tensor([float(sigma_host[0])], dtype=torch.float32))[0].item()
    step = MAX_STEPS - time_step
    mimic = interpret_scale(params.mimic_scale, params.mimic_mode, params.mimic_scale_min, step, params.sched_val)
    cfg = interpret_scale(cond_scale, params.cfg_mode, params.cfg_scale_min, step, params.sched_val)
    return mimic, cfg


def patch_dynthresh(unet_patcher, mimic_scale=7.0, threshold_percentile=1.0, mimic_mode="Constant", mimic_scale_min=0.0, cfg_mode="Constant",
                    cfg_scale_min=0.0, sched_val=1.0, separate_feature_channels="enable", scaling_startpoint="MEAN", variability_measure="AD",
                    interpolate_phi=1.0):
    """-> a clone of `unet_patcher` that carries Dynamic Thresholding (the argument order of DynamicThresholdingNode.patch).  It displaces a
    Python sampler_cfg_function, as set_model_sampler_cfg_function displaces it: the last writer wins, as in the reference."""
    if mimic_mode not in MODES or cfg_mode not in MODES:
        raise ValueError(f"unknown Dynamic Thresholding mode {mimic_mode!r} / {cfg_mode!r}")
    if scaling_startpoint not in STARTPOINTS or variability_measure not in VARIABILITIES or separate_feature_channels not in ("enable", "disable"):
        raise ValueError("unknown Dynamic Thresholding choice: " + repr((separate_feature_channels, scaling_startpoint, variability_measure)))
    m = unet_patcher.clone()
    m.model_options.pop("sampler_cfg_function", None)
    m.model_options[OPTION] = DynThreshParams(True, float(mimic_scale), float(threshold_percentile), mimic_mode, float(mimic_scale_min), cfg_mode,
                                              float(cfg_scale_min), float(sched_val), separate_feature_channels, scaling_startpoint,
                                              variability_measure, float(interpolate_phi))
    return m

