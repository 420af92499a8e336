"""Native Kohya HRFix (Deep Shrink) -- the patcher-level entry (reference: extensions-builtin/sd_forge_kohya_hrfix/scripts/kohya_hrfix.py,
PatchModelAddDownscale).

The reference installs a Python input_block_patch (or input_block_patch_after_skip) and an output_block_patch; here the parameters travel as
the plain transformer option "kohya_hrfix", which the UNet executor reads on its fast path (backend/nn/unet.py, hipops.resize_nhwc): no Python
hook, so the step stays on the captured graph, and no device read for the sigma window -- KModel tests the step's host sigma and hands the
option to the executor only inside the window (backend/modules/k_model.py).  The reference's side globals shared.kohya_shrink_shape* are
not mirrored."""
from collections import namedtuple

from ... import hipops as ops

KohyaHRFixParams = namedtuple("KohyaHRFixParams", ["block_number", "downscale_factor", "start_percent", "end_percent", "downscale_after_skip",
                                                   "downscale_method", "upscale_method", "sigma_start", "sigma_end"])

OPTION = "kohya_hrfix"
FEATURE = "Kohya HRFix"


def _check_method(name):
    if name == "bislerp":
        raise NotImplementedError("Kohya HRFix: bislerp is not separable and has no native route; the Python patches "
                                  "(input_block_patch / output_block_patch) remain available for it")
    if name not in ops.RESIZE_NHWC_MODES:     # the separable ones: one pass of fmx_resize_nhwc_f16
        raise ValueError(f"Kohya HRFix: unknown resize method {name!r}; known: {ops.RESIZE_NHWC_MODES + ('bislerp',)}")


def patch_kohya_hrfix(unet_patcher, block_number=3, downscale_factor=2.0, start_percent=0.0, end_percent=0.35, downscale_after_skip=True,
                      downscale_method="bicubic", upscale_method="bicubic"):
    """-> a clone of `unet_patcher` that carries Kohya HRFix (the reference's PatchModelAddDownscale.patch, its argument order)."""
    _check_method(downscale_method)
    _check_method(upscale_method)
    if not float(downscale_factor) > 0.0:
        raise ValueError(f"Kohya HRFix: downscale_factor must be positive, got {downscale_factor}")
    from ..modules.k_model import KModelFlux
    if isinstance(unet_patcher.model, KModelFlux):
        raise NotImplementedError("Kohya HRFix: UNet models only")
    predictor = unet_patcher.model.predictor
    if unet_patcher.model_options.get("transformer_options", {}).get("freeu_v2") is not None:
        from .native_call import message
        raise NotImplementedError(message("shrink", "freeu"))
    m = unet_patcher.clone()
    m.set_transformer_option(OPTION, KohyaHRFixParams(int(block_number), float(downscale_factor), float(start_percent), float(end_percent),
                                                      bool(downscale_after_skip), downscale_method, upscale_method,
                                                      predictor.percent_to_sigma(start_percent), predictor.percent_to_sigma(end_percent)))
    return m


def shrunk_size(height, width, downscale_factor):
    """-> (height, width) of the shrunk hidden state: the reference's round(extent * (1.0 / factor)), Python's round (ties to even)"""
    return round(height * (1.0 / downscale_factor)), round(width * (1.0 / downscale_factor))


def shrink_active(params, sigma):
    """The reference's window test on the first sample's sigma: sigma_end <= sigma <= sigma_start."""
    return sigma <= params.sigma_start and sigma >= params.sigma_end


def shrink_for_step(transformer_options, sig_host):
    """-> the job's KohyaHRFixParams when the step whose host sigmas are `sig_host` lies inside the window, else None"""
    params = (transformer_options or {}).get(OPTION)
    if params is None or not shrink_active(params, float(sig_host[0])):
        return None
    return params


def shrink_graph_key(params):
    """what an active shrink adds to a graph key: everything that decides which kernels the captured forward launches"""
    return ("kohya_hrfix", params.block_number, params.downscale_factor, params.downscale_after_skip, params.downscale_method,
            params.upscale_method)
