"""Mirror of modules/esrgan_model.py: `UpscalerESRGAN(dirname)` lists the model files (.pt / .pth / .safetensors) of <models_path>/ESRGAN and of
`dirname` as scalers; `do_upscale` runs the native RRDBNet (forge_amd.backend.nn.esrgan) tile by tile.  Differences, on purpose: no URL is ever
used (with no file there is no scaler -- the reference would download ESRGAN_4x), checkpoints are read with `torch.load(weights_only=True)` or
safetensors, a model that cannot be loaded raises (the reference prints the error and returns the image not upscaled), and the loaded model is
cached per path.  The reference's loader is the `spandrel` package; the key-layout detection here (esrgan.canonicalize) stands in for it and is
parity-unpinned against it."""
import os

import torch

from . import shared
from .upscaler import Upscaler, UpscalerData
from .upscaler_utils import upscale_with_model

_models = {}


def friendly_name(path):
    return os.path.splitext(os.path.basename(path))[0]         # modules/modelloader.py friendly_name


def load_state_dict(path):
    if path.lower().endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path, device="cpu")
    return torch.load(path, map_location="cpu", weights_only=True)


class UpscalerESRGAN(Upscaler):
    def __init__(self, dirname=None):
        self.name = "ESRGAN"
        self.model_name = "ESRGAN_4x"
        self.scalers = []
        self.user_path = dirname
        super().__init__()
        for file in self.find_models(ext_filter=[".pt", ".pth", ".safetensors"]):
            self.scalers.append(UpscalerData(friendly_name(file), file, self, 4))

    def load_model(self, path):
        model = _models.get(path)
        if model is None:
            from ..backend.nn.esrgan import RRDBNet
            device = shared.device or (shared.sd_model.device if shared.sd_model is not None else "cuda")
            model = _models[path] = RRDBNet(load_state_dict(path), device=device, name=friendly_name(path))
        return model

    def do_upscale(self, img, selected_model):
        return esrgan_upscale(self.load_model(selected_model), img)


def esrgan_upscale(model, img):
    return upscale_with_model(model, img, tile_size=shared.opts.ESRGAN_tile, tile_overlap=shared.opts.ESRGAN_tile_overlap)


def register(dirname=None):
    """(re)builds shared.sd_upscalers as modules/modelloader.py load_upscalers does for the scalers this project has: None, Lanczos, Nearest, then
    the ESRGAN model files by name"""
    from .upscaler import UpscalerLanczos, UpscalerNearest, UpscalerNone
    datas = []
    for cls in (UpscalerNone, UpscalerLanczos, UpscalerNearest):
        datas += cls().scalers
    datas += sorted(UpscalerESRGAN(dirname).scalers, key=lambda x: x.name.lower())
    shared.sd_upscalers[:] = datas
    return shared.sd_upscalers
