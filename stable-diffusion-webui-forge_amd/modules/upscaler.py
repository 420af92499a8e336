"""Mirror of modules/upscaler.py: the image-space upscaler base (`Upscaler.upscale` :54-76: destination size `// 8 * 8`, up to three passes of
`do_upscale`, a final LANCZOS resize to the destination) and the three built-in scalers (:109-151).  PIL on the host, as in the reference."""
import os

from PIL import Image

from . import shared

LANCZOS = Image.Resampling.LANCZOS if hasattr(Image, "Resampling") else Image.LANCZOS
NEAREST = Image.Resampling.NEAREST if hasattr(Image, "Resampling") else Image.NEAREST


class Upscaler:
    name = None
    model_path = None
    model_name = None
    user_path = None
    scalers: list

    def __init__(self, create_dirs=False):
        self.tile_size = shared.opts.ESRGAN_tile
        self.tile_pad = shared.opts.ESRGAN_tile_overlap
        self.device = shared.device
        self.scale = 1
        if self.model_path is None and self.name:
            self.model_path = os.path.join(shared.models_path, self.name)
        if self.model_path and create_dirs:
            os.makedirs(self.model_path, exist_ok=True)

    def do_upscale(self, img, selected_model):
        return img

    def upscale(self, img, scale, selected_model=None):
        self.scale = scale
        dest_w = int((img.width * scale) // 8 * 8)
        dest_h = int((img.height * scale) // 8 * 8)
        for i in range(3):
            if img.width >= dest_w and img.height >= dest_h and (i > 0 or scale != 1):
                break
            if shared.state.interrupted:
                break
            shape = (img.width, img.height)
            img = self.do_upscale(img, selected_model)
            if shape == (img.width, img.height):
                break
        if img.width != dest_w or img.height != dest_h:
            img = img.resize((int(dest_w), int(dest_h)), resample=LANCZOS)
        return img

    def load_model(self, path):
        pass

    def find_models(self, ext_filter=None):
        """model files (never URLs: nothing is downloaded) in <models_path>/<name> and in the user's directory, sorted by name"""
        found = []
        for d in (self.model_path, self.user_path):
            if d and os.path.isdir(d):
                for f in sorted(os.listdir(d)):
                    full = os.path.join(d, f)
                    if os.path.isfile(full) and (ext_filter is None or os.path.splitext(f)[1].lower() in ext_filter) and full not in found:
                        found.append(full)
        return found


class UpscalerData:
    def __init__(self, name, path, upscaler=None, scale=4, model=None, sha256=None):
        self.name = name
        self.data_path = path
        self.local_data_path = path
        self.scaler = upscaler
        self.scale = scale
        self.model = model
        self.sha256 = sha256

    def __repr__(self):
        return f"<UpscalerData name={self.name} path={self.data_path} scale={self.scale}>"


class UpscalerNone(Upscaler):
    name = "None"

    def __init__(self, dirname=None):
        super().__init__(False)
        self.scalers = [UpscalerData("None", None, self)]


class UpscalerLanczos(Upscaler):
    def do_upscale(self, img, selected_model=None):
        return img.resize((int(img.width * self.scale), int(img.height * self.scale)), resample=LANCZOS)

    def __init__(self, dirname=None):
        super().__init__(False)
        self.name = "Lanczos"
        self.scalers = [UpscalerData("Lanczos", None, self)]


class UpscalerNearest(Upscaler):
    def do_upscale(self, img, selected_model=None):
        return img.resize((int(img.width * self.scale), int(img.height * self.scale)), resample=NEAREST)

    def __init__(self, dirname=None):
        super().__init__(False)
        self.name = "Nearest"
        self.scalers = [UpscalerData("Nearest", None, self)]
