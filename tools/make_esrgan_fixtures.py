"""TEST INFRASTRUCTURE ONLY.  Generates tests/golden/esrgan_grid.pt with the REAL reference's tiling and upscaler-loop code
(<reference>/modules/images.py split_grid / combine_grid and <reference>/modules/upscaler.py Upscaler.upscale, imported at run time by file path;
nothing of them is copied).  Deterministic (seeded).

    python tools/make_esrgan_fixtures.py --reference /path/to/reference [--out tests/golden]

Both modules import the web UI (`modules.shared`, `sd_samplers`, `script_callbacks`, `modelloader`, ...) and a few third-party packages (pytz, piexif,
pillow_avif) that the three functions do not use: those entries of sys.modules are stubbed by permissive objects for the import and removed again.

Writes esrgan_grid.pt:
  grid[(w, h, tile, overlap)] = image (uint8 RGB [h, w, 3], tests/esrgan_refs.test_image(w, h, seed = w + h)), rows ([[y, tile_h, [[x, tile_w], ...]], ...]:
                                split_grid's origins), tiles (uint8 [count, tile, tile, 3]: the cropped tiles, PIL's black padding included), combined
                                (uint8 [h, w, 3]: combine_grid of the tiles after tile k was brightened by 16 k -- so the blend bands show which
                                tile contributes what)
  upscale[scale]              = (number of do_upscale passes, (width, height) of the result) of Upscaler.upscale on a 40 x 24 image with a fake x4
                                do_upscale (nearest resize), for scales 1, 1.5, 2, 4 and 5
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
GRID_CASES = [(48, 40, 32, 8), (33, 33, 32, 8), (24, 24, 32, 8), (64, 32, 32, 8)]
SCALES = [1, 1.5, 2, 4, 5]
STUBS = ("modules", "modules.shared", "modules.sd_samplers", "modules.script_callbacks", "modules.errors", "modules.stealth_infotext",
         "modules.paths_internal", "modules.modelloader", "pytz", "piexif", "piexif.helper", "pillow_avif")


class _Any(types.ModuleType):
    """a module whose every attribute is again such an object: truthy, callable, and good for nothing else"""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        v = _Any(f"{self.__name__}.{name}")
        setattr(self, name, v)
        return v

    def __call__(self, *a, **k):
        return self


def brighten(tile, k):
    return Image.fromarray(np.minimum(np.array(tile).astype(np.int32) + 16 * k, 255).astype(np.uint8), "RGB")


def import_reference(reference):
    saved = {k: sys.modules.get(k) for k in STUBS + ("modules.images", "modules.upscaler")}
    for name in STUBS:
        sys.modules[name] = _Any(name)
    sys.modules["modules"].__path__ = []
    shared = sys.modules["modules.shared"]
    shared.models_path = "models"
    shared.state = types.SimpleNamespace(interrupted=False)
    sys.modules["modules"].shared = shared
    try:
        mods = []
        for name in ("upscaler", "images"):
            spec = importlib.util.spec_from_file_location(f"modules.{name}", os.path.join(reference, "modules", f"{name}.py"))
            mod = importlib.util.module_from_spec(spec)
            sys.modules[f"modules.{name}"] = mod
            spec.loader.exec_module(mod)
            mods.append(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mods


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    import esrgan_refs as E
    upscaler, images = import_reference(args.reference)
    fx = {"grid": {}, "upscale": {}}
    for w, h, tile, overlap in GRID_CASES:
        img = E.test_image(w, h, seed=w + h)
        grid = images.split_grid(Image.fromarray(img.numpy(), "RGB"), tile, tile, overlap)
        rows = [[y, th, [[x, tw] for x, tw, _ in row]] for y, th, row in grid.tiles]
        tiles = [t for _, _, row in grid.tiles for _, _, t in row]
        k = 0
        for _, _, row in grid.tiles:
            for cell in row:
                cell[2] = brighten(cell[2], k)
                k += 1
        fx["grid"][(w, h, tile, overlap)] = dict(image=img, rows=rows, tiles=torch.from_numpy(np.stack([np.array(t) for t in tiles])),
                                                 combined=torch.from_numpy(np.array(images.combine_grid(grid))))

    class Fake(upscaler.Upscaler):
        name = None

        def do_upscale(self, img, selected_model=None):
            self.calls += 1
            return img.resize((img.width * 4, img.height * 4), resample=upscaler.NEAREST)

    for scale in SCALES:
        up = Fake()
        up.calls = 0
        res = up.upscale(Image.fromarray(E.test_image(40, 24, seed=1).numpy(), "RGB"), scale)
        fx["upscale"][scale] = (up.calls, tuple(res.size))
    path = os.path.join(args.out, "esrgan_grid.pt")
    torch.save(fx, path)
    print("wrote", path, os.path.getsize(path), "bytes;", {k: v for k, v in fx["upscale"].items()})


if __name__ == "__main__":
    main()
