"""Mirror of modules/upscaler_utils.py:38-88 for the native models: `upscale_with_model` splits the image into overlapping tiles on the host
(images.split_grid), sends the tiles through the model as batches -- the reference sends them one by one; the network has no cross-tile
term, so the tiles' pixels are the same -- and blends them back with images.combine_grid.  `model` is anything with
`upscale(uint8 RGB [n, h, w, 3]) -> uint8 RGB [n, s h, s w, 3]` (forge_amd.backend.nn.esrgan.RRDBNet): the BGR flip, the / 255 and the final
clamp-round of pil_image_to_torch_bgr / torch_bgr_to_pil_image (:14-35) are its pack / unpack kernels."""
import numpy as np
import torch
from PIL import Image

from . import images, shared


def _to_u8(img):
    return torch.from_numpy(np.array(img.convert("RGB")))


def upscale_pil_patch(model, img):
    return Image.fromarray(model.upscale(_to_u8(img)[None])[0].numpy(), "RGB")


def upscale_with_model(model, img, *, tile_size, tile_overlap=0, desc="tiled upscale"):
    if tile_size <= 0:
        return upscale_pil_patch(model, img)              # the whole image as one tile of arbitrary h x w
    grid = images.split_grid(img, tile_size, tile_size, tile_overlap)
    if shared.state.interrupted:
        return img
    flat = [tile for _, _, row in grid.tiles for _, _, tile in row]
    out = model.upscale(torch.stack([_to_u8(t) for t in flat]))
    scale_factor = out.shape[2] // tile_size
    it = iter(out)
    newtiles = [[y * scale_factor, h * scale_factor, [[x * scale_factor, w * scale_factor, Image.fromarray(next(it).numpy(), "RGB")] for x, w, _ in row]]
                for y, h, row in grid.tiles]
    newgrid = images.Grid(newtiles, tile_w=grid.tile_w * scale_factor, tile_h=grid.tile_h * scale_factor, image_w=grid.image_w * scale_factor,
                          image_h=grid.image_h * scale_factor, overlap=grid.overlap * scale_factor)
    return images.combine_grid(newgrid)
