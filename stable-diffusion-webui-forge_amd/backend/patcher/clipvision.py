"""Native CLIP-vision encoder -- the reference's surface (backend/patcher/clipvision.py): clip_preprocess, ClipVisionModel.encode_image, the OpenCLIP
key conversion, detection by depth and load(path).  What IP-Adapter (backend/patcher/ipadapter.py) and Revision (backend/patcher/revision.py) need
to start from an image.  The towers are backend/nn/clip_vision.py; nothing is downloaded, a file is looked up where the caller says.

clip_preprocess: movedim to NCHW; unless the image is 224 x 224 already, the antialiased bicubic resize to the reference's round(scale * side)
sizes (modules/latent_upscale.interpolate on fmx_resize_separable_f32) and the centre crop; then ONE pass of hipops.clip_patch_rows quantises to
8-bit levels, normalises and lays the crop out as the patch convolution's rows -- the normalised image itself is never stored."""
import torch

from ..nn import clip_vision as towers

SIZE = 224
# the three towers the reference knows, by family (transformers' CLIPVisionConfig fields)
_COMMON = dict(image_size=224, patch_size=14, num_channels=3, layer_norm_eps=1e-5, num_attention_heads=16)
CLIP_VISION_VITL = dict(_COMMON, hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, hidden_act="quick_gelu", projection_dim=768)
CLIP_VISION_H = dict(_COMMON, hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, hidden_act="gelu", projection_dim=1024)
CLIP_VISION_G = dict(_COMMON, hidden_size=1664, intermediate_size=8192, num_hidden_layers=48, hidden_act="gelu", projection_dim=1280)
_LAYER = "vision_model.encoder.layers.{}.layer_norm1.weight"


class Output:
    """item access and attribute access, as the reference's"""

    def __getitem__(self, key):
        return getattr(self, key)

    def __setitem__(self, key, item):
        setattr(self, key, item)


def preprocess_geometry(h, w, size=SIZE):
    """-> (resized h, resized w, top, left) of clip_preprocess for an h x w image: no resize when it is size x size already, else the short side to
    `size` with Python's round() on both, and the centre crop's offsets"""
    if h == size and w == size:
        return h, w, 0, 0
    scale = size / min(h, w)
    rh, rw = round(scale * h), round(scale * w)
    return rh, rw, (rh - size) // 2, (rw - size) // 2


def resized(image_bhwc, size=SIZE):
    """-> (fp32 NCHW device tensor after the resize, top, left)"""
    from ...modules.latent_upscale import interpolate
    if image_bhwc.dim() != 4 or image_bhwc.shape[-1] != 3:
        raise ValueError(f"clip_preprocess expects an image tensor [b, h, w, 3], got {tuple(image_bhwc.shape)}")
    if size != SIZE:
        raise NotImplementedError(f"clip_preprocess: size {size}; the towers are {SIZE} x {SIZE}")
    x = image_bhwc.movedim(-1, 1).to(dtype=torch.float32).contiguous()
    rh, rw, top, left = preprocess_geometry(x.shape[2], x.shape[3], size)
    if (rh, rw) != tuple(x.shape[2:]):
        x = interpolate(x, (rh, rw), mode="bicubic", antialias=True)
    return x, top, left


def clip_preprocess(image_bhwc, size=SIZE):
    """image [b, h, w, 3] in [0, 1] on the GPU -> fp16 [b * 256, 640], the towers' input (see the module docstring)"""
    from ... import hipops as ops
    x, top, left = resized(image_bhwc, size)
    return ops.clip_patch_rows(x, top, left)


class ClipVisionModel:
    def __init__(self, config, state_dict, device="cuda"):
        self.config = dict(config)
        self.load_device = torch.device(device)
        self.dtype = torch.float16
        self.tower = towers.CLIPVisionTower(config, state_dict, device)

    @property
    def output_width(self):
        """{output name: last dimension}: what an IP-Adapter file's clip_embeddings_dim is held against"""
        return {"image_embeds": self.tower.projection_dim, "penultimate_hidden_states": self.tower.hidden, "last_hidden_state": self.tower.hidden}

    def encode_image(self, image):
        return self.encode_pixel_rows(clip_preprocess(image.to(self.load_device)))

    @torch.inference_mode()
    def encode_pixel_rows(self, rows):
        """clip_preprocess's rows of one or several images (concatenated: one batch through the tower) -> Output, fp32"""
        out = self.tower.encode(rows)
        o = Output()
        for name in towers.OUTPUTS:
            o[name] = out[name].float()
        return o


def convert_to_transformers(sd, prefix):
    """OpenCLIP's visual tower (`prefix` = "visual.") -> transformers' keys: in_proj_weight / in_proj_bias split into q / k / v, ln_pre ->
    pre_layrnorm (transformers' own spelling), proj -> visual_projection.weight transposed.  Any other layout only loses the prefix."""
    if f"{prefix}transformer.resblocks.0.attn.in_proj_weight" not in sd:
        return {(k[len(prefix):] if prefix and k.startswith(prefix) else k): v for k, v in sd.items()}
    top = {"class_embedding": "vision_model.embeddings.class_embedding", "conv1.weight": "vision_model.embeddings.patch_embedding.weight",
           "positional_embedding": "vision_model.embeddings.position_embedding.weight", "ln_post.weight": "vision_model.post_layernorm.weight",
           "ln_post.bias": "vision_model.post_layernorm.bias", "ln_pre.weight": "vision_model.pre_layrnorm.weight", "ln_pre.bias": "vision_model.pre_layrnorm.bias"}
    block = {"ln_1": "layer_norm1", "ln_2": "layer_norm2", "mlp.c_fc": "mlp.fc1", "mlp.c_proj": "mlp.fc2", "attn.out_proj": "self_attn.out_proj"}
    out = {}
    for k, v in sd.items():
        name = k[len(prefix):] if k.startswith(prefix) else None
        if name in top:
            out[top[name]] = v
        elif name == "proj":
            out["visual_projection.weight"] = v.transpose(0, 1)
        elif name is not None and name.startswith("transformer.resblocks."):
            i, rest = name[len("transformer.resblocks."):].split(".", 1)
            to = f"vision_model.encoder.layers.{i}."
            if rest in ("attn.in_proj_weight", "attn.in_proj_bias"):
                n = v.shape[0] // 3
                for j, p in enumerate(("q_proj", "k_proj", "v_proj")):
                    out[f"{to}self_attn.{p}.{rest.rsplit('_', 1)[1]}"] = v[n * j:n * (j + 1)]
            else:
                mod, leaf = rest.rsplit(".", 1)
                out[f"{to}{block[mod]}.{leaf}" if mod in block else k] = v
        else:
            out[k] = v
    return out


def detect_config(sd):
    """by depth, as the reference does: layer 47 -> bigG, 30 -> H, 22 -> L; None otherwise"""
    for layer, config in ((47, CLIP_VISION_G), (30, CLIP_VISION_H), (22, CLIP_VISION_VITL)):
        if _LAYER.format(layer) in sd:
            return config
    return None


def load_clipvision_from_sd(sd, prefix="", convert_keys=False, device="cuda"):
    if convert_keys:
        sd = convert_to_transformers(sd, prefix)
    config = detect_config(sd)
    if config is None:
        return None
    return ClipVisionModel(config, sd, device)


def load(ckpt_path, device="cuda"):
    from ..loader import load_torch_file
    sd = load_torch_file(ckpt_path)
    if "visual.transformer.resblocks.0.attn.in_proj_weight" in sd:
        return load_clipvision_from_sd(sd, prefix="visual.", convert_keys=True, device=device)
    return load_clipvision_from_sd(sd, device=device)
