"""MI355X-native TAESD decoder: the tiny autoencoder behind the "TAESD" live-preview method and the "TAESD" VAE decode method.

Reference: modules/sd_vae_taesd.py:16-44 -- `decoder(latent_channels)` is an nn.Sequential of
    0 Clamp (tanh(x / 3) * 3), 1 conv(L, 64), 2 ReLU,
    3-5 Block x3, 6 Upsample(2), 7 conv(64, 64, bias=False),   8-10 Block x3, 11 Upsample(2), 12 conv(bias=False),
    13-15 Block x3, 16 Upsample(2), 17 conv(bias=False),        18 Block, 19 conv(64, 3)
with Block(x) = relu(conv.4(relu(conv.2(relu(conv.0(x))))) + x)  (:26-34; 64 -> 64, so `skip` is the identity and has no weights).
It takes RAW latents (no process_out) and returns an image in about [0, 1] (modules/sd_samplers_common.py:56-61 then maps it to [-1, 1]).

Here: 16-bit NHWC activations in an Arena, every 64 -> 64 convolution one launch of the direct kernel `hipops.conv3x3_c64` with its ReLU / residual /
nearest-upsample epilogues (csrc/fmx_conv_c64.hip), the first convolution on the same kernel with its weight zero-padded to 64 input channels (the
packed latent carries zeros there), the last one on `hipops.conv3x3_narrow`.  Stored tensors -- the rounding sites -- are exactly the reference
module outputs a 16-bit run of it stores, minus the pre-activation ones: conv and ReLU (and the Block's add) are one rounding here.
The encoder half (modules/sd_vae_taesd.py:47-54, `sd_vae_encode_method = "TAESD"`) is not built.
"""
import torch

from ... import hipops as ops
from ...runtime import Arena
from .unet import _conv_w

# modules/sd_vae_taesd.py:37-44 by Sequential index
_BLOCKS = ((3, 4, 5), (8, 9, 10), (13, 14, 15), (18,))
_UPS = (7, 12, 17)
_OUT = 19


def expected_keys():
    """state-dict keys of the reference `decoder()`, in execution order (biases of the three Upsample convolutions do not exist)"""
    keys = ["1.weight", "1.bias"]
    for level, blocks in enumerate(_BLOCKS):
        for i in blocks:
            for j in (0, 2, 4):
                keys += [f"{i}.conv.{j}.weight", f"{i}.conv.{j}.bias"]
        if level < len(_UPS):
            keys.append(f"{_UPS[level]}.weight")
    return keys + [f"{_OUT}.weight", f"{_OUT}.bias"]


def detect_latent_channels(state_dict):
    """latent channels of a TAESD decoder state dict, read off `1.weight` ([64, L, 3, 3]); refuses any other key layout, naming what is missing"""
    for k in expected_keys():
        if k not in state_dict:
            raise ValueError(f"not a TAESD decoder state dict (modules/sd_vae_taesd.py:37-44 nn.Sequential layout): key '{k}' is missing")
    w = state_dict["1.weight"]
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or w.shape[0] != 64 or not 1 <= w.shape[1] <= 64:
        raise ValueError(f"not a TAESD decoder state dict: '1.weight' is {tuple(w.shape)}, expected [64, latent_channels <= 64, 3, 3]")
    for k in expected_keys()[2:-2]:
        want = (64, 64, 3, 3) if k.endswith("weight") else (64,)
        if tuple(state_dict[k].shape) != want:
            raise ValueError(f"not a TAESD decoder state dict: '{k}' is {tuple(state_dict[k].shape)}, expected {want}")
    if tuple(state_dict[f"{_OUT}.weight"].shape) != (3, 64, 3, 3):
        raise ValueError(f"not a TAESD decoder state dict: '{_OUT}.weight' is {tuple(state_dict[f'{_OUT}.weight'].shape)}, expected (3, 64, 3, 3)")
    return int(w.shape[1])


class TAESDDecoder:
    latent_magnitude = 3      # modules/sd_vae_taesd.py:58-59 (kept for callers that read them; the decoder itself does not use them)
    latent_shift = 0.5

    def __init__(self, state_dict, latent_channels=None, device="cuda", dtype=torch.float16):
        if dtype not in (torch.float16, torch.bfloat16):
            raise NotImplementedError(f"TAESD element type {dtype}: the native decoder is built for float16 and bfloat16")
        found = detect_latent_channels(state_dict)
        if latent_channels is not None and int(latent_channels) != found:
            raise ValueError(f"TAESD decoder: latent_channels={latent_channels} but '1.weight' has {found} input channels")
        self.latent_channels = found
        self.device = torch.device(device)
        self.dtype = dtype
        self.tap = None             # test hook: a dict that receives every stored tensor of the next decode as fp32 NCHW (see _tap)
        self._arena = None
        dev = self.device

        def conv(k, bias=True):
            return (_conv_w(state_dict[k + ".weight"].to(dev, dtype)), state_dict[k + ".bias"].to(dev, dtype).contiguous() if bias else None)

        w1 = state_dict["1.weight"].to(dev, dtype)
        w1p = w1.new_zeros(64, 64, 3, 3)
        w1p[:, :found] = w1
        self.w = {"1": (_conv_w(w1p), state_dict["1.bias"].to(dev, dtype).contiguous())}
        for blocks in _BLOCKS:
            for i in blocks:
                for j in (0, 2, 4):
                    self.w[f"{i}.conv.{j}"] = conv(f"{i}.conv.{j}")
        for i in _UPS:
            self.w[str(i)] = conv(str(i), bias=False)
        self.w[str(_OUT)] = conv(str(_OUT))

    def _tap(self, key, t):
        if self.tap is not None:
            self.tap[key] = t.permute(0, 3, 1, 2).float().cpu()

    @staticmethod
    def arena_bytes(b, h, w):
        """four [pixels, 64] buffers per resolution level (1 + 4 + 16 + 64 times the latent's pixels), the [pixels, 4] output, the packed latent"""
        m0 = b * h * w
        return m0 * 128 * (4 * 85 + 1) + m0 * 64 * 8 + (1 << 16)

    def decode(self, z):
        """fp32 NCHW raw latent [B, L, h, w] -> the network's output, fp32 NCHW [B, 3, 8h, 8w] (an image in about [0, 1])"""
        if z.dim() != 4 or z.shape[1] != self.latent_channels:
            raise ValueError(f"TAESD decoder for {self.latent_channels} latent channels got a latent of shape {tuple(z.shape)}")
        z = z.to(device=self.device, dtype=torch.float32).contiguous()
        b, _, hh, ww = z.shape
        need = self.arena_bytes(b, hh, ww)
        if self._arena is None or self._arena.capacity < need:
            self._arena = None
            self._arena = Arena(need, self.device)
        arena = self._arena
        arena.reset()
        with arena:
            y = self._decode_impl(z)
        oh, ow = 8 * hh, 8 * ww
        out = torch.empty((b, 3, oh, ow), dtype=torch.float32, device=self.device)
        ops.strided_copy4(y, out, (b, 3, oh, ow), (oh * ow * 4, 1, ow * 4, 4), (3 * oh * ow, oh * ow, ow, 1))
        return out

    def _decode_impl(self, z):
        b, lc, hh, ww = z.shape
        dt = self.dtype
        x = ops.taesd_pack_latent(z, dtype=dt)                                                  # 0: Clamp, [B, h, w, 64] zero padded
        self._tap("0", x[..., :lc])
        bufs = [ops.empty((b * hh * ww, 64), dt) for _ in range(4)]
        cur = ops.conv3x3_c64(x, *self.w["1"], relu=True, out=bufs[0])                          # 1, 2
        self._tap("1", cur.view(b, hh, ww, 64))
        for level, blocks in enumerate(_BLOCKS):
            m = b * hh * ww
            _, ta, tb, nxt = bufs
            for i in blocks:
                k = f"{i}.conv."
                ops.conv3x3_c64(cur.view(b, hh, ww, 64), *self.w[k + "0"], relu=True, out=ta)
                self._tap(k + "0", ta.view(b, hh, ww, 64))
                ops.conv3x3_c64(ta.view(b, hh, ww, 64), *self.w[k + "2"], relu=True, out=tb)
                self._tap(k + "2", tb.view(b, hh, ww, 64))
                ops.conv3x3_c64(tb.view(b, hh, ww, 64), *self.w[k + "4"], residual=cur, relu=True, out=nxt)    # fuse(conv(x) + skip(x)): add, then ReLU
                self._tap(str(i), nxt.view(b, hh, ww, 64))
                cur, nxt = nxt, cur
            if level < len(_UPS):
                up = str(_UPS[level])
                bufs = [ops.empty((4 * m, 64), dt) for _ in range(4)]
                nxt_level = ops.conv3x3_c64(cur.view(b, hh, ww, 64), self.w[up][0], None, up2x=True, out=bufs[0])    # Upsample + conv(bias=False)
                hh, ww = 2 * hh, 2 * ww
                cur = nxt_level
                self._tap(up, cur.view(b, hh, ww, 64))
        y = ops.conv3x3_narrow(cur.view(b, hh, ww, 64), *self.w[str(_OUT)], 3)                  # 19: [pixels, 4], column 3 zeros
        self._tap(str(_OUT), y.view(b, hh, ww, 4)[..., :3])
        return y
