"""MI355X-native ESRGAN-family upscaler: RRDBNet with nf 64, gc 32 and two x2 stages (ESRGAN_4x, R-ESRGAN 4x+, R-ESRGAN 4x+ Anime6B, 4x-UltraSharp,
4x_NMKD-Siax, ...) -- the image-space upscalers of the hires pass (modules/esrgan_model.py, modules/upscaler_utils.py:38-88).

The network (the reference resolves it inside the `spandrel` package; restated in tests/esrgan_refs.py):
    fea   = conv_first(x)                                                   3 -> 64
    RRDB  = x + 0.2 * RDB3(RDB2(RDB1(x)))                                   nb of them (23, or 6 for Anime6B)
    RDB   = x + 0.2 * conv5(cat(x, x1, x2, x3, x4)),  x_k = lrelu(conv_k(cat(x, x1 .. x_{k-1})), 0.2)     64 (+32 per step) -> 32, conv5 192 -> 64
    out   = conv_last(lrelu(HRconv(lrelu(upconv2(up2(lrelu(upconv1(up2(trunk_conv(trunk) + fea)))))))))
on BGR images in [0, 1] (pil_image_to_torch_bgr / torch_bgr_to_pil_image).

Here: fp16 NHWC activations in an Arena.  A dense block lives in ONE 192-channel buffer [x | x1 | x2 | x3 | x4]: conv_k is one launch of
`hipops.conv3x3_dense` that reads columns [0, 64 + 32 (k - 1)) and writes the next 32 IN PLACE (no concatenation); conv5 writes the next block's first
64 columns into another buffer with the `0.2 * f + x` residual in its epilogue.  Three such buffers rotate A -> B -> C -> A: the third RDB's conv5 also
takes the RRDB's residual (`beta = 0.2, res2 = RRDB input`, still in A's first 64 columns) and overwrites exactly those elements -- the product
0.2 * (0.2 * conv5 + x_rdb) + x_rrdb is rounded ONCE, where a 16-bit run of the reference rounds the RDB output first (a declared site; the test
restatement models it).  conv_first runs on the dense kernel with its weight zero-padded to 64 input channels (the packed image carries zeros there),
the two upsample convolutions stage from the half-resolution source (up2x), conv_last runs on `hipops.conv3x3_narrow`.

Key layouts: `canonicalize` maps the three public ones onto the "new arch" names and refuses everything this executor is not (see its docstring).  The
reference delegates this to spandrel, which is not part of it: the loader is parity-unpinned against the reference, like huggingface_guess.
"""
import re

import torch

from ... import hipops as ops
from ...runtime import Arena
from .unet import _conv_w

NF, GC = 64, 32
_OLD_TAIL = {"model.3": "upconv1", "model.6": "upconv2", "model.8": "HRconv", "model.10": "conv_last"}
_REAL = {"conv_body": "trunk_conv", "conv_up1": "upconv1", "conv_up2": "upconv2", "conv_hr": "HRconv"}
_OTHER_ARCH = (("layers.0.residual_group", "SwinIR / HAT / DAT (window-attention transformers)"), ("relative_position", "SwinIR / HAT / DAT (window-attention transformers)"),
               ("m_head", "ScuNET"), ("m_down1", "ScuNET"), ("attn", "an attention network (SwinIR / DAT / HAT)"))


def canonicalize(state_dict):
    """-> (state dict under the "new arch" names conv_first, RRDB_trunk.N.RDBk.convj, trunk_conv, upconv1, upconv2, HRconv, conv_last; nb).
    Accepts the "old arch" layout (model.0, model.1.sub.N.RDBk.convj.0, model.1.sub.<nb>, model.3 / 6 / 8 / 10), the "new arch" one and Real-ESRGAN's
    (an optional params_ema / params wrapper, body.N.rdbk.convj, conv_body, conv_up1 / 2, conv_hr).  Raises NotImplementedError, naming the reason, for
    Real-ESRGAN x2 / x1 files (pixel-unshuffled conv_first), ESRGAN+ ("plus": conv1x1 keys), nf / gc other than 64 / 32, other scales and other
    architectures."""
    for wrap in ("params_ema", "params"):
        if wrap in state_dict and isinstance(state_dict[wrap], dict):
            state_dict = state_dict[wrap]
            break
    keys = list(state_dict)
    if any("conv1x1" in k for k in keys):
        raise NotImplementedError("ESRGAN+ ('plus') model: its dense blocks have conv1x1 shortcuts, which the native RRDBNet does not build")
    out = {}
    if any(k.startswith("model.1.sub.") for k in keys):                                     # old arch
        subs = sorted({int(m.group(1)) for k in keys for m in [re.match(r"model\.1\.sub\.(\d+)\.", k)] if m})
        nb = subs[-1]
        tail = {k.rsplit(".", 1)[0] for k in keys if not k.startswith("model.1.") and k != "model.0.weight" and k != "model.0.bias"}
        if tail != set(_OLD_TAIL):
            raise NotImplementedError(f"ESRGAN old-arch model with layers {sorted(tail)} after the trunk: only the x4 layout (two x2 stages: model.3, model.6, "
                                      "model.8, model.10) is on the native path")
        for k, v in state_dict.items():
            stem, leaf = k.rsplit(".", 1)
            m = re.fullmatch(r"model\.1\.sub\.(\d+)\.RDB(\d)\.conv(\d)\.0", stem)
            if m:
                out[f"RRDB_trunk.{m.group(1)}.RDB{m.group(2)}.conv{m.group(3)}.{leaf}"] = v
            elif stem == "model.0":
                out[f"conv_first.{leaf}"] = v
            elif stem == f"model.1.sub.{nb}":
                out[f"trunk_conv.{leaf}"] = v
            elif stem in _OLD_TAIL:
                out[f"{_OLD_TAIL[stem]}.{leaf}"] = v
            else:
                raise NotImplementedError(f"ESRGAN old-arch model: unexpected key '{k}'")
    elif any(k.startswith("body.") for k in keys) and "conv_first.weight" in state_dict:    # Real-ESRGAN
        for k, v in state_dict.items():
            stem, leaf = k.rsplit(".", 1)
            m = re.fullmatch(r"body\.(\d+)\.rdb(\d)\.conv(\d)", stem)
            if m:
                out[f"RRDB_trunk.{m.group(1)}.RDB{m.group(2)}.conv{m.group(3)}.{leaf}"] = v
            else:
                out[f"{_REAL.get(stem, stem)}.{leaf}"] = v
    elif any(k.startswith("RRDB_trunk.") for k in keys) and "conv_first.weight" in state_dict:
        out = dict(state_dict)
    else:
        for marker, what in _OTHER_ARCH:
            if any(marker in k for k in keys):
                raise NotImplementedError(f"not an RRDBNet state dict: it looks like {what}; only ESRGAN-family RRDBNet models are on the native path")
        raise NotImplementedError(f"not an RRDBNet state dict (none of the old-arch, new-arch and Real-ESRGAN key layouts): first keys {keys[:4]}")
    blocks = sorted({int(m.group(1)) for k in out for m in [re.match(r"RRDB_trunk\.(\d+)\.", k)] if m})
    nb = len(blocks)
    if not nb or blocks != list(range(nb)):
        raise NotImplementedError(f"RRDBNet state dict with trunk blocks {blocks}: expected 0 .. nb-1")
    cf = out["conv_first.weight"]
    if cf.shape[1] in (12, 48):
        raise NotImplementedError(f"Real-ESRGAN x{2 if cf.shape[1] == 12 else 1} model: conv_first takes a pixel-unshuffled input of {cf.shape[1]} channels; only x4 "
                                  "models (3 input channels) are on the native path")
    nf, gc = cf.shape[0], out["RRDB_trunk.0.RDB1.conv1.weight"].shape[0]
    if (nf, gc) != (NF, GC):
        raise NotImplementedError(f"RRDBNet with nf {nf}, gc {gc}: the native dense-block kernel is built for nf 64, gc 32")
    want = {"conv_first": (NF, 3), "trunk_conv": (NF, NF), "upconv1": (NF, NF), "upconv2": (NF, NF), "HRconv": (NF, NF), "conv_last": (3, NF)}
    for i in range(nb):
        for r in (1, 2, 3):
            for j in range(1, 6):
                want[f"RRDB_trunk.{i}.RDB{r}.conv{j}"] = (GC if j < 5 else NF, NF + GC * (j - 1))
    for name, (co, ci) in want.items():
        for leaf, shape in (("weight", (co, ci, 3, 3)), ("bias", (co,))):
            t = out.get(f"{name}.{leaf}")
            if t is None:
                raise NotImplementedError(f"RRDBNet state dict without '{name}.{leaf}': only the x4 layout with two x2 stages is on the native path")
            if tuple(t.shape) != shape:
                raise NotImplementedError(f"RRDBNet '{name}.{leaf}' is {tuple(t.shape)}, expected {shape} (3 in / 3 out channels, nf 64, gc 32)")
    extra = sorted(k for k in out if k.rsplit(".", 1)[0] not in want)
    if extra:
        raise NotImplementedError(f"RRDBNet state dict with layers the native executor does not run: {extra[:4]}")
    return out, nb


class RRDBNet:
    scale = 4
    # bytes of arena per INPUT pixel of a group: image 3, packed 64 ch, fea 64, three 192-channel block buffers, trunk 64, up1 4 x 64, up2 and HR 16 x 64,
    # conv_last 16 x 4 (fp16 each), the uint8 output 16 x 3
    BYTES_PER_PIXEL = 3 + 2 * (64 + 64 + 3 * 192 + 64 + 4 * 64 + 2 * 16 * 64 + 16 * 4) + 16 * 3

    def __init__(self, state_dict, device="cuda", name="ESRGAN", group_bytes=2 << 30):
        sd, self.nb = canonicalize(state_dict)
        self.name = name
        self.device = torch.device(device)
        self.group_bytes = int(group_bytes)
        self.tap = None             # test hook: a dict that receives every stored tensor of the next group as fp16 NHWC on the CPU
        self._arena = None
        dev = self.device

        def conv(k):
            return (_conv_w(sd[k + ".weight"].to(dev, torch.float16)), sd[k + ".bias"].to(dev, torch.float16).contiguous())

        wf = sd["conv_first.weight"].to(dev, torch.float16)
        wfp = wf.new_zeros(NF, NF, 3, 3)
        wfp[:, :3] = wf
        self.w = {"conv_first": (_conv_w(wfp), sd["conv_first.bias"].to(dev, torch.float16).contiguous())}
        for k in ("trunk_conv", "upconv1", "upconv2", "HRconv", "conv_last"):
            self.w[k] = conv(k)
        for i in range(self.nb):
            for r in (1, 2, 3):
                for j in range(1, 6):
                    k = f"RRDB_trunk.{i}.RDB{r}.conv{j}"
                    self.w[k] = conv(k)

    def _tap(self, key, t):
        if self.tap is not None:
            self.tap[key] = t.detach().cpu().clone()

    def tiles_per_group(self, h, w):
        return max(1, self.group_bytes // (h * w * self.BYTES_PER_PIXEL + 16 * Arena.ALIGN))

    def upscale(self, tiles):
        """uint8 RGB tiles [n, h, w, 3] (equal size, any device) -> uint8 RGB [n, 4h, 4w, 3] on the CPU; groups of tiles_per_group(h, w) tiles go through
        the network as one batch each.  Raises RuntimeError if the fp16 network output of a group is not finite."""
        if tiles.dtype != torch.uint8 or tiles.dim() != 4 or tiles.shape[3] != 3:
            raise TypeError(f"RRDBNet.upscale expects uint8 RGB tiles [n, h, w, 3], got {tiles.dtype} {tuple(tiles.shape)}")
        n, h, w, _ = tiles.shape
        per = self.tiles_per_group(h, w)
        need = min(n, per) * (h * w * self.BYTES_PER_PIXEL + 16 * Arena.ALIGN)
        if self._arena is None or self._arena.capacity < need:
            self._arena = None
            self._arena = Arena(need, self.device)
        out = torch.empty((n, 4 * h, 4 * w, 3), dtype=torch.uint8)
        for lo in range(0, n, per):
            self._arena.reset()
            with self._arena:
                out[lo:lo + per] = self._forward(tiles[lo:lo + per].contiguous()).cpu()
        return out

    def _forward(self, tiles):
        n, h, w, _ = tiles.shape
        m = n * h * w
        f16 = torch.float16
        img = ops.empty((n, h, w, 3), torch.uint8, self.device)
        img.copy_(tiles)
        x = ops.esrgan_pack_image(img)
        self._tap("pack", x[..., :3])
        fea = ops.empty((m, NF), f16)
        bufs = [ops.empty((m, 192), f16) for _ in range(3)]

        def nhwc(buf, c, hh=h, ww=w):
            ld = buf.stride(0)
            return buf.as_strided((n, hh, ww, c), (hh * ww * ld, ww * ld, ld, 1))

        # conv_first twice: `fea` is kept for the trunk's residual, the first block needs the same values as columns [0, 64) of its 192-channel buffer
        ops.conv3x3_dense(x, NF, *self.w["conv_first"], out=fea)
        ops.conv3x3_dense(x, NF, *self.w["conv_first"], out=bufs[0][:, :NF])
        self._tap("conv_first", fea.view(n, h, w, NF))
        for i in range(self.nb):
            a = bufs[0]
            for r in (1, 2, 3):
                cur, nxt = bufs[r - 1], bufs[r % 3]
                k = f"RRDB_trunk.{i}.RDB{r}.conv"
                for j in range(1, 5):
                    cin = NF + GC * (j - 1)
                    ops.conv3x3_dense(nhwc(cur, cin), cin, *self.w[f"{k}{j}"], slope=0.2, out=cur[:, cin:cin + GC])
                if self.tap is not None:
                    self._tap(f"{i}.{r}.in", cur.view(n, h, w, 192))                                  # [x | x1 | x2 | x3 | x4] of this block
                if r < 3:
                    ops.conv3x3_dense(nhwc(cur, 192), 192, *self.w[f"{k}5"], res1=cur[:, :NF], alpha=0.2, out=nxt[:, :NF])
                else:   # RDB3 writes the next RRDB's input over this RRDB's input, element by element: each is read (res2) by the lane that writes it
                    if self.tap is not None:
                        self._tap(f"{i}.in", a[:, :NF].reshape(n, h, w, NF))
                    ops.conv3x3_dense(nhwc(cur, 192), 192, *self.w[f"{k}5"], res1=cur[:, :NF], alpha=0.2, res2=a[:, :NF], beta=0.2, out=a[:, :NF])
                if self.tap is not None:
                    self._tap(f"{i}.{r}", nxt[:, :NF].reshape(n, h, w, NF))
        trunk = ops.conv3x3_dense(nhwc(bufs[0], NF), NF, *self.w["trunk_conv"], res1=fea)          # trunk_conv(trunk) + fea
        self._tap("trunk", trunk.view(n, h, w, NF))
        up1 = ops.conv3x3_dense(trunk.view(n, h, w, NF), NF, *self.w["upconv1"], slope=0.2, up2x=True)
        self._tap("up1", up1.view(n, 2 * h, 2 * w, NF))
        up2 = ops.conv3x3_dense(up1.view(n, 2 * h, 2 * w, NF), NF, *self.w["upconv2"], slope=0.2, up2x=True)
        self._tap("up2", up2.view(n, 4 * h, 4 * w, NF))
        hr = ops.conv3x3_dense(up2.view(n, 4 * h, 4 * w, NF), NF, *self.w["HRconv"], slope=0.2)
        self._tap("hr", hr.view(n, 4 * h, 4 * w, NF))
        y = ops.conv3x3_narrow(hr.view(n, 4 * h, 4 * w, NF), *self.w["conv_last"], 3)                # [16 m, 4], column 3 zeros
        self._tap("last", y.view(n, 4 * h, 4 * w, 4)[..., :3])
        bad = ops.count_nonfinite(y, cnt=ops.empty((1,), torch.int32))
        if bad:
            raise RuntimeError(f"ESRGAN model '{self.name}': the fp16 network output holds {bad} non-finite values (the model's activations leave fp16's "
                               "range); no image is returned")
        return ops.esrgan_unpack_image(y).view(n, 4 * h, 4 * w, 3)
