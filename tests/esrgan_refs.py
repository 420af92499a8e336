"""RRDBNet (the ESRGAN family: nf 64, gc 32, two x2 stages) restated in torch from a "new arch" state dict, for tests/test_esrgan_host.py and
tests/test_gpu_esrgan.py.

Three forms of one forward, on a BGR image batch NCHW in [0, 1]:
  * forward(sd, nb, x)                         fp64 everywhere, no rounding: the yardstick;
  * forward(sd, nb, x, sites=True)             fp64 arithmetic, rounded to fp16 exactly where the native executor (forge_amd/backend/nn/esrgan.py) stores:
                                               the packed image, conv_first, every x_k of a dense block, every dense block's output (conv5 with its
                                               fused 0.2 * f + x; the third block of an RRDB also takes 0.2 * (.) + RRDB input in the SAME rounding),
                                               trunk_conv + fea, both upsample convolutions, HRconv, conv_last; weights and biases rounded once;
  * forward(sd, nb, x, compute=torch.float16)  plain torch fp16 modules' arithmetic on the CPU (every op rounds): the fp16 floor of the parity rule.
`plant` breaks one thing, for the teeth tests: "slope" (LeakyReLU 0.1 in the dense blocks), "no_scale" (the 0.2 on conv5 dropped), "rgb" (the image fed as
RGB instead of BGR -- plant it on the input with `to_bgr01(img, rgb=True)`).

Weights are seeded (nothing large is committed): kaiming-normal (fan-in) in the dense blocks, 0.7 x that in the other convolutions (0.21 x in
conv_last, its bias at mid-grey: the image then spans levels 38 .. 145 without saturating), small random biases so that a dropped bias shows.  ESRGAN's own
INIT scale for the dense blocks is kaiming x 0.1 (BasicSR default_init_weights(scale=0.1)), but at that scale the blocks contribute next to nothing and a
wrong LeakyReLU slope moves the output by 0.8 x the end-to-end gate (measured on the CPU, as 0.3 x and 0.5 x: 0.8 and 1.2) -- a network no test could
tell from a broken one; trained ESRGAN weights are an order of magnitude above their init, and at kaiming x 1 the slope plant is 5.5 x the gate."""
import math

import numpy as np
import torch
import torch.nn.functional as F

NF, GC = 64, 32
PLANTS = ("slope", "no_scale", "rgb")


def conv_names(nb):
    names = ["conv_first"]
    for i in range(nb):
        for r in (1, 2, 3):
            names += [f"RRDB_trunk.{i}.RDB{r}.conv{j}" for j in range(1, 6)]
    return names + ["trunk_conv", "upconv1", "upconv2", "HRconv", "conv_last"]


def conv_shape(name):
    if ".RDB" in name:
        j = int(name[-1])
        return (GC if j < 5 else NF, NF + GC * (j - 1))
    return {"conv_first": (NF, 3), "conv_last": (3, NF)}.get(name, (NF, NF))


def seeded_state_dict(nb, seed=0, rdb_scale=1.0):
    """rdb_scale: the dense blocks' factor on kaiming-normal (tools/bench_esrgan.py runs 23 blocks at ESRGAN's init scale 0.1, which keeps fp16's range)"""
    g = torch.Generator("cpu").manual_seed(seed)
    sd = {}
    for name in conv_names(nb):
        co, ci = conv_shape(name)
        std = math.sqrt(2.0 / (9 * ci)) * (rdb_scale if ".RDB" in name else 0.21 if name == "conv_last" else 0.7)
        sd[name + ".weight"] = torch.randn(co, ci, 3, 3, generator=g) * std
        sd[name + ".bias"] = torch.randn(co, generator=g) * 0.02
    sd["conv_last.bias"] = sd["conv_last.bias"] + 0.5
    return sd


def relayout(sd, nb, layout):
    """the same tensors under the "old" (model.N...) or "real" (Real-ESRGAN, wrapped in params_ema) key layout"""
    out = {}
    old = {"conv_first": "model.0", "trunk_conv": f"model.1.sub.{nb}", "upconv1": "model.3", "upconv2": "model.6", "HRconv": "model.8", "conv_last": "model.10"}
    real = {"trunk_conv": "conv_body", "upconv1": "conv_up1", "upconv2": "conv_up2", "HRconv": "conv_hr"}
    for k, v in sd.items():
        stem, leaf = k.rsplit(".", 1)
        if stem.startswith("RRDB_trunk."):
            _, i, rdb, conv = stem.split(".")
            stem = f"model.1.sub.{i}.{rdb}.{conv}.0" if layout == "old" else f"body.{i}.{rdb.lower()}.{conv}"
        else:
            stem = old[stem] if layout == "old" else real.get(stem, stem)
        out[f"{stem}.{leaf}"] = v
    return out if layout == "old" else {"params_ema": out}


def test_image(w, h, seed=0):
    """uint8 RGB [h, w, 3]: smooth gradients plus noise, every channel different"""
    g = torch.Generator("cpu").manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    base = torch.stack([xx / w, yy / h, 1 - (xx + yy) / (w + h)], dim=2) * 200 + 20
    return (base + torch.randn(h, w, 3, generator=g) * 12).clamp(0, 255).to(torch.uint8)


def to_bgr01(img_u8, rgb=False):
    """modules/upscaler_utils.py:14-19: uint8 RGB [n, h, w, 3] -> float64 BGR NCHW in [0, 1]"""
    a = img_u8.numpy() if rgb else img_u8.numpy()[..., ::-1]
    return torch.from_numpy(np.ascontiguousarray(np.moveaxis(a, 3, 1)) / 255)


def to_image(y):
    """modules/upscaler_utils.py:31-34 on a batch: BGR NCHW -> uint8 RGB [n, h, w, 3]"""
    arr = 255.0 * np.moveaxis(y.float().cpu().clamp_(0, 1).numpy(), 1, 3)
    return torch.from_numpy(np.ascontiguousarray(arr.round().astype(np.uint8)[..., ::-1]))


def _r16(t, on):
    return t.to(torch.float16).to(t.dtype) if on else t


def conv(sd, name, x, sites=False):
    return F.conv2d(x, _r16(sd[name + ".weight"].to(x.dtype), sites), _r16(sd[name + ".bias"].to(x.dtype), sites), padding=1)


def rdb_ref(sd, prefix, x, sites=False, plant=None, rrdb_in=None, exact=False, taps=None):
    """one dense block -> x + 0.2 * conv5(...); with rrdb_in (the RRDB's third block): 0.2 * (that) + rrdb_in, ONE rounding in the sites form.
    taps (a list) receives [x1, x2, x3, x4] as stored."""
    slope = 0.1 if plant == "slope" else 0.2
    feats = [x]
    for j in range(1, 5):
        feats.append(_r16(F.leaky_relu(conv(sd, f"{prefix}.conv{j}", torch.cat(feats, 1), sites), slope), sites))
    if taps is not None:
        taps.extend(feats[1:])
    y = conv(sd, f"{prefix}.conv5", torch.cat(feats, 1), sites)
    y = (y if plant == "no_scale" else 0.2 * y) + x
    if rrdb_in is not None:
        if not sites and x.dtype == torch.float16:
            y = y * 0.2 + rrdb_in            # plain fp16 modules: the block's output was already rounded by the tensor type
        else:
            y = 0.2 * y + rrdb_in
    return y if exact else _r16(y, sites)


def up2(x):
    return x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def forward(sd, nb, x, sites=False, plant=None, compute=torch.float64, taps=None):
    """BGR NCHW in [0, 1] (float64, as to_bgr01 gives it) -> conv_last's output NCHW in the compute type; taps (a dict) receives the stored tensors"""
    t = {}
    x = x.to(torch.float16).to(compute) if (sites or compute == torch.float16) else x.to(compute)
    t["pack"] = x
    fea = t["conv_first"] = _r16(conv(sd, "conv_first", x, sites), sites)
    cur = fea
    for i in range(nb):
        rin = cur
        for r in (1, 2, 3):
            cur = t[f"{i}.{r}"] = rdb_ref(sd, f"RRDB_trunk.{i}.RDB{r}", cur, sites, plant, rrdb_in=rin if r == 3 else None)
    y = t["trunk"] = _r16(conv(sd, "trunk_conv", cur, sites) + fea, sites)
    y = t["up1"] = _r16(F.leaky_relu(conv(sd, "upconv1", up2(y), sites), 0.2), sites)
    y = t["up2"] = _r16(F.leaky_relu(conv(sd, "upconv2", up2(y), sites), 0.2), sites)
    y = t["hr"] = _r16(F.leaky_relu(conv(sd, "HRconv", y, sites), 0.2), sites)
    y = t["last"] = _r16(conv(sd, "conv_last", y, sites), sites)
    if taps is not None:
        taps.update(t)
    return y


def metrics(got, ref):
    d = got.double() - ref.double()
    return {"rms": float(d.pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt()), "max_rel": float(d.abs().max() / ref.double().abs().max())}


def gate(floor):
    """the project's floor rule (README "Parity", tests/parity.py): rms <= 1.25 x floor, max <= max(1e-3, 1.5 x floor)"""
    import parity
    return {"rms": parity.RMS_FACTOR * floor["rms"], "max_rel": max(parity.NORTH_STAR, parity.MAX_FACTOR * floor["max_rel"])}


def fp16_state_dict(sd):
    return {k: v.to(torch.float16) for k, v in sd.items()}
