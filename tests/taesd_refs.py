"""fp64 restatement of the TAESD decoder (reference modules/sd_vae_taesd.py:16-44) from a state dict, for tests/test_taesd_host.py and
tests/test_gpu_taesd.py.  One table of layers serves the whole-network run and the teacher-forced per-layer run.

`dtype` (None / torch.float16 / torch.bfloat16) rounds at exactly the tensors the native executor stores (forge_amd/backend/nn/taesd.py): the latent
on entry, the clamped latent, every conv (+ residual) (+ ReLU) output; weights and biases are rounded to it once.  None rounds nowhere: that form
reproduces the reference's own fp32 output (pinned by tests/test_taesd_host.py against tests/golden/taesd.pt).
`plant` breaks one thing, for the teeth tests: "relu_before_add" (Block 9: relu(conv) + x instead of relu(conv + x)), "up_round" (the Upsample
reads source index (Y + 1) >> 1 instead of Y >> 1), "no_clamp" (the tanh clamp left out)."""
import os

import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BLOCKS = ((3, 4, 5), (8, 9, 10), (13, 14, 15), (18,))
UPS = (7, 12, 17)
PLANTS = ("relu_before_add", "up_round", "no_clamp")


def load_fixture():
    """tests/golden/taesd.pt plus the decoder's state dict, which is split over taesd_weights_*.pt (no committed file above 1 MiB)"""
    fx = torch.load(os.path.join(GOLDEN, "taesd.pt"), weights_only=True)
    sd = {}
    for i in range(fx["weight_parts"]):
        sd.update(torch.load(os.path.join(GOLDEN, f"taesd_weights_{i}.pt"), weights_only=True))
    fx["state_dict"] = sd
    return fx


def state_dict_for(fx, latent_channels):
    sd = dict(fx["state_dict"])
    if latent_channels == 16:
        sd["1.weight"], sd["1.bias"] = fx["first16.weight"], fx["first16.bias"]
    return sd


def layers():
    """(key of the stored output, key of the input, weight prefix, has bias, key of the residual or None, relu, up2x), in execution order; "0" is the
    clamped latent"""
    out, prev = [("1", "0", "1", True, None, True, False)], "1"
    for level, blocks in enumerate(BLOCKS):
        for i in blocks:
            out.append((f"{i}.conv.0", prev, f"{i}.conv.0", True, None, True, False))
            out.append((f"{i}.conv.2", f"{i}.conv.0", f"{i}.conv.2", True, None, True, False))
            out.append((str(i), f"{i}.conv.2", f"{i}.conv.4", True, prev, True, False))
            prev = str(i)
        if level < len(UPS):
            out.append((str(UPS[level]), prev, str(UPS[level]), False, None, False, True))
            prev = str(UPS[level])
    out.append(("19", prev, "19", True, None, False, False))
    return out


def _rnd(t, dtype):
    return t if dtype is None else t.to(dtype).to(t.dtype)


def clamp_ref(z, dtype=None, plant=None, compute=torch.float64):
    """stored tensor "0": NCHW in the `compute` type (fp64; fp32 only to meet the reference's own fp32 run on its own terms)"""
    x = _rnd(z.to(compute), dtype)
    return x if plant == "no_clamp" else _rnd(torch.tanh(x / 3) * 3, dtype)


def upsample_ref(x, plant=None):
    if plant != "up_round":
        return x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    h, w = x.shape[2], x.shape[3]
    iy = ((torch.arange(2 * h) + 1) >> 1).clamp_max(h - 1)
    ix = ((torch.arange(2 * w) + 1) >> 1).clamp_max(w - 1)
    return x[:, :, iy][:, :, :, ix]


def layer_ref(sd, spec, x, residual=None, dtype=None, plant=None, exact=False):
    """one row of layers() on fp64 NCHW inputs -> the stored output (rounded to dtype unless exact), fp64 NCHW"""
    key, _, wk, has_bias, res_key, relu, up = spec
    if up:
        x = upsample_ref(x, plant)
    y = F.conv2d(x, _rnd(sd[wk + ".weight"].to(x.dtype), dtype), _rnd(sd[wk + ".bias"].to(x.dtype), dtype) if has_bias else None, padding=1)
    if res_key is not None:
        if plant == "relu_before_add" and key == "9":
            y, relu = torch.relu(y) + residual, False
        else:
            y = y + residual
    if relu:
        y = torch.relu(y)
    return y if exact else _rnd(y, dtype)


def decode_ref(sd, z, dtype=None, plant=None, taps=None, compute=torch.float64):
    """the whole decoder: fp32 NCHW latent -> NCHW [B, 3, 8h, 8w] in the `compute` type (fp64); taps (a dict) receives every stored tensor"""
    t = {"0": clamp_ref(z, dtype, plant, compute)}
    for spec in layers():
        t[spec[0]] = layer_ref(sd, spec, t[spec[1]], t[spec[4]] if spec[4] else None, dtype, plant)
    if taps is not None:
        taps.update(t)
    return t["19"]


def image_tail(x01):
    """modules/sd_samplers_common.py:61,71-78 on the network output of ONE sample ([3, H, W], about [0, 1]) -> uint8 [H, W, 3]"""
    x = (x01.float() * 2 - 1) * 0.5 + 0.5
    x = x.cpu().clamp(0.0, 1.0).mul(255.0).round().to(torch.uint8)
    return x.permute(1, 2, 0).contiguous()


def network_bar(got, ref, floor):
    """the bars of tests/parity.py with the fixture's floors -> (metrics, limits, names of the metrics over their limit)"""
    import parity
    d = got.double() - ref.double()
    m = {"rms": float(d.pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt()), "max_rel": float(d.abs().max() / ref.double().abs().max())}
    lim = {"rms": parity.RMS_FACTOR * floor["floor_rms"], "max_rel": max(parity.NORTH_STAR, parity.MAX_FACTOR * floor["floor_max_rel"])}
    return m, lim, [k for k in lim if not m[k] <= lim[k]]
