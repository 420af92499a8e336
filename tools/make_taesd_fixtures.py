"""TEST INFRASTRUCTURE ONLY.  Generates tests/golden/taesd.pt and tests/golden/taesd_weights_*.pt with the REAL reference's TAESD module
(<reference>/modules/sd_vae_taesd.py and sd_vae_approx.py, imported at run time by file path; nothing of them is copied).  Deterministic (seeded).

    python tools/make_taesd_fixtures.py --reference /path/to/reference [--out tests/golden]

The reference modules import `modules.devices / paths / paths_internal / shared`; those entries of sys.modules are stubbed (the network itself needs
none of them), and the stubs are removed again.

Writes
  taesd_weights_<i>.pt   the state dict of ONE `decoder(4)` as fp16 (every value fp16-representable: the fp32 reference runs on exactly these numbers),
                         its keys split over files so that no committed file is above 1 MiB
  taesd.pt               weight_parts; first16.weight / first16.bias (the first layer of a 16-channel decoder sharing every other layer);
                         cases[name] = latent (4 N(0,1): the clamp is exercised), out (the reference's fp32 `decoder(x)`), floor_rms / floor_max_rel /
                         floor_max_abs per element type (the reference module's OWN fp16 / bf16 CPU run, `copy.deepcopy(d).to(dtype)`, against its fp32
                         run), image_u8 (sample 0 as uint8 HWC); rgb_factors ([4][3], random) and rgb_out (the reference's cheap_approximation einsum)
Weights: convolutions directly followed by ReLU N(0, 2 / fan_in), the others N(0, 1 / fan_in), biases 0.1 N(0, 1); the last convolution is then
rescaled and its bias moved so that at least 90 % of the reference output lies in (0.02, 0.98) -- asserted: the uint8 tail cannot be tested on a
saturated image.
image_u8: modules/sd_samplers_common.py imports the web UI (images, sd_samplers, sd_models, modules_forge, ...) and does not import under stubs, so
what is recorded is the result of its five torch lines (:71-78 behind the `* 2 - 1` of :61), restated here.
"""
import argparse
import copy
import importlib.util
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"l4": (2, 4, 6, 10), "l16": (1, 16, 8, 8)}
STUBS = ("modules", "modules.devices", "modules.paths", "modules.paths_internal", "modules.shared")


def import_reference(reference):
    saved = {k: sys.modules.get(k) for k in STUBS}
    pkg = types.ModuleType("modules")
    pkg.__path__ = []
    sys.modules["modules"] = pkg
    for name in STUBS[1:]:
        m = types.ModuleType(name)
        sys.modules[name] = m
        setattr(pkg, name.split(".")[1], m)
    sys.modules["modules.devices"].device = torch.device("cpu")
    sys.modules["modules.devices"].dtype = torch.float32
    sys.modules["modules.paths_internal"].models_path = sys.modules["modules.paths"].models_path = os.path.join(reference, "models")
    sys.modules["modules.paths"].script_path = reference
    out = []
    try:
        for fn in ("sd_vae_taesd.py", "sd_vae_approx.py"):
            spec = importlib.util.spec_from_file_location("_ref_" + fn[:-3], os.path.join(reference, "modules", fn))
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            out.append(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return out + [sys.modules.get("modules.shared") or None]


def init_weights(net, g):
    followed_by_relu = set()
    mods = list(net.named_modules())
    for name, m in mods:
        if isinstance(m, torch.nn.Sequential):
            ch = list(m.named_children())
            for (n0, a), (_, b) in zip(ch, ch[1:]):
                if isinstance(a, torch.nn.Conv2d) and isinstance(b, torch.nn.ReLU):
                    followed_by_relu.add((name + "." if name else "") + n0)
    for name, m in mods:
        if isinstance(m, torch.nn.Conv2d):
            fan_in = m.weight.shape[1] * 9
            var = (2.0 if name in followed_by_relu else 1.0) / fan_in
            with torch.no_grad():
                m.weight.copy_((torch.randn(m.weight.shape, generator=g) * var ** 0.5).half().float())
                if m.bias is not None:
                    m.bias.copy_((0.1 * torch.randn(m.bias.shape, generator=g)).half().float())


def image_u8(x01):
    x = (x01 * 2 - 1) * 0.5 + 0.5          # sd_samplers_common.py:61 and :71
    x = x.cpu()
    x.clamp_(0.0, 1.0)
    x.mul_(255.)
    x.round_()
    return x.to(torch.uint8).permute(1, 2, 0).contiguous()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="checkout of the reference project (its modules/sd_vae_taesd.py is imported)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    taesd, approx, _ = import_reference(a.reference)
    g = torch.Generator().manual_seed(20261017)
    d4 = taesd.decoder(4).eval()
    init_weights(d4, g)
    d16 = taesd.decoder(16).eval()
    init_weights(d16, g)
    sd = d4.state_dict()
    d16.load_state_dict({**sd, "1.weight": d16.state_dict()["1.weight"], "1.bias": d16.state_dict()["1.bias"]})
    nets = {"l4": d4, "l16": d16}
    lat = {k: 4.0 * torch.randn(s, generator=g) for k, s in CASES.items()}

    with torch.no_grad():
        for k, net in nets.items():       # the depth keeps its scale (fp16 range, no dead network)
            x = lat[k]
            for i, m in enumerate(net):
                x = m(x)
                rms, mx = float(x.pow(2).mean().sqrt()), float(x.abs().max())
                assert 0.5 < rms < 20 and mx < 200, (k, i, rms, mx)
        raw = torch.cat([nets[k](lat[k]).reshape(-1) for k in CASES])
        # last layer: output = 0.5 + 0.2 * standardised  ->  +-2.4 sigma inside (0.02, 0.98)
        s, mu = 0.2 / float(raw.std()), float(raw.mean())
        w19 = (d4[19].weight * s).half().float()
        b19 = ((d4[19].bias - mu) * s + 0.5).half().float()
        for net in nets.values():
            net[19].weight.copy_(w19)
            net[19].bias.copy_(b19)
        sd = d4.state_dict()
        assert all(bool((v.half().float() == v).all()) for v in sd.values()) and len(sd) == 67
        cases = {}
        for k, net in nets.items():
            out = net(lat[k])
            inside = float(((out > 0.02) & (out < 0.98)).float().mean())
            assert inside >= 0.9, (k, inside)
            c = {"latent": lat[k], "out": out, "image_u8": image_u8(out[0])}
            for dt, nm in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
                lo = copy.deepcopy(net).to(dt)(lat[k].to(dt)).double()
                dd = lo - out.double()
                c[nm] = {"floor_rms": float(dd.pow(2).mean().sqrt() / out.double().pow(2).mean().sqrt()),
                         "floor_max_rel": float(dd.abs().max() / out.abs().max()), "floor_max_abs": float(dd.abs().max())}
            print(k, tuple(out.shape), f"inside (0.02, 0.98): {inside:.3f}", c["fp16"], c["bf16"])
            cases[k] = c
        fac = torch.randn(4, 3, generator=g)
        rgb = torch.einsum("...lxy,lr -> ...rxy", lat["l4"], fac)      # sd_vae_approx.py:74 with a table of our own (the real ones live in huggingface_guess)

    keys = list(sd)
    parts, cur, size = [], {}, 0
    for k in keys:
        nbytes = sd[k].numel() * 2
        if cur and size + nbytes > 900_000:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = sd[k].half().clone()
        size += nbytes
    parts.append(cur)
    for i, p in enumerate(parts):
        torch.save(p, os.path.join(a.out, f"taesd_weights_{i}.pt"))
    torch.save({"weight_parts": len(parts), "first16.weight": d16.state_dict()["1.weight"].half().clone(), "first16.bias": d16.state_dict()["1.bias"].half().clone(),
                "cases": cases, "rgb_factors": fac, "rgb_out": rgb}, os.path.join(a.out, "taesd.pt"))
    print("wrote", len(parts), "weight parts and taesd.pt to", a.out)


if __name__ == "__main__":
    main()
