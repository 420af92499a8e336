#!/usr/bin/env python
"""The native ESRGAN upscaler (forge_amd.backend.nn.esrgan.RRDBNet) next to the same network as plain torch convolutions in fp16 and in fp32 (fp32 is
what the reference runs: load_spandrel_model(prefer_half=False)) on the same GPU; one JSON line per leg, appended to --out.

    python tools/bench_esrgan.py --leg native|torch_fp16|torch_fp32|hires [--images 8] [--res 1024] [--nb 23] [--out profiles/esrgan_native_vs_torch.jsonl]

Workload: nb 23 synthetic weights (tests/esrgan_refs.seeded_state_dict at ESRGAN's init scale, which keeps 69 dense blocks inside fp16's range),
--images images of --res^2 split into 192 / 8 tiles by modules/images.split_grid (6 x 6 tiles at 1024^2).  A repetition times the network on the
tiles of the images (host -> device copy of the uint8 tiles and device -> host copy of the uint8 result included, as in use), wall clock between
device synchronisations; warm-up first, then the median of --reps.  The torch legs run the tiles in groups of the native leg's size, on ONE
image per repetition (they are several times slower; per-image figures compare directly).  One leg per process: a leg that a library's kernel
search makes too slow can be dropped without losing the others.
FLOP figure: 2 x the MACs of the network on the tiles' pixels -- 33.1 MFLOP per input pixel in the trunk at nb 23, the two x2 stages, HRconv and
conv_last on top (about 47 TFLOP per 1024^2 image).
--leg native also brackets every launch of ONE group with device events (hipops.KernelProfiler) and reports the dense kernel's share by cin.
--leg hires: an SDXL-shaped synthetic engine, txt2img 1024^2 -> 2048^2 at batch --images with the model registered as hires upscaler; wall-clock
seconds in decode / upscale / encode / second pass."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import conftest  # noqa: F401,E402  (registers the package alias)
import forge_amd  # noqa: E402,F401
import esrgan_refs as E  # noqa: E402
from forge_amd import hipops as ops  # noqa: E402
from forge_amd.backend.nn.esrgan import RRDBNet  # noqa: E402
from forge_amd.modules import images, shared  # noqa: E402


def network_flop(nb, npix):
    rdb = 9 * (64 + 96 + 128 + 160) * 32 + 9 * 192 * 64
    per_px = 9 * 64 * 64 + nb * 3 * rdb + 9 * 64 * 64 + 4 * 9 * 64 * 64 + 16 * 9 * 64 * 64 * 2 + 16 * 9 * 64 * 3      # conv_first zero-padded to 64
    return 2.0 * per_px * npix


def image_tiles(n, res):
    from PIL import Image
    out = []
    for i in range(n):
        grid = images.split_grid(Image.fromarray(E.test_image(res, res, seed=i).numpy(), "RGB"), shared.opts.ESRGAN_tile, shared.opts.ESRGAN_tile,
                                 shared.opts.ESRGAN_tile_overlap)
        out.append(torch.from_numpy(np.stack([np.array(t) for _, _, row in grid.tiles for _, _, t in row])))
    return out


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=["native", "torch_fp16", "torch_fp32", "hires"])
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--nb", type=int, default=23)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "esrgan_native_vs_torch.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    sd = E.seeded_state_dict(a.nb, seed=0, rdb_scale=0.1)
    row = {"leg": a.leg, "nb": a.nb, "res": a.res, "tile": shared.opts.ESRGAN_tile, "overlap": shared.opts.ESRGAN_tile_overlap, "device": torch.cuda.get_device_name(0)}
    if a.leg == "hires":
        row.update(hires_leg(a, sd, dev))
    else:
        tiles = image_tiles(a.images if a.leg == "native" else 1, a.res)
        per_image = tiles[0].shape[0]
        flop = network_flop(a.nb, per_image * tiles[0].shape[1] * tiles[0].shape[2])
        net = RRDBNet(sd, device=dev, name="bench")
        group = net.tiles_per_group(*tiles[0].shape[1:3])
        if a.leg == "native":
            batch = torch.cat(tiles)
            ms = timed(lambda: net.upscale(batch), a.reps)
            with ops.KernelProfiler() as prof:
                net._arena.reset()
                with net._arena:
                    net._forward(batch[:group])
            by = {}
            prof.summary()
            for (kind, tag), d in prof.by_tag.items():
                key = f"{kind} {tag}" if kind == "conv3x3_dense" else kind
                e = by.setdefault(key, {"launches": 0, "ms": 0.0, "tflop": 0.0})
                e["launches"] += d["launches"]
                e["ms"] += d["seconds"] * 1e3
                e["tflop"] += d["flops"] / 1e12
            total = sum(e["ms"] for e in by.values())
            row["one_group_kernels"] = {k: {"launches": e["launches"], "ms": round(e["ms"], 3), "share": round(e["ms"] / total, 4),
                                            "tflops": round(e["tflop"] / (e["ms"] * 1e-3), 1) if e["ms"] else None} for k, e in sorted(by.items())}
            row["one_group_tiles"] = group
            n_img = a.images
        else:
            dt = torch.float16 if a.leg == "torch_fp16" else torch.float32
            sdd = {k: v.to(dev, dt) for k, v in sd.items()}
            batch = tiles[0]

            def run():
                outs = []
                with torch.inference_mode():
                    for lo in range(0, batch.shape[0], group):
                        x = batch[lo:lo + group].to(dev).flip(-1).permute(0, 3, 1, 2).to(dt) / 255
                        y = E.forward(sdd, a.nb, x, compute=dt)
                        outs.append((y.float().clamp_(0, 1) * 255).round().to(torch.uint8).flip(1).permute(0, 2, 3, 1).cpu())
                return torch.cat(outs)
            ms = timed(run, a.reps)
            n_img = 1
        med = statistics.median(ms)
        row.update({"images_per_rep": n_img, "tiles_per_image": per_image, "tiles_per_group": group, "ms_per_rep": [round(v, 1) for v in ms],
                    "ms_per_image_median": round(med / n_img, 1), "ms_per_image_min_max": [round(min(ms) / n_img, 1), round(max(ms) / n_img, 1)],
                    "tflop_per_image": round(flop / 1e12, 2), "tflops": round(flop * n_img / (med * 1e-3) / 1e12, 1)})
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


def hires_leg(a, sd, dev):
    from forge_amd import synth
    from forge_amd.backend.diffusion_engine.base import build_engine
    from forge_amd.backend.nn.layout import unet_param_shapes, vae_decoder_param_shapes, vae_encoder_param_shapes
    from forge_amd.modules import esrgan_model, processing, prompt_parser as pp, sd_samplers_common, upscaler
    cfg, vcfg = synth.SDXL_UNET_CONFIG, synth.SDXL_VAE_CONFIG
    vshapes = dict(vae_decoder_param_shapes(vcfg))
    vshapes.update(vae_encoder_param_shapes(vcfg))
    eng = build_engine(cfg, synth.synth_state_dict_device(unet_param_shapes(cfg), 0, dev), vcfg, synth.synth_state_dict_device(vshapes, 1, dev), device=dev)
    b = a.images
    c, uc = synth.synth_conditioning(b, cfg["context_dim"], cfg["adm_in_channels"], seed=1234)
    half = lambda t: pp.DictWithShape({k: v.to(dev).half() for k, v in t.items()})
    shared.opts.randn_source = "CPU"
    shared.sd_model = eng
    scaler = esrgan_model.UpscalerESRGAN()
    esrgan_model._models["bench"] = RRDBNet(sd, device=dev, name="bench")
    shared.sd_upscalers[:] = [upscaler.UpscalerData("bench-esrgan", "bench", scaler, 4)]
    spent = {}

    def clocked(name, fn):
        def wrapper(*args, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*args, **kw)
            torch.cuda.synchronize()
            spent[name] = spent.get(name, 0.0) + time.perf_counter() - t0
            return out
        return wrapper
    processing.decode_first_stage = clocked("decode", processing.decode_first_stage)
    sd_samplers_common.images_tensor_to_samples = clocked("encode", sd_samplers_common.images_tensor_to_samples)
    cls = processing.StableDiffusionProcessingTxt2Img
    cls.upscale_decoded = clocked("upscale (ESRGAN tiles + host grid + LANCZOS)", cls.upscale_decoded)
    cls.sample_hr_pass = clocked("hr pass total", cls.sample_hr_pass)
    out = {}
    for rep in ("warm", "timed"):
        spent.clear()
        p = cls(sd_model=eng, c=half(c), uc=half(uc), seed=1, sampler_name="Euler", batch_size=b, steps=2, cfg_scale=7.0, width=a.res, height=a.res,
                do_decode=False, enable_hr=True, hr_scale=2, hr_upscaler="bench-esrgan", hr_second_pass_steps=4, denoising_strength=0.5, hr_cfg=7.0)
        lat = processing.process_images(p).latents
        out = {"batch": b, "hr_steps_run": "4 x 0.5", "latent": list(lat.shape), "finite": bool(torch.isfinite(lat).all()),
               "seconds": {k: round(v, 3) for k, v in spent.items()}}
        out["seconds"]["second pass (sampler)"] = round(spent["hr pass total"] - sum(v for k, v in spent.items() if k != "hr pass total"), 3)
    return out


if __name__ == "__main__":
    main()
