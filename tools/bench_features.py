#!/usr/bin/env python
"""Full-size (SDXL 1024x1024, batch 8, fp16, CFG 7) timings of the widened paths, one JSON line each: every sampler family, ControlNet,
per-block hooks (eager path), FreeU (plain / native / hooked, interleaved), AND-composed prompts, hires-fix second pass.  Not the headline
bench (bench.py): this is the check that the §8f rows hold up at the BASELINE shape -- arena sizing, 32-bit offsets, graph capture with other
batch sizes -- and what they cost.

    python tools/bench_features.py [--steps 6] [--only samplers,controlnet,hooks,freeu,and,hires]
    python tools/bench_features.py --only dynthresh  Dynamic Thresholding: plain / native at percentile 1.0 and 0.99 / the same arithmetic as a Python
                                                     sampler_cfg_function, interleaved in one process, device events around every job
    python tools/bench_features.py --only kohya      Kohya HRFix: plain / native (transformer option, captured graph) / the same arithmetic as the
                                                     reference's Python patches (eager), interleaved in one process, device events around every job
    python tools/bench_features.py --only pag        Perturbed-Attention Guidance: plain / native (third group of rows in the captured graph) / the same
                                                     arithmetic as a Python post-CFG function with an attn1 replace patch (a second, eager model call),
                                                     interleaved in one process, device events around every job
    python tools/bench_features.py --only stylealign StyleAlign: plain / native at strength 1.0 and 0.5 (captured graph) / the reference's attn1 replace
                                                    patch at both strengths on the hooked executor, timed alternately in one process
    python tools/bench_features.py --only lllite     ControlNet-LLLite: plain / native (fused adapter kernel, captured graph) / the same unit as Python
                                                     attn1 / attn2 patches on the hooked executor, and the adapter launches on their own
    python tools/bench_features.py --only ipadapter  IP-Adapter: plain / native with a base file, a plus file and two units (dual attention kernel,
                                                     captured graph) / the composite route forced / the same units as Python attn2 replace patches
    python tools/bench_features.py --only clipvision CLIP-vision encode_image of 2 images at 512 x 768 on synthetic full-size ViT-H/14 and ViT-bigG/14: native against
                                                     transformers' CLIPVisionModelWithProjection in fp16 on the same GPU; the routes are primed, then timed alternately
                                                     in one process, median of 5 -> profiles/clipvision_native_vs_torch.jsonl (--out), with the share of the two new kernels
    python tools/bench_features.py --only taesd      the TAESD decode of batch x (res/8)^2 SDXL-shaped latents (synthetic weights, fp16) next to the Full
                                                     VAE decode of the same latents in the same process: median of 5 after warm-up, events around the calls
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import conftest  # noqa: F401,E402  (registers the package alias)
import forge_amd  # noqa: E402
from forge_amd import synth  # noqa: E402
from forge_amd.backend.diffusion_engine.base import build_engine  # noqa: E402
from forge_amd.backend.nn.layout import controlnet_param_shapes, unet_param_shapes  # noqa: E402
from forge_amd.modules import processing, prompt_parser as pp, shared  # noqa: E402


def taesd_leg(batch, width, height, dev):
    from forge_amd.backend.nn.layout import vae_decoder_param_shapes
    from forge_amd.backend.nn.taesd import TAESDDecoder, expected_keys
    from forge_amd.backend.nn.vae import IntegratedAutoencoderKL
    g = torch.Generator("cpu").manual_seed(5)
    sd = {}
    for k in expected_keys():     # He-scaled: the depth keeps its scale in fp16
        shape = (64,) if k.endswith("bias") else (3 if k.startswith("19.") else 64, 4 if k == "1.weight" else 64, 3, 3)
        sd[k] = torch.randn(shape, generator=g) * (0.1 if k.endswith("bias") else (2.0 / (shape[1] * 9)) ** 0.5)
    tae = TAESDDecoder(sd, device=dev, dtype=torch.float16)
    vcfg = synth.SDXL_VAE_CONFIG
    vae = IntegratedAutoencoderKL(vcfg, synth.synth_state_dict_device(vae_decoder_param_shapes(vcfg), 1, dev), device=dev)
    z = torch.randn(batch, 4, height // 8, width // 8, generator=g).to(dev)

    def timed(fn):
        for _ in range(2):
            out = fn()
        ms = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return sorted(ms)[2], out
    t_ms, img = timed(lambda: tae.decode(z))
    f_ms, full = timed(lambda: vae.decode(vae.process_out(z)))
    print(json.dumps({"case": "TAESD decode vs Full VAE decode", "latent": list(z.shape), "dtype": "f16", "taesd_ms": round(t_ms, 3), "full_ms": round(f_ms, 3),
                      "full_over_taesd": round(f_ms / t_ms, 2), "finite": bool(torch.isfinite(img).all() and torch.isfinite(full).all()),
                      "taesd_out": list(img.shape)}), flush=True)


def clipvision_leg(dev, out_path, images=2, height=512, width=768):
    """encode_image, native against transformers in fp16, on synthetic full-size towers (module docstring)"""
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    from forge_amd import hipops as ops
    from forge_amd.backend.patcher import clipvision as cv
    g = torch.Generator(device=dev).manual_seed(11)
    image = torch.rand(images, height, width, 3, generator=g, device=dev)
    mean, std = (torch.tensor(v, device=dev).view(3, 1, 1) for v in ((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)))

    def torch_preprocess(img):
        x = img.movedim(-1, 1)
        rh, rw, top, left = cv.preprocess_geometry(x.shape[2], x.shape[3])
        x = torch.nn.functional.interpolate(x, size=(rh, rw), mode="bicubic", antialias=True)[:, :, top:top + 224, left:left + 224]
        return ((torch.clip(255.0 * x, 0, 255).round() / 255.0 - mean) / std).half()

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    lines = []
    for family, cfg in (("ViT-H/14", cv.CLIP_VISION_H), ("ViT-bigG/14", cv.CLIP_VISION_G)):
        sd = {}
        for name, shape in synth.clip_vision_param_shapes(cfg).items():
            z = torch.randn(shape, generator=g, device=dev)
            if "norm" in name:
                z = 1.0 + 0.1 * z if name.endswith(".weight") else 0.1 * z
            elif "class_embedding" in name or "position_embedding" in name:
                z = 0.5 * z
            else:
                fan = shape if not name.endswith(".bias") else synth.clip_vision_param_shapes(cfg)[name[:-5] + ".weight"]
                z = z * (float(synth.DEFAULT_GAIN) / float(torch.tensor(fan[1:]).prod()) ** 0.5)
            sd[name] = z.half()
        native = cv.ClipVisionModel(cfg, sd, dev)
        with torch.device(dev):
            ref = CLIPVisionModelWithProjection(CLIPVisionConfig(**{k: v for k, v in cfg.items()})).half().eval()
        ref.load_state_dict(sd, strict=False)
        del sd
        routes = {"native": lambda: native.encode_image(image).image_embeds,
                  "torch_fp16": lambda: ref(pixel_values=torch_preprocess(image), output_hidden_states=True).image_embeds.float()}
        with torch.inference_mode():
            outs = {k: [fn() for _ in range(2)][-1] for k, fn in routes.items()}          # primed
            ms = {k: [] for k in routes}
            for _ in range(5):
                for k, fn in routes.items():                                              # alternately
                    ms[k].append(event_ms(fn)[0])
            x, top, left = cv.resized(image)
            rows = ops.clip_patch_rows(x, top, left)
            patches = ops.linear(rows, native.tower.w["patch"])
            w = native.tower.w
            k1 = sorted(event_ms(lambda: ops.clip_patch_rows(x, top, left))[0] for _ in range(5))[2]
            k2 = sorted(event_ms(lambda: ops.clip_embed_ln(patches, w["class"], w["pos"], *w["pre"], rows_per_image=320))[0] for _ in range(5))[2]
        med = {k: sorted(v)[2] for k, v in ms.items()}
        d = (outs["native"].double() - outs["torch_fp16"].double())
        lines.append({"case": "clip-vision encode_image", "family": family, "images": images, "size": [height, width], "dtype": "f16", "native_ms": round(med["native"], 3),
                      "torch_fp16_ms": round(med["torch_fp16"], 3), "torch_over_native": round(med["torch_fp16"] / med["native"], 2),
                      "clip_patch_rows_ms": round(k1, 4), "clip_embed_ln_ms": round(k2, 4), "new_kernels_share_of_native": round((k1 + k2) / med["native"], 4),
                      "native_vs_torch_rms_rel": float(d.pow(2).mean().sqrt() / outs["torch_fp16"].double().pow(2).mean().sqrt()),
                      "finite": bool(torch.isfinite(outs["native"]).all()), "src": __import__("forge_amd")._lib.build_info()["src"]})
        print(json.dumps(lines[-1]), flush=True)
        del native, ref, routes, outs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.writelines(json.dumps(ln) + "\n" for ln in lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--height", type=int, default=0)
    ap.add_argument("--only", default="samplers,controlnet,hooks,freeu,and,hires")
    ap.add_argument("--pag-routes", default="plain,pag_native,pag_python", help="the routes of --only pag (one route alone for a kernel trace of it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clipvision_native_vs_torch.jsonl"), help="where --only clipvision writes its lines")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if "clipvision" in a.only.split(","):
        clipvision_leg(dev, a.out)
        if a.only == "clipvision":
            return
    width, height = a.width or a.res, a.height or a.res
    if "taesd" in a.only.split(","):
        taesd_leg(a.batch, width, height, dev)
        if a.only == "taesd":
            return
    cfg = synth.SDXL_UNET_CONFIG
    eng = build_engine(cfg, synth.synth_state_dict_device(unet_param_shapes(cfg), 0, dev), None, None, device=dev)
    b = a.batch
    c, uc = synth.synth_conditioning(2 * b, cfg["context_dim"], cfg["adm_in_channels"], seed=1234)
    half = lambda t, lo, hi: pp.DictWithShape({k: v[lo:hi].to(dev).half() for k, v in t.items()})
    c1, c2, u1 = half(c, 0, b), half(c, b, 2 * b), half(uc, 0, b)
    shared.opts.randn_source = "CPU"
    what = set(a.only.split(","))

    def run(label, sampler="Euler", steps=a.steps, cond=None, unet=None, model_calls_per_step=1, **kw):
        saved = eng.forge_objects_after_applying_lora
        if unet is not None:
            eng.forge_objects_after_applying_lora = saved.shallow_copy()
            eng.forge_objects_after_applying_lora.unet = unet
        try:
            def once(n):
                p = processing.StableDiffusionProcessingTxt2Img(sd_model=eng, c=cond if cond is not None else c1, uc=u1, seed=1, sampler_name=sampler,
                                                                batch_size=b, steps=n, cfg_scale=7.0, width=width, height=height, do_decode=False, **kw)
                return processing.process_images(p).latents
            once(max(3, min(steps, 4)))  # priming (arena, caches, graph)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lat = once(steps)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        finally:
            eng.forge_objects_after_applying_lora = saved
            eng.forge_objects = saved.shallow_copy()
        ok = bool(torch.isfinite(lat).all())
        print(json.dumps({"case": label, "sampler": sampler, "steps": steps, "ms_per_step": round(dt / steps * 1e3, 2),
                          "ms_total": round(dt * 1e3, 1), "finite": ok, "shape": list(lat.shape)}), flush=True)

    def freeu_leg(rounds=5, preset="SDXL"):
        """Plain, native FreeU (transformer option, captured graph) and hooked FreeU (the same arithmetic as a Python output_block_patch:
        tests/freeu_refs.py's closed form in torch fp32, so no FFT library either; eager) -- primed once each, then timed alternately, `rounds`
        windows of a.steps steps per variant, in this one process.  Also the FreeU launches of one UNet call on their own (device events,
        median of 20), which is what the native route adds to a step."""
        import freeu_refs as fr
        from forge_amd import hipops as ops
        from forge_amd.backend.patcher import freeu as pf
        p = pf.PRESETS[preset]
        mc = cfg["model_channels"]
        scales = {4 * mc: (p.b1, p.s1), 2 * mc: (p.b2, p.s2)}

        def patch(h, hsp, to):
            sc = scales.get(h.shape[1])
            return (h, hsp) if sc is None else fr.freeu_ref(h, hsp, *sc, dtype=torch.float32)
        hooked = eng.forge_objects.unet.clone()
        hooked.set_model_output_block_patch(patch)
        variants = {"plain": None, "freeu_native": pf.patch_freeu_v2(eng.forge_objects.unet, *p), "freeu_hooked": hooked}
        shapes = []                       # (n, hh, ww, c_h, c_s) of every ops.freeu call of one UNet call
        real = ops.freeu
        ops.freeu = lambda h, s, *r: (shapes.append((*h.shape, s.shape[-1])), real(h, s, *r))[1]
        saved = eng.forge_objects_after_applying_lora

        def once(unet, n):
            if unet is not None:
                eng.forge_objects_after_applying_lora = saved.shallow_copy()
                eng.forge_objects_after_applying_lora.unet = unet
            try:
                pr = processing.StableDiffusionProcessingTxt2Img(sd_model=eng, c=c1, uc=u1, seed=1, sampler_name="Euler", batch_size=b, steps=n,
                                                                 cfg_scale=7.0, width=width, height=height, do_decode=False)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lat = processing.process_images(pr).latents
                torch.cuda.synchronize()
                return time.perf_counter() - t0, lat
            finally:
                eng.forge_objects_after_applying_lora = saved
                eng.forge_objects = saved.shallow_copy()
        try:
            for unet in variants.values():    # priming (arena, caches, graphs)
                once(unet, 4)
        finally:
            ops.freeu = real
        stop = next((i for i in range(1, len(shapes)) if shapes[i][1] < shapes[i - 1][1]), len(shapes))   # the resolution only grows within one call
        per_call = shapes[:stop]
        ms = {k: [] for k in variants}
        finite = True
        for _ in range(rounds):
            for k, unet in variants.items():
                dt, lat = once(unet, a.steps)
                ms[k].append(round(dt / a.steps * 1e3, 2))
                finite = finite and bool(torch.isfinite(lat).all())
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        # the kernels alone, on tensors of the shapes the UNet call passed
        bufs = [(torch.randn(s[:4], device=dev).half(), torch.randn(*s[:3], s[4], device=dev).half(), *scales[s[3]]) for s in per_call]
        kern = []
        for i in range(23):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for args in bufs:
                ops.freeu(*args)
            e1.record()
            torch.cuda.synchronize()
            if i >= 3:
                kern.append(e0.elapsed_time(e1))
        print(json.dumps({"case": f"FreeU ({preset} preset): plain vs native (captured graph) vs hooked (Python output_block_patch, eager)", "sampler": "Euler",
                          "steps": a.steps, "rounds": rounds, "ms_per_step": med, "ms_per_step_rounds": ms,
                          "native_minus_plain_ms": round(med["freeu_native"] - med["plain"], 2),
                          "freeu_calls_per_unet_call": [list(s) for s in per_call], "freeu_kernels_ms_per_unet_call": round(sorted(kern)[len(kern) // 2], 3),
                          "finite": finite, "shape": list(lat.shape)}), flush=True)

    def dynthresh_leg(rounds=5):
        """Plain, native Dynamic Thresholding (model option, the step stays on the fused route) at threshold percentile 1.0 and 0.99, and the
        same arithmetic as a Python sampler_cfg_function installed through set_model_sampler_cfg_function (tests/dynthresh_refs.py in torch
        fp32: the stacked general route, torch.quantile, a device read of the timestep per step) -- primed once each, then timed alternately,
        `rounds` jobs of a.steps steps per variant in this one process (each after an untimed two-step job on the same route), device events around each job.  Also the op on its own on the job's
        latent shape (events, median of 20): what the native route adds to a step."""
        import dynthresh_refs as dr
        from forge_amd import hipops as ops
        from forge_amd.backend.patcher import dynthresh as pd

        def native(pct):
            return pd.patch_dynthresh(eng.forge_objects.unet, 7.0, pct)

        def hooked(pct):
            u = eng.forge_objects.unet.clone()
            u.set_model_sampler_cfg_function(dr.sampler_cfg_function_for(pd.DynThreshParams(True, 7.0, pct), u.model.predictor))
            return u
        variants = {"plain": None, "native_p1.0": native(1.0), "native_p0.99": native(0.99), "hooked_p1.0": hooked(1.0), "hooked_p0.99": hooked(0.99)}
        saved = eng.forge_objects_after_applying_lora

        def once(unet, n):
            if unet is not None:
                eng.forge_objects_after_applying_lora = saved.shallow_copy()
                eng.forge_objects_after_applying_lora.unet = unet
            try:
                pr = processing.StableDiffusionProcessingTxt2Img(sd_model=eng, c=c1, uc=u1, seed=1, sampler_name="Euler", batch_size=b, steps=n,
                                                                 cfg_scale=7.0, width=width, height=height, do_decode=False)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                lat = processing.process_images(pr).latents
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1), lat
            finally:
                eng.forge_objects_after_applying_lora = saved
                eng.forge_objects = saved.shallow_copy()
        for unet in variants.values():    # priming (arena, caches, graphs)
            once(unet, 4)
        ms = {k: [] for k in variants}
        finite = True
        for _ in range(rounds):
            for k, unet in variants.items():
                once(unet, 2)             # a job on another route came before: what follows a change of route (caches keyed on it) is not timed
                dt, lat = once(unet, a.steps)
                ms[k].append(round(dt / a.steps, 2))
                finite = finite and bool(torch.isfinite(lat).all())
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        x, y = torch.randn(lat.shape, device=dev), torch.randn(lat.shape, device=dev)
        op_ms = {}
        for name, args in (("separate_p1.0", (1.0, True, "MEAN", "AD")), ("separate_p0.99", (0.99, True, "MEAN", "AD")), ("separate_std", (1.0, True, "MEAN", "STD")),
                           ("whole_tensor_p0.99", (0.99, False, "MEAN", "AD"))):
            t = []
            for i in range(23):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.dynthresh(x, y, 7.0, 12.0, *args, 1.0)
                e1.record()
                torch.cuda.synchronize()
                if i >= 3:
                    t.append(e0.elapsed_time(e1))
            op_ms[name] = round(sorted(t)[len(t) // 2], 4)
        print(json.dumps({"case": "Dynamic Thresholding (mimic 7, CFG 7): plain vs native (model option, fused route) vs hooked (Python sampler_cfg_function, "
                                  "general route)", "sampler": "Euler", "steps": a.steps, "rounds": rounds, "ms_per_step": med, "ms_per_step_rounds": ms,
                          "native_minus_plain_ms": {k: round(med[k] - med["plain"], 2) for k in med if k.startswith("native")},
                          "hooked_minus_native_ms": {p_: round(med["hooked_" + p_] - med["native_" + p_], 2) for p_ in ("p1.0", "p0.99")},
                          "dynthresh_op_ms": op_ms, "finite": finite, "shape": list(lat.shape)}), flush=True)

    def kohya_leg(rounds=5, block_number=3, factor=2.0, method="bicubic"):
        """Plain, native Kohya HRFix (transformer option, captured graph) and the same arithmetic as the reference's Python patches
        (tests/kohya_refs.py: F.interpolate in fp32 and the device read of sigma, on the eager hooked executor), after-skip, the window open for
        every step so that every timed step is a shrunk one -- primed once each, then timed alternately, `rounds` jobs of a.steps steps per
        variant in this one process, device events around each job.  Also the resize launches of one UNet call on their own (events, median
        of 20): what the native route adds to a shrunk forward."""
        import kohya_refs as kr
        from forge_amd import hipops as ops
        from forge_amd.backend.patcher import kohya_hrfix as pk
        native = pk.patch_kohya_hrfix(eng.forge_objects.unet, block_number, factor, 0.0, 1.0, True, method, method)
        prm = native.model_options["transformer_options"]["kohya_hrfix"]
        ip, op = kr.python_patches(block_number, factor, prm.sigma_start, prm.sigma_end, method, method)
        hooked = eng.forge_objects.unet.clone()
        hooked.set_model_input_block_patch_after_skip(ip)
        hooked.set_model_output_block_patch(op)
        variants = {"plain": None, "kohya_native": native, "kohya_hooked": hooked}
        shapes = []                       # (input shape, size, mode) of every ops.resize_nhwc call
        real = ops.resize_nhwc
        ops.resize_nhwc = lambda x, size, mode="bicubic": (shapes.append((tuple(x.shape), tuple(size), mode)), real(x, size, mode))[1]
        saved = eng.forge_objects_after_applying_lora

        def once(unet, n):
            if unet is not None:
                eng.forge_objects_after_applying_lora = saved.shallow_copy()
                eng.forge_objects_after_applying_lora.unet = unet
            try:
                pr = processing.StableDiffusionProcessingTxt2Img(sd_model=eng, c=c1, uc=u1, seed=1, sampler_name="Euler", batch_size=b, steps=n,
                                                                 cfg_scale=7.0, width=width, height=height, do_decode=False)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                lat = processing.process_images(pr).latents
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1), lat
            finally:
                eng.forge_objects_after_applying_lora = saved
                eng.forge_objects = saved.shallow_copy()
        try:
            for unet in variants.values():    # priming (arena, caches, graphs)
                once(unet, 4)
        finally:
            ops.resize_nhwc = real
        per_call = shapes[:2]                 # one UNet call: the shrink after the input block, the resize back at one output block
        ms = {k: [] for k in variants}
        finite = True
        for _ in range(rounds):
            for k, unet in variants.items():
                once(unet, 2)             # a job on another route came before: what follows a change of route is not timed
                dt, lat = once(unet, a.steps)
                ms[k].append(round(dt / a.steps, 2))
                finite = finite and bool(torch.isfinite(lat).all())
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        bufs = [(torch.randn(s[0], device=dev).half(), s[1], s[2]) for s in per_call]
        kern = []
        for i in range(23):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for args in bufs:
                ops.resize_nhwc(*args)
            e1.record()
            torch.cuda.synchronize()
            if i >= 3:
                kern.append(e0.elapsed_time(e1))
        print(json.dumps({"case": f"Kohya HRFix (block {block_number}, factor {factor}, after skip, {method}, window open on every step): plain vs native "
                                  "(captured graph) vs hooked (Python input / output block patches, eager)", "sampler": "Euler", "steps": a.steps,
                          "rounds": rounds, "ms_per_step": med, "ms_per_step_rounds": ms, "native_minus_plain_ms": round(med["kohya_native"] - med["plain"], 2),
                          "hooked_minus_native_ms": round(med["kohya_hooked"] - med["kohya_native"], 2),
                          "resize_calls_per_unet_call": [[list(s[0]), list(s[1]), s[2]] for s in per_call],
                          "resize_kernels_ms_per_unet_call": round(sorted(kern)[len(kern) // 2], 4), "finite": finite, "shape": list(lat.shape)}), flush=True)

    def pag_leg(rounds=5, scale=3.0):
        """Plain, native Perturbed-Attention Guidance (model option, a third group of rows in the captured graph) and the same arithmetic as the
        reference script installs it (tests/pag_refs.py: a post-CFG function that calls the model again with an attn1 replace patch, on the eager
        hooked executor), no attenuation and the window open, so that every timed step is a guided one -- primed once each, then timed
        alternately, `rounds` jobs of a.steps steps per variant in this one process, device events around each job.  Also the copy kernel of one
        UNet call's middle block on its own next to a plain device copy of the same bytes (events, median of 20)."""
        import pag_refs as pr_
        from forge_amd import hipops as ops
        from forge_amd.backend.patcher.pag import patch_pag
        variants = {"plain": None, "pag_native": patch_pag(eng.forge_objects.unet, scale), "pag_python": pr_.python_pag(eng.forge_objects.unet, scale)}
        variants = {k: v for k, v in variants.items() if k in a.pag_routes.split(",")}
        calls = []                        # (V^T shape, out shape, window, n, hd) of every ops.attn_value_rows call
        real = ops.attn_value_rows
        ops.attn_value_rows = lambda vt, out, **kw: (calls.append((tuple(vt.shape), tuple(out.shape), kw)), real(vt, out, **kw))[1]
        saved = eng.forge_objects_after_applying_lora

        def once(unet, n):
            if unet is not None:
                eng.forge_objects_after_applying_lora = saved.shallow_copy()
                eng.forge_objects_after_applying_lora.unet = unet
            try:
                pr = processing.StableDiffusionProcessingTxt2Img(sd_model=eng, c=c1, uc=u1, seed=1, sampler_name="Euler", batch_size=b, steps=n,
                                                                 cfg_scale=7.0, width=width, height=height, do_decode=False)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                lat = processing.process_images(pr).latents
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1), lat
            finally:
                eng.forge_objects_after_applying_lora = saved
                eng.forge_objects = saved.shallow_copy()
        try:
            for unet in variants.values():    # priming (arena, caches, graphs)
                once(unet, 4)
        finally:
            ops.attn_value_rows = real
        if set(variants) != {"plain", "pag_native", "pag_python"}:      # a single route, for a profiler: timed jobs, no comparison line
            for k, unet in variants.items():
                print(json.dumps({"case": "Perturbed-Attention Guidance, route " + k, "ms_per_step": [round(once(unet, a.steps)[0] / a.steps, 2) for _ in range(rounds)]}),
                      flush=True)
            return
        depth = cfg["transformer_depth_middle"]
        per_call = calls[:depth]              # one UNet call: one copy per transformer block of the middle block
        ms = {k: [] for k in variants}
        finite = True
        for _ in range(rounds):
            for k, unet in variants.items():
                once(unet, 2)             # a job on another route came before: what follows a change of route is not timed
                dt, lat = once(unet, a.steps)
                ms[k].append(round(dt / a.steps, 2))
                finite = finite and bool(torch.isfinite(lat).all())
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        vt_shape, out_shape, kw = per_call[0]
        vt, out = torch.randn(vt_shape, device=dev).half(), torch.empty(out_shape, device=dev, dtype=torch.float16)
        nbytes = 2 * kw["count"] * kw["n"] * kw["hd"]
        src, dst = torch.empty(nbytes // 2, device=dev, dtype=torch.float16), torch.empty(nbytes // 2, device=dev, dtype=torch.float16)

        def timed(fn):
            t = []
            for i in range(23):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if i >= 3:
                    t.append(e0.elapsed_time(e1))
            return sorted(t)[len(t) // 2]
        copy_ms = timed(lambda: real(vt, out, **kw))
        plain_copy_ms = timed(lambda: dst.copy_(src))
        print(json.dumps({"case": f"Perturbed-Attention Guidance (scale {scale}, no attenuation, every step guided): plain vs native (third group of rows, "
                                  "captured graph) vs the Python route (post-CFG function + attn1 replace patch: a second, eager model call)",
                          "sampler": "Euler", "steps": a.steps, "rounds": rounds, "ms_per_step": med, "ms_per_step_rounds": ms,
                          "native_over_plain": round(med["pag_native"] / med["plain"], 3), "python_over_native": round(med["pag_python"] / med["pag_native"], 3),
                          "copy_calls_per_unet_call": len(per_call), "copy_call": {"vt": list(vt_shape), "out": list(out_shape), **kw},
                          "copy_kernel_ms": round(copy_ms, 4), "copy_kernel_GBps_read_plus_write": round(2 * nbytes / copy_ms / 1e6, 1),
                          "device_copy_same_bytes_ms": round(plain_copy_ms, 4), "device_copy_GBps_read_plus_write": round(2 * nbytes / plain_copy_ms / 1e6, 1),
                          "copy_kernels_share_of_native_step": round(len(per_call) * copy_ms / med["pag_native"], 5),
                          "finite": finite, "shape": list(lat.shape)}), flush=True)

    def stylealign_leg(rounds=3):
        """Plain, native StyleAlign (transformer option: the self-attention of each CFG group over its joined tokens, captured graph) at strength 1.0
        and 0.5, and the same patch as the reference script installs it (tests/stylealign_refs.py: an attn1 replace patch on every block, on the
        eager hooked executor) at both strengths -- primed once each, then timed alternately, `rounds` jobs of a.steps steps per route in this one
        process, device events around each job.  native 0.5 minus native 1.0 is what the ordinary attention launches plus the blend add to a
        blended step: the number a fused single-pass kernel would be judged against."""
        import stylealign_refs as sr
        from forge_amd.backend.patcher.stylealign import patch_stylealign
        base = eng.forge_objects.unet
        variants = {"plain": None, "stylealign_native_1.0": patch_stylealign(base, 1.0), "stylealign_native_0.5": patch_stylealign(base, 0.5),
                    "stylealign_python_1.0": sr.python_stylealign(base, 1.0), "stylealign_python_0.5": sr.python_stylealign(base, 0.5)}
        saved = eng.forge_objects_after_applying_lora

        def once(unet, n):
            if unet is not None:
                eng.forge_objects_after_applying_lora = saved.shallow_copy()
                eng.forge_objects_after_applying_lora.unet = unet
            try:
                pr = processing.StableDiffusionProcessingTxt2Img(sd_model=eng, c=c1, uc=u1, seed=1, sampler_name="Euler", batch_size=b, steps=n,
                                                                 cfg_scale=7.0, width=width, height=height, do_decode=False)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                lat = processing.process_images(pr).latents
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1), lat
            finally:
                eng.forge_objects_after_applying_lora = saved
                eng.forge_objects = saved.shallow_copy()
        for unet in variants.values():    # priming (arena, caches, graphs)
            once(unet, 4)
        ms = {k: [] for k in variants}
        finite = True
        for _ in range(rounds):
            for k, unet in variants.items():
                once(unet, 2)             # a job on another route came before: what follows a change of route is not timed
                dt, lat = once(unet, a.steps)
                ms[k].append(round(dt / a.steps, 2))
                finite = finite and bool(torch.isfinite(lat).all())
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        print(json.dumps({"case": f"StyleAlign (share attention in batch, groups of {b} images): plain vs native (captured graph) vs the Python route "
                                  "(attn1 replace patch on every block, eager hooked executor)", "sampler": "Euler", "steps": a.steps, "rounds": rounds,
                          "ms_per_step": med, "ms_per_step_rounds": ms,
                          "native_over_plain": {s: round(med[f"stylealign_native_{s}"] / med["plain"], 3) for s in ("1.0", "0.5")},
                          "python_over_native": {s: round(med[f"stylealign_python_{s}"] / med[f"stylealign_native_{s}"], 3) for s in ("1.0", "0.5")},
                          "own_attention_plus_blend_ms_per_step": round(med["stylealign_native_0.5"] - med["stylealign_native_1.0"], 2),
                          "finite": finite, "shape": list(lat.shape)}), flush=True)

    def lllite_leg(rounds=3):
        """Plain, native ControlNet-LLLite (transformer option "lllite": fmxl_lllite_adapt_f16 in front of the q / k / v projections of every
        transformer block, captured graph) and the same unit as Python attn1 / attn2 patches on the eager hooked executor (backend/patcher/lllite.py
        python_patch) -- seeded weights for every transformer block of the network (attn1 q / k / v and attn2 q: what the published SDXL files
        adapt), one control image, always on.  Primed once each, then timed alternately, `rounds` jobs of a.steps steps per route in this one
        process, device events around each job.  Also the adapter launches of one UNet call on their own (device events, median of 20 per distinct
        shape) with their algorithmic bytes: what the kernel itself costs, next to what the unfolded norms and the split projections cost."""
        import lllite_refs as lr
        from forge_amd import hipops as ops
        from forge_amd.backend.patcher.lllite import patch_lllite
        base = eng.forge_objects.unet
        lsd = synth.synth_lllite_state_dict(cfg, seed=21, gain=2.0, up_gain=0.5)
        image = lr.control_images(1, (height, width), 5)
        native = patch_lllite(base, lsd, image, 1.0)
        lll = native.model_options["transformer_options"]["lllite"]
        python = base.clone()
        patch = lll.python_patch()
        python.set_model_attn1_patch(patch)
        python.set_model_attn2_patch(patch)
        variants = {"plain": None, "lllite_native": native, "lllite_python": python}
        saved = eng.forge_objects_after_applying_lora
        shapes = []                       # (m, c, slots) of every ops.lllite_adapt call
        real = ops.lllite_adapt
        ops.lllite_adapt = lambda x, cond, n, slots, mult: (shapes.append((x.shape[0], x.shape[1], n, sum(s is not None for s in slots))),
                                                            real(x, cond, n, slots, mult))[1]

        def once(unet, n):
            if unet is not None:
                eng.forge_objects_after_applying_lora = saved.shallow_copy()
                eng.forge_objects_after_applying_lora.unet = unet
            try:
                pr = processing.StableDiffusionProcessingTxt2Img(sd_model=eng, c=c1, uc=u1, seed=1, sampler_name="Euler", batch_size=b, steps=n,
                                                                 cfg_scale=7.0, width=width, height=height, do_decode=False)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                lat = processing.process_images(pr).latents
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1), lat
            finally:
                eng.forge_objects_after_applying_lora = saved
                eng.forge_objects = saved.shallow_copy()
        try:
            for k, unet in variants.items():    # priming (arena, caches, graphs)
                n_before = len(shapes)
                once(unet, 4)
                if k == "lllite_native":
                    calls = len(shapes) - n_before
        finally:
            ops.lllite_adapt = real
        launches = len(lll.blocks) * 2          # per UNet call: attn1 and attn2 of every block that has modules
        per_call = shapes[:launches]
        ms = {k: [] for k in variants}
        finite = True
        for _ in range(rounds):
            for k, unet in variants.items():
                once(unet, 2)             # a job on another route came before: what follows a change of route is not timed
                dt, lat = once(unet, a.steps)
                ms[k].append(round(dt / a.steps, 2))
                finite = finite and bool(torch.isfinite(lat).all())
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        # the adapter launches of one UNet call on their own
        kernel_ms, kernel_bytes, by_shape = 0.0, 0.0, {}
        for shape in sorted(set(per_call)):
            m_, c_, n_, ns = shape
            x = torch.randn(m_, c_, device=dev).half()
            slots = [dict({k: v.to(dev) for k, v in lr.make_slot(c_, i).items()}, cond=(torch.randn(1, n_, 32, device=dev) * 0.7).half(),
                          out=torch.empty(m_, c_, dtype=torch.float16, device=dev)) if i < ns else None for i in range(3)]
            times = []
            for _ in range(23):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                real(x, None, n_, slots, 1.0)
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
            t = sorted(times[3:])[10]
            count = per_call.count(shape)
            nbytes = 2.0 * m_ * c_ * (1 + ns)
            by_shape[f"M={m_} C={c_} slots={ns}"] = {"launches_per_unet_call": count, "ms": round(t, 4), "GBps_read_plus_write": round(nbytes / t / 1e6, 1)}
            kernel_ms += count * t
            kernel_bytes += count * nbytes
        print(json.dumps({"case": f"ControlNet-LLLite ({len(lll.modules)} modules on {len(lll.blocks)} transformer blocks, batch {b}): plain vs native "
                                  "(captured graph) vs the Python route (attn1 / attn2 patches, eager hooked executor)", "sampler": "Euler", "steps": a.steps,
                          "rounds": rounds, "ms_per_step": med, "ms_per_step_rounds": ms, "native_over_plain": round(med["lllite_native"] / med["plain"], 3),
                          "python_over_native": round(med["lllite_python"] / med["lllite_native"], 3),
                          "adapter_launches_per_unet_call": len(per_call), "adapter_launches_seen_while_priming": calls,
                          "adapter_kernel_ms_per_unet_call": round(kernel_ms, 3), "adapter_kernel_bytes_per_unet_call": kernel_bytes,
                          "adapter_kernel_GBps_read_plus_write": round(kernel_bytes / kernel_ms / 1e6, 1),
                          "adapter_kernels_share_of_native_step": round(kernel_ms / med["lllite_native"], 4), "adapter_kernel_by_shape": by_shape,
                          "finite": finite, "shape": list(lat.shape)}), flush=True)

    def ipadapter_leg(rounds=3):
        """Plain; native IP-Adapter (transformer option "ipadapter": fmxi_attention_dual_f16 in place of the text attention of every cross-attention,
        captured graph) with a base file (4 image tokens), a plus file (16) and both as two units; the composite route forced on the two-unit job
        (text attention + one attention per unit and group + add_scaled, captured graph as well); and the two units as Python attn2 replace patches
        on the eager hooked executor (backend/patcher/ipadapter.py python_patch) -- seeded weights, always on.  Primed once each, then timed
        alternately, `rounds` jobs of a.steps steps per route in this one process, device events around each job.  Also one cross-attention launch
        of each distinct shape on its own, dual against composite (device events, median of 20)."""
        from forge_amd import hipops as ops
        from forge_amd.backend.patcher import ipadapter as ipa
        from forge_amd.backend.patcher.ipadapter import patch_ipadapter
        base = eng.forge_objects.unet
        files = {kind: synth.synth_ipadapter_state_dict(cfg, plus=kind == "plus", seed=31 if kind == "base" else 77, clip_dim=1280 if kind == "plus" else 1024,
                                                        **({"resampler_dim": 1280} if kind == "plus" else {})) for kind in ("base", "plus")}
        emb = {"base": synth.synth_clip_vision_embeds(False, clip_dim=1024), "plus": synth.synth_clip_vision_embeds(True, clip_dim=1280)}
        one = lambda m, kind, w: patch_ipadapter(m, files[kind], emb[kind], w)  # noqa: E731
        two = one(one(base, "base", 0.8), "plus", 0.5)
        forced = one(one(base, "base", 0.8), "plus", 0.5)
        for u in forced.model_options["transformer_options"]["ipadapter"]:
            u.force_composite = True
        python = ipa.install_python(base.clone(), one(one(base, "base", 0.8), "plus", 0.5).model_options["transformer_options"]["ipadapter"])
        variants = {"plain": None, "ipadapter_native_base": one(base, "base", 0.8), "ipadapter_native_plus": one(base, "plus", 0.8),
                    "ipadapter_native_two_units": two, "ipadapter_composite_two_units": forced, "ipadapter_python_two_units": python}
        saved = eng.forge_objects_after_applying_lora
        shapes = []
        real_dual = ops.attention_dual
        ops.attention_dual = lambda *x, **kw: (shapes.append((kw["batch"], kw["heads"], kw["nq"], kw["nk"], len(x[5]))), real_dual(*x, **kw))[1]

        def once(unet, n):
            if unet is not None:
                eng.forge_objects_after_applying_lora = saved.shallow_copy()
                eng.forge_objects_after_applying_lora.unet = unet
            try:
                pr = processing.StableDiffusionProcessingTxt2Img(sd_model=eng, c=c1, uc=u1, seed=1, sampler_name="Euler", batch_size=b, steps=n,
                                                                 cfg_scale=7.0, width=width, height=height, do_decode=False)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                lat = processing.process_images(pr).latents
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1), lat
            finally:
                eng.forge_objects_after_applying_lora = saved
                eng.forge_objects = saved.shallow_copy()
        try:
            for unet in variants.values():    # priming (arena, caches, graphs)
                once(unet, 4)
        finally:
            ops.attention_dual = real_dual
        ms = {k: [] for k in variants}
        finite = True
        for _ in range(rounds):
            for k, unet in variants.items():
                once(unet, 2)             # a job on another route came before: what follows a change of route is not timed
                dt, lat = once(unet, a.steps)
                ms[k].append(round(dt / a.steps, 2))
                finite = finite and bool(torch.isfinite(lat).all())
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        # one cross-attention of each distinct two-unit shape on its own: the dual launch against the composite route's launches
        net = eng.forge_objects.unet.model.diffusion_model
        ctx = ipa.ipadapter_for_call(two.model_options["transformer_options"], 1.0, [1, 0], 2 * b, net)
        fctx = ipa.ipadapter_for_call(forced.model_options["transformer_options"], 1.0, [1, 0], 2 * b, net)
        by_shape = {}
        for bu_, h_, nq_, nk_, nseg in sorted(set(s for s in shapes if s[4] == 2)):
            blk = next(k for k, e in ctx.blocks.items() if e["xk"].shape[2] == h_ * 64)
            q2 = torch.randn(bu_ * nq_, h_ * 64, device=dev).half()
            kc = torch.randn(bu_ * 128, h_ * 64, device=dev).half()
            vtc = torch.randn(h_ * 64, bu_ * 128, device=dev).half()
            res = {}
            for name, cx in (("dual", ctx), ("composite", fctx)):
                times = []
                for _ in range(23):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    net._cross_attention(blk, q2, kc, vtc, bu_, nq_, nk_, 128, h_, 64, cx)
                    e1.record()
                    torch.cuda.synchronize()
                    times.append(e0.elapsed_time(e1))
                res[name + "_ms"] = round(sorted(times[3:])[10], 4)
            res["launches_per_unet_call"] = sum(1 for s in [s for s in shapes if s[4] == 2][:len(ctx.blocks)] if s[:4] == (bu_, h_, nq_, nk_))
            res["dual_GBps_q_plus_o"] = round(4.0 * bu_ * nq_ * h_ * 64 / res["dual_ms"] / 1e6, 1)
            by_shape[f"B={bu_} H={h_} Nq={nq_} Nk={nk_}+20"] = res
        print(json.dumps({"case": f"IP-Adapter (batch {b}, CFG 7: two groups): plain vs native (dual attention kernel, captured graph) with a base file, a plus "
                                  "file and both vs the composite route forced vs the Python route (attn2 replace patches, eager hooked executor)",
                          "sampler": "Euler", "steps": a.steps, "rounds": rounds, "ms_per_step": med, "ms_per_step_rounds": ms,
                          "native_over_plain": {k: round(med[k] / med["plain"], 3) for k in med if k.startswith("ipadapter_native")},
                          "python_over_native": round(med["ipadapter_python_two_units"] / med["ipadapter_native_two_units"], 3),
                          "composite_over_dual": round(med["ipadapter_composite_two_units"] / med["ipadapter_native_two_units"], 3),
                          "cross_attention_by_shape_two_units": by_shape, "finite": finite, "shape": list(lat.shape)}), flush=True)

    if "ipadapter" in what:
        ipadapter_leg()
    if "lllite" in what:
        lllite_leg()
    if "one" in what:
        run(f"{width}x{height}", sampler="Euler")
    if "stylealign" in what:
        stylealign_leg()
    if "pag" in what:
        pag_leg()
    if "dynthresh" in what:
        dynthresh_leg()
    if "freeu" in what:
        freeu_leg()
    if "kohya" in what:
        kohya_leg()
    if "samplers" in what:
        for s in ("Euler", "Euler a", "DPM++ 2M", "Heun", "DPM2 a", "DPM++ 2S a", "LMS", "IPNDM_V", "DEIS", "DPM++ SDE", "DPM++ 2M SDE", "DPM++ 3M SDE",
                  "DPM fast", "DDIM", "PLMS", "UniPC", "LCM", "DDPM"):
            run("sampler", sampler=s)
    if "and" in what:
        rows = lambda t, i: {k: v[i] for k, v in t.items()}
        mc = pp.MulticondLearnedConditioning((b,), [[pp.ComposableScheduledPromptConditioning([pp.ScheduledPromptConditioning(10 ** 6, rows(c1, i))], 1.0),
                                                     pp.ComposableScheduledPromptConditioning([pp.ScheduledPromptConditioning(10 ** 6, rows(c2, i))], 0.6)]
                                                    for i in range(b)])
        run("AND-composed prompt (2 conds + uncond = UNet batch 24)", cond=mc)
    if "hooks" in what:
        unet = eng.forge_objects.unet.clone()
        unet.set_model_attn2_output_patch(lambda n, extra: n * 0.98)
        unet.set_model_output_block_patch(lambda h, hsp, to: (h, hsp * 0.95))
        run("per-block hooks installed (eager, general attention path)", unet=unet)
    if "controlnet" in what:
        from forge_amd.backend.nn.cnets import cldm
        from forge_amd.backend.patcher import controlnet as pc
        cn = cldm.ControlNet(cfg, synth.synth_state_dict_device(controlnet_param_shapes(cfg), 6, dev), device=dev)
        hint = torch.rand(1, 3, height, width, device=dev)
        unet = pc.apply_controlnet_advanced(eng.forge_objects.unet, pc.ControlNet(cn), hint, 0.8, 0.0, 1.0)
        run("ControlNet (SDXL-size control model, strength 0.8), trunk inside the captured graph", unet=unet)
        km = eng.forge_objects.unet.model
        km.use_graph = False
        try:
            run("ControlNet (SDXL-size control model, strength 0.8), eager (residuals from get_control every step)", unet=unet)
        finally:
            km.use_graph = True
    if "hires" in what:
        run("hires fix 1024 -> 1536 (Latent bicubic), 6 + 4 steps", steps=6, enable_hr=True, hr_scale=1.5, hr_upscaler="Latent (bicubic)",
            hr_second_pass_steps=4, denoising_strength=0.6, hr_cfg=7.0)


if __name__ == "__main__":
    with torch.inference_mode():
        main()
