"""TEST INFRASTRUCTURE ONLY.  Generates tests/golden/ipadapter.pt with the REAL reference: its IP-Adapter library
(<reference>/extensions-builtin/sd_forge_ipadapter/lib_ipadapter, imported from its files at run time) and, through oracle.ref_import, its UNet, its
UnetPatcher and sampling_function.  Runs only where the reference exists; deterministic (seeded).  Only tensors and settings are written.

    python tools/make_ipadapter_fixtures.py [--out tests/golden]

ipadapter.pt
    seeds / gains / hw / b / t / cfg: the UNet, the IP-Adapter files and the CLIP-vision stand-ins are drawn from seeds (synth.synth_unet_state_dict,
    synth.synth_ipadapter_state_dict, synth.synth_clip_vision_embeds), not stored
    tokens: {"base" | "plus": (cond, uncond)}: the reference's ImageProjModel, and its Resampler at the synthetic file's widths, in fp32;
            tokens_floor: {...: the same networks in fp16 against that}
    patch_calls: [{units: [(kind, weight, weight_type)], cond_or_uncond, seed, every, out}]: the reference's CrossAttentionPatch itself, called for the
                 middle block of the SDXL-shaped config on q = randn(4, 64, 128), k / v = randn(4, 77, 128) from torch.Generator(seed); the query rows ::every are kept
    results: {config: {case: denoised fp32}}, plain: {config: denoised}: sampling_function at CFG 7 with the patch installed through the
             reference's set_model_patch_replace on the network's own block keys (backend/nn/ipadapter.attn2_order); cases = CASES below
    floor: {config: {case: the reference's own fp16 run of the case against its fp32 run}}, moved: {...: rms(result - plain) / rms(result)}
    windowed: {config: {"sigma_start", "sigma_end" of a (0.2, 0.8) unit, "outside": True when its run at a sigma beyond the window equals the plain
              run exactly}}; inside the window the run equals results[config]["base/original"] exactly (asserted here)
Asserted here, on the CPU: every result differs from the plain one by at least 10 x its floor in rms.
"""
import argparse
import contextlib
import importlib
import io
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import forge_amd  # noqa: E402,F401
from forge_amd import synth  # noqa: E402
from forge_amd.backend.nn import ipadapter as nets  # noqa: E402
from forge_amd.backend.nn.layout import unet_layout  # noqa: E402
from oracle import ref_import  # noqa: E402
import lllite_refs as L  # noqa: E402

CONFIGS = ("TINY_SDXL_2LEVEL_UNET_CONFIG", "TINY_SD15_UNET_CONFIG", "TINY_SD15_WIDE_HEADS_UNET_CONFIG")     # the last: heads of 128, the composite route
WEIGHT_SEED, SEED = 0, 611
HW, B, T_ALL, CFG = (32, 32), 2, [601.0, 187.0], 7.0
KV_GAIN = 1.0          # the synthetic to_k_ip / to_v_ip at the init law's own gain already move the output by >= 10 x the floor
FILE_SEEDS = {"base": 31, "plus": 77}
# case -> [(file kind, weight, weight type)]
CASES = {"base/original": [("base", 0.8, "original")], "plus/original": [("plus", 0.8, "original")], "base/linear": [("base", 0.8, "linear")],
         "plus/channel": [("plus", 0.8, "channel")], "two_units": [("base", 0.8, "original"), ("plus", 0.5, "linear")]}
PATCH_CASES = [[("base", 0.8, "original")], [("base", 0.8, "linear")], [("plus", 0.8, "channel")], [("base", 0.8, "original"), ("plus", 0.5, "linear")]]
WINDOW = (0.2, 0.8)
PATCH_EVERY = 4        # of every patch call's output the query rows ::4 are kept (attention works row by row)
SEPARATION = 10.0


def reference_library():
    """lib_ipadapter.IPAdapterPlus from the reference's files; the modules it imports for file handling and image preprocessing only are stubbed"""
    ref_import.load_reference()
    for name, attrs in (("modules_forge", {}), ("modules_forge.shared", dict(controlnet_dir="", models_path="")),
                        ("backend.patcher.clipvision", dict(clip_preprocess=None)), ("backend.misc.image_resize", dict(adaptive_resize=None))):
        if name not in sys.modules:
            try:
                importlib.import_module(name)
            except Exception:
                m = types.ModuleType(name)
                m.__dict__.update(attrs)
                sys.modules[name] = m
    tv = sys.modules.get("torchvision")
    if tv is not None and not hasattr(tv, "transforms"):
        tv.transforms = types.ModuleType("torchvision.transforms")
    ext = os.path.join(ref_import.REFERENCE_ROOT, "extensions-builtin", "sd_forge_ipadapter")
    if ext not in sys.path:
        sys.path.insert(0, ext)
    return importlib.import_module("lib_ipadapter.IPAdapterPlus")


def rms_rel(a, ref):
    return float((a.double() - ref.double()).pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt())


def files_of(cfg):
    return {kind: synth.synth_ipadapter_state_dict(cfg, plus=kind == "plus", seed=FILE_SEEDS[kind], kv_gain=KV_GAIN) for kind in ("base", "plus")}


def reference_unit(lib, model, kind, dtype):
    """-> (an object with the reference's To_KV as .ip_layers, cond tokens, uncond tokens): ImageProjModel / Resampler are the reference's classes, the
    Resampler at the synthetic file's widths (IPAdapter.__init__ hard-codes the published ones)"""
    proj = model["image_proj"]
    ctx = int(model["ip_adapter"]["1.to_k_ip.weight"].shape[1])
    if kind == "plus":
        dim = int(proj["latents"].shape[2])
        net = lib.Resampler(dim=dim, depth=4, dim_head=64, heads=int(proj["layers.0.0.to_q.weight"].shape[0]) // 64, num_queries=int(proj["latents"].shape[1]),
                            embedding_dim=int(proj["proj_in.weight"].shape[1]), output_dim=ctx, ff_mult=4)
    else:
        net = lib.ImageProjModel(cross_attention_dim=ctx, clip_embeddings_dim=int(proj["proj.weight"].shape[1]), clip_extra_context_tokens=4)
    net.load_state_dict(proj)
    net = net.to(dtype)
    kv = lib.To_KV({k: v.clone() for k, v in model["ip_adapter"].items()}).to(dtype)
    emb = synth.synth_clip_vision_embeds(plus=kind == "plus")
    return types.SimpleNamespace(ip_layers=kv), net(emb[0].to(dtype)), net(emb[1].to(dtype))


def install(lib, patcher, files, units, order, dtype, sigmas=(999999999.9, 0.0)):
    """the reference's own installation loop (apply_ipadapter) on the network's own block keys, one call per unit"""
    work = patcher
    for kind, weight, weight_type in units:
        adapter, cond, uncond = reference_unit(lib, files[kind], kind, dtype)
        work = work.clone()
        kwargs = {"number": 0, "weight": weight, "ipadapter": adapter, "cond": cond, "uncond": uncond, "weight_type": weight_type, "mask": None,
                  "sigma_start": sigmas[0], "sigma_end": sigmas[1], "unfold_batch": False}
        for entry in order:
            lib.set_model_patch_replace(work, kwargs, nets.reference_key(entry))
            kwargs["number"] += 1
    return work


def gen(out_dir):
    from oracle import make_floor as mf
    lib = reference_library()
    pred = ref_import.build_ref_predictor()
    res = {"configs": list(CONFIGS), "weight_seed": WEIGHT_SEED, "seed": SEED, "hw": HW, "b": B, "t": T_ALL, "cfg": CFG, "kv_gain": KV_GAIN,
           "file_seeds": FILE_SEEDS, "cases": CASES, "window": WINDOW, "tokens": {}, "tokens_floor": {}, "patch_calls": [], "results": {}, "plain": {}, "floor": {},
           "moved": {}, "windowed": {}}
    sigmas = pred.sigma(torch.tensor(T_ALL))
    with torch.no_grad():
        for config in CONFIGS:
            cfg = dict(getattr(synth, config))
            order = nets.attn2_order(unet_layout(cfg))
            sd = synth.synth_unet_state_dict(cfg, seed=WEIGHT_SEED)
            nets_ref = {"fp32": ref_import.build_ref_unet(cfg, sd), "fp16": mf.half_unet(cfg, sd)}
            files = files_of(cfg)
            x, c, uc = L.case_inputs(cfg, HW, SEED, sigmas, B)
            if isinstance(c, dict):
                c, uc = ref_import.SdxlCond(c), ref_import.SdxlCond(uc)

            def run(prec, units, xs=x, sg=sigmas, window=(999999999.9, 0.0)):
                den = ref_import.RefDenoiser(nets_ref[prec], pred, [0])
                dtype = torch.float32 if prec == "fp32" else torch.float16
                with contextlib.redirect_stdout(io.StringIO()):
                    den.patcher = install(lib, den.patcher.clone(), files, units, order, dtype, window) if units else den.patcher.clone()
                den.inner_model.inner_model.forge_objects.unet = den.patcher
                return den(xs, sg, uc, c, CFG)

            plain = run("fp32", None)
            res["plain"][config] = plain
            res["results"][config], res["floor"][config], res["moved"][config] = {}, {}, {}
            for case, units in CASES.items():
                r, r16 = run("fp32", units), run("fp16", units)
                res["results"][config][case] = r
                res["floor"][config][case] = mf.metrics(r16.float(), r)
                res["moved"][config][case] = rms_rel(plain, r)
                print(config, case, "moved", round(res["moved"][config][case], 5), "floor rms_rel", round(res["floor"][config][case]["rms_rel"], 6))
                assert res["moved"][config][case] >= SEPARATION * res["floor"][config][case]["rms_rel"], (config, case)
            s0, s1 = pred.percent_to_sigma(WINDOW[0]), pred.percent_to_sigma(WINDOW[1])
            inside = run("fp32", CASES["base/original"], window=(s0, s1))
            high = torch.full_like(sigmas, float(s0) * 1.5)
            xh = x / torch.sqrt(sigmas.float() ** 2 + 1.0).view(-1, 1, 1, 1) * torch.sqrt(high.float() ** 2 + 1.0).view(-1, 1, 1, 1)
            outside = torch.equal(run("fp32", CASES["base/original"], xh, high, (s0, s1)), run("fp32", None, xh, high))
            assert s1 < float(sigmas[0]) < s0 and outside and torch.equal(inside, res["results"][config]["base/original"])
            res["windowed"][config] = {"sigma_start": float(s0), "sigma_end": float(s1), "outside": outside}
            if config == CONFIGS[0]:
                for kind in ("base", "plus"):
                    _, cond, uncond = reference_unit(lib, files[kind], kind, torch.float32)
                    res["tokens"][kind] = (cond.clone(), uncond.clone())
                    _, c16, u16 = reference_unit(lib, files[kind], kind, torch.float16)
                    res["tokens_floor"][kind] = mf.metrics(torch.cat([c16, u16]).float(), torch.cat([cond, uncond]))
                    print("tokens", kind, "floor", res["tokens_floor"][kind])
                for i, units in enumerate(PATCH_CASES):
                    for cou in ([1, 0], [0, 1]):
                        g = torch.Generator().manual_seed(100 + i)
                        q, k, v = torch.randn(4, 64, 128, generator=g), torch.randn(4, 77, 128, generator=g), torch.randn(4, 77, 128, generator=g)
                        number = [e[3] for e in order].index("middle_block.1.transformer_blocks.0")
                        patch = None
                        for kind, weight, weight_type in units:
                            adapter, cond, uncond = reference_unit(lib, files[kind], kind, torch.float32)
                            args = (weight, adapter, number, cond, uncond, weight_type)
                            always = dict(sigma_start=999999999.9, sigma_end=0.0)     # (the class's own defaults skip every call that carries no sigma)
                            if patch is None:
                                patch = lib.CrossAttentionPatch(*args, **always)
                            else:
                                patch.set_new_condition(*args, **always)
                        out = patch(q, k, v, {"cond_or_uncond": cou, "n_heads": 2, "original_shape": [4, 4, 8, 8]})
                        res["patch_calls"].append({"units": units, "cond_or_uncond": cou, "seed": 100 + i, "every": PATCH_EVERY, "out": out[:, ::PATCH_EVERY].clone()})
    path = os.path.join(out_dir, "ipadapter.pt")
    torch.save(res, path)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    if not ref_import.reference_available():
        raise SystemExit("the reference is not present: this generator runs only next to it")
    gen(args.out)


if __name__ == "__main__":
    main()
