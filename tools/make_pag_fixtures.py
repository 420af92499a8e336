"""TEST INFRASTRUCTURE ONLY.  Generates tests/golden/tiny_pag_unet.pt with the REAL reference: its Perturbed-Attention Guidance script
(<reference>/extensions-builtin/sd_forge_perturbed_attention/scripts/forge_perturbed_attention.py) and, through oracle.ref_import, its UNet,
calc_cond_uncond_batch, set_model_options_patch_replace, sampling_function and Euler sampler.  Runs only where the reference exists; deterministic
(seeded).  Only tensors and settings are written.

    python tools/make_pag_fixtures.py [--out tests/golden]

The script imports gradio and the web UI at module level, so it is not imported: the file is parsed and the function definitions `attn_proc`,
`post_cfg_function` (nested in process_before_every_sampling, closing over its `scale` and `attenuation`) and `denoiser_callback` are compiled
from its syntax tree, at run time, into a namespace that holds the reference's own calc_cond_uncond_batch and set_model_options_patch_replace and
a stand-in for the class whose attributes the script uses as globals (scale, PAG_start, PAG_end, doPAG).

tiny_pag_unet.pt  scale, cfg, cases: [{name, config, hw, t, seed (x = noise_of(seed) * sqrt(sigma^2 + 1), conditioning = synth_conditioning(seed)),
                                       cond_denoised, uncond_denoised, degraded, result_cfg7, result_cfg1 (no uncond half),
                                       floor: {the same names: the reference's own fp16-storage run against its fp32 run, oracle/make_floor.py's
                                       half_unet}, moved: rms of result_cfg7 - plain CFG over rms(result_cfg7), [block0_only: the same for the
                                       degraded pass with only transformer block 0 perturbed]}]
                  euler4: {seeds, hw, steps, params, active (per step), scales (per step), sigmas, latent, moved (rms of the job without the script - latent,
                           over rms(latent)), floor}
Asserted here, on the CPU: every result differs from its plain-CFG counterpart by at least 10 x its floor in rms (so a gate keyed to the floor cannot
pass without the feature), and on the depth-2 cases perturbing block 0 alone differs from perturbing both blocks by as much.
"""
import argparse
import ast
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import forge_amd  # noqa: E402,F401
from forge_amd import synth  # noqa: E402
from oracle import ref_import  # noqa: E402

SCALE, CFG = 3.0, 7.0
# (name, config name, latent (h, w), middle tokens, weight seed, input seed)
CASES = [
    ("sd15 32x24: 48 middle tokens, ragged, depth 1", "TINY_SD15_UNET_CONFIG", (32, 24), 48, 0, 311),
    ("sd15 32x32: 64 middle tokens, tile-aligned, depth 1", "TINY_SD15_UNET_CONFIG", (32, 32), 64, 0, 312),
    ("sdxl 32x32: 256 middle tokens, tile-aligned, depth 2", "TINY_SDXL_UNET_CONFIG", (32, 32), 256, 0, 313),
    ("sdxl 24x20: 120 middle tokens, ragged, depth 2", "TINY_SDXL_UNET_CONFIG", (24, 20), 120, 0, 314),
]
T = [601.0, 187.0]
EULER = dict(scale=3.0, attenuation=25.0, start_step=0.0, end_step=0.67)     # 4 steps at positions 0, 1/3, 2/3, 1: the fourth is outside
SEPARATION = 10.0


def case_inputs(cfg, hw, seed, sigmas, b=2):
    """x fp32 [b, c, h, w] at the noise level of `sigmas`, cond, uncond (web-UI form) -- numpy streams, so the test rebuilds them from the seed"""
    rng = np.random.Generator(np.random.PCG64([seed, 11]))
    x = torch.from_numpy(rng.standard_normal((b, cfg["in_channels"], hw[0], hw[1]), dtype=np.float32))
    x = x * torch.sqrt(sigmas.float() ** 2 + 1.0).view(-1, 1, 1, 1)
    c, uc = synth.synth_conditioning(b, cfg["context_dim"], cfg.get("adm_in_channels"), seed=seed)
    return x, c, uc


def reference_functions(log):
    """-> (namespace, make(scale, attenuation) -> (attn_proc, post_cfg_function), denoiser_callback): compiled from the reference file's syntax
    tree.  `log`: every (arguments, result) of the calc_cond_uncond_batch call inside post_cfg_function lands there."""
    ref = ref_import.load_reference()
    from backend.patcher.base import set_model_options_patch_replace      # the reference's, importable once load_reference has set the path
    path = os.path.join(ref_import.REFERENCE_ROOT, "extensions-builtin", "sd_forge_perturbed_attention", "scripts", "forge_perturbed_attention.py")
    tree = ast.parse(open(path).read(), filename=path)
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "PerturbedAttentionGuidanceForForge"]
    assert len(cls) == 1
    methods = {n.name: n for n in cls[0].body if isinstance(n, ast.FunctionDef)}
    nested = {n.name: n for n in methods["process_before_every_sampling"].body if isinstance(n, ast.FunctionDef)}
    shell = ast.parse("def make(scale, attenuation):\n    pass\n    return attn_proc, post_cfg_function\n")
    shell.body[0].body[0:1] = [nested["attn_proc"], nested["post_cfg_function"]]
    shell.body.append(methods["denoiser_callback"])
    ast.fix_missing_locations(shell)

    def recording_calc(*a):
        r = ref.sampling_function.calc_cond_uncond_batch(*a)
        log.append((a, r))
        return r
    state = SimpleNamespace(scale=SCALE, PAG_start=0.0, PAG_end=1.0, doPAG=True)
    ns = {"PerturbedAttentionGuidanceForForge": state, "set_model_options_patch_replace": set_model_options_patch_replace,
          "calc_cond_uncond_batch": recording_calc}
    exec(compile(shell, path, "exec"), ns)
    return ns, state, set_model_options_patch_replace


def rms_rel(a, ref):
    return float((a.double() - ref.double()).pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt())


def gen(out_dir, steps=4, hw=16):
    from oracle import make_golden as mg
    from oracle import make_floor as mf
    ref = ref_import.load_reference()
    pred = ref_import.build_ref_predictor()
    log = []
    ns, state, patch_replace = reference_functions(log)
    res = {"scale": SCALE, "cfg": CFG, "t": T, "cases": []}
    nets = {}

    def networks(cfg_name, wseed):
        if (cfg_name, wseed) not in nets:
            cfg = dict(getattr(synth, cfg_name))
            sd = synth.synth_unet_state_dict(cfg, seed=wseed)
            nets[(cfg_name, wseed)] = (cfg, ref_import.build_ref_unet(cfg, sd), mf.half_unet(cfg, sd))
        return nets[(cfg_name, wseed)]

    def forward(network, x, sigmas, c, uc, cond_scale):
        """one call of the reference's sampling_function with the script's post_cfg_function installed -> recorded tensors"""
        state.scale, state.doPAG = SCALE, True
        attn_proc, post = ns["make"](SCALE, 0.0)
        den = ref_import.RefDenoiser(network, pred, [0])
        den.patcher = den.patcher.clone()
        den.patcher.set_model_sampler_post_cfg_function(post)
        den.inner_model.inner_model.forge_objects.unet = den.patcher
        del log[:]
        result = den(x, sigmas, uc, c, cond_scale)
        assert len(log) == 1
        (model, cond, _, xin, sg, new_options), (degraded, _) = log[0]
        return {"result": result, "cond_denoised": den.last[1], "uncond_denoised": den.last[2], "degraded": degraded,
                "call": (attn_proc, model, cond, xin, sg, new_options)}

    with torch.no_grad():
        for name, cfg_name, lat, tokens, wseed, seed in CASES:
            cfg, net, net16 = networks(cfg_name, wseed)
            sigmas = pred.sigma(torch.tensor(T))
            x, c, uc = case_inputs(cfg, lat, seed, sigmas)
            if cfg.get("adm_in_channels") is not None:
                c, uc = ref_import.SdxlCond(c), ref_import.SdxlCond(uc)
            runs = {}
            for tag, network in (("fp32", net), ("fp16", net16)):
                r7 = forward(network, x, sigmas, c, uc, CFG)
                r1 = forward(network, x, sigmas, c, uc, 1.0)
                runs[tag] = {"cond_denoised": r7["cond_denoised"], "uncond_denoised": r7["uncond_denoised"], "degraded": r7["degraded"],
                             "result_cfg7": r7["result"], "result_cfg1": r1["result"], "call": r7["call"], "plain_cfg1": r1["cond_denoised"]}
            a, h = runs["fp32"], runs["fp16"]
            names = ("cond_denoised", "uncond_denoised", "degraded", "result_cfg7", "result_cfg1")
            floor = {k: mf.metrics(h[k].float(), a[k]) for k in names}
            plain7 = a["uncond_denoised"] + (a["cond_denoised"] - a["uncond_denoised"]) * CFG
            case = {"name": name, "config": cfg_name, "weight_seed": wseed, "hw": lat, "middle_tokens": tokens, "seed": seed,
                    "depth": cfg["transformer_depth_middle"], **{k: a[k] for k in names}, "floor": floor,
                    "moved": {"result_cfg7": rms_rel(plain7, a["result_cfg7"]), "result_cfg1": rms_rel(a["plain_cfg1"], a["result_cfg1"])}}
            for k in ("result_cfg7", "result_cfg1"):
                assert case["moved"][k] >= SEPARATION * floor[k]["rms_rel"], (name, k, case["moved"][k], floor[k])
            mid = (tokens, (lat[0] // (2 ** (len(cfg["channel_mult"]) - 1))) * (lat[1] // (2 ** (len(cfg["channel_mult"]) - 1))))
            assert mid[0] == mid[1], mid
            if cfg["transformer_depth_middle"] > 1:
                # the key ("middle", 0) matches EVERY block: perturbing block 0 alone is another computation, by more than the floor can hide
                attn_proc, model, cond, xin, sg, new_options = a["call"]
                only0 = {k: v for k, v in new_options.items()}
                only0["transformer_options"] = dict(new_options["transformer_options"])
                only0["transformer_options"]["patches_replace"] = {}
                only0 = patch_replace(only0, attn_proc, "attn1", "middle", 0, 0)
                d0, _ = ref.sampling_function.calc_cond_uncond_batch(model, cond, None, xin, sg, only0)
                r0 = plain7 + (a["cond_denoised"] - d0) * SCALE
                case["block0_only"] = rms_rel(r0, a["result_cfg7"])
                assert case["block0_only"] >= SEPARATION * floor["result_cfg7"]["rms_rel"], (name, case["block0_only"], floor["result_cfg7"])
            print(name, "| moved", case["moved"], "| block 0 only", case.get("block0_only"), "| floor rms_rel",
                  {k: round(v["rms_rel"], 6) for k, v in floor.items()})
            res["cases"].append(case)

    cfg, net, net16 = networks("TINY_SD15_UNET_CONFIG", 0)
    b = 2

    def euler(network, with_pag=True):
        c, uc = synth.synth_conditioning(b, cfg["context_dim"], None, seed=1234)
        seeds = [1000 + i for i in range(b)]
        e = EULER
        state.scale, state.PAG_start, state.PAG_end, state.doPAG = e["scale"], e["start_step"], e["end_step"], True
        attn_proc, post = ns["make"](e["scale"], e["attenuation"])
        den = ref_import.RefDenoiser(network, pred, seeds)
        den.patcher = den.patcher.clone()
        if with_pag:
            den.patcher.set_model_sampler_post_cfg_function(post)
        den.inner_model.inner_model.forge_objects.unet = den.patcher
        trace = []
        inner_call = den.__call__

        class Stepper:
            """the web UI's CFGDenoiser runs the cfg_denoiser callbacks before every model call: the script's window test"""
            inner_model = den.inner_model

            def __call__(self, *a, **kw):
                ns["denoiser_callback"](None, SimpleNamespace(sampling_step=den.step, total_sampling_steps=steps))
                trace.append((bool(state.doPAG and state.scale > 0.0), float(state.scale)))
                return inner_call(*a, **kw)
        rng = mg.ImageRNG((cfg["in_channels"], hw, hw), seeds, "CPU")
        xx = rng.next()
        sg = den.inner_model.get_sigmas(steps)
        xx = pred.noise_scaling(sg[0], xx, torch.zeros_like(xx), max_denoise=False)
        ref.kd_sampling.torch = mg._Hijack(rng)
        ref.sampling_function.sampling_prepare(den.patcher, x=xx)
        try:
            lat = ref.kd_sampling.sample_euler(Stepper(), xx, sg, extra_args={"cond": c, "uncond": uc, "cond_scale": CFG, "s_min_uncond": 0.0,
                                                                               "image_cond": None}, disable=True)
        finally:
            ref.kd_sampling.torch = torch
            ref.sampling_function.sampling_cleanup(den.patcher)
        return lat, seeds, trace, [float(v) for v in sg]

    with torch.no_grad():
        lat, seeds, trace, sg = euler(net)
        lat16, _, trace16, _ = euler(net16)
        plain, _, _, _ = euler(net, with_pag=False)
    assert trace == trace16 and [a for a, _ in trace] == [True, True, True, False], trace
    floor = mf.metrics(lat16.float(), lat)
    moved = rms_rel(plain, lat)
    assert moved >= SEPARATION * floor["rms_rel"], (moved, floor)
    res["euler4"] = {"seeds": seeds, "hw": hw, "steps": steps, "params": dict(EULER), "active": [a for a, _ in trace], "scales": [s for _, s in trace],
                     "sigmas": sg, "latent": lat, "moved": moved, "floor": floor}
    print("euler4: trace", trace, "sigmas", sg, "latent std", float(lat.std()), "moved", moved, "fp16 floor", floor)
    path = os.path.join(out_dir, "tiny_pag_unet.pt")
    torch.save(res, path)
    print(path, os.path.getsize(path), "bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    if not ref_import.reference_available():
        raise SystemExit("the reference is not present: this generator runs only next to it")
    gen(args.out)


if __name__ == "__main__":
    main()
