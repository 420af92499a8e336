"""TEST INFRASTRUCTURE ONLY.  Generates tests/golden/tiny_stylealign_unet.pt with the REAL reference: its StyleAlign script
(<reference>/extensions-builtin/sd_forge_stylealign/scripts/forge_stylealign.py) and, through oracle.ref_import, its UNet, its UnetPatcher's
set_model_replace_all, sampling_function and Euler sampler.  Runs only where the reference exists; deterministic (seeded).  Only tensors and
settings are written.

    python tools/make_stylealign_fixtures.py [--out tests/golden] [--plain FILE]
    python tools/make_stylealign_fixtures.py --record-plain FILE      on an MI355X, in a checkout of the commit BEFORE the executor took a `share`
                                                                      argument (with tests/stylealign_refs.py copied in): writes the FILE of --plain

The script imports gradio and the web UI at module level, so it is not imported: the file is parsed and the function definitions `sdp` (module
level) and `join`, `aligned_attention`, `attn1_proc` (nested in process_before_every_sampling, closing over its `strength`) are compiled from its
syntax tree, at run time, into a namespace whose `attention` is the reference's own backend.attention.

tiny_stylealign_unet.pt
    cfg, strengths, cases: [{name, config, hw, b, t, seed (x = (noise_of(seed) + CONTENT * per-image channel offsets) * sqrt(sigma^2 + 1),
                             conditioning = synth_conditioning(seed)), results: {"s<strength>/cfg7" | "s<strength>/cfg1": denoised},
                             floor: {the same names: the reference's own fp16-storage run against its fp32 run, oracle/make_floor.py's half_unet},
                             moved: {the same names: rms of result - the plain result, over rms(result)}, vs_other_strength: {...}}]
    euler4: {"s0.5" | "s1.0": {config, seeds, cond_seed, hw, steps, strength, sigmas, latent, moved, vs_other_strength, floor}}: 4-step Euler, CFG 7,
            b = 3, on the tiny SDXL network (on the tiny SD1.5 network a whole job moves by under 3 x its floor)
    proc_calls: [{q, k, v [rows, n, heads * d] fp32, heads, cond_or_uncond, cond_indices, uncond_indices, strength, out}]: the compiled attn1_proc
                itself on small random operands (tests/stylealign_refs.py's restatement is held to these on the CPU)
    plain_bits: tensors a GPU run of the executor produced BEFORE the `share` argument existed (--record-plain below wrote them, --plain merges
                them in; kept from the existing file otherwise): the plain path must still produce them bit for bit.  Recorded at commit dc6e05b
                ("Derive the ctypes binding from fmx.h; one call path in hipops"), the parent of the commit that added the option.
Asserted here, on the CPU: every result differs from its plain counterpart by at least 10 x its floor in rms, and strength 0.5 differs from strength
1.0 by as much -- a gate keyed to the floor cannot pass without the feature, or with the wrong branch.  A case that misses the separation is
run again with another input seed (seed + 100 k, SEED_TRIES times); the assertion stays.  The seeds of the two SD1.5 cases in CASES were found
that way: with pure-noise inputs sharing moves that network by about 3 x its floor, with the per-image content offset by 6 to 12 x.
"""
import argparse
import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import forge_amd  # noqa: E402,F401
from forge_amd import synth  # noqa: E402
from oracle import ref_import  # noqa: E402

CFG = 7.0
STRENGTHS = [1.0, 0.5]
T_ALL = [601.0, 187.0, 401.0, 799.0]
# (name, config name, latent (h, w), images per group, weight seed, input seed)
CASES = [
    ("sdxl 32x32 b3: n 256, T 768 aligned, depth 2", "TINY_SDXL_UNET_CONFIG", (32, 32), 3, 0, 411),
    ("sd15 32x24 b3: n 768 / 192 aligned, middle n 48 -> T 144 ragged", "TINY_SD15_UNET_CONFIG", (32, 24), 3, 0, 1712),
    ("sdxl 24x20 b3: n 120, T 360 ragged, n % 8 == 0", "TINY_SDXL_UNET_CONFIG", (24, 20), 3, 0, 413),
    ("sdxl 20x18 b3: n 90, T 270 ragged, n % 8 != 0", "TINY_SDXL_UNET_CONFIG", (20, 18), 3, 0, 414),
    ("sd15 32x24 b4: middle n 48 ragged but T 192 aligned", "TINY_SD15_UNET_CONFIG", (32, 24), 4, 0, 1012),
]
EULER = dict(config="TINY_SDXL_UNET_CONFIG", b=3, steps=4, hw=16, seed=1234)      # 64 tokens per image, T = 192
SEPARATION = 10.0


CONTENT = 4.0      # per-image, per-channel offset of the latent in units of its noise: images of one batch differ in content, which is what sharing moves
SEED_TRIES = 6     # a case that misses the separation gets another input seed (seed + 100 k); the assertion stays


def case_inputs(cfg, hw, seed, sigmas, b):
    """x fp32 [b, c, h, w] at the noise level of `sigmas` -- unit noise plus a per-image, per-channel offset of CONTENT x N(0, 1) -- and cond, uncond
    (web-UI form) -- numpy streams, so the test rebuilds them from the seed"""
    rng = np.random.Generator(np.random.PCG64([seed, 11]))
    x = torch.from_numpy(rng.standard_normal((b, cfg["in_channels"], hw[0], hw[1]), dtype=np.float32))
    x = x + CONTENT * torch.from_numpy(np.random.Generator(np.random.PCG64([seed, 12])).standard_normal((b, cfg["in_channels"], 1, 1), dtype=np.float32))
    x = x * torch.sqrt(sigmas.float() ** 2 + 1.0).view(-1, 1, 1, 1)
    c, uc = synth.synth_conditioning(b, cfg["context_dim"], cfg.get("adm_in_channels"), seed=seed)
    return x, c, uc


def reference_make():
    """-> make(strength) -> attn1_proc: compiled from the reference file's syntax tree"""
    ref = ref_import.load_reference()
    path = os.path.join(ref_import.REFERENCE_ROOT, "extensions-builtin", "sd_forge_stylealign", "scripts", "forge_stylealign.py")
    tree = ast.parse(open(path).read(), filename=path)
    sdp = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "sdp"]
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "StyleAlignForForge"]
    assert len(sdp) == 1 and len(cls) == 1
    methods = {n.name: n for n in cls[0].body if isinstance(n, ast.FunctionDef)}
    nested = {n.name: n for n in methods["process_before_every_sampling"].body if isinstance(n, ast.FunctionDef)}
    shell = ast.parse("def make(strength):\n    pass\n    return attn1_proc\n")
    shell.body[0].body[0:1] = [nested["join"], nested["aligned_attention"], nested["attn1_proc"]]
    shell.body.insert(0, sdp[0])
    ast.fix_missing_locations(shell)
    ns = {"attention": ref.attention, "torch": torch}
    exec(compile(shell, path, "exec"), ns)
    return ns["make"]


def rms_rel(a, ref):
    return float((a.double() - ref.double()).pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt())


def tag_of(strength, cfg_scale):
    return f"s{strength}/cfg{int(cfg_scale)}"


def gen(out_dir, plain_path=None):
    from oracle import make_golden as mg
    from oracle import make_floor as mf
    ref = ref_import.load_reference()
    pred = ref_import.build_ref_predictor()
    make = reference_make()
    res = {"cfg": CFG, "strengths": STRENGTHS, "t": T_ALL, "cases": []}
    nets = {}

    def networks(cfg_name, wseed):
        if (cfg_name, wseed) not in nets:
            cfg = dict(getattr(synth, cfg_name))
            sd = synth.synth_unet_state_dict(cfg, seed=wseed)
            nets[(cfg_name, wseed)] = (cfg, ref_import.build_ref_unet(cfg, sd), mf.half_unet(cfg, sd))
        return nets[(cfg_name, wseed)]

    def denoiser(network, strength, seeds=(0,)):
        den = ref_import.RefDenoiser(network, pred, list(seeds))
        den.patcher = den.patcher.clone()
        if strength is not None:
            den.patcher.set_model_replace_all(make(strength), "attn1")      # the script's own installation
        den.inner_model.inner_model.forge_objects.unet = den.patcher
        return den

    with torch.no_grad():
        def one_case(name, cfg_name, lat, b, wseed, seed):
            cfg, net, net16 = networks(cfg_name, wseed)
            t = T_ALL[:b]
            sigmas = pred.sigma(torch.tensor(t))
            x, c, uc = case_inputs(cfg, lat, seed, sigmas, b)
            if cfg.get("adm_in_channels") is not None:
                c, uc = ref_import.SdxlCond(c), ref_import.SdxlCond(uc)
            runs = {}
            for prec, network in (("fp32", net), ("fp16", net16)):
                for strength in [None] + STRENGTHS:
                    for cs in (CFG, 1.0):
                        runs[(prec, strength, cs)] = denoiser(network, strength)(x, sigmas, uc, c, cs)
            case = {"name": name, "config": cfg_name, "weight_seed": wseed, "hw": lat, "b": b, "t": t, "seed": seed, "results": {}, "floor": {},
                    "moved": {}, "vs_other_strength": {}}
            for strength in STRENGTHS:
                for cs in (CFG, 1.0):
                    k = tag_of(strength, cs)
                    r = runs[("fp32", strength, cs)]
                    case["results"][k] = r
                    case["floor"][k] = mf.metrics(runs[("fp16", strength, cs)].float(), r)
                    case["moved"][k] = rms_rel(runs[("fp32", None, cs)], r)
                    other = [s for s in STRENGTHS if s != strength][0]
                    case["vs_other_strength"][k] = rms_rel(runs[("fp32", other, cs)], r)
            print(name, "seed", seed, "| moved", {k: round(v, 5) for k, v in case["moved"].items()}, "| vs other strength",
                  {k: round(v, 5) for k, v in case["vs_other_strength"].items()}, "| floor rms_rel",
                  {k: round(v["rms_rel"], 6) for k, v in case["floor"].items()})
            return case

        for name, cfg_name, lat, b, wseed, seed in CASES:
            for k in range(SEED_TRIES):
                case = one_case(name, cfg_name, lat, b, wseed, seed + 100 * k)
                short = [(t, case["moved"][t], case["vs_other_strength"][t], case["floor"][t]["rms_rel"]) for t in case["results"]
                         if min(case["moved"][t], case["vs_other_strength"][t]) < SEPARATION * case["floor"][t]["rms_rel"]]
                if not short:
                    break
                print("   misses the separation:", short)
            assert not short, (name, short)
            res["cases"].append(case)

    cfg, net, net16 = networks(EULER["config"], 0)
    b, steps, hw = EULER["b"], EULER["steps"], EULER["hw"]

    def euler(network, strength, first_seed):
        c, uc = synth.synth_conditioning(b, cfg["context_dim"], cfg.get("adm_in_channels"), seed=EULER["seed"])
        if cfg.get("adm_in_channels") is not None:
            c, uc = ref_import.SdxlCond(c), ref_import.SdxlCond(uc)
        seeds = [first_seed + i for i in range(b)]
        den = denoiser(network, strength, seeds)
        rng = mg.ImageRNG((cfg["in_channels"], hw, hw), seeds, "CPU")
        xx = rng.next()
        sg = den.inner_model.get_sigmas(steps)
        xx = pred.noise_scaling(sg[0], xx, torch.zeros_like(xx), max_denoise=False)
        ref.kd_sampling.torch = mg._Hijack(rng)
        ref.sampling_function.sampling_prepare(den.patcher, x=xx)
        try:
            lat = ref.kd_sampling.sample_euler(den, xx, sg, extra_args={"cond": c, "uncond": uc, "cond_scale": CFG, "s_min_uncond": 0.0,
                                                                       "image_cond": None}, disable=True)
        finally:
            ref.kd_sampling.torch = torch
            ref.sampling_function.sampling_cleanup(den.patcher)
        return lat, seeds, [float(v) for v in sg]

    def euler_jobs(first_seed):
        out, lats = {}, {}
        plain, _, _ = euler(net, None, first_seed)
        for strength in (0.5, 1.0):
            lat, seeds, sg = euler(net, strength, first_seed)
            lat16, _, _ = euler(net16, strength, first_seed)
            lats[strength] = lat
            out[f"s{strength}"] = {"config": EULER["config"], "seeds": seeds, "hw": hw, "steps": steps, "strength": strength, "sigmas": sg, "latent": lat,
                                   "moved": rms_rel(plain, lat), "floor": mf.metrics(lat16.float(), lat), "cond_seed": EULER["seed"]}
        for s_, o_ in ((0.5, 1.0), (1.0, 0.5)):
            out[f"s{s_}"]["vs_other_strength"] = rms_rel(lats[o_], lats[s_])
        return out

    with torch.no_grad():
        for k in range(SEED_TRIES):
            jobs = euler_jobs(1000 + 100 * k)
            short = [(t, e["moved"], e["vs_other_strength"], e["floor"]["rms_rel"]) for t, e in jobs.items()
                     if min(e["moved"], e["vs_other_strength"]) < SEPARATION * e["floor"]["rms_rel"]]
            print("euler4 seeds from", 1000 + 100 * k, {t: (round(e["moved"], 5), round(e["vs_other_strength"], 5), round(e["floor"]["rms_rel"], 6))
                                                       for t, e in jobs.items()}, "misses the separation" if short else "")
            if not short:
                break
        assert not short, short
        res["euler4"] = jobs

    # the compiled attn1_proc on its own: [uncond ; cond] and cond-only calls of 3 images, 2 heads of 8, 12 tokens
    g = torch.Generator().manual_seed(77)
    res["proc_calls"] = []
    for strength in (1.0, 0.5, 0.3, 0.005):
        for cou in ([1, 0], [0]):
            rows, heads, n, d = 3 * len(cou), 2, 12, 8
            q, k, v = (torch.randn(rows, n, heads * d, generator=g) for _ in range(3))
            to = {"n_heads": heads, "cond_or_uncond": cou, "cond_indices": [i * 3 + j for i, cx in enumerate(cou) if cx == 0 for j in range(3)],
                  "uncond_indices": [i * 3 + j for i, cx in enumerate(cou) if cx != 0 for j in range(3)]}
            res["proc_calls"].append({"q": q, "k": k, "v": v, "heads": heads, "strength": strength, "out": make(strength)(q, k, v, dict(to)),
                                      **{kk: to[kk] for kk in ("cond_or_uncond", "cond_indices", "uncond_indices")}})

    path = os.path.join(out_dir, "tiny_stylealign_unet.pt")
    if plain_path is not None:
        res["plain_bits"] = torch.load(plain_path, map_location="cpu")
    elif os.path.exists(path):
        res["plain_bits"] = torch.load(path, map_location="cpu", weights_only=False).get("plain_bits")
    torch.save(res, path)
    print(path, os.path.getsize(path), "bytes")


def record_plain(path):
    """tests/stylealign_refs.plain_forward on the GPU, from code that does not know the option yet: refuses to run on a tree that does"""
    import inspect
    import stylealign_refs as sr
    from forge_amd.backend.nn.unet import IntegratedUNet2DConditionModel
    if {"share", "native"} & set(inspect.signature(IntegratedUNet2DConditionModel.forward_packed).parameters):     # loose, or inside the NativeCall
        raise SystemExit("this executor already takes `share`: record the plain bits from the commit before it")
    out = [sr.plain_forward(i) for i in range(len(sr.PLAIN_FORWARDS))]
    again = [sr.plain_forward(i) for i in range(len(sr.PLAIN_FORWARDS))]
    for a, b in zip(out, again):
        assert torch.equal(a, b) and bool(torch.isfinite(a.float()).all()), "the plain forward is not reproducible run to run"
    torch.save(out, path)
    print(path, [tuple(t.shape) for t in out])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--plain", default=None, help="tensors of the plain path recorded on the GPU before the feature (see the module docstring)")
    ap.add_argument("--record-plain", default=None, metavar="FILE", help="write the plain-path tensors (GPU, from the commit before the option); nothing else runs")
    args = ap.parse_args()
    if args.record_plain:
        return record_plain(args.record_plain)
    if not ref_import.reference_available():
        raise SystemExit("the reference is not present: this generator runs only next to it")
    gen(args.out, args.plain)


if __name__ == "__main__":
    main()
