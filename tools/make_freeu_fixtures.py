"""TEST INFRASTRUCTURE ONLY.  Generates tests/golden/freeu_ops.pt and tests/golden/tiny_freeu_unet.pt with the REAL reference: its FreeU script
(<reference>/extensions-builtin/sd_forge_freeu/scripts/forge_freeu.py) and, through oracle.ref_import, its UNet, sampling_function and Euler
sampler.  Runs only where the reference exists; deterministic (seeded).  Only tensors and settings are written.

    python tools/make_freeu_fixtures.py [--out tests/golden]

The FreeU script imports gradio and the web UI at module level, so it is not imported: the file is parsed and the two function definitions
`Fourier_filter` and `patch_freeu_v2` are compiled from its syntax tree, at run time, into a namespace that holds torch and a stand-in
`FreeUForForge` with the `doFreeU` switch the patch reads.

freeu_ops.pt      cases: [{shape (n, C_h, C_s, H, W), seed, checksum, b, s, rule ("4x" | "2x": which entry of the reference's scale table the
                  case goes through), h_out, hsp_out (the reference output_block_patch's fp32 outputs on the fp16-rounded inputs of
                  tests/freeu_refs.py case_inputs; for the large case only the channels listed in h_channels / hsp_channels)}]
                  The inputs are NOT stored (file size): tests re-draw them from `seed` with torch's CPU generator and compare `checksum`
                  (the exact fp64 sums).  A torch release that changes randn's CPU stream therefore makes the tests that use this file
                  fail at that assertion, not skip: regenerate the fixture with that torch.  The 48 x 40 case pins the closed form to the
                  reference on 19 / 17 of its channels only; the kernels are still checked against fp64 on all of them.
tiny_freeu_unet.pt  config (TINY_SD15_UNET_CONFIG with channel_mult (1, 2, 4)), params, x, t, ctx, eps_plain, eps_freeu (reference UNet, fp32),
                  floor / floor_plain (the reference's own fp16-storage run of the patched / plain forward against its fp32 run, by oracle/make_floor.py's
                  half_unet),
                  euler4: {seeds, hw, steps, start, end, active (per step), latent, floor}
"""
import argparse
import ast
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import forge_amd  # noqa: E402,F401
from forge_amd import synth  # noqa: E402
from oracle import ref_import  # noqa: E402

OPS_CASES = [  # (n, C_h, C_s, H, W), b, s, rule
    ((2, 64, 64, 2, 2), 1.3, 0.9, "4x"),
    ((1, 128, 64, 5, 7), 1.4, 0.2, "2x"),
    ((2, 128, 192, 8, 8), 1.2, 1.5, "4x"),
    ((1, 64, 32, 6, 3), 1.4, 0.2, "2x"),
    ((1, 256, 128, 48, 40), 1.3, 0.9, "4x"),
]
PARAMS = dict(b1=1.3, b2=1.4, s1=0.9, s2=0.2)   # the SDXL preset
WINDOW = dict(start=0.0, end=0.34)
FULL_OUTPUT_LIMIT = 1 << 16     # elements; above it the outputs are recorded on a channel subset (fixture size)


def reference_freeu():
    """-> (Fourier_filter, patch_freeu_v2, switch) compiled from the reference file's syntax tree; switch.doFreeU is what the patch reads"""
    path = os.path.join(ref_import.REFERENCE_ROOT, "extensions-builtin", "sd_forge_freeu", "scripts", "forge_freeu.py")
    tree = ast.parse(open(path).read(), filename=path)
    wanted = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("Fourier_filter", "patch_freeu_v2")]
    assert len(wanted) == 2, [n.name for n in wanted]
    switch = SimpleNamespace(doFreeU=True)
    ns = {"torch": torch, "FreeUForForge": switch}
    exec(compile(ast.Module(body=wanted, type_ignores=[]), path, "exec"), ns)
    return ns["Fourier_filter"], ns["patch_freeu_v2"], switch


class _FakePatcher:
    """what patch_freeu_v2 touches of a UnetPatcher: the model's config, clone(), set_model_output_block_patch()"""

    def __init__(self, model_channels):
        self.model = SimpleNamespace(diffusion_model=SimpleNamespace(config={"model_channels": model_channels}))
        self.patch = None

    def clone(self):
        return self

    def set_model_output_block_patch(self, fn):
        self.patch = fn


def gen_ops(out_dir):
    from freeu_refs import case_inputs, freeu_ref
    _, patch_freeu_v2, _ = reference_freeu()
    cases = []
    for i, (shape, b, s, rule) in enumerate(OPS_CASES):
        case = {"shape": shape, "seed": 4100 + i, "b": b, "s": s, "rule": rule}
        h, hsp = case_inputs(case)
        case["checksum"] = (float(h.double().sum()), float(hsp.double().sum()))
        c_h = shape[1]
        fp = _FakePatcher(c_h // 4 if rule == "4x" else c_h // 2)
        other = (7.0, 7.0)    # the scales of the rule the case does not go through: must not matter
        args = (b, other[0], s, other[1]) if rule == "4x" else (other[0], b, other[1], s)
        patch_freeu_v2(fp, *args)
        with torch.no_grad():
            h_out, hsp_out = fp.patch(h.clone(), hsp.clone(), {})
        assert h_out.dtype == torch.float32 and hsp_out.dtype == torch.float32
        mine = freeu_ref(h, hsp, b, s)
        print(shape, "closed form vs reference: h", float((mine[0] - h_out).abs().max() / h_out.abs().max()),
              "hsp", float((mine[1] - hsp_out).abs().max() / hsp_out.abs().max()))
        if h_out.numel() > FULL_OUTPUT_LIMIT:
            case["h_channels"] = list(range(0, c_h, 16)) + [c_h // 2 - 1, c_h // 2, c_h - 1]
            case["hsp_channels"] = list(range(0, shape[2], 8)) + [shape[2] - 1]
            h_out, hsp_out = h_out[:, case["h_channels"]].clone(), hsp_out[:, case["hsp_channels"]].clone()
        case["h_out"], case["hsp_out"] = h_out, hsp_out
        cases.append(case)
    torch.save({"cases": cases}, os.path.join(out_dir, "freeu_ops.pt"))


def tiny_config():
    return dict(synth.TINY_SD15_UNET_CONFIG, channel_mult=(1, 2, 4))


def gen_unet(out_dir, b=2, hw=16, steps=4):
    from oracle import make_golden as mg
    from oracle import make_floor as mf
    _, patch_freeu_v2, switch = reference_freeu()
    cfg = tiny_config()
    sd = synth.synth_unet_state_dict(cfg, seed=0)
    net = ref_import.build_ref_unet(cfg, sd)
    net.config = dict(cfg)   # the reference's loader attaches the config to the model; patch_freeu_v2 reads model_channels from it
    ref = ref_import.load_reference()
    pred = ref_import.build_ref_predictor()
    g = torch.Generator().manual_seed(77)
    x = torch.randn(b, cfg["in_channels"], hw, hw, generator=g)
    t = torch.tensor([601.0, 187.0])[:b]
    ctx = torch.randn(b, 77, cfg["context_dim"], generator=g)

    def patched_options(network):
        den = ref_import.RefDenoiser(network, pred, [0])
        return patch_freeu_v2(den.patcher, PARAMS["b1"], PARAMS["b2"], PARAMS["s1"], PARAMS["s2"]).model_options["transformer_options"]

    switch.doFreeU = True
    with torch.no_grad():
        eps_plain = net(x, t, context=ctx, transformer_options={})
        eps_freeu = net(x, t, context=ctx, transformer_options=patched_options(net))
    res = {"config": cfg, "params": dict(PARAMS), "x": x, "t": t, "ctx": ctx, "eps_plain": eps_plain, "eps_freeu": eps_freeu}
    print("forward: FreeU moves eps by", float((eps_freeu - eps_plain).abs().max() / eps_plain.abs().max()))
    # the reference's own fp16-storage run of the patched forward (oracle/make_floor.py's mechanism, called as it is)
    net16 = mf.half_unet(cfg, sd)
    net16.config = dict(cfg)
    with torch.no_grad():
        e16 = net16(x.half(), t, context=ctx.half(), transformer_options=patched_options(net16)).float()
    res["floor"] = mf.metrics(e16, eps_freeu)
    with torch.no_grad():
        res["floor_plain"] = mf.metrics(net16(x.half(), t, context=ctx.half(), transformer_options={}).float(), eps_plain)
    print("forward fp16 floor", res["floor"])

    def euler(network):
        c, uc = synth.synth_conditioning(b, cfg["context_dim"], None, seed=1234)
        seeds = [1000 + i for i in range(b)]
        den = ref_import.RefDenoiser(network, pred, seeds)
        den.patcher = patch_freeu_v2(den.patcher, PARAMS["b1"], PARAMS["b2"], PARAMS["s1"], PARAMS["s2"])
        den.inner_model.inner_model.forge_objects.unet = den.patcher
        active = []

        class Windowed:
            """sets the reference's doFreeU switch before every model call, by the expression of its denoiser_callback"""
            inner_model = den.inner_model

            def __call__(self, xx, sigma, **kw):
                this_step = den.step / (steps - 1)
                switch.doFreeU = bool(this_step >= WINDOW["start"] and this_step <= WINDOW["end"])
                active.append(switch.doFreeU)
                return den(xx, sigma, **kw)

        rng = mg.ImageRNG((cfg["in_channels"], hw, hw), seeds, "CPU")
        xx = rng.next()
        sigmas = den.inner_model.get_sigmas(steps)
        xx = pred.noise_scaling(sigmas[0], xx, torch.zeros_like(xx), max_denoise=False)
        ref.kd_sampling.torch = mg._Hijack(rng)
        ref.sampling_function.sampling_prepare(den.patcher, x=xx)
        try:
            lat = ref.kd_sampling.sample_euler(Windowed(), xx, sigmas, extra_args={"cond": c, "uncond": uc, "cond_scale": 7.0, "s_min_uncond": 0.0,
                                                                                  "image_cond": None}, disable=True)
        finally:
            ref.kd_sampling.torch = torch
            ref.sampling_function.sampling_cleanup(den.patcher)
            switch.doFreeU = True
        return lat, seeds, active

    lat, seeds, active = euler(net)
    lat16, _, _ = euler(net16)
    res["euler4"] = {"seeds": seeds, "hw": hw, "steps": steps, "start": WINDOW["start"], "end": WINDOW["end"], "active": active, "latent": lat,
                     "floor": mf.metrics(lat16.float(), lat)}
    print("euler4: active", active, "latent std", float(lat.std()), "fp16 floor", res["euler4"]["floor"])
    torch.save(res, os.path.join(out_dir, "tiny_freeu_unet.pt"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--only", choices=["ops", "unet"])
    args = ap.parse_args()
    if not ref_import.reference_available():
        raise SystemExit("the reference is not present: this generator runs only next to it")
    if args.only != "unet":
        gen_ops(args.out)
    if args.only != "ops":
        gen_unet(args.out)


if __name__ == "__main__":
    main()
