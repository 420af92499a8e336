"""TEST INFRASTRUCTURE ONLY.  Generates tests/golden/tiny_kohya_unet.pt with the REAL reference: its Kohya HRFix script
(<reference>/extensions-builtin/sd_forge_kohya_hrfix/scripts/kohya_hrfix.py) and, through oracle.ref_import, its adaptive_resize, UNet,
sampling_function and Euler sampler.  Runs only where the reference exists; deterministic (seeded).  Only tensors and settings are written.

    python tools/make_kohya_fixtures.py [--out tests/golden]

The script imports gradio and the web UI at module level, so it is not imported: the file is parsed and the class definition
`PatchModelAddDownscale` is compiled from its syntax tree, at run time, into a namespace that holds the reference's own `adaptive_resize`
(backend/misc/image_resize.py) and a stand-in `shared` for the two side globals the patches write.

tiny_kohya_unet.pt  config (TINY_SD15_UNET_CONFIG), x [2, 4, 32, 24], t, sigmas (the predictor's sigma of t: what the patch reads as
                    transformer_options["sigmas"]), ctx, eps_plain, floor_plain,
                    cases: [{block_number, downscale_factor, downscale_after_skip, downscale_method, upscale_method, start_percent, end_percent,
                             eps (reference UNet with the reference's patches, fp32), floor (the reference's own fp16-storage run of that patched
                             forward against its fp32 run, by oracle/make_floor.py's half_unet), resized: [(where, block, (H, W) after)]}]
                    euler4: {seeds, hw, steps, params, active (per step), latent, floor}
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

# (block_number, downscale_factor, downscale_after_skip, downscale_method, upscale_method)
CASES = [
    (2, 2.0, True, "bicubic", "bicubic"),
    (2, 1.5, True, "bicubic", "bicubic"),
    (1, 2.0, False, "bilinear", "nearest-exact"),
    (3, 1.5, True, "area", "bilinear"),
]
EULER = dict(block_number=2, downscale_factor=2.0, start_percent=0.0, end_percent=0.5, downscale_after_skip=True, downscale_method="bicubic",
             upscale_method="bicubic")    # 4 steps at t = 999, 666, 333, 0: percent 0.5 ends the window between the second and the third


def reference_patch():
    """-> PatchModelAddDownscale() compiled from the reference file's syntax tree, with the reference's adaptive_resize"""
    ref_import.load_reference()
    from backend.misc.image_resize import adaptive_resize    # the reference's, importable once load_reference has set the path
    path = os.path.join(ref_import.REFERENCE_ROOT, "extensions-builtin", "sd_forge_kohya_hrfix", "scripts", "kohya_hrfix.py")
    tree = ast.parse(open(path).read(), filename=path)
    wanted = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "PatchModelAddDownscale"]
    assert len(wanted) == 1
    ns = {"adaptive_resize": adaptive_resize, "shared": SimpleNamespace()}
    exec(compile(ast.Module(body=wanted, type_ignores=[]), path, "exec"), ns)
    return ns["PatchModelAddDownscale"]()


def record_resizes(patcher, log, tag=lambda: None):
    """wrap the installed patch closures: note (tag, where, block, size after) whenever one returns h at another size"""
    patches = patcher.model_options["transformer_options"]["patches"]

    def wrap(fn):
        def w(*a):
            before = tuple(a[0].shape[-2:])
            r = fn(*a)
            h = r[0] if isinstance(r, tuple) else r
            if tuple(h.shape[-2:]) != before:
                log.append((tag(), a[-1]["block"][0], int(a[-1]["block"][1]), tuple(h.shape[-2:])))
            return r
        return w
    for name in list(patches):
        patches[name] = [wrap(f) for f in patches[name]]


def gen(out_dir, b=2, steps=4, hw=16):
    from oracle import make_golden as mg
    from oracle import make_floor as mf
    op = reference_patch()
    cfg = dict(synth.TINY_SD15_UNET_CONFIG)
    sd = synth.synth_unet_state_dict(cfg, seed=0)
    net, net16 = ref_import.build_ref_unet(cfg, sd), mf.half_unet(cfg, sd)
    ref = ref_import.load_reference()
    pred = ref_import.build_ref_predictor()
    g = torch.Generator().manual_seed(78)
    x = torch.randn(b, cfg["in_channels"], 32, 24, generator=g)
    t = torch.tensor([601.0, 187.0])[:b]
    sigmas = pred.sigma(t)
    ctx = torch.randn(b, 77, cfg["context_dim"], generator=g)

    def options(network, params, log):
        den = ref_import.RefDenoiser(network, pred, [0])
        m = op.patch(den.patcher, *params)[0]
        record_resizes(m, log)
        return dict(m.model_options["transformer_options"], sigmas=sigmas)

    with torch.no_grad():
        eps_plain = net(x, t, context=ctx, transformer_options={})
        res = {"config": cfg, "x": x, "t": t, "sigmas": sigmas, "ctx": ctx, "eps_plain": eps_plain,
               "floor_plain": mf.metrics(net16(x, t, context=ctx, transformer_options={}), eps_plain), "cases": []}
        for blk, factor, after, down, up in CASES:
            params = (blk, factor, 0.0, 1.0, after, down, up)      # the window open at every sigma
            log, log16 = [], []
            eps = net(x, t, context=ctx, transformer_options=options(net, params, log))
            e16 = net16(x, t, context=ctx, transformer_options=options(net16, params, log16))
            assert log == log16 and log
            case = dict(block_number=blk, downscale_factor=factor, start_percent=0.0, end_percent=1.0, downscale_after_skip=after,
                        downscale_method=down, upscale_method=up, eps=eps, floor=mf.metrics(e16, eps), resized=[e[1:] for e in log])
            print(params, "moves eps by", float((eps - eps_plain).abs().max() / eps_plain.abs().max()), "resized", case["resized"], "floor", case["floor"])
            res["cases"].append(case)

    def euler(network):
        c, uc = synth.synth_conditioning(b, cfg["context_dim"], None, seed=1234)
        seeds = [1000 + i for i in range(b)]
        den = ref_import.RefDenoiser(network, pred, seeds)
        e = EULER
        den.patcher = op.patch(den.patcher, e["block_number"], e["downscale_factor"], e["start_percent"], e["end_percent"], e["downscale_after_skip"],
                               e["downscale_method"], e["upscale_method"])[0]
        log = []
        record_resizes(den.patcher, log, tag=lambda: den.step)
        den.inner_model.inner_model.forge_objects.unet = den.patcher
        rng = mg.ImageRNG((cfg["in_channels"], hw, hw), seeds, "CPU")
        xx = rng.next()
        sg = den.inner_model.get_sigmas(steps)
        xx = pred.noise_scaling(sg[0], xx, torch.zeros_like(xx), max_denoise=False)
        ref.kd_sampling.torch = mg._Hijack(rng)
        ref.sampling_function.sampling_prepare(den.patcher, x=xx)
        try:
            lat = ref.kd_sampling.sample_euler(den, xx, sg, extra_args={"cond": c, "uncond": uc, "cond_scale": 7.0, "s_min_uncond": 0.0,
                                                                         "image_cond": None}, disable=True)
        finally:
            ref.kd_sampling.torch = torch
            ref.sampling_function.sampling_cleanup(den.patcher)
        shrunk_steps = {e[0] for e in log if e[1] == "input"}
        return lat, seeds, [i in shrunk_steps for i in range(steps)], [float(v) for v in sg]

    with torch.no_grad():
        lat, seeds, active, sg = euler(net)
        lat16, _, active16, _ = euler(net16)
    assert active == active16
    res["euler4"] = {"seeds": seeds, "hw": hw, "steps": steps, "params": dict(EULER), "active": active, "sigmas": sg, "latent": lat,
                     "floor": mf.metrics(lat16.float(), lat)}
    print("euler4: active", active, "sigmas", sg, "latent std", float(lat.std()), "fp16 floor", res["euler4"]["floor"])
    path = os.path.join(out_dir, "tiny_kohya_unet.pt")
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
