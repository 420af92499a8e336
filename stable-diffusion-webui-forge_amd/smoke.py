"""`__graft_entry__.smoke()`: one small invocation of the hot path on cuda:0 (CFG step through the Forge call surface:
CFGDenoiser -> UNet -> sampler update -> VAE decode), checked against the CPU oracle -- end to end at the fp16 floor, and the UNet layer by layer
against the rounding oracle at the sharp gate."""
import os
import sys

import torch


def run():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    from forge_amd import _lib, synth
    from forge_amd.backend.diffusion_engine.base import build_engine
    from forge_amd.modules import processing
    from oracle import pipeline  # checker only
    assert torch.cuda.is_available(), "smoke() needs the MI355X"
    _lib.lib()
    cfg = synth.TINY_SD15_UNET_CONFIG
    sd = synth.synth_unet_state_dict(cfg, seed=0)
    vsd = synth.synth_vae_decoder_state_dict(synth.TINY_VAE_CONFIG, seed=1)
    eng = build_engine(cfg, sd, synth.TINY_VAE_CONFIG, vsd, device="cuda:0")
    c, uc = synth.synth_conditioning(2, cfg["context_dim"], None, seed=1234)
    p = processing.StableDiffusionProcessingTxt2Img(sd_model=eng, c=c.cuda(), uc=uc.cuda(), seed=3, sampler_name="Euler", batch_size=2,
                                                    steps=3, width=128, height=128)
    res = processing.process_images(p)
    lat, dec, img = pipeline.txt2img(sd, cfg, vsd, synth.TINY_VAE_CONFIG, c, uc, [3, 4], 128, 128, 3, sampler_name="Euler")
    def rel(a, ref):
        d = (a.double().cpu() - ref.double())
        return float(d.abs().max() / ref.abs().max()), float(d.pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt())
    (m1, r1), (m2, r2) = rel(res.latents, lat), rel(res.decoded, dec)
    # the yard-stick: what the REAL reference loses when it runs this same job in its own fp16 mode instead of fp32
    # (oracle/make_floor.py floors_pipeline -> tests/golden/fp16_floor.json); the north star's 1e-3 applies where that floor is below it.
    # The gate is the RMS error (a stable statistic: 1.25 x the floor, as tests/parity.py); the maximum over a 2-image job is one draw of an
    # extreme-value statistic -- round 2's smoke sat at 1.46 x the floor's maximum against a 1.5 x limit with the rms BELOW the floor -- so
    # it only has to stay within 2 x (a wrong kernel is off by orders of magnitude in both).
    import json
    fl = json.load(open(os.path.join(root, "tests", "golden", "fp16_floor.json")))
    ok = True
    for what, m, r in (("latent", m1, r1), ("decoded", m2, r2)):
        f = fl["pipeline:smoke_euler3/" + what]
        lm, lr = max(1e-3, 2.0 * f["max_rel"]), max(1e-3, 1.25 * f["rms_rel"])
        print(f"smoke: {what} rms_rel {r:.3e} (reference fp16-vs-fp32 floor {f['rms_rel']:.3e}, limit {lr:.2e}), "
              f"max_rel {m:.3e} (floor {f['max_rel']:.3e}, limit {lm:.2e})")
        ok = ok and r <= lr and m <= lm
    assert ok, "smoke parity outside the fp16 floor"
    # ... and the SHARP check (round 5; tests/test_gpu_sharp_parity.py at full size): one forward of the same UNet with every stored tensor handed out,
    # the rounding oracle (oracle/unet_fp16sites.py: the restatement with fp16 rounding at the executor's storage sites) replayed teacher-forced on them,
    # every layer within 2e-4 rms (attention outputs 7.5e-4) and 2.5 fp16 ulps per element -- a wrong constant in ONE layer fails here, not under the floor
    from oracle import unet_fp16sites as o16  # checker only
    net = eng.forge_objects.unet.model.diffusion_model
    g = torch.Generator("cpu").manual_seed(7)
    x, t, ctx = torch.randn(2, cfg["in_channels"], 16, 16, generator=g), torch.tensor([801.0, 37.0]), torch.randn(2, 77, cfg["context_dim"], generator=g)
    taps = {}
    net.tap = lambda name, tens: taps.__setitem__(name, tens.detach().to("cpu", copy=True))
    try:
        net.forward(x.cuda(), t.cuda(), context=ctx.cuda(), y=None)
    finally:
        net.tap = None
    outs, nat = {}, {}
    o16.unet_forward(sd, cfg, x, t, ctx, None, fold=dict(net.fold_trace), teacher=taps, layer_out=outs, native_view=nat, up2x=net.up2x_trace)
    worst_rms = worst_pp = 0.0
    bad = []
    for key, ref in outs.items():
        if key not in nat:
            continue
        d = (nat[key].double() - ref.double())
        rms_ref = float(ref.double().pow(2).mean().sqrt())
        rms = float(d.pow(2).mean().sqrt()) / max(rms_ref, 1e-30)
        pp = float((d.abs() / torch.clamp(ref.double().abs(), min=rms_ref)).max())
        worst_rms, worst_pp = max(worst_rms, rms), max(worst_pp, pp)
        if rms > (7.5e-4 if key.endswith((".attn1.o", ".attn2.o")) else 2e-4) or pp > 2.5e-3:   # (attention outputs: measured 1.5e-4 .. 3.5e-4, one draw here)
            bad.append((key, rms, pp))
    print(f"smoke: {len(outs)} UNet layers against the rounding oracle, layer by layer: worst rms_rel {worst_rms:.2e}, worst per-pixel {worst_pp:.2e}")
    assert len(outs) > 100 and not bad, f"layer-wise parity outside the sharp gate: {bad[:4]}"
    # the CLIP-vision encoder (backend/patcher/clipvision.py): a seeded 224 x 224 image through the tiny tower with heads of 80
    from forge_amd.backend.patcher.clipvision import ClipVisionModel
    vcfg = synth.TINY_CLIP_VISION_CONFIGS["d80"]
    emb = ClipVisionModel(vcfg, synth.synth_clip_vision_state_dict(vcfg), "cuda:0").encode_image(synth.synth_image(224, 224, 5)).image_embeds
    assert bool(torch.isfinite(emb).all())
    print("smoke: clip-vision image_embeds rms %.4f" % float(emb.pow(2).mean().sqrt()))
    print("smoke OK")
