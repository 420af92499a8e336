"""GPU: the native CLIP-vision encoder.  fmxv_clip_patch_rows_f16 (hipops.clip_patch_rows) bit for bit against the torch CPU expression of the
reference's clip_preprocess; fmxv_clip_embed_ln_f16 (hipops.clip_embed_ln) against an fp64 restatement in fp16 ulps; the preprocessing end to end
against the reference's 8-bit levels; the three towers (heads of 64 / 80 / 104) against transformers' CLIPVisionModelWithProjection in fp32 under
the floor-keyed gates of tests/parity.py (tests/golden/clipvision.pt, tools/make_clipvision_fixtures.py), with a NaN-filled arena and with the
second image exchanged; IP-Adapter from an image; Revision."""
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import forge_amd  # noqa: E402,F401
from forge_amd import hipops as ops  # noqa: E402
from forge_amd import synth  # noqa: E402
from forge_amd.backend.diffusion_engine.base import build_engine  # noqa: E402
from forge_amd.backend.patcher import clipvision as cv  # noqa: E402
from forge_amd.backend.patcher import revision as rev  # noqa: E402
from forge_amd.backend.patcher.ipadapter import patch_ipadapter  # noqa: E402
from forge_amd.modules import processing, shared  # noqa: E402
from forge_amd.modules.prompt_parser import DictWithShape  # noqa: E402

from conftest import load_golden  # noqa: E402
import clipvision_refs as R  # noqa: E402
import lllite_refs as L  # noqa: E402
import parity  # noqa: E402
from parity import check  # noqa: E402
from test_gpu_pag import engine_of  # noqa: E402

DEV = "cuda"
H16 = torch.float16
GUARD = 1024
NAN_BITS = 0x7E00
OUTPUTS = ("last_hidden_state", "penultimate_hidden_states", "image_embeds")


def bits(t):
    return t.contiguous().view(torch.int16)


def guarded(n):
    """-> (flat NaN-filled fp16 device buffer with GUARD elements on both sides, the window of n elements inside it)"""
    buf = torch.full((GUARD + n + GUARD,), float("nan"), dtype=H16, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf, n):
    b = bits(buf).cpu()
    return bool((b[:GUARD] == NAN_BITS).all()) and bool((b[GUARD + n:] == NAN_BITS).all())


# ---- the two kernels -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,rh,rw", R.PATCH_CASES)
def test_clip_patch_rows_bit_for_bit(b, rh, rw):
    """crop + quantise + normalise + im2col == torch's fp32 expression then .half(), every bit; the pad columns are +0; nothing around `out` is written"""
    x = R.patch_case(b, rh, rw)
    top, left = R.crop_of(rh, rw)
    want = R.patch_rows_ref(x, top, left)
    n = b * 256 * 640
    buf, win = guarded(n)
    got = ops.clip_patch_rows(x.to(DEV), top, left, out=win.view(b * 256, 640))
    torch.cuda.synchronize()
    got = got.cpu()
    assert torch.equal(bits(got), bits(want)), f"{int((bits(got) != bits(want)).sum())} of {n} elements differ"
    assert bool((bits(got)[:, 588:] == 0).all()) and guards_intact(buf, n)


@pytest.mark.parametrize("c,b,t_pad", R.EMBED_CASES)
def test_clip_embed_ln_vs_fp64_in_ulps(c, b, t_pad):
    """class token + patches + position embedding + pre_layrnorm against the fp64 restatement: within EMBED_GATE_ULPS = 2 fp16 ulps -- the worst
    distance of the kernel's own fp32 arithmetic from fp64 over these cases, measured on the CPU (1 ulp, tests/test_clipvision_host.py), plus one.
    The row with equal elements is beta; rows 257.. are +0 after a NaN prefill; the guards keep every bit."""
    operands = R.embed_case(c, b)
    want = R.embed_ref64(*operands, b, t_pad)
    n = b * t_pad * c
    buf, win = guarded(n)
    got = ops.clip_embed_ln(*(t.to(DEV) for t in operands), eps=R.EPS, rows_per_image=t_pad, out=win.view(b * t_pad, c))
    torch.cuda.synchronize()
    got = got.cpu().view(b, t_pad, c)
    dist = R.ulp_distance_f16(got, want)
    print(f"clip_embed_ln c {c} b {b} t_pad {t_pad}: worst {int(dist.max())} ulp, {float((dist > 0).float().mean()):.4f} of the elements off by one or more")
    assert bool(torch.isfinite(got).all()) and int(dist.max()) <= R.EMBED_GATE_ULPS
    img, tok = R.EQUAL_ROW
    assert torch.equal(bits(got[img, tok]), bits(operands[4]))
    assert bool((bits(got[:, 257:]) == 0).all()) and guards_intact(buf, n)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    g = load_golden("clipvision.pt")
    for name, floors in g["floor"].items():
        for out, v in floors.items():
            parity.FLOORS[f"clipvision.pt:{name}/{out}"] = v
    parity.FLOORS["clipvision.pt:ipadapter"] = g["ipadapter"]["floor"]
    g["levels"] = load_golden("clipvision_levels.pt")["levels"]
    g["image_tensors"] = [synth.synth_image(h, w, seed) for h, w, seed in g["images"]]
    return g


_models = {}


def model_of(fx, name):
    if name not in _models:
        t = fx["towers"][name]
        _models[name] = cv.ClipVisionModel(t["config"], synth.synth_clip_vision_state_dict(t["config"], seed=t["seed"]), DEV)
    return _models[name]


def levels_of(rows):
    """the 8-bit levels behind clip_patch_rows' output [256, 640] -> int [3, 224, 224] (fp16 keeps a level to 0.13 of a step)"""
    v = rows[:, :588].float().cpu().view(16, 16, 3, 14, 14).permute(2, 0, 3, 1, 4).reshape(3, 224, 224)
    return ((v * torch.tensor(R.STD).view(3, 1, 1) + torch.tensor(R.MEAN).view(3, 1, 1)) * 255.0).round().to(torch.int32)


def test_preprocessing_end_to_end_vs_the_references_levels(fx):
    """resize (antialiased bicubic, the existing separable kernel) + crop + quantise: the 224 x 224 image agrees exactly; the resized one in all but
    0.2 % of its pixels, and nowhere by more than one level -- ATen's own fp32 and fp64 resizes, quantised, disagree in 0.062 % of the pixels of this
    size: the quantisation is discontinuous"""
    assert [tuple(i[:2]) for i in fx["images"]] == [(224, 224), (300, 231)]
    exact = levels_of(cv.clip_preprocess(fx["image_tensors"][0].to(DEV)))
    assert torch.equal(exact, fx["levels"][0].to(torch.int32))
    x, top, left = cv.resized(fx["image_tensors"][1].to(DEV))
    assert tuple(x.shape) == (1, 3, 291, 224) and (top, left) == (33, 0)
    diff = (levels_of(cv.clip_preprocess(fx["image_tensors"][1].to(DEV))) - fx["levels"][1].to(torch.int32)).abs()
    frac = float((diff > 0).float().mean())
    print(f"preprocessing 300 x 231: {frac:.5%} of the pixels differ by one level, worst {int(diff.max())}")
    assert int(diff.max()) <= 1 and frac <= 0.002


def rows_of(fx, which):
    return torch.cat([cv.clip_preprocess(fx["image_tensors"][i].to(DEV)) for i in which])


def fixture_rows(fx, name, out, which):
    return fx["outputs"][name][out][list(which)]


def kept(fx, out, t):
    return t if out == "image_embeds" else t[:, ::fx["row_step"]]


@pytest.mark.parametrize("name", ["d64", "d80", "d104"])
def test_towers_vs_the_reference(fx, name):
    """both images as one batch, and the 300 x 231 image alone through encode_image, against the fp32 reference; then the same batch with every
    intermediate of the tower prefilled with NaN (CLIPVisionTower.allocator, the hook the tower documents): finite, within the same gates; then
    image 1 exchanged: image 0's outputs keep every bit"""
    m = model_of(fx, name)
    assert fx["row_step"] == 8 and m.tower.d == {"d64": 64, "d80": 80, "d104": 104}[name] and m.tower.dp == {"d64": 64, "d80": 80, "d104": 128}[name]
    both = m.encode_pixel_rows(rows_of(fx, (0, 1)))
    alone = m.encode_image(fx["image_tensors"][1].to(DEV))
    for out in OUTPUTS:
        assert both[out].dtype == torch.float32 and both[out].shape[0] == 2 and both[out].shape[1:] == ((257, m.tower.hidden) if out != "image_embeds" else (64,))
        check(f"clip-vision {name} {out}: batch of two", kept(fx, out, both[out]), fixture_rows(fx, name, out, (0, 1)), floor=f"clipvision.pt:{name}/{out}")
        check(f"clip-vision {name} {out}: 300 x 231 alone", kept(fx, out, alone[out]), fixture_rows(fx, name, out, (1,)), floor=f"clipvision.pt:{name}/{out}")
    # the padding rows: whatever the arena held before
    plain_alloc = m.tower.allocator
    m.tower.allocator = lambda shape, dtype=H16: torch.full(tuple(shape), float("nan"), dtype=dtype, device=DEV)
    try:
        poisoned = m.encode_pixel_rows(rows_of(fx, (0, 1)))
    finally:
        m.tower.allocator = plain_alloc
    for out in OUTPUTS:
        assert bool(torch.isfinite(poisoned[out]).all()), out
        check(f"clip-vision {name} {out}: NaN-filled arena", kept(fx, out, poisoned[out]), fixture_rows(fx, name, out, (0, 1)), floor=f"clipvision.pt:{name}/{out}")
        assert torch.equal(poisoned[out], both[out])
    # batch independence: the same launch shapes, another image 1
    other = cv.clip_preprocess(synth.synth_image(224, 224, 999).to(DEV))
    swapped = m.encode_pixel_rows(torch.cat([rows_of(fx, (0,)), other]))
    for out in OUTPUTS:
        assert torch.equal(swapped[out][0], both[out][0]), out
        assert not torch.equal(swapped[out][1], both[out][1])


# ---- IP-Adapter from an image ------------------------------------------------------------------------------------------------------------------------------
def test_ipadapter_from_an_image(fx, monkeypatch):
    """embeds=None + clip_vision + image gives bit for bit the unit of the tuple call on encode_image's own outputs (base: image_embeds and zeros; plus:
    penultimate_hidden_states of the image and of a black image, one batch through the tower); the end-to-end case against the reference; the
    encoder runs once, before the step, whose launches are those of the tuple form"""
    ip = fx["ipadapter"]
    cfg = dict(getattr(synth, ip["config"]))
    m = model_of(fx, ip["tower"])
    eng = engine_of(ip["config"], ip["weight_seed"])
    unet, km = eng.forge_objects.unet, eng.forge_objects.unet.model
    img = fx["image_tensors"][ip["image"]]
    base = synth.synth_ipadapter_state_dict(cfg, plus=False, seed=ip["file_seed"])
    encodes = []
    real_encode = m.tower.encode
    monkeypatch.setattr(m.tower, "encode", lambda rows: (encodes.append(rows.shape[0] // 256), real_encode(rows))[1])
    from_image = patch_ipadapter(unet, base, None, ip["weight"], ip["weight_type"], clip_vision=m, image=img)
    assert encodes == [1]
    e = m.encode_image(img.to(DEV)).image_embeds
    from_tuple = patch_ipadapter(unet, base, (e, torch.zeros_like(e)), ip["weight"], ip["weight_type"])
    ui, ut = (p.model_options["transformer_options"]["ipadapter"][0] for p in (from_image, from_tuple))
    assert all(torch.equal(a, b) for a, b in zip(ui.embeds, ut.embeds)) and all(torch.equal(a, b) for a, b in zip(ui.image_tokens(), ut.image_tokens()))
    check("clip-vision: image_embeds of the IP-Adapter case", e, ip["embeds"], floor=f"clipvision.pt:{ip['tower']}/image_embeds")
    # the preprocessor dict is the same call
    via_dict = patch_ipadapter(unet, base, dict(clip_vision=m, image=img, weight_type=ip["weight_type"], noise=0.0, embeds=None, unfold_batch=False), ip["weight"])
    assert torch.equal(via_dict.model_options["transformer_options"]["ipadapter"][0].embeds[0], ui.embeds[0])
    # a plus file at the tower's width: the black-image rows come from the tower, in the image's batch
    plus = synth.synth_ipadapter_state_dict(cfg, plus=True, seed=77, clip_dim=m.tower.hidden)
    del encodes[:]
    up = patch_ipadapter(unet, plus, None, 0.5, clip_vision=m, image=img).model_options["transformer_options"]["ipadapter"][0]
    assert encodes == [2]
    pair = m.encode_image(torch.cat([img, torch.zeros(1, 224, 224, 3)]).to(DEV)).penultimate_hidden_states
    assert torch.equal(up.embeds[0], pair[:1]) and torch.equal(up.embeds[1], pair[1:]) and float(up.embeds[1].abs().max()) > 0
    ut2 = patch_ipadapter(unet, plus, (pair[:1], pair[1:]), 0.5).model_options["transformer_options"]["ipadapter"][0]
    assert all(torch.equal(a, b) for a, b in zip(up.image_tokens(), ut2.image_tokens()))
    # end to end, and the launches of a call
    sig_host = km.predictor.sigma(torch.tensor(ip["t"]))
    x, cond, uncond = L.case_inputs(cfg, ip["hw"], ip["seed"], sig_host, ip["b"])
    as_ctx = lambda d: (d["crossattn"].to(DEV), d["vector"].to(DEV))  # noqa: E731
    x, sigma, c, uc = x.to(DEV), sig_host.float().to(DEV), as_ctx(cond), as_ctx(uncond)
    launches = []
    real_call = ops._call
    monkeypatch.setattr(ops, "_call", lambda name, *a: (launches.append(name), real_call(name, *a))[1])
    del encodes[:]
    counts = []
    try:
        for p in (from_image, from_tuple):
            to = p.model_options["transformer_options"]
            km.denoise_cfg(x, sigma, uc, c, ip["cfg"], transformer_options=to)          # prepares the unit's K / V
            del launches[:]
            den = km.denoise_cfg(x, sigma, uc, c, ip["cfg"], transformer_options=to).clone()
            counts.append(list(launches))
            check("ipadapter from an image vs the reference" if p is from_image else "ipadapter from the tuple vs the reference", den, ip["result"],
                  floor="clipvision.pt:ipadapter")
    finally:
        km._drop_graphs()
        km._static.clear()
    assert counts[0] == counts[1] and not any(n.startswith("fmxv_") for n in counts[0]) and encodes == []
    plain = km.denoise_cfg(x, sigma, uc, c, ip["cfg"]).clone()
    km._drop_graphs()
    km._static.clear()
    assert parity.metrics(plain, ip["result"])["rms_rel"] > 10 * ip["floor"]["rms_rel"]


# ---- Revision --------------------------------------------------------------------------------------------------------------------------------------------------
REVISION_CONFIG = dict(synth.TINY_SDXL_UNET_CONFIG, adm_in_channels=2816)


@pytest.fixture(scope="module")
def revision_engine():
    return build_engine(REVISION_CONFIG, synth.synth_unet_state_dict(REVISION_CONFIG, seed=3), None, None, device=DEV)


def run_job(eng, unet, c, uc, steps=2):
    saved = eng.forge_objects_after_applying_lora
    eng.forge_objects_after_applying_lora = saved.shallow_copy()
    eng.forge_objects_after_applying_lora.unet = unet
    try:
        move = lambda d: DictWithShape({k: v.to(DEV) for k, v in d.items()})  # noqa: E731
        shared.opts.randn_source = "CPU"
        p = processing.StableDiffusionProcessingTxt2Img(sd_model=eng, c=move(c), uc=move(uc), seed=4321, sampler_name="Euler", batch_size=2, steps=steps,
                                                        cfg_scale=7.0, width=256, height=256, do_decode=False)
        return processing.process_images(p).latents.clone()
    finally:
        eng.forge_objects_after_applying_lora = saved
        eng.forge_objects = saved.shallow_copy()


def test_revision_on_the_tiny_sdxl_engine(fx, revision_engine, monkeypatch):
    """patch_revision with the fixture's units on the fixture's `y`: the y that reaches the UNet is the reference modifier's, to one fp16 ulp; the
    context is zeroed when a unit ignores the prompt; a unit of weight 0 gives the plain job with the first 1280 columns of y zeroed"""
    eng = revision_engine
    r = fx["revision"]
    g = torch.Generator().manual_seed(r["seed"])
    y, uy = torch.randn(1, 2816, generator=g), torch.randn(1, 2816, generator=g)
    c, uc = synth.synth_conditioning(2, REVISION_CONFIG["context_dim"], 2816, seed=77)
    c, uc = dict(c, vector=y.repeat(2, 1)), dict(uc, vector=uy.repeat(2, 1))
    km = eng.forge_objects.unet.model
    seen = []
    real = km.denoise_cfg
    monkeypatch.setattr(km, "denoise_cfg", lambda x, s, uctx, cctx, *a, **kw: (seen.append((cctx, uctx)), real(x, s, uctx, cctx, *a, **kw))[1])
    embeds = lambda seed: {"image_embeds": torch.randn(1, 1280, generator=torch.Generator().manual_seed(seed)).to(DEV)}  # noqa: E731
    results = []
    for case in r["cases"]:
        unet = eng.forge_objects.unet
        for seed, weight, ignore in case["units"]:
            unet = rev.patch_revision(unet, embeds(seed), weight, 0.0, ignore)
        del seen[:]
        results.append(run_job(eng, unet, c, uc))
        assert len(seen) == 2 and seen[0][0][1] is seen[1][0][1] and seen[0][0][0] is seen[1][0][0], "the same tensors step after step"
        (cctx, cy), (uctx, uy_got) = seen[0][0][:2], seen[0][1][:2]          # (context, y[, guidance])
        for got, want in ((cy, case["y"]), (uy_got, case["uncond_y"])):
            assert got.shape == (2, 2816) and int(R.ulp_distance_f16(got.cpu().float(), want.expand(2, -1)).max()) <= 1
        ignore = any(u[2] for u in case["units"])
        assert (not bool(cctx.any()) and not bool(uctx.any())) if ignore else torch.equal(cctx.cpu().float(), c["crossattn"])
    assert not torch.equal(results[0], results[1]) and not torch.equal(results[0], results[2])
    zero_weight = run_job(eng, rev.patch_revision(eng.forge_objects.unet, embeds(901), 0.0, 0.0, False), c, uc)
    zeroed = lambda d: dict(d, vector=torch.cat([torch.zeros(2, 1280), d["vector"][:, 1280:]], 1))  # noqa: E731
    plain = run_job(eng, eng.forge_objects.unet, zeroed(c), zeroed(uc))
    assert torch.equal(zero_weight, plain) and not torch.equal(zero_weight, results[0])
