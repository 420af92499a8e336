"""TEST INFRASTRUCTURE ONLY.  Generates tests/golden/clipvision.pt and tests/golden/clipvision_levels.pt with the REAL reference: its
backend/patcher/clipvision.py (clip_preprocess, convert_to_transformers) on transformers' CLIPVisionModelWithProjection -- the class the reference
instantiates -- its IP-Adapter library and sampling_function (through tools/make_ipadapter_fixtures.py and oracle.ref_import) and its
revision_conditioning_modifier.  Runs only where the reference exists; deterministic (seeded).  Only tensors and settings are written.

    python tools/make_clipvision_fixtures.py [--out tests/golden]

clipvision.pt
    towers: {name: {config, seed}} for synth.TINY_CLIP_VISION_CONFIGS (heads of 64 / 80 / 104, 2 layers); weights are drawn from the seed
            (synth.synth_clip_vision_state_dict), not stored
    images: [(h, w, seed)]: synth.synth_image -- 224 x 224 and 300 x 231 (resized to 291 x 224, crop top 33)
    outputs: {name: {image_embeds [2, 64] in full; last_hidden_state, penultimate_hidden_states [2, 33, c]: the token rows ::8 (row 0 included)}} of
             the fp32 model on the reference's own clip_preprocess of the two images, as one batch
    floor: {name: {output: the same model in fp16 on the CPU against its fp32 run (oracle.make_floor.metrics)}}
    separation: {name: {variant: rms distance of a WRONG variant from the right last_hidden_state}} -- asserted here to be >= 10 x the floor
    geometry: {(h, w): (resized h, resized w, top, left)} observed from the reference's clip_preprocess
    converted: {key: (shape, sha256 of the fp32 bytes)} of the reference's convert_to_transformers on synth.openclip_keyed(weights of "d80")
    ipadapter: one end-to-end case -- sampling_function on TINY_SDXL_2LEVEL_UNET_CONFIG at CFG 7 with a base unit whose embeddings are the image_embeds of
               image 0 through the "d80" tower; built as tools/make_ipadapter_fixtures.py builds its cases: result, plain, floor, moved
    revision: cases of the reference's revision_conditioning_modifier on a seeded SDXL `y` [1, 2816] and a context [1, 7, 8]: units (seed, weight, ignore_prompt),
              y / c_crossattn of the cond and the uncond entries after the modifier
clipvision_levels.pt
    levels: [uint8 [3, 224, 224]] per image: the reference's preprocessed pixels as 8-bit levels (a file of its own: two of these and the token rows
            together exceed the size limit of one committed file)
"""
import argparse
import contextlib
import hashlib
import importlib
import io
import os
import sys
import types

import torch
from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection      # before oracle.ref_import stubs the packages transformers probes for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import forge_amd  # noqa: E402,F401
from forge_amd import synth  # noqa: E402
from forge_amd.backend.nn import ipadapter as nets  # noqa: E402
from forge_amd.backend.nn.layout import unet_layout  # noqa: E402
from oracle import ref_import  # noqa: E402
import lllite_refs as L  # noqa: E402

TOWER_SEEDS = {"d64": 171, "d80": 172, "d104": 173}
IMAGES = [(224, 224, 501), (300, 231, 502)]
GEOMETRY_SHAPES = [(224, 224), (300, 231), (512, 768), (225, 224), (224, 1000)]
ROW_STEP = 8
SEPARATION = 10.0
MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
IPA = dict(config="TINY_SDXL_2LEVEL_UNET_CONFIG", tower="d80", image=0, file_seed=31, weight=0.8, weight_type="original", weight_seed=0, seed=611, hw=(32, 32), b=2,
           t=[601.0, 187.0], cfg=7.0)
REVISION_CASES = [[(901, 0.7, False)], [(901, 0.7, False), (902, 0.4, False)], [(903, 1.2, True)]]
REVISION_SEED = 77


def rms_rel(a, ref):
    return float((a.double() - ref.double()).pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt())


def build_model(cfg, sd, dtype=torch.float32, **over):
    keys = ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "hidden_act", "projection_dim", "image_size", "patch_size",
            "num_channels", "layer_norm_eps")
    config = CLIPVisionConfig(**dict({k: cfg[k] for k in keys}, **over))
    model = CLIPVisionModelWithProjection(config)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    return model.to(dtype).eval()


def run(model, pixels):
    out = model(pixel_values=pixels.to(next(model.parameters()).dtype), output_hidden_states=True)
    return {"last_hidden_state": out.last_hidden_state.float(), "penultimate_hidden_states": out.hidden_states[-2].float(), "image_embeds": out.image_embeds.float()}


def class_token_last(model, pixels):
    """a WRONG variant: the class token appended behind the patches instead of in front"""
    vm = model.vision_model
    emb = vm.embeddings
    patches = emb.patch_embedding(pixels).flatten(2).transpose(1, 2)
    x = torch.cat([patches, emb.class_embedding.expand(pixels.shape[0], 1, -1)], dim=1) + emb.position_embedding.weight
    return vm.encoder(inputs_embeds=vm.pre_layrnorm(x)).last_hidden_state


def observed_geometry(ref_cv, h, w):
    """what the reference's clip_preprocess does to an h x w image: the size it asks the resize for, and the crop offsets, read off a marker pixel"""
    seen = {}
    real = torch.nn.functional.interpolate

    def fake(image, size, **kw):
        seen["size"] = tuple(int(s) for s in size)
        out = torch.zeros(image.shape[:2] + seen["size"])
        out[..., size[0] // 2, size[1] // 2] = 1.0
        return out
    torch.nn.functional.interpolate = fake
    try:
        img = torch.zeros(1, h, w, 3)
        if (h, w) == (224, 224):
            img[0, 112, 112] = 1.0
        out = ref_cv.clip_preprocess(img)
    finally:
        torch.nn.functional.interpolate = real
    rh, rw = seen.get("size", (h, w))
    at = int(out[0, 0].argmax())
    return rh, rw, rh // 2 - at // 224, rw // 2 - at % 224


def reference_revision():
    for name, attrs in (("modules_forge.supported_preprocessor", dict(PreprocessorClipVision=object, PreprocessorParameter=lambda **kw: None)),
                        ("modules_forge.shared", dict(add_supported_preprocessor=lambda p: None))):
        m = sys.modules.get(name) or types.ModuleType(name)
        for k, v in attrs.items():
            if not hasattr(m, k):
                setattr(m, k, v)
        sys.modules[name] = m
    if "modules_forge" not in sys.modules:
        sys.modules["modules_forge"] = types.ModuleType("modules_forge")
    path = os.path.join(ref_import.REFERENCE_ROOT, "extensions-builtin", "forge_preprocessor_revision", "scripts", "preprocessor_revision.py")
    src = open(path).read().split("\nclass PreprocessorClipVisionForRevision")[0]       # the modifier only: the class below it registers UI objects
    mod = types.ModuleType("reference_preprocessor_revision")
    exec(compile(src, path, "exec"), mod.__dict__)
    return mod.revision_conditioning_modifier


def gen(out_dir):
    from oracle import make_floor as mf
    ref_import.load_reference()
    ref_cv = importlib.import_module("backend.patcher.clipvision")
    res = {"towers": {}, "images": IMAGES, "row_step": ROW_STEP, "outputs": {}, "floor": {}, "separation": {}, "geometry": {}, "converted": {}}
    images = [synth.synth_image(h, w, seed) for h, w, seed in IMAGES]
    with torch.no_grad():
        pixels = torch.cat([ref_cv.clip_preprocess(im) for im in images])
        mean, std = torch.tensor(MEAN).view(3, 1, 1), torch.tensor(STD).view(3, 1, 1)
        levels = [(p * std + mean) * 255.0 for p in pixels]
        assert all(float((lv - lv.round()).abs().max()) < 1e-3 and 0 <= float(lv.round().min()) and float(lv.round().max()) <= 255 for lv in levels)
        levels = [lv.round().to(torch.uint8) for lv in levels]
        for shape in GEOMETRY_SHAPES:
            res["geometry"][shape] = observed_geometry(ref_cv, *shape)
            print("geometry", shape, res["geometry"][shape])
        for name, cfg in synth.TINY_CLIP_VISION_CONFIGS.items():
            sd = synth.synth_clip_vision_state_dict(cfg, seed=TOWER_SEEDS[name])
            res["towers"][name] = {"config": dict(cfg), "seed": TOWER_SEEDS[name]}
            model = build_model(cfg, sd)
            want = run(model, pixels)
            half = run(build_model(cfg, sd, torch.float16), pixels)
            res["floor"][name] = {k: mf.metrics(half[k], want[k]) for k in want}
            res["outputs"][name] = {k: (v if k == "image_embeds" else v[:, ::ROW_STEP]).clone() for k, v in want.items()}
            floor = res["floor"][name]["last_hidden_state"]["rms_rel"]
            last = want["last_hidden_state"]
            other_act = "gelu" if cfg["hidden_act"] == "quick_gelu" else "quick_gelu"
            no_pos = dict(sd, **{"vision_model.embeddings.position_embedding.weight": torch.zeros_like(sd["vision_model.embeddings.position_embedding.weight"])})
            wrong = {"activation_swapped": run(build_model(cfg, sd, hidden_act=other_act), pixels)["last_hidden_state"],
                     "no_position_embedding": run(build_model(cfg, no_pos), pixels)["last_hidden_state"],
                     "after_post_layernorm": model.vision_model.post_layernorm(last),
                     "class_token_last": class_token_last(model, pixels),
                     "other_image": last.flip(0)}
            res["separation"][name] = {k: rms_rel(v, last) for k, v in wrong.items()}
            print(name, "floor", {k: round(v["rms_rel"], 6) for k, v in res["floor"][name].items()}, "separation", {k: round(v, 4) for k, v in res["separation"][name].items()})
            assert all(v >= SEPARATION * floor for v in res["separation"][name].values()), (name, res["separation"][name], floor)
            if name == IPA["tower"]:
                embeds = {"fp32": want["image_embeds"][IPA["image"]:IPA["image"] + 1].clone(), "fp16": half["image_embeds"][IPA["image"]:IPA["image"] + 1].clone()}
                conv = ref_cv.convert_to_transformers(dict(synth.openclip_keyed(sd)), "visual.")
                res["converted"] = {k: (tuple(v.shape), hashlib.sha256(v.contiguous().float().numpy().tobytes()).hexdigest()) for k, v in conv.items()}
                assert set(conv) == set(sd) and all(torch.equal(conv[k], sd[k]) for k in sd)
        res["ipadapter"] = gen_ipadapter(embeds, mf)
        res["revision"] = gen_revision()
    path = os.path.join(out_dir, "clipvision.pt")
    torch.save(res, path)
    lpath = os.path.join(out_dir, "clipvision_levels.pt")
    torch.save({"images": IMAGES, "levels": levels}, lpath)
    for p in (path, lpath):
        print(p, os.path.getsize(p), "bytes")
        assert os.path.getsize(p) < 1 << 20


def gen_ipadapter(embeds, mf):
    import make_ipadapter_fixtures as M
    lib = M.reference_library()
    pred = ref_import.build_ref_predictor()
    cfg = dict(getattr(synth, IPA["config"]))
    order = nets.attn2_order(unet_layout(cfg))
    sd = synth.synth_unet_state_dict(cfg, seed=IPA["weight_seed"])
    nets_ref = {"fp32": ref_import.build_ref_unet(cfg, sd), "fp16": mf.half_unet(cfg, sd)}
    file = synth.synth_ipadapter_state_dict(cfg, plus=False, seed=IPA["file_seed"])
    sigmas = pred.sigma(torch.tensor(IPA["t"]))
    x, c, uc = L.case_inputs(cfg, IPA["hw"], IPA["seed"], sigmas, IPA["b"])
    c, uc = ref_import.SdxlCond(c), ref_import.SdxlCond(uc)

    def run(prec, patched):
        den = ref_import.RefDenoiser(nets_ref[prec], pred, [0])
        dtype = torch.float32 if prec == "fp32" else torch.float16
        work = den.patcher.clone()
        if patched:
            proj = file["image_proj"]
            net = lib.ImageProjModel(cross_attention_dim=int(file["ip_adapter"]["1.to_k_ip.weight"].shape[1]), clip_embeddings_dim=int(proj["proj.weight"].shape[1]),
                                     clip_extra_context_tokens=4)
            net.load_state_dict(proj)
            net = net.to(dtype)
            e = embeds[prec].to(dtype)
            adapter = types.SimpleNamespace(ip_layers=lib.To_KV({k: v.clone() for k, v in file["ip_adapter"].items()}).to(dtype))
            kwargs = {"number": 0, "weight": IPA["weight"], "ipadapter": adapter, "cond": net(e), "uncond": net(torch.zeros_like(e)), "weight_type": IPA["weight_type"],
                      "mask": None, "sigma_start": 999999999.9, "sigma_end": 0.0, "unfold_batch": False}
            with contextlib.redirect_stdout(io.StringIO()):
                for entry in order:
                    lib.set_model_patch_replace(work, kwargs, nets.reference_key(entry))
                    kwargs["number"] += 1
        den.patcher = work
        den.inner_model.inner_model.forge_objects.unet = work
        return den(x, sigmas, uc, c, IPA["cfg"])

    plain, r, r16 = run("fp32", False), run("fp32", True), run("fp16", True)
    out = dict(IPA, result=r, plain=plain, floor=mf.metrics(r16.float(), r), moved=rms_rel(plain, r), embeds=embeds["fp32"])
    print("ipadapter from an image: moved", round(out["moved"], 5), "floor rms_rel", round(out["floor"]["rms_rel"], 6))
    assert out["moved"] >= SEPARATION * out["floor"]["rms_rel"]
    return out


def gen_revision():
    modifier = reference_revision()
    g = torch.Generator().manual_seed(REVISION_SEED)
    y, uy = torch.randn(1, 2816, generator=g), torch.randn(1, 2816, generator=g)
    ctx, uctx = torch.randn(1, 7, 8, generator=g), torch.randn(1, 7, 8, generator=g)
    cases = []
    for units in REVISION_CASES:
        entry = lambda yy, cc: [{"model_conds": {"y": types.SimpleNamespace(cond=yy.clone()), "c_crossattn": types.SimpleNamespace(cond=cc.clone())}}]  # noqa: E731
        conds = [dict(cond=types.SimpleNamespace(image_embeds=torch.randn(1, 1280, generator=torch.Generator().manual_seed(s))), weight=w, noise_aug=0.0, ignore_prompt=ig)
                 for s, w, ig in units]
        _, _, _, uncond, cond, *_ = modifier(types.SimpleNamespace(), None, None, entry(uy, uctx), entry(y, ctx), 7.0, {"revision_conditions": conds}, 0)
        get = lambda e, k: e[0]["model_conds"][k].cond.clone()  # noqa: E731
        cases.append({"units": units, "y": get(cond, "y"), "uncond_y": get(uncond, "y"), "c_crossattn": get(cond, "c_crossattn"),
                      "uncond_c_crossattn": get(uncond, "c_crossattn")})
    return {"seed": REVISION_SEED, "context_shape": (1, 7, 8), "cases": cases}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    if not ref_import.reference_available():
        raise SystemExit("the reference is not present: this generator runs only next to it")
    gen(args.out)


if __name__ == "__main__":
    main()
