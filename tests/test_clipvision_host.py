"""CPU: the native CLIP-vision encoder -- include/fmx_clipvision.h under the rules of the other headers and every refusal of its two entry points by
message; the OpenCLIP key conversion, the detection by depth and clip_preprocess's host arithmetic against what the reference recorded
(tests/golden/clipvision.pt, tools/make_clipvision_fixtures.py); the towers' weight layout for heads of 104; the wiring's refusals, the tuple path
of IP-Adapter and the Revision modifier; and the measurement behind the GPU gate of clip_embed_ln."""
import ctypes as C
import glob
import hashlib
import os
import re
import subprocess
from types import SimpleNamespace

import pytest
import torch

import forge_amd  # noqa: F401
from forge_amd import _lib, synth
from forge_amd.backend.nn import clip_vision as towers
from forge_amd.backend.patcher import clipvision as cv
from forge_amd.backend.patcher import ipadapter as ipa
from forge_amd.backend.patcher import revision as rev
from forge_amd.backend.patcher.ipadapter import IPAdapterPatcher, patch_ipadapter
from forge_amd.backend.sampling.condition import Condition, ConditionCrossAttn

from conftest import load_golden
import clipvision_refs as R
from test_ipadapter_host import CFG, patcher
from test_pag_host import BADARG, FAKE


@pytest.fixture(scope="module")
def fx():
    return load_golden("clipvision.pt")


# ---- include/fmx_clipvision.h -------------------------------------------------------------------------------------------------------------------------
def test_header_rules():
    lib = _lib.lib()
    text = re.sub(r"/\*.*?\*/", "", open(_lib.CLIPVISION_HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(fmxv_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.search(r" T fmxv_", ln)}
    assert declared == exported == set(_lib.CLIPVISION_SIGNATURES) == {"fmxv_clip_patch_rows_f16", "fmxv_clip_embed_ln_f16"}
    p, i = C.c_void_p, C.c_int32
    assert _lib.CLIPVISION_SIGNATURES == {"fmxv_clip_patch_rows_f16": [p, p, i, i, i, i, i, p], "fmxv_clip_embed_ln_f16": [p, p, p, p, p, p, i, i, i, C.c_float, p]}
    assert all(getattr(lib, n).argtypes == a and getattr(lib, n).restype is C.c_int for n, a in _lib.CLIPVISION_SIGNATURES.items())
    older = set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.LLLITE_SIGNATURES) | set(_lib.IPADAPTER_SIGNATURES)
    assert not set(_lib.CLIPVISION_SIGNATURES) & older
    assert _lib.CONSTANTS["FMX_ABI_VERSION"] == 12 and lib.fmx_abi_version() == 12
    assert (len(_lib.SIGNATURES), len(_lib.EXT_SIGNATURES), len(_lib.LLLITE_SIGNATURES), len(_lib.IPADAPTER_SIGNATURES)) == (97, 1, 1, 1)
    assert _lib.CLIPVISION_CONSTANTS == {"FMXV_CLIP_IMAGE": 224, "FMXV_CLIP_PATCH": 14, "FMXV_CLIP_PATCH_COLS": 640, "FMXV_CLIP_TOKENS": 257}
    here = os.path.dirname(os.path.abspath(__file__))
    gpu_tests = "".join(open(f).read() for f in glob.glob(os.path.join(here, "test_gpu_*.py")))
    assert all(re.search(r"\b" + name + r"\b", gpu_tests) for name in _lib.CLIPVISION_SIGNATURES)
    # the header is part of the kernel sources' identity and of the build's dependencies
    csrc = os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc")
    assert "fmx_clipvision.h" in open(os.path.join(csrc, "src_hash.py")).read() and open(os.path.join(csrc, "Makefile")).read().count("$(ROOT)/include/fmx_clipvision.h") == 2


def test_every_refusal_by_message():
    lib = _lib.lib()
    err = lambda: lib.fmx_last_error().decode()  # noqa: E731

    def patch_rows(inp=FAKE, out=FAKE, b=1, rh=224, rw=224, top=0, left=0):
        return lib.fmxv_clip_patch_rows_f16(inp, out, b, rh, rw, top, left, None)

    for kw, msg in ((dict(inp=0), "null pointer"), (dict(out=0), "null pointer"), (dict(out=FAKE + 8), "16-byte aligned"), (dict(inp=FAKE + 2), "4-byte"),
                    (dict(b=0), "b 0 < 1"), (dict(rh=223), "plane 223 x 224 smaller than 224 x 224"), (dict(rw=200), "plane 224 x 200 smaller"),
                    (dict(rh=231, top=8), "window [8, 232) x [0, 224) leaves the 231 x 224 plane"), (dict(rw=300, left=77), "leaves the 224 x 300 plane"),
                    (dict(top=-1), "leaves"), (dict(left=-1), "leaves")):
        assert patch_rows(**kw) == BADARG and msg in err(), (kw, err())

    def embed(ptrs=(FAKE,) * 6, b=1, c=128, t_pad=320):
        return lib.fmxv_clip_embed_ln_f16(*ptrs, b, c, t_pad, 1e-5, None)

    for i in range(6):
        assert embed(ptrs=tuple(0 if j == i else FAKE for j in range(6))) == BADARG and "null pointer" in err(), i
        assert embed(ptrs=tuple(FAKE + 8 if j == i else FAKE for j in range(6))) == BADARG and "16-byte aligned" in err(), i
    for kw, msg in ((dict(b=0), "b 0 < 1"), (dict(t_pad=300), "rows_per_image 300 must be a multiple of 64 and >= 257"),
                    (dict(t_pad=256), "rows_per_image 256 must be a multiple of 64 and >= 257"), (dict(c=100), "c 100 must be a multiple of 8 in 8..4096"),
                    (dict(c=4104), "c 4104 must be a multiple of 8 in 8..4096"), (dict(c=0), "c 0")):
        assert embed(**kw) == BADARG and msg in err(), (kw, err())


# ---- the reference's surface ---------------------------------------------------------------------------------------------------------------------------
def test_key_conversion_vs_the_references(fx):
    name = "d80"
    sd = synth.synth_clip_vision_state_dict(fx["towers"][name]["config"], seed=fx["towers"][name]["seed"])
    got = cv.convert_to_transformers(dict(synth.openclip_keyed(sd)), "visual.")
    digest = lambda v: (tuple(v.shape), hashlib.sha256(v.contiguous().float().numpy().tobytes()).hexdigest())  # noqa: E731
    assert {k: digest(v) for k, v in got.items()} == fx["converted"] and len(got) == len(sd)
    assert "vision_model.pre_layrnorm.weight" in got and got["visual_projection.weight"].shape == (64, 320)
    # any other layout only loses its prefix; keys outside the prefix stay
    plain = cv.convert_to_transformers({"model.vision_model.x": 1, "other": 2}, "model.")
    assert plain == {"vision_model.x": 1, "other": 2}
    extra = cv.convert_to_transformers(dict(synth.openclip_keyed(sd), **{"transformer.resblocks.0.ln_1.weight": 7}), "visual.")
    assert extra["transformer.resblocks.0.ln_1.weight"] == 7 and len(extra) == len(sd) + 1          # the text tower of the same file is left alone


def test_detection_by_depth(monkeypatch):
    built = []
    monkeypatch.setattr(cv, "ClipVisionModel", lambda config, sd, device: built.append(config) or config)
    key = "vision_model.encoder.layers.{}.layer_norm1.weight"
    for depth, want in ((48, cv.CLIP_VISION_G), (32, cv.CLIP_VISION_H), (24, cv.CLIP_VISION_VITL)):
        sd = {key.format(i): 0 for i in range(depth)}
        assert cv.load_clipvision_from_sd(sd) is want and cv.detect_config(sd) is want
    assert cv.load_clipvision_from_sd({key.format(i): 0 for i in range(12)}) is None and cv.load_clipvision_from_sd({}) is None
    assert [(c["hidden_size"], c["num_attention_heads"], c["num_hidden_layers"], c["intermediate_size"], c["hidden_act"], c["projection_dim"])
            for c in (cv.CLIP_VISION_VITL, cv.CLIP_VISION_H, cv.CLIP_VISION_G)] == [(1024, 16, 24, 4096, "quick_gelu", 768), (1280, 16, 32, 5120, "gelu", 1024),
                                                                                  (1664, 16, 48, 8192, "gelu", 1280)]
    # the OpenCLIP layout is converted first: prefix "visual."
    sd = synth.openclip_keyed({key.format(i): torch.zeros(4) for i in range(32)})
    assert cv.load_clipvision_from_sd(dict(sd, **{"visual.transformer.resblocks.0.attn.in_proj_weight": torch.zeros(12, 4)}), "visual.", True) is cv.CLIP_VISION_H


def test_preprocess_geometry_vs_the_references(fx):
    assert set(fx["geometry"]) == {(224, 224), (300, 231), (512, 768), (225, 224), (224, 1000)}
    for (h, w), want in fx["geometry"].items():
        assert cv.preprocess_geometry(h, w) == tuple(want), (h, w)
    assert cv.preprocess_geometry(300, 231) == (291, 224, 33, 0)
    with pytest.raises(NotImplementedError, match="size 336"):
        cv.resized(torch.zeros(1, 8, 8, 3), 336)
    with pytest.raises(ValueError, match=r"\[b, h, w, 3\]"):
        cv.resized(torch.zeros(1, 3, 8, 8))


def test_output_takes_item_and_attribute_access():
    o = cv.Output()
    o["image_embeds"] = 3
    assert o.image_embeds == 3 and o["image_embeds"] == 3


# ---- the towers' weight layout ---------------------------------------------------------------------------------------------------------------------------
def test_heads_of_104_are_laid_out_128_apart(fx):
    cfg = fx["towers"]["d104"]["config"]
    H, d, dp, c = 8, 104, 128, 832
    sd = synth.synth_clip_vision_state_dict(cfg, seed=fx["towers"]["d104"]["seed"])
    w = towers.layer_weights(sd, 1, H, d)
    qk_w, qk_b = w["qk"]
    assert qk_w.shape == (2 * H * dp, c) and qk_b.shape == (2 * H * dp,) and w["v"].shape == (H * dp, c) and w["out"][0].shape == (c, H * dp)
    k = "vision_model.encoder.layers.1.self_attn."
    for part, (wt, bs) in enumerate(((sd[k + "q_proj.weight"], sd[k + "q_proj.bias"]), (sd[k + "k_proj.weight"], sd[k + "k_proj.bias"]))):
        gw, gb = qk_w[part * H * dp:(part + 1) * H * dp].view(H, dp, c), qk_b[part * H * dp:(part + 1) * H * dp].view(H, dp)
        assert torch.equal(gw[:, :d], wt.view(H, d, c)) and torch.equal(gb[:, :d], bs.view(H, d)) and not bool(gw[:, d:].any()) and not bool(gb[:, d:].any())
    gv = w["v"].view(H, dp, c)
    assert torch.equal(gv[:, :d], sd[k + "v_proj.weight"].view(H, d, c)) and not bool(gv[:, d:].any())
    go = w["out"][0].view(c, H, dp)
    assert torch.equal(go[..., :d], sd[k + "out_proj.weight"].view(c, H, d)) and not bool(go[..., d:].any())
    # out_proj(pad(o)) equals the unpadded product, and the folded bias carries W_o b_v (fp64, random data)
    g = torch.Generator().manual_seed(5)
    o = torch.randn(7, H, d, generator=g, dtype=torch.float64)
    padded = torch.zeros(7, H, dp, dtype=torch.float64)
    padded[..., :d] = o
    want = o.view(7, -1) @ sd[k + "out_proj.weight"].double().T
    assert torch.equal(padded.view(7, -1) @ w["out"][0].double().T, want) or float((padded.view(7, -1) @ w["out"][0].double().T - want).abs().max()) < 1e-12
    bias = sd[k + "out_proj.bias"].double() + sd[k + "out_proj.weight"].double() @ sd[k + "v_proj.bias"].double()
    assert float((w["out"][1].double() - bias).abs().max()) < 1e-6
    # widths 64 and 80 run as they are; any other width is refused by name
    for name, (heads, width) in (("d64", (2, 64)), ("d80", (4, 80))):
        cfg2 = fx["towers"][name]["config"]
        w2 = towers.layer_weights(synth.synth_clip_vision_state_dict(cfg2, seed=1), 0, heads, width)
        assert w2["v"].shape == (heads * width, heads * width) and towers.head_dpad(width) == width
    with pytest.raises(NotImplementedError, match="head width 96 is not one of"):
        towers.head_dpad(96)
    with pytest.raises(NotImplementedError, match="head width 96"):
        towers.CLIPVisionTower(dict(cfg, hidden_size=768), {}, "cpu")


# ---- wiring ------------------------------------------------------------------------------------------------------------------------------------------
def _base_file():
    return synth.synth_ipadapter_state_dict(CFG, plus=False, seed=31)


def test_ipadapter_wiring_refusals():
    tower64 = SimpleNamespace(output_width={"image_embeds": 64, "penultimate_hidden_states": 320}, load_device=torch.device("cpu"))
    img = torch.zeros(1, 224, 224, 3)
    with pytest.raises(NotImplementedError, match="noise 0.3 > 0"):
        patch_ipadapter(patcher(), _base_file(), None, 0.8, clip_vision=tower64, image=img, noise=0.3)
    with pytest.raises(NotImplementedError, match="noise 0.25 > 0"):
        patch_ipadapter(patcher(), _base_file(), dict(clip_vision=tower64, image=img, weight_type="original", noise=0.25, embeds=None, unfold_batch=False), 0.8)
    wide = SimpleNamespace(output_width={"image_embeds": 1024, "penultimate_hidden_states": 1280}, load_device=torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="clip_embeddings_dim is 64, this CLIP-vision tower's image_embeds are 1024 wide"):
        patch_ipadapter(patcher(), _base_file(), None, 0.8, clip_vision=wide, image=img)
    plus = synth.synth_ipadapter_state_dict(CFG, plus=True, seed=77)
    with pytest.raises(NotImplementedError, match="clip_embeddings_dim is 64, this CLIP-vision tower's penultimate_hidden_states are 320 wide"):
        patch_ipadapter(patcher(), plus, None, 0.8, clip_vision=tower64, image=img)
    with pytest.raises(ValueError, match="needs clip_vision= and image="):
        patch_ipadapter(patcher(), _base_file(), None, 0.8)
    with pytest.raises(ValueError, match=r"keys \['strength'\]"):
        patch_ipadapter(patcher(), _base_file(), dict(strength=1.0), 0.8)


def test_tuple_and_dict_forms_of_cond(monkeypatch):
    """a tuple passed as cond / embeds keeps its route: it reaches the unit as it is; the preprocessor dict with embeds= set does the same"""
    e = synth.synth_clip_vision_embeds()
    got = patch_ipadapter(patcher(), _base_file(), e, 0.8).model_options["transformer_options"]["ipadapter"][0]
    assert got.embeds[0] is e[0] and got.embeds[1] is e[1] and got.weight == 0.8 and got.weight_type == "original"
    seen = []
    monkeypatch.setattr(ipa, "embeds_from_image", lambda *a, **kw: seen.append(a) or e)
    cu = IPAdapterPatcher(_base_file())
    cu.strength = 0.6
    for cond in (e, dict(clip_vision=None, image=None, weight_type="linear", noise=0.0, embeds=e, unfold_batch=False)):
        objs = SimpleNamespace(unet=patcher())
        cu.process_before_every_sampling(SimpleNamespace(steps=10, sd_model=SimpleNamespace(forge_objects=objs)), cond, None)
        u = objs.unet.model_options["transformer_options"]["ipadapter"][0]
        assert u.embeds[0] is e[0] and u.weight == 0.6 and u.weight_type == ("linear" if isinstance(cond, dict) else "original")
    assert seen == []
    cv_model, img = object(), object()
    objs = SimpleNamespace(unet=patcher())
    cu.process_before_every_sampling(SimpleNamespace(steps=10, sd_model=SimpleNamespace(forge_objects=objs)),
                                     dict(clip_vision=cv_model, image=img, weight_type="original", noise=0.0, embeds=None, unfold_batch=False), None)
    assert len(seen) == 1 and seen[0][0] is cv_model and seen[0][1] is img and objs.unet.model_options["transformer_options"]["ipadapter"][0].embeds[0] is e[0]


def _sdxl_patcher(adm=2816):
    return patcher(dict(CFG, adm_in_channels=adm))


def test_revision_modifier_vs_the_references(fx):
    r = fx["revision"]
    g = torch.Generator().manual_seed(r["seed"])
    y, uy = torch.randn(1, 2816, generator=g), torch.randn(1, 2816, generator=g)
    ctx, uctx = torch.randn(*r["context_shape"], generator=g), torch.randn(*r["context_shape"], generator=g)
    assert len(r["cases"]) == 3
    for case in r["cases"]:
        m = _sdxl_patcher()
        for seed, weight, ignore in case["units"]:
            out = cv.Output()
            out["image_embeds"] = torch.randn(1, 1280, generator=torch.Generator().manual_seed(seed))
            m = rev.patch_revision(m, out, weight, 0.0, ignore)
        assert m.model_options["conditioning_modifiers"] == [rev.revision_conditioning_modifier] and len(m.model_options["revision_conditions"]) == len(case["units"])
        entry = lambda yy, cc: [dict(model_conds=dict(y=Condition(yy), c_crossattn=ConditionCrossAttn(cc)))]  # noqa: E731
        cond, uncond = entry(y, ctx), entry(uy, uctx)
        res = rev.revision_conditioning_modifier(m.model, None, None, uncond, cond, 7.0, m.model_options, 0)
        assert res[0] is m.model and res[5] == 7.0 and res[6] is m.model_options
        for entries, yk, ck in ((res[4], "y", "c_crossattn"), (res[3], "uncond_y", "uncond_c_crossattn")):
            assert torch.equal(entries[0]["model_conds"]["y"].cond, case[yk]) and torch.equal(entries[0]["model_conds"]["c_crossattn"].cond, case[ck])
            assert isinstance(entries[0]["model_conds"]["c_crossattn"], ConditionCrossAttn)
        assert torch.equal(cond[0]["model_conds"]["y"].cond, y) and torch.equal(uncond[0]["model_conds"]["c_crossattn"].cond, uctx)      # the caller's conds are not touched
        assert not bool(res[3][0]["model_conds"]["y"].cond[:, :1280].any()) and torch.equal(res[3][0]["model_conds"]["y"].cond[:, 1280:], uy[:, 1280:])
    assert "revision_conditions" not in _sdxl_patcher().model_options


def test_revision_refusals():
    out = {"image_embeds": torch.zeros(1, 1280)}
    with pytest.raises(NotImplementedError, match="`y` is 192 wide, SDXL's is 2816"):
        rev.patch_revision(patcher(), out, 1.0)
    with pytest.raises(NotImplementedError, match="`y` is None wide"):
        rev.patch_revision(patcher(dict(synth.TINY_SD15_UNET_CONFIG)), out, 1.0)
    unclip = _sdxl_patcher()
    unclip.model.noise_augmentor = object()
    with pytest.raises(NotImplementedError, match="noise_augmentor"):
        rev.patch_revision(unclip, out, 1.0)
    with pytest.raises(ValueError, match=r"image_embeds \(1, 64\)"):
        rev.patch_revision(_sdxl_patcher(), {"image_embeds": torch.zeros(1, 64)}, 1.0)
    m = rev.patch_revision(_sdxl_patcher(), out, 1.0)
    with pytest.raises(NotImplementedError, match="`y` is 192 wide"):
        rev.revision_conditioning_modifier(m.model, None, None, None, [dict(model_conds=dict(y=Condition(torch.zeros(1, 192))))], 7.0, m.model_options, 0)


# ---- the measurement behind the GPU gates ------------------------------------------------------------------------------------------------------------------
def test_embed_ln_kernel_order_in_fp32_vs_fp64():
    """what test_gpu_clipvision's gate on clip_embed_ln rests on: the kernel's fp32 arithmetic in its own order, rounded to fp16, against the fp64
    result rounded to fp16, over the GPU test's cases.  Measured: worst distance 1 ulp (EMBED_RESTATEMENT_ULPS); the gate is that plus one."""
    worst = 0
    for c, b, t_pad in R.EMBED_CASES:
        ops_ = R.embed_case(c, b)
        want = R.embed_ref64(*ops_, b, t_pad)
        got = R.embed_kernel_order_f32(*ops_, b, t_pad)
        dist = int(R.ulp_distance_f16(got, want).max())
        print(f"c {c} b {b} t_pad {t_pad}: worst fp16 ulp distance {dist}")
        worst = max(worst, dist)
        img, tok = R.EQUAL_ROW
        assert torch.equal(got[img, tok].half(), ops_[4]) and torch.equal(want[img, tok].half(), ops_[4]), "variance 0: the row is beta"
        assert not bool(got[:, 257:].any())
    assert worst == R.EMBED_RESTATEMENT_ULPS and R.EMBED_GATE_ULPS == worst + 1


def test_patch_rows_cases_meet_ties_and_both_clamps():
    for b, rh, rw in R.PATCH_CASES:
        x = R.patch_case(b, rh, rw)
        t = 255.0 * x
        ties = (t - t.floor() == 0.5) & (t > 0) & (t < 255)
        assert int(ties.sum()) >= 100 and int((x < 0).sum()) > 1000 and int((x > 1).sum()) > 1000 and int((x == 0).sum()) >= 400 and int((x == 1).sum()) >= 400
        top, left = R.crop_of(rh, rw)
        ref = R.patch_rows_ref(x, top, left)
        assert ref.shape == (b * 256, 640) and not bool(ref[:, 588:].any()) and bool(torch.isfinite(ref).all())
    assert [R.crop_of(rh, rw) for _, rh, rw in R.PATCH_CASES] == [(0, 0), (3, 0), (0, 38)]
