"""CPU: native IP-Adapter -- include/fmx_ipadapter.h under the rules of the other headers; file layout, detection and every refusal by message; the
cross-attention order against the reference's hard-coded lists; graph keys and the window against sigmas on both sides of both ends; the group
order under cond_or_uncond = [1, 0]; the fp64 restatements of tests/ipadapter_refs.py and python_patch against what the reference's own classes
recorded (tests/golden/ipadapter.pt, tools/make_ipadapter_fixtures.py); the kernel bound against every planted mistake."""
import ctypes as C
import glob
import os
import re
import subprocess
from types import SimpleNamespace

import pytest
import torch

import forge_amd  # noqa: F401
from forge_amd import _lib, synth
from forge_amd import distributed as fdist
from forge_amd.backend.modules import k_model
from forge_amd.backend.modules.k_prediction import Prediction
from forge_amd.backend.nn import ipadapter as nets
from forge_amd.backend.nn.layout import unet_layout
from forge_amd.backend.nn.unet import IntegratedUNet2DConditionModel as UNetExecutor
from forge_amd.backend.patcher import ipadapter as ipa
from forge_amd.backend.patcher.ipadapter import IPAdapterPatcher, patch_ipadapter
from forge_amd.backend.patcher.kohya_hrfix import patch_kohya_hrfix
from forge_amd.backend.patcher.unet import UnetPatcher

from conftest import load_golden
import ipadapter_refs as I
from test_pag_host import BADARG, FAKE, _kmodel, _Reached

CONFIG = "TINY_SDXL_2LEVEL_UNET_CONFIG"
CFG = dict(getattr(synth, CONFIG))
PIN = 2e-6          # of the tensor's maximum: the figure the other host pins use


@pytest.fixture(scope="module")
def fx():
    return load_golden("ipadapter.pt")


def files(fx, cfg=CFG):
    return {kind: synth.synth_ipadapter_state_dict(cfg, plus=kind == "plus", seed=fx["file_seeds"][kind], kv_gain=fx["kv_gain"]) for kind in ("base", "plus")}


def patcher(cfg=CFG, model=None):
    """a UnetPatcher over the few attributes patch_ipadapter reads: the predictor, the executor's layout, a device"""
    cpu = torch.device("cpu")
    model = model or SimpleNamespace(predictor=Prediction(), diffusion_model=SimpleNamespace(layout=unet_layout(cfg), device=cpu), device=cpu)
    return UnetPatcher(model=model)


def unit(fx, kind="base", weight=0.8, weight_type="original", p=None, **kw):
    return patch_ipadapter(p or patcher(), files(fx)[kind], synth.synth_clip_vision_embeds(plus=kind == "plus"), weight, weight_type, **kw)


# ---- include/fmx_ipadapter.h ------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_point_is_named_in_a_gpu_test():
    here = os.path.dirname(os.path.abspath(__file__))
    gpu_tests = "".join(open(f).read() for f in glob.glob(os.path.join(here, "test_gpu_*.py")))
    assert _lib.IPADAPTER_SIGNATURES and all(re.search(r"\b" + name + r"\b", gpu_tests) for name in _lib.IPADAPTER_SIGNATURES), sorted(_lib.IPADAPTER_SIGNATURES)


def test_library_exports_the_symbol_and_checks_its_contract():
    lib = _lib.lib()
    f = lib.fmxi_attention_dual_f16
    assert _lib.IPADAPTER_SIGNATURES == {"fmxi_attention_dual_f16": [C.POINTER(_lib.DualAttnArgs), C.c_void_p]}
    assert not set(_lib.IPADAPTER_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.LLLITE_SIGNATURES))
    assert _lib.CONSTANTS["FMX_ABI_VERSION"] == 12 and lib.fmx_abi_version() == 12
    names = [n for n, _ in _lib.DualAttnArgs._fields_]
    assert names[:20] == [n for n, _ in _lib.AttnArgs._fields_][:20] and names[20:25] == ["images_per_group", "zero_page", "xk", "xvt", "nseg"]
    assert names[25:] == [f"seg_{w}{i}" for w in ("start", "count", "weight") for i in range(4)]
    text = re.sub(r"/\*.*?\*/", "", open(_lib.IPADAPTER_HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(fmxi_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.search(r" T fmxi_", ln)}
    assert declared == exported == set(_lib.IPADAPTER_SIGNATURES)
    assert f.argtypes == _lib.IPADAPTER_SIGNATURES["fmxi_attention_dual_f16"]
    # the parser returns for the three older headers what it returned before: their struct and entry point sets
    assert set(_lib.EXT_SIGNATURES) == {"fmxe_attn_blend_f16"} and set(_lib.LLLITE_SIGNATURES) == {"fmxl_lllite_adapt_f16"} and len(_lib.SIGNATURES) == 97
    err = lambda: lib.fmx_last_error().decode()  # noqa: E731

    def args(**kw):
        a = _lib.DualAttnArgs()
        a.q = a.k = a.vt = a.o = a.xk = a.xvt = a.zero_page = FAKE
        a.batch, a.heads, a.nq, a.nk, a.nk_pad, a.dpad, a.scale, a.images_per_group, a.nseg = 4, 2, 64, 77, 128, 64, 0.125, 2, 1
        a.q_rs = a.k_rs = a.o_rs = 128
        a.q_bs, a.k_bs, a.o_bs, a.vt_bs, a.vt_hs, a.vt_ds = 64 * 128, 128 * 128, 64 * 128, 128, 64 * 512, 512
        a.seg_count0, a.seg_weight0 = 4, 1.0
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for kw, msg in ((dict(xk=0), "null pointer"), (dict(dpad=128), "dpad 128"), (dict(nk=129, nk_pad=192), "nk 129 not in 1..128"), (dict(nk=0), "nk 0"),
                    (dict(nq=0), "bad dims"), (dict(nk_pad=96), "nk_pad"), (dict(images_per_group=3), "images_per_group"), (dict(xvt=FAKE + 8), "16-byte"),
                    (dict(k_rs=100), "multiples of 8"), (dict(scale=0.0), "scale"), (dict(nseg=0), "nseg 0"), (dict(nseg=5), "nseg 5"),
                    (dict(seg_count0=0), "segment 0"), (dict(seg_start0=61), "segment 0"), (dict(nseg=2, seg_start1=3, seg_count1=2), "overlap"),
                    (dict(seg_weight0=float("nan")), "not finite"), (dict(q_rs=1 << 30, nq=2), "2 GB")):
        assert f(C.byref(args(**kw)), None) == BADARG and msg in err(), (kw, err())


# ---- files ------------------------------------------------------------------------------------------------------------------------------------------------
def test_file_layouts_detection_and_refusals(fx):
    f = files(fx)
    flat = {f"{part}.{k}": v for part, d in f["plus"].items() for k, v in d.items()}
    split = nets.split_file(flat)
    assert set(split) == {"image_proj", "ip_adapter"} and split["ip_adapter"].keys() == f["plus"]["ip_adapter"].keys()
    assert nets.is_ipadapter_file(flat) and nets.is_ipadapter_file(f["base"]) and not nets.is_ipadapter_file({"input_blocks.0.0.weight": 0})
    with pytest.raises(ValueError, match="no ip_adapter keys"):
        nets.split_file({"image_proj.proj.weight": torch.zeros(1)})
    base, plus = nets.detect(f["base"]), nets.detect(f["plus"])
    assert (base["is_plus"], base["tokens"], base["is_faceid"], base["is_full"]) == (False, 4, False, False)
    assert (plus["is_plus"], plus["tokens"], plus["cross_attention_dim"]) == (True, 16, CFG["context_dim"])
    sdxl = nets.detect({"image_proj": {"latents": 0}, "ip_adapter": {"1.to_k_ip.weight": torch.zeros(640, 2048)}})
    assert sdxl["is_sdxl"] and sdxl["cross_attention_dim"] == 1280 and sdxl["output_cross_attention_dim"] == 2048
    # refused by name, with the reason
    lora = dict(f["base"], ip_adapter=dict(f["base"]["ip_adapter"], **{"0.to_q_lora.down.weight": torch.zeros(1)}))
    with pytest.raises(NotImplementedError, match="FaceID files take a face embedding from insightface"):
        patch_ipadapter(patcher(), lora, synth.synth_clip_vision_embeds(), 1.0)
    portrait = dict(f["base"], image_proj={"proj.0.weight": 0, "proj.2.weight": 0, "norm.weight": 0})
    with pytest.raises(NotImplementedError, match="Portrait files take a face embedding from insightface"):
        patch_ipadapter(patcher(), portrait, synth.synth_clip_vision_embeds(), 1.0)
    faceid_plus = dict(lora, image_proj={"perceiver_resampler.proj_in.weight": 0})
    with pytest.raises(NotImplementedError, match="FaceID-Plus files"):
        patch_ipadapter(patcher(), faceid_plus, synth.synth_clip_vision_embeds(), 1.0)
    instant = dict(f["plus"], image_proj=dict(f["plus"]["image_proj"], **{"proj_in.weight": torch.zeros(128, 512)}))
    with pytest.raises(NotImplementedError, match="InstantID files"):
        patch_ipadapter(patcher(), instant, synth.synth_clip_vision_embeds(True), 1.0)
    full = dict(f["base"], image_proj={"proj.0.weight": 0, "proj.3.weight": 0})
    with pytest.raises(NotImplementedError, match="'full' files project all 257 CLIP tokens"):
        patch_ipadapter(patcher(), full, synth.synth_clip_vision_embeds(), 1.0)
    with pytest.raises(NotImplementedError, match="the file has 7 to_k_ip maps, this UNet has 16 cross-attentions"):
        patch_ipadapter(patcher(dict(synth.SD15_UNET_CONFIG)), f["base"], synth.synth_clip_vision_embeds(), 1.0)
    flux = k_model.KModelFlux.__new__(k_model.KModelFlux)
    with pytest.raises(NotImplementedError, match="IP-Adapter: UNet models only"):
        patch_ipadapter(UnetPatcher(model=flux), f["base"], synth.synth_clip_vision_embeds(), 1.0)
    with pytest.raises(ValueError, match="weight_type 'style'"):
        unit(fx, weight_type="style")


def test_refusals_of_companions_and_hooks(fx):
    pag = patcher()
    pag.model_options["pag"] = object()
    with pytest.raises(NotImplementedError, match="IP-Adapter with native Perturbed-Attention Guidance"):
        unit(fx, p=pag)
    lll = patcher()
    lll.set_transformer_option("lllite", object())
    with pytest.raises(NotImplementedError, match="IP-Adapter with native ControlNet-LLLite"):
        unit(fx, p=lll)
    hooked = patcher()
    hooked.set_model_attn1_output_patch(lambda out, extra: out)
    with pytest.raises(NotImplementedError, match="IP-Adapter together with Python block hooks"):
        unit(fx, p=hooked)
    to = unit(fx).model_options["transformer_options"]
    with pytest.raises(NotImplementedError, match="sharded over 2 ranks"):
        fdist.check_batch_coupled_options({"transformer_options": to}, 2)
    fdist.check_batch_coupled_options({"transformer_options": to}, 1)
    for cou, msg in ((None, "carries no cond_or_uncond"), ([0, 0], "repeats an entry"), ([0, 1, 0], "repeats an entry")):
        with pytest.raises(NotImplementedError, match=msg):
            ipa.check_cond_or_uncond(cou, 4)
    with pytest.raises(NotImplementedError, match="does not split into 2 groups"):
        ipa.check_cond_or_uncond([1, 0], 3)


def test_fallbacks_to_the_python_patch_and_the_control_unit_entry(fx):
    native = unit(fx)
    to = native.model_options["transformer_options"]
    assert [u.weight for u in to["ipadapter"]] == [0.8] and UNetExecutor._hooks(to) is None
    two = unit(fx, "plus", 0.5, "linear", p=native).model_options["transformer_options"]
    assert [(u.tokens_per_image, u.weight_type) for u in two["ipadapter"]] == [(4, "original"), (16, "linear")] and UNetExecutor._hooks(two) is None
    assert len(to["ipadapter"]) == 1, "the parent patcher keeps its own list"
    order = nets.attn2_order(unet_layout(CFG))
    for kw in (dict(attn_mask=torch.ones(1, 8, 8)), dict(unfold_batch=True)):
        py = unit(fx, **kw).model_options["transformer_options"]
        assert "ipadapter" not in py and set(py["patches_replace"]["attn2"]) == {nets.reference_key(e) for e in order}
        assert all(isinstance(p, ipa.PythonPatch) and len(p.units) == 1 for p in py["patches_replace"]["attn2"].values())
    e2 = tuple(torch.cat([e, e]) for e in synth.synth_clip_vision_embeds())
    assert "ipadapter" not in patch_ipadapter(patcher(), files(fx)["base"], e2, 1.0).model_options["transformer_options"]        # two reference images
    # a fifth unit, and a fifth 16-token unit that would make 68 tokens: every unit of the job moves to the Python patches, in order
    p = patcher()
    for i in range(4):
        p = unit(fx, "base", 0.1 * (i + 1), p=p)
    assert len(p.model_options["transformer_options"]["ipadapter"]) == 4
    p5 = unit(fx, "base", 0.9, p=p).model_options["transformer_options"]
    assert "ipadapter" not in p5 and [u.weight for u in next(iter(p5["patches_replace"]["attn2"].values())).units] == pytest.approx([0.1, 0.2, 0.3, 0.4, 0.9])
    q = patcher()
    for i in range(4):
        q = unit(fx, "plus", 0.5, p=q)
    assert sum(u.tokens_per_image for u in q.model_options["transformer_options"]["ipadapter"]) == 64
    q = patcher()
    for i in range(3):
        q = unit(fx, "plus", 0.5, p=q)
    q = unit(fx, "base", 0.5, p=q)
    assert len(q.model_options["transformer_options"]["ipadapter"]) == 4 and "ipadapter" not in unit(fx, "plus", 0.5, p=q).model_options["transformer_options"]
    # the control-unit entry: selection by key, the unit's weight and window
    assert IPAdapterPatcher.try_build_from_state_dict({"input_blocks.0.0.weight": torch.zeros(1)}) is None
    from forge_amd.backend.patcher import controlnet as pc
    cu = pc.load_controlnet(files(fx)["base"])
    assert isinstance(cu, IPAdapterPatcher)
    cu.strength, cu.start_percent, cu.end_percent = 0.7, 0.2, 0.8
    objs = SimpleNamespace(unet=patcher())
    cu.process_before_every_sampling(SimpleNamespace(steps=10, sd_model=SimpleNamespace(forge_objects=objs)), synth.synth_clip_vision_embeds(), None)
    got = objs.unet.model_options["transformer_options"]["ipadapter"][0]
    pred = Prediction()
    assert (got.weight, got.sigma_start, got.sigma_end) == (0.7, pred.percent_to_sigma(0.2), pred.percent_to_sigma(0.8))


# ---- the order of the cross-attentions ----------------------------------------------------------------------------------------------------------------
def test_key_order_equals_the_references_hard_coded_lists():
    """IPAdapterPlus.py:762-783, restated as data: SD1.5's keys carry no transformer index, SDXL's do"""
    sd15 = [("input", i) for i in (1, 2, 4, 5, 7, 8)] + [("output", i) for i in (3, 4, 5, 6, 7, 8, 9, 10, 11)] + [("middle", 0)]
    sdxl = [("input", i, j) for i in (4, 5, 7, 8) for j in range(2 if i in (4, 5) else 10)] + \
           [("output", i, j) for i in range(6) for j in range(2 if i in (3, 4, 5) else 10)] + [("middle", 0, j) for j in range(10)]
    got15 = [nets.reference_key(e) for e in nets.attn2_order(unet_layout(dict(synth.SD15_UNET_CONFIG)))]
    gotxl = [nets.reference_key(e) for e in nets.attn2_order(unet_layout(dict(synth.SDXL_UNET_CONFIG)))]
    assert got15 == sd15 and len(got15) == 16
    assert gotxl == sdxl and len(gotxl) == 70
    names = [e[3] for e in nets.attn2_order(unet_layout(dict(synth.SDXL_UNET_CONFIG)))]
    assert names[0] == "input_blocks.4.1.transformer_blocks.0" and names[24] == "output_blocks.0.1.transformer_blocks.0" and names[-1] == "middle_block.1.transformer_blocks.9"
    kv = nets.to_kv_weights(synth.ipadapter_param_shapes(CFG)["ip_adapter"], unet_layout(CFG))
    assert list(kv) == [e[3] for e in nets.attn2_order(unet_layout(CFG))] and len(kv) == 7


# ---- graph keys and the window --------------------------------------------------------------------------------------------------------------------------
def test_graph_keys_and_the_window_on_both_sides_of_both_ends(fx, monkeypatch):
    net, km, packs = _kmodel(monkeypatch)
    seen = []
    net.forward_packed = lambda *a, **kw: (seen.append(kw["native"].ipadapter), (_ for _ in ()).throw(_Reached()))[1]
    monkeypatch.setattr(ipa.ExtraContext, "prepare", lambda self, net: self)
    x = torch.zeros(2, 4, 32, 32)
    c, uc = (torch.ones(2, 77, 8), None), (torch.zeros(2, 77, 8), None)
    pred = Prediction()
    s0, s1 = pred.percent_to_sigma(0.2), pred.percent_to_sigma(0.8)
    assert s0 > s1 > 0

    def sig(v):
        s = torch.full((2,), v, dtype=torch.float64)
        s.fmx_sigma = k_model.SigmaInfo([v, v])
        return s

    one = unit(fx, start_at=0.2, end_at=0.8)
    to = one.model_options["transformer_options"]
    u = to["ipadapter"][0]
    assert (u.sigma_start, u.sigma_end) == (s0, s1)
    for v in (s0 * 1.001, s0, s0 * 0.999, s1 * 1.001, s1, s1 * 0.999):
        with pytest.raises(_Reached):
            km.denoise_cfg(x, sig(v), uc, c, 7.0, transformer_options=to)
    assert [s is not None for s in seen] == [False, True, True, True, True, False]       # the reference skips on `sigma > start or sigma < end`
    ctx = seen[1]
    assert all(s is ctx for s in seen[1:5]) and ctx.cond_or_uncond == [1, 0] and ctx.units == [u]
    base = (2, 4, 32, 32, 2)
    inside = base + ("ipadapter", ctx.serial, (1, 0), False, (u.serial, 0.8, "original"))
    assert list(km._static) == [base, inside] and list(km._gstate) == list(km._static)
    # two units with different windows: the active set is part of the key, with each unit's identity, weight and weight type
    two = unit(fx, "plus", 0.5, "channel", p=one, start_at=0.0, end_at=0.5).model_options["transformer_options"]
    u2 = two["ipadapter"][1]
    mid = pred.percent_to_sigma(0.5)
    del seen[:]
    for v in (s0 * 1.001, s0 * 0.999, mid * 0.999, s1 * 0.999):
        with pytest.raises(_Reached):
            km.denoise_cfg(x, sig(v), uc, c, 7.0, transformer_options=two)
    assert [None if s is None else [w.serial for w in s.units] for s in seen] == [[u2.serial], [u.serial, u2.serial], [u.serial], None]
    keys = list(km._static)[2:]
    assert [k[-len(s.units):] for k, s in zip(keys, seen[:2])] == [(u2.key(),), (u.key(), u2.key())] and u2.key() == (u2.serial, 0.5, "channel")
    assert len(keys) == 2 and seen[2] is ctx          # unit 1 alone: the cached context, the key `inside`, the same graph
    # apply_model takes the groups from the caller's cond_or_uncond and refuses a call without it
    with pytest.raises(NotImplementedError, match="carries no cond_or_uncond"):
        km.apply_model(torch.zeros(4, 4, 32, 32), sig(s0 * 0.9), c_crossattn=torch.zeros(4, 77, 8), transformer_options=to)
    with pytest.raises(_Reached):
        km.apply_model(torch.zeros(4, 4, 32, 32), sig(s0 * 0.9), c_crossattn=torch.zeros(4, 77, 8), transformer_options=dict(to, cond_or_uncond=[0, 1]))
    assert seen[-1].cond_or_uncond == [0, 1] and list(km._static)[-1][:6] == (4, 4, 32, 32, 1, "apply")
    # refused at the call: Python hooks, native ControlNet-LLLite, native PAG
    hooked = dict(to, patches={"attn1_output_patch": [lambda o, e: o]})
    with pytest.raises(NotImplementedError, match=r"IP-Adapter \(native\) together with Python block hooks"):
        km.denoise_cfg(x, sig(s0 * 0.9), uc, c, 7.0, transformer_options=hooked)
    with pytest.raises(NotImplementedError, match="IP-Adapter with native ControlNet-LLLite"):
        km.denoise_cfg(x, sig(s0 * 0.9), uc, c, 7.0, transformer_options=dict(to, lllite=SimpleNamespace(counter=SimpleNamespace(advance=lambda: False))))
    with pytest.raises(NotImplementedError, match="IP-Adapter with native Perturbed-Attention Guidance"):
        km.denoise_cfg(x, sig(s0 * 0.9), uc, c, 7.0, transformer_options=to, pag_scale=3.0)
    # Kohya HRFix rides along
    kohya = patch_kohya_hrfix(one, 3, 2.0, 0.0, 0.35, True, "bicubic", "bicubic").model_options["transformer_options"]
    assert kohya["ipadapter"][0] is u and UNetExecutor._hooks(kohya) is None


def test_group_order_follows_cond_or_uncond(fx):
    """the cached extra context of a call whose batch is [uncond ; cond] holds the uncond tokens' keys in group 0, and the other way round"""
    cfg = dict(synth.TINY_SD15_UNET_CONFIG)
    net = SimpleNamespace(layout=unet_layout(cfg), device=torch.device("cpu"))
    sd = synth.synth_ipadapter_state_dict(cfg, plus=False)
    to = patch_ipadapter(patcher(cfg), sd, synth.synth_clip_vision_embeds(), 0.8).model_options["transformer_options"]
    u = to["ipadapter"][0]
    b = "middle_block.1.transformer_blocks.0"
    k, v = u.block_kv(b)
    cond, uncond = u.image_tokens()
    wk, wv = u.to_kv[b]
    assert all(torch.allclose(a, t[0] @ w.T, atol=1e-5) for a, t, w in ((k[0], cond, wk), (k[1], uncond, wk), (v[0], cond, wv), (v[1], uncond, wv)))
    L = [l for l in net.layout.middle if hasattr(l, "heads")][0]
    H, d = L.heads, L.dim_head
    for cou in ([1, 0], [0, 1], [0]):
        ent = ipa.ExtraContext([u], cou).prepare(net).blocks[b]
        dp = ent["xk"].shape[2] // H
        assert ent["xk"].shape == (len(cou), 64, H * dp) and ent["xvt"].shape == (H * dp, len(cou) * 64) and ent["segments"] == [(0, 4, 0.8)]
        for g, which in enumerate(cou):
            assert torch.equal(ent["xk"][g, :4].view(4, H, dp)[..., :d].reshape(4, -1), k[which].to(torch.float16))
            assert torch.equal(ent["xvt"][:, g * 64:g * 64 + 4].T.reshape(4, H, dp)[..., :d].reshape(4, -1), v[which].to(torch.float16))
            assert not bool(ent["xk"][g, 4:].any()) and not bool(ent["xvt"][:, g * 64 + 4:(g + 1) * 64].any())      # finite zeros behind the segment
            assert not bool(ent["xk"][g].view(64, H, dp)[..., d:].any())                                               # the heads' pad columns
    assert not torch.equal(k[0], k[1])


# ---- the restatements against the reference's recordings -----------------------------------------------------------------------------------------------
def _ref_units(fx, units):
    f = files(fx)
    n = [e[3] for e in nets.attn2_order(unet_layout(CFG))].index("middle_block.1.transformer_blocks.0")
    return [(fx["tokens"][kind][0], fx["tokens"][kind][1], f[kind]["ip_adapter"][f"{2 * n + 1}.to_k_ip.weight"], f[kind]["ip_adapter"][f"{2 * n + 1}.to_v_ip.weight"],
             w, wt) for kind, w, wt in units]


def _call_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(4, 64, 128, generator=g), torch.randn(4, 77, 128, generator=g), torch.randn(4, 77, 128, generator=g)


def test_image_tokens_restatement_vs_the_references_networks(fx):
    f = files(fx)
    for kind in ("base", "plus"):
        info = nets.detect(f[kind])
        for e, want in zip(synth.synth_clip_vision_embeds(plus=kind == "plus"), fx["tokens"][kind]):
            got = ipa.image_tokens_torch(f[kind], info, e)
            assert got.shape == want.shape == (1, info["tokens"], CFG["context_dim"])
            assert float((got - want).abs().max() / want.abs().max()) <= PIN, kind


def test_patch_ref_and_python_patch_vs_the_references_patch_calls(fx):
    assert len(fx["patch_calls"]) == 8 and {tuple(c["cond_or_uncond"]) for c in fx["patch_calls"]} == {(1, 0), (0, 1)}
    assert {wt for c in fx["patch_calls"] for _, _, wt in c["units"]} == {"original", "linear", "channel"} and max(len(c["units"]) for c in fx["patch_calls"]) == 2
    for call in fx["patch_calls"]:
        q, k, v = _call_inputs(call["seed"])
        want = call["out"].double()
        got = I.patch_ref(q, k, v, 2, _ref_units(fx, call["units"]), call["cond_or_uncond"])[:, ::call["every"]]
        assert float((got - want).abs().max() / want.abs().max()) <= PIN, call["units"]
        # python_patch, in fp32 on the CPU, on the same call
        p = patcher()
        for kind, w, wt in call["units"]:
            p = unit(fx, kind, w, wt, p=p)
        units = p.model_options["transformer_options"]["ipadapter"]
        patch = ipa.python_patch(units)[("middle", 0, 0)]
        out = patch(q, k, v, {"cond_or_uncond": call["cond_or_uncond"], "n_heads": 2, "dim_head": 64})[:, ::call["every"]]
        assert float((out.double() - want).abs().max() / want.abs().max()) <= 2e-5, call["units"]      # fp32 arithmetic against the reference's fp32
        # the groups matter: the other order misses by far more
        flipped = I.patch_ref(q, k, v, 2, _ref_units(fx, call["units"]), call["cond_or_uncond"][::-1])[:, ::call["every"]]
        assert float((flipped - want).abs().max() / want.abs().max()) > 1e-3


# ---- the kernel bound has teeth ---------------------------------------------------------------------------------------------------------------------------
def test_the_kernel_bound_tells_every_planted_mistake():
    """on the inputs of the kernel test: the fp64 reference rounded to fp16 -- the best a kernel can do -- lies inside the bound, and each planted
    mistake misses it by TEETH_FACTOR"""
    scale = I.D ** -0.5
    for nq, nk, name, weights in ((64, 77, "two_units", [0.35, 1.0]), (200, 1, "two_units", [2.5, -0.5]), (64, 128, "four_of_16", [0.35, 1.0, -0.5, 2.5])):
        c = I.make_case(nq, nk, name)
        want = I.dual_ref(c, weights, scale)
        assert I.excess(want.to(torch.float16), want, I.dual_bound(want, weights)) <= 0.5
        for bug in ("joint_softmax", "one_softmax_for_all_segments", "swap_groups", "weight_before_softmax"):
            wrong = I.dual_ref(c, weights, scale, bug=bug)
            assert I.excess(wrong, want, I.dual_bound(want, weights)) >= I.TEETH_FACTOR, (nq, nk, name, bug)
