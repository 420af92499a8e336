"""CPU: native StyleAlign -- the reference's thresholds, the patcher entry, every refusal (Flux, repeated or missing cond_or_uncond, Python hooks, a
sharded batch), the graph keys, the restated attn1_proc against the outputs the reference's own function recorded, and the rounding model of
fmxe_attn_blend_f16 against the torch expression, bit for bit."""
import ctypes as C
import re
import subprocess

import pytest
import torch

import forge_amd  # noqa: F401
from forge_amd import _lib
from forge_amd import distributed as fdist
from forge_amd.backend.modules import k_model
from forge_amd.backend.nn.unet import IntegratedUNet2DConditionModel as UNetExecutor
from forge_amd.backend.patcher import stylealign as sa
from forge_amd.backend.patcher.freeu import patch_freeu_v2
from forge_amd.backend.patcher.native_call import NativeCall
from forge_amd.backend.patcher.stylealign import patch_stylealign
from forge_amd.backend.patcher.unet import UnetPatcher

from conftest import load_golden
import stylealign_refs as S
from test_pag_host import BADARG, FAKE, _kmodel, _patcher, _Reached, _sigma


def _to(strength):
    return patch_stylealign(_patcher(), strength).model_options["transformer_options"]


def test_thresholds_are_the_references():
    """forge_stylealign.py:67-82: strength < 0.01 ordinary, > 0.99 aligned, else the blend -- 0.01 and 0.99 themselves blend"""
    assert [sa.mode_of(s) for s in (0.0099, 0.01, 0.99, 0.9901)] == ["plain", "blend", "blend", "aligned"]
    assert [sa.mode(patch_stylealign(_patcher(), s)) for s in (0.0099, 0.01, 0.99, 0.9901, 0.0, 1.0)] == ["plain", "blend", "blend", "aligned", "plain", "aligned"]
    assert sa.mode(_patcher()) == "plain"


def test_patcher_entry_clones_and_strength_zero_carries_no_option():
    base = _patcher()
    m = patch_stylealign(base)
    assert m is not base and "stylealign" not in base.model_options.get("transformer_options", {})
    assert m.model_options["transformer_options"]["stylealign"] == sa.StyleAlignParams(1.0)
    for s in (0.0, 0.0099):
        assert "stylealign" not in patch_stylealign(base, s).model_options["transformer_options"]
    # a native option, not a Python hook: the executor's fast path stays
    assert UNetExecutor._hooks(m.model_options["transformer_options"]) is None
    # groups of one image: the plain route; otherwise (images per group, mode, strength)
    assert sa.share_for_call(_to(0.5), 1) is None and sa.share_for_call(None, 3) is None and sa.share_for_call({}, 3) is None
    assert sa.share_for_call(_to(0.5), 3) == sa.Share(3, "blend", 0.5) and sa.share_for_call(_to(1.0), 2) == sa.Share(2, "aligned", 1.0)


def test_flux_is_refused_at_the_patcher_and_at_the_model():
    flux = k_model.KModelFlux.__new__(k_model.KModelFlux)
    with pytest.raises(NotImplementedError, match="StyleAlign: UNet models only"):
        patch_stylealign(UnetPatcher(model=flux))
    x = torch.zeros(2, 16, 8, 8)
    with pytest.raises(NotImplementedError, match="StyleAlign: UNet models only"):
        flux.apply_model(x, _sigma(), transformer_options=_to(1.0))
    with pytest.raises(NotImplementedError, match="StyleAlign: UNet models only"):
        flux.denoise_cfg(x, _sigma(), None, (None, None, None), 1.0, transformer_options=_to(1.0))


def test_repeated_and_missing_cond_or_uncond_are_refused_before_any_launch(monkeypatch):
    net, km, packs = _kmodel(monkeypatch)
    net.prepare_context = lambda *a: pytest.fail("refusals come before the context is prepared")
    x = torch.zeros(6, 4, 8, 8)
    ctx = torch.zeros(6, 77, 8)
    with pytest.raises(NotImplementedError, match="StyleAlign.*repeats a value"):
        km.apply_model(x, _sigma(), c_crossattn=ctx, transformer_options=dict(_to(1.0), cond_or_uncond=[0, 0, 1]))
    with pytest.raises(NotImplementedError, match="StyleAlign.*no transformer_options\\['cond_or_uncond'\\]"):
        km.apply_model(x, _sigma(), c_crossattn=ctx, transformer_options=_to(1.0))
    with pytest.raises(NotImplementedError, match="StyleAlign.*does not split"):
        km.apply_model(x[:5], _sigma(), c_crossattn=ctx[:5], transformer_options=dict(_to(1.0), cond_or_uncond=[0, 1]))
    assert packs == [] and net.calls == []
    assert sa.group_size_of_call({"cond_or_uncond": [1, 0]}, 6) == 3 and sa.group_size_of_call({"cond_or_uncond": [0]}, 4) == 4


def test_python_hooks_together_with_the_native_option_are_refused(monkeypatch):
    net, km, packs = _kmodel(monkeypatch)
    x = torch.zeros(3, 4, 8, 8)
    c, uc = (torch.ones(3, 77, 8), None), (torch.zeros(3, 77, 8), None)
    hooked = dict(_to(0.5), patches_replace={"attn1": {("middle", 0): lambda q, k, v, to: v}})
    with pytest.raises(NotImplementedError, match="StyleAlign.*Python block hooks"):
        km.denoise_cfg(x, _sigma(), uc, c, 7.0, transformer_options=hooked)
    with pytest.raises(NotImplementedError, match="StyleAlign.*Python block hooks"):
        km.apply_model(torch.zeros(6, 4, 8, 8), _sigma(), c_crossattn=torch.zeros(6, 77, 8), transformer_options=dict(hooked, cond_or_uncond=[1, 0]))
    with pytest.raises(NotImplementedError, match="StyleAlign.*Python block hooks"):
        km._forward_static((3, 4, 8, 8, 2), x, None, [1.0], 2, None, transformer_options=hooked, native=NativeCall(share=sa.Share(3, "blend", 0.5)))
    with pytest.raises(NotImplementedError, match="StyleAlign.*Python block hooks"):
        UNetExecutor._forward_impl(None, None, None, None, 6, 8, 8, None, to={"patches": {}}, native=NativeCall(share=sa.Share(3, "blend", 0.5)))
    for bu, pag_from in ((7, None), (6, 4)):
        with pytest.raises(ValueError, match="StyleAlign groups of 3"):
            UNetExecutor._forward_impl(None, None, None, None, bu, 8, 8, None, native=NativeCall(pag_from=pag_from, share=sa.Share(3, "aligned", 1.0)))
    assert packs == [] and net.calls == []


def test_a_sharded_batch_is_refused_through_the_check_function():
    mo = patch_stylealign(_patcher(), 0.5).model_options
    with pytest.raises(NotImplementedError, match="StyleAlign.*2 ranks"):
        fdist.check_batch_coupled_options(mo, 2)
    fdist.check_batch_coupled_options(mo, 1)                                  # one rank holds whole groups
    fdist.check_batch_coupled_options(_patcher().model_options, 8)             # no option: nothing couples the images
    fdist.check_batch_coupled_options(None, 8)
    fdist.check_batch_coupled_options(patch_stylealign(_patcher(), 0.0).model_options, 8)


def test_the_sharded_entry_refuses_the_patcher_the_job_samples_with(monkeypatch):
    """process_images_sharded with two ranks and the option installed the way tests/test_gpu_stylealign.py and tools/bench_features.py install
    it -- on forge_objects_after_applying_lora.unet, which sample() copies over forge_objects -- while forge_objects.unet is still the unpatched
    one: refused before any collective (there is no process group here: reaching one fails in torch.distributed, which is how the job without the option ends)."""
    from forge_amd.modules import processing

    class Objs:
        vae = None

        def __init__(self, unet):
            self.unet = unet

        def shallow_copy(self):
            return Objs(self.unet)
    plain, patched = _patcher(), patch_stylealign(_patcher(), 0.5)
    monkeypatch.setattr(fdist, "group_active", lambda: True)
    monkeypatch.setattr(fdist, "world", lambda: (0, 2))

    def job(after_lora, current):
        eng = type("Engine", (), {"device": torch.device("cpu"), "forge_objects_after_applying_lora": Objs(after_lora), "forge_objects": Objs(current)})()
        return processing.StableDiffusionProcessingTxt2Img(sd_model=eng, c=torch.zeros(4, 77, 8), uc=torch.zeros(4, 77, 8), seed=1, batch_size=4,
                                                           steps=2, cfg_scale=7.0, width=32, height=32)
    for after_lora, current in ((patched, plain), (plain, patched), (patched, patched)):
        with pytest.raises(NotImplementedError, match="StyleAlign.*2 ranks"):
            processing.process_images_sharded(job(after_lora, current))
    with pytest.raises(ValueError, match="process group has not been initialized"):       # past the check, at its first collective
        processing.process_images_sharded(job(plain, plain))


def test_every_extension_entry_point_is_named_in_a_gpu_test():
    """tests/test_kernel_test_coverage.py's rule for include/fmx.h, for include/fmx_ext.h: an entry point without a GPU test that names it fails"""
    import glob
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    gpu_tests = "".join(open(f).read() for f in glob.glob(os.path.join(here, "test_gpu_*.py")))
    assert _lib.EXT_SIGNATURES and all(re.search(r"\b" + name + r"\b", gpu_tests) for name in _lib.EXT_SIGNATURES), sorted(_lib.EXT_SIGNATURES)


def test_graph_keys_carry_mode_and_strength_and_b1_is_the_plain_key(monkeypatch):
    net, km, packs = _kmodel(monkeypatch)
    seen = []
    net.forward_packed = lambda *a, **kw: (seen.append((a[3], kw["native"].pag_from, kw["native"].share)), (_ for _ in ()).throw(_Reached()))[1]
    c3, uc3 = (torch.ones(3, 77, 8), None), (torch.zeros(3, 77, 8), None)
    x3, x1 = torch.zeros(3, 4, 8, 8), torch.zeros(1, 4, 8, 8)

    def sig(b):
        s = torch.ones(b, dtype=torch.float64)
        s.fmx_sigma = k_model.SigmaInfo([1.0] * b)
        return s
    for to in (_to(0.5), _to(0.6), _to(1.0), None):
        with pytest.raises(_Reached):
            km.denoise_cfg(x3, sig(3), uc3, c3, 7.0, transformer_options=to)
    base = (3, 4, 8, 8, 2)
    assert list(km._static) == [base + ("stylealign", "blend", 0.5), base + ("stylealign", "blend", 0.6), base + ("stylealign", "aligned", 1.0), base]
    assert list(km._gstate) == list(km._static)
    assert [s for _, _, s in seen] == [sa.Share(3, "blend", 0.5), sa.Share(3, "blend", 0.6), sa.Share(3, "aligned", 1.0), None]
    # one image per group: the same key, hence the same graph, as no option at all
    with pytest.raises(_Reached):
        km.denoise_cfg(x1, sig(1), (torch.zeros(1, 77, 8), None), (torch.ones(1, 77, 8), None), 7.0, transformer_options=_to(0.5))
    assert list(km._static)[-1] == (1, 4, 8, 8, 2) and seen[-1] == (2, None, None)
    # with Perturbed-Attention Guidance and FreeU: the perturbed group is a third group of b images, both keys ride along
    fu = dict(patch_freeu_v2(_patcher(), 1.3, 1.4, 0.9, 0.2).model_options["transformer_options"], **_to(0.5))
    with pytest.raises(_Reached):
        km.denoise_cfg(x3, sig(3), uc3, c3, 7.0, transformer_options=fu, pag_scale=3.0)
    assert seen[-1] == (9, 6, sa.Share(3, "blend", 0.5))
    assert list(km._gstate)[-1] == (3, 4, 8, 8, 2, "pag", "stylealign", "blend", 0.5) + k_model.freeu_graph_key(fu["freeu_v2"])
    # apply_model: the group size from cond_or_uncond
    with pytest.raises(_Reached):
        km.apply_model(torch.zeros(6, 4, 8, 8), sig(6), c_crossattn=torch.zeros(6, 77, 8), transformer_options=dict(_to(1.0), cond_or_uncond=[1, 0]))
    assert seen[-1] == (6, None, sa.Share(3, "aligned", 1.0)) and list(km._static)[-1] == (6, 4, 8, 8, 1, "apply", "stylealign", "aligned", 1.0)


def test_own_attn1_patch_equals_the_references_recorded_outputs():
    """stylealign_refs.stylealign_attn1_patch with torch's scaled_dot_product_attention (what the reference's CPU attention reaches) against what the function compiled
    from the reference's file returned for the same fp32 operands on the CPU (tools/make_stylealign_fixtures.py proc_calls): the same torch ops in
    the same order.  Measured: 0.0 on every call (bit-identical); the gate is 1e-6 max-normalised."""
    calls = load_golden("tiny_stylealign_unet.pt")["proc_calls"]
    assert sorted({c["strength"] for c in calls}) == [0.005, 0.3, 0.5, 1.0] and {tuple(c["cond_or_uncond"]) for c in calls} == {(1, 0), (0,)}
    worst = 0.0
    for c in calls:
        to = {"n_heads": c["heads"], "cond_or_uncond": c["cond_or_uncond"], "cond_indices": c["cond_indices"], "uncond_indices": c["uncond_indices"]}
        got = S.stylealign_attn1_patch(c["strength"], S.cpu_attention)(c["q"], c["k"], c["v"], to)
        assert got.shape == c["out"].shape and got.dtype == torch.float32
        err = float((got - c["out"]).abs().max() / c["out"].abs().max())
        worst = max(worst, err)
        assert err <= 1e-6, (c["strength"], c["cond_or_uncond"], err)
        # and the fp64 reference agrees with both: groups of 3 joined (aligned), b = 1 (ordinary), or the blend
        s = c["strength"]
        own, shared = S.shared_attention_ref(c["q"], c["k"], c["v"], c["heads"], 1), S.shared_attention_ref(c["q"], c["k"], c["v"], c["heads"], 3)
        want = own if s < 0.01 else shared if s > 0.99 else (1.0 - s) * own + s * shared
        assert float((got.double() - want).abs().max()) < 1e-5
    print("restated attn1_proc vs the recorded reference outputs: worst max-normalised error", worst)


@pytest.mark.parametrize("strength", [0.01, 0.3, 0.5, 0.99])
def test_blend_rounding_model_is_the_torch_expression_bit_for_bit(strength):
    g = torch.Generator().manual_seed(int(strength * 1000))
    a, b = torch.randn(100000, generator=g).half(), torch.randn(100000, generator=g).half()
    sa_, sb_ = S.special_values()
    big = (torch.randn(4096, generator=g) * 3.0e4).half()
    tiny = (torch.randn(4096, generator=g) * 1.0e-6).half()
    a, b = torch.cat([a, sa_, big, tiny, big]), torch.cat([b, sb_, big.flip(0), tiny.flip(0), tiny])
    got, want = S.blend_ref(a, b, strength), S.torch_blend(a, b, strength)
    assert got.dtype == want.dtype == torch.float16
    assert int(torch.isnan(want).sum()) > 0 and int(torch.isinf(want).sum()) > 0 and int(((want != 0) & (want.abs() < 6.2e-5)).sum()) > 0
    assert S.same_bits_or_both_nan(got, want) == 0
    # rounding the weights to fp16 first is another function
    wrong = ((a.float() * torch.tensor(1.0 - strength).half().float()).half().float() + (b.float() * torch.tensor(strength).half().float()).half().float()).half()
    if strength != 0.5:
        assert S.same_bits_or_both_nan(wrong[:100000], want[:100000]) > 1000


def test_library_exports_the_symbol_and_checks_its_contract():
    lib = _lib.lib()
    f = lib.fmxe_attn_blend_f16
    i64, f32, vp = C.c_int64, C.c_float, C.c_void_p
    assert _lib.EXT_SIGNATURES == {"fmxe_attn_blend_f16": [vp, vp, vp, f32, f32, i64, vp]} and not set(_lib.EXT_SIGNATURES) & set(_lib.SIGNATURES)
    assert _lib.CONSTANTS["FMX_ABI_VERSION"] == 12 and lib.fmx_abi_version() == 12
    # include/fmx_ext.h under the rules tests/test_capi_symbols.py holds include/fmx.h to: every exported fmxe_* symbol is declared there, every
    # declared one is exported, and the binding lists exactly that set
    text = re.sub(r"/\*.*?\*/", "", open(_lib.EXT_HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(fmxe_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.search(r" T fmxe_", ln)}
    assert declared == exported == set(_lib.EXT_SIGNATURES)
    assert f.argtypes == _lib.EXT_SIGNATURES["fmxe_attn_blend_f16"]
    p = vp(FAKE)
    err = lambda: lib.fmx_last_error().decode()  # noqa: E731
    assert f(vp(0), p, p, 0.5, 0.5, 8, None) == BADARG and f(p, vp(0), p, 0.5, 0.5, 8, None) == BADARG and f(p, p, vp(0), 0.5, 0.5, 8, None) == BADARG
    assert "null" in err()
    assert f(p, p, p, 0.5, 0.5, 0, None) == BADARG and f(p, p, p, 0.5, 0.5, -8, None) == BADARG
    assert f(vp(FAKE + 2), p, p, 0.5, 0.5, 8, None) == BADARG and f(p, p, vp(FAKE + 8), 0.5, 0.5, 8, None) == BADARG and "aligned" in err()
