"""CPU: native FreeU -- the closed form against the real reference's torch.fft implementation (tests/golden/freeu_ops.pt, written by
tools/make_freeu_fixtures.py), the kernels' fp32 summation order against fp64, and the host side: step window, patcher entry, presets, graph
key, fast-path test, Flux refusal, the wrapper's shape check."""
import pytest
import torch

import forge_amd  # noqa: F401
from forge_amd import _lib
from forge_amd import hipops as ops
from forge_amd.backend.modules import k_model
from forge_amd.backend.nn.unet import IntegratedUNet2DConditionModel as UNetExecutor
from forge_amd.backend.patcher import freeu
from forge_amd.backend.patcher.native_call import NativeCall
from forge_amd.backend.patcher.unet import UnetPatcher

from conftest import load_golden
import freeu_refs as fr


@pytest.fixture(scope="module")
def cases():
    return load_golden("freeu_ops.pt")["cases"]


def test_closed_form_matches_the_reference_on_every_case(cases):
    """the seven-sum form + backbone rule (fp64) vs the reference's output_block_patch (fp32, torch.fft): 1e-5 of each tensor's max.  H = 2 (the -1
    bin is the Nyquist bin) and the odd sizes are the cases that could break the closed form."""
    assert [tuple(c["shape"]) for c in cases] == [(2, 64, 64, 2, 2), (1, 128, 64, 5, 7), (2, 128, 192, 8, 8), (1, 64, 32, 6, 3), (1, 256, 128, 48, 40)]
    assert any(c["s"] > 1 for c in cases) and any((c["b"], c["s"]) == (1.3, 0.9) for c in cases) and any((c["b"], c["s"]) == (1.4, 0.2) for c in cases)
    for c in cases:
        h, hsp = fr.case_inputs(c)
        h_out, hsp_out = fr.freeu_ref(h, hsp, c["b"], c["s"])
        if "h_channels" in c:
            h_out, hsp_out = h_out[:, c["h_channels"]], hsp_out[:, c["hsp_channels"]]
        for name, got, ref in (("h", h_out, c["h_out"]), ("hsp", hsp_out, c["hsp_out"])):
            err = float((got - ref.double()).abs().max() / ref.abs().max())
            print(c["shape"], name, err)
            assert err <= 1e-5, (c["shape"], name, err)
        assert float((hsp_out - (hsp if "hsp_channels" not in c else hsp[:, c["hsp_channels"]])).abs().max()) > 1e-3   # the filter does something


def test_kernel_summation_order_in_fp32_is_within_one_fp16_ulp_of_fp64(cases):
    """what the GPU test's 1-ulp gate rests on: the fp32 arithmetic in the kernels' order, rounded to fp16, is the fp64 result rounded to fp16
    or its neighbour, on every element of every case"""
    for c in cases:
        h, hsp = fr.case_inputs(c)
        r_h, r_s = fr.freeu_ref(h, hsp, c["b"], c["s"])
        k_h, k_s = fr.freeu_kernel_order_f32(fr.nhwc16(h), fr.nhwc16(hsp), c["b"], c["s"])
        worst = max(int(fr.ulp_distance_f16(k_h.half(), fr.nhwc16(r_h)).max()), int(fr.ulp_distance_f16(k_s.half(), fr.nhwc16(r_s)).max()))
        print(c["shape"], "worst fp16 ulp distance", worst)
        assert worst <= 1, (c["shape"], worst)
        c_h = h.shape[1]
        assert torch.equal(k_h[..., c_h // 2:].half(), fr.nhwc16(h)[..., c_h // 2:])


def test_freeu_active_is_the_reference_expression():
    table = [(0, 4, 0.0, 0.34), (1, 4, 0.0, 0.34), (2, 4, 0.0, 0.34), (3, 4, 0.0, 0.34), (0, 20, 0.1, 0.9), (2, 20, 0.1, 0.9), (18, 20, 0.1, 0.9),
             (17, 20, 0.1, 0.9), (19, 20, 0.0, 1.0), (5, 11, 0.5, 0.5), (0, 2, 0.5, 1.0), (1, 2, 0.5, 1.0)]
    for step, total, start, end in table:
        this_step = step / (total - 1)
        assert freeu.freeu_active(step, total, start, end) == (this_step >= start and this_step <= end), (step, total, start, end)
    assert [freeu.freeu_active(i, 4, 0.0, 0.34) for i in range(4)] == [True, True, False, False]
    assert freeu.freeu_active(0, 1, 0.0, 1.0) and not freeu.freeu_active(0, 1, 0.5, 1.0)      # one step: position 0.0, no division by zero


def test_patch_freeu_v2_returns_a_clone_and_the_presets_are_there():
    base = UnetPatcher(model=object())
    m = freeu.patch_freeu_v2(base, 1.3, 1.4, 0.9, 0.2)
    assert m is not base and "freeu_v2" not in base.model_options["transformer_options"]
    p = m.model_options["transformer_options"]["freeu_v2"]
    assert p == freeu.FreeUParams(1.3, 1.4, 0.9, 0.2, 0.0, 1.0) and (p.b1, p.b2, p.s1, p.s2, p.start, p.end) == (1.3, 1.4, 0.9, 0.2, 0.0, 1.0)
    w = freeu.patch_freeu_v2(m, 1.1, 1.2, 0.8, 0.7, start=0.2, end=0.6).model_options["transformer_options"]["freeu_v2"]
    assert (w.start, w.end) == (0.2, 0.6) and m.model_options["transformer_options"]["freeu_v2"] is p
    assert freeu.PRESETS["SDXL"][:4] == (1.3, 1.4, 0.9, 0.2) and freeu.PRESETS["Forge default"][:4] == (1.01, 1.02, 0.99, 0.95)
    assert set(freeu.PRESETS) == {"Forge default", "SD 1.4", "SD 1.5", "SD 2.1", "SDXL"}
    assert freeu.PRESETS["SD 1.4"][:4] == (1.3, 1.4, 0.9, 0.2) and freeu.PRESETS["SD 1.5"][:4] == (1.5, 1.6, 0.9, 0.2) and freeu.PRESETS["SD 2.1"][:4] == (1.4, 1.6, 0.9, 0.2)
    # a step outside the window sees a copy without the option; the patcher's dict is not written
    mo = freeu.patch_freeu_v2(base, 1.3, 1.4, 0.9, 0.2, end=0.34).model_options
    assert freeu.options_for_step(mo, 1, 4) is mo
    off = freeu.options_for_step(mo, 2, 4)
    assert "freeu_v2" not in off["transformer_options"] and "freeu_v2" in mo["transformer_options"]


def test_an_options_dict_with_only_freeu_stays_on_the_fast_path():
    assert UNetExecutor._hooks({"freeu_v2": freeu.FreeUParams(1.3, 1.4, 0.9, 0.2)}) is None
    hooked = {"freeu_v2": freeu.FreeUParams(1.3, 1.4, 0.9, 0.2), "patches": {"output_block_patch": [lambda h, s, to: (h, s)]}}
    assert UNetExecutor._hooks(hooked) is hooked


class _Net:
    """the few attributes KModel._forward_static reads before it reaches the graph key"""
    storage_dtype = computation_dtype = torch.float16
    device = torch.device("cpu")
    arena_epoch = 0
    _hooks = staticmethod(UNetExecutor._hooks)

    def __init__(self):
        self.calls = []

    def forward_packed(self, *a, **kw):
        self.calls.append(kw["native"].freeu)
        raise _Reached


class _Reached(Exception):
    pass


def test_graph_key_carries_freeu_and_is_unchanged_without_it(monkeypatch):
    assert k_model.freeu_graph_key(freeu.FreeUParams(1.3, 1.4, 0.9, 0.2)) == ("freeu", 1.3, 1.4, 0.9, 0.2)
    net = _Net()
    km = k_model.KModel(net, type("P", (), {"sigma_data": 1.0, "timestep": staticmethod(lambda s: s)})())
    monkeypatch.setattr(ops, "unet_pack_input", lambda *a, **kw: None)
    monkeypatch.setattr(torch, "empty", lambda *a, **kw: torch.zeros(*a, **{k: v for k, v in kw.items() if k != "device"}))
    x = torch.zeros(1, 4, 8, 8)
    ctxc = type("C", (), {"key": 1, "serial": 1})()
    key = (1, 4, 8, 8, 2)
    for fu in (None, freeu.FreeUParams(1.3, 1.4, 0.9, 0.2)):
        with pytest.raises(_Reached):
            km._forward_static(key, x, None, [1.0], 2, ctxc, native=NativeCall(freeu=fu))
    plain, with_freeu = list(km._gstate)
    assert plain == key                                              # today's key, nothing appended
    assert with_freeu == key + ("freeu", 1.3, 1.4, 0.9, 0.2)
    assert net.calls == [None, freeu.FreeUParams(1.3, 1.4, 0.9, 0.2)]


def test_flux_refuses_freeu():
    km = k_model.KModelFlux.__new__(k_model.KModelFlux)
    to = {"freeu_v2": freeu.FreeUParams(1.3, 1.4, 0.9, 0.2)}
    with pytest.raises(NotImplementedError, match="FreeU: UNet models only"):
        km.apply_model(None, None, transformer_options=to)
    with pytest.raises(NotImplementedError, match="FreeU: UNet models only"):
        km.denoise_cfg(None, None, None, None, 1.0, transformer_options=to)


def test_wrapper_refuses_one_pixel_sides_before_the_library(monkeypatch):
    def boom():
        raise AssertionError("the library must not be reached")
    monkeypatch.setattr(_lib, "lib", boom)
    for shape in ((1, 1, 8, 64), (1, 8, 1, 64)):
        with pytest.raises(ValueError, match="H >= 2 and W >= 2"):
            ops.freeu(torch.zeros(shape, dtype=torch.float16), torch.zeros(shape, dtype=torch.float16), 1.3, 0.9)


def test_geometry_matches_the_header_macro():
    assert ops.freeu_geometry(1, 48 * 40, 128) == (8, 1920 + 16 + 8 * 7 * 128 + 7 * 128 + 4)
    assert ops.freeu_geometry(3, 10, 8)[0] == 1 and ops.freeu_geometry(3, 10, 8)[1] == 32 + 8 + 3 * 7 * 8 + 3 * 7 * 8 + 8


def test_window_with_the_samplers_own_step_numbering(monkeypatch):
    """sampling_function under the Sampler's real bookkeeping: launch_sampling zeroes state.sampling_step and callback_state writes step i AFTER
    model call i, so call i reads max(i - 1, 0) -- one call behind, as the reference's on_cfg_denoiser callback reads it.  A 4-step job with
    the window [0, 0.34] therefore sees the positions 0, 0, 1/3, 2/3: FreeU on calls 0, 1 and 2, off on call 3.  The patcher's dict keeps
    the option throughout."""
    from types import SimpleNamespace
    from forge_amd.backend.sampling import sampling_function as sf
    from forge_amd.modules import sd_samplers_common, shared
    from forge_amd.modules.sd_samplers_cfg_denoiser import CFGDenoiserParams
    monkeypatch.setattr(shared.state, "sampling_step", 0)
    monkeypatch.setattr(shared.state, "sampling_steps", 0)
    seen = []
    monkeypatch.setattr(sf, "compile_conditions", lambda c: None)
    monkeypatch.setattr(sf, "compile_weighted_conditions", lambda c, comp: [])
    monkeypatch.setattr(sf, "sampling_function_inner",
                        lambda model, x, t, uncond, cond, cond_scale, model_options, seed, return_full: seen.append(model_options["transformer_options"].get("freeu_v2")))
    unet = freeu.patch_freeu_v2(UnetPatcher(model=object()), 1.3, 1.4, 0.9, 0.2, start=0.0, end=0.34)
    params = unet.model_options["transformer_options"]["freeu_v2"]
    denoiser = SimpleNamespace(inner_model=SimpleNamespace(inner_model=SimpleNamespace(forge_objects=SimpleNamespace(unet=unet))), p=SimpleNamespace(seeds=[1]))
    sampler = sd_samplers_common.Sampler("sample_euler")
    sampler.model_wrap_cfg, sampler.config = SimpleNamespace(), SimpleNamespace(total_steps=lambda steps: steps)
    read = []

    def euler_shaped_loop():                      # model call, then the sampler's callback with the index of the step just made
        for i in range(4):
            read.append(shared.state.sampling_step)
            sf.sampling_function(denoiser, CFGDenoiserParams(None, None, None, shared.state.sampling_step, shared.state.sampling_steps, None, None), 7.0, None)
            sampler.callback_state({"i": i})
    sampler.launch_sampling(4, euler_shaped_loop)
    assert read == [0, 0, 1, 2]
    assert seen == [params, params, params, None]
    assert unet.model_options["transformer_options"]["freeu_v2"] is params
