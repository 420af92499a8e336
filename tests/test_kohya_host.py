"""CPU: native Kohya HRFix -- the weight tables (modules/latent_upscale.axis_table, with the new mode "area") against F.interpolate /
adaptive_avg_pool2d on every kernel case, the reference's size rule and sigma window, the patcher entry and its refusals, the graph key, and
the argument contract of fmx_resize_nhwc_f16."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import forge_amd  # noqa: F401
from forge_amd import _lib
from forge_amd import hipops as ops
from forge_amd.backend.modules import k_model
from forge_amd.backend.modules.k_prediction import Prediction
from forge_amd.backend.nn.unet import IntegratedUNet2DConditionModel as UNetExecutor
from forge_amd.backend.patcher import kohya_hrfix as kh
from forge_amd.backend.patcher.freeu import patch_freeu_v2
from forge_amd.backend.patcher.native_call import NativeCall
from forge_amd.backend.patcher.unet import UnetPatcher

import kohya_refs as kr

BADARG = 10001
FAKE = 0x7F0000001000   # a 16-byte aligned non-null "device pointer": validation never dereferences it


def _patcher(model=None):
    return UnetPatcher(model=model if model is not None else type("M", (), {"predictor": Prediction()})())


def test_tables_match_torch_for_every_mode_on_every_kernel_case():
    """resize_ref (the kernel's sum, fp64) on fp32 inputs vs F.interpolate(mode, align_corners=False) -- for "area" also adaptive_avg_pool2d --
    to 1e-6 of the tensor's maximum, for each of the four modes at each kernel case's geometry"""
    for i, (shape, size, _) in enumerate(kr.KERNEL_CASES):
        g = torch.Generator().manual_seed(900 + i)
        x = torch.randn(*shape, generator=g)
        for mode in kr.MODES:
            want = F.interpolate(x, size=size, mode=mode)
            if mode == "area":
                assert torch.equal(want, F.adaptive_avg_pool2d(x, size))
            tabs = kr.tables(shape[2], shape[3], size[0], size[1], mode)
            got = kr.resize_ref(x.permute(0, 2, 3, 1), tabs).permute(0, 3, 1, 2)
            err = float((got - want.double()).abs().max() / want.abs().max())
            print(shape, size, mode, "taps", tabs[1].shape[1], "x", tabs[3].shape[1], "err", err)
            assert got.shape == want.shape and err <= 1e-6, (shape, size, mode, err)
    # uneven area windows: 5 -> 3 rows are the windows [0, 2), [1, 4), [3, 5)
    ys, yw = kr.tables(5, 7, 3, 4, "area")[:2]
    assert ys.tolist() == [0, 1, 2] and yw.shape == (3, 3) and yw[1].tolist() == pytest.approx([1 / 3] * 3) and yw[0].tolist() == [0.5, 0.5, 0.0]


def test_size_rule_is_the_references_round():
    assert kh.shrunk_size(12, 16, 1.5) == (8, 11) and kh.shrunk_size(16, 12, 1.5) == (11, 8)     # (height, width): not swapped
    assert kh.shrunk_size(5, 5, 2.0) == (2, 2)                                                   # round(2.5) = 2: ties to even
    for extent, factor in ((12, 1.5), (16, 1.5), (5, 2.0), (33, 2.0), (128, 2.0), (7, 3.0), (96, 1.75)):
        assert kh.shrunk_size(extent, 1, factor)[0] == round(extent * (1.0 / factor))
    assert (round(12 / 1.5), round(16 / 1.5), round(5 / 2.0)) == (8, 11, 2)


class _Reached(Exception):
    pass


class _Net:
    """the few attributes KModel reads before it reaches the executor"""
    storage_dtype = computation_dtype = torch.float16
    device = torch.device("cpu")
    arena_epoch = 0
    _hooks = staticmethod(UNetExecutor._hooks)

    def __init__(self):
        self.calls = []

    def prepare_context(self, ctx, y):
        return type("C", (), {"key": 1, "serial": 1})()

    def forward_packed(self, *a, **kw):
        self.calls.append(kw["native"].shrink)
        raise _Reached


def _kmodel(monkeypatch):
    net = _Net()
    km = k_model.KModel(net, Prediction())
    monkeypatch.setattr(ops, "unet_pack_input", lambda *a, **kw: None)
    monkeypatch.setattr(torch, "empty", lambda *a, **kw: torch.zeros(*a, **{k: v for k, v in kw.items() if k != "device"}))
    return net, km


def test_window_on_the_host_sigmas_both_ends_inclusive(monkeypatch):
    pred = Prediction()
    m = kh.patch_kohya_hrfix(_patcher(), 3, 2.0, 0.2, 0.6, True, "bicubic", "bicubic")
    to = m.model_options["transformer_options"]
    p = to["kohya_hrfix"]
    assert (p.sigma_start, p.sigma_end) == (pred.percent_to_sigma(0.2), pred.percent_to_sigma(0.6)) and p.sigma_end < p.sigma_start
    table = [float(s) for s in pred.sigmas]
    inside = [s for s in table if kh.shrink_for_step(to, [s]) is not None]
    assert inside == [s for s in table if p.sigma_end <= s <= p.sigma_start] and 0 < len(inside) < len(table)
    for s, want in ((p.sigma_start, True), (p.sigma_end, True), (p.sigma_start * (1 + 1e-6), False), (p.sigma_end * (1 - 1e-6), False)):
        assert (kh.shrink_for_step(to, [s]) is p) == want, s
    assert kh.shrink_for_step(to, [p.sigma_start, 0.0]) is p              # the first sample's sigma decides
    assert kh.shrink_for_step({}, [1.0]) is None and kh.shrink_for_step(None, [1.0]) is None
    # start_percent = 0 admits the largest sigma of the table and anything a sampler starts above it
    p0 = kh.patch_kohya_hrfix(_patcher(), 3, 2.0, 0.0, 0.35).model_options["transformer_options"]
    assert kh.shrink_for_step(p0, [max(table)]) is not None and kh.shrink_for_step(p0, [max(table) * 1.5]) is not None
    # KModel hands the option to the executor only inside the window, from the host's copy of sigma
    net, km = _kmodel(monkeypatch)
    x = torch.zeros(1, 4, 8, 8)
    ctx = (torch.zeros(1, 77, 8), None)
    for s in (p.sigma_start, p.sigma_end * 0.5, p.sigma_end, p.sigma_start * 2):
        sigma = torch.tensor([s], dtype=torch.float64)
        sigma.fmx_sigma = k_model.SigmaInfo([s])
        with pytest.raises(_Reached):
            km.denoise_cfg(x, sigma, None, ctx, 1.0, transformer_options=to)
    assert net.calls == [p, None, p, None]
    shrunk, plain = list(km._gstate)
    assert plain == (1, 4, 8, 8, 1) and shrunk == plain + ("kohya_hrfix", 3, 2.0, True, "bicubic", "bicubic")
    assert kh.shrink_graph_key(p) == shrunk[5:]


def test_an_options_dict_with_only_the_option_stays_on_the_fast_path():
    p = kh.patch_kohya_hrfix(_patcher()).model_options["transformer_options"]
    assert list(p) == ["kohya_hrfix"] and UNetExecutor._hooks(p) is None
    hooked = dict(p, patches={"output_block_patch": [lambda h, s, to: (h, s)]})
    assert UNetExecutor._hooks(hooked) is hooked


def test_patch_kohya_hrfix_defaults_clone_and_refusals(monkeypatch):
    base = _patcher()
    m = kh.patch_kohya_hrfix(base)
    assert m is not base and "kohya_hrfix" not in base.model_options["transformer_options"]
    p = m.model_options["transformer_options"]["kohya_hrfix"]
    assert p[:7] == (3, 2.0, 0.0, 0.35, True, "bicubic", "bicubic")           # the reference's defaults, in its argument order
    assert p.sigma_start == 999999999.9 and p.sigma_end == Prediction().percent_to_sigma(0.35)
    q = kh.patch_kohya_hrfix(m, 1, 1.5, 0.1, 0.5, False, "area", "nearest-exact").model_options["transformer_options"]["kohya_hrfix"]
    assert q[:7] == (1, 1.5, 0.1, 0.5, False, "area", "nearest-exact") and m.model_options["transformer_options"]["kohya_hrfix"] is p
    for name in ("lanczos", "nearest", ""):
        with pytest.raises(ValueError, match="unknown resize method"):
            kh.patch_kohya_hrfix(base, downscale_method=name)
        with pytest.raises(ValueError, match="unknown resize method"):
            kh.patch_kohya_hrfix(base, upscale_method=name)
    for kw in (dict(downscale_method="bislerp"), dict(upscale_method="bislerp")):
        with pytest.raises(NotImplementedError, match="Python patches.*remain available"):
            kh.patch_kohya_hrfix(base, **kw)
    with pytest.raises(ValueError, match="downscale_factor"):
        kh.patch_kohya_hrfix(base, downscale_factor=0.0)
    # Flux: at the patcher and at the model
    flux = k_model.KModelFlux.__new__(k_model.KModelFlux)
    with pytest.raises(NotImplementedError, match="Kohya HRFix: UNet models only"):
        kh.patch_kohya_hrfix(UnetPatcher(model=flux))
    to = {"kohya_hrfix": p}
    with pytest.raises(NotImplementedError, match="Kohya HRFix: UNet models only"):
        flux.apply_model(None, None, transformer_options=to)
    with pytest.raises(NotImplementedError, match="Kohya HRFix: UNet models only"):
        flux.denoise_cfg(None, None, None, None, 1.0, transformer_options=to)
    # native FreeU on the same job: at the patcher, in KModel and in the executor
    with pytest.raises(NotImplementedError, match="native FreeU"):
        kh.patch_kohya_hrfix(patch_freeu_v2(base, 1.3, 1.4, 0.9, 0.2))
    both = patch_freeu_v2(m, 1.3, 1.4, 0.9, 0.2).model_options["transformer_options"]
    net, km = _kmodel(monkeypatch)
    x, ctxc = torch.zeros(1, 4, 8, 8), net.prepare_context(None, None)
    with pytest.raises(NotImplementedError, match="native FreeU"):
        km._forward_static((1, 4, 8, 8, 1), x, None, [1.0], 1, ctxc, native=NativeCall(freeu=both["freeu_v2"], shrink=p))
    with pytest.raises(NotImplementedError, match="native FreeU"):
        UNetExecutor._forward_impl(None, None, None, None, 1, 8, 8, None, native=NativeCall(freeu=both["freeu_v2"], shrink=p))
    # ControlNet / T2I residuals with an active shrink (the reference warns and drops the control): eager residuals, a captured chain, the executor
    residuals = {"input": [], "middle": [torch.zeros(1)], "output": []}
    with pytest.raises(NotImplementedError, match="ControlNet"):
        km._forward_static((1, 4, 8, 8, 1), x, None, [1.0], 1, ctxc, control=residuals, native=NativeCall(shrink=p))
    with pytest.raises(NotImplementedError, match="ControlNet"):
        km._forward_static((1, 4, 8, 8, 1), x, None, [1.0], 1, ctxc, control_plan=[{"active": True}], native=NativeCall(shrink=p))
    with pytest.raises(NotImplementedError, match="ControlNet"):
        UNetExecutor._forward_impl(None, None, None, None, 1, 8, 8, None, control=residuals, native=NativeCall(shrink=p))
    assert net.calls == []
    # outside the window the same job runs with its ControlNet: nothing is refused before the executor
    with pytest.raises(_Reached):
        km._forward_static((1, 4, 8, 8, 1), x, None, [1.0], 1, ctxc, control=residuals, native=NativeCall(shrink=None))


def test_wrapper_refuses_other_modes_and_layouts_before_the_library(monkeypatch):
    def boom():
        raise AssertionError("the library must not be reached")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(ops, "_check_f16", lambda *a: None)
    x = torch.zeros(1, 4, 4, 8, dtype=torch.float16)
    for mode in ("bislerp", "nearest", "lanczos"):
        with pytest.raises(ValueError, match="not one of"):
            ops.resize_nhwc(x, (2, 2), mode)
    with pytest.raises(ValueError, match="contiguous NHWC"):
        ops.resize_nhwc(x.permute(0, 3, 1, 2), (2, 2), "bicubic")


def test_library_exports_the_symbol_and_checks_its_contract():
    lib = _lib.lib()
    i32, vp = C.c_int32, C.c_void_p
    assert _lib.SIGNATURES["fmx_resize_nhwc_f16"] == [vp] * 6 + [i32] * 8 + [vp]
    f = lib.fmx_resize_nhwc_f16
    assert f.argtypes == _lib.SIGNATURES["fmx_resize_nhwc_f16"]
    p = vp(FAKE)
    err = lambda: lib.fmx_last_error().decode()  # noqa: E731

    def call(n=1, h=8, w=8, c=64, oh=4, ow=4, ky=4, kx=4, src=p, dst=p):
        return f(src, dst, p, p, p, p, n, h, w, c, oh, ow, ky, kx, None)
    assert call(c=12) == BADARG and "multiple of 8" in err()
    assert call(ky=0) == BADARG and "ky" in err()
    assert call(kx=0) == BADARG and call(ky=9) == BADARG and call(kx=9) == BADARG            # a tap count above the extent cannot be in range
    for kw in (dict(n=0), dict(h=0), dict(w=-1), dict(c=0), dict(oh=0), dict(ow=0)):
        assert call(**kw) == BADARG and "positive" in err(), kw
    assert call(n=4, h=4096, w=4096, c=32, oh=8, ow=8) == BADARG and "overflows" in err()     # n*h*w*c = 2^31
    assert call(n=4, h=8, w=8, c=32, oh=4096, ow=4096) == BADARG and "overflows" in err()
    assert call(src=vp(FAKE + 8)) == BADARG and call(dst=vp(0)) == BADARG
