"""CPU: native Perturbed-Attention Guidance -- the fp32 emulation of fmx_cfg_pag_combine against the fp64 formula and the bound derived in
tests/pag_refs.py, planted bugs against that bound, the reference's step window and attenuation, the reset at sampling_prepare, the patcher entry,
every refusal, the graph keys, and the argument contracts of the two entry points."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import forge_amd  # noqa: F401
from forge_amd import _lib
from forge_amd import hipops as ops
from forge_amd.backend.modules import k_model
from forge_amd.backend.modules.k_prediction import Prediction
from forge_amd.backend.nn.layout import Res, SpatialT
from forge_amd.backend.nn.unet import IntegratedUNet2DConditionModel as UNetExecutor
from forge_amd.backend.patcher import pag
from forge_amd.backend.patcher.freeu import patch_freeu_v2
from forge_amd.backend.patcher.kohya_hrfix import patch_kohya_hrfix
from forge_amd.backend.patcher import native_call as nc
from forge_amd.backend.patcher.native_call import NativeCall
from forge_amd.backend.patcher.stylealign import Share
from forge_amd.backend.patcher.unet import UnetPatcher
from forge_amd.backend.sampling import sampling_function as sf

import kernel_refs as R
import pag_refs as P
import test_gpu_pag as G

BADARG = 10001
FAKE = 0x7F0000001000   # a 16-byte aligned non-null "device pointer": validation never dereferences it


def _patcher(model=None):
    return UnetPatcher(model=model if model is not None else type("M", (), {"predictor": Prediction()})())


# ---- fmx_cfg_pag_combine ------------------------------------------------------------------------------------------------------------------------------
def _combine_all():
    for ptype in G.PTYPES:
        for has_uncond in (True, False):
            for sd in G.SIGMA_DATAS:
                for c, ld in G.CFG_GEOS:
                    for cs in G.COND_SCALES:
                        for ps in G.PAG_SCALES:
                            eps, x, sigma = G.combine_case(has_uncond, c, ld)
                            yield (ptype, has_uncond, sd, c, ld, cs, ps), (eps.values, x.values, sigma.values, has_uncond, cs, ps, ptype, sd)


def test_combine_emulation_meets_the_bound_on_every_case():
    worst = {"denoised": 0.0, "preds": 0.0}
    for key, args in _combine_all():
        res, dc, du, dp, b_res, b_c, b_u, b_p = P.cfg_pag_combine_ref(*args)
        g_res, g_c, g_u, g_p = P.cfg_pag_combine_emul(*args)
        R.assert_within_bound(g_res, res, b_res, f"cfg_pag_combine emulation {key}")
        worst["denoised"] = max(worst["denoised"], R.excess_abs(g_res, res, b_res))
        for got, want, bound in ((g_c, dc, b_c), (g_p, dp, b_p)) + (((g_u, du, b_u),) if key[1] else ()):
            R.assert_within_bound(got, want, bound, f"cfg_pag_combine emulation {key} prediction")
            worst["preds"] = max(worst["preds"], R.excess_abs(got, want, bound))
        # the emulation's cond_pred / uncond_pred are those of the two-group emulation on the same rows
        b = args[1].shape[0]
        rows = args[0][:2 * b] if key[1] else args[0][:b]
        _, e_c, e_u = R.cfg_combine_emul(rows, args[1], args[2], 2 if key[1] else 1, args[4], args[6], args[7])
        assert torch.equal(g_c, e_c) and torch.equal(g_u, e_u), key
    print("cfg_pag_combine emulation, worst ratio to the bound:", worst)
    assert 0.05 < worst["denoised"] <= 1.0     # the bound is not vacuous either


def test_combine_planted_bugs_are_caught():
    for key, args in _combine_all():
        res, _, _, _, b_res, _, _, _ = P.cfg_pag_combine_ref(*args)
        for plant in P.PLANTS:
            e = R.excess_abs(P.cfg_pag_combine_emul(*args, plant=plant)[0], res, b_res)
            assert e > 10.0, (key, plant, e)


# ---- window, attenuation, reset, clone ------------------------------------------------------------------------------------------------------------
def test_window_is_the_references_test():
    for total in (2, 4, 20, 31):
        for start, end in ((0.0, 1.0), (0.0, 0.67), (0.25, 0.5), (0.5, 0.5), (0.6, 0.4)):
            for step in range(total):
                this = step / (total - 1)                      # denoiser_callback
                assert pag.pag_active(step, total, start, end) == (this >= start and this <= end), (step, total, start, end)
    assert [pag.pag_active(s, 4, 0.0, 0.67) for s in range(4)] == [True, True, True, False]
    assert pag.pag_active(0, 1, 0.0, 1.0) and not pag.pag_active(0, 1, 0.1, 1.0)      # a one-step job sits at position 0.0


def test_attenuation_is_the_references_repeated_subtraction():
    for scale, att in ((3.0, 25.0), (3.0, 30.0), (7.3, 0.1), (0.7, 33.3), (3.0, 0.0), (2.0, 100.0)):
        opt = pag.patch_pag(_patcher(), scale, att).model_options["pag"]
        ref = scale                                            # PerturbedAttentionGuidanceForForge.scale
        for _ in range(40):
            assert (pag.pag_for_call({"pag": opt}) is opt) == (not ref <= 0.0)
            if ref <= 0.0:                                     # post_cfg_function returns before the subtraction
                break
            assert opt.scale == ref                            # bit for bit: both are Python floats
            opt.applied()
            ref -= scale * att / 100.0
        assert opt.scale == ref
    opt = pag.patch_pag(_patcher(), 3.0, 30.0).model_options["pag"]
    seen = []
    while pag.pag_for_call({"pag": opt}) is not None:
        seen.append(opt.scale)
        opt.applied()
    assert len(seen) == 4 and seen[0] == 3.0 and 0.0 < seen[-1] < 0.31 and opt.scale < 0.0


def test_patch_pag_defaults_clone_and_reset():
    base = _patcher()
    m = pag.patch_pag(base)
    assert m is not base and "pag" not in base.model_options
    opt = m.model_options["pag"]
    assert tuple(opt.params) == (3.0, 0.0, 0.0, 1.0) and opt.scale == 3.0 and pag.PagParams() == opt.params     # the reference UI's defaults
    again = pag.patch_pag(m, 5.0, 10.0, 0.1, 0.9)
    assert again.model_options["pag"] is not opt and tuple(again.model_options["pag"].params) == (5.0, 10.0, 0.1, 0.9)
    assert m.model_options["pag"] is opt                                     # the parent keeps its own
    assert m.clone().model_options["pag"] is opt                             # a clone of the job's patcher shares the job's state
    assert list(m.model_options["transformer_options"]) == []                # not a transformer option: nothing for the executor's hook test
    # sampling_prepare puts the scale back: a hires second pass starts at the full scale again
    o2 = again.model_options["pag"]
    o2.applied()
    o2.applied()
    assert o2.scale == 5.0 - 0.5 - 0.5
    sf.sampling_prepare(again, None)
    assert o2.scale == 5.0
    sf.sampling_prepare(base, None)                                          # without the option: nothing to do


def test_options_for_step_drops_the_option_outside_the_window_and_at_scale_zero():
    m = pag.patch_pag(_patcher(), 3.0, 25.0, 0.0, 0.67)
    mo = m.model_options
    assert pag.options_for_step(mo, 2, 4) is mo
    out = pag.options_for_step(mo, 3, 4)
    assert "pag" not in out and "pag" in mo and out["transformer_options"] is mo["transformer_options"]
    mo["pag"].scale = 0.0
    assert "pag" not in pag.options_for_step(mo, 0, 4)
    plain = {"transformer_options": {}}
    assert pag.options_for_step(plain, 0, 4) is plain


# ---- sampling_function / sampling_function_inner ------------------------------------------------------------------------------------------------
class _Model:
    """what sampling_function_inner needs of a KModel on the fused route"""
    predictor = Prediction()

    def __init__(self, middle=True):
        self.calls, self.middle = [], middle

    def has_middle_attention(self):
        return self.middle

    def denoise_cfg(self, x, sigma, uctx, cctx, cond_scale, want_parts=False, transformer_options=None, control_model=None, pag_scale=None, **kw):
        self.calls.append((uctx is not None, cond_scale, pag_scale))
        den, cp, up = x * 2.0, x * 3.0, x * 4.0
        if pag_scale is None:
            return den, cp, up
        return den, cp, up, (x * 5.0 if self.middle else None)


def _cond(**extra):
    return dict(model_conds={"c_crossattn": SimpleNamespace(cond=torch.zeros(1, 77, 8))}, **extra)


def test_inner_passes_the_scale_down_and_lowers_it_once_per_model_call(monkeypatch):
    model = _Model()
    m = pag.patch_pag(_patcher(model), 3.0, 25.0)
    opt = m.model_options["pag"]
    x, sigma = torch.ones(1, 4, 8, 8), torch.tensor([1.0])
    post = []
    mo = dict(m.model_options, sampler_post_cfg_function=[lambda a: (post.append(a["denoised"].clone()), a["denoised"] + 100.0)[1]])
    out = sf.sampling_function_inner(model, x, sigma, [_cond()], [_cond()], 7.0, mo)
    out = sf.sampling_function_inner(model, x, sigma, [_cond()], [_cond()], 7.0, mo)         # the second evaluation of a two-evaluation sampler
    out1 = sf.sampling_function_inner(model, x, sigma, [_cond()], [_cond()], 1.0, mo)        # cfg scale 1: no uncond half
    assert model.calls == [(True, 7.0, 3.0), (True, 7.0, 2.25), (False, 1.0, 1.5)] and opt.scale == 0.75
    assert torch.equal(out, x * 2.0 + 100.0) and torch.equal(out1, out)
    assert len(post) == 3 and torch.equal(post[0], x * 2.0)                                  # native PAG first, then the Python post-CFG functions
    # a step whose options lack the entry (outside the window) is an ordinary step: no third group, no decrement
    plain = {k: v for k, v in mo.items() if k != "pag"}
    sf.sampling_function_inner(model, x, sigma, [_cond()], [_cond()], 7.0, plain)
    assert model.calls[-1] == (True, 7.0, None) and opt.scale == 0.75
    opt.scale = 0.0                                                                           # attenuated away: the same
    sf.sampling_function_inner(model, x, sigma, [_cond()], [_cond()], 7.0, mo)
    assert model.calls[-1] == (True, 7.0, None) and opt.scale == 0.0
    # a CFG function replaces the fused combination: the term is added to ITS result from the returned parts
    opt.reset()
    lin = []
    monkeypatch.setattr(ops, "lincomb", lambda srcs, coefs: (lin.append(coefs), sum(s * c for s, c in zip(srcs, coefs)))[1])
    mo2 = dict(m.model_options, sampler_cfg_function=lambda a: a["input"] - a["cond_denoised"] * 10.0)
    got = sf.sampling_function_inner(model, x, sigma, [_cond()], [_cond()], 7.0, mo2)
    assert lin == [[1.0, 3.0, -3.0]] and torch.equal(got, x * 30.0 + (x * 3.0 - x * 5.0) * 3.0) and opt.scale == 2.25
    # a model without a middle transformer: the term is exactly zero, the decrement still happens (the reference subtracts after every call)
    flat = _Model(middle=False)
    got = sf.sampling_function_inner(flat, x, sigma, [_cond()], [_cond()], 7.0, mo2)
    assert torch.equal(got, x * 30.0) and len(lin) == 1 and opt.scale == 1.5


def test_sampling_function_tests_the_window_where_it_does_for_freeu(monkeypatch):
    model = _Model()
    m = pag.patch_pag(_patcher(model), 3.0, 25.0, 0.0, 0.67)
    seen = []
    monkeypatch.setattr(sf, "compile_conditions", lambda c: [_cond()])
    monkeypatch.setattr(sf, "compile_weighted_conditions", lambda c, comp: [_cond()])
    monkeypatch.setattr(sf, "sampling_function_inner", lambda model, x, t, uc, c, cs, mo, seed, return_full: seen.append(mo.get("pag")))
    den = SimpleNamespace(inner_model=SimpleNamespace(inner_model=SimpleNamespace(forge_objects=SimpleNamespace(unet=m))), p=SimpleNamespace(seeds=[0]))
    for step in range(4):
        params = SimpleNamespace(x=torch.zeros(1, 4, 8, 8), sigma=torch.ones(1), text_uncond=None, text_cond=None, image_cond=None,
                                 sampling_step=step, total_sampling_steps=4)
        sf.sampling_function(den, params, 7.0, None)
    opt = m.model_options["pag"]
    assert seen == [opt, opt, opt, None]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------
class _Reached(Exception):
    pass


class _Net:
    """the few attributes KModel reads before it reaches the executor"""
    storage_dtype = computation_dtype = torch.float16
    device = torch.device("cpu")
    arena_epoch = 0
    _hooks = staticmethod(UNetExecutor._hooks)

    def __init__(self, middle_transformer=True):
        self.calls = []
        mid = [Res("middle_block.0", 8, 8)]
        if middle_transformer:
            mid += [SpatialT("middle_block.1", 8, 1, 8, 1, 8, False), Res("middle_block.2", 8, 8)]
        self.layout = SimpleNamespace(middle=mid)

    def prepare_context(self, ctx, y):
        self.ctx_rows = ctx.shape[0]
        return type("C", (), {"key": 1, "serial": 1})()

    def forward_packed(self, *a, **kw):
        self.calls.append((a[3], kw["native"].pag_from, kw["native"].freeu))
        raise _Reached


def _kmodel(monkeypatch, **kw):
    net = _Net(**kw)
    km = k_model.KModel(net, Prediction())
    packs = []
    monkeypatch.setattr(ops, "unet_pack_input", lambda x, s, reps, sd, out=None: packs.append((reps, tuple(out.shape))))
    monkeypatch.setattr(torch, "empty", lambda *a, **k: torch.zeros(*a, **{n: v for n, v in k.items() if n != "device"}))
    return net, km, packs


def _sigma(s=1.0):
    sigma = torch.tensor([s], dtype=torch.float64)
    sigma.fmx_sigma = k_model.SigmaInfo([s])
    return sigma


def test_graph_keys_batch_layout_and_freeu(monkeypatch):
    net, km, packs = _kmodel(monkeypatch)
    x = torch.zeros(1, 4, 8, 8)
    c, uc = (torch.ones(1, 77, 8), None), (torch.zeros(1, 77, 8), None)
    fu = patch_freeu_v2(_patcher(), 1.3, 1.4, 0.9, 0.2).model_options["transformer_options"]
    for uctx, to, scale in ((uc, None, 3.0), (None, None, 3.0), (uc, None, None), (uc, None, 2.25), (uc, fu, 3.0)):
        with pytest.raises(_Reached):
            km.denoise_cfg(x, _sigma(), uctx, c, 7.0, transformer_options=to, pag_scale=scale)
    # (images in the batch, first perturbed image, FreeU): [uncond ; cond ; cond] has 3 b rows and the third group starts at 2 b
    assert [(bu, first) for bu, first, _ in net.calls] == [(3, 2), (2, 1), (2, None), (3, 2), (3, 2)]
    assert net.calls[-1][2] is fu["freeu_v2"] and net.calls[0][2] is None        # native FreeU rides along
    assert [r for r, _ in packs] == [3, 2, 2, 3, 3] and packs[0][1] == (3 * 64, 64)
    # the scale is no part of any key: an attenuated step replays the same graph; inside / outside the window are two graphs
    assert list(km._static) == [(1, 4, 8, 8, 2, "pag"), (1, 4, 8, 8, 1, "pag"), (1, 4, 8, 8, 2)]
    assert list(km._gstate) == [(1, 4, 8, 8, 2, "pag"), (1, 4, 8, 8, 1, "pag"), (1, 4, 8, 8, 2),
                                (1, 4, 8, 8, 2, "pag") + k_model.freeu_graph_key(fu["freeu_v2"])]
    # the perturbed group carries the cond group's context
    ctx, _ = km._stack_ctx_pag(uc, c)
    assert ctx.shape[0] == 3 and float(ctx[0].max()) == 0.0 and float(ctx[1].min()) == 1.0 and torch.equal(ctx[2], ctx[1])
    ctx, _ = km._stack_ctx_pag(None, c)
    assert ctx.shape[0] == 2 and torch.equal(ctx[0], ctx[1])


def test_a_model_without_a_middle_transformer_gets_no_third_group(monkeypatch):
    net, km, packs = _kmodel(monkeypatch, middle_transformer=False)
    assert not km.has_middle_attention()
    with pytest.raises(_Reached):
        km.denoise_cfg(torch.zeros(1, 4, 8, 8), _sigma(), (torch.zeros(1, 77, 8), None), (torch.ones(1, 77, 8), None), 7.0, pag_scale=3.0)
    assert net.calls == [(2, None, None)] and list(km._static) == [(1, 4, 8, 8, 2)]


def test_every_refusal_names_the_feature_and_comes_before_any_launch(monkeypatch):
    name = "Perturbed-Attention Guidance"
    x, sigma = torch.ones(1, 4, 8, 8), _sigma()
    # Flux: at the patcher and at the step
    flux = k_model.KModelFlux.__new__(k_model.KModelFlux)
    with pytest.raises(NotImplementedError, match=name + ": UNet models only"):
        pag.patch_pag(UnetPatcher(model=flux))
    mo = pag.patch_pag(_patcher()).model_options
    with pytest.raises(NotImplementedError, match=name + ": UNet models only"):
        sf.sampling_function_inner(flux, x, sigma, [_cond()], [_cond()], 7.0, mo)
    # a step that is not on the fused route
    model = _Model()
    for kw, what in ((dict(cond=[_cond(area=(4, 4, 0, 0))]), "regional"), (dict(cond=[_cond(timestep_start=5.0)]), "regional"),
                     (dict(uncond=[_cond(mask=torch.ones(1, 8, 8))]), "regional"), (dict(cond=[_cond(), _cond()]), "AND-composed"),
                     (dict(cond=[_cond(strength=0.5)]), "AND-composed"), (dict(uncond=[_cond(), _cond()]), "AND-composed")):
        args = dict(cond=[_cond()], uncond=[_cond()])
        args.update(kw)
        with pytest.raises(NotImplementedError, match=name + ".*" + what):
            sf.sampling_function_inner(model, x, sigma, args["uncond"], args["cond"], 7.0, mo)
    with pytest.raises(NotImplementedError, match=name + ".*model_function_wrapper"):
        sf.sampling_function_inner(model, x, sigma, [_cond()], [_cond()], 7.0, dict(mo, model_function_wrapper=lambda f, a: None))
    assert model.calls == [] and mo["pag"].scale == 3.0                      # refused steps do not consume attenuation either
    # Python block hooks, a ControlNet / T2I chain, Kohya HRFix on the same step: in KModel, before the pack kernel
    net, km, packs = _kmodel(monkeypatch)
    c, uc = (torch.ones(1, 77, 8), None), (torch.zeros(1, 77, 8), None)
    for to in ({"patches": {"attn1_patch": [lambda *a: a]}}, {"patches_replace": {"attn1": {("middle", 0): lambda q, k, v, to: v}}},
               {"block_modifiers": [lambda h, *a: h]}):
        with pytest.raises(NotImplementedError, match=name + ".*Python block hooks"):
            km.denoise_cfg(x, sigma, uc, c, 7.0, transformer_options=to, pag_scale=3.0)
    with pytest.raises(NotImplementedError, match=name + ".*ControlNet"):
        km.denoise_cfg(x, sigma, uc, c, 7.0, control_model=SimpleNamespace(previous_controlnet=None), pag_scale=3.0)
    kohya = patch_kohya_hrfix(_patcher(), 3, 2.0, 0.0, 1.0).model_options["transformer_options"]
    with pytest.raises(NotImplementedError, match=name + " and Kohya HRFix on the same step"):
        km.denoise_cfg(x, sigma, uc, c, 7.0, transformer_options=kohya, pag_scale=3.0)
    late = patch_kohya_hrfix(_patcher(), 3, 2.0, 0.9, 1.0).model_options["transformer_options"]     # its window is elsewhere: this step is fine
    with pytest.raises(_Reached):
        km.denoise_cfg(x, _sigma(10.0), uc, c, 7.0, transformer_options=late, pag_scale=3.0)
    assert len(packs) == 1 and len(net.calls) == 1
    # the same three at the two layers below, for callers that come in there
    ctxc = net.prepare_context(torch.zeros(3, 77, 8), None)
    p = kohya["kohya_hrfix"]
    residuals = {"input": [], "middle": [torch.zeros(1)], "output": []}
    pag2 = NativeCall(pag_from=2)
    for kw, what in ((dict(native=pag2._replace(shrink=p)), "Kohya HRFix"), (dict(control=residuals), "ControlNet"),
                     (dict(control_plan=[{"active": True}]), "ControlNet"), (dict(transformer_options={"patches": {"attn1_patch": [1]}}), "Python block hooks")):
        with pytest.raises(NotImplementedError, match=name + ".*" + what):
            km._forward_static((1, 4, 8, 8, 2, "pag"), x, None, [1.0], 3, ctxc, **dict(dict(native=pag2), **kw))
    for kw, what in ((dict(native=pag2._replace(shrink=p)), "Kohya HRFix"), (dict(control=residuals), "ControlNet"), (dict(to={"patches": {}}), "Python block hooks")):
        with pytest.raises(NotImplementedError, match=name + ".*" + what):
            UNetExecutor._forward_impl(None, None, None, None, 3, 8, 8, None, **dict(dict(native=pag2), **kw))
    with pytest.raises(ValueError, match="pag_from"):
        UNetExecutor._forward_impl(None, None, None, None, 3, 8, 8, None, native=NativeCall(pag_from=3))
    assert len(packs) == 1 and len(net.calls) == 1


# ---- the exclusion table: KModel, the executor and the table itself refuse the same calls with the same words -----------------------------------------
_HOOKED = {"patches": {"attn1_patch": [len]}}
_RESIDUALS = {"input": [], "middle": [torch.zeros(1)], "output": []}


def _field_values():
    """a value for every field of the record that gets a batch of 2 x 2 images past the executor's own value checks"""
    return dict(freeu=patch_freeu_v2(_patcher(), 1.3, 1.4, 0.9, 0.2).model_options["transformer_options"]["freeu_v2"],
                shrink=patch_kohya_hrfix(_patcher(), 3, 2.0, 0.0, 1.0).model_options["transformer_options"]["kohya_hrfix"],
                pag_from=2, share=Share(2, "blend", 0.5), lllite=SimpleNamespace(serial=1, strength=1.0),
                ipadapter=SimpleNamespace(cond_or_uncond=[1, 0], graph_key=lambda: ("ipadapter", 1)))


class _Walk:
    """`self` of _forward_impl for a call that gets past every refusal: the first thing the walk itself touches says so"""
    @property
    def layout(self):
        raise _Reached

    def _lllite_check(self, *a):
        raise _Reached


def _three_levels(km, native, hooks, control):
    x, ctxc = torch.zeros(2, 4, 8, 8), type("C", (), {"key": 1, "serial": 1})()
    return (lambda: nc.check(native, hooks, chain=control is not None, residuals=control is not None),
            lambda: km._forward_static((2, 4, 8, 8, 2), x, None, [1.0, 1.0], 2, ctxc, control=control, transformer_options=hooks, native=native),
            lambda: UNetExecutor._forward_impl(_Walk(), None, None, None, 4, 8, 8, None, control=control, to=hooks, native=native))


@pytest.mark.parametrize("field, excluded, text", nc.RULES, ids=[f"{f}-{e}" for f, e, _ in nc.RULES])
def test_a_call_that_breaks_one_rule_is_refused_with_the_rules_words_at_every_level(field, excluded, text, monkeypatch):
    values = _field_values()
    native = NativeCall(**{k: values[k] for k in (field, excluded) if k in values})
    hooks = _HOOKED if excluded == nc.HOOKS else None
    control = _RESIDUALS if excluded in (nc.CHAIN, nc.RESIDUALS) else None
    present = dict(native._asdict(), hooks=hooks, chain=control, residuals=control)
    assert [r for r in nc.RULES if present[r[0]] is not None and present[r[1]] is not None] == [(field, excluded, text)]     # this rule and no other
    net, km, packs = _kmodel(monkeypatch)
    for level in _three_levels(km, native, hooks, control):
        with pytest.raises(NotImplementedError) as e:
            level()
        assert str(e.value) == text
    assert packs == [] and net.calls == [] and km._static == {}                                                           # before any launch
    assert nc.message(field, excluded) == text


def test_a_call_that_breaks_no_rule_passes_every_level(monkeypatch):
    v = _field_values()
    fine = (nc.PLAIN, NativeCall(freeu=v["freeu"], pag_from=2, share=v["share"]), NativeCall(shrink=v["shrink"], share=v["share"], ipadapter=v["ipadapter"]),
            NativeCall(freeu=v["freeu"], lllite=v["lllite"]), NativeCall(freeu=v["freeu"], ipadapter=v["ipadapter"]))
    for native in fine:
        net, km, packs = _kmodel(monkeypatch)
        by_table, by_kmodel, by_executor = _three_levels(km, native, None, None)
        assert by_table() is None
        for level in (by_kmodel, by_executor):
            with pytest.raises(_Reached):
                level()
        assert len(packs) == 1 and len(net.calls) == 1
    # hooks and residuals alone break nothing either: the plain call runs them eagerly
    net, km, packs = _kmodel(monkeypatch)
    assert nc.check(nc.PLAIN, _HOOKED, chain=True, residuals=True) is None
    with pytest.raises(_Reached):
        km._forward_static((2, 4, 8, 8, 2), torch.zeros(2, 4, 8, 8), None, [1.0, 1.0], 2, None, control=_RESIDUALS, transformer_options=_HOOKED)


# ---- the C entry points -----------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_symbols_and_checks_their_contracts():
    lib = _lib.lib()
    i32, i64, f32, vp = C.c_int32, C.c_int64, C.c_float, C.c_void_p
    assert _lib.SIGNATURES["fmx_attn_value_rows_f16"] == [vp, i64, i64, vp, i64, i64, i32, i32, i32, i32, vp]
    assert _lib.SIGNATURES["fmx_cfg_pag_combine"] == [vp, i32, vp, vp, i32, i32, i32, i32, i32, f32, f32, vp, vp, vp, vp, i32, f32, vp]
    f, g = lib.fmx_attn_value_rows_f16, lib.fmx_cfg_pag_combine
    assert f.argtypes == _lib.SIGNATURES["fmx_attn_value_rows_f16"] and g.argtypes == _lib.SIGNATURES["fmx_cfg_pag_combine"]
    p = vp(FAKE)
    err = lambda: lib.fmx_last_error().decode()  # noqa: E731

    def copy(vt=p, vt_bs=64, vt_ds=128, out=p, o_rs=64, o_bs=64 * 64, hd=64, n=64, b0=1, nb=1):
        return f(vt, vt_bs, vt_ds, out, o_rs, o_bs, hd, n, b0, nb, None)
    assert copy(vt=vp(0)) == BADARG and copy(out=vp(0)) == BADARG and "null" in err()
    assert copy(hd=60) == BADARG and "multiple of 8" in err()
    for kw in (dict(hd=0), dict(n=0), dict(b0=-1), dict(nb=0), dict(nb=65536)):
        assert copy(**kw) == BADARG, kw
    assert copy(vt_bs=63) == BADARG and copy(vt_ds=63) == BADARG and copy(o_rs=56) == BADARG and "below" in err()

    def comb(eps=p, ld=8, x=p, sigma=p, b=1, c=4, h=8, w=8, has_uncond=1, den=p, ptype=0, sd=1.0):
        return g(eps, ld, x, sigma, b, c, h, w, has_uncond, 7.0, 3.0, den, None, None, None, ptype, sd, None)
    for kw in (dict(eps=vp(0)), dict(x=vp(0)), dict(sigma=vp(0)), dict(den=vp(0)), dict(b=0), dict(c=0), dict(h=0), dict(w=0), dict(ld=3),
               dict(has_uncond=2), dict(has_uncond=-1), dict(ptype=3), dict(ptype=-1), dict(sd=0.0)):
        assert comb(**kw) == BADARG and "cfg_pag_combine" in err(), kw
    # fmx_unet_pack_input takes the third group; a fourth is still refused
    pack = lib.fmx_unet_pack_input
    assert pack(p, p, 1.0, 1, 4, 8, 8, 4, p, None) == BADARG and pack(p, p, 1.0, 1, 4, 8, 8, 0, p, None) == BADARG
