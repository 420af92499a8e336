"""CPU: native Dynamic Thresholding -- the restatement against the real reference's outputs (tests/golden/dynthresh_ops.pt, written by
tools/make_dynthresh_fixtures.py), the order-statistic form of the quantile against torch.quantile, the kernels' fp32 summation order against
fp64 (the number the GPU gate is made of), and the host side: schedules, patcher entry, the three sampler-level setters, the fused-route test,
the host-only schedule, the exported symbols."""
import ctypes
import inspect

import pytest
import torch

import forge_amd  # noqa: F401
from forge_amd import _lib
from forge_amd.backend.modules.k_prediction import Prediction, PredictionFlux
from forge_amd.backend.patcher import dynthresh as dt
from forge_amd.backend.patcher.unet import UnetPatcher
from forge_amd.backend.sampling import sampling_function as sf

from conftest import load_golden
import dynthresh_refs as dr

BRANCH = ("mimic", "cfg", "percentile", "separate", "startpoint", "variability", "phi")


@pytest.fixture(scope="module")
def fx():
    return load_golden("dynthresh_ops.pt")


def test_restatement_matches_the_reference_on_every_branch(fx):
    """fp64 restatement vs the reference's fp32 run: within 4 x the reference's own fp32-vs-fp64 distance (the fixture stores it per case)"""
    cases = fx["cases"]
    seen = {(c["separate"], c["startpoint"], c["variability"]) for c in cases}
    assert len(seen) == 8 and {c["phi"] for c in cases} == {1.0, 0.7} and {1.0, 0.99} <= {c["percentile"] for c in cases}
    assert all(c["shape"][2] <= 64 and c["shape"][3] <= 64 for c in cases)
    for c in cases:
        cond, uncond = dr.case_inputs(c)
        ref64 = dr.dynthresh_ref(cond, uncond, *[c[k] for k in BRANCH])
        err = dr.normalised_error(c["out"], ref64)
        print(c["shape"], c["separate"], c["startpoint"], c["variability"], "reference fp32 vs our fp64:", err, "its own:", c["ref_f64_distance"])
        assert err <= 4 * c["ref_f64_distance"], (c, err)
        if c.get("const_row"):
            assert ref64[0, 1].isnan().all() and not ref64[0, 0].isnan().any() and c["out"][0, 1].isnan().all()
        plain = uncond.double() + (cond.double() - uncond.double()) * c["cfg"]
        ok = ~ref64.isnan()
        if c["mimic"] < c["cfg"]:                                          # (a mimic scale above the cfg scale clamps nothing)
            assert float((ref64[ok] - plain[ok]).abs().max()) > 1e-2      # the op does something


def test_kernel_summation_order_in_fp32_against_fp64(fx):
    """the fp32 restatement of the kernels' order against fp64 on every fixture case, normalised by the case's largest |result|.  Its worst
    value is dr.KERNEL_ORDER_WORST; the GPU gate is twice that, and stays under 4 x the reference fp32 run's own distance from fp64."""
    worst = 0.0
    for c in fx["cases"]:
        cond, uncond = dr.case_inputs(c)
        args = [c[k] for k in BRANCH]
        err = dr.normalised_error(dr.dynthresh_kernel_order_f32(cond, uncond, *args), dr.dynthresh_ref(cond, uncond, *args))
        print(c["shape"], c["separate"], c["startpoint"], c["variability"], "kernel order fp32 vs fp64:", err)
        worst = max(worst, err)
    print("worst", worst, "GPU gate", dr.GPU_GATE)
    assert worst <= dr.KERNEL_ORDER_WORST <= 1.05 * worst
    assert dr.GPU_GATE == 2 * dr.KERNEL_ORDER_WORST
    assert dr.GPU_GATE <= 4 * max(c["ref_f64_distance"] for c in fx["cases"])


@pytest.mark.parametrize("n,q", [(65, 0.25), (65, 0.5), (1, 0.0), (1, 1.0), (2, 0.5), (35, 0.99), (1023, 0.999), (4096, 0.9), (4096, 0.0), (4096, 1.0),
                                 (16384, 0.99), (41600, 0.999)])
def test_quantile_restatement_is_torch_quantile(n, q):
    """sort + fp32 position + lerp, bit for bit -- also where q * (N - 1) is an integer (N = 65, q = 0.25) and under heavy ties"""
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g).abs()
    for v in (x, (x * 4).round() / 4, torch.cat([x[:-1], torch.tensor([1e4])]) if n > 1 else x):
        assert torch.equal(dr.quantile_restated(v, q), torch.quantile(v, q)), (n, q)
    if (n, q) == (65, 0.25):
        assert float(torch.tensor(q, dtype=torch.float32) * (n - 1)) == 16.0
        assert dr.quantile_restated(x, q) == x.sort().values[16]


def test_interpret_scale_matches_the_recorded_values(fx):
    m = fx["modes"]
    assert dt.MODES == m["names"] and dt.STARTPOINTS == m["startpoints"] and dt.VARIABILITIES == m["variabilities"]
    for mode in dt.MODES:
        for t in (999, 500, 0):
            got = dt.interpret_scale(m["scale"], mode, m["scale_min"], 999 - t, m["sched_val"])
            assert got == m["values"][mode][t], (mode, t, got, m["values"][mode][t])
    # frac passes 1 at timestep 0: "Linear Down" goes below its minimum, as in the reference
    assert dt.interpret_scale(7.0, "Linear Down", 0.0, 999, 1.0) == 7.0 * (1.0 - 999 / 998)


def test_wrapper_cases_match_the_restatement_at_the_host_schedule(fx):
    """the reference node's sampler_dyn_thresh on a stand-in model with our sigma table vs scales_for_sigma + the fp64 restatement on the denoised
    predictions.  The reference forms input - (input - denoised) on the way in and input - result on the way out: each costs up to an ulp
    of |input|, the first of them scaled by the cfg scale -- (2 cfg + 2) * 2^-23 * max |input|, plus the op's own fp32 distance."""
    pred = Prediction()
    for w in fx["wrapper"]:
        den_c, den_u = dr.case_inputs(w)
        x = den_c + w["sigma"] * torch.randn(w["shape"], generator=torch.Generator().manual_seed(w["x_seed"]))
        params = dt.DynThreshParams(True, *w["params"])
        mimic, cfg = dt.scales_for_sigma(params, pred, [w["sigma"]] * 2, w["cond_scale"])
        step = 999 - w["timestep"]
        assert mimic == dt.interpret_scale(params.mimic_scale, params.mimic_mode, params.mimic_scale_min, step, params.sched_val)
        ref = dr.dynthresh_ref(den_c, den_u, mimic, cfg, params.threshold_percentile, params.separate_feature_channels == "enable",
                               params.scaling_startpoint, params.variability_measure, params.interpolate_phi)
        bound = ((2 * abs(cfg) + 2) * 2.0 ** -23 * float(x.abs().max()) + 1e-6 * float(ref.abs().max())) / float(ref.abs().max())
        err = dr.normalised_error(w["out"], ref)
        print(w["params"], "sigma", w["sigma"], "err", err, "bound", bound)
        assert err <= bound
    assert {w["timestep"] for w in fx["wrapper"]} >= {999, 0}


def test_scales_for_sigma_reads_no_device_tensor_and_follows_flux():
    src = inspect.getsource(dt.scales_for_sigma)
    assert ".item()" in src and "cuda" not in src and ".cpu()" not in src
    p = dt.DynThreshParams(True, 7.0, 1.0, "Linear Up", 0.0, "Linear Down", 0.0, 1.0)
    # host floats in, host floats out: a list is all it gets
    mimic, cfg = dt.scales_for_sigma(p, Prediction(), [14.6146, 14.6146], 12.0)
    assert (mimic, cfg) == (0.0, 12.0)
    # Flux: timestep(sigma) is sigma itself, so step = 999 - sigma
    mimic, cfg = dt.scales_for_sigma(p, PredictionFlux(), [0.75], 3.0)
    step = 999 - float(torch.tensor(0.75))
    assert mimic == 7.0 * (step / 998) and cfg == 3.0 * (1.0 - step / 998)


def test_patch_dynthresh_returns_a_clone_and_the_two_setters_displace_each_other():
    parent = UnetPatcher(model=object())
    args = list(inspect.signature(dt.patch_dynthresh).parameters)
    assert args[1:] == list(dt.DynThreshParams._fields[1:])                      # the argument order of DynamicThresholdingNode.patch
    assert dt.DynThreshParams()[1:] == (7.0, 1.0, "Constant", 0.0, "Constant", 0.0, 1.0, "enable", "MEAN", "AD", 1.0) and len(dt.DynThreshParams._fields) == 12
    m = dt.patch_dynthresh(parent, 7.0, 0.99, "Half Cosine Up", 0.0, "Linear Down", 0.0, 1.0, "enable", "MEAN", "AD", 1.0)
    assert m is not parent and "dynthresh" not in parent.model_options and "sampler_cfg_function" not in m.model_options
    assert m.model_options["dynthresh"] == dt.DynThreshParams(True, 7.0, 0.99, "Half Cosine Up", 0.0, "Linear Down", 0.0, 1.0, "enable", "MEAN", "AD", 1.0)
    fn = lambda args: args["cond"]  # noqa: E731
    m.set_model_sampler_cfg_function(fn)
    assert m.model_options["sampler_cfg_function"] is fn and "dynthresh" not in m.model_options
    m2 = dt.patch_dynthresh(m, 5.0)
    assert "sampler_cfg_function" not in m2.model_options and m2.model_options["dynthresh"].mimic_scale == 5.0
    assert m.model_options["sampler_cfg_function"] is fn                           # the parent of the second clone keeps its own
    with pytest.raises(ValueError):
        dt.patch_dynthresh(parent, 7.0, 1.0, "Cosine Sideways")


def test_sampler_level_setters_write_what_the_reference_writes():
    m = UnetPatcher(model=object())
    old = lambda cond, uncond, cond_scale: uncond + (cond - uncond) * cond_scale  # noqa: E731
    m.set_model_sampler_cfg_function(old)                                          # the three-parameter "old way"
    assert m.model_options["sampler_cfg_function"]({"cond": 3.0, "uncond": 1.0, "cond_scale": 2.0, "input": None}) == 5.0
    assert "disable_cfg1_optimization" not in m.model_options
    m.set_model_sampler_cfg_function(old, disable_cfg1_optimization=True)
    assert m.model_options["disable_cfg1_optimization"] is True
    n = UnetPatcher(model=object())
    a, b, c = (lambda args: args["denoised"]), (lambda args: args["denoised"]), (lambda *a: a)
    n.set_model_sampler_post_cfg_function(a)
    clone = n.clone()
    clone.set_model_sampler_post_cfg_function(b, disable_cfg1_optimization=True)
    clone.set_model_sampler_pre_cfg_function(c)
    assert n.model_options["sampler_post_cfg_function"] == [a] and "sampler_pre_cfg_function" not in n.model_options
    assert clone.model_options["sampler_post_cfg_function"] == [a, b] and clone.model_options["sampler_pre_cfg_function"] == [c]
    assert clone.model_options["disable_cfg1_optimization"] is True and "disable_cfg1_optimization" not in n.model_options


def test_options_with_only_dynthresh_keep_the_fused_route():
    class M:
        def denoise_cfg(self):
            pass
    opts = dt.patch_dynthresh(UnetPatcher(model=M()), 7.0).model_options
    cond = [{"model_conds": {}}]
    assert sf._fused_ok(M(), cond, cond, opts)
    src = inspect.getsource(sf.sampling_function_inner)
    assert 'custom_cfg = "sampler_cfg_function" in model_options' in src       # the option is not a custom CFG function: fused_scale stays cond_scale


def test_library_exports_the_two_symbols():
    handle = ctypes.CDLL(_lib.build())
    assert hasattr(handle, "fmx_row_abs_quantile_f32") and hasattr(handle, "fmx_dynthresh_f32")
    assert len(_lib.SIGNATURES["fmx_row_abs_quantile_f32"]) == 8 and len(_lib.SIGNATURES["fmx_dynthresh_f32"]) == 13
    L = _lib.lib()
    p = ctypes.c_void_p(0x7F0000001000)
    err = lambda: L.fmx_last_error().decode()  # noqa: E731
    assert L.fmx_row_abs_quantile_f32(p, p, 8, 16, 3, 0.5, p, None) == 10001 and "whole groups" in err()
    assert L.fmx_row_abs_quantile_f32(p, p, 8, 16, 1, 1.5, p, None) == 10001 and "[0, 1]" in err()
    assert L.fmx_row_abs_quantile_f32(p, p, 2, 2 ** 31 - 1, 2, 0.5, p, None) == 10001 and "out of range" in err()
    assert L.fmx_dynthresh_f32(p, p, 1, 4, 64, 7.0, 12.0, 1.0, 0, 1.0, p, p, None) == 10001 and "alias" in err()
    q = ctypes.c_void_p(0x7F0000002000)
    assert L.fmx_dynthresh_f32(p, p, 1, 4, 64, 7.0, 12.0, 1.0, 8, 1.0, q, q, None) == 10001     # out == workspace is not checked, flags are
    assert "flag" in err()
    assert L.fmx_dynthresh_f32(p, p, 1, 4, 64, 7.0, 12.0, 2.0, 0, 1.0, q, ctypes.c_void_p(0x7F0000003000), None) == 10001 and "percentile" in err()
