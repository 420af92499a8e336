"""TEST INFRASTRUCTURE ONLY.  Generates tests/golden/dynthresh_ops.pt with the REAL reference: the DynThresh class and the
DynamicThresholdingNode of <reference>/extensions-builtin/sd_forge_dynamic_thresholding/lib_dynamic_thresholding, imported from the
reference tree by path (they need torch and math only).  Runs only where the reference exists; deterministic (seeded).  Only tensors and
settings are written.

    python tools/make_dynthresh_fixtures.py [--out tests/golden]

dynthresh_ops.pt
  cases:   [{shape, seed, checksum, const_row, mimic, cfg, percentile, separate, startpoint, variability, phi, out (the reference's fp32 result on
            the inputs of tests/dynthresh_refs.py case_inputs, schedules "Constant"), ref_f64_distance (max |fp32 run - fp64 run| / max |fp64 run|
            of the reference itself)}]   -- every branch of the scale references, the result and the interpolation
  modes:   {scale, scale_min, sched_val, values: {mode: {timestep: interpret_scale}}} at timesteps 999, 500 and 0
  wrapper: [{shape, seed, sigma, cond_scale, params (the eleven arguments of DynamicThresholdingNode.patch), timestep, out}]: the node's
            sampler_dyn_thresh called with a stand-in model whose predictor is this project's sigma table; out = input - its return value
The inputs are NOT stored: tests re-draw them from `seed` and compare `checksum`.
"""
import argparse
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import forge_amd  # noqa: E402,F401
from forge_amd.backend.modules.k_prediction import Prediction  # noqa: E402
from oracle import ref_import  # noqa: E402

import dynthresh_refs as dr  # noqa: E402

sys.path.insert(0, os.path.join(ref_import.REFERENCE_ROOT, "extensions-builtin", "sd_forge_dynamic_thresholding"))
from lib_dynamic_thresholding.dynthres import DynamicThresholdingNode  # noqa: E402
from lib_dynamic_thresholding.dynthres_core import DynThresh  # noqa: E402

BRANCHES = [(sep, sp, var) for sep in (True, False) for sp in ("MEAN", "ZERO") for var in ("AD", "STD")]


def ops_cases():
    cases, seed = [], 100
    # all eight branches on two small shapes, with the interpolation and a percentile below 1 (ignored by STD)
    for shape in ((2, 4, 5, 7), (1, 4, 33, 31)):
        for sep, sp, var in BRANCHES:
            seed += 1
            cases.append(dict(shape=shape, seed=seed, mimic=7.0, cfg=12.0, percentile=0.99, separate=sep, startpoint=sp, variability=var, phi=0.7))
    # the default branch (separate, MEAN, AD) on every small shape, percentile 1.0 and no interpolation; ties and a degenerate row
    for shape in ((1, 4, 2, 2), (2, 4, 5, 7), (2, 16, 8, 8), (1, 4, 33, 31), (1, 4, 64, 64)):
        seed += 1
        cases.append(dict(shape=shape, seed=seed, mimic=7.0, cfg=12.0, percentile=1.0, separate=True, startpoint="MEAN", variability="AD", phi=1.0))
    cases.append(dict(shape=(1, 4, 64, 64), seed=seed + 1, mimic=5.5, cfg=9.0, percentile=0.999, separate=False, startpoint="MEAN", variability="AD", phi=1.0))
    cases.append(dict(shape=(2, 4, 5, 7), seed=seed + 2, mimic=7.0, cfg=12.0, percentile=0.5, separate=True, startpoint="MEAN", variability="AD", phi=1.0,
                      const_row=True))
    cases.append(dict(shape=(2, 4, 5, 7), seed=seed + 3, mimic=12.0, cfg=7.0, percentile=0.25, separate=True, startpoint="MEAN", variability="AD", phi=0.7))
    return cases


def run_reference(case, cond, uncond):
    d = DynThresh(case["mimic"], case["percentile"], "Constant", 0.0, "Constant", 0.0, 1.0, 0, 999, case["separate"], case["startpoint"],
                  case["variability"], case["phi"])
    d.step = 0
    return d.dynthresh(cond, uncond, case["cfg"], None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()

    cases = ops_cases()
    for c in cases:
        cond, uncond = dr.case_inputs(c)
        c["checksum"] = (float(cond.double().sum()), float(uncond.double().sum()))
        c["out"] = run_reference(c, cond, uncond)
        c["ref_f64_distance"] = dr.normalised_error(c["out"], run_reference(c, cond.double(), uncond.double()))
        print(c["shape"], c["separate"], c["startpoint"], c["variability"], "reference fp32 vs fp64:", c["ref_f64_distance"])

    scale, scale_min, sched_val = 7.0, 1.5, 2.5
    values = {}
    for mode in DynThresh.Modes:
        d = DynThresh(scale, 1.0, mode, scale_min, mode, scale_min, sched_val, 0, 999, True, "MEAN", "AD", 1.0)
        values[mode] = {}
        for t in (999, 500, 0):
            d.step = 999 - t
            values[mode][t] = d.interpret_scale(scale, mode, scale_min)
    modes = dict(scale=scale, scale_min=scale_min, sched_val=sched_val, values=values, names=list(DynThresh.Modes),
                 startpoints=list(DynThresh.Startpoints), variabilities=list(DynThresh.Variabilities))

    predictor = Prediction()                      # the SD / SDXL table of this project
    wrapper = []
    for i, (params, sigma, cond_scale) in enumerate([
            ((7.0, 0.99, "Half Cosine Up", 0.0, "Linear Down", 0.0, 1.0, "enable", "MEAN", "AD", 1.0), 14.6146, 12.0),
            ((7.0, 1.0, "Constant", 0.0, "Constant", 0.0, 1.0, "enable", "MEAN", "AD", 1.0), 2.0, 9.0),
            ((6.0, 0.9, "Power Up", 1.0, "Cosine Repeating", 2.0, 2.5, "disable", "ZERO", "STD", 0.7), 0.0292, 10.0)]):
        case = dict(shape=(2, 4, 8, 8), seed=900 + i)
        den_c, den_u = dr.case_inputs(case)
        g = torch.Generator().manual_seed(950 + i)
        x = den_c + sigma * torch.randn(case["shape"], generator=g)
        captured = {}
        stub = SimpleNamespace(model=SimpleNamespace(predictor=predictor))
        stub.clone = lambda: SimpleNamespace(set_model_sampler_cfg_function=lambda fn: captured.__setitem__("fn", fn))
        DynamicThresholdingNode().patch(stub, *params)
        sig = torch.full((2,), sigma)
        out = x - captured["fn"]({"input": x, "cond": x - den_c, "uncond": x - den_u, "cond_scale": cond_scale, "sigma": sig})
        wrapper.append(dict(case, sigma=sigma, cond_scale=cond_scale, params=params, x_seed=950 + i, timestep=int(predictor.timestep(sig)[0]), out=out,
                            checksum=(float(den_c.double().sum()), float(den_u.double().sum()))))

    path = os.path.join(args.out, "dynthresh_ops.pt")
    torch.save({"cases": cases, "modes": modes, "wrapper": wrapper}, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
