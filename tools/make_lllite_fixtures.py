"""TEST INFRASTRUCTURE ONLY.  Generates tests/golden/lllite.pt with the REAL reference: its ControlNet-LLLite library
(<reference>/extensions-builtin/sd_forge_controlllite/lib_controllllite/lib_controllllite.py, loaded from its file at run time: it imports only
math and torch) and, through oracle.ref_import, its UNet, its UnetPatcher's set_model_attn1_patch / set_model_attn2_patch and sampling_function.
Runs only where the reference exists; deterministic (seeded).  Only tensors and settings are written.

    python tools/make_lllite_fixtures.py [--out tests/golden]

lllite.pt
    config (a synth config name: SDXL-shaped, transformers on two levels), weight_seed, lllite_seed, lllite_gain, up_gain: the UNet and the LLLite
    weights are drawn from seeds (synth.synth_unet_state_dict, synth.synth_lllite_state_dict), not stored; modules on attn1 q / k / v and attn2 q
    of every transformer block, conditioning depth 2 on the upper level and 3 on the lower one
    hw, b, bc, image_seed, seed, t, cfg, strengths: a latent of hw, b images per group, bc control images (tests/lllite_refs.control_images)
    cond_emb: {module name: the reference module's cond_emb [bc, n, 32]}, stored as fp16 (28 modules in fp32 would not fit the size limit of a
              committed file; the native embedding is fp16 as well)
    results: {"s<strength>/cfg7" | "s<strength>/cfg1": denoised fp32}, plain: {"cfg7" | "cfg1": denoised fp32 without the patch}
    floor: {the results' names: the reference's own fp16-storage run against its fp32 run}, moved: {...: rms(result - plain) / rms(result)},
    swapped: {...: the same against the run with the two control images swapped}
    counter: [{steps, start, end, active: [bool] over 2.5 x steps calls of the reference module}]
    patch_calls: [{block, block_index, kind, seed, strength, every, out: [q, k, v]}]: the reference's patch object itself on the middle block, called
                 with x = randn(2, 64, 128) (and, for attn2, a context randn(2, 77, 192)) from torch.Generator(seed); of every result the rows
                 ::every are kept (a module works row by row).  tests/test_lllite_host.py holds python_patch to these on the CPU.
Asserted here, on the CPU: every result differs from the plain one, and from the run with the control images swapped, by at least 10 x its floor
in rms.  Training starts `up` at zero; the weights here are drawn non-zero so that a route that drops the adapters cannot pass.
"""
import argparse
import importlib.util
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import forge_amd  # noqa: E402,F401
from forge_amd import synth  # noqa: E402
from oracle import ref_import  # noqa: E402
import lllite_refs as L  # noqa: E402

CONFIG = "TINY_SDXL_2LEVEL_UNET_CONFIG"
WEIGHT_SEED, LLLITE_SEED, IMAGE_SEED, SEED = 0, 21, 5, 611
LLLITE_GAIN, UP_GAIN = 2.0, 0.5
HW, B, BC = (32, 32), 2, 2
T_ALL = [601.0, 187.0]
CFG = 7.0
STRENGTHS = [1.0, 0.5]
WINDOWS = [(0, 0.0, 0.0), (10, 0.0, 0.0), (10, 0.25, 0.7), (7, 0.5, 0.0)]
SEPARATION = 10.0


def reference_library():
    path = os.path.join(ref_import.REFERENCE_ROOT, "extensions-builtin", "sd_forge_controlllite", "lib_controllllite", "lib_controllllite.py")
    spec = importlib.util.spec_from_file_location("_ref_lib_controllllite", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rms_rel(a, ref):
    return float((a.double() - ref.double()).pow(2).mean().sqrt() / ref.double().pow(2).mean().sqrt())


def gen(out_dir):
    import contextlib
    import io
    from oracle import make_floor as mf
    lib = reference_library()
    pred = ref_import.build_ref_predictor()
    cfg = dict(getattr(synth, CONFIG))
    sd = synth.synth_unet_state_dict(cfg, seed=WEIGHT_SEED)
    nets = {"fp32": ref_import.build_ref_unet(cfg, sd), "fp16": mf.half_unet(cfg, sd)}
    lsd = synth.synth_lllite_state_dict(cfg, seed=LLLITE_SEED, gain=LLLITE_GAIN, up_gain=UP_GAIN)
    images = L.control_images(BC, (HW[0] * 8, HW[1] * 8), IMAGE_SEED)
    sigmas = pred.sigma(torch.tensor(T_ALL))
    x, c, uc = L.case_inputs(cfg, HW, SEED, sigmas, B)
    c, uc = ref_import.SdxlCond(c), ref_import.SdxlCond(uc)

    def patch_of(strength, prec, imgs, steps=0, start=0.0, end=0.0):
        with contextlib.redirect_stdout(io.StringIO()):
            return lib.load_control_net_lllite_patch(lsd, imgs, strength, steps, start, end, torch.float32 if prec == "fp32" else torch.float16)

    def run(prec, strength, cs, imgs=images):
        den = ref_import.RefDenoiser(nets[prec], pred, [0])
        den.patcher = den.patcher.clone()
        patch = None
        if strength is not None:
            patch = patch_of(strength, prec, imgs)
            den.patcher.set_model_attn1_patch(patch)
            den.patcher.set_model_attn2_patch(patch)
        den.inner_model.inner_model.forge_objects.unet = den.patcher
        return den(x, sigmas, uc, c, cs), patch

    res = {"config": CONFIG, "weight_seed": WEIGHT_SEED, "lllite_seed": LLLITE_SEED, "lllite_gain": LLLITE_GAIN, "up_gain": UP_GAIN, "hw": HW, "b": B,
           "bc": BC, "image_seed": IMAGE_SEED, "seed": SEED, "t": T_ALL, "cfg": CFG, "strengths": STRENGTHS, "results": {}, "plain": {}, "floor": {},
           "moved": {}, "swapped": {}}
    with torch.no_grad():
        for cs in (CFG, 1.0):
            plain, _ = run("fp32", None, cs)
            res["plain"][f"cfg{int(cs)}"] = plain
            for strength in STRENGTHS:
                tag = f"s{strength}/cfg{int(cs)}"
                r, patch = run("fp32", strength, cs)
                r16, _ = run("fp16", strength, cs)
                rs, _ = run("fp32", strength, cs, images.flip(0))
                res["results"][tag] = r
                res["floor"][tag] = mf.metrics(r16.float(), r)
                res["moved"][tag] = rms_rel(plain, r)
                res["swapped"][tag] = rms_rel(rs, r)
                print(tag, "moved", round(res["moved"][tag], 5), "swapped images", round(res["swapped"][tag], 5), "floor rms_rel",
                      round(res["floor"][tag]["rms_rel"], 6))
                assert min(res["moved"][tag], res["swapped"][tag]) >= SEPARATION * res["floor"][tag]["rms_rel"], tag
                if "cond_emb" not in res:
                    res["cond_emb"] = {name: m.cond_emb.to(torch.float16).clone() for name, m in patch.modules.items()}
                    assert all(m.cond_emb is not None for m in patch.modules.values()) and len(res["cond_emb"]) == len(L_names(lsd))

        # the call counter, on one small reference module per window: active = the module returned something other than zeros
        res["counter"] = []
        g = torch.Generator().manual_seed(3)
        for steps, start, end in WINDOWS:
            start_step = math.floor(steps * start) if start > 0 else 0          # as load_control_net_lllite_patch hands them to the module
            end_step = math.floor(steps * end) if end > 0 else steps
            m = lib.LLLiteModule("m", False, 64, 1, 32, 64, 1.0, steps, start_step, end_step)
            for p in m.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.2)
            m.set_cond_image(torch.rand(1, 3, 64, 64, generator=g) * 2 - 1)
            calls = int(2.5 * steps) if steps else 5
            xs = torch.randn(1, 64, 64, generator=g)
            with contextlib.redirect_stdout(io.StringIO()):
                active = [bool(m(xs).abs().sum() > 0) for _ in range(calls)]
            res["counter"].append({"steps": steps, "start": start, "end": end, "active": active})
            print("counter", (steps, start, end), "".join("x" if a else "." for a in active))

        res["patch_calls"] = []
        for seed, strength, kind in ((1, 1.0, "attn1"), (2, 0.5, "attn2")):
            q, ctx = patch_call_inputs(seed)
            patch = patch_of(strength, "fp32", images)
            kv = q if kind == "attn1" else ctx
            out = patch(q, kv, kv, {"block": ("middle", 0), "block_index": 0})
            assert not torch.equal(out[0], q) and (kind == "attn2") == torch.equal(out[1], kv)
            res["patch_calls"].append({"block": ("middle", 0), "block_index": 0, "kind": kind, "seed": seed, "strength": strength, "every": PATCH_EVERY,
                                       "out": [o[:, ::PATCH_EVERY].clone() for o in out]})

    path = os.path.join(out_dir, "lllite.pt")
    torch.save(res, path)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


PATCH_EVERY = 4


def patch_call_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, 64, 128, generator=g), torch.randn(2, 77, 192, generator=g)


def L_names(lsd):
    return {k.split(".")[0] for k in lsd}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    if not ref_import.reference_available():
        raise SystemExit("the reference is not present: this generator runs only next to it")
    gen(args.out)


if __name__ == "__main__":
    main()
