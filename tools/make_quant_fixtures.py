"""TEST INFRASTRUCTURE ONLY.  Generates tests/golden/quant_reference.json by running the REAL reference on the CPU (imported at run time; nothing of
it is copied).  The file holds names and recorded results only:

  state_dict_dtype   the reference's backend/memory_management.py state_dict_dtype on a list of dtype mixes (marker keys first, else the majority
                     dtype by tensor count, ties to the first seen)
  fp8_storage        for a tiny Flux transformer, T5 encoder and UNet built the way backend/loader.py:100-162 builds them when the component's
                     storage type is float8 (T5: `using_forge_operations(dtype=fp8)`; UNet / Flux: the same plus `.to(dtype=fp8)`), then loaded
                     with `load_state_dict` from a dict whose tensors are stored in a mix of types: every parameter's resulting dtype.  This is
                     the list the loader's mirroring rule (backend/quant_state.py fp8_storage_dtype) is tested against.

    python tools/make_quant_fixtures.py --reference /path/to/reference [--out tests/golden/quant_reference.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MIXES = [
    [("a.weight", "float8_e4m3fn"), ("a.bias", "float8_e4m3fn"), ("b.weight", "bfloat16")],
    [("a.weight", "float8_e5m2"), ("a.bias", "float16"), ("b.weight", "float8_e5m2")],
    [("a.weight", "float16"), ("a.bias", "float8_e4m3fn")],                        # a tie: the first seen wins
    [("a.weight", "float8_e4m3fn"), ("a.bias", "float16")],
    [("a.weight", "float32"), ("a.bias", "float32"), ("b.weight", "float8_e4m3fn")],
    [("a.weight", "bfloat16"), ("b.weight", "float8_e4m3fn"), ("c.weight", "float8_e5m2"), ("d.weight", "float8_e5m2")],
    [("a.weight", "uint8"), ("a.weight.absmax", "float32"), ("a.weight.quant_map", "float32"), ("a.weight.quant_state.bitsandbytes__nf4", "uint8"),
     ("a.bias", "bfloat16")],
    [("a.bias", "float8_e4m3fn"), ("b.bias", "float8_e4m3fn"), ("c.bias", "float8_e4m3fn"), ("a.weight", "uint8"),
     ("a.weight.quant_state.bitsandbytes__fp4", "uint8")],                        # the marker key wins over any majority
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "quant_reference.json"))
    args = ap.parse_args()
    os.environ["FORGE_REFERENCE_ROOT"] = args.reference
    sys.path.insert(0, ROOT)
    import torch
    import transformers.activations  # noqa: F401 -- before the reference's import stubs are installed (oracle/make_golden.py gen_t5)
    import forge_amd  # noqa: F401
    from forge_amd import synth
    from oracle import ref_import
    ref = ref_import.load_reference()
    import importlib
    mm = importlib.import_module("backend.memory_management")
    ops = importlib.import_module("backend.operations")
    t5 = importlib.import_module("backend.nn.t5")
    load_state_dict = importlib.import_module("backend.state_dict").load_state_dict
    cpu = torch.device("cpu")

    def name(dt):
        return dt if isinstance(dt, str) else str(dt).replace("torch.", "")

    out = {"state_dict_dtype": [], "fp8_storage": {}}
    for mix in MIXES:
        sd = {k: torch.zeros(2, dtype=getattr(torch, dt)) for k, dt in mix}
        out["state_dict_dtype"].append({"tensors": [list(m) for m in mix], "result": name(mm.state_dict_dtype(sd))})

    def stored_mix(sd, fp8):
        """fp8 majority; every 5th tensor stays fp16, every 7th bf16, every 11th fp32 (by position), so each kind of parameter meets wider storage"""
        res = {}
        for i, (k, v) in enumerate(sd.items()):
            dt = torch.float32 if i % 11 == 10 else torch.bfloat16 if i % 7 == 6 else torch.float16 if i % 5 == 4 else fp8
            res[k] = v.to(dt)
        return res

    builders = {
        "flux": (lambda: ref.nn_flux.IntegratedFluxTransformer2DModel(**synth.TINY_FLUX_CONFIG), synth.synth_flux_state_dict(synth.TINY_FLUX_CONFIG), True),
        "unet": (lambda: ref.nn_unet.IntegratedUNet2DConditionModel(**{k: (list(v) if isinstance(v, (list, tuple)) and k != "channel_mult" else v)
                                                                       for k, v in synth.TINY_SDXL_UNET_CONFIG.items()}),
                 synth.synth_unet_state_dict(synth.TINY_SDXL_UNET_CONFIG), True),
        "t5": (lambda: t5.IntegratedT5(synth.TINY_T5_CONFIG), {k: v for k, v in synth.synth_t5_state_dict(synth.TINY_T5_CONFIG).items() if k != "logit_scale"}, False),
    }
    for comp, (build, sd, move) in builders.items():
        out["fp8_storage"][comp] = {}
        for fp8 in (torch.float8_e4m3fn, torch.float8_e5m2):
            stored = stored_mix(sd, fp8)
            assert mm.state_dict_dtype(stored) == fp8
            with ops.using_forge_operations(device=cpu, dtype=fp8, manual_cast_enabled=True):      # loader.py:105-107 (T5), :155-160 (UNet / Flux)
                model = build()
                if move:
                    model = model.to(device=cpu, dtype=fp8)
            load_state_dict(model, stored)
            out["fp8_storage"][comp][name(fp8)] = {k: {"stored": name(stored[k].dtype) if k in stored else None, "result": name(v.dtype)}
                                                   for k, v in model.state_dict().items()}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    for comp, kinds in out["fp8_storage"].items():
        for kind, params in kinds.items():
            kept = sorted({k for k, r in params.items() if r["result"] != kind})
            print(comp, kind, len(params), "parameters; not", kind, ":", kept[:12], "..." if len(kept) > 12 else "")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
