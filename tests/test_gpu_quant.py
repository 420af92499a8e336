"""GPU: the storage-expansion kernels (fmx_fp8_expand_* through ops.fp8_expand, fmx_bnb4_dequant_* through ops.bnb4_dequant) and the loader
route built on them (float8 and bitsandbytes NF4 / FP4 checkpoints).

Every comparison is EXACT.  fp8: all codes are representable in fp16 and bf16, so the output is the code's value.  bnb4: code16[nibble] * scale
in fp32, rounded once to the output type -- the 16-bit patterns equal the 16-bit rounding (torch's, to nearest even) of tests/quant_refs.py.
NaNs are compared by position, and must be quiet.  The end-to-end tests build the same engine twice -- from a file written at test time and
from the same values expanded on the host -- and compare weights, one forward and two Euler steps bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import forge_amd  # noqa: E402
import quant_refs as Q  # noqa: E402
from conftest import ROOT, load_golden  # noqa: E402
from forge_amd import _lib, hipops as ops, synth  # noqa: E402
from forge_amd.backend import loader, quant_state as QS  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
import bnb_write as W  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
DTYPES = [torch.float16, torch.bfloat16]
FP8 = {"e4m3fn": (Q.E4M3FN, torch.float8_e4m3fn), "e5m2": (Q.E5M2, torch.float8_e5m2)}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- fp8 -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("kind", sorted(FP8))
def test_fp8_all_256_codes(kind, dtype):
    k, fp8 = FP8[kind]
    codes = np.arange(256, dtype=np.uint8)
    out = ops.fp8_expand(dev(codes), k, (16, 16), dtype)
    assert out.shape == (16, 16) and out.dtype == dtype
    Q.assert_same_bits(out, Q.fp8_expand(codes, k), f"{kind} -> {dtype}")
    got = out.reshape(-1).cpu()
    want = torch.from_numpy(codes).view(fp8).to(dtype)                   # torch's own conversion, as bits
    nan = torch.isnan(want)
    assert torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan]) and torch.equal(torch.isnan(got), nan)
    quiet = 0x0200 if dtype == torch.float16 else 0x0040
    assert bool(((got.view(torch.int16)[nan].int() & quiet) != 0).all())  # NaN codes: a quiet NaN
    assert got.view(torch.int16)[0x80].item() == -32768                   # -0
    for spelled in (fp8, "fp8_" + kind):                                  # the kind by torch dtype and by scheme name
        assert torch.equal(ops.fp8_expand(dev(codes), spelled, (256,), dtype).view(torch.int16), out.reshape(-1).view(torch.int16))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("kind", sorted(FP8))
def test_fp8_sizes_around_the_vector_and_the_chunk(kind, dtype):
    """1, 7, 8, 9: the 8-weight vector and its tail; 255; 8192, 8193: one workgroup step and one weight more; 3 * 8192 + 5: several steps"""
    k, _ = FP8[kind]
    for n in (1, 7, 8, 9, 255, 8192, 8193, 3 * 8192 + 5):
        codes = np.random.default_rng([n, k]).integers(0, 256, n, dtype=np.uint8)
        guard = torch.full((n + 64,), -1, dtype=torch.int16, device=DEV).view(dtype)          # out is a window: nothing behind it may be written
        out = ops.fp8_expand(dev(codes), k, (n,), dtype, out=guard[:n])
        torch.cuda.synchronize()
        Q.assert_same_bits(out, Q.fp8_expand(codes, k), f"{kind} x {n} -> {dtype}")
        assert bool((guard[n:].view(torch.int16) == -1).all()), f"{kind} x {n}: wrote past the end"


# ---- bnb4 ------------------------------------------------------------------------------------------------------------------------------------------------
SIZES = [(64, 1), (64, 63), (64, 64), (64, 65), (64, 127), (64, 64 * 256), (64, 64 * 256 + 65), (128, 129), (4096, 4097), (64, 3 * 8192 + 3)]


def _state(c, quant_type, nested):
    n = c["n"]
    if nested:
        return QS.BnbQuantState(quant_type, (n,), c["blocksize"], dev(c["code16"]), dev(c["absmax"]), True, dev(c["code256"]), dev(c["absmax2"]),
                                c["blocksize2"], float(c["offset"]), None)
    return QS.BnbQuantState(quant_type, (n,), c["blocksize"], dev(c["code16"]), dev(c["absmax"]), False, None, None, 0, 0.0, None)


def _flat_case(n, blocksize, code16, seed):
    """random bytes; absmax values include 0, an fp32 denormal, a negative value and one that overflows fp16"""
    rng = np.random.default_rng([seed, n, blocksize])
    nblocks = (n + blocksize - 1) // blocksize
    absmax = rng.uniform(0.01, 4.0, nblocks).astype(np.float32)
    special = np.array([1e6, 0.0, 1e-40, -0.75], dtype=np.float32)
    if nblocks >= 4:
        absmax[:4] = special
    else:
        absmax[0] = special[seed % 4]
    return dict(packed=rng.integers(0, 256, (n + 1) // 2, dtype=np.uint8), n=n, code16=code16, blocksize=blocksize, absmax=absmax)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("nested", [False, True], ids=["flat", "nested"])
@pytest.mark.parametrize("quant_type", ["nf4", "fp4"])
def test_bnb4_bit_for_bit(quant_type, nested, dtype):
    """the sizes cover: an odd tail nibble (1, 63, 65, 127, ...); block boundaries beside a partial group of 8 (63 / 65 / 129 / 4097) -- a lane's 8
    weights start at a multiple of 8 and every block size is a multiple of 64, so no group straddles a block; nested-block crossings (64 * 256
    weights with blocksize2 64: four nested blocks; 64 * 256 + 65 with blocksize2 256: two); several workgroup steps (3 * 8192 + 3)"""
    code16 = W.TABLES[quant_type]
    for seed, (blocksize, n) in enumerate(SIZES):
        if nested:
            c = Q.nested_case(n, blocksize, 256 if n > 64 * 256 else 64, code16, W.nested_table(seed), seed)
            assert Q.bnb4_scales(n, blocksize, c["absmax"], c["code256"], c["absmax2"], c["offset"], c["blocksize2"])[0] == 0.0   # the add cancels in block 0
        else:
            c = _flat_case(n, blocksize, code16, seed)
        guard = torch.full((n + 64,), -1, dtype=torch.int16, device=DEV).view(dtype)
        out = ops.bnb4_dequant(dev(c["packed"]), _state(c, quant_type, nested), dtype, out=guard[:n])
        torch.cuda.synchronize()
        Q.assert_same_bits(out, Q.bnb4_dequant(**c), f"{quant_type} {'nested' if nested else 'flat'} blocksize {blocksize} x {n} -> {dtype}")
        assert bool((guard[n:].view(torch.int16) == -1).all()), f"{quant_type} x {n}: wrote past the end"
        if not nested and n >= 4 * blocksize:
            o = out.cpu().float()
            if dtype == torch.float16:
                assert torch.isinf(o[:blocksize]).any()                  # 1e6 * |code| > 65504: inf, as torch's cast gives
            assert bool((o[blocksize:2 * blocksize] == 0).all())


def test_bnb4_two_dimensional_shape_and_default_output():
    c = _flat_case(96 * 70, 64, W.TABLES["nf4"], 1)
    st = _state(c, "nf4", False)._replace(shape=(96, 70))
    out = ops.bnb4_dequant(dev(c["packed"]), st, BF)
    assert out.shape == (96, 70) and out.dtype == BF
    Q.assert_same_bits(out, Q.bnb4_dequant(**c), "nf4 96 x 70")


def test_wrappers_refuse_what_they_cannot_expand():
    raw = torch.zeros(64, dtype=torch.uint8, device=DEV)
    c = _flat_case(128, 64, W.TABLES["nf4"], 0)
    st = _state(c, "nf4", False)
    with pytest.raises(TypeError):
        ops.fp8_expand(raw.cpu(), 0, (64,), BF)                          # a host tensor
    with pytest.raises(TypeError):
        ops.bnb4_dequant(raw.cpu(), st, BF)
    with pytest.raises(ValueError):
        ops.fp8_expand(raw, 0, (65,), BF)                                # wrong byte count
    with pytest.raises(ValueError):
        ops.bnb4_dequant(raw[:63], st, BF)
    with pytest.raises(TypeError):
        ops.fp8_expand(raw, 0, (64,), torch.float32)                     # only 16-bit outputs
    with pytest.raises(TypeError):
        ops.bnb4_dequant(raw, st, torch.float32)
    with pytest.raises(ValueError, match="blocksize"):
        ops.bnb4_dequant(raw, st._replace(blocksize=48), BF)
    with pytest.raises(ValueError, match="blocksize"):
        ops.bnb4_dequant(raw, st._replace(blocksize=32), BF)
    for bad_out in (torch.empty(63, dtype=BF, device=DEV), torch.empty(64, dtype=torch.float16, device=DEV), torch.empty(64, dtype=BF),
                    torch.empty(128, dtype=BF, device=DEV)[::2]):    # too short, the other element type, on the host, strided
        with pytest.raises(ValueError, match="out must be"):
            ops.fp8_expand(raw, 0, (64,), BF, out=bad_out)
    with pytest.raises(ValueError, match="out must be"):
        ops.bnb4_dequant(raw, st, BF, out=torch.empty(127, dtype=BF, device=DEV))
    with pytest.raises(_lib.FmxError, match="10002"):
        ops.fp8_expand(raw, 2, (64,), BF)                                # fnuz and anything else: FMX_E_UNSUPPORTED
    with pytest.raises(_lib.FmxError, match="10001"):
        ops.fp8_expand(raw[4:], 0, (60,), BF)                            # src not 8-byte aligned


# ---- the loader route ------------------------------------------------------------------------------------------------------------------------------------
def _save(path, sd):
    from safetensors.torch import save_file
    save_file({k: v.contiguous() for k, v in sd.items()}, str(path))
    return str(path)


def _flux_file(tmp, form):
    """tiny Flux transformer stored as `form` -> (path, {name: fp32 values of the file})"""
    sd = synth.synth_flux_state_dict(synth.TINY_FLUX_CONFIG, seed=2)
    if form in FP8:
        stored = {k: v.to(FP8[form][1]) for k, v in sd.items()}
    else:
        stored = W.pack_state_dict({k: v.to(BF) for k, v in sd.items()}, form.split("-")[0], nested="nested" in form, nested_blocksize=64)
    return _save(tmp / f"tiny_flux_{form}.safetensors", stored), Q.state_dict_reference(stored)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("quant")
    return {form: _flux_file(tmp, form) for form in ("e4m3fn", "e5m2", "nf4-nested")}, tmp


def _tensors(w):
    for k, v in w.items():
        for i, t in enumerate(v if isinstance(v, (tuple, list)) else (v,)):
            if isinstance(t, torch.Tensor):
                yield f"{k}[{i}]", t


def _same_weights(net, ref_net, least=40):
    got, want = dict(_tensors(net.w)), dict(_tensors(ref_net.w))
    assert set(got) == set(want) and len(got) > least
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].dtype != torch.uint8 and "float8" not in str(got[k].dtype), k
        assert torch.equal(got[k].view(torch.int16) if got[k].element_size() == 2 else got[k], want[k].view(torch.int16) if want[k].element_size() == 2 else want[k]), k


def _flux_inputs():
    g = load_golden("tiny_flux_fwd.pt")
    return g, [g[k].to(DEV) for k in ("x", "t", "ctx", "y", "guidance")]


def _two_euler_steps(eng, g):
    from forge_amd.modules import processing
    from forge_amd.modules.prompt_parser import DictWithShape
    import forge_amd.modules.rng as rng_mod
    h, w = g["hw"]
    cond = DictWithShape({"crossattn": g["ctx"].to(DEV), "vector": g["y"].to(DEV), "guidance": g["guidance"].to(DEV)})
    p = processing.StableDiffusionProcessingTxt2Img(sd_model=eng, c=cond, uc=cond, seed=0, sampler_name="Euler", scheduler="simple", batch_size=2, steps=2,
                                                    cfg_scale=1.0, width=w * 8, height=h * 8, do_decode=False)

    class FixedNoise:
        def next(self_inner):
            return g["noise"].to(DEV)
    orig = rng_mod.ImageRNG
    rng_mod.ImageRNG = lambda *a, **k: FixedNoise()
    try:
        return processing.process_images(p).latents
    finally:
        rng_mod.ImageRNG = orig


@pytest.mark.parametrize("form", ["e4m3fn", "e5m2", "nf4-nested"])
def test_flux_engine_from_a_quantised_file_equals_the_pre_expanded_one(files, form):
    from forge_amd.backend.diffusion_engine.base import build_flux_engine
    cfg = synth.TINY_FLUX_CONFIG
    path, ref_sd = files[0][form]
    eng = loader.forge_loader(path, device=DEV)
    assert eng.model_guess["flux_config"] == cfg and eng.model_guess["dtype"] == BF
    ref_eng = build_flux_engine(cfg, ref_sd, device=DEV, dtype=BF)
    net, ref_net = eng.forge_objects.unet.model.diffusion_model, ref_eng.forge_objects.unet.model.diffusion_model
    assert net.dtype == BF
    _same_weights(net, ref_net)
    g, args = _flux_inputs()
    out, ref_out = net.forward(*args), ref_net.forward(*args)
    assert torch.isfinite(out.float()).all() and torch.equal(out, ref_out)
    lat, ref_lat = _two_euler_steps(eng, g), _two_euler_steps(ref_eng, g)
    assert torch.isfinite(lat.float()).all() and torch.equal(lat, ref_lat)


def test_wider_tensors_in_an_fp8_majority_are_rounded_to_fp8(files):
    """the reference's fp8 storage (tests/golden/quant_reference.json): the component's storage type is the majority's, the module is built in it and
    load_state_dict rounds what was stored wider -- matrices, biases and norm scales alike in a Flux transformer"""
    from forge_amd.backend.diffusion_engine.base import build_flux_engine
    cfg = synth.TINY_FLUX_CONFIG
    sd = synth.synth_flux_state_dict(cfg, seed=2)
    wide = {"img_in.weight": BF, "double_blocks.0.img_attn.qkv.bias": torch.float16, "double_blocks.0.img_attn.norm.key_norm.scale": torch.float32}
    stored = {k: v.to(wide.get(k, torch.float8_e4m3fn)) for k, v in sd.items()}
    path = _save(files[1] / "tiny_flux_mixed.safetensors", stored)
    ref_sd = {k: v.to(torch.float8_e4m3fn).float() for k, v in stored.items()}
    assert not torch.equal(ref_sd["img_in.weight"], stored["img_in.weight"].float())
    net = loader.forge_loader(path, device=DEV).forge_objects.unet.model.diffusion_model
    _same_weights(net, build_flux_engine(cfg, ref_sd, device=DEV, dtype=BF).forge_objects.unet.model.diffusion_model)


def _t5_stored(form):
    sd = {k[len("transformer."):]: v for k, v in synth.synth_t5_state_dict(synth.TINY_T5_CONFIG).items() if k != "logit_scale"}
    if form == "fp8":
        wide = {"encoder.block.1.layer.0.layer_norm.weight": torch.float16, "encoder.block.1.layer.0.SelfAttention.q.weight": torch.float16}
        stored = {k: v.to(wide.get(k, torch.float8_e4m3fn)) for k, v in sd.items()}
        ref = {}
        for k, v in stored.items():      # Linear weights: fp8 (rounded when stored wider); layer norms and the two embeddings: fp32 of what is stored
            ref[k] = v.float() if QS.fp8_storage_dtype("t5", k) == torch.float32 else v.to(torch.float8_e4m3fn).float()
        assert not torch.equal(ref["encoder.block.1.layer.0.SelfAttention.q.weight"], stored["encoder.block.1.layer.0.SelfAttention.q.weight"].float())
        assert torch.equal(ref["encoder.block.1.layer.0.layer_norm.weight"], stored["encoder.block.1.layer.0.layer_norm.weight"].float())
        return stored, ref
    linear = lambda k, v: v.dim() == 2 and k.endswith(".weight") and "shared" not in k and "relative_attention_bias" not in k  # noqa: E731
    stored = W.pack_state_dict({k: v.to(BF) for k, v in sd.items()}, "nf4", select=linear, nested=True, nested_blocksize=64)
    return stored, Q.state_dict_reference(stored)


@pytest.mark.parametrize("form", ["fp8", "nf4"])
def test_t5_through_additional_state_dicts(files, form):
    from forge_amd.backend.nn.t5 import IntegratedT5
    cfg = synth.TINY_T5_CONFIG
    stored, ref = _t5_stored(form)
    t5_path = _save(files[1] / f"tiny_t5_{form}.safetensors", stored)
    eng = loader.forge_loader(files[0]["e4m3fn"][0], device=DEV, additional_state_dicts=[t5_path])
    sd = eng.text_encoder_state_dicts["t5xxl"]
    ref_sd = {"transformer." + k: v for k, v in ref.items()}
    assert set(sd) == set(ref_sd) and all(isinstance(v, torch.Tensor) and "float8" not in str(v.dtype) and v.dtype != torch.uint8 for v in sd.values())
    ids = load_golden("tiny_t5.pt")["ids"].to(DEV)
    enc, ref_enc = IntegratedT5(cfg, sd, device=DEV, dtype=BF), IntegratedT5(cfg, ref_sd, device=DEV, dtype=BF)
    for k in ref_enc.w:
        if isinstance(ref_enc.w[k], torch.Tensor):
            assert torch.equal(enc.w[k], ref_enc.w[k]), k
    z, z_ref = enc.transformer(ids), ref_enc.transformer(ids)
    z, z_ref = (z if isinstance(z, torch.Tensor) else z[0]), (z_ref if isinstance(z_ref, torch.Tensor) else z_ref[0])
    assert torch.isfinite(z.float()).all() and torch.equal(z, z_ref)


def test_sd_unet_in_fp8_through_split_state_dict(files):
    cfg = synth.TINY_SD15_UNET_CONFIG
    base = synth.synth_unet_state_dict(cfg, seed=0)
    first = next(iter(base))
    stored = {loader.UNET_PREFIX + k: (v.half() if k == first else v.to(torch.float8_e4m3fn)) for k, v in base.items()}
    path = _save(files[1] / "tiny_sd15_fp8.safetensors", stored)
    parts, guess = loader.split_state_dict(path)
    assert guess["unet_config"] == loader.split_state_dict({loader.UNET_PREFIX + k: v.half() for k, v in base.items()})[1]["unet_config"]
    assert all(QS.is_packed(v) for v in parts["unet"].values())
    ref = {k: v.to(torch.float8_e4m3fn).half() for k, v in stored.items()}      # every STORED tensor through fp8 (the fp16 one is rounded), then exact in fp16
    net = loader.forge_loader(path, device=DEV).forge_objects.unet.model.diffusion_model
    ref_net = loader.forge_loader(ref, device=DEV).forge_objects.unet.model.diffusion_model
    fx = load_golden("tiny_sd15_unet_fwd.pt")
    args = (fx["x"].to(DEV), fx["t"].to(DEV))
    eps, ref_eps = net.forward(*args, context=fx["ctx"].to(DEV), y=None), ref_net.forward(*args, context=fx["ctx"].to(DEV), y=None)
    assert torch.isfinite(eps.float()).all() and torch.equal(eps, ref_eps)


def test_lora_merges_onto_nf4_weights_as_onto_pre_expanded_ones(files):
    from forge_amd.backend.patcher import lora as nlora
    from oracle.make_golden import synth_flux_lora
    cfg = synth.TINY_FLUX_CONFIG
    path, ref_sd = files[0]["nf4-nested"]
    strength = load_golden("tiny_flux_lora_merge.pt")["strength"]
    sd = loader.dequantize_state_dict(QS.wrap_quantized_state_dict(loader.load_torch_file(path)), DEV, BF)
    assert all(isinstance(v, torch.Tensor) for v in sd.values()) and sum(v.is_cuda for v in sd.values()) > 20
    pre = {k: v.to(BF) for k, v in ref_sd.items()}
    merged, report = nlora.merge_loras_into_flux_state_dict(sd, cfg, [(synth_flux_lora(cfg), strength)], device=DEV, dtype=BF)
    ref, ref_report = nlora.merge_loras_into_flux_state_dict(pre, cfg, [(synth_flux_lora(cfg), strength)], device=DEV, dtype=BF)
    assert report["patched"] == ref_report["patched"] > 0
    for k in ref:
        a, b = merged[k].to(DEV), ref[k].to(DEV)
        assert b.dtype == BF and torch.equal(a.to(BF), b), k
    eng = loader.forge_loader(path, loras=[(synth_flux_lora(cfg), strength)], device=DEV)
    assert eng.lora_report["patched"] == report["patched"]
