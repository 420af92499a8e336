"""CPU: the host side of float8 / bitsandbytes NF4 / FP4 checkpoint loading -- the numpy restatement of the kernels' contract (tests/quant_refs.py)
and its teeth, the writer (tools/bnb_write.py) and reader (backend/quant_state.py) of the packed format, shape-based detection on wrapped
tensors, and the per-component fp8 storage rule against what the reference recorded (tests/golden/quant_reference.json).
No tolerances anywhere: 16-bit and 32-bit patterns are compared as integers, NaNs by class."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import forge_amd  # noqa: F401
import quant_refs as Q
from conftest import GOLDEN, ROOT
from forge_amd import synth
from forge_amd.backend import loader, quant_state as QS

sys.path.insert(0, os.path.join(ROOT, "tools"))
import bnb_write as W  # noqa: E402

RECORD = json.load(open(os.path.join(GOLDEN, "quant_reference.json")))


# ---- fp8 ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("kind,fp8", [(Q.E4M3FN, torch.float8_e4m3fn), (Q.E5M2, torch.float8_e5m2)], ids=["e4m3fn", "e5m2"])
def test_fp8_table_is_torchs_conversion_for_all_256_codes(kind, fp8, dtype):
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    want = codes.view(fp8).to(dtype)
    table = Q.fp8_table(kind)
    got = torch.from_numpy(table).to(dtype)
    finite = ~torch.isnan(want)
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(got.view(torch.int16)[finite], want.view(torch.int16)[finite])
    assert torch.equal(torch.from_numpy(table)[finite], got.float()[finite])                 # the expansion is exact: nothing rounds
    assert int(torch.isnan(want).sum()) == (2 if kind == Q.E4M3FN else 6) and int(torch.isinf(want).sum()) == (0 if kind == Q.E4M3FN else 2)
    assert got.view(torch.int16)[0x80].item() == -32768                                      # -0 keeps its sign


def test_host_rounding_to_fp8_is_not_saturating():
    """the conversion the mirroring rule uses: 500 is beyond e4m3fn's 448 and becomes NaN, not 448"""
    p = QS.round_to_fp8(torch.tensor([500.0, 448.0, 0.3, -1e-9]), "fp8_e4m3fn")
    v = p.host_float()
    assert p.scheme == "fp8_e4m3fn" and p.data.dtype == torch.uint8 and torch.isnan(v[0]) and v[1] == 448.0 and v[2] == 0.3125 and v[3] == 0.0


# ---- bnb4: the restatement has teeth ---------------------------------------------------------------------------------------------------------------------
def _case(n=64 * 256 + 65 + 64 * 300, blocksize=64, blocksize2=256, seed=3):
    return Q.nested_case(n, blocksize, blocksize2, W.TABLES["nf4"], W.nested_table(1), seed)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def test_planted_errors_change_the_restatements_result():
    c = _case()
    ref = Q.bnb4_dequant(**c)
    n, bs, bs2 = c["n"], c["blocksize"], c["blocksize2"]
    i = np.arange(n)
    byte = c["packed"][i >> 1]
    scales = Q.bnb4_scales(n, bs, c["absmax"], c["code256"], c["absmax2"], c["offset"], bs2)
    # 1. nibble order swapped
    q_swapped = np.where(i & 1, byte >> 4, byte & 15)
    swapped = (c["code16"][q_swapped] * scales[i // bs]).astype(np.float32)
    assert (_bits(swapped) != _bits(ref)).mean() > 0.5
    # 2. the nested scale as one fused multiply-add (a single rounding): must differ somewhere, in the scale and in the 16-bit results
    b = np.arange(scales.size)
    fma = (c["code256"][c["absmax"]].astype(np.float64) * c["absmax2"][b // bs2].astype(np.float64) + np.float64(c["offset"])).astype(np.float32)
    assert (_bits(fma) != _bits(scales)).any()
    q = np.where(i & 1, byte & 15, byte >> 4)
    fused = (c["code16"][q] * fma[i // bs]).astype(np.float32)
    assert scales[0] == 0.0 and fma[0] != 0.0                          # block 0: the add cancels; fused, the product's rounding error is left
    for dt in (torch.float16, torch.bfloat16):
        assert not torch.equal(Q.rounded(fused, dt)[0] & 0x7fff, Q.rounded(ref, dt)[0] & 0x7fff), dt        # sign bit masked: magnitudes differ
    # 3. the nested block indexed by the element instead of by the block
    wrong_scales = (c["code256"][c["absmax"]] * c["absmax2"][np.minimum((b * bs) // bs2, c["absmax2"].size - 1)]).astype(np.float32) + c["offset"]
    wrong = (c["code16"][q] * wrong_scales[i // bs]).astype(np.float32)
    assert (_bits(wrong) != _bits(ref)).any()
    assert c["absmax2"].size >= 2 and n > bs * bs2                     # the inputs do cross a nested block


def test_element_to_nibble_and_odd_tail():
    code16 = np.arange(16, dtype=np.float32)
    out = Q.bnb4_dequant(np.array([0x12, 0x3F], dtype=np.uint8), 3, code16, 64, np.array([2.0], dtype=np.float32))
    assert out.tolist() == [2.0, 4.0, 6.0]                              # high nibble first; the low nibble of the last byte is unused


# ---- writer and reader -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nested", [False, True], ids=["flat", "nested"])
@pytest.mark.parametrize("quant_type", ["nf4", "fp4"])
def test_writer_and_reader_round_trip(quant_type, nested):
    w = torch.from_numpy(np.random.default_rng(5).standard_normal((96, 70)).astype(np.float32))      # 6720 = 105 blocks of 64
    sd = {"l.weight" + s: t for s, t in W.quantize(w, quant_type, 64, nested, 64).items()}
    sd["l.bias"] = torch.zeros(96)
    st = QS.parse_bnb_quant_state(sd, "l.weight")
    assert (st.quant_type, tuple(st.shape), st.blocksize, st.nested, st.dtype) == (quant_type, (96, 70), 64, nested, torch.bfloat16)
    assert st.code.tolist() == W.TABLES[quant_type].tolist() and st.absmax.numel() == 105
    assert (st.blocksize2, st.absmax2.numel(), st.code2.numel()) == (64, 2, 256) if nested else (st.absmax2 is None and st.code2 is None and st.offset == 0.0)
    wrapped = QS.wrap_quantized_state_dict(sd)
    assert set(wrapped) == {"l.weight", "l.bias"} and wrapped["l.bias"] is sd["l.bias"]
    p = wrapped["l.weight"]
    assert p.scheme == quant_type and tuple(p.shape) == (96, 70) and p.dim() == 2 and p.data.shape == (3360,) and sd["l.weight"].shape == (3360, 1)
    back = Q.state_dict_reference(sd)["l.weight"]
    err = (back - w).abs().max() / w.abs().max()
    assert back.shape == w.shape and err < (0.2 if quant_type == "nf4" else 0.35)        # a 4-bit quantiser, not a contract: the tables' widest gap
    if not nested:                                                                        # the largest weight of every block is reproduced exactly
        blocks = w.reshape(-1, 64)
        top = blocks.abs().argmax(dim=1)
        assert torch.equal(back.reshape(-1, 64).gather(1, top[:, None]).abs(), blocks.gather(1, top[:, None]).abs())


def test_malformed_dicts_are_refused_by_key_name():
    w = torch.from_numpy(np.random.default_rng(6).standard_normal((64, 64)).astype(np.float32))
    good = {"a.b.weight" + s: t for s, t in W.quantize(w, "nf4", 64, True, 64).items()}
    QS.wrap_quantized_state_dict(good)

    def marker(**change):
        meta = json.loads(bytes(good["a.b.weight.quant_state.bitsandbytes__nf4"].tolist()).decode())
        meta.update(change)
        return torch.tensor(list(json.dumps(meta).encode()), dtype=torch.uint8)

    for drop in (".quant_map", ".absmax", ".nested_absmax", ".nested_quant_map"):
        with pytest.raises(ValueError, match="a.b.weight" + drop.replace(".", r"\.")):
            QS.wrap_quantized_state_dict({k: v for k, v in good.items() if k != "a.b.weight" + drop})
    with pytest.raises(ValueError, match=r"a\.b\.weight"):
        QS.wrap_quantized_state_dict({**good, "a.b.weight.quant_state.bitsandbytes__nf4": marker(shape=[64, 65])})       # product != byte count
    with pytest.raises(ValueError, match=r"a\.b\.weight\.absmax"):
        QS.wrap_quantized_state_dict({**good, "a.b.weight.absmax": good["a.b.weight.absmax"][:-1]})
    with pytest.raises(ValueError, match=r"a\.b\.weight\.nested_absmax"):
        QS.wrap_quantized_state_dict({**good, "a.b.weight.nested_absmax": torch.zeros(3)})
    with pytest.raises(ValueError, match="quant_type"):
        QS.wrap_quantized_state_dict({**good, "a.b.weight.quant_state.bitsandbytes__nf4": marker(quant_type="int4")})
    with pytest.raises(ValueError, match="blocksize"):
        QS.wrap_quantized_state_dict({**good, "a.b.weight.quant_state.bitsandbytes__nf4": marker(blocksize=48)})
    with pytest.raises(ValueError, match=r"a\.b\.weight"):
        QS.wrap_quantized_state_dict({k: v for k, v in good.items() if k != "a.b.weight"})                              # the packed tensor itself
    with pytest.raises(ValueError, match="JSON"):
        QS.wrap_quantized_state_dict({**good, "a.b.weight.quant_state.bitsandbytes__nf4": torch.tensor([123, 34], dtype=torch.uint8)})


# ---- detection on wrapped tensors ------------------------------------------------------------------------------------------------------------------------
def _tiny_flux():
    return synth.TINY_FLUX_CONFIG, synth.synth_flux_state_dict(synth.TINY_FLUX_CONFIG, seed=2)


@pytest.mark.parametrize("form", ["nf4-nested", "fp4", "fp8_e4m3fn", "fp8_e5m2"])
def test_detection_reads_the_logical_shape_of_wrapped_tensors(form):
    cfg, sd = _tiny_flux()
    if form.startswith("fp8"):
        stored = {k: v.to(QS.FP8_DTYPES[form]) for k, v in sd.items()}
    else:
        stored = W.pack_state_dict({k: v.to(torch.bfloat16) for k, v in sd.items()}, form[:3], nested=form.endswith("nested"))
        assert stored["img_in.weight"].shape == (sd["img_in.weight"].numel() // 2, 1)         # the stored tensor: detection would go wrong on it
    wrapped = QS.wrap_quantized_state_dict(stored)
    assert set(wrapped) == set(sd)                                                            # the side keys never appear as model keys
    assert loader.detect_flux_config(wrapped, "") == loader.detect_flux_config(sd, "") == cfg
    parts, guess = loader.split_flux_state_dict(wrapped)
    assert guess["flux_config"] == cfg and guess["dtype"] == torch.bfloat16 and set(parts["transformer"]) == set(sd)
    assert all(tuple(wrapped[k].shape) == tuple(sd[k].shape) for k in sd)
    assert QS.component_storage(wrapped) == (form if form.startswith("fp8") else form[:3])


def test_raw_fp8_tensors_are_still_refused_by_split_flux_state_dict():
    _, sd = _tiny_flux()
    for fp8 in (torch.float8_e4m3fn, torch.float8_e5m2):
        with pytest.raises(NotImplementedError, match="wrap"):
            loader.split_flux_state_dict({k: v.to(fp8) for k, v in sd.items()})


def test_bnb_storage_is_refused_by_name_where_it_is_not_served():
    sd = synth.synth_unet_state_dict(synth.TINY_SDXL_UNET_CONFIG)
    key = next(k for k, v in sd.items() if v.dim() == 2)
    packed = W.pack_state_dict(sd, "nf4", select=lambda k, v: k == key)
    with pytest.raises(NotImplementedError, match=key.replace(".", r"\.")):
        loader.split_state_dict(packed)


def test_unet_in_fp8_passes_through_split_state_dict_wrapped():
    cfg = synth.TINY_SDXL_UNET_CONFIG
    sd = synth.synth_unet_state_dict(cfg)
    stored = {k: (v.half() if i % 9 == 0 else v.to(torch.float8_e4m3fn)) for i, (k, v) in enumerate(sd.items())}
    parts, guess = loader.split_state_dict(stored)
    plain, plain_guess = loader.split_state_dict({k: v.half() for k, v in sd.items()})
    assert guess["unet_config"] == plain_guess["unet_config"] and set(parts["unet"]) == set(plain["unet"])
    assert all(QS.is_packed(v) and v.scheme == "fp8_e4m3fn" and tuple(v.shape) == tuple(sd[k].shape) for k, v in parts["unet"].items())
    k0 = next(iter(sd))                                                   # stored wider (fp16) in an fp8 majority: rounded to fp8
    assert torch.equal(parts["unet"][k0].host_float(), sd[k0].half().to(torch.float8_e4m3fn).float())


# ---- the mirroring rule against the reference's record --------------------------------------------------------------------------------------------------
def _dt(name):
    return getattr(torch, name)


def test_component_storage_is_the_references_state_dict_dtype():
    assert len(RECORD["state_dict_dtype"]) >= 8
    for case in RECORD["state_dict_dtype"]:
        sd = {k: torch.zeros(2, dtype=_dt(dt)) for k, dt in case["tensors"]}
        for k in [k for k in sd if QS.BNB_MARKER in k]:                  # make the marked tensor a well-formed packed one
            wk = k[:k.index(QS.BNB_MARKER)]
            sd.update({wk + s: t for s, t in W.quantize(torch.ones(64), k.rsplit("__", 1)[1]).items()})
        got = QS.component_storage(QS.wrap_quantized_state_dict(sd))
        want = case["result"]
        assert (got if isinstance(got, str) else str(got).replace("torch.", "")).replace("fp8_", "float8_") == want, case


@pytest.mark.parametrize("component", ["flux", "unet", "t5"])
@pytest.mark.parametrize("kind", ["float8_e4m3fn", "float8_e5m2"])
def test_fp8_storage_rule_matches_what_the_reference_recorded(component, kind):
    params = RECORD["fp8_storage"][component][kind]
    assert len(params) > 25
    scheme = kind.replace("float8_", "fp8_")
    sd = {k: torch.full((4,), 0.3, dtype=_dt(r["stored"])) for k, r in params.items() if r["stored"] is not None}
    assert {r["stored"] for r in params.values()} >= {kind, "float16", "bfloat16", "float32"}
    out = QS.mirror_fp8_storage(QS.wrap_quantized_state_dict(sd), component)
    assert set(out) == set(sd)
    kept = 0
    for k, v in out.items():
        want = params[k]["result"]
        if want == kind:
            assert QS.is_packed(v) and v.scheme == scheme, (k, want)
            assert torch.equal(v.host_float(), sd[k].float().to(_dt(kind)).float()), k          # stored wider: rounded to fp8; stored fp8: as is
        else:
            kept += 1
            assert isinstance(v, torch.Tensor) and str(v.dtype) == "torch." + want and torch.equal(v, sd[k].to(v.dtype)), (k, want)
        assert ("fp8" if want == kind else _dt(want)) == QS.fp8_storage_dtype(component, k)
    assert kept == (0 if component != "t5" else sum(1 for r in params.values() if r["stored"] is not None and r["result"] != kind)) and (component != "t5" or kept >= 9)


def test_other_storage_types_leave_a_component_alone():
    _, sd = _tiny_flux()
    mostly16 = {k: (v.to(torch.float8_e4m3fn) if i == 3 else v.to(torch.bfloat16)) for i, (k, v) in enumerate(sd.items())}
    wrapped = QS.wrap_quantized_state_dict(mostly16)
    out = QS.mirror_fp8_storage(wrapped, "flux")
    assert QS.component_storage(wrapped) == torch.bfloat16 and all(out[k] is wrapped[k] for k in wrapped)
    assert sum(QS.is_packed(v) for v in out.values()) == 1


# ---- VAEs stay as stored ---------------------------------------------------------------------------------------------------------------------------------
def test_fp8_vae_tensors_are_cast_on_the_host_and_bnb_ones_refused_by_key():
    """a diffusers-keyed float8 VAE under 'vae.' of a Flux checkpoint (its 2-D mid-block attention weights are reshaped by the key conversion) and an
    LDM-keyed one in an SD checkpoint: plain fp32 tensors holding the stored values come out, no wrapper reaches the VAE; bnb-packed VAE tensors are
    refused by their key"""
    from test_loader_lora import _vae_ldm_to_diffusers_names
    _, tr = _tiny_flux()
    vcfg = synth.TINY_FLUX_VAE_CONFIG
    vae = synth.synth_vae_state_dict(vcfg, seed=1)
    fp8 = torch.float8_e4m3fn
    dif = _vae_ldm_to_diffusers_names(vae, len(vcfg["block_out_channels"]))
    ck = {"model.diffusion_model." + k: v.to(fp8) for k, v in tr.items()}
    ck.update({"vae." + k: v.to(fp8) for k, v in dif.items()})
    parts, guess = loader.split_flux_state_dict(QS.wrap_quantized_state_dict(ck))
    assert set(parts["vae"]) == set(vae) and guess["vae_config"]["latent_channels"] == 16
    for k, v in parts["vae"].items():
        assert isinstance(v, torch.Tensor) and v.dtype == torch.float32 and v.shape == vae[k].shape, k
        assert torch.equal(v, vae[k].to(fp8).float().reshape(v.shape)), k
    key = next(k for k, v in dif.items() if v.dim() == 2)
    packed = dict(ck)
    packed.update({"vae." + key + s: t for s, t in W.quantize(dif[key], "nf4").items()})
    with pytest.raises(NotImplementedError, match=("vae." + key).replace(".", r"\.")):
        loader.split_flux_state_dict(QS.wrap_quantized_state_dict(packed))
    ucfg = synth.TINY_SD15_UNET_CONFIG
    sdck = {loader.UNET_PREFIX + k: v.to(fp8) for k, v in synth.synth_unet_state_dict(ucfg, seed=0).items()}
    svae = synth.synth_vae_state_dict(synth.TINY_VAE_CONFIG, seed=1)
    sdck.update({loader.VAE_PREFIX + k: v.to(fp8) for k, v in svae.items()})
    sparts, _ = loader.split_state_dict(sdck)
    assert all(isinstance(v, torch.Tensor) and v.dtype == torch.float32 for v in sparts["vae"].values()) and set(sparts["vae"]) == set(svae)
    k2 = next(k for k, v in svae.items() if v.dim() == 4)
    bad = dict(sdck)
    bad.update({loader.VAE_PREFIX + k2 + s: t for s, t in W.quantize(svae[k2], "fp4").items()})
    with pytest.raises(NotImplementedError, match=(loader.VAE_PREFIX + k2).replace(".", r"\.")):
        loader.split_state_dict(bad)
