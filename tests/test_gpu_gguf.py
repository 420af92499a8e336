"""GPU: GGUF dequantisation kernels (fmx_gguf_dequant_f16 / _bf16 through ops.gguf_dequant) and the loader route built on them.

Every comparison here is EXACT: the kernels' contract is the fp32 value ggml defines rounded once to the output type, so their 16-bit patterns
equal the 16-bit rounding (torch's, round to nearest even) of tests/gguf_refs.py -- the host reference that tests/test_gguf_refs.py pins bit
for bit to the reference's own dequantiser.  NaNs are compared by position (their payload is not part of the contract)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import forge_amd  # noqa: E402
import gguf_build as B  # noqa: E402
import gguf_refs as R  # noqa: E402
from conftest import GOLDEN, load_golden  # noqa: E402
from forge_amd import _lib, hipops as ops, synth  # noqa: E402
from forge_amd.backend import loader  # noqa: E402
from forge_amd.backend.gguf_file import GGUFFile  # noqa: E402

DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]
FIXTURE = os.path.join(GOLDEN, "gguf", "blocks.gguf")


def rounded(ref32, dtype):
    """the contract's right-hand side: fp32 -> dtype, once, to nearest even, as int16 bit patterns (+ the NaN mask)"""
    t = torch.from_numpy(np.ascontiguousarray(ref32)).to(dtype)
    return t.view(torch.int16), torch.isnan(t)


def assert_same_bits(got, ref32, what):
    """got: device tensor of a 16-bit type; ref32: numpy fp32 of the same element count"""
    want, want_nan = rounded(ref32, got.dtype)
    g = got.detach().reshape(-1).cpu()
    got_nan = torch.isnan(g)
    assert g.numel() == want.numel(), what
    assert torch.equal(got_nan, want_nan), (what, "NaN positions differ", int((got_nan != want_nan).sum()))
    bad = (g.view(torch.int16) != want) & ~want_nan
    nbad = int(bad.sum())
    if nbad:
        i = int(torch.nonzero(bad)[0])
        raise AssertionError(f"{what}: {nbad} of {g.numel()} elements differ; first at {i}: got {float(g[i])!r} want {float(ref32.reshape(-1)[i])!r}")


def dequant(raw_np, qtype, n, dtype, offset=0):
    """upload the packed bytes (optionally `offset` bytes into a larger allocation) and run the kernel"""
    buf = torch.empty(raw_np.size + offset, dtype=torch.uint8, device=DEV)
    buf[offset:].copy_(torch.from_numpy(np.ascontiguousarray(raw_np).reshape(-1).copy()))
    out = ops.gguf_dequant(buf[offset:], qtype, (n,), dtype)
    torch.cuda.synchronize()
    return out


def random_blocks(qtype, n_blocks, seed):
    return np.random.default_rng([seed, qtype]).integers(0, 256, (n_blocks, R.BLOCK[qtype][1]), dtype=np.uint8)


@pytest.fixture(scope="module")
def fixture():
    return GGUFFile(FIXTURE)


# ---- the kernels -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("qtype", sorted(R.BLOCK), ids=lambda q: R.NAMES[q])
def test_fixture_tensors_bit_for_bit(fixture, qtype, dtype):
    names = [n for n, t in fixture.tensors.items() if t.qtype == qtype]
    assert names and (qtype not in R.QUANTISED or {n.split(".")[0] for n in names} >= {"rand", "nan"})
    for name in names:
        t = fixture.tensors[name]
        out = ops.gguf_dequant(torch.from_numpy(np.array(t.data)).to(DEV), t.qtype, t.shape, dtype)
        assert out.shape == t.shape and out.dtype == dtype
        with np.errstate(all="ignore"):
            assert_same_bits(out, R.dequant(t.data, qtype), f"{name} -> {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("qtype", R.QUANTISED, ids=lambda q: R.NAMES[q])
def test_sizes_the_fixture_does_not_have(qtype, dtype):
    """1 block; a prime number of blocks; counts around the 8192 weights one workgroup takes per step (not a multiple, one block more, one block
    less, several steps of a grid-stride loop is covered by the full-size test); and a block pointer one block into its allocation (2-byte but
    not 16-byte aligned for every block size: none is a multiple of 16)"""
    bw, bb = R.BLOCK[qtype]
    per_chunk = 8192 // bw
    for n_blocks, offset in ((1, 0), (7, 0), (257, 0), (per_chunk - 1, 0), (per_chunk + 1, 0), (3 * per_chunk + 5, 0), (1, bb), (per_chunk + 3, bb),
                             (2 * per_chunk, 3 * bb), (61, 2)):
        raw = random_blocks(qtype, n_blocks, 1000 + n_blocks + offset)
        out = dequant(raw, qtype, n_blocks * bw, dtype, offset)
        with np.errstate(all="ignore"):
            assert_same_bits(out, R.dequant(raw, qtype), f"{R.NAMES[qtype]} x {n_blocks} blocks at byte offset {offset} -> {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("qtype", [R.F32, R.F16, R.BF16], ids=lambda q: R.NAMES[q])
def test_float_types_odd_counts_and_alignment(qtype, dtype):
    rng = np.random.default_rng(qtype)
    for n, offset in ((1, 0), (7, 0), (8, 0), (1001, 0), (4099, 2), (64, 6)):
        vals = (rng.standard_normal(n) * np.exp(rng.uniform(-20, 20, n))).astype(np.float32)
        vals[::5] *= 1e-42 / np.maximum(np.abs(vals[::5]), 1e-30)        # fp32 subnormals among them
        if qtype == R.F32:
            raw = vals.view(np.uint8)
        elif qtype == R.F16:
            with np.errstate(over="ignore"):
                raw = vals.astype(np.float16).view(np.uint8)
        else:
            raw = torch.from_numpy(vals).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint8)
        out = dequant(raw, qtype, n, dtype, offset)
        assert_same_bits(out, R.dequant(raw, qtype), f"{R.NAMES[qtype]} x {n} at byte offset {offset} -> {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("qtype", [R.Q8_0, R.Q4_K], ids=lambda q: R.NAMES[q])
def test_full_size_tensor(qtype, dtype):
    """3072 x 21504 (Flux's widest matrix) from seeded random bytes.  Checked against the host reference on every 64th block plus the first and last
    4096 blocks: that sample bounds the host's run time, it is not a tolerance -- every sampled element must match."""
    rows, cols = 3072, 21504
    bw, bb = R.BLOCK[qtype]
    n_blocks = rows * cols // bw
    raw = random_blocks(qtype, n_blocks, 7)
    out = ops.gguf_dequant(torch.from_numpy(raw.reshape(-1)).to(DEV), qtype, (rows, cols), dtype)
    torch.cuda.synchronize()
    pick = np.unique(np.concatenate([np.arange(0, n_blocks, 64), np.arange(min(4096, n_blocks)), np.arange(max(0, n_blocks - 4096), n_blocks)]))
    got = out.reshape(n_blocks, bw)[torch.from_numpy(pick).to(DEV)]
    with np.errstate(all="ignore"):
        assert_same_bits(got, R.dequant(raw[pick], qtype), f"{R.NAMES[qtype]} 3072 x 21504 -> {dtype}, {pick.size} of {n_blocks} blocks")


def test_overflow_rounds_as_torch_does():
    """a Q8_0 block with scale 65504 and quant 127: 8.3e6 is inf in fp16 and finite in bf16"""
    blk = np.zeros((1, 34), dtype=np.uint8)
    blk[0, :2] = np.array([65504], dtype=np.float16).view(np.uint8)
    blk[0, 2], blk[0, 3], blk[0, 4] = 127, np.uint8(-127 & 0xFF), 1
    h = dequant(blk, R.Q8_0, 32, torch.float16).cpu()
    b = dequant(blk, R.Q8_0, 32, torch.bfloat16).cpu()
    assert torch.isinf(h[0]) and h[0] > 0 and torch.isinf(h[1]) and h[1] < 0 and float(h[2]) == 65504.0 and float(h[5]) == 0.0
    assert torch.isfinite(b).all() and float(b[0]) == float(torch.tensor(65504.0 * 127).to(torch.bfloat16))
    for out, dt in ((h, torch.float16), (b, torch.bfloat16)):
        assert_same_bits(out, R.dequant(blk, R.Q8_0), f"overflow -> {dt}")


def test_wrapper_refuses_what_the_kernels_do_not_expand():
    raw = torch.zeros(66, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.FmxError, match="10002"):
        ops.gguf_dequant(raw, 16, (256,), torch.bfloat16)          # IQ2_XXS
    with pytest.raises(ValueError):
        ops.gguf_dequant(raw, R.Q8_0, (64,), torch.bfloat16)       # 66 bytes are not two Q8_0 blocks
    with pytest.raises(TypeError):
        ops.gguf_dequant(raw[:34], R.Q8_0, (32,), torch.float32)
    with pytest.raises(TypeError):
        ops.gguf_dequant(raw[:34].cpu(), R.Q8_0, (32,), torch.float16)


# ---- the loader route ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_flux_gguf(tmp_path_factory):
    cfg = synth.TINY_FLUX_CONFIG
    tensors = B.quantize_state_dict(synth.synth_flux_state_dict(cfg, seed=2), seed=11)
    assert {q for _, q, _, _ in tensors} >= set(R.QUANTISED)       # every block type occurs in the file
    path = B.write(tmp_path_factory.mktemp("gguf") / "tiny_flux_q.gguf", tensors, "flux")
    return cfg, path, B.reference_state_dict(tensors)


@pytest.fixture(scope="module")
def tiny_t5_gguf(tmp_path_factory):
    cfg = synth.TINY_T5_CONFIG
    sd = {k: v for k, v in synth.synth_t5_state_dict(cfg).items() if k != "logit_scale"}
    tensors = B.quantize_state_dict(sd, seed=12, rename=B.t5_llama_name)
    assert any(n == "enc.blk.0.attn_k.weight" for n, _, _, _ in tensors) and any(n == "token_embd.weight" for n, _, _, _ in tensors)
    path = B.write(tmp_path_factory.mktemp("gguf") / "tiny_t5_q.gguf", tensors, "t5encoder")
    ref = {"transformer." + loader.t5_llama_key(k): v for k, v in B.reference_state_dict(tensors).items()}
    return cfg, path, ref


def _tensors(w):
    for k, v in w.items():
        for i, t in enumerate(v if isinstance(v, (tuple, list)) else (v,)):
            if isinstance(t, torch.Tensor):
                yield f"{k}[{i}]", t


def _flux_inputs():
    g = load_golden("tiny_flux_fwd.pt")
    return [g[k].to(DEV) for k in ("x", "t", "ctx", "y", "guidance")]


def test_flux_engine_from_gguf_equals_the_pre_dequantised_one(tiny_flux_gguf):
    """nothing downstream knows the file was quantised: every resident weight of the engine built from the .gguf equals, bit for bit, the one built
    from the dequantised state dict (fp32, rounded to the compute type by the executor), and one forward of both is bit-identical"""
    from forge_amd.backend.diffusion_engine.base import build_flux_engine
    cfg, path, ref_sd = tiny_flux_gguf
    eng = loader.forge_loader(path, device=DEV)
    assert eng.model_guess["flux_config"] == loader.detect_flux_config(ref_sd, "") and eng.model_guess["dtype"] == torch.bfloat16
    net = eng.forge_objects.unet.model.diffusion_model
    ref_net = build_flux_engine(cfg, ref_sd, device=DEV, dtype=torch.bfloat16).forge_objects.unet.model.diffusion_model
    assert net.dtype == torch.bfloat16
    got, want = dict(_tensors(net.w)), dict(_tensors(ref_net.w))
    assert set(got) == set(want) and len(got) > 40
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k].view(torch.int16), want[k].view(torch.int16)), k
    args = _flux_inputs()
    out, ref_out = net.forward(*args), ref_net.forward(*args)
    assert torch.isfinite(out.float()).all() and torch.equal(out, ref_out)
    # the caller's compute type wins over the default
    eng16 = loader.forge_loader(path, device=DEV, dtype=torch.float16)
    net16 = eng16.forge_objects.unet.model.diffusion_model
    ref16 = build_flux_engine(cfg, ref_sd, device=DEV, dtype=torch.float16).forge_objects.unet.model.diffusion_model
    for (k, a), (_, b) in zip(_tensors(net16.w), _tensors(ref16.w)):
        assert a.dtype == torch.float16 and torch.equal(a.view(torch.int16), b.view(torch.int16)), k


def test_t5_through_additional_state_dicts(tiny_flux_gguf, tiny_t5_gguf):
    from forge_amd.backend.nn.t5 import IntegratedT5
    _, flux_path, _ = tiny_flux_gguf
    cfg, t5_path, ref_sd = tiny_t5_gguf
    eng = loader.forge_loader(flux_path, device=DEV, additional_state_dicts=[t5_path])
    sd = eng.text_encoder_state_dicts["t5xxl"]
    assert set(sd) == set(ref_sd)
    ids = load_golden("tiny_t5.pt")["ids"]
    for dt in (torch.bfloat16,):      # the type the file was expanded to (the engine's compute type)
        enc = IntegratedT5(cfg, sd, device=DEV, dtype=dt)
        ref = IntegratedT5(cfg, ref_sd, device=DEV, dtype=dt)
        for k in ref.w:
            if isinstance(ref.w[k], torch.Tensor):
                assert torch.equal(enc.w[k], ref.w[k]), k
        z, z_ref = enc.transformer(ids.to(DEV)), ref.transformer(ids.to(DEV))
        z, z_ref = (z if isinstance(z, torch.Tensor) else z[0]), (z_ref if isinstance(z_ref, torch.Tensor) else z_ref[0])
        assert torch.isfinite(z.float()).all() and torch.equal(z, z_ref)


def test_lora_merges_onto_gguf_weights_as_onto_dequantised_ones(tiny_flux_gguf):
    from forge_amd.backend.patcher import lora as nlora
    from oracle.make_golden import synth_flux_lora
    cfg, path, ref_sd = tiny_flux_gguf
    strength = load_golden("tiny_flux_lora_merge.pt")["strength"]
    sd = loader.dequantize_state_dict(loader.load_torch_file(path), DEV, torch.bfloat16)
    pre = {k: v.to(torch.bfloat16) for k, v in ref_sd.items()}
    merged, report = nlora.merge_loras_into_flux_state_dict(sd, cfg, [(synth_flux_lora(cfg), strength)], device=DEV, dtype=torch.bfloat16)
    ref, ref_report = nlora.merge_loras_into_flux_state_dict(pre, cfg, [(synth_flux_lora(cfg), strength)], device=DEV, dtype=torch.bfloat16)
    assert report["patched"] == ref_report["patched"] > 0
    changed = 0
    for k in ref:
        a, b = merged[k].to(DEV), ref[k].to(DEV)      # (F32 vectors of the file that no LoRA touches are still fp32 on the GGUF side)
        assert b.dtype == torch.bfloat16 and torch.equal(a.to(torch.bfloat16), b), k
        changed += int(not torch.equal(b.cpu(), pre[k].reshape(b.shape)))
    assert changed == report["patched"]
    # through forge_loader too
    eng = loader.forge_loader(path, loras=[(synth_flux_lora(cfg), strength)], device=DEV)
    assert eng.lora_report["patched"] == report["patched"]


def test_dequantize_state_dict_leaves_no_packed_buffer_alive(tiny_flux_gguf):
    """device memory after - before = the 16-bit tensors' bytes, each rounded up to the caching allocator's 512-byte granule (what
    torch.cuda.memory_allocated counts; observed on the tiny Flux file: 14450688 bytes = the payload exactly, every tensor being a multiple of 512 bytes; the packed staging copies are all released)"""
    _, path, _ = tiny_flux_gguf
    sd = loader.load_torch_file(path)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    out = loader.dequantize_state_dict(sd, DEV, torch.bfloat16)
    torch.cuda.synchronize()
    after = torch.cuda.memory_allocated()
    dev = [v for v in out.values() if isinstance(v, torch.Tensor) and v.is_cuda]
    assert len(dev) == sum(1 for v in sd.values() if v.qtype in R.QUANTISED) > 20
    exact = sum(t.numel() * 2 for t in dev)
    granules = sum((t.numel() * 2 + 511) // 512 * 512 for t in dev)
    print(f"device bytes: after - before = {after - before}, 16-bit payload {exact}, in 512-byte granules {granules}")
    assert exact <= after - before <= granules
    assert all(isinstance(v, torch.Tensor) for v in out.values())
