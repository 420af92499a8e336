"""CPU: the host reference of the GGUF tests (tests/gguf_refs.py, written from the block layouts) is pinned BIT FOR BIT in fp32 to what the REAL
reference's numpy `dequantize` recorded for every tensor of tests/golden/gguf/blocks.gguf (all thirteen types, 100 % of the elements; NaNs, which
only the nan.* tensors hold, by position); one planted bug per family must make that comparison fail; the loader's T5 key map against the
reference's; the C entry points' refusals that need no device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import forge_amd  # noqa: F401
import gguf_refs as R
from conftest import GOLDEN
from forge_amd import _lib
from forge_amd.backend import loader
from forge_amd.backend.gguf_file import GGML_TYPES, GGUFFile

G = os.path.join(GOLDEN, "gguf")
FAKE = 0x7F0000001000


@pytest.fixture(scope="module")
def fixture():
    f = GGUFFile(os.path.join(G, "blocks.gguf"))
    expected = {}
    for fam in ("q32", "k_a", "k_b", "k_c"):
        with np.load(os.path.join(G, f"blocks_expected_{fam}.npz")) as z:
            expected.update({k: z[k] for k in z.files})
    assert set(expected) == set(f.tensors)
    return f, expected


def test_type_tables_agree():
    for qt, (bw, bb) in R.BLOCK.items():
        assert GGML_TYPES[qt][1:] == (bw, bb) and GGML_TYPES[qt][0] == R.NAMES[qt]


def test_host_reference_equals_the_real_dequantiser_bit_for_bit(fixture):
    f, expected = fixture
    seen = set()
    for name, t in f.tensors.items():
        got = R.dequant(t.data, t.qtype)
        want = expected[name]
        assert got.dtype == np.float32 and got.shape == want.shape == (t.numel,), name
        ok, nbad = R.same_bits(got, want)
        assert ok, (name, nbad)
        if not name.startswith("nan."):
            assert np.isfinite(want).all(), name      # nothing is left out of the comparison: every expected value is a number
        seen.add(t.qtype)
    assert seen == set(R.BLOCK) and len(seen) == 13
    assert sum(bool(np.isnan(expected["nan." + R.NAMES[q]]).any()) for q in R.QUANTISED) >= 8   # the nan.* tensors do hold NaNs


@pytest.mark.parametrize("bug,qtype", [(b, q) for b, qs in R.BUGS.items() for q in qs])
def test_teeth_a_planted_bug_fails_on_most_blocks(fixture, bug, qtype):
    f, expected = fixture
    name = "rand." + R.NAMES[qtype]
    bw = R.BLOCK[qtype][0]
    got = R.dequant(f.tensors[name].data, qtype, bug=bug).reshape(-1, bw)
    want = expected[name].reshape(-1, bw)
    wrong_blocks = (got.view(np.uint32) != want.view(np.uint32)).any(axis=1).mean()
    assert wrong_blocks > 0.5, (bug, name, wrong_blocks)


def test_t5_key_map_equals_the_reference():
    want = json.load(open(os.path.join(G, "t5_key_map.json")))
    assert len(want) == 30
    for k, v in want.items():
        assert loader.t5_llama_key(k) == v, k
    assert loader.t5_llama_key("enc.blk.7.attn_q.weight") == "encoder.block.7.layer.0.SelfAttention.q.weight"
    assert loader.t5_llama_key("token_embd.weight") == "shared.weight"


def test_replace_state_dict_places_components():
    import torch
    sd = {"double_blocks.0.img_attn.norm.key_norm.scale": torch.zeros(128), "vae.decoder.conv_in.weight": torch.zeros(1)}
    loader.replace_state_dict(sd, {"decoder.conv_in.weight": torch.ones(2), "decoder.conv_out.weight": torch.ones(3)})
    assert sd["vae.decoder.conv_in.weight"].shape == (2,) and "vae.decoder.conv_out.weight" in sd
    loader.replace_state_dict(sd, {"enc.blk.0.attn_k.weight": torch.ones(1), "token_embd.weight": torch.ones(4)})
    assert sd[loader.T5_PREFIX + "encoder.block.0.layer.0.SelfAttention.k.weight"].shape == (1,) and sd[loader.T5_PREFIX + "shared.weight"].shape == (4,)
    loader.replace_state_dict(sd, {"encoder.block.0.layer.0.SelfAttention.k.weight": torch.ones(5)})
    assert sd[loader.T5_PREFIX + "encoder.block.0.layer.0.SelfAttention.k.weight"].shape == (5,) and loader.T5_PREFIX + "shared.weight" not in sd
    loader.replace_state_dict(sd, {"text_model.encoder.layers.0.layer_norm1.weight": torch.ones(768)})
    assert loader.CLIP_L_PREFIX + "text_model.encoder.layers.0.layer_norm1.weight" in sd
    with pytest.raises(NotImplementedError):
        loader.replace_state_dict(sd, {"something.else": torch.ones(1)})
    ldm = {"model.diffusion_model.input_blocks.0.0.weight": torch.zeros(1), "first_stage_model.decoder.conv_in.weight": torch.zeros(1)}
    loader.replace_state_dict(ldm, {"decoder.conv_in.weight": torch.ones(2)})
    assert ldm["first_stage_model.decoder.conv_in.weight"].shape == (2,)


def test_forge_loader_keeps_its_defaults():
    import inspect
    sig = inspect.signature(loader.forge_loader)
    assert sig.parameters["additional_state_dicts"].default is None and list(sig.parameters)[:4] == ["sd", "loras", "device", "prediction_type"]


# ---- C entry points: refusals decided on the host ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


@pytest.mark.parametrize("fn", ["fmx_gguf_dequant_f16", "fmx_gguf_dequant_bf16"])
def test_entry_point_contract(lib, fn):
    f = getattr(lib, fn)
    p = C.c_void_p(FAKE)
    err = lambda: lib.fmx_last_error().decode()  # noqa: E731
    for qt in (4, 5, 9, 15, 16, 20, 23, 29, 31, 34, 35, -1, 1000):          # removed Q4_2 / Q4_3, Q8_1, Q8_K, the IQ families, TQ, nonsense
        assert f(qt, p, p, 256, None) == 10002 and str(qt) in err(), qt
    for qt, n in ((8, 48), (2, 31), (12, 128), (14, 32 * 7), (10, 257)):     # not a whole number of blocks
        assert f(qt, p, p, n, None) == 10001 and "multiple" in err(), (qt, n)
    assert f(8, None, p, 32, None) == 10001 and f(8, p, None, 32, None) == 10001
    assert f(8, p, p, 0, None) == 10001 and f(8, p, p, -32, None) == 10001
    assert f(8, C.c_void_p(FAKE + 1), p, 32, None) == 10001 and "2-byte" in err()
    assert f(8, p, C.c_void_p(FAKE + 2), 32, None) == 10001 and "16-byte" in err()
    assert lib.fmx_abi_version() == 12
