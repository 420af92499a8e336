"""CPU: the native GGUF reader (forge_amd/backend/gguf_file.py) against what the REAL reference's GGUFReader recorded for tests/golden/gguf/blocks.gguf
(tools/make_gguf_fixtures.py wrote both, the file with the reference's GGUFWriter), and its refusals of malformed input."""
import json
import os
import struct

import numpy as np
import pytest

import forge_amd  # noqa: F401
from conftest import GOLDEN
from forge_amd.backend import gguf_file
from forge_amd.backend.gguf_file import GGML_TYPES, GGUFFile, GGUFTensor

G = os.path.join(GOLDEN, "gguf")
BLOCKS = os.path.join(G, "blocks.gguf")


@pytest.fixture(scope="module")
def table():
    return json.load(open(os.path.join(G, "blocks_table.json")))


def test_tensor_table_matches_the_reference_reader(table):
    f = GGUFFile(BLOCKS)
    assert f.version == 3 and f.alignment == table["alignment"] and f.data_offset == table["data_offset"]
    assert list(f.tensors) == [t["name"] for t in table["tensors"]]            # file order
    assert len(f.tensors) == 28      # 10 x (rand, nan) + 5 gauss + 3 float
    for rec in table["tensors"]:
        t = f.tensors[rec["name"]]
        assert isinstance(t, GGUFTensor) and t.name == rec["name"]
        assert t.qtype == rec["type"] and t.type_name == rec["type_name"]
        assert list(t.shape) == rec["shape"], rec["name"]                       # the reversed ne: rows first
        assert t.data.dtype == np.uint8 and t.data.nbytes == rec["nbytes"]
        assert f.data_offset + f.offsets[rec["name"]] == rec["offset"]
        bw, bb = GGML_TYPES[t.qtype][1:]
        assert t.numel // bw * bb == rec["nbytes"] and t.shape[-1] % bw == 0
        assert not t.data.flags.owndata and not t.data.flags.writeable          # a view of the mapping, not a copy
    two_d = f.tensors["rand.Q8_0"]
    assert two_d.shape == (8, 1536 // 8 * 32) and two_d.dim() == 2 and two_d.size(0) == 8


def test_metadata_of_every_value_type(table):
    f = GGUFFile(BLOCKS)
    want = table["metadata"]
    assert set(f.metadata) == set(want)
    for k, v in want.items():
        got = f.metadata[k]
        if isinstance(v, float):
            assert got == pytest.approx(v, rel=0, abs=0) or np.float32(got) == np.float32(v), k
        else:
            assert got == v and type(got) is type(v), (k, got, v)
    assert f.architecture == "fixture"
    for key in ("u8", "i8", "u16", "i16", "u32", "i32", "f32", "u64", "i64", "f64", "bool", "str", "arr_i32", "arr_str", "arr_f32"):
        assert "fixture." + key in f.metadata
    assert f.metadata["fixture.u64"] == 2 ** 63 + 5 and f.metadata["fixture.i64"] == -2 ** 62 and f.metadata["fixture.bool"] is True
    assert f.metadata["fixture.arr_str"] == ["a", "bc", "def"]


def test_load_torch_file_returns_gguf_tensors():
    from forge_amd.backend import loader
    sd = loader.load_torch_file(BLOCKS)
    assert isinstance(sd["rand.Q4_K"], GGUFTensor) and sd["rand.Q4_K"].shape == (8, 224 // 8 * 256)


# ---- malformed input: ValueError, never an index outside the mapping -----------------------------------------------------------------------------------
def _header(n_tensors, infos=b"", version=3, magic=b"GGUF"):
    return magic + struct.pack("<IQQ", version, n_tensors, 0) + infos


def _info(name, ne, qtype, offset):
    b = name.encode()
    return struct.pack("<Q", len(b)) + b + struct.pack("<I", len(ne)) + b"".join(struct.pack("<Q", d) for d in ne) + struct.pack("<IQ", qtype, offset)


def _write(tmp_path, data, name="bad.gguf"):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def test_truncated_file(tmp_path):
    whole = open(BLOCKS, "rb").read()
    for cut in (3, 20, 100, 2000, len(whole) // 2, len(whole) - 1):
        with pytest.raises(ValueError):
            GGUFFile(_write(tmp_path, whole[:cut]))


def test_wrong_magic(tmp_path):
    whole = open(BLOCKS, "rb").read()
    with pytest.raises(ValueError, match="not a GGUF file"):
        GGUFFile(_write(tmp_path, b"GGML" + whole[4:]))


def test_unknown_version(tmp_path):
    whole = open(BLOCKS, "rb").read()
    with pytest.raises(ValueError, match="version 99"):
        GGUFFile(_write(tmp_path, whole[:4] + struct.pack("<I", 99) + whole[8:]))


def test_tensor_past_the_end_names_the_tensor(tmp_path):
    head = _header(1, _info("w.big", [32, 4], 8, 0))
    head += b"\0" * (-len(head) % 32)
    with pytest.raises(ValueError, match="w.big"):
        GGUFFile(_write(tmp_path, head + b"\0" * 100))            # needs 4 x 34 = 136 bytes
    GGUFFile(_write(tmp_path, head + b"\0" * 136, "ok.gguf"))     # exactly enough is accepted
    head = _header(1, _info("w.far", [32], 8, 1 << 40))
    with pytest.raises(ValueError, match="w.far"):
        GGUFFile(_write(tmp_path, head + b"\0" * 64))
    head = _header(1, _info("w.huge", [1 << 62, 1 << 62], 0, 0))  # an element count that overflows 64 bits
    with pytest.raises(ValueError, match="w.huge"):
        GGUFFile(_write(tmp_path, head + b"\0" * 64))


def test_row_length_not_a_multiple_of_the_block_size(tmp_path):
    head = _header(1, _info("w.ragged", [48, 2], 8, 0))
    with pytest.raises(ValueError, match="w.ragged.*48"):
        GGUFFile(_write(tmp_path, head + b"\0" * 4096))


def test_unknown_tensor_and_value_types(tmp_path):
    head = _header(1, _info("w.odd", [32], 77, 0))
    with pytest.raises(ValueError, match="w.odd"):
        GGUFFile(_write(tmp_path, head + b"\0" * 64))
    kv = struct.pack("<Q", 1) + b"k" + struct.pack("<I", 42)
    with pytest.raises(ValueError, match="value type 42"):
        GGUFFile(_write(tmp_path, b"GGUF" + struct.pack("<IQQ", 3, 0, 1) + kv + b"\0" * 64))


def test_type_table_is_consistent():
    assert set(gguf_file.DEQUANT_TYPES) <= set(GGML_TYPES)
    for num in gguf_file.DEQUANT_TYPES:
        name, bw, bb = GGML_TYPES[num]
        assert bw in (1, 32, 256) and bb % 2 == 0 and gguf_file.QTYPE[name] == num
