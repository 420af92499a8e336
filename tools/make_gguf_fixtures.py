"""TEST INFRASTRUCTURE ONLY.  Generates tests/golden/gguf/* with the REAL reference's vendored `gguf` package (imported at run time from
<reference>/packages_3rdparty; nothing of it is copied).  Deterministic (seeded).

    python tools/make_gguf_fixtures.py --reference /path/to/reference [--out tests/golden/gguf]

Writes
  blocks.gguf              by the reference's GGUFWriter.  Per quantised type (Q4_0 Q4_1 Q5_0 Q5_1 Q8_0 Q2_K Q3_K Q4_K Q5_K Q6_K):
                             rand.<T>   blocks of RANDOM BYTES (every nibble / high-bit / 6-bit-scale path is hit, not only what a quantiser
                                        emits); fp16 scale fields whose exponent bits are all ones (inf / NaN: 3-6 % of random blocks) are
                                        rewritten, so every expected value is finite
                             nan.<T>    64 random blocks that KEEP such scales (NaN positions and all other values are compared)
                             gauss.<T>  (the five types the reference can quantise) its `quantize` of Gaussian data; its K-family quantisers
                                        raise NotImplementedError, which is checked here
                           plus F32, F16 and BF16 tensors and key-value metadata of every value type.
  blocks_expected_<family>.npz  the reference's numpy `dequantize` of every tensor, fp32 (split by family: no committed file above 1 MiB)
  blocks_table.json        the tensor table (name, type, shape = reversed ne, data offset, byte length) and the metadata as the reference's
                           GGUFReader sees them
  t5_key_map.json          llama.cpp T5 tensor names -> HF names, by the key map read out of the reference's backend/loader.py (replace_state_dict)
"""
import argparse
import ast
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUANTISED = "Q4_0 Q4_1 Q5_0 Q5_1 Q8_0 Q2_K Q3_K Q4_K Q5_K Q6_K".split()
CAN_QUANTIZE = "Q4_0 Q4_1 Q5_0 Q5_1 Q8_0".split()
# byte offsets of the fp16 fields of each block layout (facts of the format)
F16_FIELDS = {"Q4_0": (0,), "Q4_1": (0, 2), "Q5_0": (0,), "Q5_1": (0, 2), "Q8_0": (0,), "Q2_K": (80, 82), "Q3_K": (108,), "Q4_K": (0, 2),
              "Q5_K": (0, 2), "Q6_K": (208,)}
N_BLOCKS = {32: 1536, 256: 224}


def finite_scales(blk, name, rng):
    """rewrite fp16 fields whose exponent is all ones (inf / NaN) with a finite random exponent"""
    for o in F16_FIELDS[name]:
        hi = blk[:, o + 1]
        bad = (hi & 0x7C) == 0x7C
        hi[bad] = (hi[bad] & 0x83) | (rng.integers(0, 31, int(bad.sum()), dtype=np.uint8) << 2)
    return blk


def t5_key_map(reference):
    src = open(os.path.join(reference, "backend", "loader.py")).read()
    table = None
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Assign) and isinstance(node.value, ast.Dict) and any("t5_format" in getattr(t, "id", "") for t in node.targets):
            table = ast.literal_eval(node.value)
    assert table, "the T5 key map was not found in the reference's backend/loader.py"
    names = ["token_embd.weight", "enc.output_norm.weight", "enc.blk.0.attn_rel_b.weight"]
    for i in (0, 1, 23):
        names += [f"enc.blk.{i}.{p}.weight" for p in ("attn_q", "attn_k", "attn_v", "attn_o", "attn_norm", "ffn_up", "ffn_down", "ffn_gate", "ffn_norm")]
    out = {}
    for k in names:
        m = k
        for s, d in table.items():       # the reference applies every replacement, in the table's order, to every key
            m = m.replace(s, d)
        out[k] = m
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="checkout of the reference project (its packages_3rdparty/gguf is imported)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "gguf"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(a.reference, "packages_3rdparty"))
    if int(np.__version__.split(".")[0]) >= 2:   # NumPy 2 removed the method the vendored reader calls on its memmap; this is NumPy's documented spelling
        np.memmap.newbyteorder = lambda self, order="S": self.view(self.dtype.newbyteorder(order))
    import gguf
    from gguf import quants
    from gguf.constants import GGML_QUANT_SIZES, GGMLQuantizationType as T

    os.makedirs(a.out, exist_ok=True)
    rng = np.random.default_rng(20240807)
    path = os.path.join(a.out, "blocks.gguf")
    w = gguf.GGUFWriter(path, "fixture")
    tensors = {}    # name -> (type name, raw uint8 [rows, bytes] or float array)

    def add(name, tname, arr):
        tensors[name] = (tname, arr)
        if arr.dtype == np.uint8:
            w.add_tensor(name, arr, raw_dtype=getattr(T, tname))
        else:
            w.add_tensor(name, arr)

    for tname in QUANTISED:
        bw, bb = GGML_QUANT_SIZES[getattr(T, tname)]
        n = N_BLOCKS[bw]
        rows = 8
        blk = finite_scales(rng.integers(0, 256, (n, bb), dtype=np.uint8), tname, rng)
        add(f"rand.{tname}", tname, blk.reshape(rows, n // rows * bb))
        add(f"nan.{tname}", tname, rng.integers(0, 256, (64, bb), dtype=np.uint8).reshape(2, 32 * bb))
        data = rng.standard_normal((16, 512)).astype(np.float32)
        if tname in CAN_QUANTIZE:
            add(f"gauss.{tname}", tname, quants.quantize(data, getattr(T, tname)))
        else:
            try:
                quants.quantize(data, getattr(T, tname))
            except NotImplementedError:
                pass
            else:
                raise AssertionError(f"the reference quantises {tname} now: add a gauss.{tname} tensor")
    add("float.F32", "F32", (rng.standard_normal((7, 33)) * np.exp(rng.uniform(-30, 30, (7, 33)))).astype(np.float32))
    add("float.F16", "F16", rng.standard_normal((5, 40)).astype(np.float16))
    bf = quants.quantize(rng.standard_normal((3, 64)).astype(np.float32) * 1e3, T.BF16)
    tensors["float.BF16"] = ("BF16", bf)
    w.add_tensor("float.BF16", bf, raw_dtype=T.BF16)
    w.add_uint8("fixture.u8", 200); w.add_int8("fixture.i8", -100); w.add_uint16("fixture.u16", 60000); w.add_int16("fixture.i16", -30000)   # noqa: E702
    w.add_uint32("fixture.u32", 4000000000); w.add_int32("fixture.i32", -2000000000); w.add_float32("fixture.f32", 0.5)                      # noqa: E702
    w.add_uint64("fixture.u64", 2 ** 63 + 5); w.add_int64("fixture.i64", -2 ** 62); w.add_float64("fixture.f64", 1.0 / 3.0)                   # noqa: E702
    w.add_bool("fixture.bool", True); w.add_string("fixture.str", "grüße, GGUF")                                                      # noqa: E702
    w.add_array("fixture.arr_i32", [1, -2, 3]); w.add_array("fixture.arr_str", ["a", "bc", "def"]); w.add_array("fixture.arr_f32", [0.25, -1.5])  # noqa: E702
    w.write_header_to_file(); w.write_kv_data_to_file(); w.write_tensors_to_file(); w.close()                                                  # noqa: E702

    # what the reference reads back
    r = gguf.GGUFReader(path)
    table = []
    expected = {}
    for t in r.tensors:
        name = str(t.name)
        table.append(dict(name=name, type=int(t.tensor_type), type_name=t.tensor_type.name, shape=[int(x) for x in reversed(t.shape.tolist())],
                          offset=int(t.data_offset), nbytes=int(t.n_bytes)))
        tname, arr = tensors[name]
        assert np.array_equal(np.asarray(t.data).reshape(-1).view(np.uint8), np.ascontiguousarray(arr).reshape(-1).view(np.uint8)), name
        expected[name] = np.ascontiguousarray(quants.dequantize(np.asarray(t.data), t.tensor_type), dtype=np.float32).reshape(-1)
        if name.startswith(("rand.", "gauss.", "float.")):
            assert np.isfinite(expected[name]).all(), name
    meta = {}
    for key, field in r.fields.items():
        if key.startswith("GGUF."):
            continue
        types = [int(x) for x in field.types]
        if types[0] == int(gguf.GGUFValueType.STRING):
            val = bytes(field.parts[field.data[0]]).decode("utf-8")
        elif types[0] == int(gguf.GGUFValueType.ARRAY):
            if types[1] == int(gguf.GGUFValueType.STRING):
                val = [bytes(field.parts[i]).decode("utf-8") for i in field.data]
            else:
                val = [field.parts[i].tolist()[0] for i in field.data]
        else:
            val = field.parts[field.data[0]].tolist()[0]
        meta[key] = val
    json.dump(dict(tensors=table, metadata=meta, data_offset=int(r.data_offset), alignment=int(r.alignment)),
              open(os.path.join(a.out, "blocks_table.json"), "w"), indent=1)
    for family, pick in (("q32", lambda n: n.split(".")[1] in CAN_QUANTIZE), ("k_a", lambda n: n.split(".")[1] in ("Q2_K", "Q3_K")),
                         ("k_b", lambda n: n.split(".")[1] in ("Q4_K", "Q5_K")), ("k_c", lambda n: n.split(".")[1] in ("Q6_K", "F32", "F16", "BF16"))):
        np.savez_compressed(os.path.join(a.out, f"blocks_expected_{family}.npz"), **{k: v for k, v in expected.items() if pick(k)})
    json.dump(t5_key_map(a.reference), open(os.path.join(a.out, "t5_key_map.json"), "w"), indent=1)
    for f in sorted(os.listdir(a.out)):
        size = os.path.getsize(os.path.join(a.out, f))
        assert size < 1 << 20, (f, size)
        print(f"{f}: {size} bytes")


if __name__ == "__main__":
    main()
