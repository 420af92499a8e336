"""Writer of the bitsandbytes packed 4-bit tensor format (`QuantState.as_dict(packed=True)`), from fp32 weights: the counterpart of
backend/quant_state.py's reader, for tests and benchmarks (no bitsandbytes package is involved).

    quantize(w, "nf4" | "fp4", blocksize=64, nested=False, nested_blocksize=256) -> {suffix: tensor}   ('' is the packed weight itself)
    pack_state_dict(sd, quant_type, ...) -> state dict in which every 2-D `.weight` is packed (only Linear weights are, operations_bnb.py:120-136)

Per block of `blocksize` weights: absmax = max |w|, every weight / absmax goes to the nearest entry of the 16-value table, two codes per byte (the
even weight in the HIGH nibble).  Nested: the absmax values minus their mean (`nested_offset`) are quantised again, to 8 bits, in blocks of
`nested_blocksize` against a 256-entry table.  The NF4 and FP4 tables below are the published ones.  The nested table is a sorted, seeded table
that contains -1, 0 and 1: the readers are table-driven, and this does NOT reproduce the library's dynamic map."""
import json

import numpy as np
import torch

NF4 = [-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635, -0.18477343022823334, -0.09105003625154495, 0.0,
       0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224, 0.44070982933044434, 0.5626170039176941,
       0.7229568362236023, 1.0]
# sign | 2 exponent bits | 1 mantissa bit, normalised by the largest magnitude (12)
FP4 = [v / 12.0 for v in (0.0, 0.0625, 8.0, 12.0, 4.0, 6.0, 2.0, 3.0)] + [-v / 12.0 for v in (0.0, 0.0625, 8.0, 12.0, 4.0, 6.0, 2.0, 3.0)]
TABLES = {"nf4": np.asarray(NF4, dtype=np.float32), "fp4": np.asarray(FP4, dtype=np.float32)}


def nested_table(seed=0):
    rng = np.random.default_rng(seed)
    t = np.sort(np.concatenate([[-1.0, 0.0, 1.0], np.sign(rng.uniform(-1, 1, 253)) * 10.0 ** rng.uniform(-4, 0, 253)])).astype(np.float32)
    assert t.size == 256
    return t


def _nearest(x, table):
    """index of the table entry nearest to each x (ties to the lower index)"""
    return np.abs(x[..., None] - table[None, :]).argmin(axis=-1).astype(np.uint8)


def _blocks(x, blocksize):
    pad = (-x.size) % blocksize
    return np.concatenate([x, np.zeros(pad, dtype=x.dtype)]).reshape(-1, blocksize)


def quantize(w, quant_type="nf4", blocksize=64, nested=False, nested_blocksize=256, dtype="bfloat16", seed=0):
    table = TABLES[quant_type]
    shape = tuple(int(s) for s in w.shape)
    x = np.ascontiguousarray(w.detach().cpu().float().numpy() if isinstance(w, torch.Tensor) else w, dtype=np.float32).reshape(-1)
    n = x.size
    blk = _blocks(x, blocksize)
    absmax = np.abs(blk).max(axis=1).astype(np.float32)
    q = _nearest(blk / np.where(absmax == 0, 1, absmax)[:, None], table).reshape(-1)[:n + (n & 1)]
    if n & 1:
        q[-1] = 0
    packed = ((q[0::2] << 4) | q[1::2]).astype(np.uint8)
    meta = {"quant_type": quant_type, "blocksize": blocksize, "dtype": dtype, "shape": list(shape)}
    out = {"": torch.from_numpy(packed).reshape(-1, 1), ".quant_map": torch.from_numpy(table.copy())}
    if nested:
        offset = np.float32(absmax.mean())
        a2 = _blocks(absmax - offset, nested_blocksize)
        absmax2 = np.abs(a2).max(axis=1).astype(np.float32)
        table2 = nested_table(seed)
        out[".absmax"] = torch.from_numpy(_nearest(a2 / np.where(absmax2 == 0, 1, absmax2)[:, None], table2).reshape(-1)[:absmax.size].copy())
        out[".nested_absmax"] = torch.from_numpy(absmax2)
        out[".nested_quant_map"] = torch.from_numpy(table2)
        meta.update(nested_blocksize=nested_blocksize, nested_dtype="float32", nested_offset=float(offset))
    else:
        out[".absmax"] = torch.from_numpy(absmax)
    out[".quant_state.bitsandbytes__" + quant_type] = torch.tensor(list(json.dumps(meta).encode("utf-8")), dtype=torch.uint8)
    return out


def pack_state_dict(sd, quant_type="nf4", select=None, **kw):
    """every tensor `select(name, tensor)` accepts (default: 2-D `.weight`s) is replaced by its packed form and side keys"""
    select = select or (lambda k, v: k.endswith(".weight") and v.dim() == 2)
    out = {}
    for k, v in sd.items():
        if select(k, v):
            for suffix, t in quantize(v, quant_type, **kw).items():
                out[k + suffix] = t
        else:
            out[k] = v
    return out
