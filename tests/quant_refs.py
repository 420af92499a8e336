"""Host reference (numpy) of the storage-expansion kernels' contract (include/fmx.h, float8 / bitsandbytes section): what fmx_fp8_expand_* and
fmx_bnb4_dequant_* must produce, in fp32 before the single rounding to the output type.

fp8: the value of each code, by bit arithmetic (e4m3fn: bias 7, no infinities, 0x7F / 0xFF NaN; e5m2: bias 15, IEEE-like).  tests/test_quant_host.py
pins the table to torch's CPU conversion for all 256 codes.
bnb4: weight i is the HIGH nibble of byte i >> 1 when i is even, the low one when odd; value = code16[nibble] * scale(block of i) in one fp32
multiply; scale = absmax[b], or nested code256[absmax_u8[b]] * absmax2[b // blocksize2] + offset: one fp32 multiply, then one fp32 add, each
rounded.  numpy float32 arithmetic rounds after every operation, which is exactly that."""
import numpy as np
import torch

E4M3FN, E5M2 = 0, 1


def fp8_table(kind):
    """fp32 values of the 256 codes (NaN codes: a quiet NaN)"""
    e_bits, m_bits = (4, 3) if kind == E4M3FN else (5, 2)
    bias = (1 << (e_bits - 1)) - 1
    out = np.zeros(256, dtype=np.float32)
    for c in range(256):
        sign = -1.0 if c & 0x80 else 1.0
        e, m = (c >> m_bits) & ((1 << e_bits) - 1), c & ((1 << m_bits) - 1)
        if kind == E4M3FN and e == 15 and m == 7:
            v = float("nan")
        elif kind == E5M2 and e == 31:
            v = float("nan") if m else sign * float("inf")
        elif e == 0:
            v = sign * m * 2.0 ** (1 - bias - m_bits)
        else:
            v = sign * (1 + m / (1 << m_bits)) * 2.0 ** (e - bias)
        out[c] = v
    return out


def fp8_expand(codes, kind):
    return fp8_table(kind)[np.asarray(codes, dtype=np.uint8)]


def bnb4_scales(n, blocksize, absmax, code256=None, absmax2=None, offset=0.0, blocksize2=0):
    """fp32 scale of every block"""
    nblocks = (n + blocksize - 1) // blocksize
    if code256 is None:
        return np.asarray(absmax, dtype=np.float32)[:nblocks]
    b = np.arange(nblocks)
    prod = np.asarray(code256, dtype=np.float32)[np.asarray(absmax, dtype=np.uint8)[:nblocks]] * np.asarray(absmax2, dtype=np.float32)[b // blocksize2]
    return prod.astype(np.float32) + np.float32(offset)


def bnb4_dequant(packed, n, code16, blocksize, absmax, code256=None, absmax2=None, offset=0.0, blocksize2=0):
    """-> fp32 [n]"""
    packed = np.asarray(packed, dtype=np.uint8).reshape(-1)
    assert packed.size == (n + 1) // 2
    i = np.arange(n)
    byte = packed[i >> 1]
    q = np.where(i & 1, byte & 15, byte >> 4)
    with np.errstate(all="ignore"):
        s = bnb4_scales(n, blocksize, absmax, code256, absmax2, offset, blocksize2)
        return (np.asarray(code16, dtype=np.float32)[q] * s[i // blocksize]).astype(np.float32)


def nested_case(n, blocksize, blocksize2, code16, code256, seed):
    """random packed bytes and nested scales for n weights whose `offset` makes the nested add round everywhere and CANCEL in block 0: offset is
    minus the rounded product code256[a] * absmax2 of that block (chosen inexact in fp32), so multiply-then-add gives a scale of exactly 0 there
    while a fused multiply-add gives the product's rounding error (~2^-14 here: visible in fp16 and bf16)"""
    rng = np.random.default_rng([seed, n, blocksize])
    nblocks = (n + blocksize - 1) // blocksize
    absmax_u8 = rng.integers(0, 256, nblocks, dtype=np.uint8)
    absmax2 = rng.uniform(500.0, 2000.0, (nblocks + blocksize2 - 1) // blocksize2).astype(np.float32)
    code256 = np.asarray(code256, dtype=np.float32)
    for a in range(255, 0, -1):                                      # the largest code whose product with absmax2[0] is inexact in fp32
        exact = np.float64(code256[a]) * np.float64(absmax2[0])
        if abs(code256[a]) > 0.25 and np.float64(np.float32(exact)) != exact:
            break
    absmax_u8[0] = a
    offset = -np.float32(code256[a] * absmax2[0])
    return dict(packed=rng.integers(0, 256, (n + 1) // 2, dtype=np.uint8), n=n, code16=np.asarray(code16, dtype=np.float32), blocksize=blocksize,
                absmax=absmax_u8, code256=code256, absmax2=absmax2, offset=offset, blocksize2=blocksize2)


def rounded(ref32, dtype):
    """the contract's right-hand side: fp32 -> dtype, once, to nearest even (torch's CPU conversion), as int16 bit patterns + the NaN mask"""
    t = torch.from_numpy(np.ascontiguousarray(ref32, dtype=np.float32)).to(dtype)
    return t.view(torch.int16), torch.isnan(t)


def assert_same_bits(got, ref32, what):
    """got: tensor of a 16-bit type; ref32: numpy fp32 of the same element count.  Integers compared, NaNs by position"""
    want, want_nan = rounded(np.asarray(ref32).reshape(-1), got.dtype)
    g = got.detach().reshape(-1).cpu()
    got_nan = torch.isnan(g)
    assert g.numel() == want.numel(), what
    assert torch.equal(got_nan, want_nan), (what, "NaN positions differ", int((got_nan != want_nan).sum()))
    bad = (g.view(torch.int16) != want) & ~want_nan
    nbad = int(bad.sum())
    if nbad:
        i = int(torch.nonzero(bad)[0])
        raise AssertionError(f"{what}: {nbad} of {g.numel()} elements differ; first at {i}: got {float(g[i])!r} want {float(np.asarray(ref32).reshape(-1)[i])!r}")


def state_dict_reference(sd, dtype=torch.float32):
    """a state dict in the packed formats (raw float8 tensors, bitsandbytes packed tensors with their side keys) -> {name: fp32 tensor}: what the
    file's bytes mean (the bnb side keys are consumed)"""
    import json
    out = {}
    marker = ".quant_state.bitsandbytes__"
    packed = {k[:k.index(marker)]: k for k in sd if marker in k}
    side = {w + s for w in packed for s in (".quant_map", ".absmax", ".nested_absmax", ".nested_quant_map")} | set(packed.values())
    for k, v in sd.items():
        if k in side:
            continue
        if k in packed:
            meta = json.loads(bytes(sd[packed[k]].tolist()).decode())
            n = int(np.prod(meta["shape"]))
            nested = "nested_blocksize" in meta
            vals = bnb4_dequant(v.numpy(), n, sd[k + ".quant_map"].numpy(), meta["blocksize"], sd[k + ".absmax"].numpy(),
                                sd[k + ".nested_quant_map"].numpy() if nested else None, sd[k + ".nested_absmax"].numpy() if nested else None,
                                np.float32(meta.get("nested_offset", 0.0)), meta.get("nested_blocksize", 0))
            out[k] = torch.from_numpy(vals.reshape(meta["shape"]).copy())
        elif v.dtype in (torch.float8_e4m3fn, torch.float8_e5m2):
            kind = E4M3FN if v.dtype == torch.float8_e4m3fn else E5M2
            out[k] = torch.from_numpy(fp8_expand(v.view(torch.uint8).numpy(), kind).copy()).reshape(v.shape)
        else:
            out[k] = v
    return out
