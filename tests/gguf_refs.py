"""Host reference for GGUF dequantisation: numpy, written from the ggml block layouts (not from the reference's vendored package, which does
not exist on the GPU box).  `dequant(raw, qtype)` -> fp32, the value ggml defines; tests/test_gguf_refs.py pins it bit for bit to what the
reference's own numpy `dequantize` recorded in tests/golden/gguf/blocks_expected.npz, and the GPU tests compare the kernels against its
16-bit rounding.

Every product below is exact in fp32 (an fp16 scale has 11 significant bits, sub-scales 4-8, quants 2-8: at most 24 together) and at most
one addition rounds, so the order of operations is fixed only where it decides inf / NaN propagation; it follows ggml's.

`bug=`: one planted mistake per family, for the teeth tests (a comparison that cannot fail shows nothing).
"""
import numpy as np

F32, F16, Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q2_K, Q3_K, Q4_K, Q5_K, Q6_K, BF16 = 0, 1, 2, 3, 6, 7, 8, 10, 11, 12, 13, 14, 30
NAMES = {F32: "F32", F16: "F16", Q4_0: "Q4_0", Q4_1: "Q4_1", Q5_0: "Q5_0", Q5_1: "Q5_1", Q8_0: "Q8_0", Q2_K: "Q2_K", Q3_K: "Q3_K",
         Q4_K: "Q4_K", Q5_K: "Q5_K", Q6_K: "Q6_K", BF16: "BF16"}
BLOCK = {F32: (1, 4), F16: (1, 2), BF16: (1, 2), Q4_0: (32, 18), Q4_1: (32, 20), Q5_0: (32, 22), Q5_1: (32, 24), Q8_0: (32, 34),
         Q2_K: (256, 84), Q3_K: (256, 110), Q4_K: (256, 144), Q5_K: (256, 176), Q6_K: (256, 210)}   # weights, bytes per block
QUANTISED = (Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q2_K, Q3_K, Q4_K, Q5_K, Q6_K)
BUGS = {"nibble_swap": (Q4_0, Q4_1, Q5_0, Q5_1, Q4_K, Q5_K, Q6_K), "q5_high_bit_word": (Q5_0, Q5_1), "k_scale_off_by_one": (Q2_K, Q3_K, Q4_K, Q5_K, Q6_K),
        "q6_no_offset": (Q6_K,), "q3_mask_inverted": (Q3_K,)}


def _f16(b):       # [n, 2] uint8 -> [n, 1] fp32
    return np.ascontiguousarray(b).view("<f2").astype(np.float32)


def _nibbles(qs, swap):
    """[n, k] bytes -> [n, 2k]: all low nibbles, then all high nibbles (the 32-weight types and each 64-weight group of Q4_K / Q5_K)"""
    lo, hi = qs & 0x0F, qs >> 4
    return np.concatenate([hi, lo] if swap else [lo, hi], axis=-1)


def _k_scale_min(s):
    """12 bytes -> 8 six-bit scales, 8 six-bit minima (Q4_K / Q5_K): entries 0..3 are the low 6 bits of bytes 0..3 / 4..7; entries 4..7 take their
    low nibble from bytes 8..11 (scale: low half, minimum: high half) and their top two bits from the top of bytes 0..3 / 4..7"""
    d, m, md = s[:, 0:4], s[:, 4:8], s[:, 8:12]
    sc = np.concatenate([d & 0x3F, (md & 0x0F) | ((d >> 2) & 0x30)], axis=-1)
    mn = np.concatenate([m & 0x3F, (md >> 4) | ((m >> 2) & 0x30)], axis=-1)
    return sc, mn


def _bits(b, width, count):
    """[n, k] bytes -> [n, count, k]: field i of each byte (`width` bits at bit i * width)"""
    sh = (np.arange(count, dtype=np.uint8) * width).reshape(1, count, 1)
    return (b[:, None, :] >> sh) & np.uint8((1 << width) - 1)


def _roll(x, bug):
    return np.roll(x, 1, axis=1) if bug == "k_scale_off_by_one" else x


def dequant_blocks(blk, qtype, bug=None):
    """[n_blocks, bytes per block] uint8 -> [n_blocks, weights per block] fp32"""
    n = blk.shape[0]
    swap = bug == "nibble_swap"
    f = np.float32
    if qtype == Q8_0:
        return blk[:, 2:].view(np.int8).astype(f) * _f16(blk[:, :2])
    if qtype == Q4_0:
        return _f16(blk[:, :2]) * (_nibbles(blk[:, 2:], swap).astype(np.int8) - np.int8(8)).astype(f)
    if qtype == Q4_1:
        return _f16(blk[:, :2]) * _nibbles(blk[:, 4:], swap).astype(f) + _f16(blk[:, 2:4])
    if qtype in (Q5_0, Q5_1):
        o = 2 if qtype == Q5_0 else 4
        qh = np.ascontiguousarray(blk[:, o:o + 4]).view("<u4")                         # [n, 1]: bit j belongs to weight j
        if bug == "q5_high_bit_word":
            qh = np.ascontiguousarray(blk[:, o + 2:o + 6]).view("<u4")
        hb = ((qh >> np.arange(32, dtype=np.uint32)[None, :]) & 1).astype(np.uint8)
        q = _nibbles(blk[:, o + 4:], swap) | (hb << 4)
        if qtype == Q5_0:
            return _f16(blk[:, :2]) * (q.astype(np.int8) - np.int8(16)).astype(f)
        return _f16(blk[:, :2]) * q.astype(f) + _f16(blk[:, 2:4])
    if qtype == Q2_K:      # scales[16] (low nibble scale, high nibble minimum), qs[64], d, dmin; weights in two halves of 128, 2-bit fields plane by plane
        sc = _roll(blk[:, :16], bug)
        dl = (_f16(blk[:, 80:82]) * (sc & 0x0F).astype(f)).reshape(n, 16, 1)
        ml = (_f16(blk[:, 82:84]) * (sc >> 4).astype(f)).reshape(n, 16, 1)
        q = np.stack([_bits(blk[:, 16 + 32 * h:48 + 32 * h], 2, 4) for h in range(2)], axis=1)   # [n, 2, 4, 32]
        return (dl * q.reshape(n, 16, 16).astype(f) - ml).reshape(n, 256)
    if qtype == Q3_K:      # hmask[32], qs[64], scales[12], d
        s = blk[:, 96:108]
        lo = np.concatenate([s[:, :8] & 0x0F, s[:, :8] >> 4], axis=-1)                            # [n, 16]
        hi = _bits(s[:, 8:12], 2, 4).reshape(n, 16)
        sc = _roll((lo | (hi << 4)).astype(np.int8) - np.int8(32), bug)
        dl = (_f16(blk[:, 108:110]) * sc.astype(f)).reshape(n, 16, 1)
        ql = np.stack([_bits(blk[:, 32 + 32 * h:64 + 32 * h], 2, 4) for h in range(2)], axis=1).reshape(n, 256)
        hb = _bits(blk[:, :32], 1, 8).reshape(n, 256)                                             # plane i of the mask belongs to weights 32 i ..
        if bug != "q3_mask_inverted":
            hb = hb ^ 1                                                                             # a SET bit means "no offset"
        q = ql.astype(np.int8) - (hb << 2).astype(np.int8)
        return (dl * q.reshape(n, 16, 16).astype(f)).reshape(n, 256)
    if qtype in (Q4_K, Q5_K):   # d, dmin, scales[12], (qh[32],) qs[128]
        sc, mn = _k_scale_min(blk[:, 4:16])
        sc, mn = _roll(sc, bug), _roll(mn, bug)
        d = (_f16(blk[:, :2]) * sc.astype(f)).reshape(n, 8, 1)
        dm = (_f16(blk[:, 2:4]) * mn.astype(f)).reshape(n, 8, 1)
        o = 16 if qtype == Q4_K else 48
        q = np.concatenate([_nibbles(blk[:, o + 32 * c:o + 32 * c + 32], swap) for c in range(4)], axis=-1)   # [n, 256]
        if qtype == Q5_K:
            q = q | (_bits(blk[:, 16:48], 1, 8).reshape(n, 256) << 4)
        return (d * q.reshape(n, 8, 32).astype(f) - dm).reshape(n, 256)
    if qtype == Q6_K:      # ql[128], qh[64], scales[16] int8, d
        sc = _roll(blk[:, 192:208].view(np.int8), bug)
        d = (_f16(blk[:, 208:210]) * sc.astype(f)).reshape(n, 16, 1)
        ql = np.concatenate([_nibbles(blk[:, 64 * h:64 * h + 64], swap) for h in range(2)], axis=-1)          # [n, 256]
        qh = np.stack([_bits(blk[:, 128 + 32 * h:160 + 32 * h], 2, 4) for h in range(2)], axis=1).reshape(n, 256)
        q = (ql | (qh << 4)).astype(np.int8)
        if bug != "q6_no_offset":
            q = q - np.int8(32)
        return (d * q.reshape(n, 16, 16).astype(f)).reshape(n, 256)
    raise NotImplementedError(f"GGML type {qtype}")


def dequant(raw, qtype, bug=None):
    """packed bytes (any shape, uint8) -> flat fp32 array of the weights"""
    raw = np.ascontiguousarray(raw).reshape(-1)
    if qtype == F32:
        return raw.view("<f4").copy()
    if qtype == F16:
        return raw.view("<f2").astype(np.float32)
    if qtype == BF16:
        return (raw.view("<u2").astype(np.uint32) << 16).view(np.float32)
    bw, bb = BLOCK[qtype]
    if raw.size % bb:
        raise ValueError(f"{raw.size} bytes is not a whole number of {NAMES[qtype]} blocks")
    return dequant_blocks(raw.reshape(-1, bb), qtype, bug).reshape(-1)


def same_bits(a, b):
    """two float arrays equal bit for bit, NaNs compared by position only -> (ok, number of differing elements)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False, -1
    u = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
    na, nb = np.isnan(a), np.isnan(b)
    bad = (na != nb) | (~na & (a.view(u) != b.view(u)))
    return not bool(bad.any()), int(bad.sum())
