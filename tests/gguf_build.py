"""Test helper: quantised GGUF twins of the tiny models the suite already uses, built at test time from seeds (a committed copy of the tiny Flux
transformer would be several MB in any GGML type).  What the blocks MEAN is not decided here: tests/gguf_refs.py is, and it is pinned bit for bit
to the reference's own dequantiser (tests/test_gguf_refs.py).  The quantisers below are simple round-to-nearest ones -- the loader must accept
any valid block, not the output of one particular quantiser -- and the K families, for which no quantiser is written, get random blocks whose
fp16 super-scales are chosen so that the weights have the magnitude of the originals."""
import os
import sys

import numpy as np

import gguf_refs as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from gguf_write import write_gguf  # noqa: E402

ROTATION = (R.Q8_0, R.Q4_K, R.Q4_0, R.Q6_K, R.Q5_1, R.Q2_K, R.Q4_1, R.Q5_K, R.Q5_0, R.Q3_K)
# llama.cpp names of a T5 encoder -> HF names: the inverse of the key map of the reference's loader (tests/golden/gguf/t5_key_map.json pins the forward one)
T5_TO_LLAMA = (("encoder.final_layer_norm", "enc.output_norm"), ("encoder.block.", "enc.blk."), ("layer.0.SelfAttention.relative_attention_bias", "attn_rel_b"),
               ("layer.0.SelfAttention.q", "attn_q"), ("layer.0.SelfAttention.k", "attn_k"), ("layer.0.SelfAttention.v", "attn_v"),
               ("layer.0.SelfAttention.o", "attn_o"), ("layer.0.layer_norm", "attn_norm"), ("layer.1.DenseReluDense.wi_1", "ffn_up"),
               ("layer.1.DenseReluDense.wo", "ffn_down"), ("layer.1.DenseReluDense.wi_0", "ffn_gate"), ("layer.1.layer_norm", "ffn_norm"),
               ("shared", "token_embd"))


def _half_bytes(x):
    return np.ascontiguousarray(x.astype("<f2")).view(np.uint8).reshape(x.shape[0], 2)


def _pack_nibbles(q):      # [n, 32] values 0..15 -> [n, 16]: weight j in the low nibble of byte j, weight j + 16 in the high one
    return (q[:, :16] | (q[:, 16:] << 4)).astype(np.uint8)


def quantize32(x, qtype):
    """[n, 32] fp32 -> [n, bytes] uint8 for the five 32-weight types"""
    amax = np.abs(x).max(axis=1, keepdims=True)
    if qtype == R.Q8_0:
        d = amax / 127
        q = np.rint(x / np.where(d == 0, 1, d)).astype(np.int8)
        return np.concatenate([_half_bytes(d), q.view(np.uint8)], axis=1)
    bits = 4 if qtype in (R.Q4_0, R.Q4_1) else 5
    top = (1 << bits) - 1
    if qtype in (R.Q4_0, R.Q5_0):
        d = amax / (top // 2)
        q = np.clip(np.rint(x / np.where(d == 0, 1, d)) + (top + 1) // 2, 0, top).astype(np.uint8)
        head = [_half_bytes(d)]
    else:
        lo, hi = x.min(axis=1, keepdims=True), x.max(axis=1, keepdims=True)
        d = (hi - lo) / top
        q = np.clip(np.rint((x - lo) / np.where(d == 0, 1, d)), 0, top).astype(np.uint8)
        head = [_half_bytes(d), _half_bytes(lo)]
    if bits == 5:
        qh = ((q >> 4).astype(np.uint32) << np.arange(32, dtype=np.uint32)[None, :]).sum(axis=1, dtype=np.uint32)
        head.append(np.ascontiguousarray(qh.astype("<u4")).view(np.uint8).reshape(-1, 4))
    return np.concatenate(head + [_pack_nibbles(q & 15)], axis=1)


_K_SCALES = {R.Q2_K: ((80, 82), 15 * 3 / 2), R.Q3_K: ((108,), 32 * 4 / 2), R.Q4_K: ((0, 2), 63 * 15 / 2), R.Q5_K: ((0, 2), 63 * 31 / 2),
             R.Q6_K: ((208,), 128 * 32 / 2)}   # offsets of the fp16 super-scales, and the typical |sub-scale x quant| they multiply


def random_k_blocks(n, qtype, magnitude, rng):
    """n random blocks of a K family whose weights are of the order of `magnitude`"""
    blk = rng.integers(0, 256, (n, R.BLOCK[qtype][1]), dtype=np.uint8)
    offs, typical = _K_SCALES[qtype]
    for o in offs:
        d = (magnitude / typical * rng.uniform(0.5, 1.5, (n, 1))).astype(np.float32)
        blk[:, o:o + 2] = _half_bytes(d)
    return blk


def quantize_tensor(w, qtype, rng):
    """fp32 array -> packed bytes [rows, bytes per row]"""
    w = np.ascontiguousarray(w, dtype=np.float32)
    bw, bb = R.BLOCK[qtype]
    if qtype == R.F32:
        return w.reshape(-1).view(np.uint8)
    if qtype == R.F16:
        return w.astype("<f2").reshape(-1).view(np.uint8)
    if bw == 32:
        return quantize32(w.reshape(-1, 32), qtype).reshape(-1)
    return random_k_blocks(w.size // 256, qtype, float(np.abs(w).mean()) or 1.0, rng).reshape(-1)


def quantize_state_dict(sd, seed=0, rename=None):
    """{name: fp32 torch tensor} -> [(name, qtype, shape, raw)]: matrices take the GGML types in rotation (a row length that is not a multiple of
    256 takes the next 32-weight type), vectors stay F32 and every fourth one F16, as real files keep norm scales and biases unquantised"""
    rng = np.random.default_rng(seed)
    out, turn, vec = [], 0, 0
    for name, t in sd.items():
        w = t.detach().cpu().float().numpy()
        if w.ndim < 2 or w.shape[-1] % 32:
            qtype = R.F16 if vec % 4 == 3 else R.F32
            vec += 1
        else:
            qtype = ROTATION[turn % len(ROTATION)]
            while R.BLOCK[qtype][0] == 256 and w.shape[-1] % 256:
                turn += 1
                qtype = ROTATION[turn % len(ROTATION)]
            turn += 1
        out.append((rename(name) if rename else name, qtype, tuple(w.shape), quantize_tensor(w, qtype, rng)))
    return out


def t5_llama_name(name):
    """'transformer.encoder.block.0.layer.0.SelfAttention.q.weight' -> 'enc.blk.0.attn_q.weight' (the names city96's T5 GGUF files use)"""
    if name.startswith("transformer."):
        name = name[len("transformer."):]
    for hf, ll in T5_TO_LLAMA:
        name = name.replace(hf, ll)
    return name


def reference_state_dict(tensors):
    """[(name, qtype, shape, raw)] -> {name: fp32 torch tensor}: what the file's blocks mean"""
    import torch
    return {name: torch.from_numpy(R.dequant(raw, qtype).reshape(shape).copy()) for name, qtype, shape, raw in tensors}


def write(path, tensors, architecture):
    return write_gguf(str(path), tensors, {"general.architecture": architecture, "general.quantization_version": 2})
