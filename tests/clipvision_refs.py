"""Cases and references of the two CLIP-vision front-end kernels (include/fmx_clipvision.h), shared by tests/test_clipvision_host.py and
tests/test_gpu_clipvision.py: built once per process, never modified.

clip_patch_rows: the torch CPU expression of the reference's clip_preprocess (fp32) followed by .half() and the unfold -- bit for bit.
clip_embed_ln: an fp64 restatement, and an fp32 restatement in the kernel's own summation order (one wave per row: lane l adds the elements of
octets l, l + 64, ... in column order, then a 6-step xor butterfly; fused multiply-adds where the kernel has them).  EMBED_RESTATEMENT_ULPS is the
worst fp16 distance between the two over EMBED_CASES, measured on the CPU by test_clipvision_host; the GPU gate is that plus one ulp."""
import functools

import numpy as np
import torch

MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
PATCH_CASES = [(1, 224, 224), (3, 231, 224), (2, 224, 300)]          # b, rh, rw: no crop; top = 3 (the odd remainder); left = 38
EMBED_CASES = [(c, b, t_pad) for c in (128, 320, 1664) for b, t_pad in ((1, 320), (3, 384))]
EMBED_RESTATEMENT_ULPS = 1      # measured: test_clipvision_host.test_embed_ln_kernel_order_in_fp32_vs_fp64
EMBED_GATE_ULPS = EMBED_RESTATEMENT_ULPS + 1
EPS = 1e-5
EQUAL_ROW = (0, 6)              # (image, token) of the row whose elements are all equal: variance 0, output = beta


def crop_of(rh, rw):
    return (rh - 224) // 2, (rw - 224) // 2


@functools.lru_cache(maxsize=None)
def patch_case(b, rh, rw):
    """fp32 [b, 3, rh, rw]: uniform in [-0.1, 1.1) (values below 0 and above 1), exact 0 and 1, and the levels (k + 0.5) / 255 -- where 255 x is
    exactly k + 0.5 in fp32 the rounding is a tie"""
    g = torch.Generator().manual_seed(1000 + b * 7 + rh + rw)
    x = torch.rand(b, 3, rh, rw, generator=g) * 1.2 - 0.1
    flat = x.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)
    ties = (torch.arange(255, dtype=torch.float32) + 0.5) / 255.0
    n = ties.numel()
    for rep in range(40):
        flat[idx[rep * n:(rep + 1) * n]] = ties
    flat[idx[40 * n:40 * n + 500]] = 0.0
    flat[idx[40 * n + 500:40 * n + 1000]] = 1.0
    return x


def quantised_levels(x):
    return torch.clip(255.0 * x, 0, 255).round()


def patch_rows_ref(x, top, left):
    """torch CPU: crop, clip(255 x, 0, 255).round() / 255, - mean, / std in fp32, .half(), unfold to [b * 256, 640] with zero columns 588..639"""
    b = x.shape[0]
    v = quantised_levels(x[:, :, top:top + 224, left:left + 224]) / 255.0
    v = ((v - torch.tensor(MEAN).view(3, 1, 1)) / torch.tensor(STD).view(3, 1, 1)).half()
    rows = v.view(b, 3, 16, 14, 16, 14).permute(0, 2, 4, 1, 3, 5).reshape(b * 256, 588)
    return torch.cat([rows, torch.zeros(b * 256, 52, dtype=torch.float16)], 1)


@functools.lru_cache(maxsize=None)
def embed_case(c, b):
    """fp16 operands: patches [b * 256, c], class [c], pos [257, c], gamma, beta [c]; row EQUAL_ROW sums to 0.5 in every column"""
    g = torch.Generator().manual_seed(2000 + c + b)
    patches = (torch.randn(b * 256, c, generator=g) * 0.7).half()
    cls = (torch.randn(c, generator=g) * 0.5).half()
    pos = (torch.randn(257, c, generator=g) * 0.5).half()
    gamma = (1.0 + 0.1 * torch.randn(c, generator=g)).half()
    beta = (0.1 * torch.randn(c, generator=g)).half()
    img, tok = EQUAL_ROW
    patches[img * 256 + tok - 1] = 0.25
    pos[tok] = 0.25
    return patches, cls, pos, gamma, beta


def _rows(patches, cls, pos, b, dtype):
    c = patches.shape[1]
    x = torch.cat([cls.to(dtype).expand(b, 1, c), patches.to(dtype).view(b, 256, c)], 1)
    return x + pos.to(dtype)


def embed_ref64(patches, cls, pos, gamma, beta, b, t_pad, eps=EPS):
    """fp64 [b, t_pad, c]: LayerNorm of class / patches + position, zero rows behind the 257 tokens"""
    x = _rows(patches, cls, pos, b, torch.float64)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    y = (x - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()
    return torch.cat([y, torch.zeros(b, t_pad - 257, x.shape[-1], dtype=torch.float64)], 1)


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)    # the product of two fp32 is exact in fp64


def _wave_sum(s):
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
    return s[:, 0]


def embed_kernel_order_f32(patches, cls, pos, gamma, beta, b, t_pad, eps=EPS):
    """the kernel's arithmetic in fp32, in its order -> fp32 [b, t_pad, c] (before the rounding to fp16)"""
    c = patches.shape[1]
    x = _rows(patches, cls, pos, b, torch.float32).reshape(b * 257, c).numpy()          # fp16 + fp16 in fp32: one fp32 addition, as in the kernel
    rows, oct_ = x.shape[0], c // 8
    J = -(-oct_ // 64)
    xp = np.zeros((rows, J * 64 * 8), dtype=np.float32)
    valid = np.zeros((J * 64 * 8,), dtype=bool)
    xp[:, :c], valid[:c] = x, True
    xp, valid = xp.reshape(rows, J, 64, 8), valid.reshape(J, 64, 8)
    s = np.zeros((rows, 64), dtype=np.float32)
    for j in range(J):
        for e in range(8):
            s = s + xp[:, j, :, e]                                                        # (an absent octet adds +0: exact)
    mean = _wave_sum(s) / np.float32(c)
    d = np.where(valid[None], xp - mean[:, None, None, None], np.float32(0))
    q = np.zeros((rows, 64), dtype=np.float32)
    for j in range(J):
        for e in range(8):
            q = _fma32(d[:, j, :, e], d[:, j, :, e], q)
    rstd = np.float32(1.0) / np.sqrt(_wave_sum(q) / np.float32(c) + np.float32(eps), dtype=np.float32)
    dn = (d.reshape(rows, -1)[:, :c] * rstd[:, None]).astype(np.float32)
    y = _fma32(dn, gamma.float().numpy()[None], beta.float().numpy()[None])
    y = torch.from_numpy(y).view(b, 257, c)
    return torch.cat([y, torch.zeros(b, t_pad - 257, c)], 1)


def ulp_distance_f16(a, b):
    """distance in fp16 representable values between two tensors rounded to fp16 (+0 and -0 are the same value)"""
    def ordered(t):
        i = t.contiguous().half().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (ordered(a) - ordered(b)).abs()
