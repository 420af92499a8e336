"""FreeU v2 restated in torch (shared by tests/test_freeu_host.py and tests/test_gpu_freeu.py).

`freeu_ref` is the closed form the kernels implement -- backbone scaling by the normalised channel mean, and for the skip feature
x + (s - 1) * low(x) with low(x) built from seven weighted sums per plane -- in fp64, NCHW like the reference's output_block_patch.
tests/test_freeu_host.py pins it to the real reference's torch.fft implementation (tests/golden/freeu_ops.pt).
`freeu_kernel_order_f32` restates what csrc/fmx_freeu.hip computes in fp32 with the kernel's summation order (lane-strided sums and an xor
butterfly for the channel mean; per-thread strided pixel sums, folded over the threads of a channel group and then over the pixel chunks,
for the seven sums).  The kernel's multiply-adds may be fused, which torch cannot restate: bitwise equality with the GPU is not claimed."""
import math

import torch

CHUNK_PIXELS = 256   # FMX_FREEU_CHUNK_PIXELS
TPB = 256


def case_inputs(case):
    """the seeded inputs of a freeu_ops.pt case: N(0, 1) + a per-channel offset (so that the channel mean and the lowest bins are not near
    zero), rounded to fp16.  -> h, hsp as fp32 NCHW holding fp16-representable values; the fixture's checksums guard the generator."""
    n, c_h, c_s, hh, ww = case["shape"]
    g = torch.Generator().manual_seed(case["seed"])
    h = torch.randn(n, c_h, hh, ww, generator=g) + 0.5 * torch.randn(n, 1, hh, ww, generator=g) + 0.3
    hsp = torch.randn(n, c_s, hh, ww, generator=g) + 0.5 * torch.randn(n, c_s, 1, 1, generator=g)
    h, hsp = h.half().float(), hsp.half().float()
    if "checksum" in case:
        got = (float(h.double().sum()), float(hsp.double().sum()))
        assert got == tuple(case["checksum"]), f"torch's seeded generator gave other inputs than the fixture was made with: {got} vs {case['checksum']}"
    return h, hsp


def bases(hh, ww, dtype=torch.float64):
    """[7, hh, ww]: 1, cos tr, sin tr, cos tc, sin tc, cos(tr+tc), sin(tr+tc)"""
    tr = (2.0 * math.pi * torch.arange(hh, dtype=torch.float64) / hh).view(hh, 1).expand(hh, ww)
    tc = (2.0 * math.pi * torch.arange(ww, dtype=torch.float64) / ww).view(1, ww).expand(hh, ww)
    return torch.stack([torch.ones(hh, ww, dtype=torch.float64), tr.cos(), tr.sin(), tc.cos(), tc.sin(), (tr + tc).cos(), (tr + tc).sin()]).to(dtype)


def freeu_ref(h, hsp, b, s, dtype=torch.float64):
    """h [N, C_h, H, W], hsp [N, C_s, H, W] -> (h', hsp') in `dtype` (new tensors)"""
    h, hsp = h.to(dtype), hsp.to(dtype)
    n, c_h, hh, ww = h.shape
    m = h.mean(1, keepdim=True)
    lo = m.reshape(n, -1).min(dim=1).values.view(n, 1, 1, 1)
    hi = m.reshape(n, -1).max(dim=1).values.view(n, 1, 1, 1)
    g = (b - 1) * ((m - lo) / (hi - lo)) + 1
    h_out = h.clone()
    h_out[:, :c_h // 2] = h[:, :c_h // 2] * g
    bs = bases(hh, ww, dtype).to(h.device)
    low = torch.zeros_like(hsp)
    for k in range(7):          # elementwise products and sums only: also runs on a device without touching a BLAS or FFT library
        low = low + (hsp * bs[k]).sum(dim=(-2, -1), keepdim=True) * bs[k]
    return h_out, hsp + (s - 1) * (low / (hh * ww))


def _trig32(hh, ww):
    tr = [2.0 * math.pi * r / hh for r in range(hh)]
    tc = [2.0 * math.pi * c / ww for c in range(ww)]
    f = lambda v: torch.tensor(v, dtype=torch.float64).float()  # noqa: E731
    return f([math.cos(a) for a in tr]), f([math.sin(a) for a in tr]), f([math.cos(a) for a in tc]), f([math.sin(a) for a in tc])


def _bases32(hh, ww):
    """[hh*ww, 7] fp32, formed as the kernels form them from the host's fp32 tables"""
    cr, sr, cc, sc = _trig32(hh, ww)
    cr, sr = cr.view(hh, 1).expand(hh, ww), sr.view(hh, 1).expand(hh, ww)
    cc, sc = cc.view(1, ww).expand(hh, ww), sc.view(1, ww).expand(hh, ww)
    return torch.stack([torch.ones(hh, ww), cr, sr, cc, sc, cr * cc - sr * sc, sr * cc + cr * sc], dim=-1).reshape(hh * ww, 7).contiguous()


def freeu_kernel_order_f32(h, skip, b, s):
    """h [N, H, W, C_h], skip [N, H, W, C_s] (fp16 values, any float dtype) -> (h', skip') fp32 BEFORE the final rounding to fp16, computed in
    fp32 in the kernels' order of operations."""
    h, skip = h.float(), skip.float()
    n, hh, ww, c_h = h.shape
    c_s = skip.shape[-1]
    hw = hh * ww
    h, skip = h.reshape(n, hw, c_h), skip.reshape(n, hw, c_s)
    # channel mean: lane l adds the 8-element sums of vectors l, l + 64, ...; xor butterfly over the 64 lanes; times 1 / C
    nv = c_h // 8
    v8 = h.reshape(n, hw, nv, 8)
    s8 = v8[..., 0].clone()
    for j in range(1, 8):
        s8 = s8 + v8[..., j]
    lanes = torch.zeros(n, hw, 64)
    for r in range(0, nv, 64):
        part = s8[..., r:r + 64]
        lanes[..., :part.shape[-1]] = lanes[..., :part.shape[-1]] + part
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[..., idx ^ o]
    mean = lanes[..., 0] * torch.tensor(1.0 / c_h, dtype=torch.float64).float()
    lo, hi = mean.min(dim=1, keepdim=True).values, mean.max(dim=1, keepdim=True).values
    g = torch.tensor(b, dtype=torch.float32).sub(1.0) * ((mean - lo) / (hi - lo)) + 1.0
    h_out = h.clone()
    h_out[..., :c_h // 2] = h[..., :c_h // 2] * g.unsqueeze(-1)
    # seven sums: a thread owns 8 channels and every nsub-th pixel of a 256-pixel chunk; threads of a group, then chunks, are added in order
    bs = _bases32(hh, ww)
    ncg = c_s // 8
    sums = torch.zeros(n, 7, c_s)
    for g0 in range(0, ncg, TPB):
        gper = min(TPB, ncg - g0)
        nsub = TPB // gper
        cols = slice(g0 * 8, (g0 + gper) * 8)
        total = None
        for start in range(0, hw, CHUNK_PIXELS):
            cnt = min(CHUNK_PIXELS, hw - start)
            acc = torch.zeros(n, nsub, 7, gper * 8)
            for it in range(-(-cnt // nsub)):
                pix = start + it * nsub + torch.arange(nsub)
                ok = (pix < start + cnt)
                pix = pix.clamp_max(hw - 1)
                x = skip[:, pix, cols]                                 # [n, nsub, gper*8]
                term = x.unsqueeze(2) * bs[pix].view(1, nsub, 7, 1)
                acc = torch.where(ok.view(1, nsub, 1, 1), acc + term, acc)
            chunk = acc[:, 0]
            for sub in range(1, nsub):
                chunk = chunk + acc[:, sub]
            total = chunk if total is None else total + chunk
        sums[:, :, cols] = torch.zeros(n, 7, gper * 8) + total
    coef = (torch.tensor(s, dtype=torch.float32) - 1.0) / (torch.tensor(float(hh)) * torch.tensor(float(ww)))
    low = sums[:, 0].unsqueeze(1).expand(n, hw, c_s).clone()
    for k in range(1, 7):
        low = low + sums[:, k].unsqueeze(1) * bs[:, k].view(1, hw, 1)
    skip_out = skip + coef * low
    return h_out.reshape(n, hh, ww, c_h), skip_out.reshape(n, hh, ww, c_s)


def ulp_distance_f16(a, b):
    """|distance| in fp16 representable values between two fp16 tensors (0 = same value; +0 and -0 are the same value)"""
    def ordered(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (ordered(a.half()) - ordered(b.half())).abs()


def nhwc16(t):
    return t.permute(0, 2, 3, 1).contiguous().half()
