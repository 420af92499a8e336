"""fp64 references and ulp tolerances shared by the kernel-level parity tests (tests/test_gpu_kernels_bf16.py, tests/test_gpu_small_kernels.py,
tests/test_gpu_gemm_windows.py, tests/test_gpu_vae_direct.py, tests/test_gpu_sampler_kernels.py, tests/test_gpu_groupnorm_routes.py,
tests/test_gpu_token_kernels.py) and their CPU companion (tests/test_kernel_ref_teeth.py), which plants one plausible bug into each reference and checks that the GPU tests'
tolerance would reject it.

Discipline: every reference is the same operation in fp64 on the kernel's own rounded inputs (the fp16 / bf16 tensors it read, upcast).
A tolerance is `ulps` units in the last place of the REFERENCE value in the output element type plus an absolute floor `atol`;
`excess()` is the largest error in units of that tolerance: <= 1 passes, and a planted bug must reach >= 4.  Plain module (not a
conftest.py): the test files import it by name."""
import math

import numpy as np
import torch
import torch.nn.functional as F

# (explicit mantissa bits, smallest normal exponent) per element type: one ulp of 1.0 is 2^-mant
_FMT = {torch.float16: (10, -14), torch.bfloat16: (7, -126), torch.float32: (23, -126)}
EPS = {dt: 2.0 ** -m for dt, (m, _) in _FMT.items()}   # fp16 2^-10 per ulp at 1 (2^-11 relative rounding), bf16 2^-7 (2^-8 relative)


def ulp(want, dtype):
    """one ulp of the fp64 values `want` in `dtype` (subnormal spacing below the normal range)"""
    mant, emin = _FMT[dtype]
    e = torch.floor(torch.log2(want.double().abs().clamp_min(2.0 ** emin)))
    return torch.exp2(e - mant)


def excess(got, want, dtype, ulps, atol=0.0):
    """max |got - want| / (ulps * ulp(want) + atol) over the finite reference values; non-finite reference entries must match exactly"""
    got, want = got.double().cpu(), want.double().cpu()
    fin = torch.isfinite(want)
    if not bool(torch.equal(got[~fin].nan_to_num(nan=1.5e308), want[~fin].nan_to_num(nan=1.5e308))):
        return math.inf
    if not bool(fin.any()):
        return 0.0
    err = (got[fin] - want[fin]).abs() / (ulps * ulp(want[fin], dtype) + atol)
    return float(err.nan_to_num(nan=math.inf).max())


def assert_within(got, want, dtype, ulps, atol, what):
    e = excess(got, want, dtype, ulps, atol)
    assert e <= 1.0, f"{what}: error {e:.3g}x the tolerance ({ulps} ulp of {dtype} + {atol:.3g})"


def rounded(x, dtype):
    """x rounded to dtype and back to fp64: the values a kernel reading `dtype` sees"""
    return x.to(dtype).double()


# ---- tolerances (ulps of the output type, absolute floor); each with the arithmetic behind it -----------------------------------------
# conv / GEMM: fp32 accumulation (relative ~1e-6 over K <= 2304) then one rounding to the output (0.5 ulp), plus the epilogue's
# fp32 adds; outputs that cancel to ~0 sit on the floor: 1 output ulp at the O(1) scale of the summed terms.
CONV_TOL = {torch.bfloat16: (1.0, EPS[torch.bfloat16]), torch.float16: (1.0, EPS[torch.float16])}
# GroupNorm apply: per-channel scale / shift folded in fp32, one fmaf + optional SiLU in fp32, one rounding: 1 ulp; the floor is one ulp at
# 1.0 for outputs near zero whose error comes from the (fp32) mean, not from their own rounding.
GN_TOL = {torch.bfloat16: (1.0, EPS[torch.bfloat16]), torch.float16: (1.0, EPS[torch.float16])}
# attention: P is rounded to the element type before the P V MFMA (one rounding of weights <= 1, relative), O rounded once: 2 ulps of O,
# floor 2 ulps at the O(1) value scale for outputs that average to ~0.
ATTN_TOL = {torch.bfloat16: (2.0, 2 * EPS[torch.bfloat16]), torch.float16: (2.0, 2 * EPS[torch.float16])}
# softmax rows: fp32 max / exp / sum, one rounding of each probability: 1 ulp; floor = 1 ulp at the smallest normal (underflowing tails)
SOFTMAX_TOL = {torch.bfloat16: (1.0, 2.0 ** -133), torch.float16: (1.0, 2.0 ** -24)}
# elementwise fp32 math (expf / erff / sinf, ~2 fp32 ulp) then one rounding to a 16-bit type: 1 ulp, floor = the smallest subnormal
# step (fp16 2^-24) so that results in the subnormal range still have to be right
ELEM_TOL = {torch.bfloat16: (1.0, 2.0 ** -133), torch.float16: (1.0, 2.0 ** -24)}
# timestep embedding: cos / sin of arguments up to 1e6 (t * 1000 * guidance), argument a = t * freq rounded in fp32 first: the fp32 rounding
# of `a` (|a| * 2^-24) is a phase error that the reference reproduces by evaluating on the same fp32 argument; 1 output ulp + floor of 1 ulp
# at 1.0 (values near a zero crossing)
TEMB_TOL = {torch.bfloat16: (1.0, EPS[torch.bfloat16]), torch.float16: (1.0, EPS[torch.float16])}
# fp32-output boundary kernels (unpack image, sample posterior): fp32 arithmetic on 16-bit inputs, __expf (a few fp32 ulp): 8 fp32 ulps,
# floor 2^-20 for outputs that cancel (mean + std * noise ~ 0)
F32_TOL = (8.0, 2.0 ** -20)


# GEMM with a GELU-tanh or GEGLU epilogue, 16-bit output: the activation is one more fp32 function of the fp32 pre-activation before the single
# rounding.  Its fp32 evaluation (tanh through exp and a reciprocal, erf by a 1.5e-7 polynomial) is wrong by ~1e-7 |x| absolute, four decades
# under a 16-bit ulp, so CONV_TOL holds unchanged.  Measured on the CPU on the inputs of tests/test_gpu_gemm_windows.py (the same formula in
# plain fp32 torch on the fp32 pre-activation, against the fp64 reference): worst 0.43x (fp16) / 0.44x (bf16) of CONV_TOL over the GELU-tanh
# and GEGLU cases -- a rounding, nothing else.  erf-GELU in place of tanh-GELU is NOT resolved at this tolerance (<= ~5e-4 absolute apart).
GEMM_ACT_TOL = dict(CONV_TOL)
# GEMM with fp32 output, as (unit per K element, unit per epilogue term).  Products of two 16-bit operands are exact in fp32, so the only errors
# are fp32 additions: any summation order of K terms is within (K - 1) 2^-24 sum_k |a_k w_k|, and the epilogue (acc * alpha, + bias, + residual:
# three roundings of partial sums no larger than the summed magnitudes) within 3 * 2^-24 (|alpha| sum|a w| + |bias| + |residual|).  `abs_bound`
# evaluates  K 2^-24 |alpha| sum|a w|  +  2^-23 (|alpha| sum|a w| + |bias| + |residual| + ...)  per element, which covers both.  Teeth: one
# dropped K element is ~ sum|a w| / K, thousands of bounds at K = 320; rounding the result through fp16 / bf16 is ~10x / ~80x the bound.
GEMM_F32_TOL = (2.0 ** -24, 2.0 ** -23)

# The VAE decoder's direct kernels (tests/test_gpu_vae_direct.py) are held to CONV_TOL / ATTN_TOL as they stand.  For the GroupNorm-fused
# convolutions the normalised activation is a rounding site that reference and kernel share (gn_silu_conv_ref rounds it once); an activation that
# the kernel's fp32 scale / shift puts on the other neighbour moves an output by |w| ulp(act), with |w| ~ 1 / sqrt(9 cin) <= 0.042: under 1/20 of
# CONV_TOL's floor per flipped activation.  Worst excess of the CPU emulations (gn_silu_conv_emul / attn512_emul below and plain fp32 convolutions:
# the kernels' arithmetic in fp32 torch) over every case of that file, fp16 / bf16, in units of the tolerance:
#   conv3x3_gn_silu 0.41 / 0.40, conv3x3_narrow 0.33 / 0.33, conv3x3_narrow_gn_silu 0.34 / 0.34, conv3x3_up2x 0.47 / 0.47, attention512 0.21 / 0.21
# (tests/test_kernel_ref_teeth.py asserts <= 1 for each and prints them).  The GPU tests print their own excess per case (`MEASURED ...`, pytest -s);
# no MI355X figures are recorded here yet.

# The 64-query attention kernels (tests/test_gpu_attention_fast.py) are held to ATTN_TOL as it stands.  They add two sites to the generic kernel's: Q is
# multiplied by scale * log2(e) and rounded AGAIN (a score moves by ~2^-mant |q| |k| scale / sqrt(3 d) per key, so a key of |k| ~ sqrt(d) costs a
# probability ~2^-mant relative: a fraction of the P rounding the tolerance already pays for -- but it grows with |k|, which is why that file's planted keys
# are at most 1.5x their query row and put the rest of the multiple into the query), and P may be as large as 2^6 before it is rounded (same RELATIVE
# rounding; fp16 / bf16 hold 2^6 without loss of precision).  Worst excess of attn64_emul (those sites in fp32 torch) against fp64 over every case of the
# file at q, k, v ~ N(0, 1), fp16 / bf16, per route at 256 CUs (tests/test_kernel_ref_teeth.py asserts <= 1 and prints them); MI355X: the worst
# "[attention excess]" line of the GPU file per route:
#   route                     emulation       MI355X (256 CUs)
#   short2<1> .. <4>          0.26 / 0.29     0.26 / 0.29
#   q64v3                     0.29 / 0.32     0.29 / 0.32
#   q64v2<64> whole           0.29 / 0.18     0.29 / 0.18
#   q64v2<64> split           0.30 / 0.31     0.30 / 0.31
#   q64v2<64> whole+split     0.28 / 0.30     0.35 / 0.32
#   ws<128>                   0.20 / 0.22     0.20 / 0.22
#   q64v2<128> split          0.19 / 0.24     0.19 / 0.24
#   ws<128>+split tail        0.29 / 0.25     0.28 / 0.27
# No family needs a tolerance of its own.  Not resolved at this tolerance: Q scaled in fp32 WITHOUT the second rounding (worst 0.23 / 0.20: closer to fp64
# than the kernels are).


# ---- references -------------------------------------------------------------------------------------------------------------------
def conv_ref(x, wt, bias=None, *, stride=1, pad=1, pad_rb=None, up=None, rowvec=None, residual=None):
    """x NHWC, wt [co, ci, kh, kw] -> NHWC fp64.  pad_rb = (right, bottom) zero columns / rows only (VAE Downsample: F.pad(x, (0, 1, 0, 1))
    then stride 2, pad 0); up = (UH, UW) nearest resize before the conv."""
    xin = x.double().permute(0, 3, 1, 2)
    if up is not None:
        xin = F.interpolate(xin, size=list(up), mode="nearest")
    if pad_rb is not None:
        xin = F.pad(xin, (0, pad_rb[0], 0, pad_rb[1]))
        pad = 0
    y = F.conv2d(xin, wt.double(), None if bias is None else bias.double(), stride=stride, padding=pad)
    if rowvec is not None:
        y = y + rowvec.double()[:, :, None, None]
    y = y.permute(0, 2, 3, 1)
    if residual is not None:
        y = y + residual.double().reshape(y.shape)
    return y


def excess_abs(got, want, bound):
    """max |got - want| / bound for a per-element absolute bound (fp64, > 0); a non-finite result is infinitely wrong"""
    got, want, bound = got.double().cpu(), want.double().cpu(), bound.double().cpu()
    return float(((got - want).abs() / bound).nan_to_num(nan=math.inf).max())


def assert_within_bound(got, want, bound, what):
    e = excess_abs(got, want, bound)
    assert e <= 1.0, f"{what}: error {e:.3g}x the derived absolute bound"


def gelu_tanh_ref(x):
    x = x.double()
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def gelu_erf_ref(x):
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gemm_ref(a0, w, *, a1=None, alpha=1.0, bias=None, rowvec=None, rows_per_image=None, act="none", gate=None, residual=None):
    """fmx_gemm_conv as a linear in fp64, the epilogue order of include/fmx.h: acc * alpha (+ bias) (+ rowvec[row // rows_per_image]) -> act ->
    (* gate[row // rows_per_image]) -> (+ residual).  a0 [M, c0], a1 [M, c1] (channel-concatenated), w [nout, c0 + c1].
    act: "none", "gelu_tanh", "gelu_erf", or "geglu" on the UN-interleaved weight (rows [value | gate]): value * gelu_erf(gate), nout / 2 columns."""
    a = a0.double() if a1 is None else torch.cat([a0.double(), a1.double()], -1)
    m = a.shape[0]
    per = rows_per_image or m
    img = torch.arange(m) // per
    v = (a @ w.double().t()) * alpha
    if bias is not None:
        v = v + bias.double()
    if rowvec is not None:
        v = v + rowvec.double()[img]
    if act == "gelu_tanh":
        v = gelu_tanh_ref(v)
    elif act == "gelu_erf":
        v = gelu_erf_ref(v)
    elif act == "geglu":
        half = v.shape[1] // 2
        v = v[:, :half] * gelu_erf_ref(v[:, half:])
    else:
        assert act == "none", act
    if gate is not None:
        v = v * gate.double()[img]
    if residual is not None:
        v = v + residual.double()
    return v


def abs_bound(a0, w, *, a1=None, alpha=1.0, terms=(), tol=GEMM_F32_TOL):
    """per-element error bound of an fp32-output GEMM (GEMM_F32_TOL): `terms` = the epilogue operands (bias, residual, ...) broadcastable to [M, nout]"""
    a = a0.double() if a1 is None else torch.cat([a0.double(), a1.double()], -1)
    mag = (a.abs() @ w.double().abs().t()) * abs(alpha)
    epi = mag.clone()
    for t in terms:
        epi = epi + t.double().abs()
    return a.shape[1] * tol[0] * mag + tol[1] * epi


def groupnorm_ref(x, gamma, beta, eps, groups=32, silu=False):
    """x NHWC (fp64 view of the rounded input) -> NHWC fp64"""
    y = F.group_norm(x.double().permute(0, 3, 1, 2), groups, gamma.double(), beta.double(), eps).permute(0, 2, 3, 1)
    return y * torch.sigmoid(y) if silu else y


def stat_sums_ref(out, n):
    """fp64 {sum, sum of squares} per (image, channel) of the stored output [n * hw, c] -> [n, c, 2]"""
    o = out.double().reshape(n, -1, out.shape[-1])
    return torch.stack([o.sum(1), (o * o).sum(1)], -1)


def attn_ref(q, k, v, scale, mask=None, causal=False):
    """q [B, H, nq, d], k / v [B, H, nk, d], mask broadcastable to [B, H, nq, nk] (additive) -> fp64 [B, H, nq, d].  causal: key j > query i
    never attends.  A row with no attending key (every score -inf) is 0, as torch's scaled_dot_product_attention returns it."""
    s = torch.einsum("bhid,bhjd->bhij", q.double(), k.double()) * scale
    if mask is not None:
        s = s + mask.double()
    if causal:
        nq, nk = s.shape[-2:]
        s = s.masked_fill(torch.ones(nq, nk, dtype=torch.bool, device=s.device).triu(1), -math.inf)
    dead = ~(s > -math.inf).any(-1, keepdim=True)
    p = torch.where(dead, torch.zeros((), dtype=s.dtype, device=s.device), s.softmax(-1))
    return torch.einsum("bhij,bhjd->bhid", p, v.double())


def softmax_ref(x):
    return x.double().softmax(-1)


def timestep_ref(t, dim, max_period=10000.0, swap=False):
    """cat([cos, sin]) of t * exp(-ln(P) k / half); the argument is formed in fp32 as the kernel does (the rounding of t * freq is part of
    the operation at t ~ 1e5, not kernel error), the cos / sin in fp64.  swap: sin first (planted bug)."""
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(half, dtype=torch.float64) / half).float()
    a = (t.float().cpu()[:, None] * freqs[None]).double()
    c, s = torch.cos(a), torch.sin(a)
    return torch.cat([s, c] if swap else [c, s], -1)


def silu_ref(x):
    x = x.double()
    return x * torch.sigmoid(x)


def act_ref(x, kind, quick_gelu_coef=1.702):
    x = x.double()
    if kind == 0:
        return x * torch.sigmoid(quick_gelu_coef * x)
    if kind == 1:
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    return x.clamp_min(0.0)


def sample_posterior_ref(moments, ld, noise, lc, scale, shift, clamp=True):
    """moments [B * npix, ld] (mean | logvar in the first 2 lc columns), noise fp32 [B, lc, h, w] -> fp64 [B, lc, h, w]"""
    b, _, hh, ww = noise.shape
    m = moments.double().reshape(b, hh * ww, ld)
    mean = m[..., :lc].permute(0, 2, 1).reshape(b, lc, hh, ww)
    logvar = m[..., lc:2 * lc].permute(0, 2, 1).reshape(b, lc, hh, ww)
    if clamp:
        logvar = logvar.clamp(-30.0, 20.0)
    return (mean + torch.exp(0.5 * logvar) * noise.double() - shift) * scale


def pack_latent_ref(z, scaling_factor, shift, ld):
    """z fp32 NCHW -> [B, H, W, ld] fp64 (columns >= C zero); the kernel divides in fp32, so the reference rounds that quotient to fp32"""
    b, c, h, w = z.shape
    out = torch.zeros(b, h, w, ld, dtype=torch.float64)
    out[..., :c] = ((z.float().cpu() / scaling_factor).double() + shift).permute(0, 2, 3, 1)
    return out


def unpack_image_ref(y, ld, c):
    return ((y.double().reshape(-1, ld)[:, :c] + 1.0) / 2.0).clamp(0.0, 1.0)


def count_nonfinite_ref(bits, high_half_ignored=False):
    """bits: int16 / uint16 view of fp16 data -> number of inf / NaN (exponent all ones).  high_half_ignored: the planted bug of a vector
    body that tests only the low 16 bits of each 32-bit word (elements at odd indices of full 8-vectors are never looked at)."""
    b = bits.to(torch.int32) & 0xFFFF
    bad = (b & 0x7C00) == 0x7C00
    if high_half_ignored:
        n = b.numel()
        full = (n // 8) * 8
        idx = torch.arange(n)
        bad = bad & ~((idx < full) & (idx % 2 == 1))
    return int(bad.sum())


def add_scaled_ref(h, c, alpha, skip_tail=False):
    """h fp16 (flat) + alpha * c -> fp64; skip_tail: the planted bug that leaves the last partial 8-vector unchanged"""
    out = h.double() + alpha * c.double()
    if skip_tail:
        full = (h.numel() // 8) * 8
        out.view(-1)[full:] = h.double().view(-1)[full:]
    return out


def add_control_nchw_ref(h, ctrl):
    """h NHWC fp16 + ctrl NCHW fp32 -> NHWC fp64"""
    return h.double() + ctrl.double().permute(0, 2, 3, 1)


def avgpool_ref(x):
    n, h, w, c = x.shape
    return x.double().reshape(n, h // 2, 2, w // 2, 2, c).mean((2, 4))


def embed_ref(ids, tok, pos):
    b, t = ids.shape
    return (tok.double()[ids.long()] + pos.double()[:t][None]).reshape(b * t, -1)


def layernorm_ref(x, gamma, beta, eps):
    return F.layer_norm(x.double(), (x.shape[-1],), gamma.double(), beta.double(), eps)


def blend_ref(a, am, b, bm):
    return a.double() * am.double() + b.double() * bm.double()


def strided_ref(src, dims, src_strides, dst_dtype):
    """the elements fmx_strided_copy4 writes, in destination index order [d0, d1, d2, d3], converted by torch: a bool source becomes
    0 / -inf; other sources convert through fp32 (the kernel's intermediate) to dst_dtype"""
    flat = src.reshape(-1).cpu()
    idx = torch.zeros(dims, dtype=torch.long)
    for i, (d, s) in enumerate(zip(dims, src_strides)):
        shape = [1, 1, 1, 1]
        shape[i] = d
        idx = idx + (torch.arange(d) * s).reshape(shape)
    v = flat[idx]
    if v.dtype == torch.bool:
        v = torch.where(v, torch.tensor(0.0), torch.tensor(-math.inf))
    return v.float().to(dst_dtype)


# ---- the VAE decoder's direct kernels (tests/test_gpu_vae_direct.py) -----------------------------------------------------------------------
def gn_silu_conv_ref(x, gamma, beta, eps, wt, bias, residual, dtype, groups=32):
    """fmx_conv3x3_gn_silu / fmx_conv3x3_narrow_gn_silu: fp64 GroupNorm + SiLU of x (NHWC), rounded ONCE to `dtype` (the staged patch holds the tensor
    groupnorm() would store: the kernel's own rounding site), zero padding of THAT tensor, fp64 3x3 convolution with wt [co, ci, 3, 3] + bias + residual"""
    act = rounded(groupnorm_ref(x, gamma, beta, eps, groups=groups, silu=True), dtype)
    return conv_ref(act, wt, bias, pad=1, residual=residual)


def up2x_ref(x, w4, bias):
    """fmx_conv3x3_up2x: the four 2 x 2 phase convolutions in fp64 on the rounded tap sums w4 [4, nout, 2 * 2 * c] the kernel receives (phase 2 py + px,
    taps (dy, dx) row-major): even output rows / columns see inputs {i - 1, i}, odd ones {i, i + 1}.  x NHWC -> [n, 2h, 2w, nout] fp64"""
    n, h, w, c = x.shape
    nout = w4.shape[1]
    xin = x.double().permute(0, 3, 1, 2)
    out = torch.zeros(n, nout, 2 * h, 2 * w, dtype=torch.float64)
    for ph in range(4):
        py, px = ph >> 1, ph & 1
        wp = w4[ph].double().view(nout, 2, 2, c).permute(0, 3, 1, 2)
        out[:, :, py::2, px::2] = F.conv2d(F.pad(xin, (1 - px, px, 1 - py, py)), wp, None if bias is None else bias.double())
    return out.permute(0, 2, 3, 1)


_UP2X_TAPS = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}     # parity -> the 3-tap indices summed into 2-tap slot 0 / 1


def fold_up2x_ref(wk, c):
    """fp64 tap sums of a [nout, 9 * c] weight (taps (ky, kx) row-major, then channels) -> [4, nout, 4 * c], written out index by index"""
    nout = wk.shape[0]
    w = wk.double().reshape(nout, 3, 3, c)
    out = torch.zeros(4, nout, 2, 2, c, dtype=torch.float64)
    for py in (0, 1):
        for px in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    for ky in _UP2X_TAPS[py][dy]:
                        for kx in _UP2X_TAPS[px][dx]:
                            out[2 * py + px, :, dy, dx] += w[:, ky, kx]
    return out.reshape(4, nout, 4 * c)


def round_to(want, dtype):
    """fp64 values rounded to nearest-even in `dtype`, evaluated in fp64 (no intermediate fp32 rounding) -> (rounded fp64, distance of `want` from the
    nearest rounding tie relative to |want|; inf at 0)"""
    u = ulp(want, dtype)
    t = want.double() / u
    tie = ((t - torch.floor(t)) - 0.5).abs() * u / want.double().abs().clamp_min(1e-300)
    return torch.round(t) * u, torch.where(want == 0, torch.full_like(tie, math.inf), tie)


def gn_fold_emul(x, gamma, beta, eps, groups=32):
    """the {scale, shift} table as csrc/fmx_norm.hip folds it: fp32 per-channel {sum, sum of squares}, mean and variance of a group in double, mean and
    rstd in fp32, scale = rstd * gamma, shift = beta - mean * scale in fp32.  x NHWC -> (scale, shift) fp32 [n, c]"""
    n, c = x.shape[0], x.shape[-1]
    xf = x.float().reshape(n, -1, c)
    cnt = float(xf.shape[1] * (c // groups))
    s = xf.sum(1).double().view(n, groups, -1).sum(-1) / cnt
    q = (xf * xf).sum(1).double().view(n, groups, -1).sum(-1) / cnt
    mean = s.float()
    rstd = torch.rsqrt((q - s * s).clamp_min(0.0).float() + eps)
    sc = rstd.repeat_interleave(c // groups, 1) * gamma.float()
    return sc, beta.float() - mean.repeat_interleave(c // groups, 1) * sc


def gn_silu_conv_emul(x, gamma, beta, eps, wt, bias, residual, dtype, groups=32, plant=None):
    """the fused kernels' arithmetic in fp32 torch: table from gn_fold_emul, one multiply-add + SiLU in fp32, rounded to `dtype`, zeros outside the image,
    fp32 convolution + bias + residual, one rounding.  plant: None, or one bug -- "pad_before_norm" (the halo holds silu(shift[c]): x padded before the
    norm), "table_of_image0", "table_one_chunk_on" (channels c use the table of c + 64), "kykx" (taps transposed)."""
    n, h, w, c = x.shape
    sc, sh = gn_fold_emul(x, gamma, beta, eps, groups)
    if plant == "table_of_image0":
        sc, sh = sc[:1].expand(n, c), sh[:1].expand(n, c)
    if plant == "table_one_chunk_on":
        idx = (torch.arange(c) + 64) % c
        sc, sh = sc[:, idx], sh[:, idx]
    silu = lambda y: y * torch.sigmoid(y)  # noqa: E731
    act = silu(x.float() * sc[:, None, None, :] + sh[:, None, None, :]).to(dtype).float().permute(0, 3, 1, 2)
    act = F.pad(act, (1, 1, 1, 1))
    if plant == "pad_before_norm":
        halo = silu(sh).to(dtype).float()[:, :, None, None].expand(n, c, h + 2, w + 2).clone()
        halo[:, :, 1:-1, 1:-1] = act[:, :, 1:-1, 1:-1]
        act = halo
    wf = wt.float().transpose(2, 3) if plant == "kykx" else wt.float()
    y = F.conv2d(act, wf, None if bias is None else bias.float()).permute(0, 2, 3, 1)
    if residual is not None:
        y = y + residual.float().reshape(y.shape)
    return y.to(dtype)


def attn512_emul(q, k, v, nk, scale, dtype, plant=None):
    """fmx_attention_single_head512 in fp32 torch: Q pre-scaled by scale * log2(e) and rounded to `dtype`, an online softmax in the log2 domain over 32-key
    steps, P rounded to `dtype` before P V, one rounding of O.  q [b, nq, 512]; k, v [b, >= nk, 512] INCLUDING whatever the buffers hold behind key nk.
    plant: None, "pad_keys_attend" (keys >= nk of the last step not masked), "no_rescale" (the accumulator keeps its scale when the maximum rises)"""
    b, nq, c = q.shape
    steps = -(-nk // 32)
    pad = steps * 32 - k.shape[1]
    if pad > 0:
        k, v = F.pad(k, (0, 0, 0, pad)), F.pad(v, (0, 0, 0, pad))
    qs = (q.float() * (scale * 1.44269504088896340736)).to(dtype).float()
    m = torch.full((b, nq), -math.inf)
    l, o = torch.zeros(b, nq), torch.zeros(b, nq, c)
    for kt in range(steps):
        sl = slice(kt * 32, kt * 32 + 32)
        s = qs @ k[:, sl].float().transpose(1, 2)
        if plant != "pad_keys_attend":
            s[:, :, max(0, nk - kt * 32):] = -math.inf
        m_new = torch.maximum(m, s.max(-1).values)
        alpha = torch.exp2(m - m_new)
        p = torch.exp2(s - m_new[..., None])
        l = l * alpha + p.sum(-1)
        if plant != "no_rescale":
            o = o * alpha[..., None]
        o = o + p.to(dtype).float() @ v[:, sl].float()
        m = m_new
    return (o / l[..., None]).to(dtype)


# ---- the 64-query attention kernels (tests/test_gpu_attention_fast.py) ----------------------------------------------------------------------------
def attn_route(b, h, nq, nk, dpad, cus):
    """the kernel(s) fmx_attention_f16 / _bf16 launch for an unmasked, non-causal problem: csrc/fmx_attention.hip launch_attn_v2 restated (default knobs,
    K / V^T / Q spans below 2 GB).  -> "generic", "short2<NB>", "q64v3", "q64v2<64> whole", "q64v2<64> split", "q64v2<64> whole+split", "ws<128>",
    "q64v2<128> split" or "ws<128>+split tail" (two launches)"""
    if dpad not in (64, 128) or nq < 256:
        return "generic"
    grid = -(-nq // 256) * h * b
    slots = (2 if dpad == 64 else 1) * cus
    ntiles = -(-nk // 64)
    rem = grid % slots
    do_split = rem > 0 and 8 * rem <= 3 * slots and ntiles >= 4 and ntiles % 2 == 0
    if dpad == 128:
        if not do_split:
            return "ws<128>"
        return "ws<128>+split tail" if grid > slots else "q64v2<128> split"
    if nk <= 128:
        return f"short2<{-(-nk // 32)}>"
    if not do_split:
        return "q64v3" if ntiles <= 4 else "q64v2<64> whole"
    return "q64v2<64> whole+split" if grid > rem else "q64v2<64> split"


ATTN_STEP = {"short2": 0, "q64v3": 32, "ws<128>": 32, "q64v2": 64}     # keys per running-maximum check of a kernel family (0: one pass over <= 128 keys)


def attn_route_emul(route):
    """-> (step, split) arguments of attn64_emul for a route name of attn_route; the two-launch route is emulated as its key-split tail (the rows it
    covers) -- the ws rows of that launch have the rounding sites of "ws<128>", which the other cases of that route cover"""
    split = route.endswith("split") or route.endswith("split tail")
    for fam, step in ATTN_STEP.items():
        if route.startswith(fam) and not split:
            return step, False
    return 64, split


_LOG2E = 1.44269504088896340736
ATTN_THR = 6.0      # log2 units a sub-tile's scores may exceed the running maximum by before it moves (csrc/fmx_attention.hip THR)


def _attn64_range(qs, k, v, nk, k0, k1, step, dtype, plant, upper):
    """keys [k0, k1) in steps of `step`: -> (m, l, o) in fp32, m in the log2 domain.  The first step sets the maximum exactly; a later one moves it only
    if any query of its 64-query wave sees a score more than 2^THR above it, and then every query of that wave moves to max(own, old)."""
    b, h, nq, d = qs.shape
    m, l, o = torch.zeros(b, h, nq), torch.zeros(b, h, nq), torch.zeros(b, h, nq, d)
    for s0 in range(k0, k1, step):
        sl = slice(s0, s0 + step)
        s = qs @ k[:, :, sl].float().transpose(-1, -2)
        masked = plant != "pad_keys_attend" and not (plant == "split_tail_unmasked" and upper)
        if masked and s0 + step > nk:
            s[..., max(0, nk - s0):] = -math.inf
        mh = (-m).to(dtype).float()                       # "- maximum" rides through the matrix pipe as a high and a low part in the element type
        s = s + (mh + (-m - mh).to(dtype).float())[..., None]
        mx = s.max(-1).values
        if s0 == k0:
            delta, alpha = mx, torch.ones_like(mx)
        else:
            over = F.pad(mx > ATTN_THR, (0, -nq % 64)).view(b, h, -1, 64).any(-1, keepdim=True).expand(-1, -1, -1, 64).reshape(b, h, -1)[..., :nq]
            if plant == "never_move":
                over = torch.zeros_like(over)
            delta = torch.where(over, mx.clamp_min(0.0), torch.zeros_like(mx))
            alpha = torch.exp2(-delta)
        m = m + delta
        l = l * alpha
        if plant != "no_rescale":
            o = o * alpha[..., None]
        p = torch.exp2(s - delta[..., None])
        l = l + p.sum(-1)
        o = o + p.to(dtype).float() @ v[:, :, sl].float()
    return m, l, o


def attn64_emul(q, k, v, nk, scale, dtype, step=64, split=False, plant=None):
    """the 64-query kernels' documented rounding sites in fp32 torch (csrc/fmx_attention.hip: attn_short2 / attn_q64v3 / attn_q64v2 / attn_ws): Q pre-scaled
    by scale * log2(e) and rounded to `dtype`; an online softmax in the log2 domain whose maximum is checked every `step` keys (64: q64v2, 32: q64v3 and ws,
    0: one exact pass, short2) and moved only past 2^6; P rounded to `dtype` before P V while the row sum adds the unrounded fp32 P; with `split` the two
    halves of an even number of 64-key tiles run on their own and merge (m, l, O) with exp2(m_half - m) weights; one rounding of O.
    q [B, H, nq, d]; k, v [B, H, >= nk, d] INCLUDING whatever the buffers hold behind key nk.  plant: None or one bug -- "pad_keys_attend" (keys >= nk not
    masked), "no_rescale" (O keeps its scale when the maximum moves), "never_move" (the threshold rule never moves the maximum), "merge_unweighted" (the halves
    added without their weights), "split_tail_unmasked" (the upper half forgets the ragged tail), "scale_after_rounding" (Q scaled in fp32, not rounded again)"""
    ntiles = -(-nk // 64)
    pad = ntiles * 64 - k.shape[2]
    if pad > 0:
        k, v = F.pad(k, (0, 0, 0, pad)), F.pad(v, (0, 0, 0, pad))
    qs = q.float() * (scale * _LOG2E)
    if plant != "scale_after_rounding":
        qs = qs.to(dtype).float()
    if step == 0:
        step = -(-nk // 32) * 32
    if split:
        assert ntiles >= 4 and ntiles % 2 == 0
        half = ntiles // 2 * 64
        m0, l0, o0 = _attn64_range(qs, k, v, nk, 0, half, step, dtype, plant, False)
        m1, l1, o1 = _attn64_range(qs, k, v, nk, half, 2 * half, step, dtype, plant, True)
        m = torch.maximum(m0, m1)
        f0, f1 = torch.exp2(m0 - m), torch.exp2(m1 - m)
        if plant == "merge_unweighted":
            f0, f1 = torch.ones_like(f0), torch.ones_like(f1)
        l, o = l0 * f0 + l1 * f1, o0 * f0[..., None] + o1 * f1[..., None]
    else:
        _, l, o = _attn64_range(qs, k, v, nk, 0, -(-nk // step) * step, step, dtype, plant, False)
    return (o * (1.0 / l)[..., None]).to(dtype)


# ---- the sampler-step kernels (tests/test_gpu_sampler_kernels.py) ---------------------------------------------------------------------------------
# fmx_unet_pack_input, fmx_im2col3x3_smallc, fmx_cfg_combine, fmx_sampler_euler_step / _lincomb3 / _lincomb / _error_norm, fmx_philox_randn
# (csrc/fmx_elementwise.hip).  Scalars that the wrappers hand over as C `float` (coefficients, sigma, sigma_next, noise_scale, cond_scale, sigma_data,
# atol, rtol) are part of the operation: every reference below takes them through f32() first, as timestep_ref rounds its argument.
#
# fp32 outputs: per-element absolute bound  R * 2^-24 * sum|terms|  (assert_within_bound), sum|terms| = the magnitudes of the terms the fp64 reference
# adds for that element, R = the number of fp32 roundings that the value of one such term passes through on its way to the stored result, counted on
# the longest chain of the kernel's source INCLUDING the roundings of the side inputs that are formed in the kernel and multiply into the term (a
# rounding of relative size 2^-24 of a factor is one of the term).  Every rounding is at most 2^-24 of a partial result that is no larger than the
# summed magnitudes, fp32 `/` and sqrtf are correctly rounded in this build (csrc/Makefile: -O3, no fast-math), and FMA contraction only removes
# roundings.  None of the counts below comes from a GPU run.
U32 = 2.0 ** -24
#   fmx_sampler_lincomb, N terms, accumulated left to right:  coef0 * src0 (1), then per further term one product and one add.  The first term passes
#     through its product and N - 1 adds: R = N (n_terms).
#   fmx_sampler_lincomb3:  bc * d0 (1), + cc * d1 (2), a * x + that (3): R = 3 (2 without old_denoised; the test uses 3 throughout).
LINCOMB3_R = 3
#   fmx_sampler_euler_step:  the term d * dt passes through  x - den (1), / sigma (2), * dt (3) where dt = sigma_next - sigma is itself rounded in
#     the kernel (4), x + that (5), + noise * noise_scale (6): R = 6.  terms: |x|, |(x - den) / sigma * dt|, |noise * noise_scale|.
EULER_R = 6
#   fmx_cfg_combine, v_prediction / edm with two halves (the longest formula of the kernel):  the term B * out passes through  s * s (1) and
#     sigma_data * sigma_data (2), their sum v (3), sqrtf(v) (4), s * sigma_data (5), the quotient cb (6), out * cb (7), x * ca + that (8): 8 roundings
#     up to the stored cond_pred / uncond_pred, then dc - du (9), * cond_scale (10), du + that (11).  The term A * x passes through fewer (s * s, sigma_data^2,
#     v, the quotient ca, x * ca, the sum: 6 and the same last 3), epsilon prediction through 2 and 5 (out * s, x - that; the same last 3).  One R per kernel:
#     denoised R = 11, cond_pred / uncond_pred R = 8.  terms of denoised (reps == 2): |A x| + |B eu|, |A x| + |B ec|, |cond_scale (dc - du)|; with one
#     half: |A x| + |B ec| and |cond_scale dc|.
#     What the count does NOT model: a rounding made in du (dc) before the subtraction reaches denoised multiplied by 1 - cond_scale (cond_scale).  At
#     cond_scale 7 and a small sigma (x dominates, dc ~ du ~ x, the guidance term is small) the un-fused worst case is (2 per half) * (6 + 7) + the
#     shared ca / cb roundings and the final add ~ 30 * 2^-24 |A x| against the bound's 22 * 2^-24 |A x|: reachable only if every rounding of both
#     halves is a full half-ulp of the adverse sign at the top of x's binade.  The figures below are the measure of how far real data stays from that.
CFG_R, CFG_PRED_R = 11, 8
#   fmx_unet_pack_input: fp16 output, a few fp32 operations (s * s + sd^2, rsqrtf, one product) and one rounding: ELEM_TOL[float16] as it stands.
#   fmx_im2col3x3_smallc: a 16-bit word shuffle: bit equality.
#   fmx_sampler_error_norm: a sum of non-negative fp32 terms, so the bound is relative.  Per element  rtol * max (1) in delta, lo - hi (2), / delta (3):
#     r carries 3, r * r twice that and its own rounding = 7.  Summation depth from the source: per-thread strided sums of ceil(n / 65536) terms (256
#     blocks x 256 threads), 6 shuffle levels, 4 waves, 256 partials added in sequence.  (7 + depth) * 2^-24 on the sum of squares, half of it on the
#     root: error_norm_rel_bound(n).  (Not in the formula, which is kept as stated: the four roundings behind the sum -- 1 / n, its root, the root of the
#     sum, their product -- which are not halved; three of the counted adds are 0 + x and exact, so the worst case is 2.5 * 2^-24 above the formula, 2% of
#     it at the smallest n.)
ERRNORM_TERM_R = 7
#   fmx_philox_randn: the four raw words bit-exact against oracle/rng.py; the normals within atol 2e-6 (the device logf / sinf), as
#     tests/test_gpu_kernels.py::test_philox_bit_exact has it.  The GPU file prints the figure per case; it is not tightened.
PHILOX_ATOL = 2e-6
#
# Worst excess (units of the bound / tolerance) over every case of tests/test_gpu_sampler_kernels.py: the emulations below (the kernels' formulas in
# plain fp32 torch, no FMA; tests/test_kernel_ref_teeth.py asserts <= 1 and prints them) and the `MEASURED` lines of the GPU file on MI355X:
#   kernel                 emulation    MI355X
#   unet_pack_input        0.500        0.500
#   im2col3x3_smallc       bit-equal    bit-equal
#   cfg_combine denoised   0.541        0.541
#   cfg_combine preds      0.274        0.274
#   euler_step             0.399        0.399
#   lincomb3               0.791        0.705
#   lincomb                0.968        0.968
#   error_norm             0.042        0.042
#   philox_randn normals   (host libm)  0.679 (1.36e-6 absolute, n = 16384)
# (lincomb's 0.968 is the single product of a one-term case, n = 4099, where the bound is that one rounding: nothing to give.  Several MI355X figures
# equal the emulation's to three digits although the kernels' code does contract (v_fma / v_fmac in the ISA): fusing a product into an add changes the
# final fp32 value of few elements, and not of the worst ones here, whose error comes from the earlier roundings and the last one.)


def f32(v):
    """a host scalar as the C `float` argument the kernel receives"""
    return float(np.float32(v))


def _taps(xc, transposed=False):
    """xc [b, c, h, w] -> [b, h, w, 9, c]: the nine zero-padded 3x3 neighbours of every pixel, tap = ky * 3 + kx (transposed: kx * 3 + ky, a planted bug)"""
    b, c, h, w = xc.shape
    xp = F.pad(xc, (1, 1, 1, 1))
    taps = [xp[:, :, ky:ky + h, kx:kx + w] for ky in range(3) for kx in range(3)]
    if transposed:
        taps = [taps[kx * 3 + ky] for ky in range(3) for kx in range(3)]
    return torch.stack(taps, 1).permute(0, 3, 4, 1, 2)


def _pack_rows(t, reps, ch_major=False):
    """[b, h, w, 9, c] -> [reps * b * h * w, 64]: column tap * c + ch (ch_major: ch * 9 + tap, a planted bug), zeros from 9 c on, `reps` stacked copies"""
    b, h, w, _, c = t.shape
    if ch_major:
        t = t.transpose(3, 4)
    out = torch.zeros(b * h * w, 64, dtype=t.dtype)
    out[:, :9 * c] = t.reshape(b * h * w, 9 * c)
    return out.repeat(reps, 1)


def pack_input_ref(x, sigma, sigma_data, reps):
    """fmx_unet_pack_input: x fp32 [b, c, h, w], sigma fp32 [b] -> fp64 [reps * b * h * w, 64] of x / sqrt(sigma^2 + sigma_data^2)"""
    b = x.shape[0]
    xc = x.double() / torch.sqrt(sigma.double() ** 2 + f32(sigma_data) ** 2).view(b, 1, 1, 1)
    return _pack_rows(_taps(xc), reps)


def pack_input_emul(x, sigma, sigma_data, reps, plant=None):
    """the kernel's arithmetic in fp32 torch (1 / sqrt for rsqrtf), rounded once to fp16.  plant: None, "ch_major" (column ch * 9 + tap), "kykx" (taps
    transposed), "sigma_of_image0", "sd2_dropped" (x / sqrt(sigma^2): the term gone), "sd_not_squared" (sigma^2 + sigma_data: invisible at sigma_data 1)"""
    b = x.shape[0]
    s = sigma.float()
    if plant == "sigma_of_image0":
        s = s[:1].expand(b)
    sd = torch.tensor(f32(sigma_data), dtype=torch.float32)
    sd2 = {"sd2_dropped": torch.zeros(()), "sd_not_squared": sd}.get(plant, sd * sd)
    xc = x.float() * (1.0 / torch.sqrt(s * s + sd2)).view(b, 1, 1, 1)
    return _pack_rows(_taps(xc, transposed=plant == "kykx"), reps, ch_major=plant == "ch_major").half()


def im2col_smallc_ref(x, c):
    """fmx_im2col3x3_smallc: x 16-bit [n, h, w, ldx] -> the same type [n * h * w, 64], moved as 16-bit words (column tap * c + ch of the first c channels)"""
    words = x.view(torch.int16)[..., :c].permute(0, 3, 1, 2)
    return _pack_rows(_taps(words), 1).view(x.dtype)


def _cfg_coefs(sigma, ptype, sigma_data, dtype, plant=None):
    """A, B [b, 1, 1, 1] of calculate_denoised in `dtype`, in the kernel's order of operations"""
    s = sigma.to(dtype).view(-1, 1, 1, 1)
    if ptype == "epsilon":
        return torch.ones_like(s), -s
    sd = torch.tensor(f32(sigma_data), dtype=dtype)
    v = s * s + sd * sd
    ca = (torch.ones((), dtype=dtype) if plant == "no_sd2_in_a" else sd * sd) / v
    sign = 1.0 if (ptype == "edm") != (plant == "edm_sign") else -1.0
    return ca, sign * s * sd / torch.sqrt(v)


def _cfg_eps(eps, b, c, reps, plant=None):
    """eps fp16 [reps * b, h, w, ld] -> (eu, ec) [b, c, h, w] (eu None with one half).  plant "ld_as_c": rows stepped c apart; "eps_nchw": the buffer
    read as [reps * b, c, h, w]; "halves_swapped" """
    n, h, w, ld = eps.shape
    if plant == "ld_as_c":
        e = eps.reshape(-1)[:n * h * w * c].view(n, h, w, c).permute(0, 3, 1, 2)
    elif plant == "eps_nchw":
        e = eps.reshape(-1)[:n * h * w * c].view(n, c, h, w)
    else:
        e = eps[..., :c].permute(0, 3, 1, 2)
    if reps == 1:
        return None, e[:b]
    return (e[b:], e[:b]) if plant == "halves_swapped" else (e[:b], e[b:])


def cfg_combine_ref(eps, x, sigma, reps, cond_scale, ptype="epsilon", sigma_data=1.0):
    """fmx_cfg_combine in fp64: eps fp16 [reps * b, h, w, ld_eps] ([uncond ; cond]), x fp32 [b, c, h, w], sigma fp32 [b] ->
    (denoised, cond_pred, uncond_pred, bound of denoised, bound of cond_pred, bound of uncond_pred); uncond_pred is 0 with one half"""
    b, c = x.shape[:2]
    cs = f32(cond_scale)
    ca, cb = _cfg_coefs(sigma, ptype, sigma_data, torch.float64)
    eu, ec = _cfg_eps(eps.double(), b, c, reps)
    ax = ca * x.double()
    dc = ax + cb * ec
    tc = ax.abs() + (cb * ec).abs()
    if reps == 1:
        den, du, tu = cs * dc, torch.zeros_like(dc), torch.zeros_like(dc)
        mag = tc + den.abs()
    else:
        du = ax + cb * eu
        tu = ax.abs() + (cb * eu).abs()
        den = du + cs * (dc - du)
        mag = tu + tc + (cs * (dc - du)).abs()
    return den, dc, du, CFG_R * U32 * mag, CFG_PRED_R * U32 * tc, CFG_PRED_R * U32 * tu


def cfg_combine_emul(eps, x, sigma, reps, cond_scale, ptype="epsilon", sigma_data=1.0, plant=None):
    """the kernel's formula in fp32 torch -> (denoised, cond_pred, uncond_pred).  plant: None, "halves_swapped", "preds_swapped" (cond_pred and uncond_pred
    exchanged), "edm_sign" (the other sign of B on v_prediction / edm), "no_sd2_in_a" (A = 1 / (sigma^2 + sd^2): has teeth only at sigma_data != 1),
    "ld_as_c", "eps_nchw" """
    b, c = x.shape[:2]
    cs = torch.tensor(f32(cond_scale), dtype=torch.float32)
    ca, cb = _cfg_coefs(sigma, ptype, sigma_data, torch.float32, plant)
    eu, ec = _cfg_eps(eps, b, c, reps, plant)
    xv = x.float()
    half = (lambda e: xv - e.float() * sigma.float().view(-1, 1, 1, 1)) if ptype == "epsilon" else (lambda e: xv * ca + e.float() * cb)
    dc = half(ec)
    if reps == 1:
        du = torch.zeros_like(dc)
        den = 0.0 + (dc - 0.0) * cs
    else:
        du = half(eu)
        den = du + (dc - du) * cs
    return (den, du, dc) if plant == "preds_swapped" else (den, dc, du)


def euler_step_ref(x, den, sigma, sigma_next, noise=None, noise_scale=0.0):
    """fmx_sampler_euler_step in fp64 -> (x_out, bound)"""
    step = (x.double() - den.double()) / f32(sigma) * (f32(sigma_next) - f32(sigma))
    out, mag = x.double() + step, x.double().abs() + step.abs()
    if noise is not None:
        out, mag = out + noise.double() * f32(noise_scale), mag + (noise.double() * f32(noise_scale)).abs()
    return out, EULER_R * U32 * mag


def euler_step_emul(x, den, sigma, sigma_next, noise=None, noise_scale=0.0, plant=None):
    """plant: None, "dt_sign" (sigma - sigma_next), "noise_before_scale" (the noise joins d before the product with dt)"""
    sg, sn = torch.tensor(f32(sigma), dtype=torch.float32), torch.tensor(f32(sigma_next), dtype=torch.float32)
    dt = sg - sn if plant == "dt_sign" else sn - sg
    d = (x.float() - den.float()) / sg
    if noise is not None and plant == "noise_before_scale":
        return x.float() + (d + noise.float() * f32(noise_scale)) * dt
    r = x.float() + d * dt
    return r if noise is None else r + noise.float() * f32(noise_scale)


def lincomb_ref(srcs, coefs):
    """fmx_sampler_lincomb in fp64 -> (sum_k coefs[k] * srcs[k], bound with R = n_terms)"""
    terms = [f32(c) * t.double() for c, t in zip(coefs, srcs)]
    return sum(terms), len(terms) * U32 * sum(t.abs() for t in terms)


def lincomb_emul(srcs, coefs, plant=None, out_before=None):
    """left to right in fp32.  plant: None, "tail_unwritten" (the n % 4 elements behind the last full float4 keep what the destination held: out_before),
    "coef_shift" (coefficient k applied to source k + 1, cyclically)"""
    if plant == "coef_shift":
        srcs = list(srcs[1:]) + list(srcs[:1])
    r = f32(coefs[0]) * srcs[0].float()
    for c, t in zip(coefs[1:], srcs[1:]):
        r = r + f32(c) * t.float()
    if plant == "tail_unwritten":
        full = (r.numel() // 4) * 4
        r = r.clone()
        r.view(-1)[full:] = out_before.float().view(-1)[full:]
    return r


def lincomb3_ref(x, d0, d1, a, b, c):
    """fmx_sampler_lincomb3 in fp64 -> (a x + b d0 + c d1, bound); d1 None: two terms"""
    terms = [f32(a) * x.double(), f32(b) * d0.double()] + ([] if d1 is None else [f32(c) * d1.double()])
    return sum(terms), LINCOMB3_R * U32 * sum(t.abs() for t in terms)


def lincomb3_emul(x, d0, d1, a, b, c):
    if d1 is None:
        return f32(a) * x.float() + f32(b) * d0.float()
    return f32(a) * x.float() + (f32(b) * d0.float() + f32(c) * d1.float())


def error_norm_rel_bound(n):
    depth = -(-n // 65536) + 6 + 4 + 256
    return 0.5 * (ERRNORM_TERM_R + depth) * U32


def error_norm_ref(x_low, x_high, x_prev, atol, rtol):
    """fmx_sampler_error_norm in fp64 -> python float; delta is formed from the fp32 atol / rtol"""
    lo = x_low.double().reshape(-1)
    delta = torch.clamp_min(f32(rtol) * torch.maximum(lo.abs(), x_prev.double().reshape(-1).abs()), f32(atol))
    return float((((lo - x_high.double().reshape(-1)) / delta) ** 2).sum().sqrt() / math.sqrt(lo.numel()))


def error_norm_emul(x_low, x_high, x_prev, atol, rtol, plant=None):
    """the two kernels in fp32 torch IN THEIR SUMMATION ORDER (256 blocks of 256 threads, element i on thread i % 65536; strided per-thread sums, the
    shuffle tree of a 64-lane wave, 4 waves and then 256 partials in sequence) -> python float.  plant: None, "prev_ignored" (|x_prev| not in the max),
    "last_block_dropped" (the n % 256 elements behind the last full block of 256 never summed), "div_n" (the root divided by n, not sqrt(n))"""
    lo, hi, pv = (t.float().reshape(-1) for t in (x_low, x_high, x_prev))
    n = lo.numel()
    big = lo.abs() if plant == "prev_ignored" else torch.maximum(lo.abs(), pv.abs())
    delta = torch.clamp_min(f32(rtol) * big, f32(atol))
    r = (lo - hi) / delta
    sq = r * r
    if plant == "last_block_dropped":
        sq = sq[:(n // 256) * 256]
    k = -(-max(sq.numel(), 1) // 65536)
    sq = F.pad(sq, (0, k * 65536 - sq.numel())).view(k, 256, 4, 64)
    acc = torch.zeros(256, 4, 64)
    for i in range(k):
        acc = acc + sq[i]
    for off in (32, 16, 8, 4, 2, 1):                    # lane l adds lane l + off; lanes past the end read their own value, lane 0 never does
        acc = acc + torch.cat([acc[..., off:], acc[..., -off:]], -1)
    waves = acc[..., 0]
    part = torch.zeros(256)
    for w in range(4):
        part = part + waves[:, w]
    t = torch.zeros(())
    for blk in range(256):
        t = t + part[blk]
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)
    return float(torch.sqrt(t) * inv) if plant == "div_n" else float(torch.sqrt(t) * torch.sqrt(inv))


def philox_raw_ref(seed, offset, n, plant=None):
    """the four Philox4x32-10 words of elements 0 .. n - 1 (oracle/rng.py: key = the seed's two words, counter = (offset, 0, index, 0)) -> uint32 [n, 4].
    plant: None, "seed_hi_ignored" (key word 1 = 0), "offset_in_word1" (counter = (0, offset, index, 0))"""
    from oracle.rng import philox4x32_10
    idx, z = np.arange(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    off = np.full(n, offset & 0xFFFFFFFF, dtype=np.uint32)
    k0 = np.full(n, seed & 0xFFFFFFFF, dtype=np.uint32)
    k1 = z if plant == "seed_hi_ignored" else np.full(n, (seed >> 32) & 0xFFFFFFFF, dtype=np.uint32)
    c = (z, off, idx, z) if plant == "offset_in_word1" else (off, z, idx, z)
    return np.stack(philox4x32_10(*c, k0, k1), 1)


# ---- the GroupNorm statistics chain (tests/test_gpu_groupnorm_routes.py) --------------------------------------------------------------------------
# Producer records (fmx_gemm_conv_stats from every tile's epilogue or the pass behind the GEMM), the stand-alone pass (fmx_groupnorm_stats) and both folds
# of fmx_groupnorm_apply.  Records are held PER CHUNK to the statistics tolerance the other files use on sums over chunks (rtol 2e-5, atol 2e-3:
# test_gpu_vae_direct.STAT_TOL, unchanged): a chunk is at most 512 fp32 additions of values |x| ~ 1, relative ~1e-6.  GroupNorm outputs: GN_TOL as it stands.
#
# The {scale, shift} table of the separate fold (gn_finalize_kernel) is the only fp32 result of the chain that a test can read.  Its unit: relative to
# |scale| for scale = rstd gamma, and to |beta| + |mean scale| (the summed magnitudes) for shift = beta - mean scale.  The tolerance is not derived but
# MEASURED, as the worst such error of gn_fold_emul2 (fp32 chunk sums, the fold in double, mean / rstd / scale / shift in fp32: the kernel's formula in plain
# torch) against fp64 over every separate-fold case of the GPU file in both element types, on the CPU:  1.96e-7 (fp16) / 1.86e-7 (bf16), recorded as 2.0e-7
# (a handful of fp32 roundings of 6e-8 each between the variance and the shift).  Four times that is allowed; tests/test_kernel_ref_teeth.py asserts that the
# emulation stays at or below the recorded figure.
GN_TABLE_EMUL = 2.0e-7
GN_TABLE_TOL = 4 * GN_TABLE_EMUL
#
# Worst excess (units of the tolerance) per part: the emulations below on the GPU file's inputs (tests/test_kernel_ref_teeth.py asserts <= 1 and prints
# them) and the worst `MEASURED` line of the GPU file on MI355X, fp16 / bf16:
#   part                                   emulation        MI355X
#   producer output vs CONV_TOL (1, 2)     -                0.400 / 0.400
#   producer records per chunk (1, 2)      0.010 / 0.010    0.009 / 0.007   (split-K: 0.006 / 0.006)
#   stand-alone pass per chunk (3)         0.013 / 0.009    0.040 / 0.048
#   GroupNorm output, fused fold (4)       0.390 / 0.381    0.390 / 0.381
#   GroupNorm output, separate fold (4)    0.400 / 0.400    0.400 / 0.400
#   scale / shift table (4)                0.245 / 0.233    0.213 / 0.231
# (The statistics tolerance is two decades above what either the emulation or the kernels need: what it resolves is a record that is wrong -- a missing or
# misplaced chunk is thousands of tolerances -- not the summation order.  The stand-alone pass adds its pixels in sequence where torch adds pairwise: 4x the
# emulation's error, still 1/20 of the tolerance.)  Of the 655 cases of the GPU file 30 are skipped, each a dispatcher refusal of a forced tile that the test
# first reproduces by its FMX_REQUIRE text: tile id 10 (no output statistics: 26 cases) and tile id 9 with upsample-on-load (4 cases).


def stat_excess(got, want, rtol, atol):
    """torch.testing.assert_close's criterion as a figure: max |got - want| / (atol + rtol |want|), <= 1 passes; a non-finite record is infinitely wrong"""
    got, want = got.double().cpu(), want.double().cpu()
    return float(((got - want).abs() / (atol + rtol * want.abs())).nan_to_num(nan=math.inf).max())


def _chunked(o, nchunks):
    """[n, hw, c] -> [n, nchunks, per, c], per = ceil(hw / nchunks) consecutive pixels per chunk, zero rows behind pixel hw (chunks past the image are empty)"""
    n, hw, c = o.shape
    per = -(-hw // nchunks)
    return F.pad(o, (0, 0, 0, nchunks * per - hw)).view(n, nchunks, per, c)


def chunk_sums_ref(out, n, nchunks):
    """fp64 {sum, sum of squares} per (image, chunk, channel) of the stored tensor [n * hw, c] (or [n, hw, c]) -> [n, nchunks, c, 2].  Chunk k of an image is
    pixels [k per, (k + 1) per), per = ceil(hw / nchunks): the rows of the k-th 128 / 256 / 512-row tile of the image for the GEMM epilogues (hw = nchunks *
    rows), the block's pixels for the statistics pass (csrc/fmx_norm.hip gn_stats_kernel); a chunk that starts behind the image is {0, 0}"""
    o = _chunked(out.double().reshape(n, -1, out.shape[-1]), nchunks)
    return torch.stack([o.sum(2), (o * o).sum(2)], -1)


def chunk_sums_emul(out, n, nchunks, plant=None):
    """the same records from fp32 sums (torch's summation order, not the kernels').  plant: None or one bug -- "last_chunk_dropped" (the last chunk of every image
    never written: a zeroed buffer keeps {0, 0}), "next_image_slot" (image i's records in image i + 1's slots, cyclically), "empty_chunk_stale" (chunks behind
    the image are not written and keep an earlier launch's record, here chunk 0's)"""
    o = _chunked(out.float().reshape(n, -1, out.shape[-1]), nchunks)
    hw = out.numel() // (n * out.shape[-1])
    p = torch.stack([o.sum(2), (o * o).sum(2)], -1)
    if plant == "last_chunk_dropped":
        p[:, -1] = 0.0
    elif plant == "next_image_slot":
        p = p.roll(1, 0)
    elif plant == "empty_chunk_stale":
        first_empty = -(-hw // -(-hw // nchunks))
        p[:, first_empty:] = p[:, :1]
    else:
        assert plant is None, plant
    return p


def gn_table_ref(x, gamma, beta, eps, groups):
    """fp64 {scale, shift} = {rstd gamma, beta - mean rstd gamma} per (image, channel) of x [n, hw, C] -> (table [n, C, 2], magnitudes [n, C, 2] =
    {|scale|, |beta| + |mean scale|}: the units of GN_TABLE_TOL)"""
    n, hw, c = x.shape
    cpg = c // groups
    xg = x.double().view(n, hw, groups, cpg)
    mean = xg.mean((1, 3))
    var = (xg * xg).mean((1, 3)) - mean * mean
    rstd = 1.0 / torch.sqrt(var.clamp_min(0.0) + eps)
    sc = rstd.repeat_interleave(cpg, 1) * gamma.double()
    ms = mean.repeat_interleave(cpg, 1) * sc
    return torch.stack([sc, beta.double() - ms], -1), torch.stack([sc.abs(), beta.double().abs() + ms.abs()], -1)


def gn_table_excess(got, x, gamma, beta, eps, groups, tol=GN_TABLE_TOL):
    want, mag = gn_table_ref(x, gamma, beta, eps, groups)
    return excess_abs(got, want, tol * mag)


def gn_fold_emul2(srcs, nchs, gamma, beta, eps, groups, fused, plant=None):
    """the table as fmx_groupnorm_apply folds it from the chunk records of one or two sources (csrc/fmx_norm.hip): fp32 records per chunk (chunk_sums_emul),
    their sum per channel in double (`fused`, the fold inside gn_apply_kernel: each channel's sum rounded to fp32 before the group sum; else gn_finalize_kernel:
    double throughout), group mean and variance in double, mean and rstd in fp32, scale = rstd gamma and shift = beta - mean scale in fp32.
    srcs: [x0 [n, hw, c0]] or [x0, x1]; nchs: their chunk counts.  -> fp32 [n, C, 2].  plant: None or one bug -- "nch1_as_nch0" (source 1's records addressed with
    source 0's chunk count: wrong strides, reads running into the next image's records), "straddle_off_by_one" (the group that straddles the two sources
    loses source 0's last channel), "eps_1e5" (eps 1e-5 whatever the caller passed)"""
    n, hw = srcs[0].shape[:2]
    sums = []
    for i, (x, nch) in enumerate(zip(srcs, nchs)):
        p = chunk_sums_emul(x, n, nch)                                  # [n, nch, c, 2]
        if plant == "nch1_as_nch0" and i == 1:
            c, wrong = x.shape[-1], nchs[0]
            flat = p.reshape(-1)
            idx = ((torch.arange(n)[:, None, None] * wrong + torch.arange(wrong)[None, :, None]) * c + torch.arange(c)[None, None, :]) * 2
            p = torch.stack([flat[idx % flat.numel()], flat[(idx + 1) % flat.numel()]], -1)
        sums.append(p.double().sum(1))
    s = torch.cat(sums, 1)                                              # [n, C, 2]
    if plant == "straddle_off_by_one":
        s = s.clone()
        s[:, srcs[0].shape[-1] - 1] = 0.0
    if fused:
        s = s.float().double()
    c = s.shape[1]
    cpg = c // groups
    g = s.view(n, groups, cpg, 2).sum(2) / float(cpg * hw)
    mean_d = g[..., 0]
    var = (g[..., 1] - mean_d * mean_d).clamp_min(0.0).float()
    mean = mean_d.float()
    rstd = torch.rsqrt(var + torch.tensor(1e-5 if plant == "eps_1e5" else eps, dtype=torch.float32))
    sc = rstd.repeat_interleave(cpg, 1) * gamma.float()
    return torch.stack([sc, beta.float() - mean.repeat_interleave(cpg, 1) * sc], -1)


def gn_apply_emul(x, table, silu, dtype):
    """y = x scale + shift (+ SiLU) in fp32, rounded once: x [n, hw, C] -> the same shape in `dtype`"""
    y = x.float() * table[:, None, :, 0] + table[:, None, :, 1]
    return (y * torch.sigmoid(y) if silu else y).to(dtype)


# ---- the token-path row norms and the q/k norm + rope kernel (tests/test_gpu_token_kernels.py) -----------------------------------------------------
# fmx_layernorm / _padded / _mod and fmx_rmsnorm (csrc/fmx_norm.hip: ln_kernel<MAXOCT, MOD>, rmsnorm_kernel<MAXOCT>), fmx_flux_qk_norm_rope
# (csrc/fmx_flux.hip).  `eps` reaches the kernels as a C `float`: the tests hand f32(eps) to the references.
#
# LN_TOL (LayerNorm, its padded and its modulated form): the form of GN_TOL.  The kernel keeps the row in registers, takes the mean and then the sum of
# (x - mean)^2 in fp32 (two passes: no E[x^2] - mean^2 cancellation), forms d * rstd * ((MOD ? 1 : 0) + g) + b in fp32 and rounds ONCE: 0.5 ulp of the
# result plus a handful of fp32 roundings (2^-24 relative each) of terms no larger than |d rstd g| + |b|.  The floor, one ulp at 1.0, is for results
# near zero -- (1 + scale) ~ 0, or d rstd g ~ -b -- whose error comes from the fp32 mean and rstd acting on terms of magnitude ~1, not from their own
# rounding.  A large common offset costs nothing: 16-bit inputs at offset 30000 are multiples of 16 (fp16) or 128 (bf16), far coarser than the fp32
# mean's rounding, so d is exact or nearly so.
LN_TOL = {torch.bfloat16: (1.0, EPS[torch.bfloat16]), torch.float16: (1.0, EPS[torch.float16])}
# RMS_TOL (T5 RMS norm): fp32 sum of squares / c (relative ~1e-6 whatever the order: every term is >= 0), rsqrtf, two fp32 products, one rounding:
# ELEM_TOL as it stands -- 1 ulp with the floor at the smallest subnormal step.  Nothing cancels, so there is no floor at the scale of 1.
RMS_TOL = dict(ELEM_TOL)
# ROPE_TOL (per-head RMS norm of q and k over 128 + rotation of interleaved pairs): about six fp32 roundings and rsqrtf on the way to the two products
# cos a and sin b, each of magnitude at most sqrt(128) |scale| ~ 12: ~1e-5 absolute at the very most, then one rounding of the result: 1 ulp.  The
# floor, one ulp at 1.0 (1e-3 in fp16), is there because cos a - sin b cancels: a result near zero carries the fp32 error of its two terms.
ROPE_TOL = {torch.bfloat16: (1.0, EPS[torch.bfloat16]), torch.float16: (1.0, EPS[torch.float16])}
#
# Worst excess (units of the tolerance) over every case of tests/test_gpu_token_kernels.py, fp16 / bf16: the emulations below (the kernels' arithmetic in
# plain fp32 torch; tests/test_kernel_ref_teeth.py asserts <= 1 and prints them) and the worst `MEASURED` line of the GPU file on MI355X:
#   kernel               tolerance    emulation        MI355X
#   layernorm            LN_TOL       0.408 / 0.437    0.408 / 0.437
#   layernorm_padded     LN_TOL       0.379 / 0.406    0.379 / 0.406
#   layernorm_mod        LN_TOL       0.443 / 0.452    0.443 / 0.452
#   rmsnorm              RMS_TOL      0.500 / 0.500    0.500 / 0.500
#   flux_qk_norm_rope    ROPE_TOL     0.391 / 0.389    0.391 / 0.389     (V^T: bit-equal)
# (No MI355X figure differs from its emulation in the third digit: the worst elements are half-ulp roundings of the result, which neither the device's
# rsqrtf nor the wave's order of summation moves.  rmsnorm's 0.500 is that single rounding with nothing else in the way.)
# Smallest excess of each planted bug over the cases on which tests/test_kernel_ref_teeth.py requires it to show (>= 4 asserted), fp16 / bf16:
#   layernorm          eps_outside_sqrt 1380 / 172 (ONLY on tables with a row of spread 1e-3), last_octet_skipped 1230 / 154 (every table of >= 5 rows)
#   layernorm_mod      eps_outside_sqrt 584 / 74, scale_shift_swapped 5230 / 914, batch0_vectors 5030 / 1140, one_plus_dropped 3170 / 861,
#                      last_octet_skipped 2640 / 321 (every plant on every case)
#   rmsnorm            mean_subtracted 83000 / 48900 and last_octet_skipped 4600 / 3700 (tables with the outlier row), eps_outside_sqrt 798 / 101 (tables
#                      with a row of scale < 1e-2)
#   flux_qk_norm_rope  sin_sign 2400 / 298, half_split 1930 / 242, k_uses_q_scale 414 / 52 (every launch), row_off_dropped 3040 / 378 (row_off > 0),
#                      eps_outside_sqrt 212 / 26 (ONLY through token rows of magnitude < 1e-2), rms_over_all_heads 130 / 16 (more than one token)


def layernorm_mod_ref(x, scale, shift, rows_per_batch, eps):
    """fmx_layernorm_mod: (1 + scale[b]) * LN(x, no affine) + shift[b], b = row // rows_per_batch.  x [rows, c], scale / shift [B, c] -> fp64"""
    img = torch.arange(x.shape[0]) // rows_per_batch
    return (1.0 + scale.double()[img]) * F.layer_norm(x.double(), (x.shape[-1],), None, None, eps) + shift.double()[img]


def rmsnorm_ref(x, w, eps):
    x = x.double()
    return x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * w.double()


def _rope_split(qkv, b, l, h):
    """qkv [b * l, >= 3 * h * 128] (any row stride) -> q, k, v as [b, l, h, 128] views of the same element type"""
    x = qkv[:, :3 * h * 128].reshape(b, l, 3, h, 128)
    return x[:, :, 0], x[:, :, 1], x[:, :, 2]


def qk_norm_rope_ref(qkv, q_scale, k_scale, pe, b, l, h, row_off, eps):
    """fmx_flux_qk_norm_rope in fp64: per-head RMS norm over 128 (eps inside the root) times the scale vector, then the rotation of the INTERLEAVED pairs
    (2i, 2i + 1) by pe[row_off + t, i] = (cos, sin).  qkv [b * l, >= 3 h 128], pe fp32 [>= row_off + l, 64, 2] -> (q, k) fp64 [b, l, h, 128]"""
    q, k, _ = _rope_split(qkv.double(), b, l, h)
    cs = pe[row_off:row_off + l].double()[None, :, None]                    # [1, l, 1, 64, 2]

    def one(t, s):
        t = t * torch.rsqrt((t * t).mean(-1, keepdim=True) + eps) * s.double()
        a, bb = t[..., 0::2], t[..., 1::2]
        return torch.stack([cs[..., 0] * a - cs[..., 1] * bb, cs[..., 1] * a + cs[..., 0] * bb], -1).reshape(b, l, h, 128)

    return one(q, q_scale), one(k, k_scale)


def _rstd_emul(ms, eps, plant):
    e = torch.tensor(eps, dtype=torch.float32)
    return 1.0 / (torch.sqrt(ms) + e) if plant == "eps_outside_sqrt" else torch.rsqrt(ms + e)


def ln_emul(x, gamma, beta, eps, dtype, rows_per_batch=None, plant=None):
    """ln_kernel in fp32 torch: mean = sum / c, variance = sum (x - mean)^2 / c (two passes), d * rstd * ((MOD ? 1 : 0) + g) + b, rounded once.
    rows_per_batch None: gamma / beta [c] (MOD = false); else MOD = true with gamma = scale [B, c], beta = shift [B, c].
    plant: None or one bug -- "eps_outside_sqrt" (1 / (sqrt(var) + eps)), "last_octet_skipped" (the last 8 channels of a row left out of both sums), and
    for MOD "scale_shift_swapped", "batch0_vectors" (every row uses batch 0's vectors), "one_plus_dropped" (scale * LN + shift)"""
    xf = x.float()
    c = xf.shape[-1]
    part = (lambda t: t[:, :c - 8]) if plant == "last_octet_skipped" else (lambda t: t)
    mean = part(xf).sum(-1, keepdim=True) / float(c)
    d = xf - mean
    rstd = _rstd_emul((part(d) * part(d)).sum(-1, keepdim=True) / float(c), eps, plant)
    if rows_per_batch is None:
        g, bt, one = gamma.float(), beta.float(), 0.0
    else:
        img = torch.arange(xf.shape[0]) // rows_per_batch
        if plant == "batch0_vectors":
            img = torch.zeros_like(img)
        g, bt, one = gamma.float()[img], beta.float()[img], 0.0 if plant == "one_plus_dropped" else 1.0
        if plant == "scale_shift_swapped":
            g, bt = bt, g
    return (d * rstd * (one + g) + bt).to(dtype)


def rmsnorm_emul(x, w, eps, dtype, plant=None):
    """rmsnorm_kernel in fp32 torch: sum of squares / c, x * rstd * w, rounded once.  plant: None or one bug -- "mean_subtracted" (LayerNorm's statistics
    and numerator), "eps_outside_sqrt", "last_octet_skipped" (the last 8 channels left out of the sum of squares)"""
    xf = x.float()
    c = xf.shape[-1]
    if plant == "mean_subtracted":
        xf = xf - xf.sum(-1, keepdim=True) / float(c)
    sq = xf * xf
    if plant == "last_octet_skipped":
        sq = sq[:, :c - 8]
    return (xf * _rstd_emul(sq.sum(-1, keepdim=True) / float(c), eps, plant) * w.float()).to(dtype)


def qk_norm_rope_emul(qkv, q_scale, k_scale, pe, b, l, h, row_off, eps, dtype, plant=None):
    """qk_norm_rope_kernel in fp32 torch, as the source has it: one pair per lane, rsqrtf(wave_sum(x0^2 + x1^2) * (1 / 128) + eps), x * r * scale, the
    rotation in fp32, one rounding.  -> (q, k) [b, l, h, 128] in `dtype`.  plant: None or one bug -- "sin_sign", "half_split" (pairs (i, i + 64): the
    rotate-half convention), "row_off_dropped" (pe[t], not pe[row_off + t]), "k_uses_q_scale", "eps_outside_sqrt", "rms_over_all_heads" (one RMS
    per token over h * 128)"""
    q, k, _ = _rope_split(qkv.float(), b, l, h)
    off = 0 if plant == "row_off_dropped" else row_off
    cs = pe[off:off + l].float()[None, :, None]
    cos, sin = cs[..., 0], -cs[..., 1] if plant == "sin_sign" else cs[..., 1]

    def one(t, s):
        sq = t * t
        pair = sq[..., 0::2] + sq[..., 1::2]
        if plant == "rms_over_all_heads":
            ms = pair.sum((-1, -2), keepdim=True) * (1.0 / (128.0 * h))
        else:
            ms = pair.sum(-1, keepdim=True) * (1.0 / 128.0)
        t = t * _rstd_emul(ms, eps, plant) * s.float()
        if plant == "half_split":
            a, bb = t[..., :64], t[..., 64:]
            return torch.cat([cos * a - sin * bb, sin * a + cos * bb], -1).to(dtype)
        a, bb = t[..., 0::2], t[..., 1::2]
        return torch.stack([cos * a - sin * bb, sin * a + cos * bb], -1).reshape(b, l, h, 128).to(dtype)

    return one(q, q_scale), one(k, q_scale if plant == "k_uses_q_scale" else k_scale)
