"""GPU (MI355X) parity of the small fp16 / fp32 kernels that the product path calls and no other kernel-level test calls directly: activations,
pooling, ControlNet residual adds, token embedding, padded LayerNorm, the VAE overflow guard, posterior sampling, masked blending, casts and
the strided layout / dtype adapter.  References: tests/kernel_refs.py (fp64 on the kernel's own rounded inputs), tolerances in output ulps;
tests/test_kernel_ref_teeth.py shows on the CPU that each tolerance rejects a planted bug.  Pure copies and conversions are compared bit for
bit with torch's own conversion."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import forge_amd  # noqa: E402,F401
from forge_amd import hipops as ops  # noqa: E402

import kernel_refs as R  # noqa: E402

DEV = "cuda"
H16 = torch.float16


def gen(seed):
    return torch.Generator("cpu").manual_seed(seed)


def f16_extremes():
    """fp16 values where conversions and activations go wrong: the largest finite, subnormals, signed zeros, the edges of exp's range"""
    return torch.tensor([65504.0, -65504.0, 2.0 ** -24, -(2.0 ** -24), 2.0 ** -20, 2.0 ** -14, 6.0e-5, 0.0, -0.0, -6.0, -9.0, -12.0, -17.0,
                         11.0, 20.0, 1e-3, -1e-3], dtype=H16)


# ---- activations ------------------------------------------------------------------------------------------------------------------
# per kind: (ulps, absolute floor).  quick-GELU / ReLU: fp32 math and one rounding (1 ulp, subnormal-step floor); erf-GELU: the kernel's
# Abramowitz-Stegun erf is documented to |abs err| <= 5e-7 of the GELU (csrc/fmx_common.hpp), so its floor is 2^-20 (9.5e-7)
ACT_TOL = {0: (1.0, 2.0 ** -24), 1: (1.0, 2.0 ** -20), 2: (0.0, 0.0)}


@pytest.mark.parametrize("kind", [ops.ACT_QUICK_GELU, ops.ACT_GELU_ERF, ops.ACT_RELU])
@pytest.mark.parametrize("n", [1, 7, 1000, 4099])
def test_act(kind, n):
    """fmx_act_f16 (quick-GELU for CLIP-L, erf-GELU, ReLU for T2I) on counts that are not a multiple of anything, fp16 extremes, +-inf and
    NaN with a payload included; the negative range -6 .. -17 makes a wrong quick-GELU coefficient visible in the small outputs."""
    x = torch.randn(n, generator=gen(1)) * 4
    ext = f16_extremes()
    x[:min(n, ext.numel())] = ext[:min(n, ext.numel())].float()
    x = x.half()
    if n >= 1000:
        bits = x.view(torch.int16)
        bits[100:104] = torch.tensor([0x7C00, -1024, 0x7E5A, -0x01A6], dtype=torch.int16)   # +inf, -inf, quiet NaN 0x7E5A, NaN 0xFE5A
    out = ops.act(x.to(DEV), kind)
    ulps, atol = ACT_TOL[kind]
    want = R.act_ref(x, kind)
    if kind == ops.ACT_RELU:
        # max(x, 0) needs no rounding: exact, and NaN in gives NaN out as torch.relu does (a NaN must reach the overflow guards downstream)
        torch.testing.assert_close(out.cpu().double(), want, rtol=0, atol=0, equal_nan=True)
    else:
        R.assert_within(out, want, H16, ulps, atol, f"act kind {kind} n {n}")


# ---- pooling / embedding / casts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h,w,c", [(2, 6, 10, 13), (1, 64, 64, 320), (3, 2, 2, 1)])
def test_avgpool2x2(n, h, w, c):
    """fmx_avgpool2x2_nhwc_f16 (T2I-Adapter): odd channel counts (no vector body to hide behind), a 1x1 output.  Four fp16 values summed in
    fp32 and scaled by 1/4: one rounding of the result, 1 ulp + subnormal floor."""
    x = (torch.randn(n, h, w, c, generator=gen(2)) * 3).half()
    got = ops.avgpool2x2(x.to(DEV))
    assert got.shape == (n, h // 2, w // 2, c)
    R.assert_within(got, R.avgpool_ref(x), H16, *R.ELEM_TOL[H16], "avgpool2x2")


def test_embed_tokens():
    """fmx_embed_tokens (CLIP): tok_emb[id] + pos_emb[t] in fp32, one rounding; batch 3 so that position t of image 2 is row 2 * 77 + t."""
    b, t, c, vocab = 3, 77, 768, 1000
    ids = torch.randint(0, vocab, (b, t), generator=gen(3), dtype=torch.int32)
    ids[:, 0], ids[:, -1] = 0, vocab - 1
    tok = (torch.randn(vocab, c, generator=gen(4)) * 0.02).half()
    pos = (torch.randn(t, c, generator=gen(5)) * 0.01).half()
    got = ops.embed_tokens(ids.to(DEV), tok.to(DEV), pos.to(DEV))
    R.assert_within(got, R.embed_ref(ids, tok, pos), H16, *R.ELEM_TOL[H16], "embed_tokens")


def test_cast_f16_rounds_to_nearest_even_and_overflows_to_inf():
    """fmx_cast_f32_to_f16: bit-identical to torch's fp32 -> fp16 conversion: ties to even (1 + 2^-11 -> 1, 1 + 3 * 2^-11 -> 1 + 2^-9), the
    overflow threshold (65519.996 -> 65504, 65520 -> inf), subnormal ties, +-inf; NaN stays NaN.  Counts with a tail."""
    special = torch.tensor([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 65519.996, 65520.0, -65520.0, 65504.0, 1e30, 2.0 ** -25,
                            3 * 2.0 ** -25, 2.0 ** -26, -(2.0 ** -25), 5.96e-8, 6.1e-5, 0.0, -0.0, math.inf, -math.inf, 2.0 ** -14 - 2.0 ** -25],
                           dtype=torch.float32)
    for n in (special.numel(), 1001, 65536 + 5):
        x = torch.randn(n, generator=gen(6)) * 1000
        x[:special.numel()] = special
        x[-3:] = special[:3]
        if n > 100:
            x[50] = math.nan
        got = ops.cast_f16(x.to(DEV)).cpu()
        want = x.half()
        nan = torch.isnan(x)
        assert bool(torch.isnan(got[nan]).all())
        assert torch.equal(got[~nan].view(torch.int16), want[~nan].view(torch.int16)), \
            f"cast differs at {torch.nonzero(got[~nan].view(torch.int16) != want[~nan].view(torch.int16))[:5].flatten().tolist()}"


def test_scale_f32_is_one_rounded_product():
    x = torch.randn(1003, generator=gen(7)) * 100
    for s in (0.18215, -3.0, 1.0 / 0.13025):
        got = ops.scale_f32(x.to(DEV), s).cpu()
        assert torch.equal(got, x * torch.tensor(s, dtype=torch.float32)), f"scale {s}"


# ---- the VAE overflow guard ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 15, 4096, 100003])
def test_count_nonfinite(n):
    """fmx_count_nonfinite_f16 decides whether a decode is redone in bf16: a false negative ships a NaN image.  +-inf and NaNs with payloads at
    even and odd positions (the high half of each 32-bit word), inside the 8-wide vector body and in the scalar tail; +-65504 and subnormals
    are finite.  Exact count."""
    g = gen(8)
    x = (torch.randn(n, generator=g) * 100).half()
    x[0], x[-1] = 65504.0, -65504.0
    bits = x.view(torch.int16)
    bits[n // 2] = 0x0001                                           # smallest subnormal: finite
    bad_bits = [0x7C00, -1024, 0x7C01, 0x7E00, 0x7FFF, -1, -0x01A6]  # +inf, -inf, signalling / quiet NaNs, NaN 0xFFFF, NaN 0xFE5A
    pos = sorted(set([1, 2, 3, n - 2, n - 3] + torch.randint(0, n, (min(n, 40),), generator=g).tolist()) - {0, n - 1, n // 2})
    for i, p in enumerate(pos):
        bits[p] = bad_bits[i % len(bad_bits)]
    want = R.count_nonfinite_ref(bits)
    assert ops.count_nonfinite(x.to(DEV)) == want
    clean = x.clone()
    clean[torch.isinf(clean) | torch.isnan(clean)] = 1.0
    assert ops.count_nonfinite(clean.to(DEV)) == 0


# ---- VAE encode's posterior sample -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_vae_sample_posterior(dtype):
    """fmx_vae_sample_posterior(_bf16): (mean + exp(logvar / 2) * noise - shift) * scale with logvar clamped to [-30, 20] (img2img encode);
    logvar on both sides of both bounds, moments rows with ld > 2 lc (padding columns hold garbage).  fp32 output: 8 fp32 ulps (__expf)."""
    b, lc, hh, ww, ld = 2, 4, 5, 7, 16
    g = gen(9)
    mo = torch.randn(b * hh * ww, ld, generator=g)
    mo[:, 2 * lc:] = 1000.0
    lv = torch.tensor([-40.0, -30.5, -30.0, -29.5, -3.0, 0.0, 5.0, 19.5, 20.0, 20.5, 25.0, 11.0])
    mo[:, lc:2 * lc] = lv[torch.randint(0, lv.numel(), (b * hh * ww, lc), generator=g)]
    mo = mo.to(dtype)
    noise = torch.randn(b, lc, hh, ww, generator=g)
    for scale, shift in ((0.18215, 0.0), (1.5305, 0.0609)):
        got = ops.vae_sample_posterior(mo.to(DEV), ld, noise.to(DEV), lc, scale=scale, shift=shift)
        want = R.sample_posterior_ref(mo, ld, noise, lc, scale, shift)
        R.assert_within(got, want, torch.float32, *R.F32_TOL, f"sample posterior {dtype}")


# ---- masked blending ---------------------------------------------------------------------------------------------------------------------
def test_blend_masked_with_aliased_output():
    """fmx_blend_masked (inpainting, regional conditioning): out = a * am + b * bm, also with out aliasing a and aliasing b.  fp32: the
    kernel may fuse one product into an fma, so 1 fp32 ulp of the result plus a floor of 2^-24 times the product magnitudes."""
    n = 4099
    g = gen(10)
    a, b = torch.randn(n, generator=g) * 4, torch.randn(n, generator=g) * 4
    am = (torch.rand(n, generator=g) > 0.5).float() * torch.rand(n, generator=g)
    bm = 1.0 - am
    want = R.blend_ref(a, am, b, bm)
    atol = 2.0 ** -24 * float((a.abs() * am + b.abs() * bm).max())
    da, db, dam, dbm = a.to(DEV), b.to(DEV), am.to(DEV), bm.to(DEV)
    R.assert_within(ops.blend_masked(da, dam, db, dbm), want, torch.float32, 1.0, atol, "blend")
    ca = da.clone()
    ops.blend_masked(ca, dam, db, dbm, out=ca)
    R.assert_within(ca, want, torch.float32, 1.0, atol, "blend, out aliases a")
    cb = db.clone()
    ops.blend_masked(da, dam, cb, dbm, out=cb)
    R.assert_within(cb, want, torch.float32, 1.0, atol, "blend, out aliases b")


# ---- ControlNet residual adds ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cdtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("b,hh,ww,c", [(1, 5, 3, 13), (2, 8, 8, 320), (1, 3, 3, 7)])
def test_add_control_channels_last(cdtype, b, hh, ww, c):
    """h NHWC += alpha * ctrl where ctrl is an NCHW view of channels-last memory (fmx_add_scaled_f16): fp16 and fp32 residuals, element counts
    with a partial last 8-vector (195, 63) and without (40 960).  fp32 add then one rounding: 1 ulp."""
    g = gen(11)
    h = (torch.randn(b, hh, ww, c, generator=g) * 2).half()
    ctrl_nhwc = (torch.randn(b, hh, ww, c, generator=g)).to(cdtype)
    alpha = 0.7
    dh = h.to(DEV)
    ops.add_control_(dh, ctrl_nhwc.to(DEV).permute(0, 3, 1, 2), alpha)
    R.assert_within(dh, R.add_scaled_ref(h, ctrl_nhwc, alpha), H16, *R.ELEM_TOL[H16], f"add_scaled {cdtype}")


@pytest.mark.parametrize("cdtype", [torch.float16, torch.float32])
def test_add_control_channels_last_unaligned(cdtype):
    """A channels-last residual (or activation) whose data_ptr is not 16-byte aligned cannot take the 16-byte vector path
    (fmx_add_scaled_f16 refuses it); add_control_ routes it to the transposing kernel instead of failing.  Same result as the aligned case."""
    b, hh, ww, c = 2, 6, 5, 24
    g = gen(12)
    h = (torch.randn(b, hh, ww, c, generator=g) * 2).half()
    ctrl = torch.randn(b, hh, ww, c, generator=g).to(cdtype)
    store = torch.zeros(ctrl.numel() + 1, dtype=cdtype, device=DEV)
    cu = store[1:].view(b, hh, ww, c)
    cu.copy_(ctrl.to(DEV))
    assert cu.data_ptr() % 16 != 0
    dh = h.to(DEV)
    ops.add_control_(dh, cu.permute(0, 3, 1, 2), 0.5)
    R.assert_within(dh, R.add_scaled_ref(h, ctrl, 0.5), H16, *R.ELEM_TOL[H16], f"unaligned residual {cdtype}")
    hstore = torch.zeros(h.numel() + 1, dtype=H16, device=DEV)
    hu = hstore[1:].view(b, hh, ww, c)
    hu.copy_(h.to(DEV))
    ops.add_control_(hu, ctrl.to(DEV).permute(0, 3, 1, 2), 0.5)
    R.assert_within(hu, R.add_scaled_ref(h, ctrl, 0.5), H16, *R.ELEM_TOL[H16], f"unaligned activation {cdtype}")
    assert float(hstore[0]) == 0.0


@pytest.mark.parametrize("b,c,hh,ww", [(3, 100, 7, 10), (1, 64, 8, 8), (2, 320, 9, 9), (2, 1, 1, 1)])
def test_add_control_nchw_transposing(b, c, hh, ww):
    """fmx_add_control_nchw: an NCHW-contiguous fp32 residual through 64 x 64 LDS patches; channel and pixel counts that are not multiples of
    64 (ragged patches on both axes), batch > 1, and the degenerate 1 x 1 x 1.  alpha is applied by torch in fp32 before the kernel; fp32
    add then one rounding: 1 ulp (+ the fp32 rounding of alpha * ctrl, far below)."""
    g = gen(13)
    h = (torch.randn(b, hh, ww, c, generator=g) * 2).half()
    ctrl = torch.randn(b, c, hh, ww, generator=g)
    dh = h.to(DEV)
    ops.add_control_(dh, ctrl.to(DEV), 0.75)
    want = R.add_control_nchw_ref(h, (ctrl * 0.75))
    R.assert_within(dh, want, H16, *R.ELEM_TOL[H16], "add_control_nchw")


# ---- padded LayerNorm (ragged SDXL token counts) --------------------------------------------------------------------------------------
def test_layernorm_padded_sdxl_ragged_tokens_leaves_pad_rows_untouched():
    """fmx_layernorm_padded_f16 at SDXL 832 x 1216's ragged level (52 x 76 = 3952 tokens, padded to 4032, c = 1280), batch 2: rows of very
    different scale (1e-2 .. 3, so that eps placement matters), every row compared; the pad rows were filled with a NaN sentinel and must hold
    exactly those bits afterwards.  fp32 statistics, one rounding of the output: 2 ulps, floor 2 ulps at 1.0 (outputs near 0 carry the fp32
    mean's error)."""
    b, n, c = 2, 52 * 76, 1280
    npad = -(-n // 64) * 64
    g = gen(14)
    rs = torch.exp(torch.empty(b * n, 1).uniform_(math.log(1e-2), math.log(3.0), generator=g))
    x = (torch.randn(b * n, c, generator=g) * rs + 0.5 * rs).half()
    gm, bt = (1 + 0.1 * torch.randn(c, generator=g)).half(), (0.1 * torch.randn(c, generator=g)).half()
    out = torch.empty(b, npad, c, dtype=H16, device=DEV)
    out.view(torch.int16).fill_(0x7E5A)
    ops.layernorm_padded(x.to(DEV), gm.to(DEV), bt.to(DEV), out, rows_per_image=n, eps=1e-5)
    got = out.cpu()
    assert bool((got[:, n:].view(torch.int16) == 0x7E5A).all()), "pad rows were written"
    R.assert_within(got[:, :n].reshape(b * n, c), R.layernorm_ref(x, gm, bt, 1e-5), H16, 2.0, 2 * R.EPS[H16], "layernorm_padded")


# ---- strided layout / dtype adapter ----------------------------------------------------------------------------------------------------
KINDS = [torch.float16, torch.float32, torch.bfloat16, torch.bool]


@pytest.mark.parametrize("src_dtype", KINDS)
@pytest.mark.parametrize("dst_dtype", [torch.float16, torch.float32, torch.bfloat16])
def test_strided_copy4_every_kind_pair(src_dtype, dst_dtype):
    """fmx_strided_copy4, every (source kind, destination kind): [B, N, H, d] -> zero-padded heads, and the V -> V^T scatter
    backend/attention.py uses (destination strides of a [H, dp, B, nkp] buffer); a bool mask becomes 0 / -inf.  Values beyond the fp16 range
    and bf16 ties included; bit-identical to torch's conversion (through fp32, as the kernel converts), untouched padding stays zero."""
    b, n, heads, d, dp = 2, 13, 3, 40, 48
    g = gen(15)
    if src_dtype == torch.bool:
        src = torch.rand(b, n, heads, d, generator=g) > 0.3
    else:
        v = torch.randn(b, n, heads, d, generator=g) * 10
        v.view(-1)[:4] = torch.tensor([1e5, -7e4, 1 + 2.0 ** -9, 2.0 ** -20])
        src = v.to(src_dtype)
    dsrc = src.to(DEV)
    st = src.stride()
    dims = (b, n, heads, d)
    want = R.strided_ref(src, dims, st, dst_dtype)
    # [B, N, H, d] -> [B, N, H, dp] zero-padded
    dst = torch.zeros(b, n, heads, dp, dtype=dst_dtype, device=DEV)
    ops.strided_copy4(dsrc, dst, dims, st, dst.stride())
    got = dst.cpu()
    assert _bits_equal(got[..., :d], want), f"head padding copy {src_dtype} -> {dst_dtype}"
    assert bool((got[..., d:] == 0).all())
    # V -> V^T: [H, dp, B, nkp], element (b, j, h, e) at h * dp*B*nkp + e * B*nkp + b * nkp + j
    nkp = 64
    vt = torch.zeros(heads, dp, b, nkp, dtype=dst_dtype, device=DEV)
    ops.strided_copy4(dsrc, vt, dims, st, (vt.stride(2), vt.stride(3), vt.stride(0), vt.stride(1)))
    gv = vt.cpu()
    assert _bits_equal(gv[:, :d, :, :n].permute(2, 3, 0, 1), want), f"V -> V^T {src_dtype} -> {dst_dtype}"
    assert bool((gv[:, d:] == 0).all()) and bool((gv[..., n:] == 0).all())


def test_strided_copy4_zero_strides_broadcast():
    """A stride of 0 broadcasts (a [1, 1, nq, nk] bool mask expanded over batch and heads, as _additive_mask builds it)."""
    b, heads, nq, nk = 2, 3, 5, 77
    m = torch.rand(nq, nk, generator=gen(16)) > 0.5
    dst = torch.empty(b, heads, nq, 80, dtype=torch.float16, device=DEV)
    ops.strided_copy4(m.to(DEV), dst, (b, heads, nq, nk), (0, 0, nk, 1), dst.stride())
    want = torch.where(m, 0.0, -math.inf).half().expand(b, heads, nq, nk)
    assert _bits_equal(dst[..., :nk].cpu(), want)


def _bits_equal(got, want):
    got, want = got.contiguous(), want.contiguous()
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    iv = {2: torch.int16, 4: torch.int32}[got.element_size()]
    return torch.equal(got.view(iv), want.view(iv))


# ---- latent resize -------------------------------------------------------------------------------------------------------------------
def test_resize_separable_against_the_weight_tables():
    """fmx_resize_separable_f32 (latent upscale, modules/latent_upscale.py): out[p, oy, ox] = sum_i sum_j yw[oy, i] xw[ox, j]
    x[p, ys[oy] + i, xs[ox] + j] with per-axis (start, weights) tables of different tap counts (2 rows, 3 columns), taps touching the last
    row / column.  fp32 sums of 6 products: F32_TOL."""
    planes, h, w, oh, ow, ky, kx = 6, 13, 9, 26, 17, 2, 3
    g = gen(17)
    x = torch.randn(planes, h, w, generator=g)
    ys = torch.clamp((torch.arange(oh) * (h - 1)) // (oh - 1), max=h - ky).to(torch.int32)
    xs = torch.clamp((torch.arange(ow) * (w - 1)) // (ow - 1), max=w - kx).to(torch.int32)
    yw, xw = torch.rand(oh, ky, generator=g), torch.rand(ow, kx, generator=g)
    yw, xw = yw / yw.sum(1, keepdim=True), xw / xw.sum(1, keepdim=True)
    got = ops.resize_separable(x.to(DEV).view(2, 3, h, w), ys, yw, xs, xw)
    assert got.shape == (2, 3, oh, ow)
    xr = torch.stack([x[:, ys.long() + i] for i in range(ky)], 2).double()                  # [p, oh, ky, w]
    rows = torch.einsum("pyiw,yi->pyw", xr, yw.double())
    xc = torch.stack([rows[:, :, xs.long() + j] for j in range(kx)], 3)                     # [p, oh, ow, kx]
    want = torch.einsum("pyxj,xj->pyx", xc, xw.double())
    R.assert_within(got.view(planes, oh, ow), want, torch.float32, *R.F32_TOL, "resize_separable")
