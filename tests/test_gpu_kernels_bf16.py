"""GPU (MI355X) kernel-level parity of the bfloat16 twins (the -DFMX_ELEM_BF16 builds, csrc/fmx_bf16_names.hpp) that product code runs and
whole-network fixtures alone guard: the VAE's convolutions, statistics and GroupNorm (the bf16 VAE is the overflow fallback, so it runs on
exactly the inputs where fp16 failed), its mid-block attention and strided softmax, T5's masked d = 64 attention, and the Flux `vec` path's
elementwise kernels.  References: tests/kernel_refs.py, fp64 on the kernel's own rounded bf16 inputs, tolerances in output ulps;
tests/test_kernel_ref_teeth.py shows on the CPU that each tolerance rejects a planted bug."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import forge_amd  # noqa: E402,F401
from forge_amd import hipops as ops  # noqa: E402

import kernel_refs as R  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16


def gen(seed):
    return torch.Generator("cpu").manual_seed(seed)


def rnd(*shape, scale=1.0, seed=0, dtype=BF):
    return (torch.randn(*shape, generator=gen(seed)) * scale).to(dtype)


# ---- convolutions as the bf16 VAE runs them (backend/nn/vae.py) ------------------------------------------------------------------------
CONV_CASES = {
    "3x3": dict(n=2, h=16, w=16, c=128, co=128, kh=3, stride=1, pad=1),
    "3x3_ragged": dict(n=1, h=9, w=7, c=64, co=64, kh=3, stride=1, pad=1),
    "down_even": dict(n=2, h=16, w=16, c=128, co=128, kh=3, stride=2, down=True),
    "down_odd": dict(n=1, h=9, w=11, c=64, co=64, kh=3, stride=2, down=True),
    "shortcut_1x1": dict(n=2, h=12, w=12, c=128, co=256, kh=1, stride=1, pad=0),
    "up_on_load": dict(n=2, h=8, w=8, c=128, co=128, kh=3, stride=1, pad=1, up=(16, 16)),
    "up_ragged": dict(n=1, h=5, w=6, c=64, co=64, kh=3, stride=1, pad=1, up=(10, 12)),
    "concat": dict(n=2, h=16, w=16, c=128, c1=64, co=128, kh=3, stride=1, pad=1),
}


def conv_case(cfg, seed=20):
    """inputs of one CONV_CASES entry, bf16 on the CPU: x, x1, torch-layout weight, bias, residual (shape of the output)"""
    n, h, w, c, c1, co, kh = cfg["n"], cfg["h"], cfg["w"], cfg["c"], cfg.get("c1", 0), cfg["co"], cfg["kh"]
    x = rnd(n, h, w, c, seed=seed)
    x1 = rnd(n, h, w, c1, seed=seed + 1) if c1 else None
    wt = rnd(co, c + c1, kh, kh, scale=1 / math.sqrt((c + c1) * kh * kh), seed=seed + 2)
    bias = rnd(co, scale=0.5, seed=seed + 3)
    ih, iw = cfg.get("up") or (h, w)
    if cfg.get("down"):
        oh, ow = (ih + 1 - 3) // 2 + 1, (iw + 1 - 3) // 2 + 1
    else:
        oh, ow = (ih + 2 * cfg["pad"] - kh) // cfg["stride"] + 1, (iw + 2 * cfg["pad"] - kh) // cfg["stride"] + 1
    res = rnd(n * oh * ow, co, seed=seed + 4)
    return x, x1, wt, bias, res, (oh, ow)


def conv_case_ref(cfg, x, x1, wt, bias, res):
    xin = torch.cat([x, x1], -1) if x1 is not None else x
    if cfg.get("down"):   # F.pad(x, (0, 1, 0, 1)) then 3x3 stride 2, pad 0 (vae.py Downsample)
        return R.conv_ref(xin, wt, bias, stride=2, pad_rb=(1, 1), residual=res)
    return R.conv_ref(xin, wt, bias, stride=cfg["stride"], pad=cfg["pad"], up=cfg.get("up"), residual=res)


@pytest.mark.parametrize("tile", [0, 6, 7])      # 0: the dispatcher's choice; 6 / 7: the pipelined 256x256 / 256x320 kernels
@pytest.mark.parametrize("case", sorted(CONV_CASES))
def test_bf16_conv(case, tile):
    """fmx_gemm_conv_bf16 as a convolution: 3x3 pad 1, the encoder's Downsample exactly as vae.py runs it (pad 0, stride 2, out_hw from a
    right / bottom zero pad that only the loader's bounds check supplies; even and odd H / W), 1x1 shortcuts, nearest x2 upsample on load,
    the two-source concat; bias and residual epilogues.  Tolerance: kernel_refs.CONV_TOL."""
    cfg = CONV_CASES[case]
    x, x1, wt, bias, res, (oh, ow) = conv_case(cfg)
    co, kh = cfg["co"], cfg["kh"]
    wk = wt.permute(0, 2, 3, 1).reshape(co, -1).contiguous()
    kw = dict(kh=kh, stride=cfg["stride"], pad=0 if cfg.get("down") else cfg["pad"], up=cfg.get("up"), force_tile=tile)
    if cfg.get("down"):
        kw["out_hw"] = (oh, ow)
    out = ops.conv_gemm(x.to(DEV), wk.to(DEV), co, x1=None if x1 is None else x1.to(DEV), bias=bias.to(DEV), residual=res.to(DEV), **kw)
    assert out.dtype == BF
    want = conv_case_ref(cfg, x, x1, wt, bias, res)
    R.assert_within(out.view(want.shape), want, BF, *R.CONV_TOL[BF], f"bf16 conv {case} tile {tile}")


# ---- producer statistics and GroupNorm ---------------------------------------------------------------------------------------------------
def gn_conv_inputs(n, hh, ww, cin, c, seed):
    """a 3x3 conv whose output channel groups have standard deviations from 3e-3 to 1 (32 groups): eps 1e-6 vs 1e-5 is visible in the
    smallest groups, and the statistics have to be right across a 300x range of scales"""
    x = rnd(n, hh, ww, cin, seed=seed)
    gscale = torch.logspace(math.log10(3e-3), 0, 32).repeat_interleave(c // 32)
    wt = (torch.randn(c, cin, 3, 3, generator=gen(seed + 1)) / math.sqrt(cin * 9) * gscale[:, None, None, None]).to(BF)
    bias = (0.3 * gscale * torch.randn(c, generator=gen(seed + 2))).to(BF)
    gamma, beta = (1 + 0.1 * torch.randn(c, generator=gen(seed + 3))).to(BF), (0.1 * torch.randn(c, generator=gen(seed + 4))).to(BF)
    return x, wt, bias, gamma, beta


@pytest.mark.parametrize("tile", [0, 6, 7])
@pytest.mark.parametrize("n,hh,ww,cin,c", [(2, 16, 16, 64, 128), (1, 32, 32, 128, 256), (2, 10, 10, 64, 512)])
def test_bf16_conv_statistics_and_groupnorm(n, hh, ww, cin, c, tile):
    """fmx_gemm_conv_stats_bf16: the per-(image, channel) {sum, sum of squares} partials against fp64 sums of the ROUNDED bf16 outputs the
    kernel stored (epilogue statistics on 16 x 16 / 32 x 32 images, the pass behind the GEMM on 10 x 10); then fmx_groupnorm_apply_bf16 fed by
    them (one source, two sources = the same tensor twice, SiLU on and off, eps 1e-6, 32 groups, 128 / 256 / 512 channels) against fp64
    GroupNorm of the stored output.  Sums: fp32 accumulation over <= 256-pixel chunks, relative 2e-5 as for fp16; GroupNorm: GN_TOL."""
    x, wt, bias, gamma, beta = gn_conv_inputs(n, hh, ww, cin, c, seed=40)
    wk = wt.permute(0, 2, 3, 1).reshape(c, -1).contiguous()
    out, st = ops.conv_gemm(x.to(DEV), wk.to(DEV), c, kh=3, pad=1, bias=bias.to(DEV), stats=True, force_tile=tile)
    assert out.dtype == BF and st is not None
    got = st.partial.reshape(-1)[:n * st.nchunks * c * 2].view(n, st.nchunks, c, 2).double().sum(1).cpu()
    torch.testing.assert_close(got, R.stat_sums_ref(out.cpu(), n), rtol=2e-5, atol=2e-3)
    o4 = out.view(n, hh, ww, c)
    oc = o4.cpu()
    g, b = gamma.to(DEV), beta.to(DEV)
    for silu in (False, True):
        y = ops.groupnorm(o4, g, b, 1e-6, silu=silu, stats=st)
        R.assert_within(y, R.groupnorm_ref(oc, gamma, beta, 1e-6, silu=silu), BF, *R.GN_TOL[BF], f"bf16 GroupNorm silu={silu}")
    g2, b2 = torch.cat([gamma, gamma]), torch.cat([beta, beta])
    y2 = ops.groupnorm(o4, g2.to(DEV), b2.to(DEV), 1e-6, x1=o4, silu=True, stats=st, stats1=st)
    R.assert_within(y2, R.groupnorm_ref(torch.cat([oc, oc], -1), g2, b2, 1e-6, silu=True), BF, *R.GN_TOL[BF], "bf16 two-source GroupNorm")
    y3 = ops.groupnorm(o4, g, b, 1e-6, silu=True)          # its own statistics pass (fmx_groupnorm_stats_bf16)
    R.assert_within(y3, R.groupnorm_ref(oc, gamma, beta, 1e-6, silu=True), BF, *R.GN_TOL[BF], "bf16 GroupNorm, own statistics")


def test_bf16_groupnorm_large_offset_values():
    """bf16 twin of test_groupnorm_large_offset_values: mean 30 standard deviations, values ~3e3 (beyond what fp16 carries precisely)."""
    n, h, w, c = 2, 64, 64, 320
    x = (torch.randn(n, h, w, c, generator=gen(320)) * 100 + 3000).to(BF)
    g, b = (1 + 0.1 * torch.randn(c, generator=gen(321))).to(BF), (0.1 * torch.randn(c, generator=gen(322))).to(BF)
    y = ops.groupnorm(x.to(DEV), g.to(DEV), b.to(DEV), 1e-5)
    R.assert_within(y, R.groupnorm_ref(x, g, b, 1e-5), BF, *R.GN_TOL[BF], "bf16 groupnorm, mean >> std")


# GroupNorm offset sweep.  The statistics are one-pass fp32 partials {sum x, sum x^2}, folded in double (csrc/fmx_norm.hip); their error
# grows as (mean / std)^2.  Measured on an MI355X with GN_TOL (1 output ulp + 1 ulp at 1.0), 2 x 32 x 32 x 256, 32 groups, largest ratio
# inside it: fp16 150 from either source (out at 200); bf16 >= 1000 from groupnorm_stats, 600 from the GEMM epilogue.  With
# the fold in fp32 fp16 left the tolerance below 100.  The real SDXL VAE's mean / std ratio is unknown here (every VAE test runs on synth.py's
# random-init weights).
OFFSET_RATIOS = (0, 10, 30, 100, 300, 1000)
OFFSET_LIMIT = 100        # asserted: inside GN_TOL up to here, for both element types and both statistics sources


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("source", ["groupnorm_stats", "gemm_epilogue"])
def test_groupnorm_offset_sweep(dtype, source):
    """mean / std in {0, 10, 30, 100, 300, 1000} at std 1 (fp16: |x| <= ~1e3) or std 100 (bf16: |x| up to ~1e5), statistics from the
    stand-alone pass or from the producing GEMM's epilogue (a 1x1 conv whose bias carries the offset).  Every ratio up to OFFSET_LIMIT must
    stay inside GN_TOL; the ratios beyond it are evaluated (and reported on failure) but only the limit is asserted."""
    std = 1.0 if dtype == torch.float16 else 100.0
    n, h, w, c, cin = 2, 32, 32, 256, 64
    gamma = (1 + 0.1 * torch.randn(c, generator=gen(330))).to(dtype)
    beta = (0.1 * torch.randn(c, generator=gen(331))).to(dtype)
    g, b = gamma.to(DEV), beta.to(DEV)
    seen = {}
    for r in OFFSET_RATIOS:
        if source == "groupnorm_stats":
            x = (torch.randn(n, h, w, c, generator=gen(332), dtype=torch.float64) * std + r * std).to(dtype).to(DEV)
            y = ops.groupnorm(x, g, b, 1e-6)
        else:
            xi = rnd(n, h, w, cin, seed=333, dtype=dtype).to(DEV)
            wk = (torch.randn(c, cin, generator=gen(334)) * std / math.sqrt(cin)).to(dtype).to(DEV)
            out, st = ops.conv_gemm(xi, wk, c, bias=torch.full((c,), r * std, dtype=dtype, device=DEV), stats=True)
            x = out.view(n, h, w, c)
            y = ops.groupnorm(x, g, b, 1e-6, stats=st)
        seen[r] = R.excess(y, R.groupnorm_ref(x.cpu(), gamma, beta, 1e-6), dtype, *R.GN_TOL[dtype])
    bad = {r: round(e, 2) for r, e in seen.items() if r <= OFFSET_LIMIT and e > 1.0}
    assert not bad, f"{dtype} {source}: outside GN_TOL at mean/std <= {OFFSET_LIMIT}: {bad} (all: { {k: round(v, 2) for k, v in seen.items()} })"


# ---- attention ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,n,nk", [(2, 1024, 1024), (2, 1000, 1000), (3, 200, 77)])
def test_bf16_attention_single_head_512_wide(b, n, nk):
    """fmx_attention_single_head512_bf16 (bf16 VAE mid-block attention) at the fp16 test's shapes: ragged query / key counts, padded keys
    holding garbage, a dominant key in the last valid row.  fp64 reference on the device; ATTN_TOL."""
    c = 512
    nkp = -(-nk // 32) * 32
    q = rnd(b * n, c, seed=121).to(DEV)
    k = torch.full((b * nkp, c), 7.0, dtype=BF, device=DEV)
    v = torch.full((b, nkp, c), -5.0, dtype=BF, device=DEV)
    k.view(b, nkp, c)[:, :nk] = rnd(b, nk, c, seed=122).to(DEV)
    v[:, :nk] = rnd(b, nk, c, seed=123).to(DEV)
    k.view(b, nkp, c)[b - 1, nk - 1] = q.view(b, n, c)[b - 1, n - 1] * 0.5
    vt = v.permute(2, 0, 1).reshape(c, b * nkp).contiguous()
    o = torch.empty(b * n, c, dtype=BF, device=DEV)
    ops.attention_single_head512(q, k, vt, o, batch=b, nq=n, nk=nk, nk_pad=nkp, q_bs=n * c, q_rs=c, k_bs=nkp * c, k_rs=c, vt_bs=nkp, vt_ds=b * nkp,
                                 scale=c ** -0.5)
    want = R.attn_ref(q.view(b, 1, n, c), k.view(b, 1, nkp, c)[:, :, :nk], v[:, None, :nk], c ** -0.5)
    R.assert_within(o.view(b, 1, n, c), want, BF, *R.ATTN_TOL[BF], f"bf16 512-wide attention b{b} n{n} nk{nk}")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("rows,n,ld", [(300, 1000, 1024), (64, 77, 128), (5, 13, 64), (2, 4099, 4160)])
def test_softmax_rows_on_a_strided_view(dtype, rows, n, ld):
    """softmax_rows_ on s[:, :n] of an [rows, ld] buffer (vae.py's strided call: ld = npad > n, n % 8 != 0): the columns n..ld hold a large
    sentinel (30.0) that must neither enter the row sums nor be written.  SOFTMAX_TOL."""
    s = torch.full((rows, ld), 30.0, dtype=dtype)
    s[:, :n] = (torch.randn(rows, n, generator=gen(60)) * 3).to(dtype)
    want = R.softmax_ref(s[:, :n])
    d = s.to(DEV)
    ops.softmax_rows_(d[:, :n])
    got = d.cpu()
    assert torch.equal(got[:, n:], s[:, n:]), "columns beyond the view were written"
    R.assert_within(got[:, :n], want, dtype, *R.SOFTMAX_TOL[dtype], f"softmax rows {dtype} n{n} ld{ld}")


def t5_bias(heads, t, tp, seed):
    """relative-position-style additive bias [H, t, tp] in bf16: a per-head table indexed by a log-bucketed (j - i), zeros beyond t"""
    rel = torch.arange(t)[None, :] - torch.arange(t)[:, None]
    bucket = torch.sign(rel) * torch.floor(torch.log2(rel.abs().float() + 1) * 3)
    table = torch.randn(heads, 64, generator=gen(seed)) * 3
    vals = table[:, (bucket + 32).long().clamp(0, 63)]
    out = torch.zeros(heads, t, tp)
    out[:, :, :t] = vals
    return out.to(BF)


@pytest.mark.parametrize("t", [1, 77, 255, 256, 300, 512])
def test_bf16_attention_t5_masked(t):
    """fmx_attention_bf16 exactly as the T5 encoder calls it (backend/nn/t5.py): d = 64, scale 1.0 on unscaled scores of magnitude ~30, an
    additive bias [H, t, tp] varying per head and per query with mask_strides (0, t * tp, tp), nq = nk = t not a multiple of 64, Q | K
    in one [B, tp, 2C] buffer and V^T [C, B * tp].  fp64 reference on the device; ATTN_TOL."""
    b, heads, d = 2, 4, 64
    c = heads * d
    tp = -(-t // 64) * 64
    qk = torch.zeros(b, tp, 2 * c, dtype=BF)
    qk[:, :t] = rnd(b, t, 2 * c, scale=1.2, seed=200 + t)     # q . k over 64 dims: std ~ 1.44 * 8 = 11.5, extremes ~ 30
    v = rnd(b, t, c, seed=300 + t)
    vt = torch.zeros(c, b * tp, dtype=BF)
    vt.view(c, b, tp)[:, :, :t] = v.permute(2, 0, 1)
    bias = t5_bias(heads, t, tp, seed=400 + t)
    dqk, dvt, dbias = qk.to(DEV), vt.to(DEV), bias.to(DEV)
    out = ops.attention(dqk, dqk[:, :, c:], dvt, batch=b, heads=heads, nq=t, nk=t, nk_pad=tp, dpad=d, scale=1.0, q_bs=tp * 2 * c, q_rs=2 * c,
                        k_bs=tp * 2 * c, k_rs=2 * c, vt_bs=tp, vt_hs=d * b * tp, vt_ds=b * tp, mask=dbias, mask_strides=(0, t * tp, tp))
    q = dqk[:, :t, :c].view(b, t, heads, d).permute(0, 2, 1, 3)
    k = dqk[:, :t, c:].view(b, t, heads, d).permute(0, 2, 1, 3)
    vv = v.to(DEV).view(b, t, heads, d).permute(0, 2, 1, 3)
    want = R.attn_ref(q, k, vv, 1.0, mask=dbias[None, :, :, :t])
    got = out.view(b, t, heads, d).permute(0, 2, 1, 3)
    R.assert_within(got, want, BF, *R.ATTN_TOL[BF], f"bf16 T5 attention t{t}")


@pytest.mark.parametrize("b,h,nq,nk", [(2, 3, 300, 300), (1, 2, 1024, 1024), (2, 4, 512, 77), (1, 2, 256, 128)])
def test_bf16_attention_d64_unmasked(b, h, nq, nk):
    """bf16 d = 64 without a mask and nq >= 256: the short-context (nk <= 128) and long-context d_head-64 kernels in their bf16 builds, which
    no other test launches; padded keys hold garbage.  ATTN_TOL."""
    d = 64
    nkp = -(-nk // 64) * 64
    q = rnd(b, nq, h, d, seed=500)
    k = torch.full((b, nkp, h, d), 6.0, dtype=BF)
    v = torch.full((b, nkp, h, d), -4.0, dtype=BF)
    k[:, :nk], v[:, :nk] = rnd(b, nk, h, d, seed=501), rnd(b, nk, h, d, seed=502)
    dq, dk, dv = q.to(DEV), k.to(DEV), v.to(DEV)
    vt = dv.permute(2, 3, 0, 1).contiguous()
    out = ops.attention(dq, dk, vt, batch=b, heads=h, nq=nq, nk=nk, nk_pad=nkp, dpad=d, scale=d ** -0.5, q_bs=nq * h * d, q_rs=h * d,
                        k_bs=nkp * h * d, k_rs=h * d, vt_bs=nkp, vt_hs=d * b * nkp, vt_ds=b * nkp)
    want = R.attn_ref(dq.permute(0, 2, 1, 3), dk.permute(0, 2, 1, 3)[:, :, :nk], dv.permute(0, 2, 1, 3)[:, :, :nk], d ** -0.5)
    R.assert_within(out.view(b, nq, h, d).permute(0, 2, 1, 3), want, BF, *R.ATTN_TOL[BF], f"bf16 attention d64 b{b} h{h} nq{nq} nk{nk}")


# ---- the Flux `vec` path and the VAE boundary ------------------------------------------------------------------------------------------
def test_bf16_silu():
    """fmx_silu_bf16 (csrc/fmx_flux.hip, separate code from the fp16 form): counts with no vector width in common, bf16 extremes (3e38,
    subnormals), +-inf.  ELEM_TOL."""
    for n in (1, 255, 4099):
        x = torch.randn(n, generator=gen(70)) * 6
        ext = torch.tensor([3.0e38, -3.0e38, 1e-39, -1e-39, 0.0, -20.0, -80.0, 88.0, math.inf, -math.inf, 2.0 ** -126])
        x[:min(n, ext.numel())] = ext[:min(n, ext.numel())]
        x = x.to(BF)
        got = ops.silu(x.to(DEV))
        assert got.dtype == BF
        R.assert_within(got, R.silu_ref(x), BF, *R.ELEM_TOL[BF], f"bf16 silu n{n}")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_timestep_embedding_flux_range(dtype):
    """fmx_timestep_embedding(_bf16) at dim 256 with t as Flux feeds it (1000 * t and 1000 * guidance: up to 1e4) and the UNet's 0..999;
    cos first, sin second.  TEMB_TOL."""
    t = torch.tensor([0.0, 1.0, 3.5, 999.0, 1000.0, 3500.0, 10000.0, 417.25])
    got = ops.timestep_embedding(t.to(DEV), 256, dtype=dtype)
    assert got.dtype == dtype
    R.assert_within(got, R.timestep_ref(t, 256), dtype, *R.TEMB_TOL[dtype], f"timestep embedding {dtype}")


@pytest.mark.parametrize("c,ld", [(4, 8), (16, 20)])
def test_bf16_vae_pack_and_unpack(c, ld):
    """fmx_vae_pack_latent_bf16 (z / scaling_factor + shift into a padded NHWC row of ld columns, padding exactly zero) and
    fmx_vae_unpack_image_bf16 (clamp((y + 1) / 2, 0, 1) out of a padded bf16 row, values outside [-1, 1] included).  ELEM_TOL / F32_TOL."""
    b, hh, ww = 2, 5, 7
    z = torch.randn(b, c, hh, ww, generator=gen(80)) * 3
    for sf, shift in ((0.18215, 0.0), (0.3611, 0.1159)):
        p = ops.vae_pack_latent(z.to(DEV), sf, shift, ld=ld, dtype=BF)
        assert p.dtype == BF and p.shape == (b, hh, ww, ld)
        want = R.pack_latent_ref(z, sf, shift, ld)
        R.assert_within(p[..., :c], want[..., :c], BF, *R.ELEM_TOL[BF], f"vae pack bf16 c{c} ld{ld}")
        assert bool((p[..., c:].float() == 0).all())
    npix, ldo = b * hh * ww, 4
    y = (torch.randn(npix, ldo, generator=gen(81)) * 1.5).to(BF)
    out = torch.empty(b, hh, ww, 3, device=DEV)
    ops.vae_unpack_image(y.to(DEV), ldo, npix, 3, out)
    R.assert_within(out.view(npix, 3), R.unpack_image_ref(y, ldo, 3), torch.float32, *R.F32_TOL, "vae unpack bf16")
