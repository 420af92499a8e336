"""CPU: the kernel-level GPU tests have teeth.  For each test in tests/test_gpu_kernels_bf16.py, tests/test_gpu_small_kernels.py, each test
family of tests/test_gpu_attention_generic.py, each window case of tests/test_gpu_gemm_windows.py, each check of tests/test_gpu_vae_direct.py, each kernel of tests/test_gpu_sampler_kernels.py, each part of tests/test_gpu_groupnorm_routes.py and each kernel of tests/test_gpu_token_kernels.py, one
plausible subtle bug is planted into the fp64 reference (tests/kernel_refs.py) and evaluated on that test's own inputs; the planted result must
lie outside the GPU test's tolerance by at least 4x (kernel_refs.excess >= 4), or -- for the exact tests -- differ in at least 4 places.
Runs without a GPU, so a tolerance too loose to catch anything fails before anyone gets a GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

import kernel_refs as R
import test_gpu_attention_generic as G
import test_gpu_gemm_windows as W
import test_gpu_kernels_bf16 as B
import test_gpu_small_kernels as S
import test_gpu_vae_direct as V

BF, H16 = torch.bfloat16, torch.float16
TEETH = 4.0


def bites(planted, want, dtype, tol, what):
    e = R.excess(planted, want, dtype, *tol)
    assert e >= TEETH, f"{what}: the planted bug is only {e:.3g}x the tolerance"


# ---- bf16 file ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["down_even", "down_odd"])
def test_conv_downsample_pad_on_the_wrong_side_is_caught(case):
    """planted: the Downsample's zero row / column taken at the top / left instead of bottom / right (a one-pixel border shift)"""
    cfg = B.CONV_CASES[case]
    x, x1, wt, bias, res, _ = B.conv_case(cfg)
    want = B.conv_case_ref(cfg, x, x1, wt, bias, res)
    xin = F.pad(x.double().permute(0, 3, 1, 2), (1, 0, 1, 0))
    planted = F.conv2d(xin, wt.double(), bias.double(), stride=2).permute(0, 2, 3, 1) + res.double().reshape(want.shape)
    bites(planted, want, BF, R.CONV_TOL[BF], case)


def test_conv_up_on_load_off_by_one_is_caught():
    """planted: nearest upsample on load reading source row (y + 1) // 2 instead of y // 2"""
    cfg = B.CONV_CASES["up_ragged"]
    x, x1, wt, bias, res, _ = B.conv_case(cfg)
    want = B.conv_case_ref(cfg, x, x1, wt, bias, res)
    uh, uw = cfg["up"]
    iy = ((torch.arange(uh) + 1) // 2).clamp(max=cfg["h"] - 1)
    ix = ((torch.arange(uw) + 1) // 2).clamp(max=cfg["w"] - 1)
    xu = x[:, iy][:, :, ix]
    planted = R.conv_ref(xu, wt, bias, pad=1, residual=res)
    bites(planted, want, BF, R.CONV_TOL[BF], "up on load")


def test_groupnorm_eps_1e5_instead_of_1e6_is_caught():
    n, hh, ww, cin, c = 2, 16, 16, 64, 128
    x, wt, bias, gamma, beta = B.gn_conv_inputs(n, hh, ww, cin, c, seed=40)
    out = R.conv_ref(x, wt, bias, pad=1).to(BF)      # stands in for the stored bf16 output
    want = R.groupnorm_ref(out, gamma, beta, 1e-6, silu=True)
    bites(R.groupnorm_ref(out, gamma, beta, 1e-5, silu=True), want, BF, R.GN_TOL[BF], "GroupNorm eps")


def test_groupnorm_statistics_missing_a_chunk_is_caught():
    """planted: the last chunk's partials dropped from the sums (relative 2e-5 tolerance of the statistics check)"""
    n, hh, ww, cin, c = 2, 10, 10, 64, 512
    x, wt, bias, _, _ = B.gn_conv_inputs(n, hh, ww, cin, c, seed=40)
    out = R.conv_ref(x, wt, bias, pad=1).to(BF).reshape(n * hh * ww, c)
    want = R.stat_sums_ref(out, n)
    planted = R.stat_sums_ref(out.view(n, hh * ww, c)[:, :-32].reshape(-1, c), n)
    with pytest.raises(AssertionError):
        torch.testing.assert_close(planted, want, rtol=2e-5, atol=2e-3)


def test_groupnorm_large_offset_mean_rounded_to_bf16_is_caught():
    """planted: the group mean rounded to bf16 before it is subtracted (ulp 16 at 3000: a shift of ~0.1 standard deviation)"""
    n, h, w, c = 1, 16, 16, 320
    x = (torch.randn(n, h, w, c, generator=B.gen(320)) * 100 + 3000).to(BF)
    g, b = (1 + 0.1 * torch.randn(c, generator=B.gen(321))).to(BF), (0.1 * torch.randn(c, generator=B.gen(322))).to(BF)
    want = R.groupnorm_ref(x, g, b, 1e-5)
    xg = x.double().reshape(n, h * w, 32, c // 32)
    mean = xg.mean((1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean((1, 3), keepdim=True)
    planted = ((xg - mean.to(BF).double()) / torch.sqrt(var + 1e-5)).reshape(n, h, w, c) * g.double() + b.double()
    bites(planted, want, BF, R.GN_TOL[BF], "GroupNorm mean rounded")


def test_attention512_padded_keys_not_masked_is_caught():
    b, n, nk, c = 3, 200, 77, 512
    nkp = -(-nk // 32) * 32
    q = B.rnd(b * n, c, seed=121).view(b, 1, n, c)
    k = torch.full((b, nkp, c), 7.0, dtype=BF)
    v = torch.full((b, nkp, c), -5.0, dtype=BF)
    k[:, :nk], v[:, :nk] = B.rnd(b, nk, c, seed=122), B.rnd(b, nk, c, seed=123)
    k[b - 1, nk - 1] = q[b - 1, 0, n - 1] * 0.5
    want = R.attn_ref(q, k[:, None, :nk], v[:, None, :nk], c ** -0.5)
    bites(R.attn_ref(q, k[:, None], v[:, None], c ** -0.5), want, BF, R.ATTN_TOL[BF], "512-wide attention over padded keys")


@pytest.mark.parametrize("dtype", [H16, BF])
def test_softmax_sum_over_the_padding_columns_is_caught(dtype):
    rows, n, ld = 64, 77, 128
    s = torch.full((rows, ld), 30.0, dtype=dtype)
    s[:, :n] = (torch.randn(rows, n, generator=B.gen(60)) * 3).to(dtype)
    want = R.softmax_ref(s[:, :n])
    bites(R.softmax_ref(s)[:, :n], want, dtype, R.SOFTMAX_TOL[dtype], "softmax over ld columns")


def test_t5_bias_of_head_0_for_every_head_is_caught():
    """planted: the mask's head stride ignored (mask_hs treated as 0): every head gets head 0's position bias"""
    b, heads, d, t = 2, 4, 64, 77
    c, tp = heads * d, 128
    qk = B.rnd(b, t, 2 * c, scale=1.2, seed=200 + t)
    v = B.rnd(b, t, c, seed=300 + t)
    bias = B.t5_bias(heads, t, tp, seed=400 + t)
    q = qk[..., :c].view(b, t, heads, d).permute(0, 2, 1, 3)
    k = qk[..., c:].view(b, t, heads, d).permute(0, 2, 1, 3)
    vv = v.view(b, t, heads, d).permute(0, 2, 1, 3)
    want = R.attn_ref(q, k, vv, 1.0, mask=bias[None, :, :, :t])
    planted = R.attn_ref(q, k, vv, 1.0, mask=bias[None, :1, :, :t])
    bites(planted, want, BF, R.ATTN_TOL[BF], "T5 bias head stride")


def test_d64_scale_folded_twice_is_caught():
    """planted: 1/sqrt(d) applied to the scores twice (e.g. once folded into log2(e) and once by the caller)"""
    b, h, nq, nk, d = 2, 4, 512, 77, 64
    q = B.rnd(b, nq, h, d, seed=500).permute(0, 2, 1, 3)
    k, v = B.rnd(b, nk, h, d, seed=501).permute(0, 2, 1, 3), B.rnd(b, nk, h, d, seed=502).permute(0, 2, 1, 3)
    want = R.attn_ref(q, k, v, d ** -0.5)
    bites(R.attn_ref(q, k, v, d ** -1.0), want, BF, R.ATTN_TOL[BF], "d64 scale")


def test_silu_tail_left_unwritten_is_caught():
    """planted: the elements past the last full 256-thread block (4096..4099) never written (zero)"""
    x = (torch.randn(4099, generator=B.gen(70)) * 6).to(BF)
    want = R.silu_ref(x)
    planted = want.clone()
    planted[4096:] = 0.0
    bites(planted, want, BF, R.ELEM_TOL[BF], "silu tail")


@pytest.mark.parametrize("dtype", [H16, BF])
def test_timestep_embedding_cos_sin_swapped_is_caught(dtype):
    t = torch.tensor([0.0, 1.0, 3.5, 999.0, 1000.0, 3500.0, 10000.0, 417.25])
    bites(R.timestep_ref(t, 256, swap=True), R.timestep_ref(t, 256), dtype, R.TEMB_TOL[dtype], "cos / sin swapped")


def test_vae_pack_shift_before_division_and_unpack_without_clamp_are_caught():
    z = torch.randn(2, 16, 5, 7, generator=B.gen(80)) * 3
    want = R.pack_latent_ref(z, 0.3611, 0.1159, 20)
    planted = torch.zeros_like(want)
    planted[..., :16] = ((z.double() + 0.1159) / 0.3611).permute(0, 2, 3, 1)
    bites(planted[..., :16], want[..., :16], BF, R.ELEM_TOL[BF], "pack: (z + shift) / sf")
    y = (torch.randn(70, 4, generator=B.gen(81)) * 1.5).to(BF)
    bites((y.double()[:, :3] + 1.0) / 2.0, R.unpack_image_ref(y, 4, 3), torch.float32, R.F32_TOL, "unpack: no clamp")


# ---- small-kernel file ------------------------------------------------------------------------------------------------------------------
def test_quick_gelu_coefficient_1_7_is_caught():
    x = torch.randn(4099, generator=S.gen(1)) * 4
    x[:17] = S.f16_extremes().float()
    x = x.half()
    bites(R.act_ref(x, 0, quick_gelu_coef=1.7), R.act_ref(x, 0), H16, S.ACT_TOL[0], "quick-GELU 1.7")


def test_erf_gelu_as_tanh_approximation_is_caught():
    x = (torch.randn(4099, generator=S.gen(1)) * 4).half()
    planted = F.gelu(x.double(), approximate="tanh")
    bites(planted, R.act_ref(x, 1), H16, S.ACT_TOL[1], "erf-GELU as tanh-GELU")


def test_relu_dropping_nan_is_caught():
    x = torch.tensor([1.0, -1.0, math.nan, math.nan, math.nan, math.nan]).half()
    assert R.excess(torch.nan_to_num(R.act_ref(x, 2), nan=0.0), R.act_ref(x, 2), H16, 1.0, 0.0) == math.inf


def test_avgpool_window_shifted_by_one_column_is_caught():
    x = (torch.randn(2, 6, 10, 13, generator=S.gen(2)) * 3).half()
    xs = torch.cat([x[:, :, 1:], x[:, :, -1:]], 2)
    bites(R.avgpool_ref(xs), R.avgpool_ref(x), H16, R.ELEM_TOL[H16], "avgpool column shift")


def test_embed_position_off_by_one_is_caught():
    b, t, c, vocab = 3, 77, 768, 1000
    ids = torch.randint(0, vocab, (b, t), generator=S.gen(3), dtype=torch.int32)
    tok = (torch.randn(vocab, c, generator=S.gen(4)) * 0.02).half()
    pos = (torch.randn(t, c, generator=S.gen(5)) * 0.01).half()
    planted = R.embed_ref(ids, tok, torch.cat([pos[1:], pos[-1:]]))
    bites(planted, R.embed_ref(ids, tok, pos), H16, R.ELEM_TOL[H16], "embed position + 1")


def test_cast_round_toward_zero_is_caught():
    x = torch.randn(1001, generator=S.gen(6)) * 1000
    want = x.half()
    wb = want.view(torch.int16)
    planted = torch.where(want.float().abs() > x.abs(), wb - 1, wb)     # one fp16 step toward zero where RNE rounded away from it
    assert int((planted != wb).sum()) >= TEETH


def test_scale_by_reciprocal_division_is_caught():
    x = torch.randn(1003, generator=S.gen(7)) * 100
    s = torch.tensor(0.18215, dtype=torch.float32)
    assert int((x / (1.0 / s) != x * s).sum()) >= TEETH


@pytest.mark.parametrize("n", [4096, 100003])
def test_count_nonfinite_ignoring_the_high_half_word_is_caught(n):
    g = S.gen(8)
    x = (torch.randn(n, generator=g) * 100).half()
    bits = x.view(torch.int16)
    pos = sorted(set([1, 2, 3, n - 2, n - 3] + torch.randint(0, n, (min(n, 40),), generator=g).tolist()) - {0, n - 1, n // 2})
    for p in pos:
        bits[p] = 0x7C00
    assert R.count_nonfinite_ref(bits) - R.count_nonfinite_ref(bits, high_half_ignored=True) >= TEETH


def test_sample_posterior_unclamped_logvar_is_caught():
    b, lc, hh, ww, ld = 2, 4, 5, 7, 16
    g = S.gen(9)
    mo = torch.randn(b * hh * ww, ld, generator=g)
    lv = torch.tensor([-40.0, -30.5, -30.0, -29.5, -3.0, 0.0, 5.0, 19.5, 20.0, 20.5, 25.0, 11.0])
    mo[:, lc:2 * lc] = lv[torch.randint(0, lv.numel(), (b * hh * ww, lc), generator=g)]
    mo = mo.half()
    noise = torch.randn(b, lc, hh, ww, generator=g)
    want = R.sample_posterior_ref(mo, ld, noise, lc, 0.18215, 0.0)
    bites(R.sample_posterior_ref(mo, ld, noise, lc, 0.18215, 0.0, clamp=False), want, torch.float32, R.F32_TOL, "logvar unclamped")


def test_blend_with_the_wrong_mask_is_caught():
    n = 4099
    g = S.gen(10)
    a, b = torch.randn(n, generator=g) * 4, torch.randn(n, generator=g) * 4
    am = (torch.rand(n, generator=g) > 0.5).float() * torch.rand(n, generator=g)
    bm = 1.0 - am
    atol = 2.0 ** -24 * float((a.abs() * am + b.abs() * bm).max())
    bites(R.blend_ref(a, am, b, am), R.blend_ref(a, am, b, bm), torch.float32, (1.0, atol), "blend b * a_mask")


def test_add_scaled_last_partial_vector_skipped_is_caught():
    b, hh, ww, c = 1, 5, 3, 13          # 195 elements: a 3-element tail
    g = S.gen(11)
    h = (torch.randn(b, hh, ww, c, generator=g) * 2).half()
    ctrl = torch.randn(b, hh, ww, c, generator=g).half()
    bites(R.add_scaled_ref(h, ctrl, 0.7, skip_tail=True), R.add_scaled_ref(h, ctrl, 0.7), H16, R.ELEM_TOL[H16], "tail skipped")


def test_add_control_nchw_read_as_nhwc_is_caught():
    b, c, hh, ww = 3, 100, 7, 10
    g = S.gen(13)
    h = (torch.randn(b, hh, ww, c, generator=g) * 2).half()
    ctrl = torch.randn(b, c, hh, ww, generator=g) * 0.75
    planted = h.double() + ctrl.double().reshape(b, hh, ww, c)
    bites(planted, R.add_control_nchw_ref(h, ctrl), H16, R.ELEM_TOL[H16], "NCHW read as NHWC")


def test_layernorm_eps_outside_the_sqrt_is_caught():
    c = 1280
    g = S.gen(14)
    rs = torch.exp(torch.empty(2000, 1).uniform_(math.log(1e-2), math.log(3.0), generator=g))
    x = (torch.randn(2000, c, generator=g) * rs + 0.5 * rs).half()
    gm, bt = (1 + 0.1 * torch.randn(c, generator=g)).half(), (0.1 * torch.randn(c, generator=g)).half()
    xd = x.double()
    mu, sd = xd.mean(-1, keepdim=True), xd.var(-1, unbiased=False, keepdim=True).sqrt()
    planted = (xd - mu) / (sd + 1e-5) * gm.double() + bt.double()
    bites(planted, R.layernorm_ref(x, gm, bt, 1e-5), H16, (2.0, 2 * R.EPS[H16]), "layernorm eps outside sqrt")


def test_bool_mask_as_one_zero_is_caught():
    m = torch.rand(5, 77, generator=S.gen(16)) > 0.5
    want = R.strided_ref(m, (1, 1, 5, 77), (0, 0, 77, 1), H16)
    planted = m.half().reshape(1, 1, 5, 77)
    assert int((planted.view(torch.int16) != want.view(torch.int16)).sum()) >= TEETH


# ---- generic attention file -------------------------------------------------------------------------------------------------------------
def _tri(t, keep):
    """additive [1, 1, t, nk_pad(t)] mask: 0 where keep(i, j), -inf elsewhere"""
    i, j = torch.arange(t)[:, None], torch.arange(G.nkpad(t))[None, :]
    return torch.where(keep(i, j), 0.0, -math.inf)[None, None]


@pytest.mark.parametrize("keep,what", [(lambda i, j: j < i, "causal diagonal excluded"), (lambda i, j: j <= i + 1, "causal off by one")])
def test_causal_boundary_bugs_are_caught(keep, what):
    t, d = 77, 64
    _, _, q, k, v = G.clip_case(t, 12, H16)
    want = G.reference(q, k, v, t, d, causal=True, dev="cpu")
    bites(G.reference(q, k, v, t, d, mask=_tri(t, keep), dev="cpu"), want, H16, R.ATTN_TOL[H16], what)


@pytest.mark.parametrize("dtype", [H16, BF])
def test_mask_stride_bugs_are_caught(dtype):
    """planted on the all-strides case: the query stride ignored (row 0 for every query), the batch stride ignored (batch 0's mask for every
    batch), the mask multiplied by the score scale (added after the scaling of the unscaled score instead of divided by it)"""
    d = 80
    mask, q, k, v, _ = G.mask_case(7, d, dtype)
    want = G.reference(q, k, v, G.MASK_NK, d, mask=mask, dev="cpu")
    tol = R.ATTN_TOL[dtype]
    bites(G.reference(q, k, v, G.MASK_NK, d, mask=mask[:, :, :1], dev="cpu"), want, dtype, tol, "mask query stride ignored")
    bites(G.reference(q, k, v, G.MASK_NK, d, mask=mask[:1], dev="cpu"), want, dtype, tol, "mask batch stride ignored")
    scaled = (mask.double() * d ** -0.5).to(dtype)
    bites(G.reference(q, k, v, G.MASK_NK, d, mask=scaled, dev="cpu"), want, dtype, tol, "mask scaled with the scores")


def test_scale_from_dpad_is_caught():
    """planted: 1 / sqrt(48) for d_head 40 (the padded width); on the first head of the SD1.5 cross-attention case"""
    b, h, nq, nk, d = 8, 8, 4096, 77, 40
    q, k, v = G.sd15_case(b, h, nq, nk, d)
    q1, k1, v1 = (t[:1, :, :1, :d].permute(0, 2, 1, 3) for t in (q, k[:, :nk], v[:, :nk]))
    want = R.attn_ref(q1, k1, v1, d ** -0.5)
    bites(R.attn_ref(q1, k1, v1, G.DPAD[d] ** -0.5), want, H16, R.ATTN_TOL[H16], "scale from dpad")


def test_nan_after_a_masked_leading_tile_is_caught():
    """planted: the rows whose first key tile is fully masked come out NaN (alpha = exp2(-inf - -inf))"""
    d = 40
    mask, q, k, v, _ = G.neg_inf_case("lead_128_some_queries", d, H16)
    want = G.reference(q, k, v, G.INF_NK, d, mask=mask, dev="cpu")
    lead = (mask[..., :64] == -math.inf).all(-1)[:, 0]                       # [B, nq]
    planted = want.clone()
    planted.permute(0, 2, 1, 3)[lead] = math.nan
    assert bool(lead.any())
    bites(planted, want, H16, R.ATTN_TOL[H16], "NaN rows after a masked leading tile")


def test_mask_pad_columns_added_is_caught():
    """planted: the ragged-tail -inf set before the mask is added, so the NaN / +inf of the mask's pad columns reach the scores"""
    d = 64
    mask, q, k, v, _ = G.neg_inf_case("pad_nan_inf", d, H16)
    nk, nkp = G.INF_NK, G.nkpad(G.INF_NK)
    want = G.reference(q, k, v, nk, d, mask=mask, dev="cpu")
    leaked = mask.double().clone()
    leaked[..., nk:] = -math.inf + leaked[..., nk:]
    bites(G.reference(q, k, v, nkp, d, mask=leaked, dev="cpu"), want, H16, R.ATTN_TOL[H16], "mask pad columns added")


# ---- GEMM window file -------------------------------------------------------------------------------------------------------------------
DTS = [H16, BF]


def _one(case_id, dtype):
    """(case, its single launch, its fp64 reference)"""
    case = W.build(case_id, dtype)
    return case, case.launches[0], W.case_refs(case_id, dtype)[0]


def _strided_read(win, rows, cols, ld):
    """the [rows, cols] elements a kernel reads from win's buffer when it steps `ld` elements per row from the window's first element"""
    idx = win.values.storage_offset() + torch.arange(rows)[:, None] * ld + torch.arange(cols)[None]
    return win.buf.reshape(-1)[idx]


def _pre(L, img_rows=None):
    """fp64 pre-activation acc * alpha + bias + rowvec[image] of a linear launch"""
    return R.gemm_ref(L.a0.values, L.w.values, a1=None if L.a1 is None else L.a1.values, alpha=L.alpha, bias=None if L.bias is None else L.bias.values,
                      rowvec=None if L.rowvec is None else L.rowvec.values, rows_per_image=img_rows or L.per)


def test_every_window_case_runs_on_each_tile_family():
    """condition of the GPU file: besides the dispatcher's own refusals nothing is skipped, so every case runs on a 2-stage 4-wave tile, a ring
    tile and -- where every launch is eligible8 -- a 256-row tile; and the operands keep the contract (16-byte bases, A / W strides % 8)"""
    for case_id in W.CASE_IDS:
        for dtype in DTS:
            case = W.build(case_id, dtype)
            runs = lambda t: all(W.refusal(L, case.out_buf, t) is None for L in case.launches)  # noqa: E731
            assert runs(0) and any(runs(t) for t in W.TWO_STAGE) and any(runs(t) for t in W.RING), case_id
            if all(W.eligible8(L, case.out_buf) for L in case.launches):
                assert any(runs(t) for t in W.ROWS256), case_id
            for L in case.launches:
                for win in (L.a0, L.a1, L.w, L.bias, L.rowvec, L.gate, L.residual):
                    if win is not None:
                        assert (win.values.storage_offset() * 2) % 16 == 0, case_id
                for win in (L.a0, L.a1, L.w):
                    assert win is None or win.values.stride(0) % 8 == 0, case_id
                out = case.out_buf[L.rows, L.cols]
                assert (out.storage_offset() * out.element_size()) % 16 == 0, case_id
    assert any(all(W.eligible8(L, W.build(c, H16).out_buf) for L in W.build(c, H16).launches) for c in W.CASE_IDS if c.startswith("out_cols_eligible8"))


@pytest.mark.parametrize("dtype", DTS)
def test_window_residual_addressed_with_ld_out_is_caught(dtype):
    """residual_window: the residual read `ld_out` instead of `ld_res` elements per row (neighbouring columns of the residual's buffer)"""
    for case_id in ("residual_window-0", "residual_window-2"):
        case, L, want = _one(case_id, dtype)
        wrong = _strided_read(L.residual, L.m, L.ncols, case.out_buf.stride(0))
        bites(want - L.residual.values.double() + wrong.double(), want, dtype, W.tolerance(L, dtype), case_id)


@pytest.mark.parametrize("dtype", DTS)
def test_window_image_index_from_the_tile_height_is_caught(dtype):
    """rowvec_gate_strided, two_source_full_epilogue: rowvec / gate image index row // roundup(per_img, 128) -- right for tile-aligned images"""
    for case_id in ("rowvec_gate_strided-0", "rowvec_gate_strided-1", "two_source_full_epilogue-0"):
        case, L, want = _one(case_id, dtype)
        img = (torch.arange(L.m) // (-(-L.per // 128) * 128)).clamp(max=L.n_img - 1)
        v = _pre(L) - (0 if L.rowvec is None else L.rowvec.values.double()[torch.arange(L.m) // L.per] - L.rowvec.values.double()[img])
        v = R.gelu_tanh_ref(v) if L.act == "gelu_tanh" else v
        v = v * L.gate.values.double()[img]
        if L.inplace:
            v = v + case.out_buf[L.rows, L.cols].double()
        bites(v, want, dtype, W.tolerance(L, dtype), case_id)


@pytest.mark.parametrize("dtype", DTS)
def test_window_alpha_applied_to_the_bias_is_caught(dtype):
    """alpha_order: (acc + bias) * alpha instead of acc * alpha + bias"""
    for case_id in ("alpha_order-0", "alpha_order-1"):
        _, L, want = _one(case_id, dtype)
        bites(want + (L.alpha - 1.0) * L.bias.values.double(), want, dtype, W.tolerance(L, dtype), case_id)


@pytest.mark.parametrize("dtype", DTS)
def test_window_a_read_from_the_wrong_place_is_caught(dtype):
    """a_windows: A read from column 0 of its buffer instead of the window's offset; the second source stepped with the first source's stride"""
    _, L, want = _one("a_windows-0", dtype)
    rows = L.a0.idx[0]
    col0 = L.a0.buf[rows, :L.a0.values.shape[1]]
    bites(R.gemm_ref(col0, L.w.values, bias=L.bias.values), want, dtype, W.tolerance(L, dtype), "a_windows-0: A from column 0")
    _, L, want = _one("a_windows-2", dtype)
    a1 = _strided_read(L.a1, L.m, L.a1.values.shape[1], L.a0.values.stride(0))
    bites(R.gemm_ref(L.a0.values, L.w.values, a1=a1, bias=L.bias.values), want, dtype, W.tolerance(L, dtype), "a_windows-2: a1 with a0's stride")


@pytest.mark.parametrize("dtype", DTS)
def test_window_ldw_ignored_is_caught(dtype):
    """w_window: weight rows taken K elements apart instead of ldw"""
    _, L, want = _one("w_window-0", dtype)
    k = L.w.values.shape[1]
    bites(R.gemm_ref(L.a0.values, _strided_read(L.w, L.nout, k, k), bias=L.bias.values), want, dtype, W.tolerance(L, dtype), "w_window-0: ldw ignored")


@pytest.mark.parametrize("case_id", ["out_cols_ragged-0", "out_cols_ragged-1"])
def test_window_last_partial_group_stored_in_full_trips_the_sentinel_rule(case_id):
    """out_cols_ragged (t = 77, 33): the last partial group of 4 columns stored as a full group writes 4 - nout % 4 pad columns of every row; the
    sentinel rule must see at least 4 changed elements.  (With the dense odd rows of out_ld_odd the same overrun lands in the head of the NEXT
    row, inside the window, and only the last row's 2-3 elements reach the sentinel: that case relies on the value comparison.)"""
    case = W.build(case_id, H16)
    L, want = case.launches[0], W.case_refs(case_id, H16)[0]
    after = case.out_buf.clone()
    flat, ld = after.reshape(-1), after.stride(0)
    full = -(-L.ncols // 4) * 4
    vals = torch.zeros(L.m, full, dtype=H16)
    vals[:, :L.ncols] = want.to(H16)
    idx = after[L.rows, L.cols].storage_offset() + torch.arange(L.m)[:, None] * ld + torch.arange(full)[None]
    flat[idx] = vals
    assert full > L.ncols and W.changed_outside(case.out_buf, after, L.rows, L.cols) >= TEETH
    clean = case.out_buf.clone()
    clean[L.rows, L.cols] = want.to(H16)
    assert W.changed_outside(case.out_buf, clean, L.rows, L.cols) == 0


@pytest.mark.parametrize("dtype", DTS)
def test_window_geglu_halves_swapped_is_caught(dtype):
    """geglu_window: gelu(value) * gate for value * gelu(gate)"""
    for case_id in ("geglu_window-0", "geglu_window-1"):
        _, L, want = _one(case_id, dtype)
        h = _pre(L)
        planted = R.gelu_erf_ref(h[:, :L.ncols]) * h[:, L.ncols:] + (0 if L.residual is None else L.residual.values.double())
        bites(planted, want, dtype, W.tolerance(L, dtype), case_id)


@pytest.mark.parametrize("dtype", DTS)
def test_window_out_cols_eligible8_row_stride_from_nout_is_caught(dtype):
    """out_cols_eligible8 (sentinel rule): rows stored nout instead of ld_out elements apart run through the left and right surroundings"""
    case, L, want = _one("out_cols_eligible8-0", dtype)
    after = case.out_buf.clone()
    idx = after[L.rows, L.cols].storage_offset() + torch.arange(L.m)[:, None] * L.nout + torch.arange(L.nout)[None]
    after.reshape(-1)[idx] = want.to(dtype)
    assert W.changed_outside(case.out_buf, after, L.rows, L.cols) >= TEETH


@pytest.mark.parametrize("dtype", DTS)
def test_fp32_output_rounded_through_the_16_bit_type_is_caught(dtype):
    """fp32_out: the result rounded to fp16 / bf16 before the fp32 store must exceed GEMM_F32_TOL by 4x; a plain fp32 evaluation stays inside"""
    for i in (0, 1):
        L = W.build_f32(i, dtype).launches[0]
        want, bound = W.f32_ref_and_bound(L)
        e = R.excess_abs(want.to(dtype), want, bound)
        assert e >= TEETH, f"fp32_out {W.F32_CASES[i]}: rounding through {dtype} is only {e:.3g}x the bound"
        plain = (L.a0.values.float() @ L.w.values.float().t()) * L.alpha + L.bias.values.float() + L.residual.values.float()
        assert R.excess_abs(plain, want, bound) <= 0.25
        dropped = want - L.alpha * L.a0.values.double()[:, -1:] * L.w.values.double()[:, -1][None]
        assert R.excess_abs(dropped, want, bound) >= 100 * TEETH


@pytest.mark.parametrize("dtype", DTS)
def test_gate_before_the_activation_is_caught_and_plain_fp32_meets_the_tolerance(dtype):
    """rowvec_gate_strided with GELU-tanh: gelu(pre * gate) for gelu(pre) * gate; and the same formulas in plain fp32 torch on the fp32
    pre-activation, rounded once, lie inside GEMM_ACT_TOL (the figure quoted at kernel_refs.GEMM_ACT_TOL)"""
    worst = 0.0
    for case_id in ("rowvec_gate_strided-1", "rowvec_gate_strided-3", "rowvec_gate_strided-4", "geglu_window-0", "geglu_window-1"):
        _, L, want = _one(case_id, dtype)
        img = torch.arange(L.m) // L.per
        if L.gate is not None:
            bites(R.gelu_tanh_ref(_pre(L) * L.gate.values.double()[img]), want, dtype, W.tolerance(L, dtype), case_id)
        pre = L.a0.values.float() @ L.w.values.float().t()
        if L.bias is not None:
            pre = pre + L.bias.values.float()
        if L.rowvec is not None:
            pre = pre + L.rowvec.values.float()[img]
        if L.act == "geglu":
            v = pre[:, :L.ncols] * F.gelu(pre[:, L.ncols:])
        else:
            v = F.gelu(pre, approximate="tanh") * L.gate.values.float()[img]
        if L.residual is not None:
            v = v + L.residual.values.float()
        worst = max(worst, R.excess(v.to(dtype), want, dtype, *R.CONV_TOL[dtype]))
    print(f"plain fp32 activation epilogues, {dtype}: worst {worst:.3g}x CONV_TOL")
    assert worst <= 1.0 and R.GEMM_ACT_TOL[dtype] == R.CONV_TOL[dtype]


# ---- the VAE decoder's direct kernels (tests/test_gpu_vae_direct.py) --------------------------------------------------------------------------
# Every planted bug goes into the fp32 emulation of the kernel's arithmetic (kernel_refs.gn_silu_conv_emul / attn512_emul, plain fp32 convolutions)
# and is judged against the GPU test's fp64 reference at the GPU test's tolerance; the unplanted emulation has to stay inside it.
WORST = {}     # kernel -> worst unplanted excess seen (printed by test_zz_report_worst_emulation_excess; the figures beside kernel_refs.CONV_TOL)


def _inside(got, want, dtype, tol, kernel, what):
    e = R.excess(got, want, dtype, *tol)
    WORST[(kernel, dtype)] = max(WORST.get((kernel, dtype), 0.0), e)
    assert e <= 1.0, f"{what}: the unplanted emulation is {e:.3g}x the tolerance"


def _gn_emul(k, dtype, residual, plant=None):
    return R.gn_silu_conv_emul(k.x, k.gamma, k.beta, V.EPS_GN, k.wt, k.bias, k.res if residual else None, dtype, groups=k.groups, plant=plant).reshape(k.m, k.nout)


@pytest.mark.parametrize("dtype", DTS)
def test_vae_gn_silu_emulation_meets_the_tolerance_on_every_case(dtype):
    for shape in V.GN_SHAPES:
        for residual in (False, True):
            _inside(_gn_emul(V.gn_case(shape, dtype), dtype, residual), V.gn_ref(shape, dtype, residual=residual), dtype, R.CONV_TOL[dtype], "conv3x3_gn_silu", shape)
    k = V.gn_case((2, 8, 32, 128), dtype, groups=16)
    _inside(_gn_emul(k, dtype, True), V.gn_ref((2, 8, 32, 128), dtype, 16, residual=True), dtype, R.CONV_TOL[dtype], "conv3x3_gn_silu", "16 groups")
    for shape in V.NARROW_SHAPES:
        k = V.gn_case(shape[:4], dtype, 32, shape[4])
        _inside(_gn_emul(k, dtype, False), V.gn_ref(shape[:4], dtype, 32, shape[4]), dtype, R.CONV_TOL[dtype], "conv3x3_narrow_gn_silu", shape)
        k = V.narrow_case(shape, dtype)
        got = F.conv2d(k.x.float().permute(0, 3, 1, 2), k.wt.float(), k.bias.float(), padding=1).permute(0, 2, 3, 1).reshape(k.m, k.nout).to(dtype)
        _inside(got, V.narrow_ref(shape, dtype), dtype, R.CONV_TOL[dtype], "conv3x3_narrow", shape)


@pytest.mark.parametrize("dtype", DTS)
@pytest.mark.parametrize("plant", ["pad_before_norm", "table_of_image0", "table_one_chunk_on", "kykx"])
def test_vae_gn_silu_planted_bugs_are_caught(plant, dtype):
    """the halo padded before the norm; image 0's {scale, shift} for every image; the table of channels c + 64; ky / kx transposed -- on a case with several
    images and chunks for the wide kernel, and on a narrow one"""
    shape = (3, 9, 33, 64) if plant in ("pad_before_norm", "kykx") else (2, 17, 65, 192)
    bites(_gn_emul(V.gn_case(shape, dtype), dtype, True, plant), V.gn_ref(shape, dtype, residual=True), dtype, R.CONV_TOL[dtype], f"gn_silu {plant}")
    nshape = (3, 5, 33, 96, 4) if plant != "table_one_chunk_on" else (2, 6, 31, 320, 4)
    k = V.gn_case(nshape[:4], dtype, 32, nshape[4])
    bites(_gn_emul(k, dtype, False, plant), V.gn_ref(nshape[:4], dtype, 32, nshape[4]), dtype, R.CONV_TOL[dtype], f"narrow gn_silu {plant}")
    kn = V.narrow_case(nshape, dtype)
    if plant == "kykx":
        got = F.conv2d(kn.x.float().permute(0, 3, 1, 2), kn.wt.float().transpose(2, 3), kn.bias.float(), padding=1).permute(0, 2, 3, 1).reshape(kn.m, kn.nout)
        bites(got.to(dtype), V.narrow_ref(nshape, dtype), dtype, R.CONV_TOL[dtype], "narrow kykx")


@pytest.mark.parametrize("dtype", DTS)
def test_vae_gn_silu_residual_addressed_with_ld_out_is_caught(dtype):
    """the residual window (ld_res 136) stepped through with ld_out = 160"""
    for shape in ((2, 8, 32, 128), (3, 9, 33, 64)):
        k = V.gn_case(shape, dtype)
        _, _, _, res = V.gn_destination(k, "residual_windows", dtype)
        idx = res.values.storage_offset() + torch.arange(k.m)[:, None] * 160 + torch.arange(V.COUT)[None]
        wrong = res.buf.reshape(-1)[idx % res.buf.numel()]
        want = V.gn_ref(shape, dtype, residual=True)
        bites(_gn_emul(k, dtype, False).double() + wrong.double(), want, dtype, R.CONV_TOL[dtype], f"residual ld {shape}")


@pytest.mark.parametrize("dtype", DTS)
def test_vae_statistics_counting_pixels_outside_the_image_are_caught(dtype):
    """planted: the out-of-image pixels of the partial tiles (value bias: what the epilogue holds for them) enter the sums"""
    for shape in ((3, 9, 33, 64), (2, 17, 65, 192), (1, 5, 7, 64)):
        n, h, w, _ = shape
        k = V.gn_case(shape, dtype)
        stored = V.gn_ref(shape, dtype).to(dtype)
        want = R.stat_sums_ref(stored, n)
        extra = -(-h // 8) * 8 * -(-w // 32) * 32 - h * w
        b = k.bias.double()
        planted = want + extra * torch.stack([b, b * b], -1)[None]
        with pytest.raises(AssertionError):
            torch.testing.assert_close(planted, want, **V.STAT_TOL)
        leaked = want.roll(1, 0) if n > 1 else None       # records of image i under image i + 1
        if leaked is not None:
            with pytest.raises(AssertionError):
                torch.testing.assert_close(leaked, want, **V.STAT_TOL)


@pytest.mark.parametrize("dtype", DTS)
def test_vae_up2x_planted_bugs_are_caught(dtype):
    """py / px swapped (phases 1 and 2 exchanged); the even rows' tap sums on the odd rows; image i's border reading image i - 1"""
    for shape in V.UP_SHAPES:
        k, want = V.up_case(shape, dtype), V.up_ref(shape, dtype)
        nout = shape[4]
        emul = R.up2x_ref(k.x.float(), k.w4.float(), k.bias.float()).float().reshape(-1, nout).to(dtype)     # fp32 operands; see the note below
        _inside(emul, want, dtype, R.CONV_TOL[dtype], "conv3x3_up2x", shape)
        bites(R.up2x_ref(k.x, k.w4[[0, 2, 1, 3]], k.bias).reshape(-1, nout), want, dtype, R.CONV_TOL[dtype], f"up2x py/px swapped {shape}")
        bites(R.up2x_ref(k.x, k.w4[[0, 1, 0, 1]], k.bias).reshape(-1, nout), want, dtype, R.CONV_TOL[dtype], f"up2x even weights on odd rows {shape}")
    shape = (3, 8, 32, 128, 136)
    k, want = V.up_case(shape, dtype), V.up_ref(shape, dtype)
    n, h, w, c, nout = shape
    tall = R.up2x_ref(k.x.reshape(1, n * h, w, c), k.w4, k.bias).reshape(-1, nout)      # the batch as ONE tall image: borders see the neighbours
    bites(tall, want, dtype, R.CONV_TOL[dtype], "up2x cross-image border")


def _fp32_sum_emul(k, dtype):
    """the phase convolutions with fp32 accumulation (torch conv2d in fp32), rounded once"""
    n, h, w, c, nout = k.shape
    xin = k.x.float().permute(0, 3, 1, 2)
    out = torch.zeros(n, nout, 2 * h, 2 * w)
    for ph in range(4):
        py, px = ph >> 1, ph & 1
        out[:, :, py::2, px::2] = F.conv2d(F.pad(xin, (1 - px, px, 1 - py, py)), k.w4[ph].float().view(nout, 2, 2, c).permute(0, 3, 1, 2), k.bias.float())
    return out.permute(0, 2, 3, 1).reshape(-1, nout).to(dtype)


@pytest.mark.parametrize("dtype", DTS)
def test_vae_up2x_fp32_emulation_meets_the_tolerance(dtype):
    for shape in V.UP_SHAPES:
        _inside(_fp32_sum_emul(V.up_case(shape, dtype), dtype), V.up_ref(shape, dtype), dtype, R.CONV_TOL[dtype], "conv3x3_up2x", shape)


def _attn_operands(a, dtype):
    """q, and k / v as the qk-halves layout holds them: rows >= nk of the image's key half are 7.0, V^T pad columns -5"""
    rows = max(a.nq, a.nk, -(-a.nk // 32) * 32)
    k = torch.full((a.b, rows, V.C512), 7.0, dtype=dtype)
    v = torch.full((a.b, rows, V.C512), -5.0, dtype=dtype)
    k[:, :a.nk], v[:, :a.nk] = a.k, a.v
    return a.q, k, v


@pytest.mark.parametrize("dtype", DTS)
def test_vae_attention512_emulation_meets_the_tolerance_on_every_case(dtype):
    cases = [(b, nq, nk, None) for b, nq, nk in V.ATTN_SHAPES] + [(2, 96, nk, s) for s, nk in V.ATTN_STRUCTURES.items()]
    for b, nq, nk, s in cases:
        a = V.attn_case(b, nq, nk, dtype, s)
        q, k, v = _attn_operands(a, dtype)
        got = R.attn512_emul(q, k, v, nk, V.C512 ** -0.5, dtype).reshape(b * nq, V.C512)
        _inside(got, V.attn_ref(b, nq, nk, dtype, s), dtype, R.ATTN_TOL[dtype], "attention512", (b, nq, nk, s))


@pytest.mark.parametrize("dtype", DTS)
def test_vae_attention512_planted_bugs_are_caught(dtype):
    """pad keys not masked (ragged last step); the accumulator not rescaled when the running maximum rises; k taken from the q half"""
    sc = V.C512 ** -0.5
    for b, nq, nk, s in ((2, 63, 31, None), (3, 65, 33, None), (2, 96, 150, "late_spike_ragged")):
        a = V.attn_case(b, nq, nk, dtype, s)
        q, k, v = _attn_operands(a, dtype)
        bites(R.attn512_emul(q, k, v, nk, sc, dtype, plant="pad_keys_attend").reshape(b * nq, -1), V.attn_ref(b, nq, nk, dtype, s), dtype, R.ATTN_TOL[dtype], f"pad keys {nk}")
    for s in ("staircase", "late_spike_ragged"):
        nk = V.ATTN_STRUCTURES[s]
        a = V.attn_case(2, 96, nk, dtype, s)
        q, k, v = _attn_operands(a, dtype)
        bites(R.attn512_emul(q, k, v, nk, sc, dtype, plant="no_rescale").reshape(2 * 96, -1), V.attn_ref(2, 96, nk, dtype, s), dtype, R.ATTN_TOL[dtype], f"no rescale {s}")
    for b, nq, nk in ((2, 64, 32), (2, 200, 77)):
        a = V.attn_case(b, nq, nk, dtype)
        q, k, v = _attn_operands(a, dtype)
        kq = torch.full_like(k, 30000.0)                 # the q half of the same rows: q, then the 30000 behind it
        kq[:, :min(nq, k.shape[1])] = q[:, :k.shape[1]]
        bites(R.attn512_emul(q, kq, v, nk, sc, dtype).reshape(b * nq, -1), V.attn_ref(b, nq, nk, dtype), dtype, R.ATTN_TOL[dtype], f"k from the q half {nk}")


def test_zz_report_worst_emulation_excess():
    """prints the worst unplanted-emulation excess per kernel and type gathered above (visible with -s): the figures beside kernel_refs.CONV_TOL"""
    for (kernel, dtype), e in sorted(WORST.items(), key=str):
        print(f"EMULATION {kernel} {dtype}: {e:.3f}")
    assert all(e <= 1.0 for e in WORST.values())


# ---- hipops.fold_up2x_weights (plain torch: runs here) -------------------------------------------------------------------------------------------
def _fold_weights(dtype, c, nout, kind, seed):
    g = B.gen(seed)
    w = torch.randn(nout, 9 * c, generator=g) / math.sqrt(9 * c)
    if kind == "binades":         # summands spread over ~24 binades, signs mixed: sums that cancel and sums whose small terms only break ties
        w = w * torch.exp2(-torch.randint(0, 25, w.shape, generator=g).float())
    elif kind == "ties":          # small integers times one ulp: many sums are exact rounding ties or one small summand away from one
        w = torch.randint(-2047, 2048, w.shape, generator=g).float() * 2.0 ** -9 + torch.exp2(-torch.randint(10, 30, w.shape, generator=g).float())
    return w.to(dtype)


@pytest.mark.parametrize("dtype", DTS)
@pytest.mark.parametrize("kind", ["plain", "binades", "ties"])
@pytest.mark.parametrize("c,nout", [(64, 8), (128, 136), (192, 40)])
def test_fold_up2x_weights_against_fp64_tap_sums(c, nout, kind, dtype):
    """the tap sums of the 16-bit weights rounded ONCE: within 1 ulp of the fp64 sums everywhere, and bit-equal to their correct rounding wherever the
    fp64 sum is not within 2^-30 (relative) of a rounding tie"""
    from forge_amd import hipops as ops
    wk = _fold_weights(dtype, c, nout, kind, 400 + c + nout)
    got = ops.fold_up2x_weights(wk, c)
    assert got.dtype == dtype and got.shape == (4, nout, 4 * c)
    want = R.fold_up2x_ref(wk, c)
    assert R.excess(got, want, dtype, 1.0, 0.0) <= 1.0
    exact, tie = R.round_to(want, dtype)
    clear = tie > 2.0 ** -30
    assert int(clear.sum()) > 0.5 * clear.numel()       # (exact ties are common among sums of two 16-bit numbers; most sums are clear of them)
    wrong = int((got.double()[clear] != exact[clear]).sum())
    assert wrong == 0, f"{wrong} of {int(clear.sum())} tap sums are not the correctly rounded fp64 sum"


# ---- the 64-query attention kernels (tests/test_gpu_attention_fast.py) ---------------------------------------------------------------------------
# kernel_refs.attn64_emul is the kernels' arithmetic in fp32 torch; it runs on every case of the GPU file in both types, unplanted (must stay inside
# ATTN_TOL) and with one bug planted (must reach 4x on at least one case of the family the bug lives in).
import test_gpu_attention_fast as A  # noqa: E402

_A_CACHE = {}


def _fast(case, dtype):
    """-> (layout, buffers, fp64 reference on the CPU, route at 256 CUs) of a case, built once"""
    key = (case.id, dtype)
    if key not in _A_CACHE:
        L, bufs = A.build(case, dtype)
        _A_CACHE[key] = (L, bufs, A.reference(bufs, L, dev="cpu"), R.attn_route(case.b, case.h, case.nq, case.nk, case.d, 256))
    return _A_CACHE[key]


def _fast_emul(case, dtype, plant=None):
    L, bufs, want, route = _fast(case, dtype)
    q, k, v = A.gather(bufs, L)
    step, split = R.attn_route_emul(route)
    got = R.attn64_emul(q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3), L.nk, L.d ** -0.5, dtype, step=step, split=split, plant=plant)
    return R.excess(got, want, dtype, *R.ATTN_TOL[dtype])


_A_SMALL = [c for c in A.CASES if c.b * c.h * c.nq <= 60000]       # (the three large launches are covered by test_fast_attention_emulation... only)


def test_fast_attention_cases_reach_every_route_at_256_cus():
    """the case list hits every row of the route table, in both types (every case runs in fp16 and bf16), and is listed under the route it reaches"""
    seen = {}
    for c in A.CASES:
        route = R.attn_route(c.b, c.h, c.nq, c.nk, c.d, 256)
        assert route == c.route, f"{c.id}: reaches {route}, listed under {c.route}"
        seen.setdefault(route, []).append(c.id)
    for route in A.ROUTES:
        print(f"ROUTE {route}: {len(seen.get(route, []))} cases x 2 types: {' '.join(seen.get(route, []))}")
    assert set(seen) == set(A.ROUTES)
    for lay, routes in (("unet_self", ("q64v3", "q64v2<64> whole", "q64v2<64> split", "q64v2<64> whole+split")), ("unet_cross", ("short2<2>", "short2<3>")),
                        ("flux", ("ws<128>", "q64v2<128> split", "ws<128>+split tail"))):
        assert {c.route for c in A.CASES if c.layout == lay} == set(routes)
    for route in A.ROUTES:                                             # K pad rows NaN / +-inf on every kernel family
        fam = route.split("<")[0] if route.startswith("short2") else route
        assert any(c.opt.get("kpad") and c.route.startswith(fam) for c in A.CASES), route


def test_attn_route_restates_the_dispatcher():
    """spot values of the rule (csrc/fmx_attention.hip attn_plan) at 256 and at 304 CUs, then kernel_refs.attn_route against the library's own plan
    (fmx_attention_route) over a sweep of shapes; masked, causal, forced-32 and large-span calls are "generic\""""
    assert R.attn_route(16, 20, 1024, 1024, 64, 256) == "q64v2<64> whole"         # 1280 entries = 2.5 rounds: 256 left, more than 3/8 of the slots
    assert R.attn_route(8, 20, 1024, 1024, 64, 256) == "q64v2<64> whole+split"    # 640 = 512 + 128
    assert R.attn_route(16, 10, 4096, 77, 64, 256) == "short2<3>"
    assert R.attn_route(2, 24, 4352, 4352, 128, 256) == "ws<128>+split tail"        # 816 = 3 rounds of 256 + 48
    assert R.attn_route(1, 24, 4352, 4352, 128, 256) == "ws<128>"                  # 408 = 256 + 152: too many left to split
    assert R.attn_route(1, 24, 1024, 1024, 128, 256) == "q64v2<128> split"
    assert R.attn_route(2, 3, 255, 77, 64, 256) == "generic" and R.attn_route(2, 3, 300, 77, 80, 256) == "generic"
    assert R.attn_route(2, 5, 52 * 256 - 37, 250, 64, 304) == "q64v3"              # 520 entries in one round of 608 slots, 520 > 3/8 of them: four whole tiles
    # ... and the restatement against the dispatcher itself: fmx_attention_route runs the library's own plan function on the host
    from forge_amd import _lib
    try:
        lib = _lib.lib()
    except _lib.FmxError as e:
        pytest.skip(f"libfmx not built: {e}")
    checked = 0
    for d in (48, 64, 80, 128, 160):
        for nq in (255, 256, 257, 1000, 4096, 4352):
            for nk in (1, 31, 32, 33, 64, 65, 77, 128, 129, 250, 256, 320, 1024, 4352):
                for b, h in ((1, 1), (2, 3), (8, 20), (16, 20), (1, 24), (2, 24)):
                    for cus in (256, 304):
                        want = R.attn_route(b, h, nq, nk, d, cus)
                        assert A.library_route(lib, A.layout("dense", b, h, nq, nk, d), cus) == want, (d, nq, nk, b, h, cus)
                        checked += 1
                    L = A.layout("dense", b, h, nq, nk, d)
                    assert A.library_route(lib, L, 256, mask=A.FAKE_PTR, mask_qs=L.nk_pad) == "generic"
                    assert A.library_route(lib, L, 256, scale=-(d ** -0.5)) == "generic"
            L = A.layout("dense", 2, 3, nq, nq, d)
            assert A.library_route(lib, L, 256, causal=1) == "generic"
    assert checked == 5 * 6 * 14 * 6 * 2
    # spans that do not fit 32-bit byte offsets: K rows 2^24 elements apart (63 x 2^25 bytes), Q rows 2^22 apart under at most 128 keys (255 x 2^23 bytes)
    for d, nk in ((64, 64), (64, 1024), (128, 1024)):
        L = A.layout("dense", 1, 1, 256, nk, d)
        assert A.library_route(lib, L, 256) != "generic" and A.library_route(lib, L, 256, k_rs=1 << 24) == "generic"
        assert A.library_route(lib, L, 256, vt_ds=1 << 24) == "generic" and A.library_route(lib, L, 256, k_rs=-L.k_rs) == "generic"
    L = A.layout("dense", 1, 1, 256, 77, 64)
    assert A.library_route(lib, L, 256) == "short2<3>" and A.library_route(lib, L, 256, q_rs=1 << 22) == "generic"
    assert A.library_route(lib, A.layout("dense", 1, 1, 256, 129, 64), 256, q_rs=1 << 22) == "q64v3"     # the looped kernels read Q through 64-bit addresses


@pytest.mark.parametrize("dtype", DTS)
def test_fast_attention_emulation_meets_the_tolerance_on_every_case(dtype):
    for c in A.CASES:
        e = _fast_emul(c, dtype)
        fam = "attention " + c.route
        WORST[(fam, dtype)] = max(WORST.get((fam, dtype), 0.0), e)
        assert e <= 1.0, f"{c.id}: the unplanted emulation is {e:.3g}x ATTN_TOL"
        if c.b * c.h * c.nq > 60000:
            _A_CACHE.pop((c.id, dtype), None)
    for (fam, dt), e in sorted(WORST.items(), key=str):
        if fam.startswith("attention ") and dt == dtype:
            print(f"EMULATION {fam} {dtype}: {e:.3f}")


_A_PLANTS = {  # plant -> the cases it has to show on (any one of them reaching 4x is enough)
    "pad_keys_attend": lambda c: c.nk % 64 != 0 and c.structure is None,
    "no_rescale": lambda c: c.structure in ("staircase", "threshold_edge", "dominant") and not c.route.startswith("short2"),
    "never_move": lambda c: c.structure in ("dominant", "dom_upper") and not c.route.startswith("short2"),
    "merge_unweighted": lambda c: c.structure in ("dom_lower", "dom_upper"),
    "split_tail_unmasked": lambda c: "split" in c.route and c.nk % 64 != 0,
}


@pytest.mark.parametrize("dtype", DTS)
@pytest.mark.parametrize("plant", sorted(_A_PLANTS))
def test_fast_attention_planted_bugs_are_caught(plant, dtype):
    """every route family the bug can live in shows it at >= 4x ATTN_TOL on at least one of its cases"""
    cases = [c for c in _A_SMALL if _A_PLANTS[plant](c)]
    fams = {}
    for c in cases:
        fams[c.route] = max(fams.get(c.route, 0.0), _fast_emul(c, dtype, plant))
    print(f"PLANT {plant} {dtype}: " + ", ".join(f"{r} {e:.3g}" for r, e in sorted(fams.items())))
    assert fams and all(e >= TEETH for e in fams.values()), fams


@pytest.mark.parametrize("dtype", DTS)
def test_fast_attention_q_scaled_without_the_second_rounding_is_not_resolved(dtype):
    """Q scaled in fp32 and NOT rounded again (one rounding site fewer than the kernels) stays inside the tolerance on every case: this file cannot tell
    the two apart, the difference is one rounding of Q"""
    worst = max(_fast_emul(c, dtype, "scale_after_rounding") for c in _A_SMALL)
    print(f"PLANT scale_after_rounding {dtype}: worst {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", DTS)
def test_fast_attention_layout_plants_are_caught(dtype):
    """q read from the k half of the q | k buffer; V^T rows taken B * n apart instead of m_tok"""
    for c in (c for c in _A_SMALL if c.layout == "unet_self"):
        L, bufs, want, _ = _fast(c, dtype)
        bites(A.reference(bufs, L, dev="cpu", q_from_k=True), want, dtype, R.ATTN_TOL[dtype], f"{c.id}: q from the k half")
        bites(A.reference(bufs, L, dev="cpu", vt_ds=L.vt_ds_wrong), want, dtype, R.ATTN_TOL[dtype], f"{c.id}: vt_ds = B * n")


@pytest.mark.parametrize("dtype", DTS)
def test_fast_attention_stores_outside_the_window_trip_the_sentinel_rule(dtype):
    """a correct scatter leaves the surroundings alone; rows [nq, l_pad) written (O addressed as if every image had l_pad queries) and one 16-byte
    store past the column window each change sentinel elements"""
    for c in (c for c in _A_SMALL if c.layout != "dense"):
        L, bufs, want, _ = _fast(c, dtype)
        after = bufs["o"].clone()
        A._view(after, L, "o", L.nq)[:] = want.permute(0, 2, 1, 3).to(dtype)
        assert A.window_violations(bufs["o"], after, L) == 0
        if c.layout == "flux":
            spill = after.clone()
            A._view(spill, L, "o", L.nk_pad)[:, L.nq:] = 0.5
            assert A.window_violations(bufs["o"], spill, L) == (L.nk_pad - L.nq) * L.b * L.h * L.d
        else:
            spill = after.clone()
            at = L.o_off + (L.nq - 1) * L.o_rs + L.h * L.d           # the 8 elements behind the last window column of image 0's last row
            spill[at:at + min(8, L.o_rs - L.h * L.d)] = 0.5
            assert A.window_violations(bufs["o"], spill, L) == min(8, L.o_rs - L.h * L.d)
            if L.o_rs - L.h * L.d < 8:                                 # the rest of a 16-byte store lands in the next row's window: values must catch it
                spill[at:at + 8] = 0.5
                got = A._view(spill, L, "o", L.nq).permute(0, 2, 1, 3)
                assert R.excess(got, want, dtype, *R.ATTN_TOL[dtype]) >= TEETH


# ---- the sampler-step kernels (tests/test_gpu_sampler_kernels.py) ---------------------------------------------------------------------------------
# The emulations of kernel_refs (the kernels' formulas in plain fp32 torch) run on every case of the GPU file: unplanted they stay inside the derived
# bound (worst excess printed: the table beside the bounds in kernel_refs.py), with one bug planted they leave it by >= 4x; the bit-exact checks see >= 4
# differing elements.
import numpy as np  # noqa: E402

import test_gpu_sampler_kernels as K  # noqa: E402


def _report(kernel, worst):
    print(f"EMULATION {kernel}: {worst:.3f}")
    assert worst <= 1.0, f"{kernel}: the unplanted fp32 emulation is {worst:.3g}x the derived bound"


def _bites_abs(planted, want, bound, what):
    e = R.excess_abs(planted, want, bound)
    assert e >= TEETH, f"{what}: the planted bug is only {e:.3g}x the bound"


def test_sampler_windows_are_aligned_and_surrounded():
    """condition of the GPU file: every window starts on a 16-byte boundary of its buffer and has surroundings on both sides"""
    wins = list(K.pack_case(0)[:2]) + [K.im2col_case(0, BF)] + list(K.cfg_case(2, 3, 3)) + list(K.step_case(3)) + K.lincomb_case(5) + list(K.errnorm_case(257, "mixed"))
    wins += [K.Out((5,), torch.float32, 2, 1), K.Out((7, 64), H16, 3, 2)]
    for w in wins:
        assert (w.lead * w.buf.element_size()) % 16 == 0 and w.lead > 0 and w.buf.numel() > w.lead + w.n
        assert w.values.is_contiguous() and w.values.data_ptr() % 16 == w.buf.data_ptr() % 16


def test_sampler_pack_input_emulation_and_planted_bugs():
    worst = 0.0
    for i in range(len(K.PACK_SHAPES)):
        x, sigma, reps = K.pack_case(i)
        for sd in K.SIGMA_DATAS:
            want = R.pack_input_ref(x.values, sigma.values, sd, reps)
            worst = max(worst, R.excess(R.pack_input_emul(x.values, sigma.values, sd, reps), want, H16, *R.ELEM_TOL[H16]))
            plants = ["kykx", "sd2_dropped"] + (["ch_major"] if x.shape[1] > 1 else []) + (["sigma_of_image0"] if x.shape[0] > 1 else [])
            if x.shape[2] == 1:
                plants.remove("kykx")      # one pixel: only the centre tap is inside the image
            for plant in plants:
                bites(R.pack_input_emul(x.values, sigma.values, sd, reps, plant), want, H16, R.ELEM_TOL[H16], f"pack {K.PACK_SHAPES[i]} sd {sd} {plant}")
            e = R.excess(R.pack_input_emul(x.values, sigma.values, sd, reps, "sd_not_squared"), want, H16, *R.ELEM_TOL[H16])
            assert e >= TEETH if sd != 1.0 else e <= 1.0, f"sigma_data not squared at sigma_data {sd}: {e:.3g}"      # has teeth only away from 1
    _report("unet_pack_input", worst)


def test_sampler_im2col_planted_bugs_are_caught():
    for i in range(len(K.IM2COL_SHAPES)):
        n, h, w, c, ldx = K.IM2COL_SHAPES[i]
        for dtype in DTS:
            x = K.im2col_case(i, dtype).values
            want = R.im2col_smallc_ref(x, c).view(torch.int16)
            assert not bool((want == x.new_tensor(30000.0).view(torch.int16)).any())      # the padding channels never appear
            dense = x.reshape(-1)[:n * h * w * c].view(n, h, w, c)                         # ldx taken as c
            if ldx != c and n * h * w > 1:
                assert int((R.im2col_smallc_ref(dense, c).view(torch.int16) != want).sum()) >= TEETH
            if h > 1:                                                                       # ky / kx transposed
                t = R._pack_rows(R._taps(x.view(torch.int16)[..., :c].permute(0, 3, 1, 2), transposed=True), 1)
                assert int((t != want).sum()) >= TEETH
            through_float = R._pack_rows(R._taps(x.float()[..., :c].permute(0, 3, 1, 2)), 1).to(dtype).view(torch.int16)
            assert bool((through_float == want).all())                                      # (the reference moves words; the values agree)


def _cfg_all():
    for ptype in K.PTYPES:
        for reps in (1, 2):
            for sd in K.SIGMA_DATAS:
                for c, ld in K.CFG_GEOS:
                    for cs in K.COND_SCALES:
                        eps, x, sigma = K.cfg_case(reps, c, ld)
                        yield (ptype, reps, sd, c, ld, cs), (eps.values, x.values, sigma.values, reps, cs, ptype, sd)


def test_sampler_cfg_combine_emulation_meets_the_bounds_on_every_case():
    worst = {"denoised": 0.0, "preds": 0.0}
    for key, args in _cfg_all():
        den, dc, du, b_den, b_c, b_u = R.cfg_combine_ref(*args)
        g_den, g_c, g_u = R.cfg_combine_emul(*args)
        worst["denoised"] = max(worst["denoised"], R.excess_abs(g_den, den, b_den))
        worst["preds"] = max(worst["preds"], R.excess_abs(g_c, dc, b_c))
        if args[3] == 2:
            worst["preds"] = max(worst["preds"], R.excess_abs(g_u, du, b_u))
        else:
            assert not bool(g_u.any()) and not bool(du.any())
    _report("cfg_combine denoised", worst["denoised"])
    _report("cfg_combine preds", worst["preds"])


def test_sampler_cfg_combine_planted_bugs_are_caught():
    """halves swapped, cond_pred <-> uncond_pred, the EDM sign on v_prediction (and the reverse), sigma_data^2 missing from A (teeth only at sigma_data 0.5:
    at 1.0 the planted emulation is asserted to PASS), ld_eps taken as c, eps indexed as NCHW"""
    for key, args in _cfg_all():
        ptype, reps, sd, c, ld, cs = key
        den, dc, du, b_den, b_c, b_u = R.cfg_combine_ref(*args)
        plant = lambda p: R.cfg_combine_emul(*args, plant=p)  # noqa: E731
        if reps == 2:
            if cs != 0.5:         # (at 0.5 the combination is symmetric in the halves; not among the cases)
                _bites_abs(plant("halves_swapped")[0], den, b_den, f"{key} halves swapped")
            _bites_abs(plant("preds_swapped")[1], dc, b_c, f"{key} cond_pred <- uncond_pred")
            _bites_abs(plant("preds_swapped")[2], du, b_u, f"{key} uncond_pred <- cond_pred")
        if ptype != "epsilon":
            _bites_abs(plant("edm_sign")[1], dc, b_c, f"{key} the other prediction type's sign")
            e = R.excess_abs(plant("no_sd2_in_a")[1], dc, b_c)
            assert e >= TEETH if sd != 1.0 else e <= 1.0, f"{key} sigma_data^2 missing from A: {e:.3g}"
            if cs != 0.0 or reps == 2:
                e = R.excess_abs(plant("no_sd2_in_a")[0], den, b_den)
                assert e >= TEETH if sd != 1.0 else e <= 1.0, f"{key} sigma_data^2 missing from A (denoised): {e:.3g}"
        if ld != c:
            _bites_abs(plant("ld_as_c")[1], dc, b_c, f"{key} ld_eps taken as c")
        _bites_abs(plant("eps_nchw")[1], dc, b_c, f"{key} eps indexed as NCHW")


def test_sampler_euler_and_lincomb3_emulation_and_planted_bugs():
    worst = {"euler_step": 0.0, "lincomb3": 0.0}
    for n in K.STEP_NS:
        x, den, old, noise = (w.values for w in K.step_case(n))
        for sigma, sigma_next in K.EULER_STEPS:
            for ns in K.EULER_NOISE:
                nz = None if ns is None else noise
                want, bound = R.euler_step_ref(x, den, sigma, sigma_next, nz, ns or 0.0)
                worst["euler_step"] = max(worst["euler_step"], R.excess_abs(R.euler_step_emul(x, den, sigma, sigma_next, nz, ns or 0.0), want, bound))
                _bites_abs(R.euler_step_emul(x, den, sigma, sigma_next, nz, ns or 0.0, plant="dt_sign"), want, bound, f"euler n {n} {sigma} dt sign")
                if nz is not None:
                    _bites_abs(R.euler_step_emul(x, den, sigma, sigma_next, nz, ns, plant="noise_before_scale"), want, bound, f"euler n {n} {sigma} noise first")
        for a, b, c, has_old in K.LINCOMB3_COEFS:
            want, bound = R.lincomb3_ref(x, den, old if has_old else None, a, b, c)
            worst["lincomb3"] = max(worst["lincomb3"], R.excess_abs(R.lincomb3_emul(x, den, old if has_old else None, a, b, c), want, bound))
            _bites_abs(R.lincomb3_emul(den, x, old if has_old else None, a, b, c), want, bound, f"lincomb3 n {n} x and denoised exchanged")
            if has_old and c != 0.0:
                _bites_abs(R.lincomb3_emul(x, den, None, a, b, c), want, bound, f"lincomb3 n {n} old_denoised dropped")
    for k, e in worst.items():
        _report(k, e)


def test_sampler_lincomb_emulation_and_planted_bugs():
    worst = 0.0
    for n in K.LINCOMB_NS:
        srcs = [w.values for w in K.lincomb_case(n)]
        sentinel = K.Out((n,), torch.float32).values
        for name, coefs in K.LINCOMB_COEFS.items():
            for k in range(1, 9):
                want, bound = R.lincomb_ref(srcs[:k], coefs[:k])
                worst = max(worst, R.excess_abs(R.lincomb_emul(srcs[:k], coefs[:k]), want, bound))
                if n % 4:      # the scalar tail behind the last full float4 left unwritten: into a fresh destination, and in place on source 0
                    _bites_abs(R.lincomb_emul(srcs[:k], coefs[:k], "tail_unwritten", sentinel), want, bound, f"lincomb n {n} terms {k} {name} tail")
                    if not (k == 1 and coefs[0] == 1.0):
                        _bites_abs(R.lincomb_emul(srcs[:k], coefs[:k], "tail_unwritten", srcs[0]), want, bound, f"lincomb n {n} terms {k} {name} tail in place")
                if k >= 2:
                    _bites_abs(R.lincomb_emul(srcs[:k], coefs[:k], "coef_shift"), want, bound, f"lincomb n {n} terms {k} {name} coefficients shifted")
    _report("lincomb", worst)


def test_sampler_error_norm_emulation_and_planted_bugs():
    worst = 0.0
    for n in K.ERRNORM_NS:
        rel = R.error_norm_rel_bound(n)
        for kind in K.ERRNORM_KINDS:
            lo, hi, pv = (w.values for w in K.errnorm_case(n, kind))
            want = R.error_norm_ref(lo, hi, pv, K.ERR_ATOL, K.ERR_RTOL)
            got = R.error_norm_emul(lo, hi, pv, K.ERR_ATOL, K.ERR_RTOL)
            if kind == "equal":
                assert want == 0.0 and got == 0.0
                continue
            worst = max(worst, abs(got - want) / (rel * want))
            ex = lambda p: abs(R.error_norm_emul(lo, hi, pv, K.ERR_ATOL, K.ERR_RTOL, p) - want) / (rel * want)  # noqa: E731
            if n > 1:
                assert ex("div_n") >= TEETH, (n, kind, "div_n")
            if kind == "mixed" and n >= 255:
                assert ex("prev_ignored") >= TEETH, (n, kind, "prev_ignored")
            if kind == "last_heavy":
                last = ((hi[-1].double() - lo[-1].double()) / R.f32(K.ERR_ATOL)) ** 2 / n
                assert last > 0.5 * want * want, "the last element does not carry most of the norm"
                if n % 256:
                    assert ex("last_block_dropped") >= TEETH, (n, kind, "last_block_dropped")
    # both sides of max(atol, rtol * max(|lo|, |prev|)) are exercised, and x_prev decides on a good part of the elements
    lo, hi, pv = (w.values for w in K.errnorm_case(65537, "mixed"))
    rel_side = R.f32(K.ERR_RTOL) * torch.maximum(lo.abs(), pv.abs()) > R.f32(K.ERR_ATOL)
    assert 0.2 < float(rel_side.float().mean()) < 0.8 and float((pv.abs() > lo.abs()).float().mean()) > 0.3
    _report("error_norm", worst)


def test_sampler_philox_planted_bugs_are_caught():
    """the high seed word ignored; the offset placed in counter word 1 -- on the seeds and offsets of the GPU file"""
    hi_seed = [s for s in K.PHILOX_SEEDS if s >> 32]
    assert hi_seed and 0 in K.PHILOX_OFFSETS and 2 ** 32 - 1 in K.PHILOX_OFFSETS
    for n in K.PHILOX_NS:
        for seed in hi_seed:
            for offset in K.PHILOX_OFFSETS:
                want = R.philox_raw_ref(seed, offset, n)
                assert int((R.philox_raw_ref(seed, offset, n, "seed_hi_ignored") != want).sum()) >= TEETH
                if offset:
                    assert int((R.philox_raw_ref(seed, offset, n, "offset_in_word1") != want).sum()) >= TEETH
    # the reference agrees with the project's own Philox restatement and its known-answer route (oracle/rng.py philox_randn uses the same words)
    from oracle.rng import philox_randn
    raw = R.philox_raw_ref(K.PHILOX_SEEDS[0], 7, 257).astype(np.float32)
    inv = np.float32(2.3283064e-10)
    u, v = raw[:, 0] * inv + inv / 2, raw[:, 1] * np.float32(2.3283064e-10 * 6.2831855) + np.float32(2.3283064e-10 * 6.2831855) / 2
    np.testing.assert_allclose(np.sqrt(-2.0 * np.log(u)) * np.sin(v), philox_randn(K.PHILOX_SEEDS[0], 7, 257), rtol=0, atol=1e-6)


# ---- the GroupNorm statistics chain (tests/test_gpu_groupnorm_routes.py) --------------------------------------------------------------------------
# kernel_refs.chunk_sums_emul (fp32 records per chunk) and gn_fold_emul2 / gn_apply_emul (both folds of fmx_groupnorm_apply in plain torch) run on the GPU
# file's own inputs: unplanted they stay inside the GPU file's tolerances (worst excess printed: the table in kernel_refs.py), with one bug planted they
# leave them by >= 4x.
import test_gpu_groupnorm_routes as N  # noqa: E402

_DT_NAME = {H16: "f16", BF: "bf16"}


def _stat_bites(planted, want, what):
    e = R.stat_excess(planted, want, **N.STAT_TOL)
    assert e >= TEETH, f"{what}: the planted bug is only {e:.3g}x the statistics tolerance"


@pytest.mark.parametrize("dtype", DTS)
def test_gn_routes_producer_chunking_emulation_and_planted_bugs(dtype):
    """every producer case at every chunk count its routes can report: fp32 records per chunk stay inside STAT_TOL; the last 128-row chunk dropped, and a
    chunk in the next image's slot, are caught per chunk AND in the sum over chunks"""
    worst = 0.0
    for form, nout, tall, dt in N.PRODUCER_CASES:
        if N.DTYPES[dt] != dtype:
            continue
        k = N.producer_case(form, dtype, nout, tall)
        stored = N.producer_ref(form, dtype, nout, tall).to(dtype)
        assert N.expected_chunks(1, k.n, k.hw) == [k.hw // 128] and N.expected_chunks(3, k.n, k.hw) == [N.ops._gn_chunks(k.n, k.hw)]
        for nch in N.expected_chunks(0, k.n, k.hw):
            worst = max(worst, R.stat_excess(R.chunk_sums_emul(stored, k.n, nch), R.chunk_sums_ref(stored, k.n, nch), **N.STAT_TOL))
        nch = k.hw // 128
        want = R.chunk_sums_ref(stored, k.n, nch)
        for plant in ("last_chunk_dropped", "next_image_slot"):
            planted = R.chunk_sums_emul(stored, k.n, nch, plant)
            _stat_bites(planted, want, f"{N.case_id(form, nout, tall, dt)} {plant}, per chunk")
            _stat_bites(planted.sum(1), want.sum(1), f"{N.case_id(form, nout, tall, dt)} {plant}, summed over chunks")
    print(f"EMULATION gn producer records {dtype}: {worst:.3f}")
    assert worst <= 1.0


def test_gn_routes_expected_chunks_table():
    """the route table of the GPU file at its two image sizes: 128-row tiles hw / 128, 256-row tiles hw / 256, the 512-row tile hw / 512 where it divides, the
    fallback count elsewhere -- and every epilogue count differs from the fallback count, so the chunk count does identify the route"""
    for hw, fb in ((256, 8), (512, 16)):
        assert N.ops._gn_chunks(N.N_IMG, hw) == fb
        for tile in N.TILES:
            want = hw // 128 if tile in (1, 2, 11, 12, 13) else hw // 256 if tile in (6, 7) else 1 if tile == 9 and hw == 512 else fb
            if tile:
                assert N.expected_chunks(tile, N.N_IMG, hw) == [want]
        assert fb not in (hw // 128, hw // 256, hw // 512) and set(N.expected_chunks(0, N.N_IMG, hw)) == {fb, hw // 128, hw // 256} | ({1} if hw == 512 else set())


@pytest.mark.parametrize("dtype", DTS)
def test_gn_routes_stats_pass_emulation_and_stale_empty_chunks(dtype):
    """fp32 records of the stand-alone pass on every case stay inside STAT_TOL; a chunk behind the image that keeps an earlier record is caught (the GPU test
    asks for exact zeros there; the tolerance alone sees it too)"""
    worst = 0.0
    for c, hw, nch in N.STATS_CASES:
        x = N.stats_case(c, hw, dtype).values
        want = R.chunk_sums_ref(x, N.STATS_N, nch)
        worst = max(worst, R.stat_excess(R.chunk_sums_emul(x, N.STATS_N, nch), want, **N.STAT_TOL))
        per = -(-hw // nch)
        if -(-hw // per) < nch:
            planted = R.chunk_sums_emul(x, N.STATS_N, nch, "empty_chunk_stale")
            assert bool(planted[:, -(-hw // per):].any()) and not bool(want[:, -(-hw // per):].any())
            _stat_bites(planted, want, f"c {c} hw {hw} nchunks {nch} stale empty chunk")
    print(f"EMULATION gn stand-alone pass records {dtype}: {worst:.3f}")
    assert worst <= 1.0


def _apply_all(dtype):
    for name, hw in N.APPLY_IDS:
        for eps in (1e-5, 1e-6):
            yield name, hw, eps, N.apply_case(name, hw, dtype)


@pytest.mark.parametrize("dtype", DTS)
def test_gn_routes_fold_emulations_meet_the_tolerances(dtype):
    """both folds in plain torch on every case of the GPU file: the output inside GN_TOL, the separate fold's table at or below the MEASURED figure
    kernel_refs.GN_TABLE_EMUL, a quarter of the tolerance (printed: the worst relative error, the figure recorded beside the constant)"""
    worst = {"fused fold": 0.0, "separate fold": 0.0, "table": 0.0}
    for name, hw, eps, k in _apply_all(dtype):
        srcs, nchs = N.apply_sources(k)
        fused, groups = k.cfg["fused"], k.cfg["groups"]
        assert N.apply_fuses(k.cfg, k.n, hw) == fused
        table = R.gn_fold_emul2(srcs, nchs, k.gamma.values, k.beta.values, R.f32(eps), groups, fused)
        if not fused:
            worst["table"] = max(worst["table"], R.gn_table_excess(table, k.x.view(k.n, hw, k.c), k.gamma.values, k.beta.values, R.f32(eps), groups, tol=1.0))
        for silu in (False, True):
            y = R.gn_apply_emul(k.x.view(k.n, hw, k.c), table, silu, dtype).reshape(k.n * hw, k.c)
            key = "fused fold" if fused else "separate fold"
            worst[key] = max(worst[key], R.excess(y, N.apply_ref(name, hw, dtype, eps, silu), dtype, *R.GN_TOL[dtype]))
    print(f"EMULATION gn output, fused fold {dtype}: {worst['fused fold']:.3f}")
    print(f"EMULATION gn output, separate fold {dtype}: {worst['separate fold']:.3f}")
    print(f"EMULATION gn scale/shift table {dtype}: worst relative error {worst['table']:.3g} = {worst['table'] / R.GN_TABLE_TOL:.3f}x GN_TABLE_TOL")
    assert worst["fused fold"] <= 1.0 and worst["separate fold"] <= 1.0
    assert worst["table"] <= R.GN_TABLE_EMUL and R.GN_TABLE_TOL == 4 * R.GN_TABLE_EMUL


@pytest.mark.parametrize("dtype", DTS)
def test_gn_routes_fold_planted_bugs_are_caught(dtype):
    """source 1 folded with source 0's chunk count (the cases whose counts differ); the straddling group losing source 0's last channel; eps 1e-5 used for
    1e-6 -- each >= 4x GN_TOL on the output of every case it applies to, and >= 4x GN_TABLE_TOL on the table where the separate fold runs"""
    for name, hw, eps, k in _apply_all(dtype):
        srcs, nchs = N.apply_sources(k)
        fused, groups, c0 = k.cfg["fused"], k.cfg["groups"], k.cfg["c0"]
        plants = []
        if len(srcs) == 2 and nchs[0] != nchs[1] and hw >= nchs[1]:     # (one pixel in three chunks: the records that the wrong stride reaches are the empty ones)
            plants.append("nch1_as_nch0")
        if len(srcs) == 2 and c0 % (k.c // groups) != 0:
            plants.append("straddle_off_by_one")
        if eps == 1e-6:
            plants.append("eps_1e5")
        for plant in plants:
            table = R.gn_fold_emul2(srcs, nchs, k.gamma.values, k.beta.values, R.f32(eps), groups, fused, plant)
            for silu in (False, True):
                y = R.gn_apply_emul(k.x.view(k.n, hw, k.c), table, silu, dtype).reshape(k.n * hw, k.c)
                bites(y, N.apply_ref(name, hw, dtype, eps, silu), dtype, R.GN_TOL[dtype], f"{name} hw {hw} eps {eps} silu {silu} {plant}")
            if not fused:
                e = R.gn_table_excess(table, k.x.view(k.n, hw, k.c), k.gamma.values, k.beta.values, R.f32(eps), groups)
                assert e >= TEETH, f"{name} hw {hw} eps {eps} {plant}: the planted table is only {e:.3g}x GN_TABLE_TOL"


def test_gn_routes_case_list_reaches_both_folds_and_every_lane_layout():
    """conditions of the GPU file: both folds are reached, for both reasons the launcher has for the separate one; a group straddles the sources in a fused and
    in a separate case; the stand-alone pass sees idle threads, one lane per octet and a second octet block, and chunk counts beyond the pixel count"""
    fused = {name: cfg["fused"] for name, cfg in N.APPLY_CASES.items()}
    assert sorted(fused.values()) == [False, False, True, True]
    for name, cfg in N.APPLY_CASES.items():
        for hw in cfg["hws"]:
            assert N.apply_fuses(cfg, N.APPLY_N, hw) == cfg["fused"]
        c = cfg["c0"] + cfg["c1"]
        ppb = -(-8192 // c)
        assert 1 in cfg["hws"] and any(hw > ppb and hw % ppb for hw in cfg["hws"])
    assert N.APPLY_CASES["separate_records"]["groups"] == 32 and N.APPLY_CASES["separate_groups"]["groups"] != 32
    assert N.APPLY_CASES["fused_wide"]["c0"] // 8 > 256
    for name in ("fused_straddle", "separate_groups"):
        cfg = N.APPLY_CASES[name]
        assert cfg["c0"] % ((cfg["c0"] + cfg["c1"]) // cfg["groups"]) != 0 and cfg["nch0"] != cfg["nch1"]
    octs = [c // 8 for c in N.STATS_C]
    assert any(o < 256 and 256 % o for o in octs) and 256 in octs and any(o > 256 for o in octs) and 1 in octs
    assert all(any(nch > hw for c, h, nch in N.STATS_CASES if h == hw) for hw in N.STATS_HW)


# ---- the token-path row norms and the q/k norm + rope kernel (tests/test_gpu_token_kernels.py) -----------------------------------------------------
# kernel_refs.ln_emul / rmsnorm_emul / qk_norm_rope_emul (the kernels' arithmetic in plain fp32 torch) run on every case of the GPU file: unplanted they stay
# inside LN_TOL / RMS_TOL / ROPE_TOL (worst excess printed: the table in kernel_refs.py), every planted bug leaves the tolerance by >= 4x on the cases named
# for it, and no fp64 reference leaves the range of the output type.
import test_gpu_token_kernels as T  # noqa: E402


def _finite(want, dtype, what):
    assert bool(torch.isfinite(want.to(dtype)).all()), f"{what}: the fp64 reference overflows {dtype}"


def _plant_report(kernel, dtype, worst, plants):
    """worst: the unplanted emulation's worst excess; plants: {plant: (its SMALLEST excess over the cases it has to show on, that case)}"""
    print(f"EMULATION {kernel} {_DT_NAME[dtype]}: {worst:.3f}")
    assert worst <= 1.0, f"{kernel} {dtype}: the unplanted fp32 emulation is {worst:.3g}x the tolerance"
    for plant, (e, case) in plants.items():
        print(f"PLANT {kernel} {_DT_NAME[dtype]} {plant}: {e:.3g} ({case})")
        assert e >= TEETH, f"{kernel} {dtype} {plant}: the planted bug is only {e:.3g}x the tolerance on {case}"


def _weakest(plants, plant, e, case):
    if e < plants.get(plant, (math.inf, None))[0]:
        plants[plant] = (e, case)


def _has_small_row(idx):
    return T.SMALL_PAIR in idx


@pytest.mark.parametrize("dtype", DTS)
def test_token_layernorm_emulation_and_planted_bugs(dtype):
    """eps outside the root shows ONLY on rows of spread 1e-3 (variance ~ eps): it must bite on every table that has such a row.  The last octet left out of the
    statistics must bite at every width on every table of 5 rows or more (at c = 8 nothing is left to sum)"""
    worst, plants = {"layernorm": 0.0, "layernorm_padded": 0.0}, {}
    cases = [(f"layernorm rows={rows},c={c}", T.ln_case(rows, c, dtype), T.ln_want(rows, c, dtype), T.pair_of_row(rows, T.LN_C.index(c))) for rows, c in T.LN_CASES]
    cases += [(f"layernorm_padded c={c}", T.pad_case(c, dtype), T.pad_want(c, dtype), T.pair_of_row(T.PAD_B * T.PAD_N, c % 7)) for c in T.PAD_C]
    for what, (x, gamma, beta), want, idx in cases:
        _finite(want, dtype, what)
        eps = R.f32(T.LN_EPS)
        worst[what.split()[0]] = max(worst[what.split()[0]], R.excess(R.ln_emul(x, gamma, beta, eps, dtype), want, dtype, *R.LN_TOL[dtype]))
        e = R.excess(R.ln_emul(x, gamma, beta, eps, dtype, plant="last_octet_skipped"), want, dtype, *R.LN_TOL[dtype])
        if x.shape[0] >= 5:
            assert e >= TEETH, f"{what}: last octet skipped is only {e:.3g}x"
            _weakest(plants, "last_octet_skipped", e, what)
            assert torch.equal(want[T.CONST_ROW], beta.double()) and torch.equal(want[T.ZERO_ROW], beta.double())      # a constant row's result is beta
        e = R.excess(R.ln_emul(x, gamma, beta, eps, dtype, plant="eps_outside_sqrt"), want, dtype, *R.LN_TOL[dtype])
        if _has_small_row(idx) and not (x.shape[0] >= 5 and idx.index(T.SMALL_PAIR) in (T.CONST_ROW, T.ZERO_ROW) and idx.count(T.SMALL_PAIR) == 1):
            assert e >= TEETH, f"{what}: eps outside the root is only {e:.3g}x although the table has a row of spread 1e-3"
            _weakest(plants, "eps_outside_sqrt", e, what)
    _plant_report("layernorm_padded", dtype, worst["layernorm_padded"], {})
    _plant_report("layernorm", dtype, worst["layernorm"], plants)
    assert set(plants) == {"last_octet_skipped", "eps_outside_sqrt"}


@pytest.mark.parametrize("dtype", DTS)
def test_token_layernorm_mod_emulation_and_planted_bugs(dtype):
    """every MOD plant must bite on EVERY case: the vectors differ per batch and between scale and shift, and 1 + scale differs from scale everywhere"""
    worst, plants = 0.0, {}
    for c, rpb, win in T.MOD_CASES:
        what = f"layernorm_mod c={c},rows_per_batch={rpb},window={win}"
        x, mods, sc, sh = T.mod_case(c, rpb, win, dtype)
        scale, shift = T.mod_vectors(mods, c, sc, sh)
        want = T.mod_want(c, rpb, win, dtype)
        _finite(want, dtype, what)
        assert (T.MOD_B * rpb) % 4 != 0 or rpb % 4 != 0                                        # blocks of four rows straddle the batches
        assert float((1.0 + scale[T.MOD_NEG_BATCH, :c // 4].double()).abs().max()) < 0.02       # the quarter where the floor is what holds
        eps = R.f32(T.MOD_EPS)
        worst = max(worst, R.excess(R.ln_emul(x, scale, shift, eps, dtype, rows_per_batch=rpb), want, dtype, *R.LN_TOL[dtype]))
        for plant in ("eps_outside_sqrt", "scale_shift_swapped", "batch0_vectors", "one_plus_dropped", "last_octet_skipped"):
            e = R.excess(R.ln_emul(x, scale, shift, eps, dtype, rows_per_batch=rpb, plant=plant), want, dtype, *R.LN_TOL[dtype])
            assert e >= TEETH, f"{what} {plant}: only {e:.3g}x"
            _weakest(plants, plant, e, what)
        # the wrong chunk of the buffer (6e4 everywhere) in place of scale
        for k in [k for k in range(T.MOD_WINDOWS[win][0]) if k not in (sc, sh)][:1]:
            e = R.excess(R.ln_emul(x, mods[:, k * c:(k + 1) * c], shift, eps, dtype, rows_per_batch=rpb), want, dtype, *R.LN_TOL[dtype])
            assert e >= TEETH, f"{what}: scale read from chunk {k} is only {e:.3g}x"
    _plant_report("layernorm_mod", dtype, worst, plants)


@pytest.mark.parametrize("dtype", DTS)
def test_token_rmsnorm_emulation_and_planted_bugs(dtype):
    """eps outside the root shows only on rows of scale <~ 1e-2 (mean square ~ eps): every table with more than one row has one, and the one-row tables at
    scale 1e-3.  The mean subtracted and the last octet left out of the sum must show wherever a row has its outlier channel, which sits in the last octet
    (eight ordinary channels out of 4096 move rstd by 0.1%: a quarter of a bf16 ulp, so without the outlier the wide bf16 rows could not show it)"""
    worst, plants = 0.0, {}
    for rows, c in T.RMS_CASES:
        what = f"rmsnorm rows={rows},c={c}"
        x, w = T.rms_case(rows, c, dtype)
        want = T.rms_want(rows, c, dtype)
        _finite(want, dtype, what)
        scales = T.rms_scales(rows, c)
        eps = R.f32(T.RMS_EPS)
        worst = max(worst, R.excess(R.rmsnorm_emul(x, w, eps, dtype), want, dtype, *R.RMS_TOL[dtype]))
        if rows >= 5:
            assert scales.count(0.0) == 1 and not bool(want[scales.index(0.0)].any()) and max(scales) > 299.0 and 0.0 < min(s for s in scales if s) < 1.1e-3
        for plant in ("mean_subtracted", "eps_outside_sqrt", "last_octet_skipped"):
            e = R.excess(R.rmsnorm_emul(x, w, eps, dtype, plant=plant), want, dtype, *R.RMS_TOL[dtype])
            must = {"mean_subtracted": max(scales) > 299.0, "eps_outside_sqrt": 0.0 < min(s for s in scales if s) < 1e-2, "last_octet_skipped": max(scales) > 299.0}[plant]
            if must:
                assert e >= TEETH, f"{what} {plant}: only {e:.3g}x"
                _weakest(plants, plant, e, what)
    _plant_report("rmsnorm", dtype, worst, plants)
    assert len(plants) == 3


_ROPE_ALL_CASES = ("sin_sign", "half_split", "k_uses_q_scale", "eps_outside_sqrt")


@pytest.mark.parametrize("dtype", DTS)
def test_token_qk_norm_rope_emulation_and_planted_bugs(dtype):
    """the sign of sin, the rotate-half convention and k normalised with q's scale must bite on every launch of every case; eps outside the root shows ONLY on
    token rows of magnitude <~ 1e-2 and must bite on every launch that has one (all with more than 8 tokens in the batch); pe[t] for pe[row_off + t] on every
    launch with row_off > 0; one RMS per token over all heads shows through the heads' own chi-square spread (~6% of an element) on every launch with more
    than one token"""
    worst, plants = 0.0, {}
    for name, (b, h, l_pad, launches, window) in T.ROPE_CASES.items():
        pe, Ls = T.rope_case(name, dtype)
        eps = R.f32(T.ROPE_EPS)
        for L, (wq, wk) in zip(Ls, T.rope_want(name, dtype)):
            what = f"{name} tokens={L['tokens']}@{L['row_off']}"
            _finite(wq, dtype, what)
            _finite(wk, dtype, what)
            args = (L["qkv"], L["qs"], L["ks"], pe, b, L["tokens"], h, L["row_off"], eps, dtype)

            def ex(plant=None):
                q, k = R.qk_norm_rope_emul(*args, plant=plant)
                return max(R.excess(q, wq, dtype, *R.ROPE_TOL[dtype]), R.excess(k, wk, dtype, *R.ROPE_TOL[dtype]))

            worst = max(worst, ex())
            rms = L["qkv"].double().pow(2).mean(-1).sqrt()
            must = {p: True for p in ("sin_sign", "half_split", "k_uses_q_scale")}
            must["eps_outside_sqrt"] = bool(((rms > 0) & (rms < 1e-2)).any())
            must["row_off_dropped"] = L["row_off"] > 0
            must["rms_over_all_heads"] = b * L["tokens"] > 2
            for plant, m in must.items():
                if m:
                    e = ex(plant)
                    assert e >= TEETH, f"{what} {plant}: only {e:.3g}x"
                    _weakest(plants, plant, e, what)
            if window:
                assert L["qkv"].stride(0) == 3 * h * T.D + T.ROPE_WINDOW[1] and float(L["buf"][0, 0]) > 5e4 and float(L["buf"][0, -1]) > 5e4
    _plant_report("flux_qk_norm_rope", dtype, worst, plants)
    assert len(plants) == 6


def test_token_rope_cases_reach_every_store_path():
    """conditions of the GPU file, from the kernel's store rule restated (a 32-token half is stored as four 16-byte vectors iff it is full and its first column
    is a multiple of 8 elements, else element by element): the case list has vector halves, FULL halves on the scalar path at 8-byte and at 2-byte alignment,
    ragged halves, empty halves, and pad columns behind the last token; the rope ids differ for every token"""
    seen = set()
    for name, (b, h, l_pad, launches, window) in T.ROPE_CASES.items():
        for tokens, row_off in launches:
            assert l_pad >= row_off + tokens
            for bi in range(b):
                for t0 in range(0, tokens, 64):
                    for half in (0, 1):
                        valid = min(32, tokens - (t0 + half * 32))
                        col = bi * l_pad + row_off + t0 + half * 32
                        align = 8 if col % 8 == 0 else 4 if col % 4 == 0 else 1
                        seen.add(("empty",) if valid <= 0 else ("full" if valid == 32 else "ragged", align))
        covered = max(t + o for t, o in launches)
        seen.add(("pad", l_pad > covered))
    assert {("full", 8), ("full", 4), ("full", 1), ("ragged", 8), ("ragged", 1), ("empty",), ("pad", True), ("pad", False)} <= seen, seen
    pe = T.rope_pe(138)
    assert len({tuple(r.tolist()) for r in pe.reshape(138, -1)}) == 138


def test_token_norm_widths_sit_on_every_dispatch_threshold():
    """launch_ln: MAXOCT 1 / 2 / 3 / 8 at c / 8 <= 64 / 128 / 192 / else; fmx_rmsnorm: 1 / 2 / 4 / 8 at 64 / 128 / 256 / else -- each threshold has the width on
    it and the next one up, and no row count fills its last block"""
    for widths, thr in ((T.LN_C, (64, 128, 192)), (T.RMS_C, (64, 128, 256))):
        for t in thr:
            assert 8 * t in widths and 8 * t + 8 in widths
        assert 8 in widths and 4096 in widths
    assert all(r % 4 for r in T.ROWS) and all((T.MOD_B * rpb) % 4 for _, rpb, _ in T.MOD_CASES) and (T.PAD_B * T.PAD_N) % 4
