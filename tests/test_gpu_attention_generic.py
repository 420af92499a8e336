"""GPU (MI355X) parity of the generic attention kernel `attn_kernel<DP>` (csrc/fmx_attention.hip) behind fmx_attention_f16 / _bf16: every call
that is not an unmasked d_head 64 / 128 problem with >= 256 queries.  That is all of SD1.5's attention (d_head 40 / 80 / 160 -> dpad
48 / 80 / 160), CLIP's causal self-attention, T5's position bias and every masked `attention_function` call.  Covered here: the real SD1.5
shapes, ragged query / key counts, causal attention at every tile boundary, additive masks through all eight broadcast-stride combinations,
and -inf structures that leave whole key tiles or whole rows without an attending key.

Reference: kernel_refs.attn_ref in fp64 on the rounded inputs the kernel read, computed on the device one batch and a few heads at a time;
a row without an attending key is 0 (torch's scaled_dot_product_attention).  Every element is checked against kernel_refs.ATTN_TOL; each
check prints its excess (in units of the tolerance) as "[attention excess] <family> ...".  K / V rows beyond nk hold garbage, the Q / K
columns d..dpad are zero (include/fmx.h) and the output columns d..dpad must come back 0.  The case builders run on the CPU:
tests/test_kernel_ref_teeth.py plants bugs into the reference on these same inputs."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import forge_amd  # noqa: E402,F401
from forge_amd import hipops as ops  # noqa: E402

import kernel_refs as R  # noqa: E402

DEV = "cuda"
H16, BF = torch.float16, torch.bfloat16
DPAD = {40: 48, 64: 64, 80: 80, 128: 128, 160: 160}
WIDTHS = tuple(DPAD)
NEG = -math.inf


def gen(seed):
    return torch.Generator("cpu").manual_seed(seed)


def nkpad(nk):
    return -(-nk // 64) * 64


# ---- case builders (CPU tensors) ---------------------------------------------------------------------------------------------------------
def inputs(b, h, nq, nk, d, dtype, seed, qscale=1.0):
    """q [B, nq, H, dpad], k / v [B, nk_pad, H, dpad] in `dtype`.  Columns d..dpad are zero; keys nk..nk_pad hold garbage (K 7.0, V -3.0)."""
    dp, nkp = DPAD[d], nkpad(nk)
    g = gen(seed)
    q = torch.zeros(b, nq, h, dp, dtype=dtype)
    k = torch.zeros(b, nkp, h, dp, dtype=dtype)
    v = torch.zeros(b, nkp, h, dp, dtype=dtype)
    q[..., :d] = (torch.randn(b, nq, h, d, generator=g) * qscale).to(dtype)
    k[:, :nk, :, :d] = torch.randn(b, nk, h, d, generator=g).to(dtype)
    v[:, :nk, :, :d] = torch.randn(b, nk, h, d, generator=g).to(dtype)
    k[:, nk:, :, :d] = 7.0
    v[:, nk:, :, :d] = -3.0
    return q, k, v


def mask_strides(mask):
    """(batch, head, query) element strides of a [B | 1, H | 1, nq | 1, nk_pad] mask buffer; a dimension of size 1 is broadcast (stride 0)"""
    if mask is None:
        return (0, 0, 0)
    mb, mh, mq, nkp = mask.shape
    return (mh * mq * nkp if mb > 1 else 0, mq * nkp if mh > 1 else 0, nkp if mq > 1 else 0)


def reference(q, k, v, nk, d, mask=None, causal=False, dev=DEV):
    """fp64 [B, H, nq, d] of the case (q / k / v as `inputs` builds them, mask [B | 1, H | 1, nq | 1, nk_pad]); one batch and as many heads
    as keep the score tensor at <= 2^25 elements per step"""
    b, nq, h, _ = q.shape
    out = torch.empty(b, h, nq, d, dtype=torch.float64, device=dev)
    hc = max(1, min(h, (1 << 25) // (nq * nk)))
    for bi in range(b):
        for h0 in range(0, h, hc):
            hs = slice(h0, min(h, h0 + hc))
            qq = q[bi:bi + 1, :, hs, :d].to(dev).permute(0, 2, 1, 3)
            kk = k[bi:bi + 1, :nk, hs, :d].to(dev).permute(0, 2, 1, 3)
            vv = v[bi:bi + 1, :nk, hs, :d].to(dev).permute(0, 2, 1, 3)
            m = None
            if mask is not None:
                mb = bi if mask.shape[0] > 1 else 0
                m = mask[mb:mb + 1, hs if mask.shape[1] > 1 else slice(None), :, :nk].to(dev)
            out[bi:bi + 1, hs] = R.attn_ref(qq, kk, vv, d ** -0.5, mask=m, causal=causal)
    return out


def launch(q, k, v, nk, d, mask=None, causal=False):
    """fmx_attention_(b)f16 on the device copies; d_head 64 / 128 without mask or causal flag take the 32-query kernel (force32) -> [B, nq, H, dpad]"""
    b, nq, h, dp = q.shape
    nkp = k.shape[1]
    dq, dk = q.to(DEV), k.to(DEV)
    vt = v.to(DEV).permute(2, 3, 0, 1).contiguous()          # [H, dpad, B, nk_pad] == V^T[(h, d)][b * nk_pad + j]
    force32 = mask is None and not causal and dp in (64, 128)
    out = ops.attention(dq, dk, vt, batch=b, heads=h, nq=nq, nk=nk, nk_pad=nkp, dpad=dp, scale=d ** -0.5, q_bs=nq * h * dp, q_rs=h * dp,
                        k_bs=nkp * h * dp, k_rs=h * dp, vt_bs=nkp, vt_hs=dp * b * nkp, vt_ds=b * nkp, force32=force32, causal=causal,
                        mask=None if mask is None else mask.to(DEV), mask_strides=mask_strides(mask))
    return out.view(b, nq, h, dp)


def check(out, want, d, dtype, family, what):
    """every element of out[..., :d] (as [B, H, nq, d]) within ATTN_TOL of the fp64 reference; the pad columns d..dpad exactly 0"""
    got = out[..., :d].permute(0, 2, 1, 3)
    e = R.excess(got, want, dtype, *R.ATTN_TOL[dtype])
    print(f"[attention excess] {family} {what}: {e:.3f}")
    assert e <= 1.0, f"{what}: error {e:.3g}x ATTN_TOL[{dtype}]"
    if out.shape[-1] > d:
        assert float(out[..., d:].abs().max()) == 0.0, f"{what}: output pad columns d..dpad written"


# ---- head widths at SD1.5's sizes, ragged counts -------------------------------------------------------------------------------------------
# (b, h, nq, nk, d): SD1.5 self-attention per UNet level (64 x 64, 32 x 32, 16 x 16 latents), cross-attention over the 77-token context at each
# width, and d_head 64 / 128 below 256 queries or with force32 (the only ways those widths reach this kernel unmasked)
SD15 = [(8, 8, 4096, 4096, 40), (8, 8, 1024, 1024, 80), (8, 8, 256, 256, 160), (8, 8, 4096, 77, 40), (8, 8, 1024, 77, 80), (8, 8, 256, 77, 160),
        (2, 5, 200, 300, 64), (2, 4, 1024, 77, 64), (2, 3, 200, 200, 128), (1, 4, 512, 333, 128)]
RAGGED_NQ, RAGGED_NK = (1, 33, 97, 300), (1, 63, 65, 200)
HEAD_QSCALE = 2.0      # q . k / sqrt(d) with standard deviation 2: attention as peaked as trained SD layers, not a flat average


def sd15_case(b, h, nq, nk, d):
    return inputs(b, h, nq, nk, d, H16, seed=nq + 7 * nk + d, qscale=HEAD_QSCALE)


@pytest.mark.parametrize("b,h,nq,nk,d", SD15)
def test_head_widths_sd15(b, h, nq, nk, d):
    q, k, v = sd15_case(b, h, nq, nk, d)
    out = launch(q, k, v, nk, d)
    check(out, reference(q, k, v, nk, d), d, H16, "widths", f"b{b} h{h} nq{nq} nk{nk} d{d}")


def ragged_case(nq, nk, dtype):
    """d cycles through every width so that each of the 16 (nq, nk) pairs of a dtype runs at one of them and each width gets >= 3 pairs"""
    i = RAGGED_NQ.index(nq) * len(RAGGED_NK) + RAGGED_NK.index(nk)
    d = WIDTHS[i % len(WIDTHS)]
    return d, inputs(2, 3, nq, nk, d, dtype, seed=1000 + i)


@pytest.mark.parametrize("dtype", [H16, BF])
@pytest.mark.parametrize("nk", RAGGED_NK)
@pytest.mark.parametrize("nq", RAGGED_NQ)
def test_ragged_counts(nq, nk, dtype):
    d, (q, k, v) = ragged_case(nq, nk, dtype)
    check(launch(q, k, v, nk, d), reference(q, k, v, nk, d), d, dtype, "ragged", f"{dtype} nq{nq} nk{nk} d{d}")


# ---- causal ------------------------------------------------------------------------------------------------------------------------------
CLIP_T = (1, 31, 32, 33, 64, 65, 77, 128, 200, 300)


def clip_case(t, heads, dtype, b=2, d=64):
    """CLIP's layout (backend/nn/clip.py): Q | K in one [B, tp, 2C] buffer, V^T [C, B * tp]; rows t..tp hold garbage.  -> (qk, vt, q, k, v)
    with q / k / v the [B, tokens, H, d] views the reference reads"""
    c, tp = heads * d, nkpad(t)
    g = gen(2000 + 31 * t + heads)
    qk = torch.full((b, tp, 2 * c), 7.0).to(dtype)
    qk[:, :t] = torch.randn(b, t, 2 * c, generator=g).to(dtype)
    vt = torch.full((c, b, tp), -3.0).to(dtype)
    vt[:, :, :t] = torch.randn(c, b, t, generator=g).to(dtype)
    vt = vt.reshape(c, b * tp)
    q = qk[:, :t, :c].reshape(b, t, heads, d)
    k = qk[:, :, c:].reshape(b, tp, heads, d)
    v = vt.view(heads, d, b, tp).permute(2, 3, 0, 1)
    return qk, vt, q, k, v


@pytest.mark.parametrize("dtype", [H16, BF])
@pytest.mark.parametrize("heads", [12, 20])
@pytest.mark.parametrize("t", CLIP_T)
def test_causal_clip_layout(t, heads, dtype):
    """the CLIP text encoder's call: d 64, causal, nq == nk == t at and around every 32 / 64-key boundary, up to 300 tokens (>= 256 queries
    with the causal flag must still take the generic kernel)"""
    b, d = 2, 64
    qk, vt, q, k, v = clip_case(t, heads, dtype, b=b, d=d)
    c, tp = heads * d, nkpad(t)
    dqk = qk.to(DEV)
    out = ops.attention(dqk, dqk[:, :, c:], vt.to(DEV), batch=b, heads=heads, nq=t, nk=t, nk_pad=tp, dpad=d, scale=d ** -0.5, q_bs=tp * 2 * c,
                        q_rs=2 * c, k_bs=tp * 2 * c, k_rs=2 * c, vt_bs=tp, vt_hs=d * b * tp, vt_ds=b * tp, causal=True)
    check(out.view(b, t, heads, d), reference(q, k, v, t, d, causal=True), d, dtype, "causal", f"CLIP {dtype} t{t} heads{heads}")


CAUSAL_WIDTH_CASES = [(d, t) for d in (40, 80, 128, 160) for t in (77, 200)] + [(64, 256), (64, 520), (128, 256), (128, 520)]


def causal_case(d, t, dtype):
    return inputs(2, 3, t, t, d, dtype, seed=3000 + t + d)


@pytest.mark.parametrize("dtype", [H16, BF])
@pytest.mark.parametrize("d,t", CAUSAL_WIDTH_CASES)
def test_causal_widths(d, t, dtype):
    q, k, v = causal_case(d, t, dtype)
    check(launch(q, k, v, t, d, causal=True), reference(q, k, v, t, d, causal=True), d, dtype, "causal", f"{dtype} d{d} t{t}")


# ---- additive masks --------------------------------------------------------------------------------------------------------------------------
MASK_B, MASK_H, MASK_NQ, MASK_NK = 3, 3, 97, 200


def mask_case(combo, d, dtype):
    """combo bit 2 / 1 / 0: the mask varies per batch / head / query (non-zero mask_bs / mask_hs / mask_qs), else that stride is 0.  Biases
    uniform in +-3, or +-30 (T5's position-bias range) on alternate (combo, width) pairs; the mask's pad columns hold large finite garbage
    the kernel must not read as keys.  -> (mask [B|1, H|1, nq|1, nk_pad], q, k, v, magnitude)"""
    i = WIDTHS.index(d)
    mag = 3.0 if (combo + i) % 2 == 0 else 30.0
    g = gen(4000 + 8 * i + combo)
    shape = (MASK_B if combo & 4 else 1, MASK_H if combo & 2 else 1, MASK_NQ if combo & 1 else 1, nkpad(MASK_NK))
    mask = torch.full(shape, 1000.0)
    mask[..., :MASK_NK] = (torch.rand(*shape[:3], MASK_NK, generator=g) * 2 - 1) * mag
    q, k, v = inputs(MASK_B, MASK_H, MASK_NQ, MASK_NK, d, dtype, seed=4100 + 8 * i + combo)
    return mask.to(dtype), q, k, v, mag


@pytest.mark.parametrize("dtype", [H16, BF])
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("combo", range(8))
def test_additive_mask_strides(combo, d, dtype):
    mask, q, k, v, mag = mask_case(combo, d, dtype)
    what = f"{dtype} d{d} strides {mask_strides(mask)} +-{mag:g}"
    check(launch(q, k, v, MASK_NK, d, mask=mask), reference(q, k, v, MASK_NK, d, mask=mask), d, dtype, "mask", what)


# ---- -inf structures -----------------------------------------------------------------------------------------------------------------------
INF_B, INF_H, INF_NQ, INF_NK = 2, 2, 150, 200          # 4 key tiles, the last one ragged (8 keys)
INF_CASES = ("lead_tile", "lead_128_some_queries", "middle_tile", "last_key_only", "anti_causal", "dead_rows", "min_f16_and_inf", "pad_nan_inf")


def neg_inf_case(name, d, dtype):
    """-> (mask [B|1, H|1, nq|1, nk_pad] in dtype, q, k, v, dead) with dead a bool [B, nq] of the rows where no key attends in any head"""
    b, h, nq, nk = INF_B, INF_H, INF_NQ, INF_NK
    nkp = nkpad(nk)
    g = gen(5000 + 17 * INF_CASES.index(name) + d)
    i = torch.arange(nq)[:, None]
    j = torch.arange(nkp)[None, :]
    if name == "lead_tile":                       # keys 0..63 hidden from every query (left padding)
        m = torch.where(j < 64, NEG, 0.0)[None, None]
    elif name == "lead_128_some_queries":         # keys 0..127 hidden from every third query (a different third per batch)
        hide = (j < 128) & ((i + torch.arange(b)[:, None, None]) % 3 == 0)
        m = torch.where(hide, NEG, 0.0)[:, None]
    elif name == "middle_tile":                   # head 0 loses keys 64..127, head 1 keys 128..191
        m = torch.zeros(1, h, 1, nkp)
        m[0, 0, 0, 64:128] = NEG
        m[0, 1, 0, 128:192] = NEG
    elif name == "last_key_only":                 # only key nk - 1, in the ragged last tile
        m = torch.where(j == nk - 1, 0.0, NEG)[None, None]
    elif name == "anti_causal":                   # query i attends keys >= i: the leading tiles of late queries are fully masked
        m = torch.where(j >= i, 0.0, NEG)[None, None]
    elif name == "dead_rows":                     # a random 30 % hidden, and rows with no key at all (rows 0 and nq - 1 of batch 0)
        m = torch.where(torch.rand(b, 1, nq, nkp, generator=g) < 0.3, NEG, 0.0)
        m[:, :, 2::5] = NEG
        m[0, :, 0] = NEG
        m[0, :, nq - 1] = NEG
    elif name == "min_f16_and_inf":               # -65504 beside -inf: leading tile -inf on even rows, rows 3 mod 7 see only -65504 keys
        # The rows of -65504 keys are the tightest case of the file: the kernel adds mask / scale to the unscaled score in fp32, and at
        # |s| ~ 65504 * sqrt(d) the fp32 spacing costs the q . k part its low bits.  Measured on an MI355X (fp16): 0.55 (d 40) to 0.91
        # (d 160) of ATTN_TOL; every other -inf structure stays below 0.15.
        r = torch.rand(1, 1, nq, nkp, generator=g)
        m = torch.where(r < 0.3, NEG, torch.where(r < 0.6, -65504.0, 0.0))
        m[:, :, 0::2, :64] = NEG
        m[:, :, 3::7] = torch.where(m[:, :, 3::7] == 0.0, -65504.0, m[:, :, 3::7])
    elif name == "pad_nan_inf":                   # a finite +-3 bias, the mask's pad columns nk..nk_pad alternately NaN and +inf
        m = (torch.rand(b, 1, nq, nkp, generator=g) * 2 - 1) * 3
        m[..., nk::2] = math.nan
        m[..., nk + 1::2] = math.inf
    else:
        raise KeyError(name)
    m = m.clone()
    if name != "pad_nan_inf":
        m[..., nk:] = 0.0
    dead = (m[..., :nk] == NEG).all(-1).expand(b, h, nq).all(1)
    q, k, v = inputs(b, h, nq, nk, d, dtype, seed=5100 + 17 * INF_CASES.index(name) + d)
    return m.to(dtype), q, k, v, dead


@pytest.mark.parametrize("dtype", [H16, BF])
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("name", INF_CASES)
def test_neg_inf_structures(name, d, dtype):
    """whole key tiles, leading tiles or whole rows without an attending key: finite where any key attends, exactly 0 where none does
    (torch's scaled_dot_product_attention), NaN / +inf in the mask's pad columns ignored"""
    mask, q, k, v, dead = neg_inf_case(name, d, dtype)
    out = launch(q, k, v, INF_NK, d, mask=mask)
    want = reference(q, k, v, INF_NK, d, mask=mask)
    check(out, want, d, dtype, "-inf", f"{name} {dtype} d{d}")
    if bool(dead.any()):
        assert float(out.float()[dead.to(DEV)].abs().max()) == 0.0, f"{name}: fully masked rows are not 0"
