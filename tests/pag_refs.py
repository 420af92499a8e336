"""References for native Perturbed-Attention Guidance (tests/test_pag_host.py on the CPU, tests/test_gpu_pag.py on the MI355X): the fp64 formula of
fmx_cfg_pag_combine with a per-element bound derived below, its fp32 emulation in the kernel's order with planted bugs, the indexed expectation of
fmx_attn_value_rows_f16, the inputs of the fixture cases rebuilt from their seeds, and the reference script's arithmetic restated as a Python
post-CFG function with an attn1 replace patch (the route the native one is compared with).

fmx_cfg_pag_combine, per element (u = 2^-24, every fp32 operation rounds by at most u of its result; FMA contraction only removes roundings; the
fp16 eps are inputs, read exactly):
    du, dc, dp    calculate_denoised of the three groups: the expressions of fmx_cfg_combine, whose derivation (kernel_refs.py, CFG_PRED_R = 8)
                  bounds each by 8 u t_g with t_g = |A x| + |B e_g|.
    g  = (dc - du) * cond_scale        two roundings of its own: 2 u |g|
    den = du + g                       one rounding: u |den|
    p  = (dc - dp) * pag_scale         two roundings: 2 u |p|
    res = den + p                      one rounding: u |res|
The roundings made in du, dc, dp reach the result multiplied by the coefficient of that prediction in
    res = (1 - cond_scale) du + (cond_scale + pag_scale) dc - pag_scale dp,
which is the part kernel_refs.py's count for fmx_cfg_combine states it does not model; here it is modelled, since with two scales the factor on dc
is their sum:
    bound = u (8 (|1 - cs| t_u + |cs + ps| t_c + |ps| t_p) + 2 |g| + |den| + 2 |p| + |res|) * (1 + 2^-10)
Without the uncond half den = 0 + (dc - 0) * cond_scale is one product: t_u and the term 2 |g| + |den| become |den| alone, the coefficient of dc stays
cs + ps.  The factor 1 + 2^-10 covers the second-order terms (products of two roundings, at most 2^-24 of the first-order ones each).  The
magnitudes are those of the fp64 reference.  Nothing here comes from a GPU run."""
import numpy as np
import torch

import kernel_refs as R

SECOND_ORDER = 1.0 + 2.0 ** -10


def _groups(eps, b, c, has_uncond):
    """eps [(2 + has_uncond) * b, h, w, ld] -> (eu or None, ec, ep), each [b, c, h, w]"""
    e = eps[..., :c].permute(0, 3, 1, 2)
    if has_uncond:
        return e[:b], e[b:2 * b], e[2 * b:3 * b]
    return None, e[:b], e[b:2 * b]


def cfg_pag_combine_ref(eps, x, sigma, has_uncond, cond_scale, pag_scale, ptype="epsilon", sigma_data=1.0):
    """fmx_cfg_pag_combine in fp64 -> (denoised, cond_pred, uncond_pred, degraded_pred, bound of denoised, bound of cond_pred, bound of uncond_pred,
    bound of degraded_pred); uncond_pred is 0 without the uncond half"""
    b, c = x.shape[:2]
    cs, ps = R.f32(cond_scale), R.f32(pag_scale)
    ca, cb = R._cfg_coefs(sigma, ptype, sigma_data, torch.float64)
    eu, ec, ep = _groups(eps.double(), b, c, has_uncond)
    ax = ca * x.double()
    dc, tc = ax + cb * ec, ax.abs() + (cb * ec).abs()
    dp, tp = ax + cb * ep, ax.abs() + (cb * ep).abs()
    p = ps * (dc - dp)
    if has_uncond:
        du, tu = ax + cb * eu, ax.abs() + (cb * eu).abs()
        g = cs * (dc - du)
        den = du + g
        comb = abs(1.0 - cs) * 8 * tu + 2 * g.abs() + den.abs()
    else:
        du, tu = torch.zeros_like(dc), torch.zeros_like(dc)
        den = cs * dc
        comb = den.abs()
    res = den + p
    bound = R.U32 * SECOND_ORDER * (comb + 8 * (abs(cs + ps) * tc + abs(ps) * tp) + 2 * p.abs() + res.abs())
    return res, dc, du, dp, bound, R.CFG_PRED_R * R.U32 * tc, R.CFG_PRED_R * R.U32 * tu, R.CFG_PRED_R * R.U32 * tp


PLANTS = ("term_sign", "du_for_dc", "scale_on_dp_only")


def cfg_pag_combine_emul(eps, x, sigma, has_uncond, cond_scale, pag_scale, ptype="epsilon", sigma_data=1.0, plant=None):
    """the kernel's formula in fp32 torch, in its order -> (denoised, cond_pred, uncond_pred, degraded_pred).  plant: None, "term_sign"
    (den - (dc - dp) * s), "du_for_dc" ((du - dp) * s: the uncond prediction in the term; 0 stands in without the uncond half), "scale_on_dp_only"
    (den + (dc - dp * s))"""
    b, c = x.shape[:2]
    cs = torch.tensor(R.f32(cond_scale), dtype=torch.float32)
    ps = torch.tensor(R.f32(pag_scale), dtype=torch.float32)
    ca, cb = R._cfg_coefs(sigma, ptype, sigma_data, torch.float32)
    eu, ec, ep = _groups(eps, b, c, has_uncond)
    xv = x.float()
    half = (lambda e: xv - e.float() * sigma.float().view(-1, 1, 1, 1)) if ptype == "epsilon" else (lambda e: xv * ca + e.float() * cb)
    dc, dp = half(ec), half(ep)
    if has_uncond:
        du = half(eu)
        den = du + (dc - du) * cs
    else:
        du = torch.zeros_like(dc)
        den = 0.0 + (dc - 0.0) * cs
    if plant == "term_sign":
        res = den - (dc - dp) * ps
    elif plant == "du_for_dc":
        res = den + (du - dp) * ps
    elif plant == "scale_on_dp_only":
        res = den + (dc - dp * ps)
    else:
        assert plant is None, plant
        res = den + (dc - dp) * ps
    return res, dc, du, dp


# ---- fmx_attn_value_rows_f16 ------------------------------------------------------------------------------------------------------------------------
# (images, first image of the window, images in it, n tokens, n_pad columns per image in V^T, hd features): one tile; token tail + two feature
# tiles; a single token; token tail across two tiles + feature tail tile count 3; the SDXL width (20 feature tiles) with a ragged token count
COPY_CASES = [(3, 2, 1, 64, 64, 64), (3, 1, 2, 35, 64, 128), (2, 1, 1, 1, 64, 64), (4, 2, 2, 100, 128, 192), (2, 0, 2, 120, 128, 1280)]


def value_rows_expected(vt_words, out_words, first, count, n, hd):
    """vt_words [hd, images, n_pad], out_words [images, n, ld >= hd] (both int16 views) -> the output the kernel must leave: rows of the window
    replaced by the indexed copy, every other word as it was"""
    want = out_words.clone()
    want[first:first + count, :, :hd] = vt_words[:, first:first + count, :n].permute(1, 2, 0)
    return want


# ---- the fixture's inputs ---------------------------------------------------------------------------------------------------------------------------
def case_inputs(cfg, hw, seed, sigmas, b=2):
    """tools/make_pag_fixtures.py case_inputs: x fp32 [b, c, h, w] at the noise level of `sigmas`, cond, uncond of synth_conditioning(seed)"""
    from forge_amd import synth
    rng = np.random.Generator(np.random.PCG64([seed, 11]))
    x = torch.from_numpy(rng.standard_normal((b, cfg["in_channels"], hw[0], hw[1]), dtype=np.float32))
    x = x * torch.sqrt(sigmas.float() ** 2 + 1.0).view(-1, 1, 1, 1)
    c, uc = synth.synth_conditioning(b, cfg["context_dim"], cfg.get("adm_in_channels"), seed=seed)
    return x, c, uc


# ---- the reference's arithmetic as Python hooks -----------------------------------------------------------------------------------------------------
def python_pag(unet_patcher, scale, attenuation=0.0, log=None):
    """-> a clone of `unet_patcher` with Perturbed-Attention Guidance as the reference script installs it, restated for this code base's
    calc_cond_uncond_batch (three return values): a post-CFG function that runs the cond batch again with the attn1 replace patch
    `lambda q, k, v, to: v` at ("middle", 0) -- on the hooked executor -- and adds (cond_denoised - degraded) * scale."""
    from forge_amd.backend.sampling.sampling_function import calc_cond_uncond_batch
    state = {"scale": float(scale)}

    def attn_proc(q, k, v, to):
        return v

    def post_cfg_function(args):
        denoised = args["denoised"]
        if state["scale"] <= 0.0:
            return denoised
        options = dict(args["model_options"])
        to = dict(options.get("transformer_options", {}))
        to["patches_replace"] = {"attn1": {("middle", 0): attn_proc}}
        options["transformer_options"] = to
        _, degraded, _ = calc_cond_uncond_batch(args["model"], args["cond"], None, args["input"], args["sigma"], options)
        if log is not None:
            log.append(degraded)
        result = denoised + (args["cond_denoised"] - degraded) * state["scale"]
        state["scale"] -= scale * attenuation / 100.0
        return result
    m = unet_patcher.clone()
    m.set_model_sampler_post_cfg_function(post_cfg_function)
    return m
