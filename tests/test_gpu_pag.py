"""GPU: native Perturbed-Attention Guidance.  fmx_attn_value_rows_f16 (hipops.attn_value_rows) bit for bit against the indexed expectation with
canaries around it; fmx_cfg_pag_combine (hipops.cfg_pag_combine) against the fp64 formula and the bound derived in tests/pag_refs.py; the
executor's `pag_from` on the stored attention operands; KModel.denoise_cfg against the reference with the reference's own script
(tests/golden/tiny_pag_unet.pt, tools/make_pag_fixtures.py); a windowed, attenuated sampling run on the captured-graph path; the native route
against the same arithmetic as a Python post-CFG function with an attn1 replace patch on the hooked executor."""
from functools import lru_cache

import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import forge_amd  # noqa: E402,F401
from forge_amd import hipops as ops  # noqa: E402
from forge_amd import synth  # noqa: E402
from forge_amd.backend.diffusion_engine.base import build_engine  # noqa: E402
from forge_amd.backend.patcher.native_call import NativeCall  # noqa: E402
from forge_amd.backend.patcher.pag import patch_pag  # noqa: E402
from forge_amd.modules import processing, sd_samplers_common, shared  # noqa: E402

from conftest import load_golden  # noqa: E402
import kernel_refs as R  # noqa: E402
import pag_refs as P  # noqa: E402
import parity  # noqa: E402
from parity import check  # noqa: E402
from test_gpu_gemm_windows import bits  # noqa: E402
from test_gpu_sampler_kernels import CFG_B, CFG_GEOS, CFG_HW, CFG_SIGMAS, COND_SCALES, F32, H16, PTYPES, SIGMA_DATAS, Out, Win, gen, measured, untouched  # noqa: E402,F401

DEV = "cuda"
PAG_SCALES = [3.0, 0.75]     # (1.0 would hide a scale applied to the wrong factor)
CANARY = 0x5A3C              # a finite fp16 pattern (215.5) that no copy of random words reproduces over a whole row


# ---- fmx_attn_value_rows_f16 ------------------------------------------------------------------------------------------------------------------------
# P.COPY_CASES, then: `out` as a view with a row stride of hd + 24 (an arena view wider than the heads); V^T from a base 2 elements into its buffer
# and O from a base 2 elements into its buffer (neither 16-byte aligned: the 2-byte path)
COPY_VARIANTS = [(case, 0, 0, 0) for case in P.COPY_CASES] + [((3, 1, 2, 35, 64, 128), 24, 0, 0), ((3, 1, 2, 35, 64, 128), 0, 2, 0),
                                                              ((4, 2, 2, 100, 128, 192), 0, 0, 2)]


@pytest.mark.parametrize("variant", range(len(COPY_VARIANTS)))
def test_attn_value_rows_is_a_bit_exact_copy_that_stays_in_its_window(variant):
    (images, first, count, n, n_pad, hd), extra_ld, vt_off, out_off = COPY_VARIANTS[variant]
    g = gen(700 + variant)
    ld = hd + extra_ld
    # every 16-bit pattern may occur (NaNs, infinities, denormals): the kernel moves words
    vt_buf = torch.randint(-32768, 32768, (vt_off + hd * images * n_pad + 8,), generator=g, dtype=torch.int32).to(torch.int16)
    out_buf = torch.full((out_off + images * n * ld + 64,), CANARY, dtype=torch.int16)
    vt_words = vt_buf[vt_off:vt_off + hd * images * n_pad].view(hd, images, n_pad)
    out_words = out_buf[out_off:out_off + images * n * ld].view(images, n, ld)
    want = out_buf.clone()
    want[out_off:out_off + images * n * ld] = P.value_rows_expected(vt_words, out_words, first, count, n, hd).reshape(-1)
    assert int((want != out_buf).sum()) > 0.9 * count * n * hd
    runs = []
    for _ in range(2):
        dvt, dout = vt_buf.to(DEV), out_buf.to(DEV)
        vt = dvt[vt_off:vt_off + hd * images * n_pad].view(torch.float16).view(hd, images * n_pad)
        out = dout[out_off:out_off + images * n * ld].view(torch.float16).view(images * n, ld)
        assert (vt.data_ptr() % 16 == 0) == (vt_off == 0) and (out.data_ptr() % 16 == 0) == (out_off == 0)
        ops.attn_value_rows(vt, out, first=first, count=count, n=n, hd=hd, vt_bs=n_pad, vt_ds=images * n_pad)
        torch.cuda.synchronize()
        assert torch.equal(dvt.cpu(), vt_buf)                                     # the source is read only
        runs.append(dout.cpu())
    wrong = int((runs[0] != want).sum())
    assert wrong == 0, f"{COPY_VARIANTS[variant]}: {wrong} words differ from the indexed expectation (canaries included)"
    assert torch.equal(runs[0], runs[1])


# ---- fmx_cfg_pag_combine ------------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def combine_case(has_uncond, c, ld):
    """test_gpu_sampler_kernels.cfg_case with the perturbed group behind the others: x at the scale a latent has at its sigma, eps N(0, 1) fp16 with
    30000 in the padding columns"""
    groups = 3 if has_uncond else 2
    g = gen(500 + 10 * groups + c + ld)
    h, w = CFG_HW
    sigma = torch.tensor(CFG_SIGMAS)
    x = torch.randn(CFG_B, c, h, w, generator=g) * torch.sqrt(1 + sigma * sigma).view(-1, 1, 1, 1)
    eps = torch.full((groups * CFG_B, h, w, ld), 30000.0, dtype=H16)
    eps[..., :c] = torch.randn(groups * CFG_B, h, w, c, generator=g).half()
    return Win(eps, 2, 1), Win(x, 1, 3), Win(sigma, 2, 1)


@pytest.mark.parametrize("sd", SIGMA_DATAS)
@pytest.mark.parametrize("has_uncond", [True, False])
@pytest.mark.parametrize("ptype", PTYPES)
def test_cfg_pag_combine(ptype, has_uncond, sd):
    """denoised and degraded_pred within their derived bounds of the fp64 formula for every geometry, cond_scale and pag_scale; cond_pred / uncond_pred
    bit-equal to what fmx_cfg_combine writes from the same rows; absent optional outputs untouched"""
    worst = {"denoised": 0.0, "degraded": 0.0}
    for c, ld in CFG_GEOS:
        eps, x, sigma = combine_case(has_uncond, c, ld)
        for cs in COND_SCALES:
            for ps in PAG_SCALES:
                for parts in (True, False):
                    what = f"cfg_pag_combine {ptype} uncond {has_uncond} sigma_data {sd} c {c} ld {ld} cond_scale {cs} pag_scale {ps} parts {parts}"
                    outs = [Out(x.shape, F32, 1 + k, 1) for k in range(6)]
                    den, cond, unc, deg, cond2, unc2 = (o.on(DEV) for o in outs)
                    de = eps.on(DEV)
                    ops.cfg_pag_combine(de, ld, x.on(DEV), sigma.on(DEV), has_uncond, cs, ps, denoised=den, cond_pred=cond if parts else None,
                                        uncond_pred=unc if parts else None, degraded_pred=deg if parts else None, prediction_type=ptype, sigma_data=sd)
                    torch.cuda.synchronize()
                    untouched(what, eps, x, sigma, *outs[:4])
                    want, _, _, want_p, b_den, _, _, b_p = P.cfg_pag_combine_ref(eps.values, x.values, sigma.values, has_uncond, cs, ps, ptype, sd)
                    worst["denoised"] = max(worst["denoised"], R.excess_abs(den, want, b_den))
                    R.assert_within_bound(den, want, b_den, what)
                    if not parts:
                        for o in outs[1:4]:
                            assert torch.equal(bits(o.dbuf.cpu()), bits(o.buf)), f"{what}: an absent output was written"
                        continue
                    worst["degraded"] = max(worst["degraded"], R.excess_abs(deg, want_p, b_p))
                    R.assert_within_bound(deg, want_p, b_p, what + " degraded_pred")
                    # the first rows of eps are exactly what fmx_cfg_combine takes: [uncond ; cond] or [cond]
                    ops.cfg_combine(de, ld, x.dbuf[x.lead:x.lead + x.n].view(x.shape), sigma.dbuf[sigma.lead:sigma.lead + sigma.n], 2 if has_uncond else 1, cs,
                                    denoised=torch.empty_like(den), cond_pred=cond2, uncond_pred=unc2, prediction_type=ptype, sigma_data=sd)
                    torch.cuda.synchronize()
                    assert torch.equal(bits(cond.cpu()), bits(cond2.cpu())), f"{what}: cond_pred differs from fmx_cfg_combine's bits"
                    assert torch.equal(bits(unc.cpu()), bits(unc2.cpu())), f"{what}: uncond_pred differs from fmx_cfg_combine's bits"
    measured("cfg_pag_combine denoised", f"{ptype} uncond={has_uncond} sd={sd}", worst["denoised"])
    measured("cfg_pag_combine degraded", f"{ptype} uncond={has_uncond} sd={sd}", worst["degraded"])


# ---- the executor -------------------------------------------------------------------------------------------------------------------------------------
# one transformer level of 320 channels (5 heads of 64), depth 2 in the middle: at 3 x 16384 tokens the GEMM dispatcher's cost model puts the projections
# on the 256 x 320 tile (192 tiles, one round), so norm1 runs folded into the q|k and V^T projections (asserted below on fold_trace)
FOLD_CONFIG = dict(in_channels=4, model_channels=320, out_channels=4, num_res_blocks=[1], channel_mult=(1,), num_head_channels=64,
                   use_spatial_transformer=True, transformer_depth=[1], transformer_depth_middle=2, transformer_depth_output=[1, 1],
                   context_dim=128, use_linear_in_transformer=True)
TAP_CASES = [("folded", FOLD_CONFIG, (128, 128), 16384), ("plain", synth.TINY_SDXL_UNET_CONFIG, (32, 32), 256), ("plain", synth.TINY_SD15_UNET_CONFIG, (32, 32), 64),
             ("ragged", synth.TINY_SDXL_UNET_CONFIG, (24, 20), 120), ("ragged", synth.TINY_SD15_UNET_CONFIG, (32, 24), 48)]


@pytest.mark.parametrize("i", range(len(TAP_CASES)))
def test_perturbed_images_get_v_in_every_middle_block_and_nowhere_else(i):
    from forge_amd.backend.nn.unet import IntegratedUNet2DConditionModel
    branch, cfg, (hh, ww), mid_tokens = TAP_CASES[i]
    net = IntegratedUNet2DConditionModel(cfg, synth.synth_unet_state_dict(cfg, seed=3), device=DEV)
    b, bu = 1, 3
    g = gen(40 + i)
    x = torch.randn(b, cfg["in_channels"], hh, ww, generator=g).to(DEV)
    ctx = torch.randn(bu, 77, cfg["context_dim"], generator=g).to(DEV)
    y = torch.randn(bu, cfg["adm_in_channels"], generator=g).to(DEV) if cfg.get("adm_in_channels") else None
    xcol = ops.unet_pack_input(x, torch.tensor([2.0], device=DEV), bu, 1.0)
    t = torch.full((bu,), 400.0, device=DEV)
    taps = {}
    keep = 2048          # tokens per image that leave the device (the folded case stores 16384)
    net.tap = lambda name, tens: taps.__setitem__(name, tens[:, :keep].detach().to("cpu", copy=True)) if name.endswith((".attn1.o", ".attn1.v")) else None
    try:
        net.forward_packed(xcol, t, net.prepare_context(ctx, y), bu, hh, ww, native=NativeCall(pag_from=2))
    finally:
        net.tap = None
    torch.cuda.synchronize()
    blocks = sorted(k[:-len(".attn1.o")] for k in taps if k.endswith(".attn1.o"))
    middle = [k for k in blocks if k.startswith("middle_block.")]
    assert len(middle) == cfg["transformer_depth_middle"] and len(blocks) > len(middle)
    seen = {"middle": 0, "other": 0}
    for k in blocks:
        o, v = taps[k + ".attn1.o"], taps.get(k + ".attn1.v")
        if k in middle:
            assert v is not None and o.shape == v.shape and o.shape[:2] == (bu, min(mid_tokens, keep)), (k, o.shape)
            folded = net.fold_trace[k][0]
            assert folded == (branch == "folded") and (mid_tokens % 64 != 0) == (branch == "ragged"), (k, branch, net.fold_trace[k])
            assert torch.equal(bits(o[2]), bits(v[2])), f"{k}: the perturbed image's attention output is not its V"
            assert float(v[2].float().abs().max()) > 0.0
            for img in (0, 1):
                assert not torch.equal(o[img], v[img]), f"{k}: image {img} is not perturbed and must get real attention"
            seen["middle"] += 1
        elif v is not None:      # (a ragged block outside the middle stores no operands)
            for img in range(bu):
                assert not torch.equal(o[img], v[img]), f"{k}: no image is perturbed outside the middle block"
            seen["other"] += 1
    # (the tiny SDXL network has transformers at one level only: at a ragged size none of its other blocks stores operands)
    assert seen["middle"] == len(middle) and (seen["other"] > 0 or branch == "ragged"), seen


@pytest.fixture(scope="module")
def fx():
    g = load_golden("tiny_pag_unet.pt")
    # the fixture carries its own floors (the reference's fp16-storage runs, oracle/make_floor.py's mechanism): same gate as every floor-keyed check
    for i, c in enumerate(g["cases"]):
        for k, v in c["floor"].items():
            parity.FLOORS[f"tiny_pag_unet.pt:{i}/{k}"] = v
    parity.FLOORS["tiny_pag_unet.pt:euler4/latent"] = g["euler4"]["floor"]
    return g


_engines = {}


def engine_of(config_name, seed=0, fresh=False):
    if fresh or (config_name, seed) not in _engines:
        cfg = dict(getattr(synth, config_name))
        eng = build_engine(cfg, synth.synth_unet_state_dict(cfg, seed=seed), None, None, device=DEV)
        if fresh:
            return eng
        _engines[(config_name, seed)] = eng
    return _engines[(config_name, seed)]


@pytest.mark.parametrize("i", range(4))
def test_denoise_cfg_with_pag_vs_reference(fx, i):
    """each fixture case at CFG 7 (three groups) and CFG 1 (two) through KModel.denoise_cfg under the floor-keyed gates; the same call without the
    option misses the gate of the result -- an implementation that ignores the option cannot pass"""
    want_cases = [("TINY_SD15_UNET_CONFIG", (32, 24), 48, 1), ("TINY_SD15_UNET_CONFIG", (32, 32), 64, 1), ("TINY_SDXL_UNET_CONFIG", (32, 32), 256, 2),
                  ("TINY_SDXL_UNET_CONFIG", (24, 20), 120, 2)]
    assert [(c["config"], tuple(c["hw"]), c["middle_tokens"], c["depth"]) for c in fx["cases"]] == want_cases
    assert fx["scale"] == 3.0 and fx["cfg"] == 7.0 and fx["t"] == [601.0, 187.0]
    c = fx["cases"][i]
    eng = engine_of(c["config"], c["weight_seed"])
    km = eng.forge_objects.unet.model
    cfg = dict(getattr(synth, c["config"]))
    sig_host = km.predictor.sigma(torch.tensor(fx["t"]))
    x, cond, uncond = P.case_inputs(cfg, c["hw"], c["seed"], sig_host)
    x, sigma = x.to(DEV), sig_host.float().to(DEV)
    as_ctx = (lambda d: (d["crossattn"].to(DEV), d["vector"].to(DEV))) if isinstance(cond, dict) else (lambda t: (t.to(DEV), None))
    cctx, uctx = as_ctx(cond), as_ctx(uncond)
    name = f"tiny_pag case {i} ({c['name']})"
    for tag, u, cs in (("result_cfg7", uctx, 7.0), ("result_cfg1", None, 1.0)):
        den, cp, up, dg = km.denoise_cfg(x, sigma, u, cctx, cs, want_parts=True, pag_scale=fx["scale"])
        key = f"tiny_pag_unet.pt:{i}/"
        check(f"{name} {tag}: native PAG vs the reference with its script", den, c[tag], floor=key + tag)
        if u is not None:
            check(f"{name}: degraded prediction", dg, c["degraded"], floor=key + "degraded")
            check(f"{name}: cond prediction", cp, c["cond_denoised"], floor=key + "cond_denoised")
            check(f"{name}: uncond prediction", up, c["uncond_denoised"], floor=key + "uncond_denoised")
            assert parity.metrics(dg, c["cond_denoised"])["rms_rel"] > 10 * c["floor"]["degraded"]["rms_rel"]     # the third group IS perturbed
        plain = km.denoise_cfg(x, sigma, u, cctx, cs)
        m, lim = parity.metrics(plain, c[tag]), parity.limits(key + tag)[1]
        print(f"{name} {tag} without the option: rms_rel {m['rms_rel']:.3e} against the gate {lim['rms_rel']:.3e}")
        assert m["rms_rel"] > 5 * lim["rms_rel"] and c["moved"][tag] >= 10 * c["floor"][tag]["rms_rel"], (tag, m, lim)
    if c["depth"] > 1:
        assert c["block0_only"] >= 10 * c["floor"]["result_cfg7"]["rms_rel"]      # perturbing one block of two would miss the gate as well


def run_job(eng, fx, unet=None):
    e4 = fx["euler4"]
    cfg = synth.TINY_SD15_UNET_CONFIG
    b = len(e4["seeds"])
    saved = eng.forge_objects_after_applying_lora
    if unet is not None:
        eng.forge_objects_after_applying_lora = saved.shallow_copy()
        eng.forge_objects_after_applying_lora.unet = unet
    try:
        c, uc = synth.synth_conditioning(b, cfg["context_dim"], None, seed=1234)
        shared.opts.randn_source = "CPU"
        p = processing.StableDiffusionProcessingTxt2Img(sd_model=eng, c=c.to(DEV), uc=uc.to(DEV), seed=e4["seeds"][0], sampler_name="Euler", batch_size=b,
                                                        steps=e4["steps"], cfg_scale=7.0, width=e4["hw"] * 8, height=e4["hw"] * 8, do_decode=False)
        return processing.process_images(p).latents.clone()
    finally:
        eng.forge_objects_after_applying_lora = saved
        eng.forge_objects = saved.shallow_copy()


def test_windowed_attenuated_sampling_on_the_graph_path(fx, monkeypatch):
    """4-step Euler, CFG 7, window [0, 0.67], attenuation 25 as the fixture's run of the reference's sampler with the reference's script: three
    guided steps at scales 3, 2.25, 1.5 on ONE captured graph, the fourth on the plain one, no hooked forward; the same bits again on the same patcher
    (the scale starts over at sampling_prepare).  The fixture numbers the model calls 0..3; the UI's progress counter (state.sampling_step, what the
    reference's callback also reads) is written after a step and so runs one call behind: it is advanced here so that call i sees position i / 3, as
    tests/test_gpu_freeu.py does."""
    monkeypatch.setattr(sd_samplers_common.Sampler, "callback_state", lambda self, d: setattr(shared.state, "sampling_step", d["i"] + 1))
    e4 = fx["euler4"]
    assert e4["active"] == [True, True, True, False] and e4["scales"][:3] == [3.0, 2.25, 1.5] and e4["params"]["attenuation"] == 25.0
    eng = engine_of("TINY_SD15_UNET_CONFIG")
    km = eng.forge_objects.unet.model
    net = km.diffusion_model
    hooked, scales, copies = [], [], []
    real_hooked = net._attn_block_hooked
    monkeypatch.setattr(net, "_attn_block_hooked", lambda *a, **kw: (hooked.append(1), real_hooked(*a, **kw))[1], raising=False)
    real_comb, real_copy = ops.cfg_pag_combine, ops.attn_value_rows
    monkeypatch.setattr(ops, "cfg_pag_combine", lambda *a, **kw: (scales.append(a[6]), real_comb(*a, **kw))[1])
    monkeypatch.setattr(ops, "attn_value_rows", lambda *a, **kw: (copies.append((kw["first"], kw["count"])), real_copy(*a, **kw))[1])
    unet = patch_pag(eng.forge_objects.unet, **e4["params"])
    opt = unet.model_options["pag"]
    km._drop_graphs()
    lat = run_job(eng, fx, unet)
    check("tiny_pag 4-step Euler with windowed, attenuated native PAG vs reference", lat, e4["latent"], floor="tiny_pag_unet.pt:euler4/latent")
    assert scales == [3.0, 2.25, 1.5] and opt.scale == 0.75                 # the fourth step is outside the window: no decrement there
    keys = list(km._graphs)
    # at most two graphs: the guided steps' and the plain steps' (a single plain step ends in its eager warm-up run and captures nothing)
    assert 1 <= len(keys) <= 2 and sum("pag" in k for k in keys) == 1 and all(k[:5] == (2, 4, 16, 16, 2) for k in keys), keys
    assert hooked == []
    # one copy per middle block and guided forward that Python walked (two warm-ups and the capture; replays launch from the graph), images [2b, 3b)
    assert set(copies) == {(4, 2)} and 1 <= len(copies) <= 3, copies
    again = run_job(eng, fx, unet)                                          # a second job on the same patcher
    assert torch.equal(again, lat) and scales == [3.0, 2.25, 1.5] * 2 and opt.scale == 0.75
    assert len(km._graphs) <= 2
    # without the option the job lands elsewhere, by more than the floor can hide
    plain = run_job(eng, fx)
    assert parity.metrics(plain, e4["latent"])["rms_rel"] > 5 * parity.limits("tiny_pag_unet.pt:euler4/latent")[1]["rms_rel"]
    assert e4["moved"] >= 10 * e4["floor"]["rms_rel"]


def test_native_route_vs_the_python_post_cfg_route(fx, monkeypatch):
    """the same guidance as the reference script installs it -- a post-CFG function that calls the model again with an attn1 replace patch, which
    sends that call to the hooked executor -- against the native route, every step guided, attenuation 25"""
    eng = engine_of("TINY_SD15_UNET_CONFIG")
    net = eng.forge_objects.unet.model.diffusion_model
    hooked = []
    real_hooked = net._attn_block_hooked
    monkeypatch.setattr(net, "_attn_block_hooked", lambda *a, **kw: (hooked.append(a[0]), real_hooked(*a, **kw))[1], raising=False)
    native = run_job(eng, fx, patch_pag(eng.forge_objects.unet, 3.0, 25.0, 0.0, 1.0))
    assert hooked == []
    degraded = []
    via_python = run_job(eng, fx, P.python_pag(eng.forge_objects.unet, 3.0, 25.0, log=degraded))
    assert len(degraded) == 4 and len(hooked) > 0 and any(k.startswith("middle_block.") for k in hooked)
    check("tiny_pag 4-step Euler: native PAG vs the Python post-CFG route", native, via_python, floor="tiny_pag_unet.pt:euler4/latent")
