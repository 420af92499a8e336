"""GPU: native ControlNet-LLLite.  fmxl_lllite_adapt_f16 (hipops.lllite_adapt) against the fp64 restatement within the derived bound of
tests/lllite_refs.py; the executor against the reference's own patch on its own UNet (tests/golden/lllite.pt, tools/make_lllite_fixtures.py) and
against the same arithmetic as Python patches on the hooked executor; the window, the folds of the blocks without modules, the cond image of
image i % Bc; a 6-step Euler job on the captured-graph path against the same job run eagerly, and a Heun job for the per-call counter."""
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import forge_amd  # noqa: E402,F401
from forge_amd import hipops as ops  # noqa: E402
from forge_amd import runtime, synth  # noqa: E402
from forge_amd.backend.patcher import lllite as ll  # noqa: E402
from forge_amd.backend.patcher.lllite import patch_lllite  # noqa: E402
from forge_amd.backend.patcher.native_call import NativeCall  # noqa: E402
from forge_amd.modules import processing, shared  # noqa: E402
from forge_amd.modules.prompt_parser import DictWithShape  # noqa: E402

from conftest import load_golden  # noqa: E402
import lllite_refs as L  # noqa: E402
import parity  # noqa: E402
from parity import check  # noqa: E402
from test_gpu_gemm_windows import bits  # noqa: E402
from test_gpu_pag import engine_of  # noqa: E402

DEV = "cuda"
H16 = torch.float16
CANARY = 215.5
GUARD = 512          # elements behind every out


# ---- fmxl_lllite_adapt_f16 ------------------------------------------------------------------------------------------------------------------------------
_refs = {}


def refs_of(c, geo):
    """the case and its fp64 references, computed once and shared: {(slot, multiplier): (y, bound)}"""
    key = (c, geo)
    if key not in _refs:
        images, n, bc = geo
        x, conds, slots = L.make_case(c, images, n, bc)
        _refs[key] = (x, conds, slots, {(s, m): L.adapt_ref(x, conds[s], n, slots[s], m) for s in range(3) for m in L.MULTIPLIERS})
    return _refs[key]


def launch(x, conds, slots, n, mask, mult):
    m, c = x.shape
    xd = x.to(DEV)
    bufs = [torch.full((m * c + GUARD,), CANARY, dtype=H16, device=DEV) if on else None for on in mask]
    dev = [None if not on else dict({k: v.to(DEV) for k, v in slots[s].items()}, cond=conds[s].to(DEV), out=bufs[s][:m * c].view(m, c))
           for s, on in enumerate(mask)]
    outs = ops.lllite_adapt(xd, None, n, dev, mult)
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), x), "x was written"
    return outs, bufs


@pytest.mark.parametrize("geo", L.GEOMETRIES)
@pytest.mark.parametrize("c", L.CHANNELS)
def test_lllite_adapt_vs_fp64_within_the_derived_bound(c, geo):
    """fmxl_lllite_adapt_f16: every slot mask and multiplier of the case; at multiplier 0 the output is x exactly; an absent slot returns None;
    the guard elements behind every out keep their value"""
    images, n, bc = geo
    x, conds, slots, refs = refs_of(c, geo)
    worst = 0.0
    for mask in L.MASKS:
        for mult in L.MULTIPLIERS:
            outs, bufs = launch(x, conds, slots, n, mask, mult)
            for s, on in enumerate(mask):
                if not on:
                    assert outs[s] is None
                    continue
                got = outs[s].cpu()
                assert got.shape == x.shape and outs[s].data_ptr() == bufs[s].data_ptr()
                y, bound = refs[(s, mult)]
                e = L.excess(got, y, bound)
                worst = max(worst, e)
                assert e <= 1.0, f"C {c} {geo} mask {mask} multiplier {mult} slot {s}: {e:.3f} x the bound"
                if mult == 0.0:
                    assert torch.equal(got, x), f"C {c} {geo} slot {s}: multiplier 0 must return x"
                assert bool((bufs[s][x.numel():] == CANARY).all()), f"C {c} {geo} slot {s}: elements behind out were written"
    print(f"[lllite_adapt] C {c} (images, n, Bc) {geo}: worst {worst:.3f} x the bound")
    assert worst > 0.01       # the bound is not vacuous


def test_lllite_adapt_is_bit_identical_over_three_launches_and_has_teeth():
    c, geo = 640, (4, 192, 4)
    images, n, bc = geo
    x, conds, slots, refs = refs_of(c, geo)
    runs = [[o.cpu() for o in launch(x, conds, slots, n, (True, True, True), 0.35)[0]] for _ in range(3)]
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(bits(a), bits(b))
    # the gate tells the slots apart, and the images' embeddings: the k output against q's reference, image i against embedding i (no % Bc)
    y, bound = refs[(0, 0.35)]
    assert L.excess(runs[0][1], y, bound) >= L.TEETH_FACTOR
    c2, geo2 = 320, (4, 64, 2)
    x2, conds2, slots2, _ = refs_of(c2, geo2)
    got = launch(x2, conds2, slots2, 64, (True, False, False), 0.35)[0][0].cpu()
    yb, bb = L.adapt_ref(x2, conds2[0], 64, slots2[0], 0.35, bug="cond_without_mod")
    assert L.excess(got, yb, bb) >= L.TEETH_FACTOR


# ---- the executor against the reference ---------------------------------------------------------------------------------------------------------------------
CONFIG = "TINY_SDXL_2LEVEL_UNET_CONFIG"


@pytest.fixture(scope="module")
def fx():
    g = load_golden("lllite.pt")
    assert g["config"] == CONFIG and tuple(g["hw"]) == (32, 32) and (g["b"], g["bc"]) == (2, 2) and g["strengths"] == [1.0, 0.5] and g["cfg"] == 7.0
    for k, v in g["floor"].items():
        parity.FLOORS[f"lllite.pt:{k}"] = v
    return g


@pytest.fixture(scope="module")
def job(fx):
    """the fixture's job on the device, built once: engine, KModel, inputs, LLLite weights, control images"""
    cfg = dict(getattr(synth, CONFIG))
    eng = engine_of(CONFIG, fx["weight_seed"])
    km = eng.forge_objects.unet.model
    sig_host = km.predictor.sigma(torch.tensor(fx["t"]))
    x, cond, uncond = L.case_inputs(cfg, fx["hw"], fx["seed"], sig_host, fx["b"])
    as_ctx = lambda d: (d["crossattn"].to(DEV), d["vector"].to(DEV))  # noqa: E731
    lsd = synth.synth_lllite_state_dict(cfg, seed=fx["lllite_seed"], gain=fx["lllite_gain"], up_gain=fx["up_gain"])
    imgs = L.control_images(fx["bc"], (fx["hw"][0] * 8, fx["hw"][1] * 8), fx["image_seed"])
    return dict(cfg=cfg, eng=eng, km=km, net=km.diffusion_model, x=x.to(DEV), sigma=sig_host.float().to(DEV), c=as_ctx(cond), uc=as_ctx(uncond), lsd=lsd,
                imgs=imgs)


def unit(job, strength=1.0, imgs=None, lsd=None, **kw):
    return patch_lllite(job["eng"].forge_objects.unet, lsd or job["lsd"], job["imgs"] if imgs is None else imgs, strength, **kw)


def python_unit(job, strength=1.0, **kw):
    """the same unit as Python attn1 / attn2 patches: what patch_lllite installs where the native route does not apply"""
    lll = unit(job, strength, **kw).model_options["transformer_options"]["lllite"]
    m = job["eng"].forge_objects.unet.clone()
    patch = lll.python_patch()
    m.set_model_attn1_patch(patch)
    m.set_model_attn2_patch(patch)
    return m


def test_native_cond_embeddings_vs_the_references(fx, job):
    """conditioning1 through the existing GEMM and ReLU kernels (fp16 storage between the convolutions) against the reference's fp32 chain: the
    image and the two or three stage outputs are rounded to fp16 -- at most four roundings of 2^-11 relative, each amplified by at most the gain 2
    the fixture's weights give a later stage: 4 x 2^-11 x 2 = 3.9e-3 of the embedding's largest value"""
    lll = unit(job).model_options["transformer_options"]["lllite"]
    lll.prepare()
    torch.cuda.synchronize()
    for name, want in fx["cond_emb"].items():
        got = lll.cond_emb(lll.modules[name]).cpu()
        assert got.shape == want.shape and got.dtype == H16
        err = float((got.double() - want.double()).abs().max() / want.double().abs().max())
        assert err <= 4e-3, (name, err)


def test_denoise_cfg_vs_the_reference_with_its_patch(fx, job):
    """CFG 7 ([uncond ; cond]: a batch of 2 x Bc, image i on control image i % Bc) and CFG 1, strengths 1.0 and 0.5, under the floor-keyed gates of
    tests/parity.py; without the option, at the other strength and with the two control images swapped the same call misses the gate"""
    km, x, sigma = job["km"], job["x"], job["sigma"]
    for strength in fx["strengths"]:
        to = unit(job, strength).model_options["transformer_options"]
        other = unit(job, 1.5 - strength).model_options["transformer_options"]
        swapped = unit(job, strength, imgs=job["imgs"].flip(0)).model_options["transformer_options"]
        for cs, u in ((7.0, job["uc"]), (1.0, None)):
            tag = f"s{strength}/cfg{int(cs)}"
            den = km.denoise_cfg(x, sigma, u, job["c"], cs, transformer_options=to)
            check(f"lllite {tag}: native ControlNet-LLLite vs the reference with its patch", den, fx["results"][tag], floor=f"lllite.pt:{tag}")
            lim = parity.limits(f"lllite.pt:{tag}")[1]["rms_rel"]
            for what, opts in (("without the option", None), ("at the other strength", other), ("with the control images swapped", swapped)):
                m = parity.metrics(km.denoise_cfg(x, sigma, u, job["c"], cs, transformer_options=opts), fx["results"][tag])
                print(f"{tag} {what}: rms_rel {m['rms_rel']:.3e} against the gate {lim:.3e}")
                assert m["rms_rel"] > 3 * lim, (tag, what, m, lim)
            assert min(fx["moved"][tag], fx["swapped"][tag]) >= 10 * fx["floor"][tag]["rms_rel"]
            check(f"lllite plain cfg{int(cs)}: the unpatched call vs the reference", km.denoise_cfg(x, sigma, u, job["c"], cs), fx["plain"][f"cfg{int(cs)}"],
                  floor=f"lllite.pt:{tag}")


def test_native_route_vs_python_patch_on_the_hooked_executor(fx, job, monkeypatch):
    km, net, x, sigma = job["km"], job["net"], job["x"], job["sigma"]
    hooked, adapts = [], []
    real_hooked, real_adapt = net._attn_block_hooked, ops.lllite_adapt
    monkeypatch.setattr(net, "_attn_block_hooked", lambda *a, **kw: (hooked.append(a[0]), real_hooked(*a, **kw))[1], raising=False)
    monkeypatch.setattr(ops, "lllite_adapt", lambda *a, **kw: (adapts.append(a[4]), real_adapt(*a, **kw))[1])
    for strength in fx["strengths"]:
        tag = f"s{strength}/cfg7"
        del hooked[:], adapts[:]
        native = km.denoise_cfg(x, sigma, job["uc"], job["c"], 7.0, transformer_options=unit(job, strength).model_options["transformer_options"])
        assert hooked == [] and len(adapts) >= 14 and set(adapts) == {strength}          # two launches per block that has modules: attn1, attn2
        via_python = km.denoise_cfg(x, sigma, job["uc"], job["c"], 7.0, transformer_options=python_unit(job, strength).model_options["transformer_options"])
        assert len(hooked) == 7
        check(f"lllite {tag}: native vs python_patch on the hooked executor", native, via_python, floor=f"lllite.pt:{tag}", both_fp16=True)


def test_outside_the_window_the_call_is_the_plain_call_bit_for_bit(fx, job):
    km, x, sigma = job["km"], job["x"], job["sigma"]
    plain = km.denoise_cfg(x, sigma, job["uc"], job["c"], 7.0).clone()
    to = unit(job, 1.0, steps=4, start_percent=0.5, end_percent=0.0).model_options["transformer_options"]       # calls 0, 1 off; 2, 3 on
    keys = set(km._static)
    off = [km.denoise_cfg(x, sigma, job["uc"], job["c"], 7.0, transformer_options=to).clone() for _ in range(2)]
    assert set(km._static) == keys, "a call outside the window must use the plain key"
    on = km.denoise_cfg(x, sigma, job["uc"], job["c"], 7.0, transformer_options=to).clone()
    assert all(torch.equal(bits(o.cpu()), bits(plain.cpu())) for o in off)
    assert not torch.equal(on, plain) and any("lllite" in k for k in set(km._static) - keys)
    # multiplier 0 inside the window: the unfolded route on x itself
    zero = km.denoise_cfg(x, sigma, job["uc"], job["c"], 7.0, transformer_options=unit(job, 0.0).model_options["transformer_options"])
    check("lllite strength 0 vs the plain call", zero, plain, floor="lllite.pt:s1.0/cfg7", both_fp16=True)


def test_a_block_without_modules_keeps_its_folds():
    """one transformer level of 320 channels at 3 x 16384 tokens, where norm1, norm2 and norm3 of every block run folded (tests/test_gpu_pag.py
    FOLD_CONFIG): with modules on the FIRST middle block only, that block runs norm1 and norm2 unfolded and everything else folds as before"""
    from forge_amd.backend.nn.unet import IntegratedUNet2DConditionModel
    from test_gpu_pag import FOLD_CONFIG
    cfg = dict(FOLD_CONFIG)
    net = IntegratedUNet2DConditionModel(cfg, synth.synth_unet_state_dict(cfg, seed=3), device=DEV)
    bu, hh, ww = 3, 128, 128
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 4, hh, ww, generator=g).to(DEV)
    ctx = torch.randn(bu, 77, cfg["context_dim"], generator=g).to(DEV)
    xcol = ops.unet_pack_input(x, torch.tensor([2.0], device=DEV), bu, 1.0)
    t = torch.full((bu,), 400.0, device=DEV)
    ctxc = net.prepare_context(ctx, None)
    plain = net.forward_packed(xcol, t, ctxc, bu, hh, ww).clone()
    trace_plain = dict(net.fold_trace)
    first = "middle_block.1.transformer_blocks.0"
    assert trace_plain[first] == (True, True, True) and len(trace_plain) == 5, trace_plain
    lsd = {k: v for k, v in synth.synth_lllite_state_dict(cfg, seed=9, gain=2.0, up_gain=0.5).items() if "middle_block_1_transformer_blocks_0_" in k}
    lll = ll.LLLite(lsd, L.control_images(1, (hh * 8, ww * 8), 3), 1.0, 0, 0.0, 0.0, DEV)
    assert list(lll.blocks) == [first] and lll.native_ok()
    lll.prepare()
    eps = net.forward_packed(xcol, t, ctxc, bu, hh, ww, native=NativeCall(lllite=lll))
    torch.cuda.synchronize()
    trace = dict(net.fold_trace)
    assert trace[first] == (False, False, True), trace[first]
    assert {k: v for k, v in trace.items() if k != first} == {k: v for k, v in trace_plain.items() if k != first}
    assert bool(torch.isfinite(eps.float()).all()) and not torch.equal(eps, plain)


# ---- sampling -----------------------------------------------------------------------------------------------------------------------------------------------
def run_job(job, unet, sampler, steps, use_graph=True):
    eng, cfg, km = job["eng"], job["cfg"], job["km"]
    saved, saved_graph = eng.forge_objects_after_applying_lora, km.use_graph
    eng.forge_objects_after_applying_lora = saved.shallow_copy()
    eng.forge_objects_after_applying_lora.unet = unet
    km.use_graph = use_graph
    try:
        c, uc = synth.synth_conditioning(2, cfg["context_dim"], cfg.get("adm_in_channels"), seed=77)
        move = lambda d: DictWithShape({k: v.to(DEV) for k, v in d.items()})  # noqa: E731
        shared.opts.randn_source = "CPU"
        p = processing.StableDiffusionProcessingTxt2Img(sd_model=eng, c=move(c), uc=move(uc), seed=4321, sampler_name=sampler, batch_size=2, steps=steps,
                                                        cfg_scale=7.0, width=256, height=256, do_decode=False)
        return processing.process_images(p).latents.clone()
    finally:
        km.use_graph = saved_graph
        eng.forge_objects_after_applying_lora = saved
        eng.forge_objects = saved.shallow_copy()


def test_euler_job_on_the_graph_equals_the_job_run_eagerly(job, monkeypatch):
    """6 Euler steps, window (0.25, 0.7): calls 1, 2, 3 carry the adapters.  Two graphs, the plain one (calls 0, 4, 5) and the unit's (1, 2, 3): each
    warms up on its first call, captures on its second -- the capture is launched once -- and replays its third"""
    km, net = job["km"], job["net"]
    hooked, launches, calls = [], [], []
    real_hooked, real_launch, real_static = net._attn_block_hooked, runtime.HipGraph.launch, km._forward_static
    monkeypatch.setattr(net, "_attn_block_hooked", lambda *a, **kw: (hooked.append(1), real_hooked(*a, **kw))[1], raising=False)
    monkeypatch.setattr(runtime.HipGraph, "launch", lambda self, s: (launches.append(1), real_launch(self, s))[1])
    monkeypatch.setattr(km, "_forward_static", lambda *a, **kw: (calls.append(kw["native"].lllite is not None), real_static(*a, **kw))[1])
    km._drop_graphs()
    km._static.clear()
    window = dict(steps=6, start_percent=0.25, end_percent=0.7)
    on_graph = run_job(job, unit(job, 1.0, **window), "Euler", 6)
    assert calls == [False, True, True, True, False, False] == L.counter_sequence(6, 0.25, 0.7, 6)
    assert len(launches) == 4 and hooked == [], (launches, hooked)
    assert sum("lllite" in k for k in km._graphs) == 1 and len(km._graphs) == 2, list(km._graphs)
    eager = run_job(job, unit(job, 1.0, **window), "Euler", 6, use_graph=False)
    assert len(launches) == 4
    assert torch.equal(bits(on_graph.cpu()), bits(eager.cpu())), parity.metrics(on_graph, eager)
    plain = run_job(job, job["eng"].forge_objects.unet, "Euler", 6)
    assert parity.metrics(on_graph, plain)["rms_rel"] > 1e-2      # the window did something


def test_heun_job_advances_the_counter_per_model_call(job, monkeypatch):
    """Heun calls the model twice per step (once on the last): the unit's counter runs through its window twice as fast and wraps, as the reference's does"""
    km = job["km"]
    calls = []
    real_static = km._forward_static
    monkeypatch.setattr(km, "_forward_static", lambda *a, **kw: (calls.append(kw["native"].lllite is not None), real_static(*a, **kw))[1])
    steps = 4
    run_job(job, unit(job, 1.0, steps=steps, start_percent=0.0, end_percent=0.5), "Heun", steps)
    assert len(calls) > steps, calls
    assert calls == L.counter_sequence(steps, 0.0, 0.5, len(calls)), calls
    assert calls[:6] == [True, True, False, False, True, True]          # on for two CALLS (one step), off for two, and on again after the wrap
