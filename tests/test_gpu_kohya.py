"""GPU: native Kohya HRFix (Deep Shrink).  The kernel fmx_resize_nhwc_f16 (through hipops.resize_nhwc) against the fp64 sum of
tests/kohya_refs.py with a derived bound; the executor's option against the reference UNet with the reference's own patches installed
(tests/golden/tiny_kohya_unet.pt, tools/make_kohya_fixtures.py); a windowed sampling run on the captured-graph path; the native route against
the same arithmetic as Python patches on the hooked executor."""
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import forge_amd  # noqa: E402,F401
from forge_amd import hipops as ops  # noqa: E402
from forge_amd import synth  # noqa: E402
from forge_amd.backend.diffusion_engine.base import build_engine  # noqa: E402
from forge_amd.backend.patcher.kohya_hrfix import KohyaHRFixParams, patch_kohya_hrfix  # noqa: E402
from forge_amd.modules import processing, shared  # noqa: E402

from conftest import load_golden  # noqa: E402
import kohya_refs as kr  # noqa: E402
import parity  # noqa: E402
from parity import check  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def fx():
    g = load_golden("tiny_kohya_unet.pt")
    # the fixture carries its own floors (the reference's fp16-storage runs, oracle/make_floor.py's mechanism): same gate as every floor-keyed check
    parity.FLOORS["tiny_kohya_unet.pt:eps_plain"] = g["floor_plain"]
    for i, c in enumerate(g["cases"]):
        parity.FLOORS[f"tiny_kohya_unet.pt:eps/{i}"] = c["floor"]
    parity.FLOORS["tiny_kohya_unet.pt:euler4/latent"] = g["euler4"]["floor"]
    return g


def make_engine(fx):
    cfg = fx["config"]
    return build_engine(cfg, synth.synth_unet_state_dict(cfg, seed=0), None, None, device=DEV)


@pytest.fixture(scope="module")
def engine(fx):
    return make_engine(fx)


def params_of(case, sigma_start=999999999.9, sigma_end=0.0):
    return KohyaHRFixParams(case["block_number"], case["downscale_factor"], case["start_percent"], case["end_percent"], case["downscale_after_skip"],
                            case["downscale_method"], case["upscale_method"], sigma_start, sigma_end)


def test_kernel_vs_fp64_on_every_case():
    """every case twice with the same bits; |got - ref| <= 1/2 ulp_fp16(ref) + (ky kx + 2) 2^-24 sum |w_y w_x x| per element (kohya_refs.kernel_bound)"""
    for i, (shape, size, mode) in enumerate(kr.KERNEL_CASES):
        x16 = kr.case_input(i, shape).permute(0, 2, 3, 1).contiguous().half()          # NHWC fp16
        tabs = kr.tables(shape[2], shape[3], size[0], size[1], mode)
        ref = kr.resize_ref(x16, tabs)
        bound = kr.kernel_bound(x16, tabs, ref)
        xd = x16.to(DEV)
        runs = [ops.resize_nhwc(xd, size, mode) for _ in range(2)]
        torch.cuda.synchronize()
        got = runs[0].cpu()
        assert got.dtype == torch.float16 and tuple(got.shape) == (shape[0], size[0], size[1], shape[1]) and runs[0].is_contiguous()
        assert runs[0].data_ptr() != runs[1].data_ptr() and torch.equal(got, runs[1].cpu()), (shape, size, mode)
        assert ops._attached_stats(runs[0]) is None                                    # a fresh tensor: the next GroupNorm takes its own pass
        ratio = float(((got.double() - ref).abs() / bound).max())
        print(shape, "->", size, mode, "taps", tabs[1].shape[1], "x", tabs[3].shape[1], "worst |got - ref| / bound", round(ratio, 4))
        assert ratio <= 1.0, (shape, size, mode, ratio)
        assert float(ref.abs().max()) > 0.5                                            # the case computes something


def test_unet_forward_with_shrink_vs_reference(fx, engine, monkeypatch):
    net = engine.forge_objects.unet.model.diffusion_model
    x, t, ctx = fx["x"].to(DEV), fx["t"].to(DEV), fx["ctx"].to(DEV)
    assert tuple(fx["x"].shape) == (2, 4, 32, 24) and fx["t"].tolist() == [601.0, 187.0] and fx["config"] == synth.TINY_SD15_UNET_CONFIG
    want_cases = [(2, 2.0, True, "bicubic", "bicubic"), (2, 1.5, True, "bicubic", "bicubic"), (1, 2.0, False, "bilinear", "nearest-exact"),
                  (3, 1.5, True, "area", "bilinear")]
    assert [(c["block_number"], c["downscale_factor"], c["downscale_after_skip"], c["downscale_method"], c["upscale_method"]) for c in fx["cases"]] == want_cases
    plain = net.forward(x, t, context=ctx)
    check("tiny_kohya unet forward without the option vs the reference's plain forward", plain, fx["eps_plain"], floor="tiny_kohya_unet.pt:eps_plain")
    for i, c in enumerate(fx["cases"]):
        key = f"tiny_kohya_unet.pt:eps/{i}"
        gate = parity.limits(key)[1]["max_rel"]
        moved = parity.max_rel(c["eps"], fx["eps_plain"])
        assert moved > 10 * gate, (i, moved, gate)             # an executor that ignores the option cannot pass the check below
        taps = []
        monkeypatch.setattr(net, "tap", lambda name, tt: taps.append((name, tuple(tt.shape[1:3]))) if name.endswith(".shrink") else None, raising=False)
        eps = net.forward(x, t, context=ctx, transformer_options={"kohya_hrfix": params_of(c)})
        monkeypatch.setattr(net, "tap", None, raising=False)
        check(f"tiny_kohya unet forward, case {i} {want_cases[i]}: native shrink vs the reference with its patches", eps, c["eps"], floor=key)
        assert taps == [(f"{where}.{blk}.shrink", tuple(hw)) for where, blk, hw in c["resized"]], (taps, c["resized"])
    # the fourth case: the Upsample goes from 6 x 4 straight to the stored skip's 16 x 12 and no output block resizes
    assert [w for w, _, _ in fx["cases"][3]["resized"]] == ["input"]


def run_job(eng, fx, unet=None):
    e4, cfg = fx["euler4"], fx["config"]
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


def test_windowed_sampling_on_the_graph_path(fx, engine, monkeypatch):
    """4-step Euler, CFG 7, the window closed between the second and the third step, as the fixture's run of the reference's sampler with the
    reference's patches: two shrunk steps on one captured graph, two plain steps on another, no hooked forward, nothing read back"""
    e4 = fx["euler4"]
    assert e4["active"] == [True, True, False, False]
    km = engine.forge_objects.unet.model
    net = km.diffusion_model
    calls, hooked = [], []
    real = ops.resize_nhwc
    monkeypatch.setattr(ops, "resize_nhwc", lambda *a, **kw: (calls.append(a[1:]), real(*a, **kw))[1])
    real_hooked = net._attn_block_hooked
    monkeypatch.setattr(net, "_attn_block_hooked", lambda *a, **kw: (hooked.append(1), real_hooked(*a, **kw))[1], raising=False)
    real_hooks = net._hooks
    hook_dicts = []
    monkeypatch.setattr(net, "_hooks", lambda to: (lambda r: (hook_dicts.append(r is not None), r)[1])(real_hooks(to)), raising=False)
    unet = patch_kohya_hrfix(engine.forge_objects.unet, **e4["params"])
    p = unet.model_options["transformer_options"]["kohya_hrfix"]
    assert [p.sigma_end <= s <= p.sigma_start for s in e4["sigmas"][:4]] == e4["active"]
    km._drop_graphs()
    lat = run_job(engine, fx, unet)
    check("tiny_kohya 4-step Euler with windowed native shrink vs reference", lat, e4["latent"], floor="tiny_kohya_unet.pt:euler4/latent")
    keys = list(km._graphs)
    assert len(keys) == 2 and sorted("kohya_hrfix" in k for k in keys) == [False, True], keys
    assert [k for k in keys if "kohya_hrfix" in k][0][-6:] == ("kohya_hrfix", 2, 2.0, True, "bicubic", "bicubic")
    assert hooked == [] and hook_dicts and not any(hook_dicts)
    # two shrunk steps, two resizes each: the eager warm-up runs and one capture call Python, the replay launches from the graph
    assert len(calls) % 2 == 0 and 4 <= len(calls) <= 6, calls
    assert set(calls) == {((4, 4), "bicubic"), ((8, 8), "bicubic")}
    km.use_graph = False
    try:
        eager = run_job(engine, fx, unet)
    finally:
        km.use_graph = True
    assert torch.equal(eager, lat)
    # a following job without the option on the same engine: the result of an engine that never saw it, bit for bit, and no resize launch
    n0 = len(calls)
    after = run_job(engine, fx)
    fresh = run_job(make_engine(fx), fx)
    assert torch.equal(after, fresh) and len(calls) == n0
    assert parity.max_rel(after, lat) > 1e-2


def test_native_route_vs_python_patches_on_the_hooked_executor(fx, engine, monkeypatch):
    """the first fixture case as the native option and as the reference's two patch functions restated with F.interpolate (tests/kohya_refs.py):
    a shape-changing input_block_patch_after_skip and output_block_patch through the hooked executor"""
    net = engine.forge_objects.unet.model.diffusion_model
    x, t, ctx = fx["x"].to(DEV), fx["t"].to(DEV), fx["ctx"].to(DEV)
    c = fx["cases"][0]
    hooked, calls, resized = [], [], []
    real_hooked = net._attn_block_hooked
    monkeypatch.setattr(net, "_attn_block_hooked", lambda *a, **kw: (hooked.append(1), real_hooked(*a, **kw))[1], raising=False)
    real = ops.resize_nhwc
    monkeypatch.setattr(ops, "resize_nhwc", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    native = net.forward(x, t, context=ctx, transformer_options={"kohya_hrfix": params_of(c)}).clone()
    assert hooked == [] and len(calls) == 2
    ip, op = kr.python_patches(c["block_number"], c["downscale_factor"], 999999999.9, 0.0, c["downscale_method"], c["upscale_method"], resized)
    to = {"patches": {"input_block_patch_after_skip": [ip], "output_block_patch": [op]}, "sigmas": fx["sigmas"].to(DEV)}
    via_patches = net.forward(x, t, context=ctx, transformer_options=to)
    assert len(hooked) > 0 and len(calls) == 2                       # the patch lists ran on the hooked executor; no native resize there
    assert [(w, b) for w, b in resized] == [(w, b) for w, b, _ in c["resized"]]
    check("tiny_kohya unet forward: native shrink vs the Python patch route", native, via_patches, floor="tiny_kohya_unet.pt:eps/0", both_fp16=True)
    check("tiny_kohya unet forward: the Python patch route vs the reference", via_patches, c["eps"], floor="tiny_kohya_unet.pt:eps/0")
