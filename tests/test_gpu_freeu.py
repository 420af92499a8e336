"""GPU: native FreeU.  The kernels fmx_freeu_reduce_f16 / fmx_freeu_apply_f16 (through hipops.freeu) against the fp64 closed form of
tests/freeu_refs.py, which tests/test_freeu_host.py pins to the real reference; the executor's option against the reference UNet with the
reference's own FreeU patch installed (tests/golden/tiny_freeu_unet.pt, tools/make_freeu_fixtures.py); the native route against a Python
output_block_patch; a windowed sampling run on the captured-graph path."""
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import forge_amd  # noqa: E402,F401
from forge_amd import _lib  # noqa: E402
from forge_amd import hipops as ops  # noqa: E402
from forge_amd import synth  # noqa: E402
from forge_amd.backend.diffusion_engine.base import build_engine  # noqa: E402
from forge_amd.backend.patcher.freeu import FreeUParams, patch_freeu_v2  # noqa: E402
from forge_amd.modules import processing, sd_samplers_common, shared  # noqa: E402

from conftest import load_golden  # noqa: E402
import freeu_refs as fr  # noqa: E402
import parity  # noqa: E402
from parity import check  # noqa: E402

DEV = "cuda"
FREEU_BLOCKS = (0, 1, 2, 3, 4)   # the output blocks of the fixture's UNet whose h has 4x or 2x model_channels channels


@pytest.fixture(scope="module")
def fx():
    g = load_golden("tiny_freeu_unet.pt")
    # the fixture carries its own floors (the reference's fp16-storage runs, oracle/make_floor.py's mechanism): same gate as every floor-keyed check
    parity.FLOORS["tiny_freeu_unet.pt:eps"] = g["floor"]
    parity.FLOORS["tiny_freeu_unet.pt:eps_plain"] = g["floor_plain"]
    parity.FLOORS["tiny_freeu_unet.pt:euler4/latent"] = g["euler4"]["floor"]
    return g


def make_engine(fx):
    cfg = fx["config"]
    return build_engine(cfg, synth.synth_unet_state_dict(cfg, seed=0), None, None, device=DEV)


@pytest.fixture(scope="module")
def engine(fx):
    return make_engine(fx)


class _ChunkSpy:
    """the library, with the pixel-chunk count of every fmx_freeu_reduce_f16 / fmx_freeu_apply_f16 call noted on the way through"""

    def __init__(self, real, seen):
        self._real, self._seen = real, seen

    def __getattr__(self, name):
        f = getattr(self._real, name)
        if name in ("fmx_freeu_reduce_f16", "fmx_freeu_apply_f16"):
            return lambda *a: (self._seen.append(a[8]), f(*a))[1]      # (h, c_h, skip, c_s, n, hh, ww, trig, nchunks, ...)
        return f


def test_kernels_vs_fp64_on_every_case(monkeypatch):
    """fmx_freeu_reduce_f16 + fmx_freeu_apply_f16: every output element is the fp64 result rounded to fp16 or its neighbour; the half of h that
    FreeU does not scale keeps its bits; two runs give the same bits; the 48 x 40 case spans 8 pixel chunks, the last one half full."""
    chunks, real_lib = [], _lib.lib()
    monkeypatch.setattr(_lib, "lib", lambda: _ChunkSpy(real_lib, chunks))
    for c in load_golden("freeu_ops.pt")["cases"]:
        del chunks[:]
        h, hsp = fr.case_inputs(c)
        r_h, r_s = fr.freeu_ref(h, hsp, c["b"], c["s"])
        h16, s16 = fr.nhwc16(h), fr.nhwc16(hsp)
        runs = []
        for _ in range(2):
            gh, gs = h16.to(DEV), s16.to(DEV)
            oh, os_ = ops.freeu(gh, gs, c["b"], c["s"])
            assert oh is gh and os_ is gs                      # in place
            torch.cuda.synchronize()
            runs.append((gh.cpu(), gs.cpu()))
        hw = c["shape"][3] * c["shape"][4]
        assert chunks == [-(-hw // 256)] * 4                   # what the wrapper passed: reduce and apply, two runs
        if tuple(c["shape"][3:]) == (48, 40):
            assert chunks[0] == 8 and hw % 256 == 128
        (g_h, g_s) = runs[0]
        assert torch.equal(g_h, runs[1][0]) and torch.equal(g_s, runs[1][1]), c["shape"]
        d_h, d_s = int(fr.ulp_distance_f16(g_h, fr.nhwc16(r_h)).max()), int(fr.ulp_distance_f16(g_s, fr.nhwc16(r_s)).max())
        print(c["shape"], "worst fp16 ulp distance: h", d_h, "skip", d_s)
        assert d_h <= 1 and d_s <= 1, (c["shape"], d_h, d_s)
        c_h = c["shape"][1]
        assert torch.equal(g_h[..., c_h // 2:], h16[..., c_h // 2:])
        assert not torch.equal(g_h[..., :c_h // 2], h16[..., :c_h // 2]) and not torch.equal(g_s, s16)


def test_unet_forward_with_freeu_vs_reference(fx, engine):
    net = engine.forge_objects.unet.model.diffusion_model
    x, t, ctx = fx["x"].to(DEV), fx["t"].to(DEV), fx["ctx"].to(DEV)
    gate = max(parity.limits("tiny_freeu_unet.pt:eps")[1]["max_rel"], parity.limits("tiny_freeu_unet.pt:eps_plain")[1]["max_rel"])
    moved = parity.max_rel(fx["eps_freeu"], fx["eps_plain"])
    assert moved > 10 * gate, (moved, gate)                   # an executor that ignores the option cannot pass the first check below
    eps = net.forward(x, t, context=ctx, transformer_options={"freeu_v2": FreeUParams(**fx["params"])})
    check("tiny_freeu unet forward with native FreeU vs the reference with its FreeU patch", eps, fx["eps_freeu"], floor="tiny_freeu_unet.pt:eps")
    plain = net.forward(x, t, context=ctx)
    check("tiny_freeu unet forward without the option vs the reference's plain forward", plain, fx["eps_plain"], floor="tiny_freeu_unet.pt:eps_plain")


def test_native_route_vs_a_python_output_block_patch(fx, engine, monkeypatch):
    """The same engine with FreeU as a Python output_block_patch (tests/freeu_refs.py in fp32 on the device, no FFT).  A hooked forward runs
    other kernels upstream (the hooked transformer blocks keep their LayerNorms unfolded), so the two routes' FreeU INPUTS differ in their last
    bits and the tensors tapped on the two routes cannot agree to 1 ulp.  The 1-ulp statement is therefore made on identical inputs: every
    hook call also runs ops.freeu on a copy of what the hook received.  The tapped tensors of the native route are held against what the
    Python patch returned at the same block by the gate of the UNet output (two fp16-storage runs of one network: an activation inside the
    network has passed fewer rounding sites than the output that the gate's floor was measured on)."""
    net = engine.forge_objects.unet.model.diffusion_model
    x, t, ctx = fx["x"].to(DEV), fx["t"].to(DEV), fx["ctx"].to(DEV)
    p = FreeUParams(**fx["params"])
    mc = fx["config"]["model_channels"]
    scales = {4 * mc: (p.b1, p.s1), 2 * mc: (p.b2, p.s2)}
    hook_calls, worst, patched = [], [], {}

    def patch(h, hsp, to):
        hook_calls.append(to["block"])
        sc = scales.get(h.shape[1])
        if sc is None:
            return h, hsp
        kh, ks = ops.freeu(h.permute(0, 2, 3, 1).contiguous().clone(), hsp.permute(0, 2, 3, 1).contiguous().clone(), *sc)   # copies: freeu works in place
        rh, rs = fr.freeu_ref(h, hsp, *sc, dtype=torch.float32)
        worst.append((to["block"], int(fr.ulp_distance_f16(kh.cpu(), fr.nhwc16(rh.cpu())).max()), int(fr.ulp_distance_f16(ks.cpu(), fr.nhwc16(rs.cpu())).max())))
        patched[f"output.{to['block'][1]}.freeu.h"], patched[f"output.{to['block'][1]}.freeu.skip"] = fr.nhwc16(rh), fr.nhwc16(rs)
        return rh, rs

    taps = {}
    calls = []
    real = ops.freeu
    monkeypatch.setattr(ops, "freeu", lambda *a: (calls.append(1), real(*a))[1])
    monkeypatch.setattr(net, "tap", lambda name, tt: taps.__setitem__(name, tt.clone()) if ".freeu." in name else None, raising=False)
    native = net.forward(x, t, context=ctx, transformer_options={"freeu_v2": p}).clone()
    monkeypatch.setattr(net, "tap", None, raising=False)
    # channel_mult (1, 2, 4), one ResBlock per level: h has 256, 256, 256, 128, 128, 64 channels at the six output blocks -- three on the 4x rule, two on the 2x rule
    assert hook_calls == [] and len(calls) == len(FREEU_BLOCKS)
    assert sorted(taps) == sorted(f"output.{bi}.freeu.{w}" for bi in FREEU_BLOCKS for w in ("h", "skip"))
    hooked = net.forward(x, t, context=ctx, transformer_options={"patches": {"output_block_patch": [patch]}})
    assert len(hook_calls) == len(fx["config"]["channel_mult"]) * 2 and [b for b, _, _ in worst] == [("output", bi) for bi in FREEU_BLOCKS]
    print("kernel vs the Python patch on the patch's own inputs, fp16 ulps (block, h, skip):", worst)
    assert all(dh <= 1 and ds <= 1 for _, dh, ds in worst), worst
    check("tiny_freeu unet forward: native FreeU vs the Python patch route", native, hooked, floor="tiny_freeu_unet.pt:eps", both_fp16=True)
    assert sorted(patched) == sorted(taps)
    for name in sorted(taps):
        check(f"tiny_freeu {name}: tapped on the native route vs returned by the Python patch", taps[name], patched[name], floor="tiny_freeu_unet.pt:eps",
              both_fp16=True)
    # without the option nothing is launched for FreeU
    n0 = len(calls)
    net.forward(x, t, context=ctx)
    assert len(calls) == n0


def run_job(eng, fx, unet=None, steps=None):
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
                                                        steps=steps or e4["steps"], cfg_scale=7.0, width=e4["hw"] * 8, height=e4["hw"] * 8, do_decode=False)
        return processing.process_images(p).latents.clone()
    finally:
        eng.forge_objects_after_applying_lora = saved
        eng.forge_objects = saved.shallow_copy()


def test_windowed_sampling_on_the_graph_path(fx, engine, monkeypatch):
    """4-step Euler, CFG 7, FreeU in the window [0, 0.34]: on for the model calls 0 and 1, off for 2 and 3, as the fixture's reference run.
    The fixture numbers the model calls 0..3; the UI's progress counter (state.sampling_step, what the reference's callback also reads) is
    written after a step and so runs one call behind: it is advanced here so that call i sees position i / 3."""
    e4 = fx["euler4"]
    assert e4["active"] == [True, True, False, False]
    monkeypatch.setattr(sd_samplers_common.Sampler, "callback_state", lambda self, d: setattr(shared.state, "sampling_step", d["i"] + 1))
    km = engine.forge_objects.unet.model
    calls = []
    real = ops.freeu
    monkeypatch.setattr(ops, "freeu", lambda *a: (calls.append(1), real(*a))[1])
    p = FreeUParams(**fx["params"])
    unet = patch_freeu_v2(engine.forge_objects.unet, p.b1, p.b2, p.s1, p.s2, start=e4["start"], end=e4["end"])
    km._drop_graphs()
    lat = run_job(engine, fx, unet)
    check("tiny_freeu 4-step Euler with windowed native FreeU vs reference", lat, e4["latent"], floor="tiny_freeu_unet.pt:euler4/latent")
    keys = list(km._graphs)
    assert len(keys) == 2 and sorted("freeu" in k for k in keys) == [False, True], keys
    assert [k for k in keys if "freeu" in k][0][-5:] == ("freeu", p.b1, p.b2, p.s1, p.s2)
    # two FreeU steps, five blocks each: eager warm-up runs and one capture call Python, replays launch from the graph
    nb = len(FREEU_BLOCKS)
    assert len(calls) % nb == 0 and 2 * nb <= len(calls) <= 3 * nb, len(calls)
    km.use_graph = False
    try:
        eager = run_job(engine, fx, unet)
    finally:
        km.use_graph = True
    assert torch.equal(eager, lat)
    # a following job without FreeU on the same engine: the result of an engine that never saw FreeU, bit for bit, and no FreeU launch
    n0 = len(calls)
    after = run_job(engine, fx)
    fresh = run_job(make_engine(fx), fx)
    assert torch.equal(after, fresh) and len(calls) == n0
    assert parity.max_rel(after, lat) > 1e-2
