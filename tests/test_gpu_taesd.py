"""GPU (MI355X) tests of the native TAESD decoder: the 64 -> 64 direct convolution fmx_conv3x3_c64 (ops.conv3x3_c64), fmx_taesd_pack_latent
(ops.taesd_pack_latent) and fmx_latent_rgb (ops.latent_rgb) against fp64; the executor forge_amd.backend.nn.taesd.TAESDDecoder against the REAL
reference's fp32 output (tests/golden/taesd.pt, tools/make_taesd_fixtures.py) and, layer by layer, against the rounded fp64 restatement
(tests/taesd_refs.py); the call surface (decode method, live previews).

Kernel level follows tests/test_gpu_vae_direct.py: sentinel-filled oversize destinations that must be bit-identical outside the written window,
inputs as ROW windows of buffers holding 30000 around them (so image 0's top border and the last image's bottom border have 30000 next to them in
memory where the kernel must see zeros; n = 2 shows a halo read into the neighbouring image), references in fp64 on the rounded inputs, tolerance
kernel_refs.CONV_TOL (same arithmetic: fp32 accumulation over K = 576, fp32 epilogue adds, one rounding).  The kernel's tile is 8 x 32 output pixels."""
import ctypes as C
import math
from functools import lru_cache

import pytest
import torch

pytestmark = pytest.mark.gpu

import forge_amd  # noqa: E402,F401
from forge_amd import hipops as ops  # noqa: E402

import kernel_refs as R  # noqa: E402
import taesd_refs as T  # noqa: E402
from test_gpu_gemm_windows import Win, changed_outside, gen, rnd, sentinel_buffer  # noqa: E402

DEV = "cuda"
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
# (n, h, w) of the INPUT: sub-tile; one past an 8 x 32 tile in both directions; whole tiles
SHAPES = [(2, 5, 7), (2, 9, 33), (1, 16, 64)]
# with up2x: 10 x 14 (sub-tile) and 10 x 34 (one past the tile in both directions of the OUTPUT)
UP_SHAPES = [(2, 5, 7), (1, 5, 17)]
VARIANTS = ("bias", "bias_relu", "bias_residual_relu")
# 2 x 5 x 33 = 330 tiles, ragged in both directions: more tiles than the device has CUs, so persistent workgroups walk on to a SECOND tile (some of them:
# the others take one), staged into the other LDS buffer under the first one's MFMA loop, and the second tiles lie in the other image
WALK_SHAPE = (2, 37, 1050)


def tap_major(wt):
    return wt.permute(0, 2, 3, 1).reshape(wt.shape[0], -1).contiguous()


@lru_cache(maxsize=None)
def c64_case(shape, dtype, up):
    n, h, w = shape
    seed = 9100 + 17 * h + w + (1000 if up else 0)
    m = n * (h << up) * (w << up)
    return dict(x=rnd(n, h, w, 64, seed=seed, dtype=dtype), wt=rnd(64, 64, 3, 3, scale=1 / math.sqrt(576), seed=seed + 1, dtype=dtype),
                bias=rnd(64, scale=0.5, seed=seed + 2, dtype=dtype), res=rnd(m, 64, seed=seed + 3, dtype=dtype), m=m)


@lru_cache(maxsize=None)
def c64_ref(shape, dtype, up, bias, residual, relu):
    k = c64_case(shape, dtype, up)
    n, h, w = shape
    y = R.conv_ref(k["x"], k["wt"], k["bias"] if bias else None, up=(2 * h, 2 * w) if up else None, residual=k["res"] if residual else None)
    y = y.reshape(k["m"], 64)
    return torch.relu(y) if relu else y


def assert_tiles_exceed_cus(n, oh, ow):
    """the tile walk of a persistent kernel is covered only while a launch has more 8 x 32 tiles than the device has CUs"""
    from forge_amd import _lib
    cus = C.c_int(0)
    _lib.check(_lib.lib().fmx_device_info(C.byref(cus), None, None, 0), "fmx_device_info")
    tiles = n * ((oh + 7) // 8) * ((ow + 31) // 32)
    assert tiles > cus.value > 0, f"{tiles} tiles on {cus.value} CUs: no workgroup walks to a second tile"


def run_c64(shape, dtype, up, bias, residual, relu, what):
    k = c64_case(shape, dtype, up)
    n, h, w = shape
    m = k["m"]
    if shape == WALK_SHAPE:
        assert_tiles_exceed_cus(n, h << up, w << up)
    x = Win(k["x"].reshape(n * h * w, 64), 2, 3).on(DEV).view(n, h, w, 64)
    wk = Win(tap_major(k["wt"]), 1, 2).on(DEV)
    b = Win(k["bias"], left=8, right=8).on(DEV) if bias else None
    res = Win(k["res"], 3, 2, 4, 4).on(DEV) if residual else None          # columns [4, 68) of a 72-wide buffer: ld_res = 72
    buf = sentinel_buffer(2 + m + 3, 96, dtype)                           # the output: columns [16, 80) of a 96-wide buffer: ld_out = 96
    rows, cols = slice(2, 2 + m), slice(16, 80)
    dbuf = buf.to(DEV)
    ops.conv3x3_c64(x, wk, b, residual=res, relu=relu, up2x=up, out=dbuf[rows, cols])
    torch.cuda.synchronize()
    after = dbuf.cpu()
    assert changed_outside(buf, after, rows, cols) == 0, f"{what}: wrote outside its output window"
    want = c64_ref(shape, dtype, up, bias, residual, relu)
    e = R.excess(after[rows, cols], want, dtype, *R.CONV_TOL[dtype])
    print(f"[taesd] {what}: {e:.3f} x CONV_TOL")
    assert e <= 1.0, f"{what}: error {e:.3g}x CONV_TOL"


def case_id(*parts):
    return "-".join("x".join(map(str, p)) if isinstance(p, tuple) else str(p) for p in parts)


C64_CASES = [(s, v, d) for d in DTYPES for v in VARIANTS for s in SHAPES] + [(WALK_SHAPE, "bias_residual_relu", d) for d in DTYPES]


@pytest.mark.parametrize("shape,variant,dt", C64_CASES, ids=[case_id(*c) for c in C64_CASES])
def test_conv3x3_c64(shape, variant, dt):
    run_c64(shape, DTYPES[dt], False, True, "residual" in variant, "relu" in variant, f"conv3x3_c64 {shape} {variant} {dt}")


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("shape", UP_SHAPES + SHAPES[1:], ids=lambda s: "x".join(map(str, s)))
def test_conv3x3_c64_up2x_no_bias(shape, dt):
    run_c64(shape, DTYPES[dt], True, False, False, False, f"conv3x3_c64 up2x {shape} {dt}")


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("shape", UP_SHAPES[1:], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("variant", VARIANTS)
def test_conv3x3_c64_up2x_epilogues(shape, variant, dt):
    run_c64(shape, DTYPES[dt], True, True, "residual" in variant, "relu" in variant, f"conv3x3_c64 up2x {shape} {variant} {dt}")


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("lc", [4, 16, 64])
def test_taesd_pack_latent(lc, dt):
    dtype = DTYPES[dt]
    z = 4.0 * torch.randn(2, lc, 5, 7, generator=gen(77 + lc))
    z[0, 0, 0, :4] = torch.tensor([12.0, -12.0, 0.0, 3.0])
    z[1, lc - 1, 4, 6] = -12.0
    buf = sentinel_buffer(2 * 5 * 7 + 3, 64, dtype)
    dbuf = buf.to(DEV)
    ops.taesd_pack_latent(z.to(DEV), out=dbuf[:70].view(2, 5, 7, 64))
    torch.cuda.synchronize()
    after = dbuf.cpu()
    assert changed_outside(buf, after, slice(0, 70), slice(0, 64)) == 0
    got = after[:70].view(2, 5, 7, 64)
    want = torch.tanh(R.rounded(z.permute(0, 2, 3, 1), dtype) / 3) * 3                 # exact, of the ROUNDED latent (|x| = 12 -> 2.998)
    R.assert_within(got[..., :lc], want, dtype, *R.ELEM_TOL[dtype], f"taesd_pack_latent L={lc} {dt}")
    assert bool((got[..., lc:] == 0).all()), "channels >= L must be zeros"


def test_latent_rgb():
    fx = fixture()
    z, fac = fx["cases"]["l4"]["latent"], fx["rgb_factors"]
    got = ops.latent_rgb(z.to(DEV), fac)
    want = torch.einsum("blxy,lr->brxy", z.double(), fac.double())
    assert R.excess(got, want, torch.float32, *R.F32_TOL) <= 1.0
    torch.testing.assert_close(got.cpu(), fx["rgb_out"], rtol=1e-5, atol=1e-5)          # the reference's own fp32 einsum
    z16 = torch.randn(1, 16, 9, 33, generator=gen(5))
    f16 = torch.randn(16, 3, generator=gen(6))
    assert R.excess(ops.latent_rgb(z16.to(DEV), f16.tolist()), torch.einsum("blxy,lr->brxy", z16.double(), f16.double()), torch.float32, *R.F32_TOL) <= 1.0


# ---- network level ------------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def fixture():
    return T.load_fixture()


@lru_cache(maxsize=None)
def native_run(case, dt):
    """-> (decoder, output fp32 NCHW on the CPU, taps) of one tapped decode"""
    from forge_amd.backend.nn.taesd import TAESDDecoder
    fx = fixture()
    lc = fx["cases"][case]["latent"].shape[1]
    dec = TAESDDecoder(T.state_dict_for(fx, lc), device=DEV, dtype=DTYPES[dt])
    assert dec.latent_channels == lc
    dec.tap = {}
    out = dec.decode(fx["cases"][case]["latent"].to(DEV)).cpu()
    taps, dec.tap = dec.tap, None
    return dec, out, taps


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("case", ["l4", "l16"])
def test_decoder_against_the_reference(case, dt):
    fx = fixture()
    c = fx["cases"][case]
    dec, out, _ = native_run(case, dt)
    assert out.shape == c["out"].shape and out.dtype == torch.float32
    m, lim, bad = T.network_bar(out, c["out"], c["fp16" if dt == "f16" else dt])
    print(f"[taesd] decode {case} {dt}: rms {m['rms']:.3e} (limit {lim['rms']:.3e})  max_rel {m['max_rel']:.3e} (limit {lim['max_rel']:.3e})")
    assert not bad, f"decode {case} {dt}: {bad} over the limit: {m} vs {lim}"
    again = dec.decode(c["latent"].to(DEV)).cpu()                                      # untapped, recycled arena: the same bits
    assert torch.equal(again, out)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("case", ["l4", "l16"])
def test_every_stored_tensor_teacher_forced(case, dt):
    """every stored tensor against the rounded restatement of ITS layer on the NATIVE inputs of that layer, at CONV_TOL (the clamp at ELEM_TOL)"""
    fx = fixture()
    dtype = DTYPES[dt]
    lc = fx["cases"][case]["latent"].shape[1]
    sd = T.state_dict_for(fx, lc)
    _, _, taps = native_run(case, dt)
    e0 = R.excess(taps["0"], torch.tanh(R.rounded(fx["cases"][case]["latent"], dtype) / 3) * 3, dtype, *R.ELEM_TOL[dtype])
    worst = ("-", 0.0)         # of the convolutions: the clamp has a bar of its own
    assert e0 <= 1.0, f"clamped latent: {e0:.3g}x ELEM_TOL"
    specs = T.layers()
    assert set(taps) == {"0"} | {s[0] for s in specs}
    for spec in specs:
        x = taps[spec[1]].double()
        if spec[1] == "0":
            assert x.shape[1] == lc
        want = T.layer_ref(sd, spec, x, taps[spec[4]].double() if spec[4] else None, dtype, exact=True)
        e = R.excess(taps[spec[0]], want, dtype, *R.CONV_TOL[dtype])
        if e > worst[1]:
            worst = (spec[0], e)
        assert e <= 1.0, f"layer {spec[0]} ({case}, {dt}): {e:.3g}x CONV_TOL"
    print(f"[taesd] teacher-forced {case} {dt}: worst layer {worst[0]} at {worst[1]:.3f} x CONV_TOL")


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("case", ["l4", "l16"])
def test_preview_image_levels(case, dt):
    c = fixture()["cases"][case]
    _, out, _ = native_run(case, dt)
    got = T.image_tail(out[0]).int()
    allowed = 1 + math.ceil(255 * c["fp16" if dt == "f16" else dt]["floor_max_abs"])
    worst = int((got - c["image_u8"].int()).abs().max())
    print(f"[taesd] preview {case} {dt}: worst level difference {worst} (allowed {allowed})")
    assert worst <= allowed


# ---- call surface -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def tiny_engine(tmp_path, monkeypatch):
    """a tiny SD1.5-shaped engine with a VAE, and the fixture decoder as <models_path>/VAE-taesd/taesd_decoder.pth"""
    from forge_amd import synth
    from forge_amd.backend.diffusion_engine.base import build_engine
    from forge_amd.modules import sd_vae_taesd, shared
    cfg = synth.TINY_SD15_UNET_CONFIG
    eng = build_engine(cfg, synth.synth_unet_state_dict(cfg, seed=0), synth.TINY_VAE_CONFIG, synth.synth_vae_decoder_state_dict(synth.TINY_VAE_CONFIG, seed=1), device=DEV)
    (tmp_path / "VAE-taesd").mkdir()
    torch.save(T.state_dict_for(fixture(), 4), tmp_path / "VAE-taesd" / "taesd_decoder.pth")
    monkeypatch.setattr(shared, "models_path", str(tmp_path))
    monkeypatch.setattr(shared, "sd_model", eng)
    monkeypatch.setattr(shared, "state", shared.State())
    monkeypatch.setattr(sd_vae_taesd, "sd_vae_taesd_models", {})
    return eng, cfg


def test_decode_method_routes_final_images(tiny_engine, monkeypatch):
    from forge_amd.modules import processing, sd_samplers_common, shared
    eng, _ = tiny_engine
    z = fixture()["cases"]["l4"]["latent"].to(DEV)
    full = eng.decode_first_stage(z)
    assert torch.equal(processing.decode_first_stage(eng, z), full)                       # "Full": what it returned before
    monkeypatch.setattr(shared.opts, "sd_vae_decode_method", "TAESD")
    got = processing.decode_first_stage(eng, z)
    assert torch.equal(got, sd_samplers_common.samples_to_images_tensor(z, 3))
    want = fixture()["cases"]["l4"]["out"] * 2 - 1
    assert got.shape == want.shape and float((got.cpu() - want).abs().max()) < 0.01        # 8 x the latent, whatever the engine's own VAE does
    assert [tuple(x.shape) for x in processing.decode_latent_batch(eng, z)] == [tuple(want.shape[1:])] * 2


def test_live_previews_during_sampling(tiny_engine, monkeypatch):
    from forge_amd import synth
    from forge_amd.modules import processing, sd_samplers_common, shared
    eng, cfg = tiny_engine
    c, uc = synth.synth_conditioning(2, cfg["context_dim"], None, seed=1234)

    def job():
        shared.state = st = shared.State()
        p = processing.StableDiffusionProcessingTxt2Img(sd_model=eng, c=c.to(DEV), uc=uc.to(DEV), seed=3, sampler_name="Euler", batch_size=2, steps=5,
                                                        width=128, height=96)
        return processing.process_images(p).latents.clone(), st

    made, seen = [], []
    real, preview = sd_samplers_common.samples_to_images_tensor, sd_samplers_common.sample_to_image

    def counted(samples, *a, **k):        # the preview's entry point (the final decode goes through decode_first_stage)
        made.append(shared.state.sampling_step)
        seen.append(samples[:1].clone())
        return preview(samples, *a, **k)
    monkeypatch.setattr(sd_samplers_common, "sample_to_image", counted)
    off, st = job()
    assert made == [] and st.current_image is None and st.id_live_preview == 0               # previews off: the preview path is never entered
    for k, v in dict(live_previews_enable=True, show_progress_every_n_steps=2, show_progress_type="TAESD").items():
        monkeypatch.setattr(shared.opts, k, v)
    on, st = job()
    # the denoiser calls of a 5-step Euler run see state.sampling_step = 0, 0, 1, 2, 3 (the sampler's callback sets it to i AFTER step i,
    # modules/sd_samplers_common.py:271 of the reference): the rule `sampling_step % 2 == 0` fires on the first, second and fourth call
    assert made == [0, 0, 2] and st.id_live_preview == 3
    assert st.current_image.size == (128, 96) and st.current_image.mode == "RGB"             # 8 x the 16 x 12 latent
    assert torch.equal(on, off), "previews changed the sampled latents"
    want = (real(seen[-1], 3)[0] * 0.5 + 0.5).float().cpu().clamp(0.0, 1.0).mul(255.0).round().to(torch.uint8).permute(1, 2, 0)
    import numpy as np
    assert np.array_equal(np.asarray(st.current_image), want.numpy())                        # sample 0 of the latent of the last due call
