"""GPU (MI355X) tests of the native ESRGAN upscalers: the dense-block convolution fmx_conv3x3_dense_f16 (ops.conv3x3_dense) and the pixel kernels
fmx_esrgan_pack_image / fmx_esrgan_unpack_image against fp64 / the numpy formulas; the executor forge_amd.backend.nn.esrgan.RRDBNet against the
restatements of tests/esrgan_refs.py; the call surface (hires fix with an image-space upscaler).

Kernel level follows tests/test_gpu_taesd.py: inputs as windows of buffers holding 30000 around them (rows above and below, and -- the input's pixel
pitch being wider than cin -- the columns right of the channels the kernel may read; n = 2 shows a halo read into the neighbouring image),
sentinel-filled oversize destinations that must be bit-identical outside the written window, references in fp64 on the rounded inputs, tolerance
kernel_refs.CONV_TOL (fp32 accumulation over K = 9 cin <= 1728, fp32 epilogue, one rounding).  The kernel's tile is 8 x 32 output pixels, so the
shapes are the TAESD ones: sub-tile, one past the tile in both directions, whole tiles."""
import math
from functools import lru_cache

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import forge_amd  # noqa: E402,F401
from forge_amd import hipops as ops  # noqa: E402

import kernel_refs as R  # noqa: E402
from test_gpu_gemm_windows import Win, changed_outside, gen, rnd, sentinel_buffer  # noqa: E402
from test_gpu_taesd import WALK_SHAPE, assert_tiles_exceed_cus, case_id  # noqa: E402

DEV = "cuda"
H16 = torch.float16
SHAPES = [(2, 5, 7), (2, 9, 33), (1, 16, 64)]
UP_SHAPES = [(2, 5, 7), (1, 5, 17)]
CINS = (64, 96, 128, 160, 192)
COUTS = (32, 64)
F02 = float(torch.tensor(0.2, dtype=torch.float32))          # the value the kernel receives for 0.2
# name -> (slope, alpha or None, beta or None)
EPILOGUES = {"bias": (1.0, None, None), "slope": (F02, None, None), "res1": (1.0, F02, None), "res1_res2": (F02, F02, F02)}
WORST = {}


def tap_major(wt):
    return wt.permute(0, 2, 3, 1).reshape(wt.shape[0], -1).contiguous()


@lru_cache(maxsize=None)
def dense_case(shape, cin, cout, up):
    n, h, w = shape
    seed = 7300 + 131 * h + 7 * w + cin + 3 * cout + (1000 if up else 0)
    m = n * (h << up) * (w << up)
    return dict(x=rnd(n, h, w, cin, seed=seed), wt=rnd(cout, cin, 3, 3, scale=1 / math.sqrt(9 * cin), seed=seed + 1), bias=rnd(cout, scale=0.5, seed=seed + 2),
                res1=rnd(m, cout, seed=seed + 3), res2=rnd(m, cout, seed=seed + 4), m=m)


def dense_ref(k, shape, up, slope, alpha, beta, res1=None):
    n, h, w = shape
    y = R.conv_ref(k["x"], k["wt"], k["bias"], up=(2 * h, 2 * w) if up else None).reshape(k["m"], -1)
    y = torch.where(y >= 0, y, slope * y)
    if alpha is not None:
        y = alpha * y + (k["res1"] if res1 is None else res1).double()
    if beta is not None:
        y = beta * y + k["res2"].double()
    return y


def x_window(values, n, h, w, cin, right=8):
    """the input as channels [0, cin) of pixels of pitch cin + right, 30000 in the pad columns and in rows above and below"""
    xw = Win(values.reshape(n * h * w, cin), 2, 3, 0, right).on(DEV)
    ld = cin + right
    return xw.as_strided((n, h, w, cin), (h * w * ld, w * ld, ld, 1))


def run_dense(shape, cin, cout, epi, up=False):
    slope, alpha, beta = EPILOGUES[epi]
    k = dense_case(shape, cin, cout, up)
    n, h, w = shape
    m = k["m"]
    if shape == WALK_SHAPE:
        assert_tiles_exceed_cus(n, h << up, w << up)
    x = x_window(k["x"], n, h, w, cin)
    wk = Win(tap_major(k["wt"]), 1, 2).on(DEV)
    b = Win(k["bias"], left=8, right=8).on(DEV)
    r1 = Win(k["res1"], 3, 2, 4, 4).on(DEV) if alpha is not None else None      # ld_res1 = cout + 8
    r2 = Win(k["res2"], 1, 1, 8, 4).on(DEV) if beta is not None else None       # ld_res2 = cout + 12
    buf = sentinel_buffer(2 + m + 3, 96, H16)
    rows, cols = slice(2, 2 + m), slice(16, 16 + cout)
    dbuf = buf.to(DEV)
    ops.conv3x3_dense(x, cin, wk, b, slope=slope, res1=r1, alpha=alpha or 1.0, res2=r2, beta=beta or 1.0, up2x=up, out=dbuf[rows, cols])
    torch.cuda.synchronize()
    after = dbuf.cpu()
    what = f"conv3x3_dense {shape} {cin}->{cout} {epi}{' up2x' if up else ''}"
    assert changed_outside(buf, after, rows, cols) == 0, f"{what}: wrote outside its output window"
    e = R.excess(after[rows, cols], dense_ref(k, shape, up, slope, alpha, beta), H16, *R.CONV_TOL[H16])
    WORST[cin] = max(WORST.get(cin, 0.0), e)
    print(f"[esrgan] {what}: {e:.3f} x CONV_TOL (worst so far at cin {cin}: {WORST[cin]:.3f})")
    assert e <= 1.0, f"{what}: error {e:.3g}x CONV_TOL"


# the last two: the tile walk (see WALK_SHAPE) across the wrap from a tile's last channel chunk to chunk 0 of the workgroup's next tile, at both widths
DENSE_CASES = [(s, ci, co, e) for e in EPILOGUES for co in COUTS for ci in CINS for s in SHAPES] + [(WALK_SHAPE, 96, 32, "res1_res2"),
                                                                                                 (WALK_SHAPE, 192, 64, "res1_res2")]


@pytest.mark.parametrize("shape,cin,cout,epi", DENSE_CASES, ids=[case_id(*c) for c in DENSE_CASES])
def test_conv3x3_dense(shape, cin, cout, epi):
    run_dense(shape, cin, cout, epi)


@pytest.mark.parametrize("epi", ["bias", "slope"])
@pytest.mark.parametrize("shape", UP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv3x3_dense_up2x(shape, epi):
    run_dense(shape, 64, 64, epi, up=True)


@pytest.mark.parametrize("cin", CINS)
def test_conv3x3_dense_in_place_window(cin):
    """the dense block's form: x = columns [0, cin) of a 192-wide (224 for cin 192) sentinel buffer, out = columns [cin, cin + 32) of the SAME buffer,
    res1 = its columns [0, 32); the input columns and everything right of the window stay bit for bit"""
    shape = (2, 9, 33)
    n, h, w = shape
    k = dense_case(shape, cin, 32, False)
    m, width = k["m"], 224 if cin == 192 else 192
    buf = sentinel_buffer(2 + m + 3, width, H16)
    rows = slice(2, 2 + m)
    buf[rows, :cin] = k["x"].reshape(m, cin)
    dbuf = buf.to(DEV)
    x = dbuf[rows, :cin].as_strided((n, h, w, cin), (h * w * width, w * width, width, 1))
    ops.conv3x3_dense(x, cin, tap_major(k["wt"]).to(DEV), k["bias"].to(DEV), slope=F02, res1=dbuf[rows, :32], alpha=F02, out=dbuf[rows, cin:cin + 32])
    torch.cuda.synchronize()
    after = dbuf.cpu()
    assert changed_outside(buf, after, rows, slice(cin, cin + 32)) == 0, f"in-place cin {cin}: touched the input columns or something outside the window"
    e = R.excess(after[rows, cin:cin + 32], dense_ref(k, shape, False, F02, F02, None, res1=k["x"].reshape(m, cin)[:, :32]), H16, *R.CONV_TOL[H16])
    print(f"[esrgan] conv3x3_dense in place cin {cin}: {e:.3f} x CONV_TOL")
    assert e <= 1.0


def test_conv3x3_dense_refuses_other_shapes_and_overlapping_windows():
    from forge_amd._lib import FmxError
    x = torch.zeros(1, 4, 4, 192, dtype=H16, device=DEV)
    w48 = torch.zeros(32, 9 * 48, dtype=H16, device=DEV)
    with pytest.raises(FmxError, match="cin must be"):
        ops.conv3x3_dense(x, 48, w48)
    with pytest.raises(FmxError, match="cout must be"):
        ops.conv3x3_dense(x, 64, torch.zeros(16, 9 * 64, dtype=H16, device=DEV))
    with pytest.raises(FmxError, match="up2x"):
        ops.conv3x3_dense(x, 96, torch.zeros(32, 9 * 96, dtype=H16, device=DEV), up2x=True)
    w96 = torch.zeros(32, 9 * 96, dtype=H16, device=DEV)
    with pytest.raises(FmxError, match="disjoint from the input columns"):
        ops.conv3x3_dense(x, 96, w96, out=x.view(16, 192)[:, 64:96])
    with pytest.raises(FmxError, match="res2 requires res1"):
        ops.conv3x3_dense(x, 96, w96, res2=torch.zeros(16, 32, dtype=H16, device=DEV))


# ---- pack / unpack ----------------------------------------------------------------------------------------------------------------------------------
def test_esrgan_pack_image():
    v = torch.arange(256, dtype=torch.int32)
    img = torch.stack([v, (v + 85) % 256, (v * 7 + 170) % 256], dim=1).to(torch.uint8).view(1, 16, 16, 3)          # every level in every channel
    img = torch.cat([img, torch.randint(0, 256, (1, 16, 16, 3), generator=gen(11), dtype=torch.uint8)])
    buf = sentinel_buffer(512 + 3, 64, H16)
    dbuf = buf.to(DEV)
    ops.esrgan_pack_image(img.to(DEV), out=dbuf[:512].view(2, 16, 16, 64))
    torch.cuda.synchronize()
    after = dbuf.cpu()
    assert changed_outside(buf, after, slice(0, 512), slice(0, 64)) == 0
    # modules/upscaler_utils.py:14-19 (float64 / 255), then the cast to the model's type
    want = torch.from_numpy(np.ascontiguousarray(img.numpy()[..., ::-1]) / 255).to(H16).view(512, 3)
    assert torch.equal(after[:512, :3].view(torch.int16), want.view(torch.int16))
    assert bool((after[:512, 3:].view(torch.int16) == 0).all()), "channels 3..63 must be (+0) zeros"


def test_esrgan_unpack_image():
    allv = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(H16)
    allv = allv[torch.isfinite(allv)]                                            # every finite fp16 value: all ties of 255 v among them
    ties = allv[(allv.double() * 255 * 2 % 2 == 1) & (allv > 0) & (allv < 1)]
    assert ties.tolist() == [0.5]             # 255 is odd and fp16 values are dyadic: 127.5 (-> 128, the even neighbour) is the only tie inside (0, 1)
    vals = torch.cat([allv, ties])
    vals = torch.cat([vals, vals.new_zeros((-vals.numel()) % 3)]).view(-1, 3)
    npix = vals.shape[0]
    y = Win(vals, 1, 1, 0, 5).on(DEV)                                            # ld = 8
    buf = torch.full((npix + 2, 3), 0x5A, dtype=torch.uint8)
    dbuf = buf.to(DEV)
    ops.esrgan_unpack_image(y, out=dbuf[:npix])
    torch.cuda.synchronize()
    after = dbuf.cpu()
    assert bool((after[npix:] == 0x5A).all())
    # modules/upscaler_utils.py:31-34: clamp in fp32, 255.0 * arr (fp32), numpy round (half to even), uint8, BGR -> RGB
    arr = (255.0 * vals.float().clamp_(0, 1).numpy()).round().astype(np.uint8)[:, ::-1]
    assert np.array_equal(after[:npix].numpy(), arr)


# ---- executor ---------------------------------------------------------------------------------------------------------------------------------------
NB, IMG_W, IMG_H, TILE, OVERLAP = 2, 48, 40, 32, 8


def nchw(t):
    return t.permute(0, 3, 1, 2).double()


@lru_cache(maxsize=None)
def tiny_case():
    """the seeded nb = 2 network, the 48 x 40 image as its four 32 x 32 tiles, and the three restatements of the tiles' forward (computed once)"""
    import esrgan_refs as E
    from PIL import Image
    from forge_amd.modules import images
    sd = E.seeded_state_dict(NB, seed=0)
    img = E.test_image(IMG_W, IMG_H, seed=0)
    grid = images.split_grid(Image.fromarray(img.numpy(), "RGB"), TILE, TILE, OVERLAP)
    tiles = torch.from_numpy(np.stack([np.array(t) for _, _, row in grid.tiles for _, _, t in row]))
    assert tuple(tiles.shape) == (4, TILE, TILE, 3)
    x = E.to_bgr01(tiles)
    sd16 = {k: v.to(H16).float() for k, v in sd.items()}
    with torch.inference_mode():
        ref = E.forward(sd, NB, x)
        floor = E.metrics(E.forward(sd16, NB, x, compute=H16), ref)
    return dict(sd=sd, img=img, tiles=tiles, x=x, ref=ref, floor=floor)


@lru_cache(maxsize=None)
def native_tiny():
    """-> (model, uint8 output tiles, taps) of one tapped run of the four tiles"""
    from forge_amd.backend.nn.esrgan import RRDBNet
    import esrgan_refs as E
    k = tiny_case()
    net = RRDBNet(E.relayout(k["sd"], NB, "old"), device=DEV, name="tiny")
    assert net.nb == NB
    net.tap = {}
    out = net.upscale(k["tiles"])
    taps, net.tap = net.tap, None
    return net, out, taps


def test_executor_every_stored_tensor_teacher_forced():
    """every stored tensor against the fp64 restatement of ITS layer on the NATIVE inputs of that layer, at CONV_TOL (the packed image bit for bit)"""
    import esrgan_refs as E
    import torch.nn.functional as F
    k = tiny_case()
    _, _, taps = native_tiny()
    sd = k["sd"]
    worst = ["-", 0.0]

    def check(name, got, want):
        e = R.excess(nchw(got), want, H16, *R.CONV_TOL[H16])
        if e > worst[1]:
            worst[:] = [name, e]
        assert e <= 1.0, f"stored tensor {name}: {e:.3g}x CONV_TOL"

    want_pack = E.to_bgr01(k["tiles"]).to(H16)
    assert torch.equal(taps["pack"].permute(0, 3, 1, 2).view(torch.int16), want_pack.view(torch.int16))
    conv = lambda name, x: E.conv(sd, name, x, sites=True)              # fp64 arithmetic on the fp16-rounded weights
    check("conv_first", taps["conv_first"], conv("conv_first", nchw(taps["pack"])))
    for i in range(NB):
        for r in (1, 2, 3):
            blk = nchw(taps[f"{i}.{r}.in"])
            p = f"RRDB_trunk.{i}.RDB{r}.conv"
            for j in range(1, 5):
                cin = 64 + 32 * (j - 1)
                check(f"{i}.{r}.x{j}", taps[f"{i}.{r}.in"][..., cin:cin + 32], F.leaky_relu(conv(f"{p}{j}", blk[:, :cin]), F02))
            y = F02 * conv(f"{p}5", blk) + blk[:, :64]
            if r == 3:
                y = F02 * y + nchw(taps[f"{i}.in"])
            check(f"{i}.{r}", taps[f"{i}.{r}"], y)
    check("trunk", taps["trunk"], conv("trunk_conv", nchw(taps[f"{NB - 1}.3"])) + nchw(taps["conv_first"]))
    check("up1", taps["up1"], F.leaky_relu(conv("upconv1", E.up2(nchw(taps["trunk"]))), F02))
    check("up2", taps["up2"], F.leaky_relu(conv("upconv2", E.up2(nchw(taps["up1"]))), F02))
    check("hr", taps["hr"], F.leaky_relu(conv("HRconv", nchw(taps["up2"])), F02))
    check("last", taps["last"], conv("conv_last", nchw(taps["hr"])))
    print(f"[esrgan] teacher-forced: worst stored tensor {worst[0]} at {worst[1]:.3f} x CONV_TOL")


def test_executor_output_against_fp64_within_the_fp16_floor():
    """conv_last's output against the fp64 restatement, by the project's floor rule: the floor is the torch-fp16 CPU run of the same restatement
    against fp64, computed here; rms <= 1.25 x floor, max <= max(1e-3, 1.5 x floor)"""
    import esrgan_refs as E
    k = tiny_case()
    _, _, taps = native_tiny()
    m, lim = E.metrics(nchw(taps["last"]), k["ref"]), E.gate(k["floor"])
    print(f"[esrgan] end to end: rms {m['rms']:.3e} = {m['rms'] / k['floor']['rms']:.3f} x floor (gate {lim['rms']:.3e}); "
          f"max_rel {m['max_rel']:.3e} = {m['max_rel'] / k['floor']['max_rel']:.3f} x floor (gate {lim['max_rel']:.3e})")
    assert m["rms"] <= lim["rms"] and m["max_rel"] <= lim["max_rel"]


def test_executor_image_within_one_level_and_groups_do_not_matter():
    import esrgan_refs as E
    from forge_amd.backend.nn.esrgan import RRDBNet
    k = tiny_case()
    net, out, _ = native_tiny()
    assert out.dtype == torch.uint8 and tuple(out.shape) == (4, 4 * TILE, 4 * TILE, 3)
    worst = int((out.int() - E.to_image(k["ref"]).int()).abs().max())
    print(f"[esrgan] image: worst level difference to the fp64 restatement {worst}")
    assert worst <= 1
    assert torch.equal(net.upscale(k["tiles"]), out)                                         # untapped, recycled arena: the same bits
    small = RRDBNet(k["sd"], device=DEV, name="tiny", group_bytes=1)                         # a byte budget below one tile: groups of one
    assert small.tiles_per_group(TILE, TILE) == 1 and torch.equal(small.upscale(k["tiles"]), out)


def test_executor_raises_on_a_non_finite_output():
    from forge_amd.backend.nn.esrgan import RRDBNet
    k = tiny_case()
    sd = dict(k["sd"])
    sd["HRconv.bias"] = torch.full((64,), 60000.0)
    sd["conv_last.weight"] = torch.full((3, 64, 3, 3), 4.0)
    with pytest.raises(RuntimeError, match="ESRGAN model 'blown'.*non-finite"):
        RRDBNet(sd, device=DEV, name="blown").upscale(k["tiles"][:1])


def test_untiled_and_tiled_routes_agree_away_from_seams():
    """tile_size = 0 sends the 48 x 40 image as ONE tile (an h x w that is no tile size): its image is within 1 level of the fp64 restatement of the
    whole image.  Tiled (32 / 8), the part of the result that comes from tile (0, 0) alone and lies 16 / 24 pixels from that tile's inner edges
    (x < 16, y < 8 of the source) differs from the untiled one by what the tile's zero border does to the fp64 restatement there, plus the two
    1-level bounds."""
    import esrgan_refs as E
    from PIL import Image
    from forge_amd.modules import upscaler_utils
    k = tiny_case()
    net, out, _ = native_tiny()
    pil = Image.fromarray(k["img"].numpy(), "RGB")
    whole = torch.from_numpy(np.array(upscaler_utils.upscale_with_model(net, pil, tile_size=0)))
    tiled = torch.from_numpy(np.array(upscaler_utils.upscale_with_model(net, pil, tile_size=TILE, tile_overlap=OVERLAP)))
    assert tuple(whole.shape) == tuple(tiled.shape) == (4 * IMG_H, 4 * IMG_W, 3)
    with torch.inference_mode():
        ref_whole = E.to_image(E.forward(k["sd"], NB, E.to_bgr01(k["img"][None])))[0]
    assert int((whole.int() - ref_whole.int()).abs().max()) <= 1
    reg = (slice(0, 4 * 8), slice(0, 4 * 16))
    assert torch.equal(tiled[reg], out[0][reg])                                              # that part is tile (0, 0)'s own pixels
    border = (ref_whole[reg].int() - E.to_image(k["ref"][:1])[0][reg].int()).abs()
    diff = (whole[reg].int() - tiled[reg].int()).abs()
    print(f"[esrgan] untiled vs tiled away from seams: worst {int(diff.max())} levels (the fp64 restatement's own: {int(border.max())})")
    assert bool((diff <= border + 2).all())


# ---- call surface -----------------------------------------------------------------------------------------------------------------------------------
def test_hires_fix_with_an_esrgan_upscaler(tmp_path, monkeypatch):
    """txt2img with enable_hr and a registered ESRGAN model: runs, lands on the target latent shape, and equals the same steps composed by hand
    (decode -> truncate to uint8 -> resize_image -> encode -> sample_img2img with the same seeds) bit for bit"""
    import esrgan_refs as E
    from PIL import Image
    from forge_amd import synth
    from forge_amd.backend.diffusion_engine.base import build_engine
    from forge_amd.modules import esrgan_model, images, processing, rng, sd_samplers, sd_samplers_common, shared
    cfg = synth.TINY_SD15_UNET_CONFIG
    vcfg = dict(synth.TINY_VAE_CONFIG, block_out_channels=(64, 64, 128, 128))                # four levels: latent = size / 8, as the call surface assumes
    eng = build_engine(cfg, synth.synth_unet_state_dict(cfg, seed=0), vcfg, synth.synth_vae_state_dict(vcfg, seed=1), device=DEV)
    (tmp_path / "ESRGAN").mkdir()
    torch.save(E.relayout(E.seeded_state_dict(NB, seed=0), NB, "real"), tmp_path / "ESRGAN" / "4x-Tiny.pth")
    monkeypatch.setattr(shared, "models_path", str(tmp_path))
    monkeypatch.setattr(shared, "sd_model", eng)
    monkeypatch.setattr(shared, "device", None)
    monkeypatch.setattr(shared, "state", shared.State())
    monkeypatch.setattr(shared, "sd_upscalers", [])
    monkeypatch.setattr(shared.opts, "ESRGAN_tile", TILE)
    monkeypatch.setattr(shared.opts, "randn_source", "CPU")
    assert [s.name for s in esrgan_model.register()][-1] == "4x-Tiny"
    c, uc = synth.synth_conditioning(2, cfg["context_dim"], None, seed=1234)
    c, uc = c.to(DEV), uc.to(DEV)
    kw = dict(sd_model=eng, c=c, uc=uc, seed=3, sampler_name="Euler", batch_size=2, steps=4, cfg_scale=7.0, width=128, height=96, do_decode=False)
    hr = dict(enable_hr=True, hr_scale=2, hr_upscaler="4x-Tiny", hr_second_pass_steps=3, denoising_strength=0.6, hr_cfg=5.0)

    torch.manual_seed(7)
    res = processing.process_images(processing.StableDiffusionProcessingTxt2Img(**kw, **hr))
    assert tuple(res.latents.shape) == (2, 4, 24, 32) and bool(torch.isfinite(res.latents).all())

    with torch.inference_mode():          # as process_images_inner runs
        torch.manual_seed(7)
        first = processing.process_images(processing.StableDiffusionProcessingTxt2Img(**kw)).latents
        dec = processing.decode_first_stage(eng, first)
        assert tuple(dec.shape) == (2, 3, 96, 128)
        low = torch.clamp((dec.float() + 1.0) / 2.0, min=0.0, max=1.0)
        ups = []
        for xs in low:
            im = Image.fromarray((255. * np.moveaxis(xs.cpu().numpy(), 0, 2)).astype(np.uint8))
            im = images.resize_image(0, im, 256, 192, upscaler_name="4x-Tiny")
            assert im.size == (256, 192)
            ups.append(np.moveaxis(np.array(im).astype(np.float32) / 255.0, 2, 0))
        decoded = torch.from_numpy(np.array(ups)).to(DEV)
        samples = sd_samplers_common.images_tensor_to_samples(decoded, None, eng)
        p = processing.StableDiffusionProcessingTxt2Img(**kw, **hr)
        p.init_hr()
        p.is_hr_pass, p.seeds, p.all_seeds, p.subseeds, p.iteration = True, [3, 4], [3, 4], [0, 1], 0
        p.sampler = sd_samplers.create_sampler("Euler", eng)
        p.rng = rng.ImageRNG(tuple(samples.shape[1:]), p.seeds, subseeds=p.subseeds, subseed_strength=0.0, device=samples.device)
        noise = p.rng.next()
        eng.forge_objects = eng.forge_objects_after_applying_lora.shallow_copy()
        want = p.sampler.sample_img2img(p, samples.contiguous(), noise, c, uc, steps=3, image_conditioning=samples.new_zeros(2, 5, 1, 1))
    assert torch.equal(res.latents, want)
    # the ESRGAN pass is what separates this from LANCZOS alone
    lanczos = images.resize_image(0, Image.fromarray((255. * np.moveaxis(low[0].cpu().numpy(), 0, 2)).astype(np.uint8)), 256, 192)
    assert not np.array_equal(np.array(lanczos), (ups[0].transpose(1, 2, 0) * 255).round().astype(np.uint8))
