"""CPU: the host side of the native ESRGAN upscalers -- key-layout canonicalisation and refusals (forge_amd/backend/nn/esrgan.py), the tiling and
the upscaler loop against the reference's own results (tests/golden/esrgan_grid.pt, tools/make_esrgan_fixtures.py), the teeth of the restatements
in tests/esrgan_refs.py that tests/test_gpu_esrgan.py gates the executor with, and init_hr's upscaler lookup."""
from functools import lru_cache

import numpy as np
import pytest
import torch
from PIL import Image

import forge_amd  # noqa: F401
from forge_amd.backend.nn import esrgan
from forge_amd.modules import images, processing, shared, upscaler

import esrgan_refs as E
from taesd_refs import GOLDEN

NB, W, H = 2, 48, 40          # the tiny network and image of the end-to-end GPU test


# ---- loader -----------------------------------------------------------------------------------------------------------------------------------------
def test_three_key_layouts_canonicalise_to_the_same_tensors():
    sd = E.seeded_state_dict(NB, seed=3)
    for layout in ("new", "old", "real"):
        src = sd if layout == "new" else E.relayout(sd, NB, layout)
        if layout != "new":
            assert not set(src) & set(sd)
        got, nb = esrgan.canonicalize(src)
        assert nb == NB and set(got) == set(sd), layout
        assert all(torch.equal(got[k], sd[k]) for k in sd), layout
    inner = E.relayout(sd, NB, "real")["params_ema"]
    assert esrgan.canonicalize({"params": inner})[1] == NB and esrgan.canonicalize(inner)[1] == NB      # the wrapper is optional


def _with(sd, **kw):
    out = dict(sd)
    out.update(kw)
    return out


@pytest.mark.parametrize("case,match", [
    ("real_x2", "Real-ESRGAN x2"), ("real_x1", "Real-ESRGAN x1"), ("plus", "conv1x1"), ("nf", "nf 32, gc 32"), ("gc", "nf 64, gc 16"),
    ("swinir", "SwinIR"), ("scunet", "ScuNET"), ("old_x2", "two x2 stages"), ("unknown", "not an RRDBNet"), ("one_stage", "upconv2"),
])
def test_refusals_name_their_reason(case, match):
    sd = E.seeded_state_dict(1, seed=4)
    z = torch.zeros
    if case in ("real_x2", "real_x1"):
        src = {"params_ema": _with(E.relayout(sd, 1, "real")["params_ema"], **{"conv_first.weight": z(64, 12 if case == "real_x2" else 48, 3, 3)})}
    elif case == "plus":
        src = _with(sd, **{"RRDB_trunk.0.RDB1.conv1x1.weight": z(32, 64, 1, 1)})
    elif case == "nf":
        src = _with(sd, **{"conv_first.weight": z(32, 3, 3, 3)})
    elif case == "gc":
        src = _with(sd, **{"RRDB_trunk.0.RDB1.conv1.weight": z(16, 64, 3, 3)})
    elif case == "swinir":
        src = {"conv_first.weight": z(180, 3, 3, 3), "layers.0.residual_group.blocks.0.attn.relative_position_bias_table": z(225, 6)}
    elif case == "scunet":
        src = {"m_head.0.weight": z(64, 3, 3, 3), "m_down1.0.trans_block.ln1.weight": z(64)}
    elif case == "old_x2":
        src = {k: v for k, v in E.relayout(sd, 1, "old").items() if not k.startswith(("model.8.", "model.10."))}
    elif case == "one_stage":
        src = {k: v for k, v in sd.items() if not k.startswith("upconv2.")}
    else:
        src = {"encoder.weight": z(4, 4)}
    with pytest.raises(NotImplementedError, match=match):
        esrgan.canonicalize(src)


# ---- tiling and the upscaler loop against the reference's results -----------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def grid_fixture():
    return torch.load(f"{GOLDEN}/esrgan_grid.pt", weights_only=True)


@pytest.mark.parametrize("case", [(48, 40, 32, 8), (33, 33, 32, 8), (24, 24, 32, 8), (64, 32, 32, 8)], ids=lambda c: "x".join(map(str, c)))
def test_split_and_combine_grid_match_the_reference(case):
    w, h, tile, overlap = case
    fx = grid_fixture()["grid"][case]
    assert torch.equal(fx["image"], E.test_image(w, h, seed=w + h))
    grid = images.split_grid(Image.fromarray(fx["image"].numpy(), "RGB"), tile, tile, overlap)
    assert [[y, th, [[x, tw] for x, tw, _ in row]] for y, th, row in grid.tiles] == fx["rows"]
    assert (grid.tile_w, grid.tile_h, grid.image_w, grid.image_h, grid.overlap, grid.tile_count) == (tile, tile, w, h, overlap, fx["tiles"].shape[0])
    tiles = np.stack([np.array(t) for _, _, row in grid.tiles for _, _, t in row])
    assert np.array_equal(tiles, fx["tiles"].numpy())
    k = 0
    for _, _, row in grid.tiles:
        for cell in row:
            cell[2] = Image.fromarray(np.minimum(np.array(cell[2]).astype(np.int32) + 16 * k, 255).astype(np.uint8), "RGB")
            k += 1
    assert np.array_equal(np.array(images.combine_grid(grid)), fx["combined"].numpy())


def test_grid_cases_cover_what_they_are_for():
    g = grid_fixture()["grid"]
    shape = lambda c: (len(g[c]["rows"]), len(g[c]["rows"][0][2]))
    assert shape((48, 40, 32, 8)) == (2, 2) and shape((64, 32, 32, 8)) == (1, 3) and shape((24, 24, 32, 8)) == (1, 1)
    assert g[(33, 33, 32, 8)]["rows"][1][0] == 1 and g[(33, 33, 32, 8)]["rows"][0][2][1][0] == 1        # the last-tile clamp: origin 33 - 32
    small = g[(24, 24, 32, 8)]           # an image smaller than the tile: the clamp puts the origin at 24 - 32 = -8, PIL pads the crop with black
    assert small["rows"] == [[-8, 32, [[-8, 32]]]]
    assert bool((small["tiles"][0, :8] == 0).all()) and bool((small["tiles"][0, :, :8] == 0).all()) and torch.equal(small["tiles"][0, 8:, 8:], small["image"])


@pytest.mark.parametrize("scale", [1, 1.5, 2, 4, 5])
def test_upscaler_loop_pass_count_and_size(scale):
    class Fake(upscaler.Upscaler):
        calls = 0

        def do_upscale(self, img, selected_model=None):
            self.calls += 1
            return img.resize((img.width * 4, img.height * 4), resample=upscaler.NEAREST)

    up = Fake()
    res = up.upscale(Image.fromarray(E.test_image(40, 24, seed=1).numpy(), "RGB"), scale)
    assert (up.calls, tuple(res.size)) == tuple(grid_fixture()["upscale"][scale])


def test_resize_image_modes_and_the_upscaler_lookup(monkeypatch):
    class Times4(upscaler.Upscaler):
        def do_upscale(self, img, selected_model=None):
            return img.resize((img.width * 4, img.height * 4), resample=upscaler.NEAREST)

    up = Times4()
    monkeypatch.setattr(shared, "sd_upscalers", [upscaler.UpscalerNone().scalers[0], upscaler.UpscalerData("x4", None, up)])
    im = Image.fromarray(E.test_image(40, 24, seed=2).numpy(), "RGB")
    got = images.resize_image(0, im, 80, 48, upscaler_name="x4")
    want = im.resize((160, 96), resample=upscaler.NEAREST).resize((80, 48), resample=upscaler.LANCZOS)
    assert np.array_equal(np.array(got), np.array(want))
    assert np.array_equal(np.array(images.resize_image(0, im, 80, 48)), np.array(im.resize((80, 48), resample=upscaler.LANCZOS)))      # no name: LANCZOS
    assert images.resize_image(1, im, 64, 64, upscaler_name="x4").size == (64, 64) and images.resize_image(2, im, 64, 64, upscaler_name="x4").size == (64, 64)
    fill = np.array(images.resize_image(1, im, 64, 64))
    assert np.array_equal(fill, np.array(im.resize((106, 64), resample=upscaler.LANCZOS))[:, 21:85])     # mode 1: 40 * 64 // 24 = 106 wide, centred, cropped


# ---- teeth of the restatements ----------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def tiny():
    sd = E.seeded_state_dict(NB, seed=0)
    img = E.test_image(W, H, seed=0)[None]
    x = E.to_bgr01(img)
    sd16 = {k: v.to(torch.float16).float() for k, v in sd.items()}       # the numbers every 16-bit run holds; fp64 runs on the unrounded ones
    with torch.inference_mode():
        ref = E.forward(sd, NB, x)
        fp16 = E.forward(sd16, NB, x, compute=torch.float16)
        sites = E.forward(sd, NB, x, sites=True)
    return dict(sd=sd, img=img, x=x, ref=ref, fp16=fp16, sites=sites, floor=E.metrics(fp16, ref))


def test_sites_restatement_stays_within_the_end_to_end_gate():
    t = tiny()
    m, lim = E.metrics(t["sites"], t["ref"]), E.gate(t["floor"])
    print(f"[esrgan] fp16 floor {t['floor']}; sites restatement {m}; gate {lim}; output range [{float(t['ref'].min()):.3f}, {float(t['ref'].max()):.3f}]")
    assert m["rms"] <= lim["rms"] and m["max_rel"] <= lim["max_rel"]


@pytest.mark.parametrize("plant", E.PLANTS)
def test_planted_errors_exceed_the_gate(plant):
    t = tiny()
    with torch.inference_mode():
        bad = E.forward(t["sd"], NB, E.to_bgr01(t["img"], rgb=True) if plant == "rgb" else t["x"], sites=True, plant=plant)
    m, lim = E.metrics(bad, t["ref"]), E.gate(t["floor"])
    print(f"[esrgan] plant {plant}: rms {m['rms'] / lim['rms']:.1f} x the gate, max {m['max_rel'] / lim['max_rel']:.1f} x the gate")
    assert m["rms"] > lim["rms"] and m["max_rel"] > lim["max_rel"]


def test_fp16_image_is_within_one_level_of_the_fp64_one():
    """the condition that lets the GPU test assert the same of the native image"""
    t = tiny()
    a, b = E.to_image(t["fp16"]).int(), E.to_image(t["ref"]).int()
    assert int((a - b).abs().max()) <= 1
    assert 32 < int(b.max()) - int(b.min()), "the image must use a range of levels for this to mean anything"


# ---- call surface -------------------------------------------------------------------------------------------------------------------------------------------
def test_init_hr_looks_the_upscaler_up(monkeypatch):
    monkeypatch.setattr(shared, "sd_upscalers", [upscaler.UpscalerData("tiny-esrgan", "/nowhere/tiny-esrgan.pth", None)])
    p = processing.StableDiffusionProcessingTxt2Img(enable_hr=True, hr_upscaler="tiny-esrgan", width=64, height=64, hr_scale=2)
    p.init_hr()
    assert p.latent_scale_mode is None and (p.hr_upscale_to_x, p.hr_upscale_to_y) == (128, 128)
    p = processing.StableDiffusionProcessingTxt2Img(enable_hr=True, hr_upscaler="Latent (bicubic)", width=64, height=64)
    p.init_hr()
    assert p.latent_scale_mode is not None
    p = processing.StableDiffusionProcessingTxt2Img(enable_hr=True, hr_upscaler="R-ESRGAN 4x+", width=64, height=64)
    with pytest.raises(Exception, match="could not find upscaler named R-ESRGAN 4x\\+"):
        p.init_hr()


def test_esrgan_scalers_come_from_files_only(tmp_path, monkeypatch):
    from forge_amd.modules import esrgan_model
    monkeypatch.setattr(shared, "models_path", str(tmp_path / "models"))
    monkeypatch.setattr(shared, "sd_upscalers", [])
    assert esrgan_model.UpscalerESRGAN(str(tmp_path)).scalers == []                       # no file, no scaler (and no URL)
    torch.save(E.seeded_state_dict(1, seed=1), tmp_path / "4x-Tiny.pth")
    (tmp_path / "notes.txt").write_text("x")
    names = [s.name for s in esrgan_model.register(str(tmp_path))]
    assert names == ["None", "Lanczos", "Nearest", "4x-Tiny"]
    data = shared.sd_upscalers[-1]
    assert data.data_path.endswith("4x-Tiny.pth") and data.scale == 4 and isinstance(data.scaler, esrgan_model.UpscalerESRGAN)
