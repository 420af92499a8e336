"""CPU: the host side of the native TAESD decoder and of live previews -- the fp64 restatement (tests/taesd_refs.py) pinned to the REAL reference's
output (tests/golden/taesd.pt, made by tools/make_taesd_fixtures.py), state-dict layout detection, weight-file choice and lookup, the uint8 image
tail, the preview period rule, the argument contract of fmx_conv3x3_c64, and the teeth of the network-level bar tests/test_gpu_taesd.py applies."""
import ctypes as C
import socket
import types

import pytest
import torch

import forge_amd  # noqa: F401
from forge_amd import _lib
from forge_amd.backend.nn import taesd as native
from forge_amd.modules import sd_samplers_common, sd_vae_approx, sd_vae_taesd, shared

import taesd_refs as T

FX = T.load_fixture()
CASES = {"l4": 4, "l16": 16}


@pytest.mark.parametrize("case", list(CASES))
def test_restatement_reproduces_the_reference(case):
    """The recorded output is the reference's fp32 run, which carries its own fp32 rounding through 35 layers: the restatement's table of layers,
    run in fp32 as the reference runs, reproduces it to 1e-6 of its maximum; the fp64 run of the same table (the teacher of every other test) is
    within the fp32 run's accumulated rounding of it: 35 layers x 2^-24 relative, against the largest activation of the depth (|max| <= 34 by the
    fixture tool's own check, times the last layer's gain below 1) -- 35 * 6e-8 * 34 = 7e-5 absolute, far below one fp16 ulp of the output."""
    c = FX["cases"][case]
    sd = T.state_dict_for(FX, CASES[case])
    got32 = T.decode_ref(sd, c["latent"], compute=torch.float32)
    d32 = float((got32.double() - c["out"].double()).abs().max())
    got = T.decode_ref(sd, c["latent"])
    d64 = float((got - c["out"].double()).abs().max())
    print(f"[taesd] restatement vs reference {case}: fp32 run {d32:.3e}, fp64 run {d64:.3e}, max |ref| {float(c['out'].abs().max()):.3f}")
    assert got32.dtype == torch.float32 and got.dtype == torch.float64
    assert d32 <= 1e-6 * float(c["out"].abs().max())
    assert d64 <= 35 * 2.0 ** -24 * 34


def test_fixture_is_what_the_tool_promises():
    sd = FX["state_dict"]
    assert len(sd) == 67 and sorted(sd) == sorted(native.expected_keys())
    assert all(v.dtype == torch.float16 for v in sd.values())
    for c in FX["cases"].values():
        inside = ((c["out"] > 0.02) & (c["out"] < 0.98)).float().mean()
        assert inside >= 0.9 and float(c["latent"].abs().max()) > 9        # unsaturated image, exercised clamp


def test_layout_detection_and_refusal():
    assert native.detect_latent_channels(T.state_dict_for(FX, 4)) == 4
    assert native.detect_latent_channels(T.state_dict_for(FX, 16)) == 16
    sd = T.state_dict_for(FX, 4)
    del sd["9.conv.2.bias"]
    with pytest.raises(ValueError, match=r"'9\.conv\.2\.bias' is missing"):
        native.detect_latent_channels(sd)
    enc = {"0.weight": torch.zeros(64, 3, 3, 3)}                            # an encoder file
    with pytest.raises(ValueError, match=r"'1\.weight' is missing"):
        native.detect_latent_channels(enc)
    bad = T.state_dict_for(FX, 4)
    bad["12.weight"] = torch.zeros(64, 32, 3, 3)
    with pytest.raises(ValueError, match=r"'12\.weight' is \(64, 32, 3, 3\)"):
        native.detect_latent_channels(bad)
    with pytest.raises(ValueError, match="latent_channels=16"):
        native.TAESDDecoder(T.state_dict_for(FX, 4), latent_channels=16, device="cpu")


@pytest.mark.parametrize("attrs,name", [
    (dict(is_sdxl=False), "taesd_decoder.pth"),
    (dict(is_sdxl=True), "taesdxl_decoder.pth"),
    (dict(is_sdxl=False, is_flux=True), "taef1_decoder.pth"),
    (dict(is_sd3=True, is_sdxl=False), "taesd3_decoder.pth"),
    (dict(is_sdxl=True, is_webui_legacy_model=lambda: False), "taef1_decoder.pth"),
])
def test_weight_file_per_family(attrs, name):
    assert sd_vae_taesd.decoder_model_name(types.SimpleNamespace(**attrs)) == name


def test_missing_weights_raise_and_nothing_is_downloaded(tmp_path, monkeypatch):
    def no_network(*a, **k):
        raise AssertionError("TAESD lookup opened a network connection")
    monkeypatch.setattr(socket.socket, "connect", no_network)
    monkeypatch.setattr(torch.hub, "download_url_to_file", no_network)
    monkeypatch.setattr(shared, "models_path", str(tmp_path))
    monkeypatch.setattr(shared, "sd_model", types.SimpleNamespace(is_sdxl=True, device="cpu"))
    monkeypatch.setattr(sd_vae_taesd, "sd_vae_taesd_models", {})
    with pytest.raises(FileNotFoundError, match="taesdxl_decoder.pth") as e:
        sd_vae_taesd.decoder_model()
    assert str(tmp_path) in str(e.value)
    with pytest.raises(NotImplementedError, match="encoder"):
        sd_vae_taesd.encoder_model()
    monkeypatch.setattr(shared.opts, "sd_vae_encode_method", "TAESD")
    with pytest.raises(NotImplementedError, match="TAESD encoder"):
        sd_samplers_common.images_tensor_to_samples(torch.zeros(1, 3, 8, 8))


def test_weights_file_is_found_and_cached(tmp_path, monkeypatch):
    made = []

    class Fake:
        def __init__(self, sd, device=None, dtype=None):
            made.append((sorted(sd)[0], device, dtype))
    monkeypatch.setattr(native, "TAESDDecoder", Fake)
    (tmp_path / "VAE-taesd").mkdir()
    torch.save(T.state_dict_for(FX, 4), tmp_path / "VAE-taesd" / "taesd_decoder.pth")
    monkeypatch.setattr(shared, "models_path", str(tmp_path))
    monkeypatch.setattr(shared, "sd_model", types.SimpleNamespace(is_sdxl=False, device="cpu"))
    monkeypatch.setattr(sd_vae_taesd, "sd_vae_taesd_models", {})
    a, b = sd_vae_taesd.decoder_model(), sd_vae_taesd.decoder_model()
    assert a is b and made == [("1.bias", "cpu", torch.float16)]


@pytest.mark.parametrize("case", list(CASES))
def test_uint8_tail_is_exact(case, monkeypatch):
    c = FX["cases"][case]
    assert torch.equal(T.image_tail(c["out"][0]), c["image_u8"])
    # and through the module's own five lines: the decoder replaced by the recorded float output
    dec = types.SimpleNamespace(decode=lambda z: c["out"][:1].clone())
    monkeypatch.setattr(sd_vae_taesd, "decoder_model", lambda: dec)
    img = sd_samplers_common.single_sample_to_image(c["latent"][0], approximation=3)
    assert img.size == (c["out"].shape[3], c["out"].shape[2])
    import numpy as np
    assert np.array_equal(np.asarray(img), c["image_u8"].numpy())


def test_cheap_approximation_needs_factors(monkeypatch):
    monkeypatch.setattr(shared, "sd_model", types.SimpleNamespace(is_sdxl=True))
    with pytest.raises(NotImplementedError, match="latent_rgb_factors"):
        sd_vae_approx.cheap_approximation(torch.zeros(1, 4, 2, 2))
    assert sd_vae_approx.model() is None
    fmt = types.SimpleNamespace(latent_format=types.SimpleNamespace(latent_rgb_factors=[[1, 2, 3]]))
    assert sd_vae_approx.latent_rgb_factors(types.SimpleNamespace(model_config=fmt)) == [[1, 2, 3]]


class Untouchable:
    """a stand-in latent: any use of it (a launch, a copy, a synchronisation) raises"""

    def __getattr__(self, name):
        raise AssertionError(f"the latent was touched ({name}) with previews off")


def test_period_rule_over_25_steps(monkeypatch):
    calls = []
    monkeypatch.setattr(sd_samplers_common, "sample_to_image", lambda latent, *a, **k: calls.append(shared.state.sampling_step) or f"img{len(calls)}")
    st = shared.State()
    monkeypatch.setattr(shared, "state", st)
    for k, v in dict(live_previews_enable=True, show_progress_every_n_steps=10, show_progress_type="TAESD").items():
        monkeypatch.setattr(shared.opts, k, v)

    def run(latent="lat"):
        calls.clear()
        for step in range(25):
            st.sampling_step = step
            sd_samplers_common.store_latent(latent)
        return list(calls)

    assert run() == [0, 10, 20] and st.current_image == "img3" and st.id_live_preview == 3 and st.current_latent == "lat"
    monkeypatch.setattr(shared.opts, "show_progress_every_n_steps", 4)
    assert run() == [0, 4, 8, 12, 16, 20, 24]
    for off in (dict(show_progress_every_n_steps=0), dict(show_progress_every_n_steps=-1), dict(live_previews_enable=False)):
        with monkeypatch.context() as m:
            for k, v in off.items():
                m.setattr(shared.opts, k, v)
            before = st.id_live_preview
            assert run(Untouchable()) == [] and st.id_live_preview == before      # previews off: nothing called, the latent not even looked at
    # a polling caller (shared_state.py:145-152): the difference rule, and only when parallel processing is allowed
    monkeypatch.setattr(shared.opts, "show_progress_every_n_steps", 10)
    monkeypatch.setattr(shared, "parallel_processing_allowed", True)
    st2 = shared.State()
    monkeypatch.setattr(shared, "state", st2)
    calls.clear()
    for step in range(25):
        st2.sampling_step = step
        sd_samplers_common.store_latent("lat")          # stores, never decodes: the poller does
        st2.set_current_image()
    assert calls == [10, 20] and st2.current_image_sampling_step == 20 and st2.id_live_preview == 2
    monkeypatch.setattr(shared, "parallel_processing_allowed", False)
    st2.sampling_step = 40
    st2.set_current_image()
    assert calls == [10, 20]


def test_new_options_default_to_the_present_behaviour():
    o = shared.opts
    assert (o.live_previews_enable, o.show_progress_every_n_steps, o.show_progress_type, o.sd_vae_encode_method, o.sd_vae_decode_method) == \
        (False, 10, "Approx NN", "Full", "Full")
    assert sd_samplers_common.approximation_indexes == {"Full": 0, "Approx NN": 1, "Approx cheap": 2, "TAESD": 3}
    model = types.SimpleNamespace(decode_first_stage=lambda x: ("full", x))
    from forge_amd.modules import processing
    assert processing.decode_first_stage(model, "z") == ("full", "z")


BADARG = 10001
FAKE = 0x7F0000001000


@pytest.mark.parametrize("sfx", ["_f16", "_bf16"])
def test_conv3x3_c64_contract(sfx):
    try:
        lib = _lib.lib()
    except _lib.FmxError as e:
        pytest.skip(f"libfmx not built: {e}")
    fn = getattr(lib, "fmx_conv3x3_c64" + sfx)
    p = C.c_void_p(FAKE)

    def call(cin=64, cout=64, x=p, ld_out=64, res=None, ld_res=0, relu=1, up=0):
        return fn(x, 1, 8, 8, cin, p, p, cout, res, ld_res, relu, up, p, ld_out, None)
    for cin, cout in ((32, 64), (128, 64), (64, 32), (64, 128)):
        assert call(cin=cin, cout=cout) == BADARG and "64 input and 64 output channels" in lib.fmx_last_error().decode()
    assert call(x=C.c_void_p(FAKE + 8)) == BADARG and "alignment" in lib.fmx_last_error().decode()
    assert call(ld_out=66) == BADARG and call(res=p, ld_res=32) == BADARG and "leading dimensions" in lib.fmx_last_error().decode()
    assert call(up=2) == BADARG and call(relu=3) == BADARG
    assert lib.fmx_taesd_pack_latent(p, 1, 65, 4, 4, p, None) == BADARG and lib.fmx_taesd_pack_latent_bf16(p, 1, 0, 4, 4, p, None) == BADARG
    assert lib.fmx_latent_rgb(p, (C.c_float * 3)(), 1, 65, 16, p, None) == BADARG


# ---- teeth: the network-level bar of tests/test_gpu_taesd.py, applied to the ROUNDED restatement, passes it and rejects three planted bugs -------
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("case", list(CASES))
def test_network_bar_has_teeth(case, dt):
    dtype = {"fp16": torch.float16, "bf16": torch.bfloat16}[dt]
    c = FX["cases"][case]
    sd = T.state_dict_for(FX, CASES[case])
    m, lim, bad = T.network_bar(T.decode_ref(sd, c["latent"], dtype), c["out"], c[dt])
    assert not bad, f"the rounded restatement itself misses the bar: {m} vs {lim}"
    for plant in T.PLANTS:
        m, lim, bad = T.network_bar(T.decode_ref(sd, c["latent"], dtype, plant=plant), c["out"], c[dt])
        assert bad, f"plant {plant} slips under the bar ({case}, {dt}): {m} vs {lim}"
