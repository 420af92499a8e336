"""GPU: native IP-Adapter.  fmxi_attention_dual_f16 (hipops.attention_dual) against the fp64 restatement of tests/ipadapter_refs.py within
2 ulp(O) + 2 EPS (1 + sum |w|): every text length, query count, segment layout and weight of ipadapter_refs; O as a column window of a
sentinel-filled buffer, Q / K surrounded by 30000, finite -3 in the V^T pads, NaN in the extra K rows outside the segments; three launches give
the same bits; every refused call returns before touching O."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import forge_amd  # noqa: E402,F401
from forge_amd import _lib  # noqa: E402
from forge_amd import hipops as ops  # noqa: E402

import ipadapter_refs as I  # noqa: E402
import kernel_refs as R  # noqa: E402
from test_gpu_gemm_windows import bits  # noqa: E402

DEV = "cuda"
H16 = torch.float16
CANARY = 215.5
GUARD = 1024                 # elements in front of and behind O
SCALE = I.D ** -0.5
O_EXTRA, O_COL0 = 36, 8      # O is columns [8, 8 + H * 64) of rows of H * 64 + 36 elements: every other row starts on an 8-byte boundary only
O_ROWS_EXTRA = 3             # rows between the images of O that the launch must leave alone
QK_EXTRA = 64                # columns beside Q and K, rows behind them


class Buffers:
    """the case on the device in the executors' layouts, with what the ABI allows around the operands"""

    def __init__(self, c):
        b, nq, h, d = c["q"].shape
        nk = c["nk"]
        self.b, self.nq, self.h, self.nk, self.nk_pad = b, nq, h, nk, (nk + 63) // 64 * 64
        hd = h * d
        self.q = torch.full((b, nq + 5, hd + QK_EXTRA), I.SURROUND, dtype=H16)
        self.q[:, :nq, :hd] = c["q"].reshape(b, nq, hd)
        self.k = torch.full((b, self.nk_pad, hd + QK_EXTRA), I.SURROUND, dtype=H16)
        self.k[:, :nk, :hd] = c["k"].reshape(b, nk, hd)
        self.vt = torch.full((hd, b, self.nk_pad), I.VT_PAD, dtype=H16)           # V^T [H * 64 rows][B * nk_pad]
        self.vt[:, :, :nk] = c["v"].reshape(b, nk, hd).permute(2, 0, 1)
        g = c["xk"].shape[0]
        self.xk = c["xk"].reshape(g, I.XKEYS, hd).clone()                           # [G, 64, H * 64]
        self.xvt = torch.full((hd, g, I.XKEYS), I.VT_PAD, dtype=H16)
        for s, n in c["segments"]:
            self.xvt[:, :, s:s + n] = c["xv"].reshape(g, I.XKEYS, hd)[:, s:s + n].permute(2, 0, 1)
        self.groups = g
        self.o_rs = hd + O_EXTRA
        self.o_bs = (nq + O_ROWS_EXTRA) * self.o_rs
        for name in ("q", "k", "vt", "xk", "xvt"):
            setattr(self, name, getattr(self, name).to(DEV))
        self.xvt = self.xvt.view(hd, g * I.XKEYS)

    def fresh_o(self):
        return torch.full((GUARD + self.b * self.o_bs + GUARD,), CANARY, dtype=H16, device=DEV)

    def launch(self, segments, weights, obuf=None, **over):
        obuf = self.fresh_o() if obuf is None else obuf
        hd = self.h * I.D
        out = obuf[GUARD + O_COL0:].as_strided((self.b * (self.nq + O_ROWS_EXTRA), hd), (self.o_rs, 1))
        kw = dict(batch=self.b, heads=self.h, nq=self.nq, nk=self.nk, nk_pad=self.nk_pad, dpad=I.D, scale=SCALE, images_per_group=self.b // self.groups,
                  q_bs=self.q.stride(0), q_rs=self.q.stride(1), k_bs=self.k.stride(0), k_rs=self.k.stride(1), vt_bs=self.nk_pad, vt_hs=I.D * self.vt.stride(0),
                  vt_ds=self.vt.stride(0), out=out, o_bs=self.o_bs)
        kw.update(over)
        ops.attention_dual(self.q, self.k, self.vt, self.xk, self.xvt, [(s, n, w) for (s, n), w in zip(segments, weights)], **kw)
        torch.cuda.synchronize()
        return obuf

    def window(self, obuf):
        """-> (O [B, H, nq, D] on the CPU, mask of the buffer's elements that belong to the window)"""
        hd = self.h * I.D
        idx = (GUARD + O_COL0 + torch.arange(self.b)[:, None, None] * self.o_bs + torch.arange(self.nq)[None, :, None] * self.o_rs + torch.arange(hd)[None, None, :])
        inside = torch.zeros(obuf.numel(), dtype=torch.bool)
        inside[idx.reshape(-1)] = True
        o = obuf.cpu()[idx.reshape(-1)].view(self.b, self.nq, self.h, I.D).permute(0, 2, 1, 3)
        return o, inside


_cases = {}


def case_of(nq, nk, name):
    """the case, its device buffers and its fp64 terms, made once and shared"""
    key = (nq, nk, name)
    if key not in _cases:
        c = I.make_case(nq, nk, name)
        _cases[key] = (c, Buffers(c), I.dual_terms(c, SCALE))
    return _cases[key]


@pytest.mark.parametrize("nk", I.NKS)
@pytest.mark.parametrize("nq", I.NQS)
def test_attention_dual_vs_fp64_within_the_bound(nq, nk):
    """fmxi_attention_dual_f16: every segment layout and weight; everything outside O's window keeps its bits; at weight 0 a single segment gives
    text-only attention within ATTN_TOL"""
    worst = 0.0
    for name in I.SEGMENTS:
        c, buf, (text, terms) = case_of(nq, nk, name)
        for w in I.WEIGHTS:
            weights = I.weights_of(name, w)
            obuf = buf.launch(c["segments"], weights)
            got, inside = buf.window(obuf)
            want = text + sum(wi * t for wi, t in zip(weights, terms))
            e = I.excess(got, want, I.dual_bound(want, weights))
            worst = max(worst, e)
            assert e <= 1.0, f"nq {nq} nk {nk} {name} weights {weights}: {e:.3f} x the bound"
            assert bool((obuf.cpu()[~inside] == CANARY).all()), f"nq {nq} nk {nk} {name}: elements outside O's window were written"
            if all(wi == 0.0 for wi in weights):
                R.assert_within(got, text, H16, *R.ATTN_TOL[H16], f"nq {nq} nk {nk} {name}: weight 0 against text-only attention")
    print(f"[attention_dual] nq {nq} nk {nk}: worst {worst:.3f} x the bound")
    assert worst > 0.01       # the bound is not vacuous


def test_attention_dual_is_bit_identical_over_three_launches_and_has_teeth():
    c, buf, _ = case_of(320, 77, "two_units")
    weights = [0.35, 1.0]
    runs = [buf.window(buf.launch(c["segments"], weights))[0] for _ in range(3)]
    assert torch.equal(bits(runs[0]), bits(runs[1])) and torch.equal(bits(runs[0]), bits(runs[2]))
    # the gate tells the kernel's arithmetic from each planted mistake on this very output
    for bug in ("joint_softmax", "one_softmax_for_all_segments", "swap_groups", "weight_before_softmax"):
        wrong = I.dual_ref(c, weights, SCALE, bug=bug)
        assert I.excess(runs[0], wrong, I.dual_bound(wrong, weights)) >= I.TEETH_FACTOR, bug


def test_attention_dual_follows_the_group_of_each_image():
    """images_per_group 1 and 4 on the same buffers: image b reads group b // images_per_group"""
    c = I.make_case(64, 77, "base4", seed=3)
    c4 = dict(c, xk=c["xk"].repeat(2, 1, 1, 1), xv=c["xv"].repeat(2, 1, 1, 1))
    c4["xk"][2:] *= 0.5
    buf = Buffers(c4)
    got = buf.window(buf.launch(c["segments"], [1.0]))[0]
    text, terms = I.dual_terms(c4, SCALE, images_per_group=1)
    want = text + terms[0]
    assert I.excess(got, want, I.dual_bound(want, [1.0])) <= 1.0
    c1 = dict(c, xk=c["xk"][1:], xv=c["xv"][1:])
    buf = Buffers(c1)
    got = buf.window(buf.launch(c["segments"], [1.0]))[0]
    text, terms = I.dual_terms(c1, SCALE, images_per_group=4)
    want = text + terms[0]
    assert I.excess(got, want, I.dual_bound(want, [1.0])) <= 1.0


BAD = [
    ("dpad", dict(dpad=48), "dpad 48"),
    ("no text key", dict(nk=0), "nk 0 not in 1..128"),
    ("too many text keys", dict(nk=129, nk_pad=192), "nk 129 not in 1..128"),
    ("nk_pad", dict(nk_pad=100), "nk_pad"),
    ("no query", dict(nq=0), "bad dims"),
    ("groups", dict(images_per_group=3), "images_per_group"),
    ("stride", dict(q_rs=129), "multiples of 8"),
]
BAD_SEGMENTS = [
    ("no segment", [], "segments"),
    ("five segments", [(i * 4, 4, 1.0) for i in range(5)], "segments"),
    ("empty segment", [(0, 0, 1.0)], "does not lie inside"),
    ("negative start", [(-1, 4, 1.0)], "does not lie inside"),
    ("past 64", [(60, 5, 1.0)], "does not lie inside"),
    ("overlap", [(0, 8, 1.0), (7, 4, 1.0)], "overlap"),
    ("weight", [(0, 4, float("inf"))], "not finite"),
]


def test_attention_dual_refuses_before_touching_o():
    """every FMX_E_BADARG case of include/fmx_ipadapter.h, by message; O keeps every bit"""
    c, buf, _ = case_of(64, 77, "base4")
    obuf = buf.fresh_o()
    for what, over, msg in BAD:
        with pytest.raises((_lib.FmxError, ValueError), match=msg):
            buf.launch(c["segments"], [1.0], obuf=obuf, **over)
    for what, segs, msg in BAD_SEGMENTS:
        with pytest.raises((_lib.FmxError, ValueError), match=msg):
            ops.attention_dual(buf.q, buf.k, buf.vt, buf.xk, buf.xvt, segs, batch=buf.b, heads=buf.h, nq=buf.nq, nk=buf.nk, nk_pad=buf.nk_pad, dpad=I.D,
                               scale=SCALE, images_per_group=2, q_bs=buf.q.stride(0), q_rs=buf.q.stride(1), k_bs=buf.k.stride(0), k_rs=buf.k.stride(1),
                               vt_bs=buf.nk_pad, vt_hs=I.D * buf.vt.stride(0), vt_ds=buf.vt.stride(0),
                               out=obuf[GUARD + O_COL0:].as_strided((buf.b * (buf.nq + O_ROWS_EXTRA), buf.h * I.D), (buf.o_rs, 1)), o_bs=buf.o_bs)
    # the library itself, past the wrapper's own checks: a null extra context and a misaligned one
    a = _lib.DualAttnArgs()
    a.q, a.k, a.vt, a.o = (C.c_void_p(t.data_ptr()) for t in (buf.q, buf.k, buf.vt, obuf))
    a.batch, a.heads, a.nq, a.nk, a.nk_pad, a.dpad, a.scale, a.images_per_group, a.nseg = 4, 2, 64, 77, 128, 64, SCALE, 2, 1
    a.seg_count0, a.seg_weight0 = 4, 1.0
    a.q_rs = a.k_rs = a.o_rs = 128
    a.vt_ds = 512
    lib = _lib.lib()
    assert lib.fmxi_attention_dual_f16(C.byref(a), None) == _lib.CONSTANTS["FMX_E_BADARG"] and b"null pointer" in lib.fmx_last_error()
    a.xk, a.xvt = C.c_void_p(buf.xk.data_ptr() + 2), C.c_void_p(buf.xvt.data_ptr())
    assert lib.fmxi_attention_dual_f16(C.byref(a), None) == _lib.CONSTANTS["FMX_E_BADARG"] and b"16-byte alignment" in lib.fmx_last_error()
    torch.cuda.synchronize()
    assert bool((obuf == CANARY).all())


# ---- the executor against the reference -------------------------------------------------------------------------------------------------------------------
from forge_amd import runtime, synth  # noqa: E402
from forge_amd.backend.nn import ipadapter as nets  # noqa: E402
from forge_amd.backend.patcher import controlnet as pc  # noqa: E402
from forge_amd.backend.patcher import ipadapter as ipa  # noqa: E402
from forge_amd.backend.patcher.ipadapter import patch_ipadapter  # noqa: E402
from forge_amd.backend.patcher.kohya_hrfix import patch_kohya_hrfix  # noqa: E402
from forge_amd.modules import processing, shared  # noqa: E402
from forge_amd.modules.prompt_parser import DictWithShape  # noqa: E402

from conftest import load_golden  # noqa: E402
import lllite_refs as L  # noqa: E402
import parity  # noqa: E402
from parity import check  # noqa: E402
from test_gpu_pag import engine_of  # noqa: E402

# heads of 64, and heads of 16 / 32 padded to 64: the dual route; heads of 64 and of 128 (padded to 160): the dual route and, at 128, the composite route
CONFIGS = ("TINY_SDXL_2LEVEL_UNET_CONFIG", "TINY_SD15_UNET_CONFIG", "TINY_SD15_WIDE_HEADS_UNET_CONFIG")


@pytest.fixture(scope="module")
def fx():
    g = load_golden("ipadapter.pt")
    assert tuple(g["configs"]) == CONFIGS and tuple(g["hw"]) == (32, 32) and g["b"] == 2 and g["cfg"] == 7.0 and g["kv_gain"] == 1.0
    # (the gain the image tokens needed to move the output by 10 x the floor: the init law's own, 1.0 -- asserted per case below)
    for config in CONFIGS:
        for case, v in g["floor"][config].items():
            parity.FLOORS[f"ipadapter.pt:{config}/{case}"] = v
    for kind, v in g["tokens_floor"].items():
        parity.FLOORS[f"ipadapter.pt:tokens/{kind}"] = v
    return g


_jobs = {}


@pytest.fixture(scope="module", autouse=True)
def leave_no_static_buffers():
    """the engines are shared with other test files (test_gpu_pag.engine_of): the sampling jobs below create KModel's static buffers under
    inference mode, which a later direct denoise_cfg call of another file on the same shape could not write to"""
    yield
    for job in _jobs.values():
        job["km"]._drop_graphs()
        job["km"]._static.clear()


def job_of(fx, config):
    """the fixture's job of one config on the device, built once: engine, KModel, inputs, the two IP-Adapter files and their embeddings"""
    if config not in _jobs:
        cfg = dict(getattr(synth, config))
        eng = engine_of(config, fx["weight_seed"])
        km = eng.forge_objects.unet.model
        sig_host = km.predictor.sigma(torch.tensor(fx["t"]))
        x, cond, uncond = L.case_inputs(cfg, fx["hw"], fx["seed"], sig_host, fx["b"])
        as_ctx = lambda d: (d["crossattn"].to(DEV), d["vector"].to(DEV)) if isinstance(d, dict) else (d.to(DEV), None)  # noqa: E731
        files = {kind: synth.synth_ipadapter_state_dict(cfg, plus=kind == "plus", seed=fx["file_seeds"][kind], kv_gain=fx["kv_gain"]) for kind in ("base", "plus")}
        _jobs[config] = dict(cfg=cfg, eng=eng, km=km, net=km.diffusion_model, x=x.to(DEV), sigma=sig_host.float().to(DEV), c=as_ctx(cond), uc=as_ctx(uncond),
                             files=files)
    return _jobs[config]


def units(job, spec, unet=None, **kw):
    """spec [(file kind, weight, weight type)] -> the patched UnetPatcher"""
    m = unet or job["eng"].forge_objects.unet
    for kind, weight, weight_type in spec:
        m = patch_ipadapter(m, job["files"][kind], synth.synth_clip_vision_embeds(plus=kind == "plus"), weight, weight_type, **kw)
    return m


def python_units(job, spec, **kw):
    """the same units as attn2 replace patches: what patch_ipadapter installs where the native route does not apply"""
    return ipa.install_python(job["eng"].forge_objects.unet.clone(), units(job, spec, **kw).model_options["transformer_options"]["ipadapter"])


class Counted:
    """counts the launches of the two routes' own ops"""

    def __init__(self, monkeypatch, net):
        self.dual, self.added, self.hooked = [], [], []
        real_dual, real_add, real_hooked = ops.attention_dual, ops.add_scaled_, net._attn_block_hooked
        monkeypatch.setattr(ops, "attention_dual", lambda *a, **kw: (self.dual.append(len(a[5])), real_dual(*a, **kw))[1])
        monkeypatch.setattr(ops, "add_scaled_", lambda *a, **kw: (self.added.append(a[2]), real_add(*a, **kw))[1])
        monkeypatch.setattr(net, "_attn_block_hooked", lambda *a, **kw: (self.hooked.append(a[0]), real_hooked(*a, **kw))[1], raising=False)

    def clear(self):
        del self.dual[:], self.added[:], self.hooked[:]


@pytest.mark.parametrize("config", CONFIGS)
def test_denoise_cfg_vs_the_reference_with_its_patch(fx, config, monkeypatch):
    """CFG 7 ([uncond ; cond]: the two groups read different image tokens), base and plus files, one and two units, the three weight types, under
    the floor-keyed gates of tests/parity.py; without the option the same call misses the gate by far"""
    job = job_of(fx, config)
    km, x, sigma = job["km"], job["x"], job["sigma"]
    count = Counted(monkeypatch, job["net"])
    plain = km.denoise_cfg(x, sigma, job["uc"], job["c"], 7.0).clone()
    check(f"ipadapter {config}: the unpatched call vs the reference", plain, fx["plain"][config], floor=f"ipadapter.pt:{config}/base/original")
    assert set(fx["cases"]) == {"base/original", "plus/original", "base/linear", "plus/channel", "two_units"}
    for case, spec in fx["cases"].items():
        tag = f"{config}/{case}"
        count.clear()
        den = km.denoise_cfg(x, sigma, job["uc"], job["c"], 7.0, transformer_options=units(job, spec).model_options["transformer_options"]).clone()
        assert count.hooked == []
        assert set(count.dual) == {len(spec)} and len(count.dual) + len(count.added) // len(spec) == 7, "every cross-attention took one of the two routes"
        if config == CONFIGS[2]:
            assert len(count.added) == 4 * len(spec), "the four blocks at 256 channels have heads of 128: the composite route"
        else:
            assert count.added == [], "heads padded to 64: one dual launch per cross-attention"
        check(f"ipadapter {tag}: native IP-Adapter vs the reference with its patch", den, fx["results"][config][case], floor=f"ipadapter.pt:{tag}")
        floor = fx["floor"][config][case]["rms_rel"]
        moved = parity.metrics(den, plain)["rms_rel"]
        print(f"{tag}: moved {moved:.3e} from the unpatched call, floor {floor:.3e}")
        assert moved >= 10 * floor and fx["moved"][config][case] >= 10 * floor
        assert parity.metrics(plain, fx["results"][config][case])["rms_rel"] > 3 * parity.limits(f"ipadapter.pt:{tag}")[1]["rms_rel"]


@pytest.mark.parametrize("config", CONFIGS)
def test_native_route_vs_python_patch_on_the_hooked_executor(fx, config, monkeypatch):
    job = job_of(fx, config)
    km, x, sigma = job["km"], job["x"], job["sigma"]
    count = Counted(monkeypatch, job["net"])
    for case, spec in fx["cases"].items():
        count.clear()
        native = km.denoise_cfg(x, sigma, job["uc"], job["c"], 7.0, transformer_options=units(job, spec).model_options["transformer_options"]).clone()
        assert count.hooked == []
        via_python = km.denoise_cfg(x, sigma, job["uc"], job["c"], 7.0, transformer_options=python_units(job, spec).model_options["transformer_options"])
        assert len(count.hooked) == 7
        check(f"ipadapter {config}/{case}: native vs python_patch on the hooked executor", native, via_python, floor=f"ipadapter.pt:{config}/{case}", both_fp16=True)


def test_image_projections_on_the_device_vs_the_references(fx):
    """ImageProjModel and the Resampler on the existing ops against the reference's fp32 networks, under the floor of its own fp16 run"""
    job = job_of(fx, CONFIGS[0])
    for kind in ("base", "plus"):
        u = units(job, [(kind, 1.0, "original")]).model_options["transformer_options"]["ipadapter"][0]
        got = torch.cat(u.image_tokens())
        assert got.dtype == H16 and got.is_cuda and got.shape == (2, 16 if kind == "plus" else 4, job["cfg"]["context_dim"])
        check(f"ipadapter image tokens ({kind})", got, torch.cat(fx["tokens"][kind]), floor=f"ipadapter.pt:tokens/{kind}")


@pytest.mark.parametrize("config", CONFIGS)
def test_outside_the_window_the_call_is_the_plain_call_bit_for_bit(fx, config):
    job = job_of(fx, config)
    km, x = job["km"], job["x"]
    w = fx["windowed"][config]
    assert w["outside"] and w["sigma_end"] < float(job["sigma"][0]) < w["sigma_start"]
    to = units(job, fx["cases"]["base/original"], start_at=fx["window"][0], end_at=fx["window"][1]).model_options["transformer_options"]
    for s in (w["sigma_start"] * 1.5, w["sigma_end"] * 0.5):
        sigma = torch.full_like(job["sigma"], s)
        plain = km.denoise_cfg(x, sigma, job["uc"], job["c"], 7.0).clone()
        keys = set(km._static)
        off = km.denoise_cfg(x, sigma, job["uc"], job["c"], 7.0, transformer_options=to).clone()
        assert set(km._static) == keys, "a call outside the window must use the plain key"
        assert torch.equal(bits(off.cpu()), bits(plain.cpu()))
    keys = set(km._static)
    on = km.denoise_cfg(x, job["sigma"], job["uc"], job["c"], 7.0, transformer_options=to).clone()
    assert any("ipadapter" in k for k in set(km._static) - keys)
    check(f"ipadapter {config}: inside the window vs the reference", on, fx["results"][config]["base/original"], floor=f"ipadapter.pt:{config}/base/original")


def test_dual_route_vs_composite_route_on_the_same_block_inputs(fx):
    """one cross-attention of the SDXL-shaped net (2 heads of 64, 1024 queries, 77 text keys, two units) through both routes on the same Q, text
    K / V^T and cached extra context, each against the fp64 reference on those tensors.  Dual: the kernel bound.  Composite: every term is its own
    attention launch (ATTN_TOL each, the units' scaled by |w|) and the sum is rounded to fp16 once per unit: + 1 ulp(O) per unit."""
    job = job_of(fx, CONFIGS[0])
    net = job["net"]
    to = units(job, fx["cases"]["two_units"]).model_options["transformer_options"]
    ctx = ipa.ipadapter_for_call(to, 1.0, [1, 0], 4, net)
    b = "input_blocks.3.1.transformer_blocks.0"
    ent = ctx.blocks[b]
    bu, n, H, d, tokens, tp = 4, 1024, 2, 64, 77, 128
    g = torch.Generator().manual_seed(9)
    q2 = torch.randn(bu * n, H * d, generator=g).to(H16).to(DEV)
    kc = torch.randn(bu * tp, H * d, generator=g).to(H16).to(DEV)
    vtc = torch.randn(H * d, bu * tp, generator=g).to(H16).to(DEV)
    dual = net._cross_attention(b, q2, kc, vtc, bu, n, tokens, tp, H, d, ctx).cpu()
    ctx.force_composite = True
    try:
        comp = net._cross_attention(b, q2, kc, vtc, bu, n, tokens, tp, H, d, ctx).cpu()
    finally:
        ctx.force_composite = False
    heads = lambda t, rows: t.cpu().double().view(-1, rows, H, d).permute(0, 2, 1, 3)   # noqa: E731
    q, k, v = heads(q2, n), heads(kc, tp)[:, :, :tokens], heads(vtc.T.contiguous(), tp)[:, :, :tokens]
    text = R.attn_ref(q, k, v, d ** -0.5)
    grp = torch.arange(bu) // 2
    xk, xv = heads(ent["xk"].reshape(-1, H * d), 64)[grp], heads(ent["xvt"].T.contiguous(), 64)[grp]
    weights = [w for _, _, w in ent["segments"]]
    terms = [R.attn_ref(q, xk[:, :, s:s + c], xv[:, :, s:s + c], d ** -0.5) for s, c, _ in ent["segments"]]
    want = text + sum(w * t for w, t in zip(weights, terms))
    as_o = lambda t: t.view(bu, n, H, d).permute(0, 2, 1, 3)   # noqa: E731
    e_dual = I.excess(as_o(dual), want, I.dual_bound(want, weights))
    tol = lambda t: R.ATTN_TOL[H16][0] * R.ulp(t, H16) + R.ATTN_TOL[H16][1]   # noqa: E731
    comp_bound = tol(text) + sum(abs(w) * tol(t) for w, t in zip(weights, terms)) + len(terms) * R.ulp(want, H16)
    e_comp = I.excess(as_o(comp), want, comp_bound)
    print(f"[dual vs composite] dual {e_dual:.3f} x its bound, composite {e_comp:.3f} x its bound")
    assert e_dual <= 1.0 and e_comp <= 1.0 and e_dual > 0.01 and weights == [0.8, 1.0]


# ---- sampling -----------------------------------------------------------------------------------------------------------------------------------------------
def run_job(job, unet, steps, use_graph=True, size=256):
    eng, cfg, km = job["eng"], job["cfg"], job["km"]
    saved, saved_graph = eng.forge_objects_after_applying_lora, km.use_graph
    eng.forge_objects_after_applying_lora = saved.shallow_copy()
    eng.forge_objects_after_applying_lora.unet = unet
    km.use_graph = use_graph
    try:
        c, uc = synth.synth_conditioning(2, cfg["context_dim"], cfg.get("adm_in_channels"), seed=77)
        move = lambda d: DictWithShape({k: v.to(DEV) for k, v in d.items()}) if isinstance(d, dict) else d.to(DEV)  # noqa: E731
        shared.opts.randn_source = "CPU"
        p = processing.StableDiffusionProcessingTxt2Img(sd_model=eng, c=move(c), uc=move(uc), seed=4321, sampler_name="Euler", batch_size=2, steps=steps,
                                                        cfg_scale=7.0, width=size, height=size, do_decode=False)
        return processing.process_images(p).latents.clone()
    finally:
        km.use_graph = saved_graph
        eng.forge_objects_after_applying_lora = saved
        eng.forge_objects = saved.shallow_copy()


def test_euler_job_on_the_graph_equals_the_job_run_eagerly(fx, monkeypatch):
    """6 Euler steps, start_at 0.2, end_at 0.8: exactly two graphs are captured, the plain one and the unit's, and the latents equal the eager job's"""
    job = job_of(fx, CONFIGS[0])
    km, net = job["km"], job["net"]
    count = Counted(monkeypatch, net)
    calls = []
    real_static = km._forward_static
    monkeypatch.setattr(km, "_forward_static", lambda *a, **kw: (calls.append(kw["native"].ipadapter is not None), real_static(*a, **kw))[1])
    km._drop_graphs()
    km._static.clear()
    spec = fx["cases"]["base/original"]
    on_graph = run_job(job, units(job, spec, start_at=0.2, end_at=0.8), 6)
    import re
    pattern = "".join("x" if on else "." for on in calls)
    assert len(calls) == 6 and re.fullmatch(r"\.+x{2,}\.*", pattern) and pattern.count(".") >= 2, pattern      # one window; both graphs get their second call
    assert count.hooked == []
    assert sum(any(isinstance(p, str) and p == "ipadapter" for p in k) for k in km._graphs) == 1 and len(km._graphs) == 2, list(km._graphs)
    eager = run_job(job, units(job, spec, start_at=0.2, end_at=0.8), 6, use_graph=False)
    assert torch.equal(bits(on_graph.cpu()), bits(eager.cpu())), parity.metrics(on_graph, eager)
    plain = run_job(job, job["eng"].forge_objects.unet, 6)
    assert parity.metrics(on_graph, plain)["rms_rel"] > 1e-2      # the window did something


def test_job_with_kohya_hrfix(fx, monkeypatch):
    """Kohya HRFix shrinks the hidden state inside its window: the kernel does not care about the number of queries.  Native against the same
    units as Python patches (which take the whole job, Kohya included, to the hooked executor)."""
    job = job_of(fx, CONFIGS[0])
    count = Counted(monkeypatch, job["net"])
    kohya = lambda m: patch_kohya_hrfix(m, 3, 2.0, 0.0, 0.5, True, "bicubic", "bicubic")  # noqa: E731
    spec = fx["cases"]["two_units"]
    native = run_job(job, kohya(units(job, spec)), 4)
    assert count.hooked == [] and len(count.dual) > 0 and bool(torch.isfinite(native).all())
    via_python = run_job(job, kohya(python_units(job, spec)), 4)
    assert len(count.hooked) > 0
    m = parity.metrics(native, via_python)
    print("ipadapter + Kohya HRFix, 4 Euler steps: native vs python_patch", m)
    assert m["rms_rel"] < 3e-2 and parity.metrics(native, run_job(job, kohya(job["eng"].forge_objects.unet), 4))["rms_rel"] > 10 * m["rms_rel"]


def test_job_with_a_controlnet(fx, monkeypatch):
    """a ControlNet chain rides along: its residuals are added where they always are, the cross-attentions take the dual route"""
    from forge_amd.backend.nn.cnets import cldm
    job = job_of(fx, CONFIGS[0])
    cfg = job["cfg"]
    count = Counted(monkeypatch, job["net"])
    cn = pc.ControlNet(cldm.ControlNet(cfg, synth.synth_controlnet_state_dict(cfg, seed=6), device=DEV))
    hint = torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(2)).to(DEV)
    chain = lambda m: pc.apply_controlnet_advanced(m, cn, hint, 0.8, 0.0, 1.0)  # noqa: E731
    spec = fx["cases"]["base/original"]
    native = run_job(job, chain(units(job, spec)), 4)
    assert count.hooked == [] and len(count.dual) > 0 and bool(torch.isfinite(native).all())
    via_python = run_job(job, chain(python_units(job, spec)), 4)
    m = parity.metrics(native, via_python)
    print("ipadapter + ControlNet, 4 Euler steps: native vs python_patch", m)
    assert m["rms_rel"] < 3e-2 and parity.metrics(native, run_job(job, chain(job["eng"].forge_objects.unet), 4))["rms_rel"] > 10 * m["rms_rel"]


@pytest.mark.parametrize("companion", ("freeu", "dynthresh", "stylealign"))
def test_job_with_a_native_companion(fx, companion, monkeypatch):
    """FreeU, Dynamic Thresholding and StyleAlign ride along on the native route: no hooked block, the dual launches run, and the units still move
    the result; native against the same units as Python patches where the companion has a route beside Python hooks (FreeU, Dynamic Thresholding)"""
    from forge_amd.backend.patcher.dynthresh import patch_dynthresh
    from forge_amd.backend.patcher.freeu import patch_freeu_v2
    from forge_amd.backend.patcher.stylealign import patch_stylealign
    job = job_of(fx, CONFIGS[0])
    count = Counted(monkeypatch, job["net"])
    add = {"freeu": lambda m: patch_freeu_v2(m, 1.3, 1.4, 0.9, 0.2), "dynthresh": lambda m: patch_dynthresh(m, 7.0, 0.99),
           "stylealign": lambda m: patch_stylealign(m, 0.5)}[companion]
    spec = fx["cases"]["two_units"]
    native = run_job(job, add(units(job, spec)), 4)
    assert count.hooked == [] and len(count.dual) > 0 and bool(torch.isfinite(native).all())
    without = run_job(job, add(job["eng"].forge_objects.unet), 4)
    moved = parity.metrics(native, without)["rms_rel"]
    assert moved > 3e-2, moved
    if companion != "stylealign":          # (native StyleAlign refuses Python block hooks beside it)
        m = parity.metrics(native, run_job(job, add(python_units(job, spec)), 4))
        print(f"ipadapter + {companion}, 4 Euler steps: native vs python_patch", m)
        assert m["rms_rel"] < 3e-2 and moved > 10 * m["rms_rel"]
