"""GPU: native StyleAlign.  fmxe_attn_blend_f16 (hipops.attn_blend) bit for bit against the torch expression of the reference; the shared attention
in the executor's layouts against fp64; every attn1 of every transformer block on the stored operands; KModel.denoise_cfg against the reference
with the reference's own script (tests/golden/tiny_stylealign_unet.pt, tools/make_stylealign_fixtures.py); 4-step jobs on the captured-graph path;
the native route against the same patch as a Python attn1 replace hook on the hooked executor; the plain path against its bits from before."""
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import forge_amd  # noqa: E402,F401
from forge_amd import hipops as ops  # noqa: E402
from forge_amd import runtime, synth  # noqa: E402
from forge_amd.backend.nn.layout import SpatialT  # noqa: E402
from forge_amd.backend.nn.unet import IntegratedUNet2DConditionModel as UNetExecutor  # noqa: E402
from forge_amd.backend.patcher.native_call import NativeCall  # noqa: E402
from forge_amd.backend.patcher.pag import patch_pag  # noqa: E402
from forge_amd.backend.patcher.stylealign import Share, patch_stylealign  # noqa: E402
from forge_amd.modules import processing, shared  # noqa: E402
from forge_amd.modules.prompt_parser import DictWithShape  # noqa: E402

from conftest import load_golden  # noqa: E402
import kernel_refs as R  # noqa: E402
import parity  # noqa: E402
import stylealign_refs as S  # noqa: E402
from parity import check  # noqa: E402
from test_gpu_attention_fast import cu_count, gen  # noqa: E402
from test_gpu_gemm_windows import bits  # noqa: E402
from test_gpu_pag import engine_of  # noqa: E402

DEV = "cuda"
H16 = torch.float16
TOL = R.ATTN_TOL[H16]      # the bound tests/test_gpu_attention_fast.py / test_gpu_attention_generic.py hold fmx_attention_f16 to
CANARY = 215.5


# ---- fmxe_attn_blend_f16 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alias", ["separate", "own", "shared"])
@pytest.mark.parametrize("strength", [0.01, 0.3, 0.5, 0.99])
def test_attn_blend_is_the_torch_expression_bit_for_bit(strength, alias):
    """fmxe_attn_blend_f16 against `(1.0 - s) * own + s * shared` on fp16 CPU tensors: every n, out separate or aliasing an input, the special
    values (NaN by position, everything else by bit pattern), nothing written behind n"""
    sa_, sb_ = S.special_values()
    for n in (1, 7, 8, 4097, 3 * 120 * 128, sa_.numel()):
        g = gen(int(strength * 100) + n)
        if n == sa_.numel():
            a, b = sa_, sb_
        else:
            a, b = torch.randn(n, generator=g).half(), torch.randn(n, generator=g).half()
        want = S.torch_blend(a, b, strength)
        tail = 24
        bufs = [torch.full((n + tail,), CANARY, dtype=H16) for _ in range(3)]
        bufs[0][:n], bufs[1][:n] = a, b
        da, db, dout = (t.to(DEV) for t in bufs)
        out = {"separate": dout, "own": da, "shared": db}[alias]
        res = ops.attn_blend(da[:n], db[:n], strength, out=out[:n])
        torch.cuda.synchronize()
        assert res.data_ptr() == out.data_ptr()
        got = out.cpu()
        wrong = S.same_bits_or_both_nan(got[:n], want)
        assert wrong == 0, f"strength {strength} n {n} out={alias}: {wrong} of {n} values differ from the torch expression"
        for name, t, src in (("own", da, bufs[0]), ("shared", db, bufs[1]), ("out", dout, bufs[2])):
            tc = t.cpu()
            assert torch.equal(bits(tc[n:]), bits(src[n:])), f"n {n} out={alias}: elements behind n of {name} were written"
            if t is not out:
                assert S.same_bits_or_both_nan(tc[:n], src[:n]) == 0, f"n {n} out={alias}: {name} is an input and was written"
    fresh = ops.attn_blend(da[:n], db[:n], strength)          # out=None: a new tensor
    assert fresh.data_ptr() not in (da.data_ptr(), db.data_ptr()) and fresh.shape == (n,)


# ---- the shared attention in the executor's layouts ---------------------------------------------------------------------------------------------------
def executor_operands(groups, b, n, heads, d, dp, seed, tpad):
    """[Q | K] rows and V^T columns as _attn_block leaves them: `tpad` rows / columns per group (= b * n: dense).  Pad rows of Q and K hold NaN, pad
    columns of V^T finite garbage, the head columns d .. dp zeros.  -> (qk, vt on the device, q, k, v [groups * b, n, heads * dp] on the CPU)"""
    g = gen(seed)
    t_seq, hd = b * n, heads * dp
    q, k, v = (torch.zeros(groups, t_seq, heads, dp, dtype=H16) for _ in range(3))
    for t in (q, k, v):
        t[..., :d] = torch.randn(groups, t_seq, heads, d, generator=g).half()
    q[..., :d] *= 2.0         # scores with a standard deviation of 2: attention as peaked as trained layers, not a flat average
    qk = torch.full((groups, tpad, 2 * hd), float("nan"), dtype=H16)
    qk[:, :t_seq, :hd], qk[:, :t_seq, hd:] = q.reshape(groups, t_seq, hd), k.reshape(groups, t_seq, hd)
    vt = (torch.randn(hd, groups, tpad, generator=g) * 3.0).half()
    vt[:, :, :t_seq] = v.reshape(groups, t_seq, hd).permute(2, 0, 1)
    per_image = lambda t: t.reshape(groups * b, n, hd)  # noqa: E731
    return qk.reshape(groups * tpad, 2 * hd).to(DEV), vt.reshape(hd, groups * tpad).to(DEV), per_image(q), per_image(k), per_image(v)


def route_of(groups, heads, t_seq, tpad, dp, hd, cols):
    import ctypes as C
    from forge_amd import _lib
    a = _lib.AttnArgs()
    a.q = a.k = a.vt = a.o = a.zero_page = 0x7F0000001000
    a.batch, a.heads, a.nq, a.nk, a.nk_pad, a.dpad, a.scale = groups, heads, t_seq, t_seq, tpad, dp, 0.125
    a.q_bs, a.q_rs, a.k_bs, a.k_rs, a.vt_bs, a.vt_hs, a.vt_ds = tpad * 2 * hd, 2 * hd, tpad * 2 * hd, 2 * hd, tpad, dp * cols, cols
    a.o_bs, a.o_rs = t_seq * hd, hd
    buf = C.create_string_buffer(64)
    _lib.check(_lib.lib().fmx_attention_route(C.byref(a), cu_count(), buf, len(buf)), "fmx_attention_route")
    return buf.value.decode()


# (groups, b, n, heads, d, dpad): T 768 on a fast route; T 360 in group-padded buffers of 384; SD1.5's d 40 at its MFMA granule, T 192, generic
SHARED_CASES = [(2, 3, 256, 2, 64, 64), (2, 3, 120, 2, 64, 64), (2, 4, 48, 2, 40, 48)]


@pytest.mark.parametrize("i", range(len(SHARED_CASES)))
def test_shared_attention_in_the_executors_layout_vs_fp64(i):
    groups, b, n, heads, d, dp = SHARED_CASES[i]
    t_seq, hd = b * n, heads * dp
    tpad = -(-t_seq // 64) * 64
    qk, vt, q, k, v = executor_operands(groups, b, n, heads, d, dp, 60 + i, tpad)
    route = route_of(groups, heads, t_seq, tpad, dp, hd, groups * tpad)
    assert (route == "generic") == (i == 2), route
    if dp == 64:
        o = UNetExecutor._shared_attention(None, qk, vt, groups * b, n, tpad, heads, d, Share(b, "aligned", 1.0), None, False)
    else:       # the executor pads heads of up to 64 to 64; the narrower granule through the same strides
        o = ops.attention(qk, qk[:, hd:], vt, batch=groups, heads=heads, nq=t_seq, nk=t_seq, nk_pad=tpad, dpad=dp, scale=d ** -0.5, q_bs=tpad * 2 * hd,
                          q_rs=2 * hd, k_bs=tpad * 2 * hd, k_rs=2 * hd, vt_bs=tpad, vt_hs=dp * groups * tpad, vt_ds=groups * tpad, o_bs=t_seq * hd)
    torch.cuda.synchronize()
    assert o.shape == (groups * b * n, hd)
    want = S.shared_attention_ref(q, k, v, heads, b, scale=d ** -0.5)
    e = R.excess(o.view(groups * b, n, hd), want, H16, *TOL)
    print(f"[stylealign shared attention] {SHARED_CASES[i]} route {route}: {e:.3f} x ATTN_TOL")
    assert e <= 1.0
    # not the ordinary attention: the gate tells them apart
    assert R.excess(o.view(groups * b, n, hd), S.shared_attention_ref(q, k, v, heads, 1, scale=d ** -0.5), H16, *TOL) > 10.0


# ---- every attn1 of every block -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    g = load_golden("tiny_stylealign_unet.pt")
    for i, c in enumerate(g["cases"]):
        for k, v in c["floor"].items():
            parity.FLOORS[f"tiny_stylealign_unet.pt:{i}/{k}"] = v
    for k, e in g["euler4"].items():
        parity.FLOORS[f"tiny_stylealign_unet.pt:euler4/{k}"] = e["floor"]
    return g


WANT_CASES = [("TINY_SDXL_UNET_CONFIG", (32, 32), 3), ("TINY_SD15_UNET_CONFIG", (32, 24), 3), ("TINY_SDXL_UNET_CONFIG", (24, 20), 3),
              ("TINY_SDXL_UNET_CONFIG", (20, 18), 3), ("TINY_SD15_UNET_CONFIG", (32, 24), 4)]


def tapped_forward(cfg, hh, ww, bu, share, pag_from=None, seed=0):
    net = engine_of_net(cfg)
    g = gen(80 + seed)
    xs = torch.randn(bu, cfg["in_channels"], hh, ww, generator=g).to(DEV) * 2.0
    ctx = torch.randn(bu, 77, cfg["context_dim"], generator=g).to(DEV)
    y = torch.randn(bu, cfg["adm_in_channels"], generator=g).to(DEV) if cfg.get("adm_in_channels") else None
    xcol = ops.unet_pack_input(xs, torch.full((bu,), 2.0, device=DEV), 1, 1.0)
    t = torch.full((bu,), 400.0, device=DEV)
    taps = {}
    wanted = tuple(f".attn{a}.{w}" for a in (1, 2) for w in "qkvo")
    net.tap = lambda name, tens: taps.__setitem__(name, tens.detach().to("cpu", copy=True)) if name.endswith(wanted) else None
    try:
        net.forward_packed(xcol, t, net.prepare_context(ctx, y), bu, hh, ww, native=NativeCall(pag_from=pag_from, share=share))
    finally:
        net.tap = None
    torch.cuda.synchronize()
    return net, taps


_nets = {}


def engine_of_net(cfg):
    key = tuple(sorted((k, str(v)) for k, v in cfg.items()))
    if key not in _nets:
        _nets[key] = UNetExecutor(cfg, synth.synth_unet_state_dict(cfg, seed=3), device=DEV)
    return _nets[key]


def blocks_of(net):
    return {f"{L.key}.transformer_blocks.{di}": L for L in net.layout.all_layers() if isinstance(L, SpatialT) for di in range(L.depth)}


def check_blocks(net, taps, share, groups_of_block, what):
    """attn1.o of every transformer block against the fp64 shared attention (or the blend of the two fp64 attentions) of that block's own stored
    operands; attn2.o against its ordinary attention.  groups_of_block(key) -> (rows that are shared, rows whose O must be V bit for bit)"""
    blocks = blocks_of(net)
    assert len(blocks) >= 3 and all(k + ".attn1.o" in taps and k + ".attn1.q" in taps for k in blocks), sorted(taps)
    worst = 0.0
    for key, L in blocks.items():
        q, k, v, o = (taps[f"{key}.attn1.{w}"] for w in "qkvo")
        scale = L.dim_head ** -0.5
        rows, vrows = groups_of_block(key)
        sh = S.shared_attention_ref(q[:rows], k[:rows], v[:rows], L.heads, share.b, scale=scale)
        own = S.shared_attention_ref(q[:rows], k[:rows], v[:rows], L.heads, 1, scale=scale)
        want = sh if share.mode == "aligned" else (1.0 - share.strength) * own + share.strength * sh
        e = R.excess(o[:rows], want, H16, *TOL)
        worst = max(worst, e)
        assert e <= 1.0, f"{what} {key} attn1.o: {e:.3g} x ATTN_TOL of the fp64 {share.mode} attention"
        assert R.excess(o[:rows], own, H16, *TOL) > 1.0, f"{what} {key}: attn1.o is the ordinary attention"
        if vrows:
            assert torch.equal(bits(o[rows:rows + vrows]), bits(v[rows:rows + vrows])), f"{what} {key}: the perturbed group's O is not its V"
        q2, k2, v2, o2 = (taps[f"{key}.attn2.{w}"] for w in "qkvo")
        e2 = R.excess(o2, S.shared_attention_ref(q2, k2, v2, L.heads, 1, scale=scale), H16, *TOL)
        assert e2 <= 1.0, f"{what} {key} attn2.o: {e2:.3g} x ATTN_TOL of its ordinary attention"
    print(f"[stylealign blocks] {what}: worst attn1.o {worst:.3f} x ATTN_TOL over {len(blocks)} blocks")


@pytest.mark.parametrize("mode", ["aligned", "blend"])
@pytest.mark.parametrize("i", range(len(WANT_CASES)))
def test_every_attn1_of_every_block_is_shared_and_attn2_is_not(fx, i, mode):
    assert [(c["config"], tuple(c["hw"]), c["b"]) for c in fx["cases"]] == WANT_CASES
    name, (hh, ww), b = WANT_CASES[i]
    cfg = dict(getattr(synth, name))
    share = Share(b, mode, 1.0 if mode == "aligned" else 0.5)
    net, taps = tapped_forward(cfg, hh, ww, 2 * b, share, seed=i)
    check_blocks(net, taps, share, lambda key: (2 * b, 0), f"case {i} {mode}")


@pytest.mark.parametrize("mode", ["aligned", "blend"])
def test_with_pag_the_perturbed_group_keeps_v_in_the_middle_and_is_a_group_elsewhere(mode):
    cfg = dict(synth.TINY_SDXL_UNET_CONFIG)
    b = 3
    share = Share(b, mode, 1.0 if mode == "aligned" else 0.5)
    net, taps = tapped_forward(cfg, 32, 32, 3 * b, share, pag_from=2 * b, seed=9)
    assert any(k.startswith("middle_block.") for k in blocks_of(net))
    check_blocks(net, taps, share, lambda key: (2 * b, b) if key.startswith("middle_block.") else (3 * b, 0), f"pag + {mode}")


# ---- KModel against the reference -----------------------------------------------------------------------------------------------------------------------
def as_ctx(d):
    return (d["crossattn"].to(DEV), d["vector"].to(DEV)) if isinstance(d, dict) else (d.to(DEV), None)


@pytest.mark.parametrize("i", range(len(WANT_CASES)))
def test_denoise_cfg_vs_the_reference_with_its_script(fx, i):
    """every fixture case at CFG 7 ([uncond ; cond]) and CFG 1 (cond only), strengths 1.0 and 0.5, under the floor-keyed gates with the unchanged
    factors of tests/parity.py; the same call without the option, and with the other strength, misses the gate"""
    c = fx["cases"][i]
    assert (c["config"], tuple(c["hw"]), c["b"]) == WANT_CASES[i] and fx["cfg"] == 7.0 and fx["strengths"] == [1.0, 0.5]
    eng = engine_of(c["config"], c["weight_seed"])
    km = eng.forge_objects.unet.model
    cfg = dict(getattr(synth, c["config"]))
    sig_host = km.predictor.sigma(torch.tensor(c["t"]))
    x, cond, uncond = S.case_inputs(cfg, c["hw"], c["seed"], sig_host, c["b"])
    x, sigma = x.to(DEV), sig_host.float().to(DEV)
    cctx, uctx = as_ctx(cond), as_ctx(uncond)
    for strength in fx["strengths"]:
        to = patch_stylealign(eng.forge_objects.unet, strength).model_options["transformer_options"]
        other = patch_stylealign(eng.forge_objects.unet, 1.5 - strength).model_options["transformer_options"]
        for cs, u in ((7.0, uctx), (1.0, None)):
            tag = f"s{strength}/cfg{int(cs)}"
            key = f"tiny_stylealign_unet.pt:{i}/{tag}"
            den = km.denoise_cfg(x, sigma, u, cctx, cs, transformer_options=to)
            check(f"tiny_stylealign case {i} ({c['name']}) {tag}: native StyleAlign vs the reference with its script", den, c["results"][tag], floor=key)
            lim = parity.limits(key)[1]["rms_rel"]
            for what, opts in (("without the option", None), ("at the other strength", other)):
                m = parity.metrics(km.denoise_cfg(x, sigma, u, cctx, cs, transformer_options=opts), c["results"][tag])
                print(f"case {i} {tag} {what}: rms_rel {m['rms_rel']:.3e} against the gate {lim:.3e}")
                assert m["rms_rel"] > 3 * lim, (tag, what, m, lim)
            assert min(c["moved"][tag], c["vs_other_strength"][tag]) >= 10 * c["floor"][tag]["rms_rel"]


# ---- sampling on the captured-graph path ----------------------------------------------------------------------------------------------------------------
def run_job(eng, e4, unet=None, images=None):
    """the fixture's 4-step Euler job (its first `images` images) through process_images -> the latents"""
    cfg = dict(getattr(synth, e4["config"]))
    b = len(e4["seeds"])
    saved = eng.forge_objects_after_applying_lora
    if unet is not None:
        eng.forge_objects_after_applying_lora = saved.shallow_copy()
        eng.forge_objects_after_applying_lora.unet = unet
    try:
        c, uc = synth.synth_conditioning(b, cfg["context_dim"], cfg.get("adm_in_channels"), seed=e4["cond_seed"])
        b = images or b
        move = lambda d: DictWithShape({k: v[:b].to(DEV) for k, v in d.items()}) if isinstance(d, dict) else d[:b].to(DEV)  # noqa: E731
        shared.opts.randn_source = "CPU"
        p = processing.StableDiffusionProcessingTxt2Img(sd_model=eng, c=move(c), uc=move(uc), seed=e4["seeds"][0], sampler_name="Euler", batch_size=b,
                                                        steps=e4["steps"], cfg_scale=7.0, width=e4["hw"] * 8, height=e4["hw"] * 8, do_decode=False)
        return processing.process_images(p).latents.clone()
    finally:
        eng.forge_objects_after_applying_lora = saved
        eng.forge_objects = saved.shallow_copy()


def test_euler_jobs_replay_their_own_graph_and_b1_is_the_plain_job(fx, monkeypatch):
    """4-step Euler, CFG 7, b = 3: strength 0.5, then 1.0 on the same engine, each against its own fixture (a stale capture of the other strength would
    miss it); no hooked forward, the fourth step a graph replay; one image per group is the job without the option, bit for bit"""
    eng = engine_of(fx["euler4"]["s0.5"]["config"])
    km = eng.forge_objects.unet.model
    net = km.diffusion_model
    hooked, launches, blends = [], [], []
    real_hooked = net._attn_block_hooked
    monkeypatch.setattr(net, "_attn_block_hooked", lambda *a, **kw: (hooked.append(1), real_hooked(*a, **kw))[1], raising=False)
    real_launch, real_blend = runtime.HipGraph.launch, ops.attn_blend
    monkeypatch.setattr(runtime.HipGraph, "launch", lambda self, s: (launches.append(1), real_launch(self, s))[1])
    monkeypatch.setattr(ops, "attn_blend", lambda *a, **kw: (blends.append(a[2]), real_blend(*a, **kw))[1])
    km._drop_graphs()
    lats = {}
    for strength in (0.5, 1.0):
        e4 = fx["euler4"][f"s{strength}"]
        assert e4["strength"] == strength and e4["steps"] == 4 and len(e4["seeds"]) == 3
        n_launch, n_blend = len(launches), len(blends)
        lats[strength] = run_job(eng, e4, patch_stylealign(eng.forge_objects.unet, strength))
        check(f"tiny_stylealign 4-step Euler at strength {strength} vs reference", lats[strength], e4["latent"], floor=f"tiny_stylealign_unet.pt:euler4/s{strength}")
        assert e4["moved"] >= 10 * e4["floor"]["rms_rel"] and e4["vs_other_strength"] >= 10 * e4["floor"]["rms_rel"]
        # KModel._forward_static: step 1 is an eager warm-up, step 2 warms up again and captures (the capture is launched once), steps 3 and 4 replay
        assert len(launches) - n_launch == 3, launches
        assert (len(blends) > n_blend) == (strength == 0.5) and set(blends) <= {0.5}
    keys = [k for k in km._graphs if "stylealign" in k]
    assert sorted(k[5:] for k in keys) == [("stylealign", "aligned", 1.0), ("stylealign", "blend", 0.5)] and all(k[:5] == (3, 4, 16, 16, 2) for k in keys), keys
    assert hooked == []
    lim = parity.limits("tiny_stylealign_unet.pt:euler4/s0.5")[1]["rms_rel"]
    assert parity.metrics(lats[1.0], fx["euler4"]["s0.5"]["latent"])["rms_rel"] > 3 * lim
    # the first job again: its own graph, the same bits
    again = run_job(eng, fx["euler4"]["s0.5"], patch_stylealign(eng.forge_objects.unet, 0.5))
    assert torch.equal(again, lats[0.5])
    # b = 1
    with_option = run_job(eng, fx["euler4"]["s0.5"], patch_stylealign(eng.forge_objects.unet, 0.5), images=1)
    without = run_job(eng, fx["euler4"]["s0.5"], images=1)
    assert torch.equal(with_option, without) and not any(k[0] == 1 and "stylealign" in k for k in km._graphs)
    assert hooked == []


def test_native_route_vs_the_python_replace_patch_on_the_hooked_executor(fx, monkeypatch):
    eng = engine_of(fx["euler4"]["s0.5"]["config"])
    net = eng.forge_objects.unet.model.diffusion_model
    hooked = []
    real_hooked = net._attn_block_hooked
    monkeypatch.setattr(net, "_attn_block_hooked", lambda *a, **kw: (hooked.append(a[0]), real_hooked(*a, **kw))[1], raising=False)
    for strength in (0.5, 1.0):
        e4 = fx["euler4"][f"s{strength}"]
        del hooked[:]
        native = run_job(eng, e4, patch_stylealign(eng.forge_objects.unet, strength))
        assert hooked == []
        via_python = run_job(eng, e4, S.python_stylealign(eng.forge_objects.unet, strength))
        assert len(hooked) > 0
        check(f"tiny_stylealign 4-step Euler at strength {strength}: native vs the Python replace patch", native, via_python,
              floor=f"tiny_stylealign_unet.pt:euler4/s{strength}", both_fp16=True)


# ---- the plain path ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(S.PLAIN_FORWARDS)))
def test_plain_path_produces_the_bits_it_produced_before_the_option_existed(fx, i):
    want = fx["plain_bits"][i]
    got = S.plain_forward(i)
    assert got.shape == want.shape and got.dtype == want.dtype == H16
    assert torch.equal(bits(got), bits(want)), f"plain forward {S.PLAIN_FORWARDS[i]}: {int((bits(got) != bits(want)).sum())} of {got.numel()} values changed"
