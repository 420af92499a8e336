"""GPU: native Dynamic Thresholding.  fmx_row_abs_quantile_f32 (through hipops.row_abs_quantile) bit for bit against torch.quantile on the
CPU; fmx_dynthresh_f32 (through hipops.dynthresh) against the fp64 restatement of tests/dynthresh_refs.py, which tests/test_dynthresh_host.py
pins to the real reference; and the option end to end on the tiny SD1.5 engine against the same engine with the restated function installed
as a Python sampler_cfg_function."""
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402

import forge_amd  # noqa: E402,F401
from forge_amd import hipops as ops  # noqa: E402
from forge_amd import synth  # noqa: E402
from forge_amd.backend.diffusion_engine.base import build_engine  # noqa: E402
from forge_amd.backend.patcher.dynthresh import patch_dynthresh  # noqa: E402
from forge_amd.modules import processing, prompt_parser as pp, shared  # noqa: E402
from oracle.make_golden import multicond_case  # noqa: E402

from conftest import load_golden  # noqa: E402
import dynthresh_refs as dr  # noqa: E402
import parity  # noqa: E402
from parity import check  # noqa: E402

DEV = "cuda"
QS = (0.0, 0.25, 0.5, 0.99, 0.999, 1.0)
# 1, 2, 5 x 7; around one wave; around a 1024-thread workgroup; two sizes of many strides; the first size past 160 KB of fp32
ROW_LENGTHS = (1, 2, 35, 63, 64, 65, 1023, 1056, 4096, 16384, 41600)
SHAPES = ((1, 4, 2, 2), (2, 4, 5, 7), (2, 16, 8, 8), (1, 4, 33, 31), (2, 4, 64, 64), (1, 4, 128, 128), (1, 4, 208, 200))
BRANCHES = [(sep, sp, var) for sep in (True, False) for sp in ("MEAN", "ZERO") for var in ("AD", "STD")]
PHI_PCT = ((1.0, 1.0), (0.7, 0.99))


def three_rows(n, seed):
    """Gaussian | Gaussian quantised to multiples of 0.25 (ties) | a row with one large outlier"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(3, n, generator=g)
    x[1] = (x[1] * 4).round() / 4
    x[2, n // 2] = 1e4
    return x


@pytest.mark.parametrize("n", ROW_LENGTHS)
def test_row_abs_quantile_is_torch_quantile_bit_for_bit(n):
    x = three_rows(n, n)
    center = torch.tensor([0.125, 0.25, -0.5]) if n < 4 else x.mean(dim=1)
    center[1] = 0.25                                         # keeps the quantised row's distances on the 0.25 grid: heavy ties
    ref_in = (x - center[:, None]).abs()
    gx, gc = x.to(DEV), center.to(DEV)
    for q in QS:
        got = ops.row_abs_quantile(gx, gc, q).cpu()
        ref = torch.quantile(ref_in, q, dim=1)
        assert torch.equal(got, ref), (n, q, got, ref)


@pytest.mark.parametrize("rows_per_group", [1, 8])
def test_row_abs_quantile_over_groups_of_rows(rows_per_group):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(8, 4096, generator=g)
    x[3] = (x[3] * 4).round() / 4
    center = x.mean(dim=1)
    ref_in = (x - center[:, None]).abs().view(8 // rows_per_group, -1)
    for q in QS:
        got = ops.row_abs_quantile(x.to(DEV), center.to(DEV), q, rows_per_group=rows_per_group).cpu()
        assert got.shape == (8 // rows_per_group,)
        assert torch.equal(got, torch.quantile(ref_in, q, dim=1)), (rows_per_group, q)


def test_row_abs_quantile_max_shortcut_returns_the_general_routes_bits():
    """q == 1 takes one max pass.  A row of 2^12 + 1 values whose largest value occurs twice: at q = 1 - 2^-12 the position is exactly N - 2,
    which the selection passes find -- the same value, so the same bits."""
    n = 4097
    x = three_rows(n, 11)
    center = x.mean(dim=1)
    d = (x - center[:, None]).abs()
    for r in range(3):
        x[r, 5] = x[r, int(d[r].argmax())]
    d = (x - center[:, None]).abs()
    top = d.sort(dim=1).values
    assert torch.equal(top[:, -1], top[:, -2])
    q = 1.0 - 2.0 ** -12
    assert float(torch.tensor(q, dtype=torch.float32) * (n - 1)) == n - 2
    general, shortcut = ops.row_abs_quantile(x.to(DEV), center.to(DEV), q).cpu(), ops.row_abs_quantile(x.to(DEV), center.to(DEV), 1.0).cpu()
    assert torch.equal(general, shortcut) and torch.equal(shortcut, top[:, -1]) and torch.equal(general, torch.quantile(d, q, dim=1))


def op_cases():
    cases = []
    for shape in (SHAPES[0], SHAPES[1], SHAPES[3]):          # the two smallest shapes and a mid-size one: every branch
        for br in BRANCHES:
            for phi, pct in PHI_PCT:
                cases.append((shape, br, phi, pct))
    for shape in SHAPES:                                      # the default branch on every shape
        for phi, pct in PHI_PCT + ((1.0, 0.99),):
            case = (shape, (True, "MEAN", "AD"), phi, pct)
            if case not in cases:
                cases.append(case)
    return cases


def test_dynthresh_vs_fp64_on_every_branch_and_shape():
    """max |kernel - fp64| / max |fp64| <= dr.GPU_GATE: twice what the kernels' summation order costs in fp32 on the host
    (tests/test_dynthresh_host.py), the factor for the device's division and square root; two runs give the same bits"""
    worst = 0.0
    for i, (shape, (sep, sp, var), phi, pct) in enumerate(op_cases()):
        cond, uncond = dr.case_inputs(dict(shape=shape, seed=500 + i))
        args = (7.0, 12.0, pct, sep, sp, var, phi)
        ref = dr.dynthresh_ref(cond, uncond, *args)
        gc, gu = cond.to(DEV), uncond.to(DEV)
        got = ops.dynthresh(gc, gu, *args)
        again = ops.dynthresh(gc, gu, *args, out=torch.empty_like(gc))
        assert torch.equal(got, again), (shape, sep, sp, var)
        assert torch.equal(gc.cpu(), cond) and torch.equal(gu.cpu(), uncond)
        err = dr.normalised_error(got, ref)
        print(shape, sep, sp, var, "phi", phi, "percentile", pct, "err", err)
        worst = max(worst, err)
        assert err <= dr.GPU_GATE, (shape, sep, sp, var, phi, pct, err)
    print("worst", worst, "gate", dr.GPU_GATE)


def test_dynthresh_percentile_one_equals_the_general_route():
    """rows of 17 x 241 = 2^12 + 1 values whose largest |centred cfg target| occurs twice: percentile 1 - 2^-12 selects rank N - 2 by the
    digit passes, percentile 1.0 takes the max pass -- one value, so every output bit agrees"""
    shape = (1, 4, 17, 241)
    cond, uncond = dr.case_inputs(dict(shape=shape, seed=77))
    for _ in range(2):   # moving a value moves the mean: repeat until the duplicate is the maximum of the final rows
        cfg_f = (uncond + (cond - uncond) * 12.0).flatten(2)
        am = (cfg_f - cfg_f.mean(dim=2, keepdim=True)).abs().argmax(dim=2)
        for r in range(4):
            j = int(am[0, r])
            k = (j + 1000) % 4097
            cond.view(1, 4, -1)[0, r, k], uncond.view(1, 4, -1)[0, r, k] = cond.view(1, 4, -1)[0, r, j], uncond.view(1, 4, -1)[0, r, j]
    cfg_f = (uncond + (cond - uncond) * 12.0).flatten(2)
    top = (cfg_f - cfg_f.mean(dim=2, keepdim=True)).abs().sort(dim=2).values
    assert torch.equal(top[..., -1], top[..., -2])
    gc, gu = cond.to(DEV), uncond.to(DEV)
    # per-row references only: the tensor-wide group has 4 * 4097 values, where 1 - 2^-12 is no whole rank
    a = ops.dynthresh(gc, gu, 7.0, 12.0, 1.0, True, "MEAN", "AD", 1.0)
    b = ops.dynthresh(gc, gu, 7.0, 12.0, 1.0 - 2.0 ** -12, True, "MEAN", "AD", 1.0)
    assert torch.equal(a, b)
    assert dr.normalised_error(a, dr.dynthresh_ref(cond, uncond, 7.0, 12.0, 1.0, True, "MEAN", "AD", 1.0)) <= dr.GPU_GATE


def test_dynthresh_constant_row_is_nan_where_the_reference_is():
    case = dict(shape=(2, 4, 5, 7), seed=321, const_row=True)
    cond, uncond = dr.case_inputs(case)
    for pct in (1.0, 0.5):
        ref = dr.dynthresh_ref(cond, uncond, 7.0, 12.0, pct, True, "MEAN", "AD", 1.0)
        got = ops.dynthresh(cond.to(DEV), uncond.to(DEV), 7.0, 12.0, pct, True, "MEAN", "AD", 1.0).cpu()
        assert ref[0, 1].isnan().all() and int(ref.isnan().sum()) == 35
        assert torch.equal(got.isnan(), ref.isnan())
        assert torch.allclose(got.double(), ref, rtol=0, atol=dr.GPU_GATE * float(ref[~ref.isnan()].abs().max()), equal_nan=True)


def test_dynthresh_wrapper_refuses_what_the_kernel_cannot_take():
    x = torch.zeros(1, 4, 8, 8, device=DEV)
    with pytest.raises(TypeError):
        ops.dynthresh(x.half(), x.half(), 7.0, 12.0, 1.0, True, "MEAN", "AD", 1.0)
    with pytest.raises(ValueError):
        ops.dynthresh(x, x[:, :2], 7.0, 12.0, 1.0, True, "MEAN", "AD", 1.0)
    with pytest.raises(forge_amd._lib.FmxError):
        ops.dynthresh(x, x.clone(), 7.0, 12.0, 1.0, True, "MEAN", "AD", 1.0, out=x)
    with pytest.raises(ValueError):
        ops.row_abs_quantile(x.view(4, 64), torch.zeros(4, device=DEV), 0.5, rows_per_group=3)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
CFG = synth.TINY_SD15_UNET_CONFIG
PARAMS = (7.0, 0.99, "Half Cosine Up", 0.0, "Linear Down", 0.0, 1.0, "enable", "MEAN", "AD", 1.0)
FLOOR = ["tiny_sd15_cfg_paths.pt:plain", "tiny_sd15_cfg_paths.pt:cfg_functions"]


@pytest.fixture(scope="module")
def engine():
    return build_engine(CFG, synth.synth_unet_state_dict(CFG, seed=0), None, None, device=DEV)


def run(eng, g, c, uc, unet=None):
    shared.opts.randn_source = "CPU"
    saved = eng.forge_objects_after_applying_lora
    if unet is not None:
        eng.forge_objects_after_applying_lora = saved.shallow_copy()
        eng.forge_objects_after_applying_lora.unet = unet
    try:
        p = processing.StableDiffusionProcessingTxt2Img(sd_model=eng, c=c, uc=uc, seed=g["seeds"][0], sampler_name="Euler", batch_size=len(g["seeds"]),
                                                        steps=4, cfg_scale=12.0, width=g["hw"] * 8, height=g["hw"] * 8, do_decode=False)
        return processing.process_images(p).latents.clone()
    finally:
        eng.forge_objects_after_applying_lora = saved
        eng.forge_objects = saved.shallow_copy()


def hooked_twin(eng):
    from forge_amd.backend.patcher.dynthresh import DynThreshParams
    unet = eng.forge_objects.unet.clone()
    unet.set_model_sampler_cfg_function(dr.sampler_cfg_function_for(DynThreshParams(True, *PARAMS), unet.model.predictor))
    return unet


def test_sampling_with_the_option_vs_the_function_installed_through_the_setter(engine, monkeypatch):
    """4-step Euler at CFG 12: the native option against the same engine with the restated sampler_dyn_thresh as a Python sampler_cfg_function
    (which takes the stacked general route); ops.dynthresh runs once per model call on the native route and never without the option; the
    plain route's latents do not change by the option having been used on the engine."""
    g = load_golden("tiny_sd15_cfg_paths.pt")
    c, uc = synth.synth_conditioning(len(g["seeds"]), CFG["context_dim"], None, seed=1234)
    c, uc = c.to(DEV), uc.to(DEV)
    calls = []
    real = ops.dynthresh
    monkeypatch.setattr(ops, "dynthresh", lambda *a, **k: (calls.append(a[0].shape), real(*a, **k))[1])
    before = run(engine, g, c, uc)                        # before patch_dynthresh was ever called on this engine
    assert calls == []
    native = run(engine, g, c, uc, patch_dynthresh(engine.forge_objects.unet, *PARAMS))
    assert len(calls) == 4 and all(tuple(s) == tuple(native.shape) for s in calls)
    assert "dynthresh" not in engine.forge_objects.unet.model_options
    hooked = run(engine, g, c, uc, hooked_twin(engine))
    assert len(calls) == 4
    check("tiny_sd15 4-step Euler CFG 12: native Dynamic Thresholding vs the function through set_model_sampler_cfg_function", native, hooked,
          floor=FLOOR, both_fp16=True)
    gate = parity.limits(FLOOR, both_fp16=True)[1]["max_rel"]
    moved = parity.max_rel(native, before)
    print("native vs plain CFG 12:", moved, "gate", gate)
    assert moved > gate
    after = run(engine, g, c, uc)
    assert len(calls) == 4 and torch.equal(after, before)


def test_and_composed_prompt_with_the_option_vs_its_hooked_twin(engine):
    """the general route (several conds with strengths, one stacked model call) hands its two predictions to the same op"""
    g = load_golden("tiny_sd15_cfg_paths.pt")
    c4, uc, comp = multicond_case(CFG)
    c4, uc = c4.to(DEV), uc.to(DEV)
    multicond = pp.MulticondLearnedConditioning((2,), [[pp.ComposableScheduledPromptConditioning([pp.ScheduledPromptConditioning(4, c4[i])], w)
                                                        for i, w in parts] for parts in comp])
    native = run(engine, g, multicond, uc, patch_dynthresh(engine.forge_objects.unet, *PARAMS))
    hooked = run(engine, g, multicond, uc, hooked_twin(engine))
    check("tiny_sd15 AND-composed prompt, 4-step Euler CFG 12: native Dynamic Thresholding vs its hooked twin", native, hooked,
          floor="tiny_sd15_cfg_paths.pt:and_composed", both_fp16=True)
    assert parity.max_rel(native, run(engine, g, multicond, uc)) > parity.limits("tiny_sd15_cfg_paths.pt:and_composed", both_fp16=True)[1]["max_rel"]
