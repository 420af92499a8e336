"""Dynamic Thresholding restated in torch (shared by tests/test_dynthresh_host.py, tests/test_gpu_dynthresh.py and
tools/make_dynthresh_fixtures.py).

`dynthresh_ref` is steps 2-6 of the reference's DynThresh.dynthresh (conds_per_batch 1, no weights, experiment_mode 0) in the dtype asked
for -- fp64 on the fp32 inputs is the yardstick of the kernels; tests/test_dynthresh_host.py pins it to the real reference's outputs
(tests/golden/dynthresh_ops.pt).  `quantile_restated` is the order-statistic form of torch.quantile that csrc/fmx_dynthresh.hip selects.
`dynthresh_kernel_order_f32` restates what the kernels compute in fp32 with their summation order: per-thread strided sums, an xor butterfly
inside a wave, the waves in order, the chunks in order.  The kernels round every operation once, as torch's CPU operators do, so this is
the GPU's result up to the device's division and square root."""
import torch

CHUNK = 2048      # FMX_DYNTHRESH_CHUNK
TPB = 256         # threads of the partial-sum pass
SEL_TPB = 1024    # threads of the reference pass
WAVE = 64


def case_inputs(case):
    """the seeded inputs of a dynthresh_ops.pt case: cond / uncond as two correlated N(0, 1) latents with per-row offsets.  `const_row`:
    row (0, 1) of both is the constant 0.5 (every sum of it is exact, so the row is degenerate in fp32 as in fp64)."""
    b, c, hh, ww = case["shape"]
    g = torch.Generator().manual_seed(case["seed"])
    uncond = torch.randn(b, c, hh, ww, generator=g) + 0.3 * torch.randn(b, c, 1, 1, generator=g)
    cond = uncond + 0.25 * torch.randn(b, c, hh, ww, generator=g) + 0.05 * torch.randn(b, c, 1, 1, generator=g)
    if case.get("const_row"):
        cond[0, 1] = 0.5
        uncond[0, 1] = 0.5
    if "checksum" in case:
        got = (float(cond.double().sum()), float(uncond.double().sum()))
        assert got == tuple(case["checksum"]), f"torch's seeded generator gave other inputs than the fixture was made with: {got} vs {case['checksum']}"
    return cond, uncond


def quantile_restated(values, q):
    """values: 1-D fp32 -> 0-dim fp32: sort; pos = float32(q) * (N - 1) in fp32; lerp(v[floor pos], v[ceil pos], pos - floor pos)"""
    v = values.sort().values
    pos = torch.tensor(q, dtype=torch.float32) * (v.numel() - 1)
    lo, hi = pos.floor(), pos.ceil()
    return torch.lerp(v[int(lo)], v[int(hi)], pos - lo)


def dynthresh_ref(cond, uncond, mimic, cfg, percentile, separate, startpoint, variability, phi, dtype=torch.float64):
    cond, uncond = cond.to(dtype), uncond.to(dtype)
    rel = cond - uncond
    mim_t, cfg_t = uncond + rel * mimic, uncond + rel * cfg
    mim_f, cfg_f = mim_t.flatten(2), cfg_t.flatten(2)
    mim_mean, cfg_mean = mim_f.mean(dim=2, keepdim=True), cfg_f.mean(dim=2, keepdim=True)
    mim_c, cfg_c = mim_f - mim_mean, cfg_f - cfg_mean
    if variability == "STD":
        mim_ref, cfg_ref = (mim_c.std(dim=2, keepdim=True), cfg_c.std(dim=2, keepdim=True)) if separate else (mim_c.std(), cfg_c.std())
    elif separate:
        mim_ref, cfg_ref = mim_c.abs().amax(dim=2, keepdim=True), torch.quantile(cfg_c.abs(), percentile, dim=2, keepdim=True)
    else:
        mim_ref, cfg_ref = mim_c.abs().max(), torch.quantile(cfg_c.abs(), percentile)
    if startpoint == "ZERO":
        res = cfg_f * (mim_ref / cfg_ref)
    elif variability == "STD":
        res = cfg_c / cfg_ref * mim_ref + cfg_mean
    else:
        m = torch.maximum(mim_ref, cfg_ref)
        res = torch.minimum(torch.maximum(cfg_c, -m), m) / m * mim_ref + cfg_mean
    res = res.unflatten(2, cond.shape[2:])
    if phi != 1.0:
        res = res * phi + cfg_t * (1.0 - phi)
    return res


def _butterfly(v):
    """v [..., 64] -> [...]: the xor butterfly of wave_sum (offsets 32, 16, ... 1); every lane ends with the same value"""
    idx = torch.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ o]
    return v[..., 0]


def block_sum(rows, threads):
    """the workgroup sum of the kernels over a list of 1-D fp32 rows: thread t adds row[t], row[t + threads], ... of every row in turn,
    then the butterfly per wave, then the waves in order"""
    acc = torch.zeros(threads, dtype=torch.float32)
    for r in rows:
        pad = (-r.numel()) % threads
        r = torch.cat([r, torch.zeros(pad, dtype=torch.float32)]).view(-1, threads)
        for it in range(r.shape[0]):
            acc = acc + r[it]
    waves = _butterfly(acc.view(-1, WAVE))
    t = waves[0]
    for k in range(1, waves.numel()):
        t = t + waves[k]
    return t


def row_mean_kernel_order(row):
    """one row's mean as the partial-sum pass and the reference pass form it"""
    t = torch.zeros((), dtype=torch.float32)
    for s in range(0, row.numel(), CHUNK):
        t = t + block_sum([row[s:s + CHUNK]], TPB)
    return t / torch.tensor(float(row.numel()), dtype=torch.float32)


def dynthresh_kernel_order_f32(cond, uncond, mimic, cfg, percentile, separate, startpoint, variability, phi):
    f32 = torch.float32
    cond, uncond = cond.to(f32), uncond.to(f32)
    b, c = cond.shape[:2]
    mimic, cfg = torch.tensor(mimic, dtype=f32), torch.tensor(cfg, dtype=f32)
    rel = cond - uncond
    mim_f, cfg_f = (uncond + rel * mimic).reshape(b * c, -1), (uncond + rel * cfg).reshape(b * c, -1)
    rows, hw = mim_f.shape
    mim_mean = torch.stack([row_mean_kernel_order(r) for r in mim_f]).view(rows, 1)
    cfg_mean = torch.stack([row_mean_kernel_order(r) for r in cfg_f]).view(rows, 1)
    mim_c, cfg_c = mim_f - mim_mean, cfg_f - cfg_mean
    groups = [[r] for r in range(rows)] if separate else [list(range(rows))]
    mim_ref, cfg_ref = torch.empty(rows, 1), torch.empty(rows, 1)
    for grp in groups:
        if variability == "STD":
            count = torch.tensor(float(len(grp) * hw), dtype=f32)
            refs = []
            for cen in (mim_c, cfg_c):
                m2 = block_sum([cen[r] for r in grp], SEL_TPB) / count
                ss = block_sum([(cen[r] - m2) * (cen[r] - m2) for r in grp], SEL_TPB)
                refs.append((ss / (count - 1.0)).sqrt())
        else:
            refs = [mim_c[grp].abs().max(), quantile_restated(cfg_c[grp].abs().reshape(-1), percentile)]
        mim_ref[grp], cfg_ref[grp] = refs[0], refs[1]
    if startpoint == "ZERO":
        res = cfg_f * (mim_ref / cfg_ref)
    elif variability == "STD":
        res = cfg_c / cfg_ref * mim_ref + cfg_mean
    else:
        m = torch.maximum(mim_ref, cfg_ref)
        res = torch.minimum(torch.maximum(cfg_c, -m), m) / m * mim_ref + cfg_mean
    if phi != 1.0:
        res = res * torch.tensor(phi, dtype=f32) + cfg_f * torch.tensor(1.0 - phi, dtype=f32)
    return res.view(cond.shape)


def normalised_error(got, ref):
    """max |got - ref| / max |ref| over the positions where ref is finite; NaN positions must coincide"""
    got, ref = got.double().cpu(), ref.double().cpu()
    assert torch.equal(got.isnan(), ref.isnan()), "NaN positions differ"
    ok = ~ref.isnan()
    return float((got[ok] - ref[ok]).abs().max() / ref[ok].abs().max())


def sampler_cfg_function_for(params, predictor):
    """the reference's sampler_dyn_thresh restated with torch ops (dynthres.py:36-45): a Python sampler_cfg_function for
    UnetPatcher.set_model_sampler_cfg_function, the hooked twin of the native route in the GPU tests and in tools/bench_features.py"""
    from forge_amd.backend.patcher.dynthresh import MAX_STEPS, interpret_scale

    def sampler_dyn_thresh(args):
        x = args["input"]
        cond, uncond = x - args["cond"], x - args["uncond"]
        time_step = predictor.timestep(args["sigma"].detach().float().cpu())[0].item()   # the reference's device read
        step = MAX_STEPS - time_step
        mimic = interpret_scale(params.mimic_scale, params.mimic_mode, params.mimic_scale_min, step, params.sched_val)
        cfg = interpret_scale(args["cond_scale"], params.cfg_mode, params.cfg_scale_min, step, params.sched_val)
        res = dynthresh_ref(cond, uncond, mimic, cfg, params.threshold_percentile, params.separate_feature_channels == "enable",
                            params.scaling_startpoint, params.variability_measure, params.interpolate_phi, dtype=torch.float32)
        return x - res
    return sampler_dyn_thresh


# worst distance of dynthresh_kernel_order_f32 from the fp64 restatement over the cases of tests/golden/dynthresh_ops.pt, normalised by the
# case's largest |result|, as tests/test_dynthresh_host.py measures it; the GPU gate doubles it for what torch cannot restate (the device's
# division and square root)
KERNEL_ORDER_WORST = 1.0e-6   # measured 9.93e-7: the tensor-wide 0.999-quantile of 64 x 64 x 4 values, whose fp32 position is 2e-4 off the exact one
GPU_GATE = 2 * KERNEL_ORDER_WORST
