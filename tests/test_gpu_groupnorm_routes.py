"""GPU (MI355X) kernel-level tests of the GroupNorm statistics chain, route by route: the per-(image, chunk, channel) {sum, sum of squares} records that
fmx_gemm_conv_stats leaves from the epilogue of every tile family (128-, 256- and 512-row tiles, with and without split-K) or from the pass behind the
GEMM, the stand-alone pass fmx_groupnorm_stats on every lane layout, and both folds of fmx_groupnorm_apply (inside the apply blocks; the separate
finalize launch) -- each against fp64 on the stored tensor, PER CHUNK, in fp16 and bf16.

Conventions (tests/test_gpu_gemm_windows.py, whose helpers this file imports): inputs come from the module-level builders below on the CPU with seeded
generators (tests/test_kernel_ref_teeth.py imports them and shows that each check rejects a planted bug), references from tests/kernel_refs.py in fp64
on the rounded inputs, cached.  Sentinel rule: every destination (output, record buffer, scale / shift workspace, GroupNorm output) is larger than what
the launch may write and pre-filled with a finite bit pattern that is never a result; afterwards everything outside the written part is bit-identical and
nothing inside it still holds the pattern.  Every input is a window of a buffer whose surroundings hold 30000.

Which route ran is asserted, not assumed: the chunk count a producer reports is compared with the rule of gemm_conv_one (csrc/fmx_gemm.hip) restated in
`expected_chunks`; the fold that fmx_groupnorm_apply took shows in the scale / shift workspace, which only the separate finalize writes.

Every test prints `MEASURED <part> <case>: <excess>` (pytest -s), the worst error in units of the tolerance; test_zz_report prints the worst per part and
the number of skipped cases (dispatcher refusals only, each matched by its FMX_REQUIRE text before the skip)."""
import math
import re
from functools import lru_cache

import pytest
import torch

pytestmark = pytest.mark.gpu

import forge_amd  # noqa: E402,F401
from forge_amd import _lib  # noqa: E402
from forge_amd import hipops as ops  # noqa: E402

import kernel_refs as R  # noqa: E402
from test_gpu_gemm_windows import SENTINEL, TILES, Win, bits, changed_outside, gen, rnd, sentinel_buffer  # noqa: E402
from test_gpu_vae_direct import STAT_TOL, Obj, f32_sentinel, tap_major  # noqa: E402

DEV = "cuda"
BF, H16 = torch.bfloat16, torch.float16
DTYPES = {"f16": H16, "bf16": BF}
WORST, SKIPPED = {}, []      # (part, type) -> worst excess seen; ids of the cases the dispatcher refused


def measured(part, dt, what, e):
    WORST[(part, dt)] = max(WORST.get((part, dt), 0.0), e)
    print(f"MEASURED {part} {what}: {e:.3f}")
    return e


def sfx(dtype):
    return "_bf16" if dtype == BF else "_f16"


def check_records(part, part_before, used, what):
    """the sentinel rule of a float32 destination: each of the first `used` floats was written, everything behind them is bit-identical to before"""
    p = part.cpu()
    left = int((bits(p[:used]) == SENTINEL[4]).sum())
    assert left == 0, f"{what}: {left} of the first {used} floats were never written"
    assert torch.equal(bits(p[used:]), bits(part_before[used:])), f"{what}: written beyond the first {used} floats"
    return p[:used]


# ---- 1. producer statistics: every tile id, the executors' forms ------------------------------------------------------------------------------------
N_IMG, CIN = 3, 128                  # an odd image count (tile -> image), 18 K-tiles for the 3x3 forms
NOUTS = (320, 136)                   # 136 is ragged on every tile width
PARTIAL_TAIL = 4096                  # floats behind what ops.stats_buffer would give
ROWS128, ROWS256, ROWS512 = (1, 2, 11, 12, 13), (6, 7), (9,)
# form -> geometry as a function of the output size (oh, ow): input size, stride, pad, upsample target, explicit output size
FORMS = {
    "a": lambda oh, ow: dict(ihw=(oh, ow), kh=3, stride=1, pad=1),                                    # bias + a row vector that is a column window of an [n, 3 nout] table
    "b": lambda oh, ow: dict(ihw=(oh, ow), kh=3, stride=1, pad=1),                                    # bias + residual
    "c": lambda oh, ow: dict(ihw=(2 * oh, 2 * ow), kh=3, stride=2, pad=1),                            # the UNet's Downsample
    "d": lambda oh, ow: dict(ihw=(oh // 2, ow // 2), kh=3, stride=1, pad=1, up=(oh, ow)),             # upsample on load
    "e": lambda oh, ow: dict(ihw=(oh, ow), kh=1, stride=1, pad=0),                                    # linear with n, h, w given + residual (proj_out)
    "f": lambda oh, ow: dict(ihw=(2 * oh, 2 * ow), kh=3, stride=2, pad=0, out_hw=(oh, ow)),           # the VAE encoder's Downsample (bf16 only)
}
# (form, nout, tall, type): per image 16 x 16, and form (a) at 32 x 16 so that the 512-row tile has a whole chunk
PRODUCER_CASES = [(f, nout, False, dt) for f in FORMS for nout in NOUTS for dt in sorted(DTYPES) if f != "f" or dt == "bf16"]
PRODUCER_CASES += [("a", nout, True, dt) for nout in NOUTS for dt in sorted(DTYPES)]


def expected_chunks(tile, n, hw):
    """records per image that a statistics launch on a forced tile id reports: the rule of gemm_conv_one (csrc/fmx_gemm.hip) -- hw / 128 for the 128-row
    tiles, hw / 256 for the 256 x 256 and 256 x 320 tiles, hw / 512 for the 512-row tile, each only when it divides hw, and the count of the pass behind the
    GEMM for everything else.  -> the list of legal counts: one entry for a forced tile; at the dispatcher's own choice (id 0) any tile may run"""
    fallback = ops._gn_chunks(n, hw)
    table = {t: fallback for t in TILES if t != 0}
    for ids, rows in ((ROWS128, 128), (ROWS256, 256), (ROWS512, 512)):
        if hw % rows == 0:
            table.update({t: hw // rows for t in ids})
    assert all(v <= ops._stats_geometry(n, hw)[1] for v in table.values())      # the capacity conv_gemm hands over never forces the fallback here
    return sorted(set(table.values())) if tile == 0 else [table[tile]]


@lru_cache(maxsize=None)
def producer_case(form, dtype, nout, tall=False):
    oh, ow = (32, 16) if tall else (16, 16)
    geo = FORMS[form](oh, ow)
    ih, iw = geo["ihw"]
    kh, n = geo["kh"], N_IMG
    m = n * oh * ow
    seed = 9000 + 100 * sorted(FORMS).index(form) + nout + (7 if tall else 0)
    wt = rnd(nout, CIN, kh, kh, scale=1 / math.sqrt(CIN * kh * kh), seed=seed + 1, dtype=dtype)
    k = Obj(form=form, n=n, oh=oh, ow=ow, hw=oh * ow, m=m, nout=nout, kh=kh, ih=ih, iw=iw, stride=geo["stride"], pad=geo["pad"], up=geo.get("up"),
            out_hw=geo.get("out_hw"), wt=wt, x=Win(rnd(n * ih * iw, CIN, seed=seed, dtype=dtype), 8, 8, 32, 32), wk=Win(tap_major(wt), 1, 2),
            bias=Win(rnd(nout, scale=0.5, seed=seed + 2, dtype=dtype), left=8, right=8), rowvec=None, residual=None)
    if form == "a":
        k.rowvec = Win(rnd(n, nout, scale=0.5, seed=seed + 3, dtype=dtype), 0, 0, nout, nout)
    if form in ("b", "e"):
        k.residual = Win(rnd(m, nout, seed=seed + 4, dtype=dtype), 3, 2, 8, 16)
    return k


@lru_cache(maxsize=None)
def producer_ref(form, dtype, nout, tall=False):
    """fp64 output [M, nout] of a producer case"""
    k = producer_case(form, dtype, nout, tall)
    val = lambda w: None if w is None else w.values  # noqa: E731
    x4 = k.x.values.reshape(k.n, k.ih, k.iw, CIN)
    if k.out_hw is not None:     # F.pad(x, (0, 1, 0, 1)) then stride 2, pad 0
        y = R.conv_ref(x4, k.wt, k.bias.values, stride=2, pad_rb=(1, 1))
    else:
        y = R.conv_ref(x4, k.wt, k.bias.values, stride=k.stride, pad=k.pad, up=k.up, rowvec=val(k.rowvec), residual=val(k.residual))
    assert y.shape[1:3] == (k.oh, k.ow)
    return y.reshape(k.m, nout)


def refusal(k, tile):
    """the FMX_REQUIRE text (csrc/fmx_gemm.hip, gemm_conv_one) with which the dispatcher refuses a statistics launch of this case on a forced tile, or None"""
    if tile == 10:
        return "gemm: the 256x160 two-workgroup tile takes plain linear GEMMs (one source, no output statistics"
    if tile == 9 and k.up is not None:
        return "gemm: the 512x128 tile takes no GEGLU, second source or upsample-on-load"
    return None


OUT_ABOVE = OUT_BELOW = 8


def out_buffer(k, dtype):
    return sentinel_buffer(OUT_ABOVE + k.m + OUT_BELOW, k.nout, dtype), slice(OUT_ABOVE, OUT_ABOVE + k.m)


def launch_producer(k, dtype, tile, stats):
    """one conv_gemm launch into a given sentinel buffer -> (the whole output buffer, GnStats or None, the record buffer, the record buffer before (CPU))"""
    buf, rows = out_buffer(k, dtype)
    dbuf = buf.to(DEV)
    on = lambda w: None if w is None else w.on(DEV)  # noqa: E731
    x = k.x.on(DEV)
    if k.kh == 3:
        x, geo = x.view(k.n, k.ih, k.iw, CIN), {}
    else:
        geo = dict(n=k.n, h=k.oh, w=k.ow)
    kw = dict(kh=k.kh, stride=k.stride, pad=k.pad, up=k.up, out_hw=k.out_hw, bias=on(k.bias), rowvec=on(k.rowvec), residual=on(k.residual), out=dbuf[rows],
              ld_out=k.nout, force_tile=tile, **geo)
    st = part = part_before = None
    if stats:
        part_before = f32_sentinel(ops.stats_buffer(k.n, k.hw, k.nout).numel() + PARTIAL_TAIL)
        part = part_before.to(DEV)
        _, st = ops.conv_gemm(x, k.wk.on(DEV), k.nout, stats=True, stats_partial=part, **kw)
    else:
        ops.conv_gemm(x, k.wk.on(DEV), k.nout, **kw)
    torch.cuda.synchronize()
    return dbuf, st, part, part_before


def check_producer(form, nout, tall, dt, tile, what, chunks=None):
    """one statistics launch and the same launch without statistics -> (output buffer, record buffer), both on the CPU, after the checks of part 1"""
    dtype = DTYPES[dt]
    k = producer_case(form, dtype, nout, tall)
    dbuf, st, part, part_before = launch_producer(k, dtype, tile, True)
    legal = chunks if chunks is not None else expected_chunks(tile, k.n, k.hw)
    assert st is not None and st.nchunks in legal, f"{what}: {st.nchunks} records per image, the route of tile id {tile} gives {legal}"
    plain = launch_producer(k, dtype, tile, False)[0].cpu()
    before, rows = out_buffer(k, dtype)
    got = dbuf.cpu()
    nbad = changed_outside(before, got, rows, slice(None))
    assert nbad == 0, f"{what}: {nbad} elements outside the output rows changed"
    out, pl = got[rows], plain[rows]
    if not torch.equal(bits(out), bits(pl)):     # the rule of test_gemm_output_statistics: at most one ulp apart, in at most a handful of elements
        d = (out.double() - pl.double()).abs()
        assert bool((d <= R.ulp(pl.double(), dtype)).all()) and int((d > 0).sum()) <= max(2, d.numel() // 100000), \
            f"{what}: {int((d > 0).sum())} of {d.numel()} elements differ from the launch without statistics, max {float(d.max()):.4g}"
    e = measured("producer output", dt, what, R.excess(out, producer_ref(form, dtype, nout, tall), dtype, *R.CONV_TOL[dtype]))
    assert e <= 1.0, f"{what}: the stored output is {e:.3g}x CONV_TOL from fp64"
    used = k.n * st.nchunks * nout * 2
    rec = check_records(part, part_before, used, what).view(k.n, st.nchunks, nout, 2)
    e = measured("producer records", dt, what, R.stat_excess(rec, R.chunk_sums_ref(out, k.n, st.nchunks), **STAT_TOL))
    assert e <= 1.0, f"{what}: a per-chunk record is {e:.3g}x the statistics tolerance from the fp64 sum over its rows of the stored output"
    return got, part.cpu()


def case_id(form, nout, tall, dt):
    return f"{form}-{nout}{'-32x16' if tall else ''}-{dt}"


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("form,nout,tall,dt", PRODUCER_CASES, ids=[case_id(*c) for c in PRODUCER_CASES])
def test_producer_statistics(form, nout, tall, dt, tile):
    """fmx_gemm_conv_stats on every tile id in the forms the executors launch: the chunk count is the one the tile's route gives (`expected_chunks`: that is
    the route check), the stored output equals the launch without statistics and is within CONV_TOL of fp64, every per-chunk record is the fp64 sum over that
    chunk's rows of the stored output within STAT_TOL, and exactly n * nchunks * nout * 2 floats of the record buffer were written."""
    what = f"{case_id(form, nout, tall, dt)} tile {tile}"
    k = producer_case(form, DTYPES[dt], nout, tall)
    why = refusal(k, tile)
    if why is not None:
        with pytest.raises(_lib.FmxError, match=re.escape(why)):
            launch_producer(k, DTYPES[dt], tile, True)
        SKIPPED.append(what)
        pytest.skip(f"the dispatcher refuses tile {tile} here: {why}")
    check_producer(form, nout, tall, dt, tile, what)


# ---- 2. split-K with statistics ----------------------------------------------------------------------------------------------------------------------
SPLITK_CASES = [(f, nout, dt) for f in "abc" for nout in NOUTS for dt in sorted(DTYPES)]


@pytest.mark.parametrize("splits", [2, 3])
@pytest.mark.parametrize("tile", [1, 2, 11, 13])
@pytest.mark.parametrize("form,nout,dt", SPLITK_CASES, ids=[case_id(f, nout, False, dt) for f, nout, dt in SPLITK_CASES])
def test_split_k_with_statistics(form, nout, dt, tile, splits, monkeypatch):
    """The last-arriving workgroup of a split-K tile sums the slots and runs the statistics epilogue (forced through FMX_GEMM_SPLITK, as
    test_split_k_matches_and_is_deterministic does): the checks of part 1 with hw / 128 records per image, the launch went through the workspace, output and
    records are bit-identical over three launches, the arrival counters are left zero, and an unsplit launch afterwards is correct."""
    what = f"split-K x{splits} {case_id(form, nout, False, dt)} tile {tile}"
    k = producer_case(form, DTYPES[dt], nout)
    monkeypatch.setenv("FMX_ALLOW_KNOBS", "1")
    monkeypatch.setenv("FMX_GEMM_SPLITK", str(splits))
    ws = ops.splitk_workspace(torch.device(DEV, torch.cuda.current_device()))
    ws[65536:65536 + (1 << 20)].zero_()
    out1, rec1 = check_producer(form, nout, False, dt, tile, what, chunks=[k.hw // 128])
    assert bool(ws[65536:65536 + (1 << 20)].any()), f"{what}: the launch did not go through the split-K workspace"
    assert not bool(ws[:65536].any()), f"{what}: arrival counters not left zero"
    for i in (2, 3):
        dbuf, st, part, _ = launch_producer(k, DTYPES[dt], tile, True)
        assert st.nchunks == k.hw // 128
        assert torch.equal(bits(dbuf.cpu()), bits(out1)), f"{what}: launch {i} stored other output bits than launch 1"
        assert torch.equal(bits(part.cpu()), bits(rec1)), f"{what}: launch {i} left other record bits than launch 1"
    assert not bool(ws[:65536].any()), f"{what}: arrival counters not left zero after three launches"
    monkeypatch.setenv("FMX_GEMM_SPLITK", "0")
    ws[65536:65536 + (1 << 20)].zero_()
    check_producer(form, nout, False, dt, tile, what + ", unsplit afterwards", chunks=[k.hw // 128])
    assert not bool(ws[65536:65536 + (1 << 20)].any()), f"{what}: FMX_GEMM_SPLITK=0 still split"


# ---- 3. the stand-alone statistics pass ----------------------------------------------------------------------------------------------------------------
# c: one octet with 256 pixel lanes; 40 octets (6 lanes, 16 idle threads); 256 octets (one lane each); 320 octets (a second octet block)
STATS_C, STATS_HW, STATS_N = (8, 320, 2048, 2560), (1, 35, 256), 2
STATS_CASES = [(c, hw, nch) for c in STATS_C for hw in STATS_HW for nch in (1, 7, hw + 5, 1024)]


@lru_cache(maxsize=None)
def stats_case(c, hw, dtype):
    """[n * hw, c] with a mean per channel, as a window with pixel stride c + 24"""
    g = gen(12000 + c + hw)
    return Win((torch.randn(STATS_N * hw, c, generator=g) + 0.5 * torch.randn(c, generator=g)).to(dtype), 2, 3, 8, 16)


def run_stats(x, n, hw, nchunks, dtype, tail=64):
    """fmx_groupnorm_stats on the device window x [n * hw, c] -> (record buffer with `tail` sentinel floats behind the records, the buffer before (CPU))"""
    c = x.shape[1]
    before = f32_sentinel(n * nchunks * c * 2 + tail)
    part = before.to(DEV)
    name = "fmx_groupnorm_stats" + sfx(dtype)
    _lib.check(getattr(_lib.lib(), name)(x.data_ptr(), c, x.stride(0), n, hw, part.data_ptr(), nchunks, ops.stream_ptr()), name)
    torch.cuda.synchronize()
    return part, before


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("c,hw,nchunks", STATS_CASES)
def test_groupnorm_stats_pass(c, hw, nchunks, dt):
    """fmx_groupnorm_stats called directly (the wrapper fixes nchunks) on every lane layout of gn_stats_kernel, with one chunk, ragged chunks, more chunks
    than pixels and the largest count: every record within STAT_TOL of the fp64 sum over its chunk's pixels, chunks behind the image exactly {0, 0}, and
    exactly n * nchunks * c * 2 floats written."""
    dtype = DTYPES[dt]
    what = f"c {c} hw {hw} nchunks {nchunks} {dt}"
    xw = stats_case(c, hw, dtype)
    x = xw.on(DEV)
    assert x.stride(0) == c + 24 and x.data_ptr() % 16 == 0
    part, before = run_stats(x, STATS_N, hw, nchunks, dtype)
    rec = check_records(part, before, STATS_N * nchunks * c * 2, what).view(STATS_N, nchunks, c, 2)
    per = -(-hw // nchunks)
    first_empty = -(-hw // per)
    assert not bool(rec[:, first_empty:].any()), f"{what}: a chunk behind the image is not exactly zero"
    e = measured("stand-alone pass records", dt, what, R.stat_excess(rec, R.chunk_sums_ref(xw.values, STATS_N, nchunks), **STAT_TOL))
    assert e <= 1.0, f"{what}: a per-chunk record is {e:.3g}x the statistics tolerance from the fp64 sum over its pixels"


# ---- 4. apply, both folds ------------------------------------------------------------------------------------------------------------------------------
APPLY_N = 2
# fused = the fold inside gn_apply_kernel (32 groups, <= 12 288 records, <= 1024 blocks); hws: one pixel, and counts that are no multiple of the block's pixels
# (ceil(8192 / C): 9, 4, 4, 22) -- the record-count case also at the 8 x 8 level's 64
APPLY_CASES = {
    "fused_straddle": dict(c0=320, c1=640, nch0=2, nch1=1, groups=32, hws=(1, 35), fused=True),            # 30 channels per group: group 10 straddles the sources
    "fused_wide": dict(c0=2560, c1=0, nch0=3, nch1=0, groups=32, hws=(1, 35), fused=True),                 # 320 octets per pixel > 256 threads
    "separate_records": dict(c0=1280, c1=1280, nch0=8, nch1=8, groups=32, hws=(1, 64, 67), fused=False),   # 20 480 records
    "separate_groups": dict(c0=256, c1=128, nch0=2, nch1=3, groups=16, hws=(1, 35), fused=False),          # 24 channels per group: group 10 straddles
}
APPLY_IDS = [(name, hw) for name, cfg in APPLY_CASES.items() for hw in cfg["hws"]]


def apply_fuses(cfg, n, hw):
    """the launcher's rule (csrc/fmx_norm.hip, fmx_groupnorm_apply_f16) restated"""
    c = cfg["c0"] + cfg["c1"]
    ppb = max(1, -(-8192 // c))
    return cfg["groups"] == 32 and cfg["c0"] * cfg["nch0"] + cfg["c1"] * cfg["nch1"] <= 12288 and n * -(-hw // ppb) <= 1024


@lru_cache(maxsize=None)
def apply_case(name, hw, dtype):
    """the gn_conv_inputs construction (tests/test_gpu_kernels_bf16.py): channel-group standard deviations from 3e-3 to 1, so that eps is visible in the small
    groups; the two channels either side of the source boundary carry +- 4 group standard deviations, so that a fold which loses or misplaces one of them moves
    its group's mean and variance by far more than a bf16 ulp.  Sources are windows with pixel strides c0 + 24 and c1 + 40."""
    cfg = APPLY_CASES[name]
    c0, c1, groups = cfg["c0"], cfg["c1"], cfg["groups"]
    c, n = c0 + c1, APPLY_N
    g = gen(13000 + c + 7 * hw + groups)
    gscale = torch.logspace(math.log10(3e-3), 0, groups).repeat_interleave(c // groups)
    x = torch.randn(n * hw, c, generator=g) * gscale + 0.3 * gscale * torch.randn(c, generator=g)
    if c1:
        x[:, c0 - 1] += 4 * gscale[c0 - 1]
        x[:, c0] -= 4 * gscale[c0]
    x = x.to(dtype)
    gamma, beta = (1 + 0.1 * torch.randn(c, generator=g)).to(dtype), (0.1 * torch.randn(c, generator=g)).to(dtype)
    return Obj(cfg=cfg, n=n, hw=hw, c=c, x=x, x0=Win(x[:, :c0].contiguous(), 2, 3, 8, 16), x1=Win(x[:, c0:].contiguous(), 3, 2, 16, 24) if c1 else None,
               gamma=Win(gamma, left=8, right=8), beta=Win(beta, left=8, right=8))


def apply_sources(k):
    """-> ([x0 [n, hw, c0]] or [x0, x1], their chunk counts): what kernel_refs.gn_fold_emul2 takes"""
    srcs = [k.x[:, :k.cfg["c0"]].reshape(k.n, k.hw, -1)] + ([k.x[:, k.cfg["c0"]:].reshape(k.n, k.hw, -1)] if k.cfg["c1"] else [])
    return srcs, [k.cfg["nch0"], k.cfg["nch1"]][:len(srcs)]


@lru_cache(maxsize=None)
def apply_ref(name, hw, dtype, eps, silu):
    k = apply_case(name, hw, dtype)
    return R.groupnorm_ref(k.x.view(k.n, k.hw, 1, k.c), k.gamma.values, k.beta.values, R.f32(eps), groups=k.cfg["groups"], silu=silu).reshape(k.n * k.hw, k.c)


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("name,hw", APPLY_IDS)
def test_groupnorm_apply_folds(name, hw, silu, eps, dt):
    """fmx_groupnorm_apply called directly on statistics from fmx_groupnorm_stats with the case's chunk counts (two sources: different counts), a sentinel-filled
    scale / shift workspace and sentinel rows around y.  The fused fold never writes the workspace and the separate finalize writes exactly n * C * 2 floats of it:
    that is how the fold that ran is asserted.  Output within GN_TOL of fp64 GroupNorm of the sources; the record buffers bit-unchanged; the separate fold's table
    within kernel_refs.GN_TABLE_TOL of fp64 {rstd gamma, beta - mean rstd gamma}."""
    dtype = DTYPES[dt]
    what = f"{name} hw {hw} silu {silu} eps {eps} {dt}"
    k = apply_case(name, hw, dtype)
    cfg, n, c = k.cfg, k.n, k.c
    c0, c1, groups = cfg["c0"], cfg["c1"], cfg["groups"]
    assert apply_fuses(cfg, n, hw) == cfg["fused"]
    x0 = k.x0.on(DEV)
    x1 = k.x1.on(DEV) if c1 else None
    assert x0.stride(0) == c0 + 24 and (x1 is None or x1.stride(0) == c1 + 40)
    p0, p0_before = run_stats(x0, n, hw, cfg["nch0"], dtype)
    p1, p1_before = run_stats(x1, n, hw, cfg["nch1"], dtype) if c1 else (None, None)
    p0_snap, p1_snap = p0.clone(), p1.clone() if c1 else None
    ybuf_before = sentinel_buffer(3 + n * hw + 5, c, dtype)
    rows = slice(3, 3 + n * hw)
    ybuf = ybuf_before.to(DEV)
    ss_before = f32_sentinel(n * c * 2 + 64)
    ss = ss_before.to(DEV)
    gamma, beta = k.gamma.on(DEV), k.beta.on(DEV)
    fn = "fmx_groupnorm_apply" + sfx(dtype)
    _lib.check(getattr(_lib.lib(), fn)(x0.data_ptr(), x1.data_ptr() if c1 else None, c0, c1, x0.stride(0), x1.stride(0) if c1 else 0, n, hw, p0.data_ptr(), cfg["nch0"],
                                       p1.data_ptr() if c1 else None, cfg["nch1"], groups, float(eps), gamma.data_ptr(), beta.data_ptr(), 1 if silu else 0,
                                       ss.data_ptr(), ybuf[rows].data_ptr(), ops.stream_ptr()), fn)
    torch.cuda.synchronize()
    got = ybuf.cpu()
    nbad = changed_outside(ybuf_before, got, rows, slice(None))
    assert nbad == 0, f"{what}: {nbad} elements outside y changed"
    assert torch.equal(bits(p0), bits(p0_snap)) and (not c1 or torch.equal(bits(p1), bits(p1_snap))), f"{what}: apply changed a record buffer"
    if cfg["fused"]:
        assert torch.equal(bits(ss.cpu()), bits(ss_before)), f"{what}: the scale / shift workspace was written: the separate finalize ran where the fused fold should"
    else:
        table = check_records(ss, ss_before, n * c * 2, what + " scale / shift workspace (the separate finalize should have run)").view(n, c, 2)
        e = measured("scale/shift table", dt, what, R.gn_table_excess(table, k.x.view(n, hw, c), k.gamma.values, k.beta.values, R.f32(eps), groups))
        assert e <= 1.0, f"{what}: the scale / shift table is {e:.3g}x GN_TABLE_TOL from fp64"
    e = measured("GroupNorm output, " + ("fused fold" if cfg["fused"] else "separate fold"), dt, what,
                 R.excess(got[rows], apply_ref(name, hw, dtype, eps, silu), dtype, *R.GN_TOL[dtype]))
    assert e <= 1.0, f"{what}: the output is {e:.3g}x GN_TOL from fp64 GroupNorm"


def test_zz_report():
    """prints the worst excess per part and element type seen above, and the number of skipped cases (visible with -s): the figures recorded in kernel_refs.py"""
    for (part, dt), e in sorted(WORST.items()):
        print(f"MEASURED worst {part} {dt}: {e:.3f}")
    print(f"SKIPPED {len(SKIPPED)} cases, every one a dispatcher refusal matched by its FMX_REQUIRE text")
    assert all(e <= 1.0 for e in WORST.values())
