"""GPU (MI355X) kernel-level tests of the VAE decoder's direct kernels -- fmx_conv3x3_gn_silu, fmx_conv3x3_narrow, fmx_conv3x3_narrow_gn_silu,
fmx_conv3x3_up2x, fmx_attention_single_head512 (both element types) -- against fp64 at the smallest shapes that cross every tile and chunk
boundary.  The executors run these kernels on large tensors only, so no small end-to-end fixture reaches them.

Conventions (tests/test_gpu_gemm_windows.py, whose helpers this file imports): inputs come from the module-level builders below on the CPU with seeded
generators (tests/test_kernel_ref_teeth.py imports them and shows that each check rejects a planted bug), references from tests/kernel_refs.py in
fp64 on the rounded inputs, cached.  Sentinel rule: every destination is larger than what the launch may write and pre-filled with a finite bit
pattern; afterwards everything outside the written window is bit-identical.  Every input is a window of a buffer whose surroundings hold 30000,
where the contract allows a stride (the activations of the convolutions are contiguous by contract: they are ROW windows, so image 0's top border
and the last image's bottom border have 30000 next to them in memory where the kernel must see zeros).

GroupNorm-fused cases use `teeth_x`: every (image, group) has a mean and a standard deviation of its own, so the table of another image or another
group is far outside the tolerance (identically distributed groups would hide it in the sampling noise of the statistics)."""
import math
from functools import lru_cache

import pytest
import torch

pytestmark = pytest.mark.gpu

import forge_amd  # noqa: E402,F401
from forge_amd import hipops as ops  # noqa: E402

import kernel_refs as R  # noqa: E402
from test_gpu_gemm_windows import BIG, SENTINEL, Win, bits, changed_outside, gen, rnd, sentinel_buffer  # noqa: E402

DEV = "cuda"
BF, H16 = torch.bfloat16, torch.float16
DTYPES = {"f16": H16, "bf16": BF}
EPS_GN = 1e-6
STAT_TOL = dict(rtol=2e-5, atol=2e-3)


def teeth_x(n, h, w, c, groups, dtype, seed):
    """NHWC activations whose (image, group) means lie in [-2, 2] and standard deviations in [0.05, 2] (log scale), permuted differently per image;
    |mean| <= 8 std, far inside the ratio of 100 that test_gpu_kernels_bf16.OFFSET_LIMIT asserts"""
    g = gen(seed)
    std = torch.logspace(math.log10(0.05), math.log10(2.0), groups)
    mean = torch.linspace(-2.0, 2.0, groups)
    imgs = []
    for _ in range(n):
        s = std[torch.randperm(groups, generator=g)]
        m = torch.maximum(torch.minimum(mean[torch.randperm(groups, generator=g)], 8 * s), -8 * s)
        imgs.append(torch.randn(h, w, c, generator=g) * s.repeat_interleave(c // groups) + m.repeat_interleave(c // groups))
    return torch.stack(imgs).to(dtype)


def tap_major(wt):
    """torch's [co, ci, 3, 3] -> the kernels' [co, (ky, kx, ci)]"""
    return wt.permute(0, 2, 3, 1).reshape(wt.shape[0], -1).contiguous()


class Obj:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def f32_sentinel(numel):
    return torch.full((numel,), SENTINEL[4], dtype=torch.int32).view(torch.float32)


def check_stats(st, part_before, part, out, n, nch, c, what):
    """records of the STORED output: nch per image, fp64 sums per image (pixels outside the image do not count, images do not mix), tail untouched"""
    assert st.nchunks == nch, f"{what}: {st.nchunks} statistics records per image, expected {nch}"
    used = n * nch * c * 2
    got = part.cpu()[:used].view(n, nch, c, 2).double().sum(1)
    torch.testing.assert_close(got, R.stat_sums_ref(out.cpu(), n), **STAT_TOL)
    assert torch.equal(bits(part.cpu()[used:]), bits(part_before[used:])), f"{what}: the statistics buffer was written beyond n * nchunks records"


# ---- 1. fmx_conv3x3_gn_silu: tile 8 x 32 pixels, 64-channel chunks, 128 outputs -------------------------------------------------------------
GN_SHAPES = [(1, 5, 7, 64), (2, 8, 32, 128), (3, 9, 33, 64), (2, 17, 65, 192), (1, 16, 64, 256)]
GN_VARIANTS = ("plain", "residual", "residual_windows", "inplace")
COUT = 128


@lru_cache(maxsize=None)
def gn_case(shape, dtype, groups=32, nout=COUT):
    n, h, w, c = shape
    seed = 7000 + 13 * h + w + c + nout
    wt = rnd(nout, c, 3, 3, scale=1 / math.sqrt(9 * c), seed=seed + 1, dtype=dtype)
    return Obj(shape=shape, groups=groups, nout=nout, m=n * h * w, x=teeth_x(n, h, w, c, groups, dtype, seed), wt=wt,
               gamma=(1 + 0.1 * torch.randn(c, generator=gen(seed + 2))).to(dtype), beta=(0.8 + 0.3 * torch.randn(c, generator=gen(seed + 3))).to(dtype),
               bias=rnd(nout, scale=0.5, seed=seed + 4, dtype=dtype), res=rnd(n * h * w, nout, seed=seed + 5, dtype=dtype))


@lru_cache(maxsize=None)
def gn_ref(shape, dtype, groups=32, nout=COUT, residual=False, bias=True):
    k = gn_case(shape, dtype, groups, nout)
    return R.gn_silu_conv_ref(k.x, k.gamma, k.beta, EPS_GN, k.wt, k.bias if bias else None, k.res if residual else None, dtype,
                              groups=groups).reshape(k.m, nout)


def gn_windows(k):
    """the case's operands as windows of 30000-filled buffers (x and the weight contiguous by contract: row windows)"""
    c = k.shape[-1]
    return Obj(x=Win(k.x.reshape(k.m, c), 2, 3), wk=Win(tap_major(k.wt), 1, 2), gamma=Win(k.gamma, left=8, right=8), beta=Win(k.beta, left=8, right=8),
               bias=Win(k.bias, left=8, right=8))


def gn_destination(k, variant, dtype):
    """-> (sentinel buffer on the CPU, row slice, column slice, residual Win or None): dense [M, 128] between sentinel rows, or -- with windows / in
    place -- columns [16, 144) of a 160-wide buffer (ld_out = 160); the residual window columns [4, 132) of a 136-wide one (ld_res = 136)"""
    wide = variant in ("residual_windows", "inplace")
    buf = sentinel_buffer(2 + k.m + 3, 160 if wide else COUT, dtype)
    rows, cols = slice(2, 2 + k.m), slice(16, 16 + COUT) if wide else slice(0, COUT)
    res = None
    if variant == "inplace":
        buf[rows, cols] = k.res
    elif variant == "residual_windows":
        res = Win(k.res, 3, 2, 4, 4)
    elif variant == "residual":
        res = Win(k.res, 3, 2)
    return buf, rows, cols, res


def tiles_of(h, w, th, tw):
    return -(-h // th) * -(-w // tw)


def run_gn_silu(k, variant, dtype, what, stats_of=None):
    n, h, w, c = k.shape
    W_ = gn_windows(k)
    buf, rows, cols, res = gn_destination(k, variant, dtype)
    dbuf = buf.to(DEV)
    out = dbuf[rows, cols]
    x = W_.x.on(DEV).view(n, h, w, c)
    st_x = stats_of(x) if stats_of is not None else ops.groupnorm_stats(x)
    tiles = tiles_of(h, w, 8, 32)
    part_before = f32_sentinel(n * tiles * COUT * 2 + 1024)
    part = part_before.to(DEV)
    residual = out if variant == "inplace" else None if res is None else res.on(DEV)
    got, st = ops.conv3x3_gn_silu(x, W_.gamma.on(DEV), W_.beta.on(DEV), EPS_GN, W_.wk.on(DEV), W_.bias.on(DEV), residual=residual, out=out, groups=k.groups,
                                  stats=st_x, stats_partial=part)
    torch.cuda.synchronize()
    nchanged = changed_outside(buf, dbuf.cpu(), rows, cols)
    assert nchanged == 0, f"{what}: {nchanged} elements outside the output window changed"
    want = gn_ref(k.shape, dtype, k.groups, COUT, residual=variant != "plain")
    e = R.excess(out, want, dtype, *R.CONV_TOL[dtype])
    print(f"MEASURED conv3x3_gn_silu {what}: {e:.3f}x CONV_TOL")
    R.assert_within(out, want, dtype, *R.CONV_TOL[dtype], what)
    check_stats(st, part_before, part, out, n, tiles, COUT, what)
    return st_x


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("variant", GN_VARIANTS)
@pytest.mark.parametrize("shape", GN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv3x3_gn_silu(shape, variant, dt):
    """Image inside one tile, exactly one tile, one row and column past a tile, partial tiles on both axes with three chunks, four chunks; without
    residual, with a dense one, with `out` and `residual` as column and row windows (ld_out 160, ld_res 136), and in place (residual is out).  Output
    within CONV_TOL of gn_silu_conv_ref; one statistics record per tile and image whose sums are those of the stored output."""
    run_gn_silu(gn_case(shape, DTYPES[dt]), variant, DTYPES[dt], f"{shape} {variant} {dt}")


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_conv3x3_gn_silu_16_groups(dt):
    shape = (2, 8, 32, 128)
    run_gn_silu(gn_case(shape, DTYPES[dt], groups=16), "residual_windows", DTYPES[dt], f"{shape} 16 groups {dt}")


def identity_producer(x):
    """the statistics of x as a producing GEMM leaves them: a 1 x 1 convolution with the identity as its weight reproduces x exactly (one non-zero
    product per output, exact in fp32) and hands over the records of its epilogue or of the pass behind it"""
    n, h, w, c = x.shape
    eye = torch.eye(c, dtype=x.dtype, device=x.device)
    y, st = ops.conv_gemm(x, eye, c, stats=True)
    assert st is not None and st.nchunks > 1 and torch.equal(bits(y.view(x.shape)), bits(x))
    return st


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("shape", [(2, 8, 32, 128), (1, 16, 64, 256)], ids=lambda s: "x".join(map(str, s)))
def test_conv3x3_gn_silu_on_a_producers_statistics(shape, dt):
    """x_nchunks > 1: the statistics of x come from conv_gemm(stats=True) instead of groupnorm_stats"""
    run_gn_silu(gn_case(shape, DTYPES[dt]), "residual", DTYPES[dt], f"{shape} producer statistics {dt}", stats_of=identity_producer)


# ---- 2. fmx_conv3x3_narrow / fmx_conv3x3_narrow_gn_silu: tile 4 x 32, channel walk 128 / 64 / 32 ----------------------------------------------
NARROW_SHAPES = [(2, 3, 5, 32, 1), (1, 4, 32, 64, 3), (3, 5, 33, 96, 4), (1, 9, 70, 224, 2), (2, 6, 31, 320, 4)]
NARROW_VARIANTS = ("ld4", "ld12", "ld4_nobias")


@lru_cache(maxsize=None)
def narrow_case(shape, dtype):
    """plain form: x ~ N(0, 1); the fused form takes gn_case(shape[:4], dtype, 32, nout) (every channel count here divides into 32 groups)"""
    n, h, w, c, nout = shape
    seed = 8000 + 13 * h + w + c + nout
    return Obj(shape=shape[:4], nout=nout, m=n * h * w, x=rnd(n, h, w, c, seed=seed, dtype=dtype),
               wt=rnd(nout, c, 3, 3, scale=1 / math.sqrt(9 * c), seed=seed + 1, dtype=dtype), bias=rnd(nout, scale=0.5, seed=seed + 4, dtype=dtype))


@lru_cache(maxsize=None)
def narrow_ref(shape, dtype, bias=True):
    k = narrow_case(shape, dtype)
    return R.conv_ref(k.x, k.wt, k.bias if bias else None, pad=1).reshape(k.m, k.nout)


def run_narrow(k, variant, dtype, want, what, fused=None):
    """ld4: a [M, 4] destination between sentinel rows, columns >= nout written as zeros.  ld12: columns [4, 4 + nout) of a 12-wide buffer, nothing
    else changes (the zero fill belongs to ld_out == 4 alone)."""
    n, h, w, c = k.shape
    nout, ld = k.nout, 12 if variant == "ld12" else 4
    buf = sentinel_buffer(2 + k.m + 3, ld, dtype)
    rows = slice(2, 2 + k.m)
    cols = slice(4, 4 + nout) if ld == 12 else slice(0, 4)
    dbuf = buf.to(DEV)
    x = Win(k.x.reshape(k.m, c), 2, 3).on(DEV).view(n, h, w, c)
    wk = Win(tap_major(k.wt), 1, 2).on(DEV)
    bias = None if variant == "ld4_nobias" else Win(k.bias, left=8, right=8).on(DEV)
    if fused is None:
        ops.conv3x3_narrow(x, wk, bias, nout, out=dbuf[rows, cols], ld_out=ld)
    else:
        ops.conv3x3_narrow_gn_silu(x, Win(k.gamma, left=8, right=8).on(DEV), Win(k.beta, left=8, right=8).on(DEV), EPS_GN, wk, bias, nout, groups=k.groups,
                                   out=dbuf[rows, cols], ld_out=ld, stats=fused(x))
    torch.cuda.synchronize()
    nchanged = changed_outside(buf, dbuf.cpu(), rows, cols)
    assert nchanged == 0, f"{what}: {nchanged} elements outside the output window changed"
    got = dbuf[rows, cols]
    if ld == 4:
        assert bool((bits(got[:, nout:]) == 0).all()), f"{what}: columns >= nout of an ld_out = 4 output must be +0"
    e = R.excess(got[:, :nout], want, dtype, *R.CONV_TOL[dtype])
    print(f"MEASURED conv3x3_narrow{'_gn_silu' if fused else ''} {what}: {e:.3f}x CONV_TOL")
    R.assert_within(got[:, :nout], want, dtype, *R.CONV_TOL[dtype], what)


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("variant", NARROW_VARIANTS)
@pytest.mark.parametrize("shape", NARROW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv3x3_narrow(shape, variant, dt):
    """Image smaller than a tile, exactly one tile, one past it with a 64 + 32 chunk walk, 128 + 64 + 32, 128-channel chunks with ragged tiles; 1 to 4
    outputs; ld_out 4 (zero fill), ld_out 12 into a column window (only nout columns change), without bias.  CONV_TOL against conv_ref."""
    dtype = DTYPES[dt]
    run_narrow(narrow_case(shape, dtype), variant, dtype, narrow_ref(shape, dtype, bias=variant != "ld4_nobias"), f"{shape} {variant} {dt}")


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("variant", NARROW_VARIANTS)
@pytest.mark.parametrize("shape", NARROW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv3x3_narrow_gn_silu(shape, variant, dt):
    """The same shapes and destinations with GroupNorm (32 groups) + SiLU in the staging, on `teeth_x`; CONV_TOL against gn_silu_conv_ref."""
    dtype = DTYPES[dt]
    k = gn_case(shape[:4], dtype, 32, shape[4])
    run_narrow(k, variant, dtype, gn_ref(shape[:4], dtype, 32, shape[4], bias=variant != "ld4_nobias"), f"{shape} {variant} {dt}", fused=ops.groupnorm_stats)


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_conv3x3_narrow_gn_silu_on_a_producers_statistics(dt):
    dtype, shape = DTYPES[dt], (2, 8, 32, 128)
    run_narrow(gn_case(shape, dtype, 32, 3), "ld4", dtype, gn_ref(shape, dtype, 32, 3), f"{shape} producer statistics {dt}", fused=identity_producer)


# ---- 3. fmx_conv3x3_up2x: w % 32 == 0, h * w % 256 == 0, c % 64 == 0 ---------------------------------------------------------------------
UP_SHAPES = [(1, 8, 32, 64, 64), (3, 8, 32, 128, 136), (2, 16, 32, 192, 320), (1, 8, 64, 64, 328)]


@lru_cache(maxsize=None)
def up_case(shape, dtype):
    """image i carries a constant offset of its own (+8, -8, +8 ...): a border row that read the neighbouring image's pixels instead of zeros is far off"""
    n, h, w, c, nout = shape
    seed = 9000 + 13 * h + w + c + nout
    x = rnd(n, h, w, c, seed=seed, dtype=torch.float32) + torch.tensor([8.0, -8.0, 8.0, -8.0][:n])[:, None, None, None]
    wk = rnd(nout, 9 * c, scale=1 / math.sqrt(9 * c), seed=seed + 1, dtype=dtype)
    return Obj(shape=shape, x=x.to(dtype), wk=wk, w4=ops.fold_up2x_weights(wk, c), bias=rnd(nout, scale=0.5, seed=seed + 2, dtype=dtype))


@lru_cache(maxsize=None)
def up_ref(shape, dtype, bias=True):
    k = up_case(shape, dtype)
    return R.up2x_ref(k.x, k.w4, k.bias if bias else None).reshape(-1, shape[4])


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", UP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv3x3_up2x(shape, with_bias, dt):
    """The four phase convolutions against up2x_ref on the same rounded tap sums, CONV_TOL; 4 h w / 256 statistics records per image with the sums of
    the stored output; nout of 64, 136 (one partial column tile), 320 (exactly the tile) and 328 (one tile and a remainder: the entry point asks for a
    multiple of 8 only).  hipops.conv3x3_up2x allocates its own dense output and cannot express a window, so the dense form is what is tested: the
    allocator hook hands it rows [2, 2 + M) of a sentinel buffer, and the rows above and below must stay untouched."""
    dtype = DTYPES[dt]
    n, h, w, c, nout = shape
    k = up_case(shape, dtype)
    m = n * 4 * h * w
    buf = sentinel_buffer(2 + m + 3, nout, dtype)
    dbuf = buf.to(DEV)
    rows, cols = slice(2, 2 + m), slice(0, nout)
    nch = 4 * h * w // 256
    part_before = f32_sentinel(n * nch * nout * 2 + 1024)
    part = part_before.to(DEV)

    def alloc(shape_, dt_):
        if tuple(shape_) == (m, nout) and dt_ == dtype:
            return dbuf[rows]
        return torch.empty(shape_, dtype=dt_, device=DEV)
    x = Win(k.x.reshape(n * h * w, c), 2, 3).on(DEV).view(n, h, w, c)
    prev = ops.set_allocator(alloc)
    try:
        out, st = ops.conv3x3_up2x(x, Win(k.w4.reshape(4 * nout, 4 * c), 1, 2).on(DEV).view(4, nout, 4 * c), Win(k.bias, left=8, right=8).on(DEV) if with_bias else None,
                                   nout, stats_partial=part)
    finally:
        ops.set_allocator(prev)
    torch.cuda.synchronize()
    assert out.data_ptr() == dbuf[rows].data_ptr()
    what = f"{shape} {'bias' if with_bias else 'no bias'} {dt}"
    nchanged = changed_outside(buf, dbuf.cpu(), rows, cols)
    assert nchanged == 0, f"{what}: {nchanged} elements outside the output changed"
    want = up_ref(shape, dtype, with_bias)
    e = R.excess(out, want, dtype, *R.CONV_TOL[dtype])
    print(f"MEASURED conv3x3_up2x {what}: {e:.3f}x CONV_TOL")
    R.assert_within(out, want, dtype, *R.CONV_TOL[dtype], what)
    check_stats(st, part_before, part, out, n, nch, nout, what)


# ---- 4. fmx_attention_single_head512: 64 queries per workgroup, 32-key steps ---------------------------------------------------------------
C512 = 512
ATTN_SHAPES = [(1, 1, 1), (2, 63, 31), (2, 64, 32), (3, 65, 33), (1, 130, 97), (2, 200, 77)]
ATTN_STRUCTURES = {"negative_scores": 160, "staircase": 160, "late_spike_ragged": 150, "first_step_spike_then_flat": 160}    # -> nk, at b = 2, nq = 96


@lru_cache(maxsize=None)
def attn_case(b, nq, nk, dtype, structure=None):
    """q [b, nq, 512], k / v [b, nk, 512] on the CPU.  Structures (the builders of test_gpu_kernels.test_attention_running_maximum_paths at 512 wide,
    five 32-key steps): every score strongly negative; a maximum that rises in every step for query 50; the dominant key the last valid one of a
    ragged last step; a dominant key in the first step, flat scores behind it."""
    seed = 9500 + 7 * nq + nk
    q, k, v = (rnd(b, n_, C512, seed=seed + i, dtype=torch.float32) for i, n_ in enumerate((nq, nk, nk)))
    if structure is None and nk > 1:
        k[b - 1, nk - 1] = q[b - 1, nq - 1] * 0.5          # a dominant key in the last valid row, for the last query
    elif structure == "negative_scores":
        q, k = q.abs(), -k.abs() - 0.5
    elif structure == "staircase":
        for t in range(5):
            k[:, t * 32 + 5] = q[:, 50] * (0.3 + 0.1 * t)
    elif structure == "late_spike_ragged":
        k[:, nk - 1] = q[:, 70] * 0.6
    elif structure == "first_step_spike_then_flat":
        k = k * 0.05
        k[:, 3] = q[:, 10] * 0.6
    return Obj(b=b, nq=nq, nk=nk, q=q.to(dtype), k=k.to(dtype), v=v.to(dtype))


@lru_cache(maxsize=None)
def attn_ref(b, nq, nk, dtype, structure=None):
    a = attn_case(b, nq, nk, dtype, structure)
    want = R.attn_ref(a.q[:, None], a.k[:, None], a.v[:, None], C512 ** -0.5)[:, 0]
    assert bool(torch.isfinite(want).all())
    return want.reshape(b * nq, C512)


def attn_buffers(a, dtype, separate_k=False):
    """the VAE's layout: q and k the two halves of one [b * n, 1024] buffer, n = max(nq, nk) rows per image (q rows >= nq hold 30000, k rows >= nk
    hold 7.0); separate_k: q a row window of a 512-wide buffer, k token-major [b * nk_pad, 512] with NaN in its pad rows.  V^T [512, b * nk_pad] with -5 in
    the pad columns.  -> (q Win | the qk buffer, k Win | None, vt, strides) on the CPU"""
    b, nq, nk = a.b, a.nq, a.nk
    nkp = -(-nk // 32) * 32
    vt = torch.full((b, nkp, C512), -5.0, dtype=dtype)
    vt[:, :nk] = a.v
    vt = vt.permute(2, 0, 1).reshape(C512, b * nkp).contiguous()
    if separate_k:
        qw = Win(a.q.reshape(b * nq, C512), 2, 3)
        k = torch.full((b, nkp, C512), math.nan, dtype=dtype)        # include/fmx.h: k rows >= nk are never read and may hold anything
        k[:, :nk] = a.k
        return qw, Win(k.reshape(b * nkp, C512)), vt, dict(q_bs=nq * C512, q_rs=C512, k_bs=nkp * C512, k_rs=C512, vt_bs=nkp, vt_ds=b * nkp)
    n = max(nq, nk)
    qk = torch.empty(b, n, 2 * C512, dtype=dtype)
    qk[..., :C512], qk[..., C512:] = BIG, 7.0
    qk[:, :nq, :C512], qk[:, :nk, C512:] = a.q, a.k
    qk = qk.reshape(b * n, 2 * C512)
    return qk, None, vt, dict(q_bs=n * 2 * C512, q_rs=2 * C512, k_bs=n * 2 * C512, k_rs=2 * C512, vt_bs=nkp, vt_ds=b * nkp)


def run_attn512(a, dtype, want, what, separate_k=False):
    b, nq, nk = a.b, a.nq, a.nk
    qw, kw, vt, strides = attn_buffers(a, dtype, separate_k)
    if separate_k:
        q, k = qw.on(DEV), kw.on(DEV)
    else:
        qk = qw.to(DEV)
        q, k = qk[:, :C512], qk[:, C512:]
    buf = sentinel_buffer(2 + b * nq + 3, 640, dtype)
    rows, cols = slice(2, 2 + b * nq), slice(64, 64 + C512)
    dbuf = buf.to(DEV)
    ops.attention_single_head512(q, k, vt.to(DEV), dbuf[rows, cols], batch=b, nq=nq, nk=nk, nk_pad=-(-nk // 32) * 32, scale=C512 ** -0.5, **strides)
    torch.cuda.synchronize()
    nchanged = changed_outside(buf, dbuf.cpu(), rows, cols)
    assert nchanged == 0, f"{what}: {nchanged} elements outside the output window changed"
    e = R.excess(dbuf[rows, cols], want, dtype, *R.ATTN_TOL[dtype])
    print(f"MEASURED attention512 {what}: {e:.3f}x ATTN_TOL")
    R.assert_within(dbuf[rows, cols], want, dtype, *R.ATTN_TOL[dtype], what)


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("b,nq,nk", ATTN_SHAPES)
def test_attention512_qk_halves_of_one_buffer(b, nq, nk, dt):
    """q_rs = k_rs = 1024 (the layout backend/nn/vae.py uses), o a column window of a 640-wide sentinel buffer; fewer than 64 queries, fewer than 32
    keys, one past each, several query tiles with a ragged last one, pad keys holding 7.0 / -5."""
    dtype = DTYPES[dt]
    run_attn512(attn_case(b, nq, nk, dtype), dtype, attn_ref(b, nq, nk, dtype), f"b{b} nq{nq} nk{nk} {dt}")


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_attention512_separate_token_major_k(dt):
    dtype = DTYPES[dt]
    run_attn512(attn_case(3, 65, 33, dtype), dtype, attn_ref(3, 65, 33, dtype), f"separate k b3 nq65 nk33 {dt}", separate_k=True)


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("structure", sorted(ATTN_STRUCTURES))
def test_attention512_running_maximum_paths(structure, dt):
    dtype, nk = DTYPES[dt], ATTN_STRUCTURES[structure]
    run_attn512(attn_case(2, 96, nk, dtype, structure), dtype, attn_ref(2, 96, nk, dtype, structure), f"{structure} {dt}")


# ---- contract refusals (host side, FMX_E_BADARG) ----------------------------------------------------------------------------------------------
def test_refusals_name_the_rule():
    x = rnd(1, 8, 32, 64, dtype=H16).to(DEV)
    w4 = torch.zeros(4, 12, 256, dtype=H16, device=DEV)
    with pytest.raises(Exception, match="output channels of 8"):
        ops.conv3x3_up2x(x, w4, None, 12)
    k = gn_case((1, 5, 7, 64), H16)
    with pytest.raises(Exception, match="bad leading dimensions"):
        ops.conv3x3_gn_silu(x, k.gamma.to(DEV), k.beta.to(DEV), EPS_GN, tap_major(k.wt).to(DEV), None, out=torch.zeros(256, 130, dtype=H16, device=DEV)[:, :128],
                            stats=ops.groupnorm_stats(x))
