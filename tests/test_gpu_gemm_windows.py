"""GPU (MI355X) kernel-level tests of fmx_gemm_conv_f16 / _bf16 on the operand forms the executors use and the dense-buffer tests never reach:
output, residual, row vector, gate, A and W as WINDOWS of larger buffers (every leading dimension of fmx_gemm_args away from its dense value),
in-place residuals on row windows, the two-source form with a full epilogue, `alpha`, GEGLU into a wider buffer, and fp32 output.

Conventions (tests/test_gpu_kernels_bf16.py): inputs are built on the CPU by the module-level builders below (tests/test_kernel_ref_teeth.py
imports them and shows that each check rejects a planted bug), moved to the device inside the test, references from tests/kernel_refs.py in
fp64 on the rounded inputs.  Contract: every base pointer stays 16-byte aligned and every A / W stride a multiple of 8 elements, as include/fmx.h
asks -- window offsets are multiples of 8 elements.

Sentinel rule: every destination is larger than the window that the launch may write (columns left and right where the case has a column
window, rows above and below), pre-filled with a finite bit pattern; after the launch everything outside the window is bit-identical to before.
Every input is a window of a buffer whose surroundings hold 30000, so a read from the wrong place is far outside any tolerance.

Tile families: every 16-bit case runs at the dispatcher's choice (force_tile 0) and on every tile id the older tests force; the only skips are
the dispatcher's own refusals (`refusal`, one rule per FMX_REQUIRE of csrc/fmx_gemm.hip).  fp32 output cannot be forced (the hook lives in the
sign of out_f32): those cases run at the dispatcher's choice."""
import math
from functools import lru_cache

import pytest
import torch

pytestmark = pytest.mark.gpu

import forge_amd  # noqa: E402,F401
from forge_amd import hipops as ops  # noqa: E402

import kernel_refs as R  # noqa: E402

DEV = "cuda"
BF, H16 = torch.bfloat16, torch.float16
DTYPES = {"f16": H16, "bf16": BF}
BIG = 30000.0                       # surroundings of every input window (finite in fp16 and bf16)
SENTINEL = {2: 0x7A5A, 4: 0x7A5A5A5A}   # destination fill by element size: fp16 ~5.2e4, bf16 / fp32 ~2.8e35 -- finite, never a result
INT = {2: torch.int16, 4: torch.int32}
TILES = (0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
TWO_STAGE, RING, ROWS256 = (1, 2, 3, 5), (11, 12, 13, 14, 15), (6, 7, 8, 9, 10)
ACTS = {"none": ops.ACT_NONE, "geglu": ops.ACT_GEGLU, "gelu_tanh": ops.ACT_GELU_TANH}


def gen(seed):
    return torch.Generator("cpu").manual_seed(seed)


def rnd(*shape, scale=1.0, seed=0, dtype=H16):
    return (torch.randn(*shape, generator=gen(seed)) * scale).to(dtype)


class Win:
    """a 1-D / 2-D operand as a window of a larger buffer: `buf` (CPU) holds `fill` everywhere but in buf[idx] = values"""

    def __init__(self, values, above=0, below=0, left=0, right=0, fill=BIG):
        if values.dim() == 1:
            shape, self.idx = (left + values.shape[0] + right,), (slice(left, left + values.shape[0]),)
        else:
            r, c = values.shape
            shape, self.idx = (above + r + below, left + c + right), (slice(above, above + r), slice(left, left + c))
        self.buf = torch.full(shape, fill, dtype=values.dtype)
        self.buf[self.idx] = values

    @property
    def values(self):
        return self.buf[self.idx]

    def on(self, dev):
        return self.buf.to(dev)[self.idx]


def sentinel_buffer(rows, cols, dtype):
    size = torch.empty((), dtype=dtype).element_size()
    return torch.full((rows, cols), SENTINEL[size], dtype=INT[size]).view(dtype)


def bits(t):
    return t.view(INT[t.element_size()])


def changed_outside(before, after, rows, cols):
    """number of elements of the destination buffer outside the window [rows, cols] whose bits differ from before the launch"""
    diff = bits(before) != bits(after)
    diff[rows, cols] = False
    return int(diff.sum())


class Launch:
    """one conv_gemm call: Win operands, geometry, and the window (rows, cols) of the case's destination buffer that it writes"""

    def __init__(self, **kw):
        self.a1 = self.bias = self.rowvec = self.gate = self.residual = None
        self.inplace, self.alpha, self.act, self.kh, self.pad, self.n_img, self.hw = False, 1.0, "none", 1, 0, 1, None
        self.__dict__.update(kw)

    @property
    def ncols(self):
        return self.nout // 2 if self.act == "geglu" else self.nout


class Case:
    def __init__(self, out_buf, launches):
        self.out_buf, self.launches = out_buf, launches


def make(dtype, seed, *, m=None, n_img=1, per=None, k0=128, k1=0, nout=128, a0_pad=(0, 0, 0, 0), a1_pad=(0, 0, 0, 0), w_pad=(0, 0, 0, 0), bias=True,
         rowvec=None, gate=None, residual=None, out_pad=(2, 3, 8, 16), alpha=1.0, act="none", out_dtype=None, conv=None, bias_scale=0.5):
    """one linear (or, with conv=(n, h, w), 3x3 pad 1 convolution) launch.  *_pad = (above, below, left, right) rows / columns of surroundings.
    rowvec / gate: None or the pad of their [n_img, nout] window; residual: None, a pad (a window of its own buffer), or "inplace" (the
    destination window holds it)."""
    if conv is not None:
        n_img, per = conv[0], conv[1] * conv[2]
    per = per or m
    m = n_img * per
    kk = 9 if conv is not None else 1
    w = rnd(nout, kk * (k0 + k1), scale=1 / math.sqrt(kk * (k0 + k1)), seed=seed + 2, dtype=dtype)
    L = Launch(a0=Win(rnd(m, k0, seed=seed, dtype=dtype), *a0_pad), w=Win(w, *w_pad), nout=nout, n_img=n_img, per=per, alpha=alpha, act=act, m=m,
               kh=3 if conv is not None else 1, pad=1 if conv is not None else 0, hw=None if conv is None else conv[1:])
    if k1:
        L.a1 = Win(rnd(m, k1, seed=seed + 1, dtype=dtype), *a1_pad)
    if bias:
        L.bias = Win(rnd(nout, scale=bias_scale, seed=seed + 3, dtype=dtype), left=8, right=8)
    if rowvec is not None:
        L.rowvec = Win(rnd(n_img, nout, scale=0.5, seed=seed + 4, dtype=dtype), *rowvec)
    if gate is not None:
        L.gate = Win(rnd(n_img, nout, scale=0.7, seed=seed + 5, dtype=dtype), *gate)
    ncols = L.ncols
    out_dtype = out_dtype or dtype
    above, below, left, right = out_pad
    out = sentinel_buffer(above + m + below, left + ncols + right, out_dtype)
    L.rows, L.cols = slice(above, above + m), slice(left, left + ncols)
    if residual == "inplace":
        assert out_dtype == dtype
        L.inplace = True
        out[L.rows, L.cols] = rnd(m, ncols, seed=seed + 6, dtype=dtype)
    elif residual is not None:
        L.residual = Win(rnd(m, ncols, seed=seed + 6, dtype=dtype), *residual)
    return Case(out, [L])


def clip_vt(dtype, seed, t):
    """backend/nn/clip.py:84, operand-swapped V^T = W_v X^T per image: A = the weight [c, K], W = one image's activations [t, K], the output a
    column window [bi * tp, bi * tp + t) of vt [c, 64 + b * tp] (64 more columns on the left so that image 0 has a left neighbour too)"""
    c, k, b = 192, 128, 2
    tp = -(-t // 64) * 64
    wv = Win(rnd(c, k, scale=1 / math.sqrt(k), seed=seed, dtype=dtype), 2, 2, 0, 0)
    out = sentinel_buffer(2 + c + 2, 64 + b * tp, dtype)
    launches = []
    for bi in range(b):
        x = Win(rnd(t, k, seed=seed + 1 + bi, dtype=dtype), 3, 5, 0, 0)
        launches.append(Launch(a0=wv, w=x, nout=t, m=c, per=c, rows=slice(2, 2 + c), cols=slice(64 + bi * tp, 64 + bi * tp + t)))
    return Case(out, launches)


MODS = (0, 0, 256, 256)        # a [n, nout] window in the middle of a [n, nout + 512] modulation-style buffer
# name -> list of (builder, kwargs); every entry is one parametrised test id "name-i"
WINDOW_CASES = {
    # nout % 8 == 0, the destination a column window at a multiple of 8 of a wider buffer, ragged M (the last one long enough in K for split-K)
    "out_cols_eligible8": [(make, dict(m=300, k0=128, nout=320, out_pad=(3, 2, 64, 56))),
                           (make, dict(m=1000, k0=64, nout=256, out_pad=(2, 3, 8, 24))),
                           (make, dict(m=320, k0=128, nout=160, out_pad=(2, 3, 160, 8))),
                           (make, dict(m=1000, k0=640, nout=328, out_pad=(2, 3, 16, 40)))],
    # clip.py:84: nout = t ragged, ld_out a multiple of 64, two images into adjacent windows
    "out_cols_ragged": [(clip_vt, dict(t=77)), (clip_vt, dict(t=33)), (clip_vt, dict(t=132))],
    # dense rows whose length is not a multiple of 4 (backend/patcher/lora.py: ld_out = w2.shape[1]); bias, dense residual of the same odd row length
    "out_ld_odd": [(make, dict(m=150, k0=128, nout=77, out_pad=(8, 8, 0, 0), residual=(8, 8, 0, 0))),
                   (make, dict(m=150, k0=64, nout=90, out_pad=(8, 8, 0, 0), residual=(16, 8, 0, 0)))],
    # ld_res != ld_out (residual a column window of a wider buffer); in place on a row window of a taller tensor (flux.py:213)
    "residual_window": [(make, dict(m=1000, k0=640, nout=320, out_pad=(2, 3, 8, 8), residual=(3, 2, 64, 128))),
                        (make, dict(m=300, k0=128, nout=320, out_pad=(40, 24, 0, 0), residual="inplace", a0_pad=(16, 8, 0, 0))),
                        (make, dict(m=300, k0=128, nout=132, out_pad=(2, 3, 0, 4), residual=(3, 2, 32, 36)))],
    # images whose row count is no multiple of a tile height; rowvec and gate column windows of wider buffers; the one-row gate slice of flux.py:213
    "rowvec_gate_strided": [(make, dict(n_img=3, per=100, k0=128, nout=256, rowvec=MODS, gate=MODS)),
                            (make, dict(n_img=3, per=300, k0=128, nout=256, rowvec=MODS, gate=MODS, act="gelu_tanh")),
                            (make, dict(n_img=1, per=100, k0=128, nout=256, rowvec=(1, 2, 256, 256), gate=(2, 1, 256, 256))),
                            (make, dict(n_img=1, per=300, k0=128, nout=256, rowvec=(1, 2, 256, 256), gate=(2, 1, 256, 256), act="gelu_tanh")),
                            (make, dict(n_img=4, per=100, k0=64, nout=320, bias=False, rowvec=MODS, gate=MODS, act="gelu_tanh"))],
    # A a column window (a0_stride > c0), a row window, two sources with different strides; linear and 3x3 convolution (pixel stride > c)
    "a_windows": [(make, dict(m=300, k0=128, nout=136, a0_pad=(0, 0, 64, 64))),
                  (make, dict(m=300, k0=128, nout=136, a0_pad=(24, 8, 0, 0))),
                  (make, dict(m=300, k0=128, k1=64, nout=136, a0_pad=(8, 8, 64, 0), a1_pad=(16, 0, 64, 192))),
                  (make, dict(conv=(2, 9, 7), k0=64, nout=72, a0_pad=(8, 8, 32, 32))),
                  (make, dict(conv=(2, 9, 7), k0=64, k1=64, nout=72, a0_pad=(8, 8, 32, 32), a1_pad=(0, 16, 8, 0)))],
    # ldw > K: the weight a column and row window of a wider matrix; linear and 3x3
    "w_window": [(make, dict(m=300, k0=128, nout=136, w_pad=(3, 5, 64, 64))),
                 (make, dict(conv=(2, 9, 7), k0=64, nout=72, w_pad=(3, 5, 64, 0)))],
    # flux.py:236 in small: two sources, bias, gate, residual in place, several images of a ragged row count
    "two_source_full_epilogue": [(make, dict(n_img=3, per=100, k0=128, k1=192, nout=128, gate=MODS, residual="inplace", out_pad=(8, 8, 0, 0),
                                             a1_pad=(0, 0, 0, 64)))],
    # acc * alpha + bias + rowvec + residual: alpha on the accumulator only
    "alpha_order": [(make, dict(n_img=3, per=100, k0=128, nout=136, alpha=0.5, rowvec=MODS, residual=(3, 2, 8, 8), bias_scale=1.0)),
                    (make, dict(n_img=3, per=100, k0=128, nout=136, alpha=-2.0, rowvec=MODS, residual=(3, 2, 8, 8), bias_scale=1.0))],
    # GEGLU writes nout / 2 columns into a wider buffer (with and without a residual window)
    "geglu_window": [(make, dict(m=300, k0=128, nout=320, act="geglu", out_pad=(2, 3, 8, 24))),
                     (make, dict(m=300, k0=128, nout=320, act="geglu", out_pad=(2, 3, 8, 24), residual=(3, 2, 64, 32)))],
}
# fp32 destination with alpha, bias and a 16-bit residual, nout a multiple of 8 and ragged, at sizes across the dispatcher's regimes
F32_CASES = [dict(m=m, k0=320, nout=nout, alpha=0.75, residual=(3, 2, 8, right - 8), out_pad=(2, 3, 8, right), out_dtype=torch.float32)
             for m in (150, 2048, 16384) for nout, right in ((320, 24), (77, 11))]
CASE_IDS = [f"{name}-{i}" for name, subs in WINDOW_CASES.items() for i in range(len(subs))]


@lru_cache(maxsize=None)
def build(case_id, dtype):
    name, i = case_id.rsplit("-", 1)
    builder, kw = WINDOW_CASES[name][int(i)]
    return builder(dtype, 1000 + 10 * CASE_IDS.index(case_id), **kw)


def launch_ref(L, out_before):
    """fp64 reference of one launch: [M, ncols]"""
    res = out_before[L.rows, L.cols] if L.inplace else None if L.residual is None else L.residual.values
    if L.kh == 3:
        n, (h, w) = L.n_img, L.hw
        a = L.a0.values if L.a1 is None else torch.cat([L.a0.values, L.a1.values], -1)
        wt = L.w.values.view(L.nout, 3, 3, -1).permute(0, 3, 1, 2)
        assert L.alpha == 1.0 and L.act == "none" and L.gate is None
        return R.conv_ref(a.view(n, h, w, -1), wt, None if L.bias is None else L.bias.values, pad=1,
                          rowvec=None if L.rowvec is None else L.rowvec.values, residual=res).reshape(L.m, L.nout)
    val = lambda x: None if x is None else x.values  # noqa: E731
    return R.gemm_ref(L.a0.values, L.w.values, a1=val(L.a1), alpha=L.alpha, bias=val(L.bias), rowvec=val(L.rowvec), rows_per_image=L.per, act=L.act,
                      gate=val(L.gate), residual=res)


@lru_cache(maxsize=None)
def case_refs(case_id, dtype):
    case = build(case_id, dtype)
    return [launch_ref(L, case.out_buf) for L in case.launches]


def eligible8(L, out_buf):
    """FastEpilogue::eligible8 (csrc/fmx_gemm_common.hpp) of a launch, from what the wrapper will pass"""
    def ok(win, rows_matter=True):
        if win is None:
            return True
        v = win.values
        ld = v.stride(0) if v.dim() == 2 and rows_matter else 0
        return ld % 8 == 0 and (v.storage_offset() * v.element_size()) % 16 == 0
    out = out_buf[L.rows, L.cols]
    return (out_buf.element_size() == 2 and L.nout % 8 == 0 and out.stride(0) % 8 == 0 and (out.storage_offset() * 2) % 16 == 0 and
            ok(L.bias) and ok(L.rowvec) and ok(L.gate) and ok(L.residual))


def refusal(L, out_buf, tile):
    """why the dispatcher refuses to run this launch on a forced tile (the FMX_REQUIRE lines of gemm_conv_one, csrc/fmx_gemm.hip), or None"""
    geglu, conv = L.act == "geglu", L.kh != 1
    if tile in ROWS256 and not eligible8(L, out_buf):
        return "gemm: the 256-row kernels need fp16 output, 16-byte aligned epilogue operands, leading dimensions / nout multiples of 8"
    if tile == 10 and (conv or L.a1 is not None):
        return "gemm: the 256x160 two-workgroup tile takes plain linear GEMMs (one source, no output statistics)"
    if tile == 9 and (geglu or (conv and L.a1 is not None)):
        return "gemm: the 512x128 tile takes no GEGLU, second source or upsample-on-load"
    if tile in (12, 14, 15) and geglu:
        return "gemm: the 128x160 / 64x160 / 160x64 ring tiles do not support GEGLU"
    if tile == 5 and geglu:
        return "gemm: the 128x160 tile does not support GEGLU"
    return None


def tolerance(L, dtype):
    return R.GEMM_ACT_TOL[dtype] if L.act in ("geglu", "gelu_tanh") else R.CONV_TOL[dtype]


def run_launch(L, dbuf, tile=0):
    """launch L into its window of the device buffer `dbuf`; -> (the window, the buffer as it was before the launch)"""
    before = dbuf.clone()
    out = dbuf[L.rows, L.cols]
    dev = dbuf.device
    on = lambda x: None if x is None else x.on(dev)  # noqa: E731
    a0, a1, w, bias = on(L.a0), on(L.a1), on(L.w), on(L.bias)
    if L.act == "geglu":      # the kernel reads [16 value | 16 gate] interleaved rows; the reference works on the un-interleaved weight
        w, bias = ops.geglu_interleave(w.contiguous(), None if bias is None else bias.contiguous())
    if L.kh == 3:
        n, (h, wd) = L.n_img, L.hw
        a0 = a0.view(n, h, wd, -1)
        a1 = None if a1 is None else a1.view(n, h, wd, -1)
        geo = {}
    else:
        geo = dict(n=L.n_img, h=1, w=L.per)
    ops.conv_gemm(a0, w, L.nout, x1=a1, kh=L.kh, pad=L.pad, bias=bias, rowvec=on(L.rowvec), gate=on(L.gate), residual=out if L.inplace else on(L.residual),
                  act=ACTS[L.act], alpha=L.alpha, out=out, ld_out=dbuf.stride(0), force_tile=tile, **geo)
    torch.cuda.synchronize()
    return out, before


def check_case(case_id, dtype, tile, what):
    case = build(case_id, dtype)
    for L in case.launches:
        why = refusal(L, case.out_buf, tile)
        if why is not None:
            pytest.skip(f"the dispatcher refuses tile {tile} here: {why}")
    dbuf = case.out_buf.to(DEV)
    outs = []
    for i, (L, want) in enumerate(zip(case.launches, case_refs(case_id, dtype))):
        out, before = run_launch(L, dbuf, tile)
        n = changed_outside(before.cpu(), dbuf.cpu(), L.rows, L.cols)
        assert n == 0, f"{what} launch {i}: {n} elements outside the output window changed"
        R.assert_within(out, want, dtype, *tolerance(L, dtype), f"{what} launch {i}")
        outs.append(out.clone())
    # an earlier launch's window must have survived the later ones (adjacent windows of one buffer)
    for i, L in enumerate(case.launches[:-1]):
        assert torch.equal(bits(dbuf[L.rows, L.cols]), bits(outs[i])), f"{what}: launch {i}'s window was changed by a later launch"
    return dbuf


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("case_id", [c for c in CASE_IDS if not c.startswith(("rowvec_gate", "geglu"))])
def test_gemm_windows(case_id, dt, tile):
    """act NONE (with and without a gate) on every window form of WINDOW_CASES: the window within CONV_TOL of fp64, everything around it untouched."""
    check_case(case_id, DTYPES[dt], tile, f"{case_id} {dt} tile {tile}")


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("case_id", [c for c in CASE_IDS if c.startswith(("rowvec_gate", "geglu"))])
def test_gemm_windows_activation_and_gate(case_id, dt, tile):
    """Row vector and gate per image (images of 100 / 300 rows: an image boundary inside every tile), GELU-tanh off and on, GEGLU into a wider
    buffer; tolerance kernel_refs.GEMM_ACT_TOL (= CONV_TOL).  The gate after the activation is resolved (gelu(acc * gate) is hundreds of
    tolerances away); WHICH GELU is not: erf-GELU in place of tanh-GELU differs by <= ~5e-4 absolute, 0.5x (fp16) / 0.06x (bf16) of the
    tolerance, and gate / GELU-tanh exist with 16-bit output only, so no kernel-level test can tell the two apart."""
    check_case(case_id, DTYPES[dt], tile, f"{case_id} {dt} tile {tile}")


@lru_cache(maxsize=None)
def build_f32(i, dtype):
    return make(dtype, 5000 + 10 * i, **F32_CASES[i])


def f32_ref_and_bound(L):
    want = R.gemm_ref(L.a0.values, L.w.values, alpha=L.alpha, bias=L.bias.values, residual=L.residual.values)
    return want, R.abs_bound(L.a0.values, L.w.values, alpha=L.alpha, terms=(L.bias.values, L.residual.values))


@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("i", range(len(F32_CASES)))
def test_gemm_fp32_output(i, dt):
    """float32 destination (a window of a wider sentinel-filled fp32 buffer) with alpha, bias and a 16-bit residual window, nout 320 and 77,
    M 150 / 2048 / 16384, at the dispatcher's choice of tile.  Tolerance: the derived per-element bound kernel_refs.GEMM_F32_TOL."""
    dtype = DTYPES[dt]
    case = build_f32(i, dtype)
    L = case.launches[0]
    dbuf = case.out_buf.to(DEV)
    out, before = run_launch(L, dbuf)
    assert out.dtype == torch.float32
    n = changed_outside(before.cpu(), dbuf.cpu(), L.rows, L.cols)
    assert n == 0, f"fp32 output {F32_CASES[i]}: {n} elements outside the output window changed"
    want, bound = f32_ref_and_bound(L)
    R.assert_within_bound(out, want, bound, f"fp32 output M={L.m} nout={L.nout} {dt}")


SPLITK_CASES = ("out_cols_eligible8-3", "residual_window-0")     # K = 640: ten K-tiles, three workgroups per output tile


@pytest.mark.parametrize("tile", [1, 2, 11, 13])
@pytest.mark.parametrize("dt", sorted(DTYPES))
@pytest.mark.parametrize("case_id", SPLITK_CASES)
def test_gemm_windows_split_k(case_id, dt, tile, monkeypatch):
    """The split-K hand-over (FMX_GEMM_SPLITK=3) writing a window: same sentinel rule and tolerance; the partial-accumulator area of the workspace
    was written (the launch did split), the arrival counters are left zero, and a second launch gives the same bits."""
    monkeypatch.setenv("FMX_ALLOW_KNOBS", "1")
    monkeypatch.setenv("FMX_GEMM_SPLITK", "3")
    ws = ops.splitk_workspace(torch.device(DEV, torch.cuda.current_device()))
    ws[65536:65536 + (1 << 20)].zero_()
    first = check_case(case_id, DTYPES[dt], tile, f"split-K {case_id} {dt} tile {tile}")
    assert bool(ws[65536:65536 + (1 << 20)].any()), "the launch did not go through the split-K workspace"
    assert not bool(ws[:65536].any()), "arrival counters not left zero"
    second = check_case(case_id, DTYPES[dt], tile, f"split-K {case_id} {dt} tile {tile}, second launch")
    assert torch.equal(bits(first), bits(second))
    assert not bool(ws[:65536].any()), "arrival counters not left zero after the second launch"
