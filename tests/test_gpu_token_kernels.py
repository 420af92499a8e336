"""GPU (MI355X) kernel-level tests of the kernels between the GEMMs and the attention on the token path -- fmx_layernorm / _padded / _mod and fmx_rmsnorm
(csrc/fmx_norm.hip: ln_kernel<MAXOCT, MOD>, rmsnorm_kernel<MAXOCT>) and fmx_flux_qk_norm_rope (csrc/fmx_flux.hip) -- in fp16 and bf16 against the fp64
references and the ulp tolerances of tests/kernel_refs.py (LN_TOL, RMS_TOL, ROPE_TOL), at the shapes where such kernels go wrong: every width on either side
of a MAXOCT threshold of the launchers, row counts that are no multiple of the four rows of a block, blocks that straddle two batches of the modulation
vectors, vectors taken as column windows of [B, 6c] / [B, 3c] / [B, 2c] buffers, rows where eps decides the result, constant and zero rows, an outlier
channel that dominates the sum of squares, and for the V^T store of the rope kernel every alignment of the destination (16 bytes: vector stores; 8 and 2
bytes: the scalar fallback on full and on ragged 32-token halves), two launches into one joint sequence, and qkv read out of a wider row.

Conventions (tests/test_gpu_sampler_kernels.py): inputs are built on the CPU by the cached module-level builders below from seeded generators
(tests/test_kernel_ref_teeth.py imports them, runs the fp32 emulations on them and plants the bugs) and moved to the device inside the test; no GPU work at
import.  Every destination is a window of a larger buffer that holds a NaN bit pattern everywhere (0x7E01 fp16, 0x7FC1 bf16: never a result, and a value
left unwritten fails the tolerance as NaN); after the launch everything the contract does not name is bit-identical to before.  Every case prints
`MEASURED <kernel> <case> <dtype> <excess>` (pytest -s): the worst error in units of the tolerance, the figures beside the tolerances in tests/kernel_refs.py."""
import math
from functools import lru_cache

import pytest
import torch

pytestmark = pytest.mark.gpu

import forge_amd  # noqa: E402,F401
from forge_amd import hipops as ops  # noqa: E402
from forge_amd.backend.nn.flux import _rope_table  # noqa: E402

import kernel_refs as R  # noqa: E402

DEV = "cuda"
H16, BF = torch.float16, torch.bfloat16
DTYPES = {"f16": H16, "bf16": BF}
NAN_BITS = {H16: 0x7E01, BF: 0x7FC1}                 # destination fill: a quiet NaN with a payload no kernel produces
BIG = 6e4                                           # what the surroundings of an input window hold: finite in fp16, ruins any result that reads it
LEAD, TAIL = 8, 40                                  # sentinel elements in front of (16 bytes: the window stays aligned) and behind every destination


def gen(seed):
    return torch.Generator("cpu").manual_seed(seed)


def bits(t):
    return t.view(torch.int16)


class Dst:
    """a destination tensor as a 16-byte aligned window of a flat buffer filled with NAN_BITS"""

    def __init__(self, shape, dtype):
        self.shape, self.dtype, self.n = tuple(shape), dtype, math.prod(shape)
        self.buf = torch.full((LEAD + self.n + TAIL,), NAN_BITS[dtype], dtype=torch.int16)

    def on(self, dev):
        self.dbuf = self.buf.to(dev)
        return self.dbuf[LEAD:LEAD + self.n].view(self.dtype).view(self.shape)

    def back(self):
        """-> (the window on the CPU, number of elements in front of / behind it whose bits changed)"""
        after = self.dbuf.cpu()
        outside = int((after[:LEAD] != NAN_BITS[self.dtype]).sum() + (after[LEAD + self.n:] != NAN_BITS[self.dtype]).sum())
        return after[LEAD:LEAD + self.n].view(self.dtype).view(self.shape), outside


def measured(kernel, case, dt, e):
    print(f"MEASURED {kernel} {case} {dt} {e:.3f}")
    return e


# ---- row data ---------------------------------------------------------------------------------------------------------------------------------------
ROWS = (1, 5, 37)                                    # none a multiple of the 4 rows of a block
PAIRS = [(0.0, 1.0), (0.3, 2.0), (10.0, 1.0), (100.0, 1.0), (1000.0, 1.0), (30000.0, 8.0), (0.0, 1e-3)]     # (offset, spread) of a LayerNorm row
LN_C = (8, 512, 520, 1024, 1032, 1536, 1544, 3072, 4096)           # launch_ln: MAXOCT 1 / 2 / 3 / 8 at c / 8 <= 64 / 128 / 192 / else
RMS_C = (8, 512, 520, 1024, 1032, 2048, 2056, 4096)                # fmx_rmsnorm: MAXOCT 1 / 2 / 4 / 8 at c / 8 <= 64 / 128 / 256 / else
LN_EPS, MOD_EPS, RMS_EPS, ROPE_EPS = 1e-5, 1e-6, 1e-6, 1e-6
CONST_ROW, ZERO_ROW = 1, 3                            # of a table with at least 5 rows
SMALL_PAIR = len(PAIRS) - 1                           # the rows on which eps decides the result


def pair_of_row(rows, first):
    """index into PAIRS per row: consecutive pairs from `first` on, so that a one-row table still moves through the pairs from case to case"""
    return [(first + r) % len(PAIRS) for r in range(rows)]


def ln_rows(rows, c, dtype, g, first=0, special=True):
    """[rows, c] in `dtype`: row r ~ offset + spread * N(0, 1) of its pair; with `special` and >= 5 rows, row CONST_ROW holds one value and row ZERO_ROW zeros"""
    idx = pair_of_row(rows, first)
    off = torch.tensor([PAIRS[i][0] for i in idx])[:, None]
    spread = torch.tensor([PAIRS[i][1] for i in idx])[:, None]
    x = off + spread * torch.randn(rows, c, generator=g)
    if special and rows >= 5:
        x[CONST_ROW] = 10.5
        x[ZERO_ROW] = 0.0
    return x.to(dtype)


def affine(c, dtype, g):
    """gamma ~ 1 +- 0.1, beta ~ 0.2 (+- 0.05)"""
    return (1.0 + 0.1 * torch.randn(c, generator=g)).to(dtype), (0.2 + 0.05 * torch.randn(c, generator=g)).to(dtype)


# ---- layernorm --------------------------------------------------------------------------------------------------------------------------------------
LN_CASES = [(rows, c) for rows in ROWS for c in LN_C]


@lru_cache(maxsize=None)
def ln_case(rows, c, dtype):
    g = gen(1000 + 7 * c + rows)
    x = ln_rows(rows, c, dtype, g, first=LN_C.index(c))
    gamma, beta = affine(c, dtype, g)
    return x, gamma, beta


@lru_cache(maxsize=None)
def ln_want(rows, c, dtype):
    return R.layernorm_ref(*ln_case(rows, c, dtype), R.f32(LN_EPS))


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("rows,c", LN_CASES)
def test_layernorm(rows, c, dt):
    """every row within LN_TOL of the fp64 LayerNorm of the rounded inputs, the output of the inputs' type, nothing written around the destination"""
    dtype = DTYPES[dt]
    x, gamma, beta = ln_case(rows, c, dtype)
    dst = Dst((rows, c), dtype)
    out = ops.layernorm(x.to(DEV), gamma.to(DEV), beta.to(DEV), LN_EPS, out=dst.on(DEV))
    torch.cuda.synchronize()
    assert out.dtype == dtype and out.shape == (rows, c)
    got, outside = dst.back()
    e = measured("layernorm", f"rows={rows},c={c}", dt, R.excess(got, ln_want(rows, c, dtype), dtype, *R.LN_TOL[dtype]))
    assert e <= 1.0, f"layernorm rows {rows} c {c} {dt}: {e:.3g}x LN_TOL"
    assert outside == 0, f"layernorm rows {rows} c {c} {dt}: {outside} elements around the destination changed"
    fresh = ops.layernorm(x.to(DEV), gamma.to(DEV), beta.to(DEV), LN_EPS)
    assert fresh.dtype == dtype and torch.equal(bits(fresh.cpu()), bits(got)), "the wrapper's own output differs from the out= form"


def test_layernorm_wrappers_refuse_mixed_types():
    x, g = torch.zeros(4, 64, dtype=H16, device=DEV), torch.zeros(64, dtype=BF, device=DEV)
    with pytest.raises(TypeError):
        ops.layernorm(x, g, g)
    with pytest.raises(TypeError):
        ops.layernorm(x, g.half(), g.half(), out=torch.empty(4, 64, dtype=BF, device=DEV))
    with pytest.raises(TypeError):
        ops.layernorm_padded(x, g.half(), g.half(), torch.empty(1, 8, 64, dtype=BF, device=DEV), 4)


# ---- rmsnorm ----------------------------------------------------------------------------------------------------------------------------------------
RMS_CASES = [(rows, c) for rows in ROWS for c in RMS_C]
RMS_OUTLIER = {H16: 6e4, BF: 3e5}                    # one channel of every scale-300 row: a T5-style outlier that dominates the sum of squares
RMS_ONE_ROW_SCALES = (300.0, 1e-3, 1.0)              # a one-row table takes these in turn over the widths


def rms_scales(rows, c):
    """row scales on a logarithmic grid from 1e-3 to 300 (both ends included), shuffled; the zero row of a table with >= 5 rows is marked 0"""
    if rows == 1:
        return [RMS_ONE_ROW_SCALES[RMS_C.index(c) % 3]]
    s = torch.logspace(-3.0, math.log10(300.0), rows)[torch.randperm(rows, generator=gen(2000 + c + rows))].tolist()
    s[next(r for r in (ZERO_ROW, 2, 0) if s[r] not in (min(s), max(s)))] = 0.0
    return s


@lru_cache(maxsize=None)
def rms_case(rows, c, dtype):
    """the outlier sits in the last 8 channels because eight N(0, 1) channels out of 4096 move rstd by 0.1%, a quarter of a bf16 ulp: at that width only
    an outlier makes a sum of squares that misses the last octet visible"""
    g = gen(2100 + 7 * c + rows)
    scales = rms_scales(rows, c)
    x = torch.randn(rows, c, generator=g) * torch.tensor(scales)[:, None]
    for r, s in enumerate(scales):
        if s > 299.0:
            x[r, c - 8 + int(torch.randint(8, (1,), generator=g))] = RMS_OUTLIER[dtype]
    return x.to(dtype), (1.0 + 0.1 * torch.randn(c, generator=g)).to(dtype)


@lru_cache(maxsize=None)
def rms_want(rows, c, dtype):
    return R.rmsnorm_ref(*rms_case(rows, c, dtype), R.f32(RMS_EPS))


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("rows,c", RMS_CASES)
def test_rmsnorm(rows, c, dt):
    """every row within RMS_TOL (1 ulp, no floor at the scale of 1) of the fp64 RMS norm, the zero row exactly zero, nothing written around the destination"""
    dtype = DTYPES[dt]
    x, w = rms_case(rows, c, dtype)
    dst = Dst((rows, c), dtype)
    out = ops.rmsnorm(x.to(DEV), w.to(DEV), RMS_EPS, out=dst.on(DEV))
    torch.cuda.synchronize()
    assert out.dtype == dtype and out.shape == (rows, c)
    got, outside = dst.back()
    e = measured("rmsnorm", f"rows={rows},c={c}", dt, R.excess(got, rms_want(rows, c, dtype), dtype, *R.RMS_TOL[dtype]))
    assert e <= 1.0, f"rmsnorm rows {rows} c {c} {dt}: {e:.3g}x RMS_TOL"
    assert outside == 0, f"rmsnorm rows {rows} c {c} {dt}: {outside} elements around the destination changed"
    assert ops.rmsnorm(x.to(DEV), w.to(DEV), RMS_EPS).dtype == dtype


# ---- layernorm_mod ----------------------------------------------------------------------------------------------------------------------------------
MOD_B = 3
MOD_WINDOWS = {"6c(1,0)": (6, 1, 0), "6c(4,3)": (6, 4, 3), "3c(1,0)": (3, 1, 0), "2c(1,0)": (2, 1, 0)}      # buffer width / c, scale chunk, shift chunk (flux.py)
MOD_CASES = [(c, rpb, win) for c in (520, 3072) for rpb in (37, 50) for win in MOD_WINDOWS]
MOD_NEG_BATCH = 1                                    # the batch whose scale is ~ -1 on the first quarter of its channels


@lru_cache(maxsize=None)
def mod_case(c, rpb, win, dtype):
    """-> (x [B * rpb, c], mods [B, k c], scale chunk, shift chunk): every chunk of mods other than the two holds BIG"""
    k, sc, sh = MOD_WINDOWS[win]
    g = gen(3000 + 11 * c + rpb + 100 * sc + k)
    x = ln_rows(MOD_B * rpb, c, dtype, g, first=rpb + sc)
    mods = torch.full((MOD_B, k * c), BIG)
    scale, shift = 0.5 * torch.randn(MOD_B, c, generator=g), 0.5 * torch.randn(MOD_B, c, generator=g)
    scale[MOD_NEG_BATCH, :c // 4] = -1.0 + 2e-3 * torch.randn(c // 4, generator=g)
    mods[:, sc * c:(sc + 1) * c], mods[:, sh * c:(sh + 1) * c] = scale, shift
    return x, mods.to(dtype), sc, sh


def mod_vectors(mods, c, sc, sh):
    return mods[:, sc * c:(sc + 1) * c], mods[:, sh * c:(sh + 1) * c]


@lru_cache(maxsize=None)
def mod_want(c, rpb, win, dtype):
    x, mods, sc, sh = mod_case(c, rpb, win, dtype)
    return R.layernorm_mod_ref(x, *mod_vectors(mods, c, sc, sh), rpb, R.f32(MOD_EPS))


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("c,rpb,win", MOD_CASES)
def test_layernorm_mod(c, rpb, win, dt):
    """(1 + scale[b]) LN(x) + shift[b] within LN_TOL with blocks of four rows that straddle two batches, the vectors as column windows of a wider buffer whose
    other chunks hold 6e4"""
    dtype = DTYPES[dt]
    x, mods, sc, sh = mod_case(c, rpb, win, dtype)
    scale, shift = mod_vectors(mods.to(DEV), c, sc, sh)
    dst = Dst(tuple(x.shape), dtype)
    out = ops.layernorm_mod(x.to(DEV), scale, shift, rpb, MOD_EPS, out=dst.on(DEV))
    torch.cuda.synchronize()
    assert out.dtype == dtype and out.shape == x.shape
    got, outside = dst.back()
    e = measured("layernorm_mod", f"c={c},rows_per_batch={rpb},window={win}", dt, R.excess(got, mod_want(c, rpb, win, dtype), dtype, *R.LN_TOL[dtype]))
    assert e <= 1.0, f"layernorm_mod c {c} rows per batch {rpb} window {win} {dt}: {e:.3g}x LN_TOL"
    assert outside == 0, f"layernorm_mod c {c} rows per batch {rpb} window {win} {dt}: {outside} elements around the destination changed"
    assert ops.layernorm_mod(x.to(DEV), scale, shift, rpb, MOD_EPS).dtype == dtype


# ---- layernorm_padded -------------------------------------------------------------------------------------------------------------------------------
PAD_B, PAD_N, PAD_NPAD = 3, 37, 64
PAD_C = (320, 1544)


@lru_cache(maxsize=None)
def pad_case(c, dtype):
    g = gen(4000 + c)
    x = ln_rows(PAD_B * PAD_N, c, dtype, g, first=c % 7)
    gamma, beta = affine(c, dtype, g)
    return x, gamma, beta


@lru_cache(maxsize=None)
def pad_want(c, dtype):
    return R.layernorm_ref(*pad_case(c, dtype), R.f32(LN_EPS))


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("c", PAD_C)
def test_layernorm_padded(c, dt):
    """rows 0 .. n - 1 of every image within LN_TOL; rows n .. n_pad - 1 and the surroundings of the buffer keep the sentinel bit for bit"""
    dtype = DTYPES[dt]
    x, gamma, beta = pad_case(c, dtype)
    dst = Dst((PAD_B, PAD_NPAD, c), dtype)
    out = ops.layernorm_padded(x.to(DEV), gamma.to(DEV), beta.to(DEV), dst.on(DEV), rows_per_image=PAD_N, eps=LN_EPS)
    torch.cuda.synchronize()
    assert out.dtype == dtype and out.shape == (PAD_B, PAD_NPAD, c)
    got, outside = dst.back()
    e = measured("layernorm_padded", f"c={c}", dt, R.excess(got[:, :PAD_N].reshape(PAD_B * PAD_N, c), pad_want(c, dtype), dtype, *R.LN_TOL[dtype]))
    assert e <= 1.0, f"layernorm_padded c {c} {dt}: {e:.3g}x LN_TOL"
    stale = int((bits(got[:, PAD_N:]) != NAN_BITS[dtype]).sum())
    assert stale == 0 and outside == 0, f"layernorm_padded c {c} {dt}: {stale} pad-row elements and {outside} elements around the buffer changed"


# ---- q/k norm + rope + V^T --------------------------------------------------------------------------------------------------------------------------
D = 128
ROPE_AXES, ROPE_THETA = [16, 56, 56], 10000
ROPE_WINDOW = (8, 72)                                 # ld_qkv case: qkv starts at column 8 of rows that are 72 columns wider than 3 H D
# name -> (b, h, l_pad, [(tokens, row_off) per launch into the same buffers], qkv as a window of a wider row)
ROPE_CASES = {
    "joint37+101": (2, 3, 192, [(37, 0), (101, 37)], False),    # H D = 384; the second launch stores V^T at odd columns: full halves, a ragged tail, 54 pad columns
    "t1": (2, 2, 64, [(1, 0)], False),                           # one token: both halves ragged or empty
    "t63": (2, 2, 64, [(63, 0)], False),                         # a vector half and a 31-token half
    "t64": (2, 2, 64, [(64, 0)], False),                         # a tile that is exactly full: vector stores only
    "t65": (2, 2, 128, [(65, 0)], False),                        # one token spills into a second tile
    "t100@40": (2, 2, 192, [(100, 40)], False),                  # 16-byte aligned offset, ragged last tile
    "t64@4": (2, 2, 128, [(64, 4)], False),                      # full halves at an 8-byte aligned offset: the scalar path
    "ld_window_t70@8": (2, 2, 128, [(70, 8)], True),
}


def rope_pe(ltot):
    """ids that differ for every token of the joint sequence (a 7-wide grid in axes 1 and 2, axis 0 cycling), none of them 0: no token has sin = 0"""
    t = torch.arange(ltot)
    return _rope_table(torch.stack([t % 3 + 1, t // 7 + 1, t % 7 + 1], -1).float(), ROPE_AXES, ROPE_THETA)


@lru_cache(maxsize=None)
def rope_case(name, dtype):
    """-> (pe, [launch]) with launch = dict(qkv = the [b * tokens, 3 h d] tensor or window, buf = the buffer the window lies in, qs, ks, tokens, row_off)"""
    b, h, l_pad, launches, window = ROPE_CASES[name]
    g = gen(5000 + sum(ord(ch) for ch in name))
    hd = h * D
    out = []
    for tokens, row_off in launches:
        mag = torch.exp(torch.empty(b * tokens).uniform_(math.log(1e-3), math.log(30.0), generator=g))     # log-uniform row magnitudes
        vals = torch.randn(b * tokens, 3 * hd, generator=g) * mag[:, None]
        if b * tokens > 1:
            vals[(b * tokens) // 2] = 0.0
        if window:
            buf = torch.full((b * tokens, 3 * hd + ROPE_WINDOW[1]), BIG)
            buf[:, ROPE_WINDOW[0]:ROPE_WINDOW[0] + 3 * hd] = vals
            buf = buf.to(dtype)
            qkv = buf[:, ROPE_WINDOW[0]:ROPE_WINDOW[0] + 3 * hd]
        else:
            buf = qkv = vals.to(dtype)
        out.append(dict(qkv=qkv, buf=buf, tokens=tokens, row_off=row_off, qs=(1.0 + 0.1 * torch.randn(D, generator=g)).to(dtype),
                        ks=(1.0 + 0.1 * torch.randn(D, generator=g)).to(dtype)))
    return rope_pe(max(t + o for t, o in launches)), out


@lru_cache(maxsize=None)
def rope_want(name, dtype):
    """-> per launch (q, k) fp64 [b, tokens, h, d]"""
    b, h = ROPE_CASES[name][:2]
    pe, launches = rope_case(name, dtype)
    return [R.qk_norm_rope_ref(L["qkv"], L["qs"], L["ks"], pe, b, L["tokens"], h, L["row_off"], R.f32(ROPE_EPS)) for L in launches]


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", list(ROPE_CASES))
def test_flux_qk_norm_rope(name, dt):
    """q and k of every written row within ROPE_TOL, V^T of every written column bit-equal to v, every other element of the three buffers (rows of the joint
    sequence that no launch covers, pad rows / columns, the buffers' surroundings) bitwise the sentinel -- checked once after all launches of the case"""
    dtype = DTYPES[dt]
    b, h, l_pad, _, window = ROPE_CASES[name]
    hd = h * D
    pe, launches = rope_case(name, dtype)
    qd, kd, vd = Dst((b, l_pad, hd), dtype), Dst((b, l_pad, hd), dtype), Dst((hd, b * l_pad), dtype)
    qo, ko, vt = qd.on(DEV), kd.on(DEV), vd.on(DEV)
    pe_dev = pe.to(DEV)
    for L in launches:
        buf = L["buf"].to(DEV)
        qkv = buf[:, ROPE_WINDOW[0]:ROPE_WINDOW[0] + 3 * hd] if window else buf
        assert qkv.stride(0) == L["qkv"].stride(0) and (not window or qkv.stride(0) == 3 * hd + ROPE_WINDOW[1])
        ops.flux_qk_norm_rope(qkv, L["qs"].to(DEV), L["ks"].to(DEV), pe_dev, qo, ko, vt, batch=b, tokens=L["tokens"], heads=h, head_dim=D,
                              row_off=L["row_off"], l_pad=l_pad, eps=ROPE_EPS)
    torch.cuda.synchronize()
    (gq, oq), (gk, ok), (gv, ov) = qd.back(), kd.back(), vd.back()
    assert oq == 0 and ok == 0 and ov == 0, f"{name} {dt}: {oq} / {ok} / {ov} elements around the q / k / V^T buffers changed"
    written = torch.zeros(l_pad, dtype=torch.bool)
    worst = 0.0
    gvt = gv.view(h, D, b, l_pad)
    for L, (wq, wk) in zip(launches, rope_want(name, dtype)):
        rows = slice(L["row_off"], L["row_off"] + L["tokens"])
        written[rows] = True
        worst = max(worst, R.excess(gq[:, rows].reshape(wq.shape), wq, dtype, *R.ROPE_TOL[dtype]), R.excess(gk[:, rows].reshape(wk.shape), wk, dtype, *R.ROPE_TOL[dtype]))
        v = R._rope_split(L["qkv"], b, L["tokens"], h)[2]                                       # [b, tokens, h, d]
        assert torch.equal(bits(gvt[:, :, :, rows].permute(2, 3, 0, 1).contiguous()), bits(v.contiguous())), f"{name} {dt}: V^T is not a copy of v"
    e = measured("flux_qk_norm_rope", name, dt, worst)
    assert e <= 1.0, f"flux_qk_norm_rope {name} {dt}: {e:.3g}x ROPE_TOL"
    for what, t in (("q", gq[:, ~written]), ("k", gk[:, ~written]), ("V^T", gvt[..., ~written])):
        n = int((bits(t.contiguous()) != NAN_BITS[dtype]).sum())
        assert n == 0, f"flux_qk_norm_rope {name} {dt}: {n} elements of {what} outside the written rows changed"
