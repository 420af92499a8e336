"""GPU (MI355X) kernel-level tests of the sampler-step kernels of csrc/fmx_elementwise.hip -- fmx_unet_pack_input, fmx_im2col3x3_smallc,
fmx_cfg_combine, fmx_sampler_euler_step / _lincomb3 / _lincomb / _error_norm, fmx_philox_randn -- against the fp64 references and derived bounds of
tests/kernel_refs.py, at the shapes where such kernels go wrong: odd sizes, sizes around a block of 256 and a float4, one pixel, per-image sigmas
(one of them 0), sigma_data 0.5, a padded eps row, every prediction type with one and two halves, optional outputs present and absent.

Conventions (tests/test_gpu_gemm_windows.py): inputs are built on the CPU by the module-level builders below from seeded generators
(tests/test_kernel_ref_teeth.py imports them, runs the fp32 emulations on them and plants the bugs), moved to the device inside the test.
Every input tensor is a contiguous, 16-byte aligned window of a larger buffer whose surroundings hold 30000 (fp16 / bf16) or 3e30 (fp32); every
output is a window of a larger buffer pre-filled with the sentinel bit pattern of tests/test_gpu_gemm_windows.py, and after the launch everything
outside the window is bit-identical to before.  Every test prints `MEASURED <kernel> <case>: <excess>` (pytest -s): the worst error in units
of the bound, the figures beside the bounds in tests/kernel_refs.py."""
import ctypes as C
import math
from functools import lru_cache

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import forge_amd  # noqa: E402,F401
from forge_amd import _lib  # noqa: E402
from forge_amd import hipops as ops  # noqa: E402

import kernel_refs as R  # noqa: E402
from test_gpu_gemm_windows import INT, SENTINEL, bits  # noqa: E402

DEV = "cuda"
F32, H16, BF = torch.float32, torch.float16, torch.bfloat16
BIG = {H16: 30000.0, BF: 30000.0, F32: 3e30}       # surroundings of every input window
ALIGN = {2: 8, 4: 4}                                # elements per 16 bytes


def gen(seed):
    return torch.Generator("cpu").manual_seed(seed)


class Win:
    """a contiguous tensor as a window of a larger flat buffer: `buf` (CPU) holds `fill` before and behind the values"""

    def __init__(self, values, lead=1, trail=1, fill=None):
        a = ALIGN[values.element_size()]
        self.lead, self.n, self.shape = lead * a, values.numel(), tuple(values.shape)
        self.buf = torch.full((self.lead + self.n + trail * a + 3,), BIG[values.dtype] if fill is None else fill, dtype=values.dtype)
        self.buf[self.lead:self.lead + self.n] = values.reshape(-1)

    def view(self, buf):
        return buf[self.lead:self.lead + self.n].view(self.shape)

    @property
    def values(self):
        return self.view(self.buf)

    def on(self, dev):
        """-> the window on the device (its buffer is kept in .dbuf for changed_outside)"""
        self.dbuf = self.buf.to(dev)
        return self.view(self.dbuf)

    def changed_outside(self):
        """number of elements of the device buffer outside the window whose bits differ from before the launch"""
        diff = bits(self.buf) != bits(self.dbuf.cpu())
        diff[self.lead:self.lead + self.n] = False
        return int(diff.sum())


class Out(Win):
    """a destination: a window of a buffer that holds the sentinel bit pattern everywhere (the window included)"""

    def __init__(self, shape, dtype, lead=1, trail=1):
        size = torch.empty((), dtype=dtype).element_size()
        a = ALIGN[size]
        self.lead, self.n, self.shape = lead * a, math.prod(shape), tuple(shape)
        self.buf = torch.full((self.lead + self.n + trail * a + 3,), SENTINEL[size], dtype=INT[size]).view(dtype)


def measured(kernel, case, e):
    print(f"MEASURED {kernel} {case}: {e:.3f}")
    return e


def untouched(what, *wins):
    for w in wins:
        n = w.changed_outside()
        assert n == 0, f"{what}: {n} elements outside a window changed"


# ---- unet_pack_input --------------------------------------------------------------------------------------------------------------------------------
PACK_SHAPES = [(2, 4, 5, 7, 2), (1, 7, 3, 3, 1), (3, 1, 1, 1, 2), (2, 4, 16, 12, 1)]     # (b, c, h, w, reps): 9c = 63 leaves one zero column; one pixel
PACK_SIGMAS = [14.6, 0.7, 0.0]                                                            # the last b of these: image b - 1 has sigma exactly 0 (unet.py:759)
SIGMA_DATAS = [1.0, 0.5]


@lru_cache(maxsize=None)
def pack_case(i):
    b, c, h, w, reps = PACK_SHAPES[i]
    g = gen(100 + i)
    x = torch.randn(b, c, h, w, generator=g) * 3
    x.view(-1)[::5] *= 1e-5                     # results in the fp16 subnormal range
    return Win(x, 2, 1), Win(torch.tensor(PACK_SIGMAS[-b:]), 1, 1), reps


@pytest.mark.parametrize("sd", SIGMA_DATAS)
@pytest.mark.parametrize("i", range(len(PACK_SHAPES)))
def test_unet_pack_input(i, sd):
    """all 64 columns of every row within ELEM_TOL[fp16] of x / sqrt(sigma^2 + sigma_data^2) at column (ky * 3 + kx) * c + ch; exact zeros in the padding
    taps and from column 9 c on; the second rep bit-equal to the first"""
    x, sigma, reps = pack_case(i)
    b, c, h, w = x.shape
    out = Out((reps * b * h * w, 64), H16, 3, 2)
    got = ops.unet_pack_input(x.on(DEV), sigma.on(DEV), reps, sigma_data=sd, out=out.on(DEV))
    torch.cuda.synchronize()
    untouched("unet_pack_input", x, sigma, out)
    want = R.pack_input_ref(x.values, sigma.values, sd, reps)
    got = got.cpu()
    e = measured("unet_pack_input", f"{PACK_SHAPES[i]} sd={sd}", R.excess(got, want, H16, *R.ELEM_TOL[H16]))
    assert e <= 1.0, f"unet_pack_input {PACK_SHAPES[i]} sigma_data {sd}: {e:.3g}x ELEM_TOL"
    assert int((bits(got)[want == 0] != 0).sum()) == 0, "padding taps / columns >= 9 c are not +0"
    assert torch.equal(bits(got[:b * h * w]), bits(got[(reps - 1) * b * h * w:])), "the second rep differs from the first"


# ---- im2col3x3_smallc -------------------------------------------------------------------------------------------------------------------------------
IM2COL_SHAPES = [(2, 5, 7, 4, 8), (1, 3, 3, 7, 8), (1, 1, 1, 1, 8), (2, 4, 6, 4, 64)]    # (n, h, w, c, ldx)


@lru_cache(maxsize=None)
def im2col_case(i, dtype):
    n, h, w, c, ldx = IM2COL_SHAPES[i]
    x = torch.full((n, h, w, ldx), 30000.0, dtype=dtype)                  # channels >= c must never appear
    v = (torch.randn(n, h, w, c, generator=gen(200 + i)) * 4).to(dtype)
    flat = v.view(-1)
    flat[0], flat[-1] = math.inf, -math.inf                                # corners: copied into the most taps' padding neighbours
    flat[flat.numel() // 2] = -0.0
    x[..., :c] = v
    return Win(x, 1, 2)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("i", range(len(IM2COL_SHAPES)))
def test_im2col3x3_smallc(i, dt):
    """a 16-bit word shuffle: every one of the 64 columns bit-equal to the reference (the first c channels only, +-inf and -0 copied as they are)"""
    dtype = {"f16": H16, "bf16": BF}[dt]
    x = im2col_case(i, dtype)
    n, h, w, c, _ = IM2COL_SHAPES[i]
    out = Out((n * h * w, 64), dtype, 2, 1)
    got = ops.im2col3x3_smallc(x.on(DEV), c, out=out.on(DEV))
    torch.cuda.synchronize()
    untouched("im2col3x3_smallc", x, out)
    wrong = int((bits(got.cpu()) != bits(R.im2col_smallc_ref(x.values, c))).sum())
    measured("im2col3x3_smallc", f"{IM2COL_SHAPES[i]} {dt}", float(wrong))
    assert wrong == 0, f"im2col3x3_smallc {IM2COL_SHAPES[i]} {dt}: {wrong} words differ"


# ---- cfg_combine ------------------------------------------------------------------------------------------------------------------------------------
PTYPES = ["epsilon", "v_prediction", "edm"]
CFG_B, CFG_HW = 3, (5, 7)
CFG_SIGMAS = [0.03, 80.0, 2.5]                   # per image
COND_SCALES = [7.0, 1.0, 0.0, -1.5]
CFG_GEOS = [(4, 4), (4, 8), (3, 3), (3, 8)]      # (c, ld_eps): the out head pads to 8


@lru_cache(maxsize=None)
def cfg_case(reps, c, ld):
    """x at the scale a latent has at its sigma, eps N(0, 1) fp16 with 30000 in the padding columns; one case per geometry (every prediction type, sigma_data
    and cond_scale reads the same inputs)"""
    g = gen(300 + 10 * reps + c + ld)
    h, w = CFG_HW
    sigma = torch.tensor(CFG_SIGMAS)
    x = torch.randn(CFG_B, c, h, w, generator=g) * torch.sqrt(1 + sigma * sigma).view(-1, 1, 1, 1)
    eps = torch.full((reps * CFG_B, h, w, ld), 30000.0, dtype=H16)
    eps[..., :c] = torch.randn(reps * CFG_B, h, w, c, generator=g).half()
    return Win(eps, 2, 1), Win(x, 1, 3), Win(sigma, 2, 1)


def cfg_variants():
    """(c, ld, cond_scale, cond_pred present, uncond_pred present) of one (prediction type, reps, sigma_data) test"""
    return [(c, ld, cs, cp, up) for c, ld in CFG_GEOS for cs in COND_SCALES for cp in (False, True) for up in (False, True)]


@pytest.mark.parametrize("sd", SIGMA_DATAS)
@pytest.mark.parametrize("reps", [1, 2])
@pytest.mark.parametrize("ptype", PTYPES)
def test_cfg_combine(ptype, reps, sd):
    """denoised, cond_pred and uncond_pred within their derived bounds of the fp64 formula for every geometry, cond_scale and combination of optional
    outputs; with one half uncond_pred is exactly 0"""
    worst = {"denoised": 0.0, "preds": 0.0}
    for c, ld, cs, cp, up in cfg_variants():
        eps, x, sigma = cfg_case(reps, c, ld)
        what = f"cfg_combine {ptype} reps {reps} sigma_data {sd} c {c} ld {ld} cond_scale {cs} preds {cp}/{up}"
        outs = [Out(x.shape, F32, 1 + k, 1) for k in range(3)]
        den, cond, unc = (o.on(DEV) for o in outs)
        ops.cfg_combine(eps.on(DEV), ld, x.on(DEV), sigma.on(DEV), reps, cs, denoised=den, cond_pred=cond if cp else None,
                        uncond_pred=unc if up else None, prediction_type=ptype, sigma_data=sd)
        torch.cuda.synchronize()
        untouched(what, eps, x, sigma, *outs)
        want_den, want_c, want_u, b_den, b_c, b_u = R.cfg_combine_ref(eps.values, x.values, sigma.values, reps, cs, ptype, sd)
        worst["denoised"] = max(worst["denoised"], R.excess_abs(den, want_den, b_den))
        R.assert_within_bound(den, want_den, b_den, what)
        for present, got, o, want, bound, name in ((cp, cond, outs[1], want_c, b_c, "cond_pred"), (up, unc, outs[2], want_u, b_u, "uncond_pred")):
            if not present:
                assert torch.equal(bits(o.dbuf.cpu()), bits(o.buf)), f"{what}: absent {name} written"
            elif name == "uncond_pred" and reps == 1:
                assert int((bits(got.cpu()) != 0).sum()) == 0, f"{what}: uncond_pred is not exactly 0"
            else:
                worst["preds"] = max(worst["preds"], R.excess_abs(got, want, bound))
                R.assert_within_bound(got, want, bound, f"{what} {name}")
    measured("cfg_combine denoised", f"{ptype} reps={reps} sd={sd}", worst["denoised"])
    measured("cfg_combine preds", f"{ptype} reps={reps} sd={sd}", worst["preds"])


# ---- euler_step, lincomb3 ---------------------------------------------------------------------------------------------------------------------------
STEP_NS = [1, 3, 255, 256, 257, 4099]
EULER_STEPS = [(14.6146, 10.3), (0.6, 0.0292), (0.0292, 0.0)]        # (sigma, sigma_next); the last one is the last step
EULER_NOISE = [None, 0.7]                                              # noise_scale (None: no noise tensor)


@lru_cache(maxsize=None)
def step_case(n):
    """x, denoised, old_denoised, noise: flat fp32 of n elements"""
    g = gen(400 + n)
    return tuple(Win(torch.randn(n, generator=g) * s, 1 + k, 1) for k, s in enumerate((4.0, 1.0, 1.0, 1.0)))


def _dpmpp_2m(sigma_prev, sigma, sigma_next):
    """(a, b, c) of the DPM++ 2M update as k_diffusion/sampling.py passes them to lincomb3"""
    t_prev, t, t_next = (-math.log(s) for s in (sigma_prev, sigma, sigma_next))
    h, e = t_next - t, -math.expm1(-(t_next - t))
    r = (t - t_prev) / h
    return sigma_next / sigma, e * (1 + 1 / (2 * r)), -e / (2 * r)


# (a, b, c, old_denoised present): k_model.py:288 x - out * sigma; k_model.py:306 (1 - s) uncond + s cond; DPM++ 2M first / later steps; c == 0 with a tensor
LINCOMB3_COEFS = [(1.0, -14.6146, 0.0, False), (1.0, -0.0292, 0.0, False), (1.0 - 7.0, 7.0, 0.0, False), (0.705, 0.295, 0.0, False),
                  _dpmpp_2m(20.0, 14.6146, 10.3) + (True,), _dpmpp_2m(0.9, 0.6, 0.0292) + (True,), (0.5, 1.25, 0.0, True)]


@pytest.mark.parametrize("n", STEP_NS)
def test_euler_step(n):
    x, den, _, noise = step_case(n)
    worst = 0.0
    for sigma, sigma_next in EULER_STEPS:
        for ns in EULER_NOISE:
            what = f"euler_step n {n} sigma {sigma} -> {sigma_next} noise_scale {ns}"
            out = Out((n,), F32, 2, 2)
            nz = None if ns is None else noise
            got = ops.euler_step(x.on(DEV), den.on(DEV), sigma, sigma_next, noise=None if nz is None else nz.on(DEV), noise_scale=ns or 0.0, out=out.on(DEV))
            torch.cuda.synchronize()
            untouched(what, x, den, out, *([] if nz is None else [nz]))
            want, bound = R.euler_step_ref(x.values, den.values, sigma, sigma_next, None if nz is None else nz.values, ns or 0.0)
            worst = max(worst, R.excess_abs(got, want, bound))
            R.assert_within_bound(got, want, bound, what)
    measured("euler_step", f"n={n}", worst)


@pytest.mark.parametrize("n", STEP_NS)
def test_lincomb3(n):
    x, d0, d1, _ = step_case(n)
    worst = 0.0
    for a, b, c, old in LINCOMB3_COEFS:
        what = f"lincomb3 n {n} coefficients {a, b, c} old_denoised {old}"
        out = Out((n,), F32, 1, 2)
        got = ops.lincomb3(x.on(DEV), d0.on(DEV), d1.on(DEV) if old else None, a, b, c, out=out.on(DEV))
        torch.cuda.synchronize()
        untouched(what, x, d0, out, *([d1] if old else []))
        want, bound = R.lincomb3_ref(x.values, d0.values, d1.values if old else None, a, b, c)
        worst = max(worst, R.excess_abs(got, want, bound))
        R.assert_within_bound(got, want, bound, what)
    measured("lincomb3", f"n={n}", worst)


# ---- lincomb ----------------------------------------------------------------------------------------------------------------------------------------
LINCOMB_NS = [1, 3, 4, 5, 1023, 1024, 1025, 4099]
TO_D = 0.0292                                     # the 1 / sigma, -1 / sigma pair of to_d at the last sigma: cancels heavily
LINCOMB_COEFS = {"mixed": [0.7, -1.3, 0.25, 31.0, -0.5, 1.25e-3, 1.5, -0.75],
                 "to_d": [1 / TO_D, -1 / TO_D, 0.25, 2.0, -0.5, 0.125, 1.5, -0.75]}


@lru_cache(maxsize=None)
def lincomb_case(n):
    """eight fp32 sources of n elements; source 1 is source 0 less a denoising-sized difference (x and denoised at sigma 0.0292)"""
    g = gen(500 + n)
    srcs = [torch.randn(n, generator=g) * s for s in (3.0, 1.0, 1.0, 0.1, 5.0, 100.0, 1.0, 2.0)]
    srcs[1] = srcs[0] - TO_D * srcs[1]
    return [Win(s, 1 + k % 3, 1) for k, s in enumerate(srcs)]


@pytest.mark.parametrize("n", LINCOMB_NS)
def test_lincomb(n):
    """1 .. 8 terms, two coefficient sets, at sizes around a float4 and a block"""
    srcs = lincomb_case(n)
    worst = 0.0
    for name, coefs in LINCOMB_COEFS.items():
        for k in range(1, 9):
            what = f"lincomb n {n} terms {k} {name}"
            out = Out((n,), F32, 2, 1)
            got = ops.lincomb([s.on(DEV) for s in srcs[:k]], coefs[:k], out=out.on(DEV))
            torch.cuda.synchronize()
            untouched(what, out, *srcs[:k])
            want, bound = R.lincomb_ref([s.values for s in srcs[:k]], coefs[:k])
            worst = max(worst, R.excess_abs(got, want, bound))
            R.assert_within_bound(got, want, bound, what)
    measured("lincomb", f"n={n}", worst)


@pytest.mark.parametrize("alias", ["first", "last"])
@pytest.mark.parametrize("n", LINCOMB_NS)
def test_lincomb_in_place(n, alias):
    """x_out aliasing srcs[0] and aliasing a later source (include/fmx.h allows both): same bound, and the surroundings of the aliased buffer survive"""
    srcs = lincomb_case(n)
    worst = 0.0
    for k in (2, 5, 8):
        dev = [s.on(DEV) for s in srcs[:k]]
        dst = 0 if alias == "first" else k - 1
        want, bound = R.lincomb_ref([s.values for s in srcs[:k]], LINCOMB_COEFS["to_d"][:k])
        got = ops.lincomb(dev, LINCOMB_COEFS["to_d"][:k], out=dev[dst])
        torch.cuda.synchronize()
        assert got.data_ptr() == dev[dst].data_ptr()
        untouched(f"lincomb in place n {n} terms {k}", *srcs[:k])
        worst = max(worst, R.excess_abs(got, want, bound))
        R.assert_within_bound(got, want, bound, f"lincomb in place ({alias}) n {n} terms {k}")
        for j in range(k):
            assert j == dst or torch.equal(bits(dev[j].cpu()), bits(srcs[j].values)), "a source that is not the destination changed"
    measured("lincomb", f"n={n} in place {alias}", worst)


def test_lincomb_refuses_unaligned_pointers():
    """a source or the output one element off 16-byte alignment: the call fails on the host (FMX_REQUIRE), nothing is launched or written"""
    n = 64
    buf = [torch.full((n + 8,), 1.0, device=DEV) for _ in range(3)]
    out = Out((n,), F32, 1, 1)
    dst = out.on(DEV)
    with pytest.raises(_lib.FmxError, match="unaligned source"):
        ops.lincomb([buf[0][:n], buf[1][1:n + 1]], [1.0, 2.0], out=dst)
    with pytest.raises(_lib.FmxError, match="unaligned source"):
        ops.lincomb([buf[0][1:n + 1]], [1.0], out=dst)
    with pytest.raises(_lib.FmxError, match="unaligned output"):
        ops.lincomb([buf[0][:n], buf[1][:n]], [1.0, 2.0], out=buf[2][1:n + 1])
    torch.cuda.synchronize()
    assert torch.equal(bits(out.dbuf.cpu()), bits(out.buf)) and bool((buf[2] == 1.0).all())


# ---- error_norm -------------------------------------------------------------------------------------------------------------------------------------
ERRNORM_NS = [1, 255, 256, 257, 65536, 65537, 200003]
ERRNORM_KINDS = ["mixed", "equal", "last_heavy"]
ERR_ATOL, ERR_RTOL = 0.0078, 0.05


@lru_cache(maxsize=None)
def errnorm_case(n, kind):
    """x_low, x_high, x_prev.  Magnitudes spread over 1e-3 .. 30 so that delta is atol on some elements and rtol * |x_low| or rtol * |x_prev| on others
    (x_prev is the larger one on about half of them); "equal": x_high == x_low; "last_heavy": the last element alone carries most of the norm"""
    g = gen(600 + n)
    mag = torch.exp(torch.empty(n).uniform_(math.log(1e-3), math.log(30.0), generator=g))
    lo = torch.randn(n, generator=g) * mag
    pv = torch.randn(n, generator=g) * mag * torch.exp(torch.empty(n).uniform_(-3.0, 3.0, generator=g))
    hi = lo + 0.02 * mag * torch.randn(n, generator=g)
    if kind == "equal":
        hi = lo.clone()
    if kind == "last_heavy":
        lo[-1], pv[-1] = 0.001, 0.002                      # delta = atol
        hi[-1] = lo[-1] + ERR_ATOL * 40.0 * math.sqrt(n)
    return Win(lo, 1, 1), Win(hi, 2, 1), Win(pv, 3, 1)


@pytest.mark.parametrize("kind", ERRNORM_KINDS)
@pytest.mark.parametrize("n", ERRNORM_NS)
def test_error_norm(n, kind):
    """within the derived relative bound of the fp64 norm; two calls give the same bits; x_low == x_high gives exactly 0"""
    lo, hi, pv = errnorm_case(n, kind)
    got = ops.error_norm(lo.on(DEV), hi.on(DEV), pv.on(DEV), ERR_ATOL, ERR_RTOL)
    again = ops.error_norm(lo.view(lo.dbuf), hi.view(hi.dbuf), pv.view(pv.dbuf), ERR_ATOL, ERR_RTOL)
    untouched("error_norm", lo, hi, pv)
    want = R.error_norm_ref(lo.values, hi.values, pv.values, ERR_ATOL, ERR_RTOL)
    assert got == again, "the reduction is not deterministic"
    if kind == "equal":
        measured("error_norm", f"n={n} {kind}", 0.0)
        assert got == 0.0 and want == 0.0
        return
    e = measured("error_norm", f"n={n} {kind}", abs(got - want) / (R.error_norm_rel_bound(n) * want))
    assert e <= 1.0, f"error_norm n {n} {kind}: {got} against {want}, {e:.3g}x the derived relative bound"


# ---- philox_randn -----------------------------------------------------------------------------------------------------------------------------------
PHILOX_NS = [1, 5, 257, 16384]
PHILOX_SEEDS = [0x1234567800000005, 12345]
PHILOX_OFFSETS = [0, 2 ** 32 - 1]


@pytest.mark.parametrize("n", PHILOX_NS)
def test_philox_randn(n):
    """raw words bit-exact against oracle/rng.py (a seed with a non-zero high word, offsets 0 and 2^32 - 1), normals within 2e-6 of the host's Box-Muller,
    with and without the raw output; once per size straight into windows of sentinel buffers"""
    from oracle.rng import philox_randn
    worst = 0.0
    for seed in PHILOX_SEEDS:
        for offset in PHILOX_OFFSETS:
            want_raw, want = R.philox_raw_ref(seed, offset, n), philox_randn(seed, offset, n)
            out, raw = ops.philox_randn(seed, offset, n, DEV, want_raw=True)
            only = ops.philox_randn(seed, offset, n, DEV, want_raw=False)
            np.testing.assert_array_equal(raw.cpu().numpy().view(np.uint32), want_raw)
            assert torch.equal(bits(out), bits(only)), "the normals depend on want_raw"
            diff = float(np.abs(out.cpu().numpy().astype(np.float64) - want.astype(np.float64)).max())
            worst = max(worst, diff / R.PHILOX_ATOL)
            np.testing.assert_allclose(out.cpu().numpy(), want, rtol=0, atol=R.PHILOX_ATOL)
    seed, offset = PHILOX_SEEDS[0], PHILOX_OFFSETS[1]
    o, r = Out((n,), F32, 1, 1), Out((n, 4), torch.int32, 2, 1)
    do, dr = o.on(DEV), r.on(DEV)
    _lib.check(_lib.lib().fmx_philox_randn(C.c_uint64(seed), C.c_uint32(offset), do.data_ptr(), dr.data_ptr(), n, ops.stream_ptr()), "fmx_philox_randn")
    torch.cuda.synchronize()
    untouched("philox_randn", o, r)
    np.testing.assert_array_equal(dr.cpu().numpy().view(np.uint32), R.philox_raw_ref(seed, offset, n))
    np.testing.assert_allclose(do.cpu().numpy(), philox_randn(seed, offset, n), rtol=0, atol=R.PHILOX_ATOL)
    measured("philox_randn", f"n={n}", worst)
