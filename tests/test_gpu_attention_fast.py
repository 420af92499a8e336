"""GPU (MI355X) parity of the 64-query attention kernels behind fmx_attention_f16 / _bf16 (csrc/fmx_attention.hip): every unmasked, non-causal call at
d_head 64 / 128 with >= 256 queries -- attn_short2_kernel<1..4> (d 64, <= 128 keys), attn_q64v3_kernel (d 64, <= 4 key tiles), attn_q64v2_kernel<64> (whole
workgroups, key-split workgroups and both in one launch), attn_ws_kernel<128>, attn_q64v2_kernel<128> (key-split only) and the ws launch with a key-split
tail behind it.  Which kernel a shape reaches depends on the CU count (kernel_refs.attn_route restates the dispatcher's rule, attn_plan; tests/
test_kernel_ref_teeth.py compares the two over a sweep of shapes through fmx_attention_route); the case list is sized for 256 CUs, and that file asserts
that it reaches every route in both element types.  Here the CU count is read from the device, the library's route for it must equal the restated one and
is printed per case; on another part the values are still checked and nothing is asserted about which route a case was listed under.

Spans that do not fit the 64-query kernels' 32-bit byte offsets (K / V^T of a (batch, head) >= 2e9 bytes, or Q under at most 128 keys) go to the generic
32-query kernel, which addresses with 64-bit pointers: test_large_span_falls_back_to_the_generic_kernel.  The generic kernel's own cases (masks, causal,
d_head 48 / 80 / 160, fewer than 256 queries) are tests/test_gpu_attention_generic.py.

Reference: kernel_refs.attn_ref in fp64 on the rounded inputs, on the device in slices of <= 2^25 scores; every element within kernel_refs.ATTN_TOL; each
check prints "[attention excess] <route> <layout> <case>: x.xxx".  Layouts are the executors' (backend/nn/unet.py self- and cross-attention, backend/nn/
flux.py): in every non-dense layout the surroundings of q / k hold 30000, the V^T pad columns [nk, nk_pad) a finite -3, and O is a window of a larger
sentinel-filled buffer of which every element outside the window must come back bit-identical.  The case builders run on the CPU:
tests/test_kernel_ref_teeth.py plants bugs into kernel_refs.attn64_emul and into these builders on the same inputs."""
import ctypes as C
import math
from types import SimpleNamespace as NS

import pytest
import torch

pytestmark = pytest.mark.gpu

import forge_amd  # noqa: E402,F401
from forge_amd import hipops as ops  # noqa: E402

import kernel_refs as R  # noqa: E402
import test_gpu_attention_generic as G  # noqa: E402

DEV = "cuda"
H16, BF = torch.float16, torch.bfloat16
DTS = [H16, BF]
GARBAGE, VPAD, SENTINEL, GUARD = 30000.0, -3.0, -777.0, 2     # GUARD: rows of surroundings in front of and behind every non-dense buffer
LOG2E = 1.44269504088896340736
QSCALE = 1.0


def gen(seed):
    return torch.Generator("cpu").manual_seed(seed)


def pad64(n):
    return -(-n // 64) * 64


# ---- values ----------------------------------------------------------------------------------------------------------------------------------------
KEY_GAIN = 1.5     # a planted key is at most this multiple of its query row: every OTHER query's score with it carries the rounding of the pre-scaled Q at |k| size


def _plant(q, k, d, qi, targets):
    """targets [(key, log2 score)]: each key becomes a multiple of query row qi that scores the target (log2 domain: what the kernels' maximum sees).  The
    multiple is split: the keys take at most KEY_GAIN, the query row itself is scaled by the rest."""
    targets = [(key, t) for key, t in targets if 0 <= key < k.shape[1]]
    row = q[:, qi].float()
    unit = (row * row).sum(-1) * (d ** -0.5) * LOG2E
    gain = (max(t for _, t in targets) / unit / KEY_GAIN).clamp_min(1.0)
    q[:, qi] = (row * gain[..., None]).to(q.dtype)
    for key, t in targets:
        k[:, key] = (row * (t / unit / gain)[..., None]).to(k.dtype)


def values(b, h, nq, nk, d, dtype, seed, structure=None):
    """logical q [B, nq, H, d], k / v [B, nk, H, d] in `dtype`.  structure: None (random), or one of
    negative        every score far below zero: the first step must set a negative maximum exactly
    staircase       query 100's maximum climbs 5 log2 units per 64-key tile (below the 2^6 threshold each time, above it every second), query 101's by 7
    threshold_edge  query 7's maximum climbs by 5.9, 6.1, 0.5, 6.0, 12, 5.9 ... per tile, alternately in the first and second 32-key sub-tile
    dominant        dominant keys in the first tile (query 3), in the LAST valid key at 2^200 (query 5: an unmoved maximum overflows every format), on
                    both sides of the first 32-key edge (queries 9, 10) and at the first key of the last 32-key sub-tile (query 12)
    dom_lower / dom_upper   (key-split) a key at 2^30 (query 7) and one at 2^140 (query 9: the other half's merge weight underflows) in that half only
    equal_halves    (key-split) the upper half of K repeats the lower half: both halves arrive with the same maximum and row sum"""
    g = gen(seed)
    q = (torch.randn(b, nq, h, d, generator=g) * QSCALE).to(dtype)
    k = torch.randn(b, nk, h, d, generator=g).to(dtype)
    v = torch.randn(b, nk, h, d, generator=g).to(dtype)
    nt = -(-nk // 64)
    half = nt // 2 * 64
    if structure == "negative":
        q, k = q.abs(), (-(k.float().abs()) - 0.5).to(dtype)
    elif structure == "staircase":
        _plant(q, k, d, 100, [(t * 64 + 5, 4.0 + 5.0 * t) for t in range(nt)])
        _plant(q, k, d, 101, [(t * 64 + 37, 4.0 + 7.0 * t) for t in range(nt)])
    elif structure == "threshold_edge":
        levels = torch.tensor((6.0, 5.9, 6.1, 0.5, 6.0, 12.0, 5.9, 6.1)).cumsum(0).tolist()
        _plant(q, k, d, 7, [(t * 64 + (1 if t % 2 == 0 else 33), levels[t]) for t in range(nt)])
    elif structure == "dominant":
        _plant(q, k, d, 3, [(3, 14.0)])
        _plant(q, k, d, 9, [(31, 14.0)])
        _plant(q, k, d, 10, [(32, 14.0)])
        _plant(q, k, d, 12, [((nk - 1) // 32 * 32, 20.0)])
        _plant(q, k, d, 5, [(nk - 1, 200.0)])
    elif structure == "dom_lower":
        _plant(q, k, d, 7, [(5, 30.0)])
        _plant(q, k, d, 9, [(70, 140.0)])
    elif structure == "dom_upper":
        _plant(q, k, d, 7, [(half + 5, 30.0)])
        _plant(q, k, d, 9, [(nk - 1, 140.0)])
    elif structure == "equal_halves":
        assert nk == 2 * half
        k[:, half:] = k[:, :half]
    elif structure is not None:
        raise KeyError(structure)
    return q, k, v


# ---- layouts ---------------------------------------------------------------------------------------------------------------------------------------
def layout(name, b, h, nq, nk, d, o_extra=8):
    """element offsets / strides of a launch in the buffers "q", "k" (may be the same buffer as "q"), "vt" and "o" -> namespace with
    sizes {buffer: elements}, kbuf (name of the buffer k lives in), q_off q_bs q_rs k_off k_bs k_rs vt_off vt_bs vt_hs vt_ds nk_pad o_off o_bs o_rs
    (o_rs None: no O buffer, the launch allocates a dense one).  Layouts as the executors launch them:
    dense       q [B][nq][H][d], k [B][nk_pad][H][d], vt [H][d][B][nk_pad]
    unet_self   backend/nn/unet.py:399-427: q | k the column halves of one [B * n_pad][2 hd] buffer, vt [hd][m_tok] with m_tok > B * n_pad, O a column window
                [B * nq][hd] of a buffer with rows of hd + o_extra
    unet_cross  unet.py:450: q [B * nq][hd], the cached context K [B * 128][hd] / V^T [hd][B * 128] with nk valid keys per image, O as unet_self
    flux        backend/nn/flux.py:151: q, k [B][l_pad][hd] with nq = nk = L < l_pad, vt [hd][B * l_pad], O [B][l_pad][hd] (o_bs = l_pad * hd)"""
    hd = h * d
    L = NS(name=name, b=b, h=h, nq=nq, nk=nk, d=d, kbuf="k")
    if name == "dense":
        nkp = pad64(nk)
        L.sizes = {"q": b * nq * hd, "k": b * nkp * hd, "vt": hd * b * nkp}
        L.q_off, L.q_bs, L.q_rs = 0, nq * hd, hd
        L.k_off, L.k_bs, L.k_rs = 0, nkp * hd, hd
        L.vt_off, L.vt_bs, L.vt_hs, L.vt_ds = 0, nkp, d * b * nkp, b * nkp
        L.nk_pad, L.o_off, L.o_bs, L.o_rs = nkp, 0, nq * hd, None
        return L
    if name == "unet_self":
        assert nq == nk
        nkp = pad64(nk)
        m_tok = b * nkp + 64
        L.kbuf = "q"
        L.sizes = {"q": (b * nkp + 2 * GUARD) * 2 * hd, "vt": hd * m_tok}
        L.q_off, L.q_bs, L.q_rs = GUARD * 2 * hd, nkp * 2 * hd, 2 * hd
        L.k_off, L.k_bs, L.k_rs = L.q_off + hd, nkp * 2 * hd, 2 * hd
        L.vt_off, L.vt_bs, L.vt_hs, L.vt_ds = 0, nkp, d * m_tok, m_tok
        L.vt_ds_wrong = b * nk                                        # (teeth) the row stride a reader would take from the token count
    elif name == "unet_cross":
        nkp = 128
        L.sizes = {"q": (b * nq + 2 * GUARD) * hd, "k": b * nkp * hd, "vt": hd * b * nkp}
        L.q_off, L.q_bs, L.q_rs = GUARD * hd, nq * hd, hd
        L.k_off, L.k_bs, L.k_rs = 0, nkp * hd, hd
        L.vt_off, L.vt_bs, L.vt_hs, L.vt_ds = 0, nkp, d * b * nkp, b * nkp
    elif name == "flux":
        assert nq == nk
        nkp = pad64(nk)
        L.sizes = {"q": (b * nkp + 2 * GUARD) * hd, "k": (b * nkp + 2 * GUARD) * hd, "vt": hd * b * nkp, "o": (b * nkp + 2 * GUARD) * hd}
        L.q_off, L.q_bs, L.q_rs = GUARD * hd, nkp * hd, hd
        L.k_off, L.k_bs, L.k_rs = GUARD * hd, nkp * hd, hd
        L.vt_off, L.vt_bs, L.vt_hs, L.vt_ds = 0, nkp, d * b * nkp, b * nkp
        L.nk_pad, L.o_off, L.o_bs, L.o_rs = nkp, GUARD * hd, nkp * hd, hd
        return L
    else:
        raise KeyError(name)
    o_rs = hd + o_extra
    L.sizes["o"] = (b * nq + 2 * GUARD) * o_rs
    L.nk_pad, L.o_off, L.o_bs, L.o_rs = nkp, GUARD * o_rs, nq * o_rs, o_rs
    return L


def _view(buf, L, which, rows):
    """[B, rows, H, d] view of the operand in its buffer"""
    b, h, d = L.b, L.h, L.d
    if which == "vt":
        return torch.as_strided(buf, (b, rows, h, d), (L.vt_bs, 1, L.vt_hs, L.vt_ds), L.vt_off)
    off, bs, rs = {"q": (L.q_off, L.q_bs, L.q_rs), "k": (L.k_off, L.k_bs, L.k_rs), "o": (L.o_off, L.o_bs, L.o_rs)}[which]
    return torch.as_strided(buf, (b, rows, h, d), (bs, rs, d, 1), off)


def fill(L, q, k, v, dtype, kpad="garbage"):
    """the launch's buffers (CPU): everything 30000 / sentinel first, then the V^T pad columns -3, then the operands through their views.
    kpad "nonfinite": K rows [nk, nk_pad) hold NaN, +inf and -inf in turn."""
    bufs = {n: torch.full((sz,), SENTINEL if n == "o" else GARBAGE).to(dtype) for n, sz in L.sizes.items()}
    kb = bufs[L.kbuf]
    if L.nk_pad > L.nk:
        _view(bufs["vt"], L, "vt", L.nk_pad)[:, L.nk:] = VPAD
        if kpad == "nonfinite":
            pad = _view(kb, L, "k", L.nk_pad)[:, L.nk:]
            pad[..., 0::3] = math.nan
            pad[..., 1::3] = math.inf
            pad[..., 2::3] = -math.inf
    _view(bufs["q"], L, "q", L.nq)[:] = q
    _view(kb, L, "k", L.nk)[:] = k
    _view(bufs["vt"], L, "vt", L.nk)[:] = v
    return bufs


def gather(bufs, L, q_from_k=False, vt_ds=None):
    """what a kernel reads through the launch's strides: q [B, nq, H, d], k / v [B, nk_pad, H, d] (pad rows included).  Teeth: q_from_k reads q at k's
    offset, vt_ds overrides the V^T row stride."""
    M = NS(**vars(L))
    if q_from_k:
        M.q_off = L.k_off
    if vt_ds is not None:
        M.vt_ds = vt_ds
    return _view(bufs["q"], M, "q", L.nq), _view(bufs[L.kbuf], M, "k", L.nk_pad), _view(bufs["vt"], M, "vt", L.nk_pad)


def window_violations(before, after, L):
    """number of elements of the O buffer outside the launch's window [B, nq, H * d] whose bits changed"""
    win = torch.zeros(before.numel(), dtype=torch.bool)
    _view(win, L, "o", L.nq)[:] = True
    return int((before.view(torch.int16)[~win] != after.view(torch.int16)[~win]).sum())


# ---- cases -------------------------------------------------------------------------------------------------------------------------------------------
# (id, route at 256 CUs, b, h, nq, nk, d, layout, structure, options)
def _c(route, b, h, nq, nk, d, lay="dense", structure=None, **opt):
    tag = f"{lay}-b{b}h{h}q{nq}k{nk}d{d}" + (f"-{structure}" if structure else "") + "".join(f"-{k}{v}" for k, v in opt.items())
    return NS(id=tag, route=route, b=b, h=h, nq=nq, nk=nk, d=d, layout=lay, structure=structure, opt=opt)


NQ_EDGES = (256, 257, 300, 511, 513)
CASES = []
# short2<NB>: nk on and next to every 32-key block, nq cycling through the edges; one launch of more tiles than 2 x CUs workgroups (they walk across
# (batch, head) changes and restage K / V^T)
for i, nk in enumerate((1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128)):
    CASES.append(_c(f"short2<{-(-nk // 32)}>", 2, 3, NQ_EDGES[i % 5], nk, 64))
CASES.append(_c("short2<3>", 3, 7, 128 * 25 + 5, 77, 64))
# q64v3: three key tiles at any grid, four tiles with 193 .. 511 entries
for i, nk in enumerate((129, 160, 161, 192)):
    CASES.append(_c("q64v3", 2, 3, NQ_EDGES[i % 5], nk, 64))
for nk in (193, 255, 256):
    CASES.append(_c("q64v3", 3, 7, 256 * 9 + 1, nk, 64))
# q64v2<64> whole: an odd number (>= 5) of key tiles
for i, nk in enumerate((257, 300, 319, 320, 385)):
    CASES.append(_c("q64v2<64> whole", 2, 3, NQ_EDGES[i % 5], nk, 64))
# q64v2<64>, every workgroup key-split: <= 192 entries, an even number (>= 4) of tiles; 193 / 321: ONE valid key in the upper half's last tile
for i, nk in enumerate((193, 250, 256, 321, 384, 500)):
    CASES.append(_c("q64v2<64> split", 2, 3, NQ_EDGES[i % 5], nk, 64))
CASES.append(_c("q64v2<64> whole+split", 2, 5, 52 * 256 - 37, 250, 64))          # 520 entries = one round of 512 + 8 as 16 key-split workgroups
# d_head 128
for i, nk in enumerate((77, 129, 192, 257, 320)):
    CASES.append(_c("ws<128>", 2, 3, NQ_EDGES[i % 5], nk, 128))
for i, nk in enumerate((193, 250, 256, 384)):
    CASES.append(_c("q64v2<128> split", 2, 3, NQ_EDGES[i % 5], nk, 128))
CASES.append(_c("ws<128>+split tail", 3, 11, 2048 - 37, 256, 128))                # 264 entries: 256 on the ws kernel, 8 as 16 key-split workgroups
# value structures on every route that keeps a deferred maximum (short2 takes one exact pass: it gets the dominant keys and the negative scores)
STRUCT_AT = [("q64v3", 192, 64), ("q64v2<64> whole", 300, 64), ("q64v2<64> split", 250, 64), ("ws<128>", 300, 128), ("q64v2<128> split", 250, 128)]
for route, nk, d in STRUCT_AT:
    for s in ("negative", "staircase", "threshold_edge", "dominant"):
        CASES.append(_c(route, 2, 2, 300, nk, d, structure=s))
    if route.endswith("split"):
        CASES += [_c(route, 2, 2, 300, nk, d, structure=s) for s in ("dom_lower", "dom_upper")] + [_c(route, 2, 2, 300, 256, d, structure="equal_halves")]
CASES += [_c("short2<3>", 2, 2, 300, 77, 64, structure=s) for s in ("negative", "dominant")]
CASES += [_c("q64v3", 3, 7, 256 * 9 + 1, 250, 64, structure="dominant"), _c("q64v2<64> whole+split", 2, 5, 52 * 256 - 37, 250, 64, structure="dominant"),
          _c("ws<128>+split tail", 3, 11, 2048 - 37, 256, 128, structure="dominant")]
# the executors' layouts
CASES += [_c("q64v2<64> split", 2, 3, 256, 256, 64, "unet_self", o_extra=8), _c("q64v2<64> split", 2, 3, 256, 256, 64, "unet_self", o_extra=4),
          _c("q64v2<64> whole", 2, 3, 320, 320, 64, "unet_self", o_extra=4), _c("q64v2<64> whole", 2, 3, 300, 300, 64, "unet_self", o_extra=8),
          _c("q64v2<64> split", 2, 3, 384, 384, 64, "unet_self", "dominant", o_extra=4), _c("q64v3", 6, 35, 256, 256, 64, "unet_self", o_extra=4),
          _c("q64v2<64> whole+split", 10, 52, 256, 256, 64, "unet_self", o_extra=8),
          _c("short2<3>", 2, 10, 513, 77, 64, "unet_cross", o_extra=8), _c("short2<2>", 2, 10, 300, 33, 64, "unet_cross", o_extra=4),
          _c("short2<3>", 3, 7, 128 * 25 + 5, 80, 64, "unet_cross", o_extra=4),
          _c("ws<128>", 2, 3, 300, 300, 128, "flux"), _c("q64v2<128> split", 1, 3, 333, 333, 128, "flux"), _c("ws<128>", 3, 24, 333, 333, 128, "flux"),
          _c("ws<128>+split tail", 3, 44, 333, 333, 128, "flux", "dominant")]
# K rows [nk, nk_pad) hold NaN / +-inf: keys >= nk are masked out whatever they hold (include/fmx.h)
CASES += [_c("short2<3>", 2, 3, 300, 77, 64, kpad="nonfinite"), _c("q64v3", 2, 3, 300, 161, 64, kpad="nonfinite"),
          _c("q64v2<64> whole", 2, 3, 300, 300, 64, kpad="nonfinite"), _c("q64v2<64> split", 2, 3, 300, 250, 64, kpad="nonfinite"),
          _c("ws<128>", 2, 3, 300, 300, 128, kpad="nonfinite"), _c("q64v2<128> split", 2, 3, 300, 250, 128, kpad="nonfinite"),
          _c("ws<128>+split tail", 3, 44, 333, 333, 128, "flux", kpad="nonfinite"), _c("q64v2<64> whole+split", 2, 5, 52 * 256 - 37, 250, 64, kpad="nonfinite")]
ROUTES = ("short2<1>", "short2<2>", "short2<3>", "short2<4>", "q64v3", "q64v2<64> whole", "q64v2<64> split", "q64v2<64> whole+split", "ws<128>",
          "q64v2<128> split", "ws<128>+split tail")
assert len({c.id for c in CASES}) == len(CASES)


def build(case, dtype):
    """-> (layout, buffers) of a case on the CPU"""
    c = case
    seed = 9000 + 7 * CASES.index(c) + (1 if dtype == BF else 0)
    q, k, v = values(c.b, c.h, c.nq, c.nk, c.d, dtype, seed, c.structure)
    L = layout(c.layout, c.b, c.h, c.nq, c.nk, c.d, **{k_: v_ for k_, v_ in c.opt.items() if k_ == "o_extra"})
    return L, fill(L, q, k, v, dtype, kpad=c.opt.get("kpad", "garbage"))


def reference(bufs, L, dev=DEV, **plant):
    """fp64 [B, H, nq, d] of what the launch's strides address (kernel_refs.attn_ref, in slices)"""
    q, k, v = gather(bufs, L, **plant)
    return G.reference(q, k, v, L.nk, L.d, dev=dev)


# ---- the GPU test ------------------------------------------------------------------------------------------------------------------------------------
FAKE_PTR = 0x7F0000001000      # a 16-byte aligned non-null "device pointer" for fmx_attention_route, which dereferences nothing


def library_route(lib, L, cus, **override):
    """the route name the library's own dispatch plan gives a launch of layout L on `cus` compute units (fmx_attention_route: host only, no device)"""
    from forge_amd import _lib
    a = _lib.AttnArgs()
    a.q = a.k = a.vt = a.o = a.zero_page = FAKE_PTR
    a.batch, a.heads, a.nq, a.nk, a.nk_pad, a.dpad, a.scale = L.b, L.h, L.nq, L.nk, L.nk_pad, L.d, L.d ** -0.5
    a.q_bs, a.q_rs, a.k_bs, a.k_rs, a.vt_bs, a.vt_hs, a.vt_ds = L.q_bs, L.q_rs, L.k_bs, L.k_rs, L.vt_bs, L.vt_hs, L.vt_ds
    a.o_bs, a.o_rs = L.o_bs, L.o_rs or L.h * L.d
    for k_, v_ in override.items():
        setattr(a, k_, v_)
    buf = C.create_string_buffer(64)
    _lib.check(lib.fmx_attention_route(C.byref(a), cus, buf, len(buf)), "fmx_attention_route")
    return buf.value.decode()


def cu_count():
    from forge_amd import _lib
    cus = C.c_int(0)
    _lib.check(_lib.lib().fmx_device_info(C.byref(cus), None, None, 0), "fmx_device_info")
    return cus.value


def launch(bufs, L):
    """-> (out [B, nq, H, d] on the device, O buffer after the launch on the CPU or None)"""
    dv = {n: t.to(DEV) for n, t in bufs.items()}
    out = None if L.o_rs is None else torch.as_strided(dv["o"], (L.nq, L.h * L.d), (L.o_rs, 1), L.o_off)
    res = ops.attention(dv["q"][L.q_off:], dv[L.kbuf][L.k_off:], dv["vt"][L.vt_off:], batch=L.b, heads=L.h, nq=L.nq, nk=L.nk, nk_pad=L.nk_pad, dpad=L.d,
                        scale=L.d ** -0.5, q_bs=L.q_bs, q_rs=L.q_rs, k_bs=L.k_bs, k_rs=L.k_rs, vt_bs=L.vt_bs, vt_hs=L.vt_hs, vt_ds=L.vt_ds, out=out,
                        o_bs=None if out is None else L.o_bs)
    torch.cuda.synchronize()
    if out is None:
        return res.view(L.b, L.nq, L.h, L.d), None
    return _view(dv["o"], L, "o", L.nq), dv["o"].cpu()


@pytest.mark.parametrize("dtype", DTS, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_fast_attention(case, dtype):
    cus = cu_count()
    route = R.attn_route(case.b, case.h, case.nq, case.nk, case.d, cus)
    if cus == 256:
        assert route == case.route, f"{case.id}: reaches {route}, listed under {case.route}"
    L, bufs = build(case, dtype)
    from forge_amd import _lib
    assert library_route(_lib.lib(), L, cus) == route, f"{case.id}: kernel_refs.attn_route says {route}"
    want = reference(bufs, L)
    assert bool(torch.isfinite(want).all())
    got, o_after = launch(bufs, L)
    e = R.excess(got.permute(0, 2, 1, 3), want, dtype, *R.ATTN_TOL[dtype])
    print(f"[attention excess] {route} {case.layout} {case.id} {'f16' if dtype == H16 else 'bf16'} ({cus} CUs): {e:.3f}")
    assert e <= 1.0, f"{case.id}: error {e:.3g}x ATTN_TOL[{dtype}] on {route}"
    if o_after is not None:
        assert window_violations(bufs["o"], o_after, L) == 0, f"{case.id}: the launch wrote outside its window of O"


# ---- spans beyond 32-bit byte offsets ------------------------------------------------------------------------------------------------------------------
# (name, nk, the stride that is stretched, its value in elements): b = h = 1, d 64, 256 queries.  The rows lie 2^24 (K) / 2^22 (Q) elements apart in a
# buffer of ~2.1 GB that is allocated but, apart from those rows, never written or read.
LARGE_SPAN = [("k_span", 64, "k_rs", 1 << 24),      # K rows 0 .. 63: 63 x 2^24 x 2 bytes >= 2e9
              ("q_span", 77, "q_rs", 1 << 22)]      # Q rows 0 .. 255 under <= 128 keys (short2 reads Q through a descriptor): 255 x 2^22 x 2 bytes >= 2e9


@pytest.mark.parametrize("dtype", DTS, ids=["f16", "bf16"])
@pytest.mark.parametrize("name,nk,which,stride", LARGE_SPAN, ids=[c[0] for c in LARGE_SPAN])
def test_large_span_falls_back_to_the_generic_kernel(name, nk, which, stride, dtype):
    """a K / V^T / Q span that the 64-query kernels' 32-bit offsets cannot address runs on the generic kernel (64-bit addresses), within its ATTN_TOL"""
    from forge_amd import _lib
    nq, d = 256, 64
    q, k, v = G.inputs(1, 1, nq, nk, d, dtype, seed=7700 + nk)
    L = layout("dense", 1, 1, nq, nk, d)
    setattr(L, which, stride)
    assert ((L.nk_pad - 1) * L.k_rs + d) * 2 >= 2e9 or ((nq - 1) * L.q_rs + d) * 2 >= 2e9
    cus = cu_count()
    assert library_route(_lib.lib(), layout("dense", 1, 1, nq, nk, d), cus) == R.attn_route(1, 1, nq, nk, d, cus) != "generic"
    assert library_route(_lib.lib(), L, cus) == "generic"
    want = G.reference(q, k, v, nk, d)
    rows = {"k_rs": k, "q_rs": q}[which][0, :, 0]
    big = torch.empty((rows.shape[0] - 1) * stride + d, dtype=dtype, device=DEV)
    torch.as_strided(big, tuple(rows.shape), (stride, 1)).copy_(rows)
    dq, dk = (big, k.to(DEV)) if which == "q_rs" else (q.to(DEV), big)
    vt = v.to(DEV).permute(2, 3, 0, 1).contiguous()
    out = ops.attention(dq, dk, vt, batch=1, heads=1, nq=nq, nk=nk, nk_pad=L.nk_pad, dpad=d, scale=d ** -0.5, q_bs=L.q_bs, q_rs=L.q_rs, k_bs=L.k_bs,
                        k_rs=L.k_rs, vt_bs=L.vt_bs, vt_hs=L.vt_hs, vt_ds=L.vt_ds)
    torch.cuda.synchronize()
    e = R.excess(out.view(1, nq, 1, d).permute(0, 2, 1, 3), want, dtype, *R.ATTN_TOL[dtype])
    print(f"[attention excess] generic large-span {name} {'f16' if dtype == H16 else 'bf16'}: {e:.3f}")
    del big, dq, dk
    torch.cuda.empty_cache()
    assert e <= 1.0, f"{name}: error {e:.3g}x ATTN_TOL[{dtype}] on the generic kernel"
