"""References for native ControlNet-LLLite (tests/test_lllite_host.py on the CPU, tests/test_gpu_lllite.py on the MI355X): the fp64 restatement of
fmxl_lllite_adapt_f16 with its three declared roundings, the per-element bound it is held to, an fp32 emulation of the kernel's summation order,
the planted bugs the bound must catch, seeded kernel cases, and the inputs of the fixture (tests/golden/lllite.pt, tools/make_lllite_fixtures.py)
rebuilt from their seeds.

The bound is derived, not chosen.  The kernel rounds to fp16 at exactly three sites -- down's output d, mid's output m, the final output -- and
accumulates in fp32 in another order than the fp64 restatement, which can move a hidden value across a rounding boundary: by one fp16 ulp.  So an
element may differ from the fp64 value by
    ulp(out)  +  |mult| * ( sum_j |Wu[c, j]| ulp(m_j)  +  sum_j |Wu[c, j]| sum_i |Wm[j, E + i]| ulp(d_i) )
one output ulp (the final rounding and the fp32 epilogue), plus what a one-ulp flip of EVERY hidden value could move: a flip of m_j moves the
output by |Wu[c, j]| ulp(m_j); a flip of d_i moves the pre-activation of m_j by |Wm[j, E + i]| ulp(d_i), and ReLU is 1-Lipschitz.  ulp() is the
fp16 spacing at the value (2^-24 at and below the subnormals).
"""
import numpy as np
import torch

D, E = 64, 32
BUGS = ("mid_relu_dropped", "cat_halves_swapped", "cond_without_mod", "multiplier_dropped", "bu_dropped", "k_uses_q_weights")

# excess (max |got - fp64| / bound) measured on the CPU with the fp32 emulation (tests/test_lllite_host.py prints them again):
#   the emulation itself: worst 0.23 over every channel count, geometry, multiplier and slot of the GPU file's cases
#   the planted bugs at multiplier 0.35 on case (C 320, 4 images, n 64, Bc 2), the smallest of the three slots (the required factor is 4):
MEASURED_EXCESS = {"mid_relu_dropped": 216.9, "cat_halves_swapped": 208.4, "cond_without_mod": 110.7, "multiplier_dropped": 386.3, "bu_dropped": 22.6,
                   "k_uses_q_weights": 439.2}
TEETH_FACTOR = 4.0      # the convention of tests/test_kernel_ref_teeth.py


def ulp16(v):
    """fp16 spacing at |v| (fp64 tensor in, fp64 out): 2^(floor(log2 |v|) - 10), 2^-24 below the smallest normal"""
    a = v.abs().double().clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10.0)


def h16(v):
    """one rounding to fp16, back in fp64"""
    return v.to(torch.float16).double()


def cond_rows(cond, images, n, bug=None):
    """[images * n, E]: image i uses embedding i % Bc"""
    bc = cond.shape[0]
    idx = [min(i, bc - 1) if bug == "cond_without_mod" else i % bc for i in range(images)]      # the bug: the kernel would run past the embedding
    return cond[idx].reshape(images * n, -1)


def adapt_ref(x, cond, n, slot, mult, bug=None):
    """fp64 restatement with the three declared roundings -> (y fp64 [M, C]: the value BEFORE the final rounding, bound fp64 [M, C]).
    x [M, C] fp16, cond [Bc, n, E] fp16, slot: dict of fp16 wd bd wm bm wu bu."""
    xd = x.double()
    w = {k: slot[k].double() for k in ("wd", "bd", "wm", "bm", "wu", "bu")}
    images = x.shape[0] // n
    ce = cond_rows(cond, images, n, bug).double()
    d = h16(torch.relu(xd @ w["wd"].T + w["bd"]))
    cat = torch.cat([d, ce], 1) if bug == "cat_halves_swapped" else torch.cat([ce, d], 1)
    pre = cat @ w["wm"].T + w["bm"]
    m = h16(pre if bug == "mid_relu_dropped" else torch.relu(pre))
    up = m @ w["wu"].T + (0.0 if bug == "bu_dropped" else w["bu"])
    y = up * (1.0 if bug == "multiplier_dropped" else float(np.float32(mult))) + xd
    awu = w["wu"].abs()
    hidden = ulp16(m) @ awu.T + (ulp16(d) @ w["wm"][:, E:].abs().T) @ awu.T
    bound = ulp16(y) + abs(float(mult)) * hidden
    return y, bound


def adapt_emul32(x, cond, n, slot, mult, bug=None):
    """The kernel's arithmetic in fp32 on the CPU: every product accumulated over K in the MFMA's steps of 32 (fp32 partial dot products added in
    order), bias and ReLU in fp32, the two hidden roundings, and the epilogue (acc + bu) * mult + x as one fused multiply-add -> fp16 [M, C]"""
    def mm(a16, w16):
        acc = torch.zeros(a16.shape[0], w16.shape[0], dtype=torch.float32)
        for k0 in range(0, a16.shape[1], 32):
            acc = acc + a16[:, k0:k0 + 32].float() @ w16[:, k0:k0 + 32].float().T
        return acc
    images = x.shape[0] // n
    ce = cond_rows(cond, images, n, bug)
    d = torch.relu(mm(x, slot["wd"]) + slot["bd"].float()).half()
    cat = torch.cat([d, ce], 1) if bug == "cat_halves_swapped" else torch.cat([ce, d], 1)
    pre = mm(cat, slot["wm"]) + slot["bm"].float()
    m = (pre if bug == "mid_relu_dropped" else torch.relu(pre)).half()
    up = mm(m, slot["wu"])
    if bug != "bu_dropped":
        up = up + slot["bu"].float()
    mf = 1.0 if bug == "multiplier_dropped" else float(np.float32(mult))
    return (up.double() * mf + x.double()).float().half()       # the fused multiply-add: one rounding to fp32, then the rounding to fp16


def excess(got, y, bound):
    """max over the elements of |got - y| / bound"""
    return float(((got.double() - y).abs() / bound).max())


# ---- seeded kernel cases --------------------------------------------------------------------------------------------------------------------------------
CHANNELS = (320, 640, 1280)
GEOMETRIES = ((1, 64, 1), (4, 64, 2), (3, 128, 1), (4, 192, 4))       # (images, n, Bc)
MASKS = ((True, True, True), (True, False, False), (False, True, True))   # q|k|v, q only, k|v
MULTIPLIERS = (1.0, 0.35, 0.0)


def make_slot(c, seed):
    """weights at the scale of a trained, well-conditioned module: unit-variance rows in, unit-variance hidden values, an `up` whose result is of
    the order of x (a non-zero up: training starts it at zero, and a route that drops the adapter would pass)"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    return {"wd": (r(D, c) * (2.0 / c) ** 0.5).half(), "bd": (r(D) * 0.1).half(), "wm": (r(D, E + D) * (2.0 / (E + D)) ** 0.5).half(),
            "bm": (r(D) * 0.1).half(), "wu": (r(c, D) * (1.0 / D) ** 0.5).half(), "bu": (r(c) * 0.1).half()}


def make_case(c, images, n, bc, seed=0):
    """-> x [images * n, c] fp16 (LayerNorm-like rows), three cond embeddings [Bc, n, E] (one per slot, as every module has its own), three slots"""
    g = torch.Generator().manual_seed(1000 * seed + c + 7 * images + n + bc)
    x = torch.randn(images * n, c, generator=g).half()
    conds = [(torch.randn(bc, n, E, generator=g) * 0.7).half() for _ in range(3)]
    slots = [make_slot(c, 31 * seed + c + i) for i in range(3)]
    return x, conds, slots


# ---- the fixture's inputs ---------------------------------------------------------------------------------------------------------------------------------
def control_images(bc, size, seed):
    """[Bc, H, W, 3] fp32 in 0 .. 1: full-contrast waves of per-image frequencies plus noise, from a numpy stream (images that differ as much as two
    control images do: the embedding of one must not pass for the other's)"""
    rng = np.random.Generator(np.random.PCG64([seed, 41]))
    h, w = size
    yy, xx = np.meshgrid(np.linspace(0, 1, h, dtype=np.float32), np.linspace(0, 1, w, dtype=np.float32), indexing="ij")
    out = np.empty((bc, h, w, 3), dtype=np.float32)
    for i in range(bc):
        for ch in range(3):
            fx, fy, ph = rng.uniform(1.0, 6.0, 3)
            out[i, :, :, ch] = 0.5 + 0.5 * np.sin(2 * np.pi * (fx * xx + fy * yy) + ph) + 0.1 * rng.standard_normal((h, w), dtype=np.float32)
    return torch.from_numpy(np.clip(out, 0.0, 1.0))


def case_inputs(cfg, hw, seed, sigmas, b):
    """x fp32 [b, c, h, w] at the noise level of `sigmas`, cond, uncond of synth_conditioning(seed) -- numpy streams, rebuilt from the seed"""
    from forge_amd import synth
    rng = np.random.Generator(np.random.PCG64([seed, 11]))
    x = torch.from_numpy(rng.standard_normal((b, cfg["in_channels"], hw[0], hw[1]), dtype=np.float32))
    x = x * torch.sqrt(sigmas.float() ** 2 + 1.0).view(-1, 1, 1, 1)
    c, uc = synth.synth_conditioning(b, cfg["context_dim"], cfg.get("adm_in_channels"), seed=seed)
    return x, c, uc


def counter_sequence(steps, start, end, calls):
    """what the reference's per-module counter does, call by call, restated for the host test's cross-check of the recorded sequences"""
    import math
    s0 = math.floor(steps * start) if start > 0 else 0
    s1 = math.floor(steps * end) if end > 0 else steps
    cur, out = 0, []
    for _ in range(calls):
        if steps <= 0:
            out.append(True)
            continue
        if cur < s0:
            cur += 1
            out.append(False)
            continue
        active = cur < s1
        cur += 1
        if cur >= steps:
            cur = 0
        out.append(active)
    return out
