"""fp64 restatements for the native IP-Adapter tests, shared by tests/test_ipadapter_host.py (CPU) and tests/test_gpu_ipadapter.py.

The kernel (include/fmx_ipadapter.h):   O = attention(q, k_text, v_text) + sum_s w_s * attention(q, xk[group, seg_s], xv[group, seg_s])
with kernel_refs.attn_ref per term on the rounded inputs, an independent softmax per segment, image b reading group b // images_per_group.
Bound per element: 2 ulp(O) + 2 * EPS[fp16] * (1 + sum |w_s|) -- kernel_refs.ATTN_TOL with its floor scaled by the number of weighted terms, each of
which carries one rounding of its probabilities to fp16 (relative 2^-11 of weights <= |w_s|, on values of the O(1) scale the cases draw).

The patch (lib_ipadapter/IPAdapterPlus.py CrossAttentionPatch.__call__), `patch_ref`: the same sum with the reference's three weight types."""
import math

import torch

import kernel_refs as R

H16 = torch.float16
TEETH_FACTOR = 4.0      # the convention of tests/test_kernel_ref_teeth.py
D = 64
XKEYS = 64

# the shapes of the kernel test: batch 4 = 2 groups x 2 images, 2 heads
BATCH, GROUPS, HEADS = 4, 2, 2
NQS = (64, 200, 320)          # one tile; a ragged tile; a tile change inside a workgroup's walk
NKS = (1, 77, 128)
SEGMENTS = {                  # name -> [(start, count)]
    "base4": [(0, 4)],
    "plus16": [(0, 16)],
    "two_units": [(0, 4), (4, 16)],
    "one_key": [(0, 1)],
    "four_of_16": [(0, 16), (16, 16), (32, 16), (48, 16)],
    "offset_nan_outside": [(20, 16)],
}
WEIGHTS = (0.0, 0.35, 1.0, -0.5, 2.5)
SURROUND = 30000.0            # what lies around Q and K
VT_PAD = -3.0                 # finite, in the V^T pads and in the extra V^T outside the segments


def weights_of(name, w):
    """the weights of a case's segments: the first carries `w`, the others walk on through WEIGHTS (so one of several may be 0)"""
    i = WEIGHTS.index(w)
    return [WEIGHTS[(i + j) % len(WEIGHTS)] for j in range(len(SEGMENTS[name]))]


def make_case(nq, nk, name, seed=0):
    """-> dict of fp16 CPU tensors: q [B, nq, H, D], k / v [B, nk, H, D], xk / xv [G, 64, H, D] (NaN in the xk rows outside the segments of the
    `offset_nan_outside` case, random elsewhere: a key outside every segment must not matter either way)"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * nq + nk + 13 * sorted(SEGMENTS).index(name))
    rn = lambda *s: torch.randn(*s, generator=g).to(H16)  # noqa: E731
    c = {"q": rn(BATCH, nq, HEADS, D), "k": rn(BATCH, nk, HEADS, D), "v": rn(BATCH, nk, HEADS, D), "xk": rn(GROUPS, XKEYS, HEADS, D) * 1.5,
         "xv": rn(GROUPS, XKEYS, HEADS, D), "segments": list(SEGMENTS[name]), "nq": nq, "nk": nk, "name": name}
    if name == "offset_nan_outside":
        inside = torch.zeros(XKEYS, dtype=torch.bool)
        for s, n in c["segments"]:
            inside[s:s + n] = True
        c["xk"][:, ~inside] = math.nan
    return c


def _bhnd(t):
    return t.permute(0, 2, 1, 3).double()


def dual_terms(c, scale, images_per_group=BATCH // GROUPS, bug=None):
    """-> (text [B, H, nq, D] fp64, [segment terms, unweighted]).  bug: None, or 'swap_groups' (image b reads the other group)"""
    q, k, v = _bhnd(c["q"]), _bhnd(c["k"]), _bhnd(c["v"])
    text = R.attn_ref(q, k, v, scale)
    grp = torch.arange(q.shape[0]) // images_per_group
    if bug == "swap_groups":
        grp = (c["xk"].shape[0] - 1) - grp
    xk, xv = _bhnd(c["xk"])[grp], _bhnd(c["xv"])[grp]
    return text, [R.attn_ref(q, xk[:, :, s:s + n], xv[:, :, s:s + n], scale) for s, n in c["segments"]]


def dual_ref(c, weights, scale, bug=None):
    """fp64 reference of fmxi_attention_dual_f16 on the case -> [B, H, nq, D].  bug plants one of the mistakes the bound must tell from the
    kernel: 'joint_softmax' (one softmax over text and image keys, the image probabilities weighted), 'one_softmax_for_all_segments' (one softmax
    over all segments' keys), 'swap_groups', 'weight_before_softmax' (the weight scales the scores instead of the output)"""
    q = _bhnd(c["q"])
    grp = torch.arange(q.shape[0]) // (q.shape[0] // c["xk"].shape[0])
    xk, xv = _bhnd(c["xk"])[grp], _bhnd(c["xv"])[grp]
    if bug == "joint_softmax":
        k, v = _bhnd(c["k"]), _bhnd(c["v"])
        ks = torch.cat([k] + [xk[:, :, s:s + n] for s, n in c["segments"]], 2)
        vs = torch.cat([v] + [xv[:, :, s:s + n] * w for (s, n), w in zip(c["segments"], weights)], 2)
        return R.attn_ref(q, ks, vs, scale)
    if bug == "one_softmax_for_all_segments":
        text, _ = dual_terms(c, scale)
        ks = torch.cat([xk[:, :, s:s + n] for s, n in c["segments"]], 2)
        vs = torch.cat([xv[:, :, s:s + n] * w for (s, n), w in zip(c["segments"], weights)], 2)
        return text + R.attn_ref(q, ks, vs, scale)
    if bug == "weight_before_softmax":
        text, _ = dual_terms(c, scale)
        return text + sum(R.attn_ref(q, xk[:, :, s:s + n], xv[:, :, s:s + n], scale * w) for (s, n), w in zip(c["segments"], weights))
    text, terms = dual_terms(c, scale, bug=bug)
    return text + sum(w * t for w, t in zip(weights, terms))


def dual_bound(want, weights):
    """per element: 2 ulp(O) + 2 EPS[fp16] (1 + sum |w_s|)"""
    return 2.0 * R.ulp(want, H16) + 2.0 * R.EPS[H16] * (1.0 + sum(abs(w) for w in weights))


def excess(got, want, bound):
    """max |got - want| / bound; a non-finite got is infinitely wrong"""
    err = (got.double() - want.double()).abs() / bound
    return float(err.nan_to_num(nan=math.inf).max())


# ---- the patch ------------------------------------------------------------------------------------------------------------------------------------------
def patch_ref(q, k, v, heads, units, cond_or_uncond):
    """fp64 restatement of CrossAttentionPatch.__call__ (no mask, one reference image): q [B, N, C], k / v [B, Nk, C];
    units: [(cond tokens [1, T, Cc], uncond tokens, to_k_ip weight [C, Cc], to_v_ip weight, weight, weight_type)] -> [B, N, C]"""
    def heads_of(t):
        return t.double().view(t.shape[0], t.shape[1], heads, -1).transpose(1, 2)

    def attend(qq, kk, vv):
        o = R.attn_ref(heads_of(qq), heads_of(kk), heads_of(vv), (qq.shape[-1] // heads) ** -0.5)
        return o.transpose(1, 2).reshape(qq.shape[0], qq.shape[1], -1)

    per = q.shape[0] // len(cond_or_uncond)
    out = attend(q, k, v)
    for cond, uncond, wk, wv, weight, weight_type in units:
        toks = torch.cat([(cond, uncond)[i].double().repeat(per, 1, 1) for i in cond_or_uncond])
        ik, iv = toks @ wk.double().T, toks @ wv.double().T
        factor = 1.0
        if weight_type == "linear":
            ik, iv = ik * weight, iv * weight
        elif weight_type == "channel":
            mean = iv.mean(1, keepdim=True)
            w = weight * (ik.shape[-1] / 1280.0)
            ik, iv = ik * w, (iv - mean) + mean * w
        else:
            factor = weight
        out = out + attend(q, ik, iv) * factor
    return out
