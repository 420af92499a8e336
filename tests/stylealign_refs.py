"""References for native StyleAlign (tests/test_stylealign_host.py on the CPU, tests/test_gpu_stylealign.py on the MI355X): the reference script's
patch written for this code base (the A/B baseline on the hooked executor; held to the real script's recorded outputs on the CPU), the fp64
shared attention, the rounding model of fmxe_attn_blend_f16, the inputs of the fixture cases rebuilt from their seeds, and the two plain forwards whose bits the fixture holds from before
the executor knew the option."""
import numpy as np
import torch


# ---- the script's patch, written for this code base ---------------------------------------------------------------------------------------------------
def cpu_attention(q, k, v, heads, mask=None):
    """multi-head attention on [rows, tokens, heads * d] CPU tensors through torch's fused op, which is what the reference's CPU runs reach"""
    def split(t):
        return t.unflatten(-1, (heads, -1)).movedim(-2, 1)       # [rows, heads, tokens, d]
    o = torch.nn.functional.scaled_dot_product_attention(split(q), split(k), split(v), attn_mask=mask)
    return o.movedim(1, -2).flatten(-2)


def stylealign_attn1_patch(strength, attention):
    """-> an attn1 replace patch (q, k, v, extra_options) -> o that does what forge_stylealign.py:51-86 does, on `attention(q, k, v, heads=, mask=)`.
    Per entry of extra_options["cond_or_uncond"] it takes the rows of that kind (cond_indices for 0, uncond_indices otherwise) as one group:
    the group's ordinary attention below the lower threshold, one attention over the group's joined tokens above the upper one, and between
    them the two blended as `(1.0 - strength) * ordinary + strength * joined` -- that expression and its operand order are the arithmetic
    under test (fp16 tensors times Python floats), so they are kept as the script has them.  Groups come back concatenated in entry order."""
    from forge_amd.backend.patcher.stylealign import mode_of
    mode = mode_of(strength)                       # the script's thresholds: "plain" < 0.01, "aligned" > 0.99, else "blend"

    def ordinary(group, heads):
        return attention(*group, heads=heads, mask=None)

    def joined(group, heads):
        images, tokens, width = group[0].shape
        as_one = [t.reshape(1, images * tokens, width) for t in group]
        return attention(*as_one, heads=heads, mask=None).reshape(images, tokens, -1)

    def patch(q, k, v, extra_options):
        heads = extra_options["n_heads"]
        rows_of = {True: extra_options["cond_indices"], False: extra_options["uncond_indices"]}
        out = []
        for kind in extra_options["cond_or_uncond"]:
            rows = rows_of[kind == 0]
            if len(rows) == 0:
                continue
            group = (q[rows], k[rows], v[rows])
            if mode == "plain":
                out.append(ordinary(group, heads))
            elif mode == "aligned":
                out.append(joined(group, heads))
            else:
                own, shared = ordinary(group, heads), joined(group, heads)
                out.append((1.0 - strength) * own + strength * shared)
        return torch.cat(out, dim=0)
    return patch


def python_stylealign(unet_patcher, strength):
    """-> a clone of `unet_patcher` with StyleAlign installed the way the reference script installs it: an attn1 replace patch on every block
    (set_model_replace_all), which sends every model call to the hooked executor; the attention inside it is this project's own"""
    from forge_amd.backend import attention
    m = unet_patcher.clone()
    m.set_model_replace_all(stylealign_attn1_patch(float(strength), attention.attention_function), "attn1")
    return m


# ---- fp64 ---------------------------------------------------------------------------------------------------------------------------------------------
def shared_attention_ref(q, k, v, heads, b, scale=None):
    """q [Bu, n, H * d], k, v [Bu, nk, H * d] -> fp64 [Bu, n, H * d]: softmax(Q K^T * scale) V over the joined tokens of every group of b
    consecutive images (b = 1: ordinary attention).  scale: default d ** -0.5; given by the caller when the heads are zero-padded beyond d."""
    bu, n, hd = q.shape
    d = hd // heads
    g = bu // b
    q, k, v = (t.double().reshape(g, b * t.shape[1], heads, d).transpose(1, 2) for t in (q, k, v))
    s = torch.softmax(q @ k.transpose(-1, -2) * (d ** -0.5 if scale is None else scale), dim=-1)
    return (s @ v).transpose(1, 2).reshape(bu, n, hd)


def blend_ref(own, shared, strength):
    """The rounding model of fmxe_attn_blend_f16 on fp16 CPU tensors: each product an fp32 multiply by the fp32 weight rounded to fp16, the sum an
    fp32 add rounded to fp16; w_own = fp32(1.0 - strength) with the subtraction in double, w_shared = fp32(strength)."""
    wo = torch.tensor(np.float32(1.0 - float(strength)))
    ws = torch.tensor(np.float32(float(strength)))
    pa = (own.float() * wo).half()
    pb = (shared.float() * ws).half()
    return (pa.float() + pb.float()).half()


def torch_blend(own, shared, strength):
    """the reference expression itself, on fp16 CPU tensors"""
    return (1.0 - strength) * own + strength * shared


def special_values():
    """fp16: +-0, the smallest and largest subnormals, the smallest normal, +-65504, +-inf, NaN -- and every pair of them"""
    bits = [0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x8400, 0x3C00, 0xBC00, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00, 0x3555, 0xB555]
    v = torch.tensor(bits, dtype=torch.int32).to(torch.int16).view(torch.float16)
    a = v.repeat_interleave(len(bits))
    b = v.repeat(len(bits))
    return a.contiguous(), b.contiguous()


def same_bits_or_both_nan(a, b):
    """NaNs compared by position, everything else by bit pattern -> the count of mismatches"""
    an, bn = torch.isnan(a), torch.isnan(b)
    diff = (a.view(torch.int16) != b.view(torch.int16)) & ~(an & bn)
    return int(diff.sum()) + int((an != bn).sum())


# ---- the fixture's inputs ---------------------------------------------------------------------------------------------------------------------------
CONTENT = 4.0


def case_inputs(cfg, hw, seed, sigmas, b):
    """tools/make_stylealign_fixtures.py case_inputs: x fp32 [b, c, h, w] (unit noise plus a per-image, per-channel offset of CONTENT x N(0, 1)) at the noise level of `sigmas`, cond, uncond of synth_conditioning(seed)"""
    from forge_amd import synth
    rng = np.random.Generator(np.random.PCG64([seed, 11]))
    x = torch.from_numpy(rng.standard_normal((b, cfg["in_channels"], hw[0], hw[1]), dtype=np.float32))
    x = x + CONTENT * torch.from_numpy(np.random.Generator(np.random.PCG64([seed, 12])).standard_normal((b, cfg["in_channels"], 1, 1), dtype=np.float32))
    x = x * torch.sqrt(sigmas.float() ** 2 + 1.0).view(-1, 1, 1, 1)
    c, uc = synth.synth_conditioning(b, cfg["context_dim"], cfg.get("adm_in_channels"), seed=seed)
    return x, c, uc


# ---- the plain path, as it was ------------------------------------------------------------------------------------------------------------------------
# (config name, latent (h, w), rows): a tile-aligned and a ragged token count, four rows each
PLAIN_FORWARDS = [("TINY_SDXL_UNET_CONFIG", (32, 32), 4), ("TINY_SD15_UNET_CONFIG", (32, 24), 4)]


def plain_forward(i, device="cuda"):
    """forward_packed of a fresh executor with no option at all -> eps fp16 on the CPU.  tests/golden/tiny_stylealign_unet.pt["plain_bits"][i] is
    this function's result on an MI355X from the commit before the executor took a `share` argument."""
    from forge_amd import hipops as ops
    from forge_amd import synth
    from forge_amd.backend.nn.unet import IntegratedUNet2DConditionModel
    name, (hh, ww), bu = PLAIN_FORWARDS[i]
    cfg = dict(getattr(synth, name))
    net = IntegratedUNet2DConditionModel(cfg, synth.synth_unet_state_dict(cfg, seed=5), device=device)
    g = torch.Generator().manual_seed(900 + i)
    x = torch.randn(bu, cfg["in_channels"], hh, ww, generator=g).to(device)
    ctx = torch.randn(bu, 77, cfg["context_dim"], generator=g).to(device)
    y = torch.randn(bu, cfg["adm_in_channels"], generator=g).to(device) if cfg.get("adm_in_channels") else None
    xcol = ops.unet_pack_input(x, torch.full((bu,), 2.0, device=device), 1, 1.0)
    t = torch.tensor([400.0, 120.0, 800.0, 33.0][:bu], device=device)
    eps = net.forward_packed(xcol, t, net.prepare_context(ctx, y), bu, hh, ww)
    torch.cuda.synchronize()
    return eps.detach().to("cpu", copy=True)
