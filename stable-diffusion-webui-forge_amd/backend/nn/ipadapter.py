"""IP-Adapter's own networks (reference: extensions-builtin/sd_forge_ipadapter, lib_ipadapter/IPAdapterPlus.py and resampler.py): the image
projection that turns CLIP-vision embeddings into 4 or 16 image tokens, and the per-block to_k_ip / to_v_ip maps.  They run ONCE per job, outside
any capture, on the existing ops: ops.linear, ops.layernorm, ops.attention (generic route: 16 queries) and the activation kernel -- no torch
arithmetic on the path (copies into padded buffers only).  The CLIP-vision encoder itself is not here: the caller hands its embeddings in."""
import torch

from .layout import SpatialT

FEATURE = "IP-Adapter"
DIM_HEAD = 64                # PerceiverAttention's head width in every published file
K_GRANULE = 64               # the GEMM's K granule: narrower inputs are zero-padded


def split_file(state_dict):
    """A loaded IP-Adapter file -> {"image_proj": {...}, "ip_adapter": {...}}: .bin / .pth files hold the two dicts, .safetensors files flat keys
    with the prefixes `image_proj.` / `ip_adapter.` (forge_ipadapter.py:113-135)."""
    if "ip_adapter" in state_dict and isinstance(state_dict["ip_adapter"], dict):
        return {"image_proj": dict(state_dict.get("image_proj") or {}), "ip_adapter": dict(state_dict["ip_adapter"])}
    out = {"image_proj": {}, "ip_adapter": {}}
    for key, value in state_dict.items():
        for part in out:
            if key.startswith(part + "."):
                out[part][key[len(part) + 1:]] = value
    if not out["ip_adapter"]:
        raise ValueError(f"{FEATURE}: the file has no ip_adapter keys")
    return out


def is_ipadapter_file(state_dict):
    keys = state_dict.keys()
    return "ip_adapter" in keys or any(isinstance(k, str) and k.startswith("ip_adapter.") for k in keys)


def detect(model):
    """The reference's own tests on the split file (IPAdapterPlus.py:605-617) -> dict(is_plus, is_full, is_faceid, is_portrait, is_sdxl,
    cross_attention_dim, output_cross_attention_dim, tokens)"""
    proj, ip = model["image_proj"], model["ip_adapter"]
    is_full = "proj.3.weight" in proj
    is_portrait = "proj.2.weight" in proj and "proj.3.weight" not in proj and "0.to_q_lora.down.weight" not in ip
    is_faceid = is_portrait or "0.to_q_lora.down.weight" in ip
    is_plus = is_full or "latents" in proj or "perceiver_resampler.proj_in.weight" in proj
    out_dim = int(ip["1.to_k_ip.weight"].shape[1])
    is_sdxl = out_dim == 2048
    return dict(is_plus=is_plus, is_full=is_full, is_faceid=is_faceid, is_portrait=is_portrait, is_sdxl=is_sdxl,
                cross_attention_dim=1280 if is_plus and is_sdxl and not is_faceid else out_dim, output_cross_attention_dim=out_dim,
                tokens=16 if is_plus or is_portrait else 4)


def refuse_unsupported(model, info):
    """by name, with the reason, before anything is built"""
    if "0.to_q_lora.down.weight" in model["ip_adapter"] or info["is_faceid"]:
        kind = "Portrait" if info["is_portrait"] else ("FaceID-Plus" if info["is_plus"] else "FaceID")
        raise NotImplementedError(f"{FEATURE}: {kind} files take a face embedding from insightface, which this backend does not run")
    if info["is_full"]:
        raise NotImplementedError(f"{FEATURE}: 'full' files project all 257 CLIP tokens; the attention kernel takes at most 64 extra keys")
    if "latents" in model["image_proj"] and int(model["image_proj"]["proj_in.weight"].shape[1]) == 512:
        raise NotImplementedError(f"{FEATURE}: InstantID files resample a 512-wide face embedding from insightface, which this backend does not run")


def attn2_order(layout):
    """The reference's numbering of the cross-attentions (IPAdapterPlus.py:762-783), derived from the UNet's own transformer blocks: input blocks,
    then output blocks, then the middle block -> [(kind, block number, transformer index or None, executor block name)].  A UNet whose
    transformers all have depth 1 (SD1.5) is keyed without the index, as the reference keys it."""
    def of(kind, blocks):
        for number, blk in enumerate(blocks):
            for L in blk:
                if isinstance(L, SpatialT):
                    for di in range(L.depth):
                        yield kind, number, di, f"{L.key}.transformer_blocks.{di}"
    entries = list(of("input", layout.input_blocks)) + list(of("output", layout.output_blocks)) + list(of("middle", [layout.middle]))
    indexed = any(di > 0 for _, _, di, _ in entries) or layout_is_sdxl(layout)
    return [(kind, number, di if indexed else None, name) for kind, number, di, name in entries]


def layout_is_sdxl(layout):
    return getattr(layout, "adm_in_channels", None) is not None


def reference_key(entry):
    """the patches_replace["attn2"] key the reference installs its patch under: (kind, number) or (kind, number, index)"""
    kind, number, di, _ = entry
    return (kind, number) if di is None else (kind, number, di)


def to_kv_weights(ip_adapter, layout):
    """{executor block name: (to_k_ip weight, to_v_ip weight)}: key "{2n+1}.to_k_ip.weight" belongs to the n-th cross-attention of attn2_order"""
    order = attn2_order(layout)
    count = sum(1 for k in ip_adapter if k.endswith(".to_k_ip.weight"))
    if count != len(order):
        raise NotImplementedError(f"{FEATURE}: the file has {count} to_k_ip maps, this UNet has {len(order)} cross-attentions: the file was made for "
                                  "another model family")
    return {name: (ip_adapter[f"{2 * n + 1}.to_k_ip.weight"], ip_adapter[f"{2 * n + 1}.to_v_ip.weight"]) for n, (_, _, _, name) in enumerate(order)}


# ---- the image projection on the device ---------------------------------------------------------------------------------------------------------------
def _f16(t, device):
    return t.detach().to(device=device, dtype=torch.float16).contiguous()


def _pad_k(w, device):
    """[out, k] -> fp16 [out, k padded to the GEMM's K granule] on the device"""
    w = _f16(w, device)
    pad = -w.shape[1] % K_GRANULE
    return torch.nn.functional.pad(w, (0, pad)) if pad else w


def _rows(x, k):
    """[M, c] fp16 -> [M, k] zero-padded (a copy only where c < k)"""
    if x.shape[1] == k:
        return x.contiguous()
    out = torch.zeros(x.shape[0], k, dtype=torch.float16, device=x.device)
    out[:, :x.shape[1]] = x
    return out


class ImageProj:
    """ImageProjModel (base files): Linear -> reshape to `tokens` tokens -> LayerNorm"""

    def __init__(self, sd, tokens, device):
        self.tokens = tokens
        self.w, self.b = _pad_k(sd["proj.weight"], device), _f16(sd["proj.bias"], device)
        self.g, self.beta = _f16(sd["norm.weight"], device), _f16(sd["norm.bias"], device)

    def __call__(self, embeds):
        """[B, D] -> fp16 [B, tokens, cross_attention_dim]"""
        from ... import hipops as ops
        if embeds.dim() != 2:
            raise ValueError(f"{FEATURE}: a base file takes CLIP image_embeds [B, D], got {tuple(embeds.shape)}")
        x = _rows(_f16(embeds, self.w.device), self.w.shape[1])
        y = ops.linear(x, self.w, self.b, out=torch.empty(x.shape[0], self.w.shape[0], dtype=torch.float16, device=x.device))
        c = self.g.shape[0]
        y = y.view(x.shape[0] * self.tokens, c)
        return ops.layernorm(y, self.g, self.beta, out=torch.empty_like(y)).view(x.shape[0], self.tokens, c)


class Resampler:
    """The perceiver resampler of the "plus" files (resampler.py): proj_in, depth x (PerceiverAttention over cat(x, latents) with heads of 64,
    FeedForward with erf-GELU and no biases), proj_out, norm_out"""

    def __init__(self, sd, device):
        self.device = device
        self.latents = _f16(sd["latents"], device)[0]                      # [queries, dim]
        self.proj_in = (_pad_k(sd["proj_in.weight"], device), _f16(sd["proj_in.bias"], device))
        self.proj_out = (_f16(sd["proj_out.weight"], device), _f16(sd["proj_out.bias"], device))
        self.norm_out = (_f16(sd["norm_out.weight"], device), _f16(sd["norm_out.bias"], device))
        self.layers = []
        i = 0
        while f"layers.{i}.0.to_q.weight" in sd:
            p = f"layers.{i}."
            wkv = _f16(sd[p + "0.to_kv.weight"], device)
            inner = wkv.shape[0] // 2
            self.layers.append(dict(n1=(_f16(sd[p + "0.norm1.weight"], device), _f16(sd[p + "0.norm1.bias"], device)),
                                    n2=(_f16(sd[p + "0.norm2.weight"], device), _f16(sd[p + "0.norm2.bias"], device)),
                                    q=_f16(sd[p + "0.to_q.weight"], device), k=wkv[:inner].contiguous(), v=wkv[inner:].contiguous(),
                                    out=_f16(sd[p + "0.to_out.weight"], device),
                                    ln=(_f16(sd[p + "1.0.weight"], device), _f16(sd[p + "1.0.bias"], device)),
                                    ff1=_f16(sd[p + "1.1.weight"], device), ff2=_f16(sd[p + "1.3.weight"], device)))
            i += 1
        dim = self.latents.shape[1]
        inner = self.layers[0]["q"].shape[0]
        if inner % DIM_HEAD or dim % K_GRANULE or inner % K_GRANULE:
            raise NotImplementedError(f"{FEATURE}: resampler width {dim} / inner width {inner}: the heads are {DIM_HEAD} wide and the GEMMs take "
                                      f"multiples of {K_GRANULE}")
        self.heads = inner // DIM_HEAD

    def __call__(self, x):
        """[B, n1, D] (CLIP penultimate hidden states) -> fp16 [B, queries, output_dim]"""
        from ... import hipops as ops
        if x.dim() != 3:
            raise ValueError(f"{FEATURE}: a plus file takes CLIP penultimate_hidden_states [B, 257, D], got {tuple(x.shape)}")
        dev = self.device
        new = lambda *s: torch.empty(*s, dtype=torch.float16, device=dev)   # noqa: E731
        B, n1, _ = x.shape
        nq, dim = self.latents.shape
        inner = self.heads * DIM_HEAD
        x2 = _rows(_f16(x, dev).reshape(B * n1, -1), self.proj_in[0].shape[1])
        x2 = ops.linear(x2, *self.proj_in, out=new(B * n1, dim))
        lat = self.latents.repeat(B, 1)                                      # [B * nq, dim]
        nk = n1 + nq
        nkp = -(-nk // 64) * 64
        for L in self.layers:
            kv_in = torch.zeros(B, nkp, dim, dtype=torch.float16, device=dev)    # cat(norm1(x), norm2(latents)) per image, zero rows behind
            kv_in[:, :n1] = ops.layernorm(x2, *L["n1"], out=new(B * n1, dim)).view(B, n1, dim)
            ln2 = ops.layernorm(lat, *L["n2"], out=new(B * nq, dim))
            kv_in[:, n1:nk] = ln2.view(B, nq, dim)
            kv2 = kv_in.view(B * nkp, dim)
            q = ops.linear(ln2, L["q"], out=new(B * nq, inner))
            k = ops.linear(kv2, L["k"], out=new(B * nkp, inner))
            vt = ops.conv_gemm(L["v"], kv2, B * nkp, out=new(inner, B * nkp), ld_out=B * nkp)    # V^T [inner, B * nkp] (operand swap)
            # (q * s) (k * s)^T with s = dim_head ** -0.25 is q k^T * dim_head ** -0.5
            o = ops.attention(q, k, vt, batch=B, heads=self.heads, nq=nq, nk=nk, nk_pad=nkp, dpad=DIM_HEAD, scale=DIM_HEAD ** -0.5, q_bs=nq * inner,
                              q_rs=inner, k_bs=nkp * inner, k_rs=inner, vt_bs=nkp, vt_hs=DIM_HEAD * B * nkp, vt_ds=B * nkp, out=new(B * nq, inner))
            lat = ops.linear(o, L["out"], residual=lat, out=new(B * nq, dim))
            h = ops.linear(ops.layernorm(lat, *L["ln"], out=new(B * nq, dim)), L["ff1"], out=new(B * nq, L["ff1"].shape[0]))
            h = ops.act(h, ops.ACT_GELU_ERF, out=h)
            lat = ops.linear(h, L["ff2"], residual=lat, out=new(B * nq, dim))
        y = ops.linear(lat, *self.proj_out, out=new(B * nq, self.proj_out[0].shape[0]))
        return ops.layernorm(y, *self.norm_out, out=torch.empty_like(y)).view(B, nq, -1)


def build_image_proj(model, info, device):
    return Resampler(model["image_proj"], device) if info["is_plus"] else ImageProj(model["image_proj"], info["tokens"], device)
