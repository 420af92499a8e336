"""Native IP-Adapter -- the patcher-level entry (reference: extensions-builtin/sd_forge_ipadapter, IPAdapterApply.apply_ipadapter and
CrossAttentionPatch of lib_ipadapter/IPAdapterPlus.py).

For every cross-attention of the UNet the reference computes
    out = attention(q, k_text, v_text) + sum over units of w_u * attention(q, k_ip_u, v_ip_u)
where k_ip / v_ip are a per-block linear map of the unit's 4 or 16 image tokens, the cond and the uncond rows of the batch using different tokens.
It installs that as Python `patches_replace["attn2"]` hooks.  Here the loaded units travel as the plain transformer option "ipadapter" (a list:
two units on one job are common), which KModel reads on the fused route -- window test on the host's copy of sigma -- and hands to the UNet
executor as an ExtraContext: per block the image K / V^T of the active units, cached per job next to the text K / V^T, one segment per unit.
A block with heads of 64 and at most 128 text keys runs ONE launch of fmxi_attention_dual_f16 (hipops.attention_dual) in place of its text
attention; every other head width runs the composite route (text attention, one attention per unit and group into scratch, add_scaled), on
existing kernels.  Both stay on the captured graph.  `python_patch` is the same arithmetic as attn2 replace patches, written here: what the
hooked executor runs where the native route does not apply, and what tests and tools/bench_features.py compare against.

Weight types: "original" scales the unit's term (the segment weight); "linear" and "channel" are transformations of the unit's K / V, done once
when the unit is prepared, with segment weight 1.  `embeds` are the CLIP-vision encoder's outputs, handed in by the caller or computed from an
image by backend/patcher/clipvision.ClipVisionModel (embeds_from_image), once per job and before any graph."""
import math

import torch

from ..nn import ipadapter as nets

OPTION = "ipadapter"
FEATURE = nets.FEATURE
MAX_UNITS, MAX_TOKENS = 4, 64          # what fmxi_attention_dual_f16 takes: segments, extra keys
WEIGHT_TYPES = ("original", "linear", "channel")

_serials = iter(range(1, 1 << 62))


def _dpad(d):
    from ..nn.unet import _dpad as f
    return f(d)


def transform_kv(k, v, weight, weight_type):
    """the reference's weight types on one unit's keys / values [..., T, C] (IPAdapterPlus.py:459-475), in the tensors' own dtype
    -> (k, v, factor of the unit's attention term)"""
    if weight_type.startswith("linear"):
        return k * weight, v * weight, 1.0
    if weight_type.startswith("channel"):
        mean = torch.mean(v, dim=-2, keepdim=True)
        w = weight * (float(k.shape[-1]) / 1280.0)
        return k * w, (v - mean) + mean * w, 1.0
    if weight_type.startswith("original"):
        return k, v, float(weight)
    return k, v, 1.0          # (the reference applies no weight at all to a type it does not know)


class Unit:
    """One IP-Adapter file on one pair of CLIP-vision embeddings: the image tokens (computed once, backend/nn/ipadapter.py) and per cross-attention
    block the keys / values of the cond and the uncond tokens."""

    def __init__(self, model, info, layout, embeds, weight, weight_type, sigma_start, sigma_end, device, attn_mask=None, unfold_batch=False):
        if weight_type not in WEIGHT_TYPES:
            raise ValueError(f"{FEATURE}: weight_type {weight_type!r}; known: {WEIGHT_TYPES}")
        self.info, self.device = info, torch.device(device)
        self.weight, self.weight_type = float(weight), weight_type
        self.sigma_start, self.sigma_end = float(sigma_start), float(sigma_end)
        self.attn_mask, self.unfold_batch = attn_mask, bool(unfold_batch)
        self.to_kv = nets.to_kv_weights(model["ip_adapter"], layout)          # refuses a file made for another model family
        self.order = nets.attn2_order(layout)
        self.model = model
        clip_embed, clip_embed_zeroed = embeds
        self.embeds = (clip_embed, clip_embed_zeroed)
        self.images = int(clip_embed.shape[0])
        self.tokens_per_image = int(info["tokens"])
        self.serial = next(_serials)
        self._tokens = None          # (cond, uncond) fp16 [images, T, C] on the device
        self._kv = {}                # block -> (k [2, T, H * d], v [2, T, H * d]) fp16, index 0 cond / 1 uncond, weight type applied
        self.joint = {}              # (serials of the active units, cond_or_uncond) -> ExtraContext whose first unit this is
        self.force_composite = False

    # ---- once per job, outside any capture ----------------------------------------------------------------------------------------------------
    def image_tokens(self):
        if self._tokens is None:
            if self.device.type == "cuda":
                proj = nets.build_image_proj(self.model, self.info, self.device)
                both = proj(torch.cat([self.embeds[0], self.embeds[1]]))
                self._tokens = (both[:self.images].contiguous(), both[self.images:].contiguous())
            else:
                self._tokens = tuple(image_tokens_torch(self.model, self.info, e.float()) for e in self.embeds)
        return self._tokens

    def block_kv(self, block):
        """(k, v) [2, T, C_inner] of the block (first reference image), the weight type applied; fp16 through ops.linear on the GPU, torch off it"""
        kv = self._kv.get(block)
        if kv is None:
            cond, uncond = self.image_tokens()
            toks = torch.cat([cond[:1], uncond[:1]])                                           # [2, T, C]
            wk, wv = self.to_kv[block]
            if toks.is_cuda:
                from ... import hipops as ops
                rows = toks.reshape(-1, toks.shape[-1]).contiguous()
                f16 = lambda w: w.detach().to(device=self.device, dtype=torch.float16).contiguous()   # noqa: E731
                k = ops.linear(rows, f16(wk), out=torch.empty(rows.shape[0], wk.shape[0], dtype=torch.float16, device=self.device)).view(2, -1, wk.shape[0])
                v = ops.linear(rows, f16(wv), out=torch.empty(rows.shape[0], wv.shape[0], dtype=torch.float16, device=self.device)).view(2, -1, wv.shape[0])
            else:
                k, v = toks @ wk.to(toks).T, toks @ wv.to(toks).T
            k, v, _ = transform_kv(k, v, self.weight, self.weight_type)
            kv = self._kv[block] = (k.contiguous(), v.contiguous())
        return kv

    @property
    def segment_weight(self):
        return self.weight if self.weight_type == "original" else 1.0

    def active(self, sigma):
        """the reference's window test, on a host float: `sigma > sigma_start or sigma < sigma_end` skips the unit"""
        return not (sigma > self.sigma_start or sigma < self.sigma_end)

    def native_ok(self):
        return self.attn_mask is None and not self.unfold_batch and self.images == 1 and self.tokens_per_image <= MAX_TOKENS

    def key(self):
        return (self.serial, self.weight, self.weight_type)


def image_tokens_torch(model, info, embeds):
    """the image projection in torch fp32 (python_patch off the GPU; the tests' yardstick for backend/nn/ipadapter.py) -> [B, T, C]"""
    sd = {k: v.float() for k, v in model["image_proj"].items()}
    F = torch.nn.functional
    if not info["is_plus"]:
        c = sd["norm.weight"].shape[0]
        y = F.linear(embeds, sd["proj.weight"], sd["proj.bias"]).reshape(-1, info["tokens"], c)
        return F.layer_norm(y, (c,), sd["norm.weight"], sd["norm.bias"])
    x = F.linear(embeds, sd["proj_in.weight"], sd["proj_in.bias"])
    lat = sd["latents"].repeat(x.shape[0], 1, 1)
    dim = lat.shape[-1]
    i = 0
    while f"layers.{i}.0.to_q.weight" in sd:
        p = f"layers.{i}."
        xn = F.layer_norm(x, (dim,), sd[p + "0.norm1.weight"], sd[p + "0.norm1.bias"])
        ln = F.layer_norm(lat, (dim,), sd[p + "0.norm2.weight"], sd[p + "0.norm2.bias"])
        q = F.linear(ln, sd[p + "0.to_q.weight"])
        k, v = F.linear(torch.cat([xn, ln], dim=-2), sd[p + "0.to_kv.weight"]).chunk(2, dim=-1)
        heads = q.shape[-1] // nets.DIM_HEAD
        sp = lambda t: t.view(t.shape[0], t.shape[1], heads, -1).transpose(1, 2)   # noqa: E731
        w = torch.softmax((sp(q) @ sp(k).transpose(-2, -1)) * nets.DIM_HEAD ** -0.5, dim=-1)
        o = (w @ sp(v)).permute(0, 2, 1, 3).reshape(lat.shape[0], lat.shape[1], -1)
        lat = F.linear(o, sd[p + "0.to_out.weight"]) + lat
        h = F.layer_norm(lat, (dim,), sd[p + "1.0.weight"], sd[p + "1.0.bias"])
        lat = F.linear(F.gelu(F.linear(h, sd[p + "1.1.weight"])), sd[p + "1.3.weight"]) + lat
        i += 1
    y = F.linear(lat, sd["proj_out.weight"], sd["proj_out.bias"])
    return F.layer_norm(y, (y.shape[-1],), sd["norm_out.weight"], sd["norm_out.bias"])


class ExtraContext:
    """What the UNet executor gets for one model call: the active units, the group order, and per block the cached extra K / V^T.
    blocks[name] = dict(xk [G, 64, H * dp], xvt [H * dp, G * 64], segments [(start, count, weight)],            (the dual route's operands)
                        units [(xk_u [G, 64, H * dp], xvt_u [H * dp, G * 64], count, weight)])                   (the composite route's)
    Group g of the batch holds the images g * (Bu // G) ...: cond tokens where cond_or_uncond[g] == 0, uncond tokens where it is 1."""

    def __init__(self, units, cond_or_uncond):
        self.units, self.cond_or_uncond = list(units), list(cond_or_uncond)
        self.blocks = {}
        self.serial = next(_serials)          # a context built again gets new tensors: no graph captured on the old ones may be replayed
        # the composite route on every block, heads of 64 included: the timing baseline of tools/bench_features.py (a unit's `force_composite`)
        self.force_composite = any(u.force_composite for u in self.units)

    def graph_key(self):
        return (OPTION, self.serial, tuple(self.cond_or_uncond), self.force_composite) + tuple(u.key() for u in self.units)

    def prepare(self, net):
        """every block's operands on the device, outside any capture (idempotent)"""
        from ..nn.layout import SpatialT
        if self.blocks:
            return self
        groups = len(self.cond_or_uncond)
        dev = net.device
        for L in net.layout.all_layers():
            if not isinstance(L, SpatialT):
                continue
            H, d = L.heads, L.dim_head
            dp = _dpad(d)
            for di in range(L.depth):
                b = f"{L.key}.transformer_blocks.{di}"
                xk = torch.zeros(groups, MAX_TOKENS, H, dp, dtype=torch.float16, device=dev)
                xv = torch.zeros(groups, MAX_TOKENS, H, dp, dtype=torch.float16, device=dev)
                segments, per_unit, at = [], [], 0
                for u in self.units:
                    k, v = u.block_kv(b)                                   # [2, T, H * d]
                    t = k.shape[1]
                    sel = torch.tensor(self.cond_or_uncond, device=k.device)
                    ku = torch.zeros(groups, MAX_TOKENS, H, dp, dtype=torch.float16, device=dev)
                    vu = torch.zeros(groups, MAX_TOKENS, H, dp, dtype=torch.float16, device=dev)
                    ku[:, :t, :, :d] = k[sel].view(groups, t, H, d)
                    vu[:, :t, :, :d] = v[sel].view(groups, t, H, d)
                    xk[:, at:at + t] = ku[:, :t]
                    xv[:, at:at + t] = vu[:, :t]
                    segments.append((at, t, u.segment_weight))
                    per_unit.append((ku.view(groups, MAX_TOKENS, H * dp), vu.view(groups * MAX_TOKENS, H * dp).T.contiguous(), t, u.segment_weight))
                    at += t
                self.blocks[b] = dict(xk=xk.view(groups, MAX_TOKENS, H * dp), xvt=xv.view(groups * MAX_TOKENS, H * dp).T.contiguous(),
                                      segments=segments, units=per_unit)
        return self


def units_of(transformer_options):
    return (transformer_options or {}).get(OPTION) or None


def check_cond_or_uncond(cond_or_uncond, batch):
    if not cond_or_uncond:
        raise NotImplementedError(f"{FEATURE} (native): the call carries no cond_or_uncond, so the cond and the uncond rows of its batch cannot be told apart")
    if len(set(cond_or_uncond)) != len(cond_or_uncond) or any(c not in (0, 1) for c in cond_or_uncond):
        raise NotImplementedError(f"{FEATURE} (native): cond_or_uncond {list(cond_or_uncond)} repeats an entry: the batch must hold every group once")
    if batch % len(cond_or_uncond):
        raise NotImplementedError(f"{FEATURE} (native): a batch of {batch} images does not split into {len(cond_or_uncond)} groups")


def ipadapter_for_call(transformer_options, sigma, cond_or_uncond, batch, net):
    """One model call on the fused route -> the ExtraContext of the units whose window holds the call's sigma (a host float), prepared, or None
    (no option, or every unit outside its window: the plain call, the plain graph, bit for bit).  What cannot run beside the native route is
    refused before (native_call.resolve_call)."""
    units = units_of(transformer_options)
    if units is None:
        return None
    check_cond_or_uncond(cond_or_uncond, batch)
    active = [u for u in units if u.active(float(sigma))]
    if not active:
        return None
    key = (tuple(u.serial for u in active), tuple(cond_or_uncond))
    ctx = active[0].joint.get(key)
    if ctx is None:
        ctx = active[0].joint[key] = ExtraContext(active, cond_or_uncond)
    return ctx.prepare(net)


def check_world(transformer_options, world_size):
    """The sharded entry splits a job's batch over the ranks: a shard no longer holds the groups cond_or_uncond names.  Refused before any collective."""
    if units_of(transformer_options) is not None and world_size > 1:
        raise NotImplementedError(f"{FEATURE} with a batch sharded over {world_size} ranks: image b of a call reads the tokens of group "
                                  "b // (batch / groups), which a shard does not preserve; run the job on one rank")


# ---- the Python route ---------------------------------------------------------------------------------------------------------------------------------
class PythonPatch:
    """CrossAttentionPatch.__call__ for one cross-attention block, in this project's words: an attn2 replace patch (q, k, v, extra_options) -> out,
    all [B, N, heads * dim_head].  One object per block carries all units of the job, in the order they were installed."""

    def __init__(self, block, units):
        self.block, self.units = block, units

    @staticmethod
    def attention(q, k, v, heads):
        B, n, c = q.shape
        sp = lambda t: t.view(t.shape[0], t.shape[1], heads, c // heads).transpose(1, 2)   # noqa: E731
        o = torch.nn.functional.scaled_dot_product_attention(sp(q), sp(k), sp(v))
        return o.transpose(1, 2).reshape(B, n, c)

    def __call__(self, q, k, v, extra_options):
        cond_or_uncond = extra_options["cond_or_uncond"]
        sigma = extra_options["sigmas"][0] if "sigmas" in extra_options else None
        sigma = float(sigma) if sigma is not None else 999999999.9
        heads = extra_options["n_heads"]
        b, qs = q.shape[0], q.shape[1]
        batch_prompt = b // len(cond_or_uncond)
        out = self.attention(q, k, v, heads)
        for u in self.units:
            if not u.active(sigma):
                continue
            cond, uncond = u.image_tokens()
            wk, wv = (w.to(device=q.device, dtype=q.dtype) for w in u.to_kv[self.block])
            cond, uncond = cond.to(q), uncond.to(q)
            if u.unfold_batch and cond.shape[0] > 1:
                fit = lambda t: torch.cat((t, t[-1:].repeat(batch_prompt - t.shape[0], 1, 1)))[:batch_prompt] if t.shape[0] != batch_prompt else t   # noqa: E731
                cond, uncond = fit(cond), fit(uncond)
                rep = 1
            else:
                rep = batch_prompt
            kc, ku, vc, vu = (t.repeat(rep, 1, 1) for t in (cond @ wk.T, uncond @ wk.T, cond @ wv.T, uncond @ wv.T))
            ip_k = torch.cat([(kc, ku)[i] for i in cond_or_uncond])
            ip_v = torch.cat([(vc, vu)[i] for i in cond_or_uncond])
            ip_k, ip_v, factor = transform_kv(ip_k, ip_v, u.weight, u.weight_type)
            out_ip = self.attention(q, ip_k, ip_v, heads)
            if factor != 1.0:
                out_ip = out_ip * factor
            if u.attn_mask is not None:
                _, _, lh, lw = extra_options["original_shape"]
                mh = lh / math.sqrt(lh * lw / qs)
                mh = int(mh) + int((qs % int(mh)) != 0)
                mw = qs // mh
                m = torch.nn.functional.interpolate(u.attn_mask.to(q.device).float().unsqueeze(1), size=(mh, mw), mode="bicubic").squeeze(1)
                m = torch.cat((m, m[-1:].repeat(max(0, batch_prompt - m.shape[0]), 1, 1)))[:batch_prompt]
                m = m.repeat(len(cond_or_uncond), 1, 1).view(b, -1, 1).to(q.dtype)
                out_ip = out_ip * m
            out = out + out_ip
        return out.to(q.dtype)


def python_patch(units, layout=None):
    """-> {reference key (kind, number[, index]): PythonPatch} for every cross-attention of the units' UNet: what install_python sets as
    patches_replace["attn2"]"""
    units = list(units) if isinstance(units, (list, tuple)) else [units]
    return {nets.reference_key(e): PythonPatch(e[3], units) for e in units[0].order}


def install_python(m, units):
    for key, patch in python_patch(units).items():
        m.set_model_attn2_replace(patch, *key)
    return m


def _python_units(to):
    """the units a patcher already runs through python_patch (all blocks carry the same list)"""
    for p in ((to.get("patches_replace") or {}).get("attn2") or {}).values():
        if isinstance(p, PythonPatch):
            return list(p.units)
    return []


def _has_foreign_hooks(to):
    """Python block hooks other than IP-Adapter's own replace patches"""
    from ..nn.unet import IntegratedUNet2DConditionModel as Net
    rest = dict(to)
    rep = {k: {kk: p for kk, p in v.items() if not isinstance(p, PythonPatch)} for k, v in (to.get("patches_replace") or {}).items()}
    rest["patches_replace"] = {k: v for k, v in rep.items() if v}
    return Net._hooks(rest) is not None


PREPROCESSOR_KEYS = ("clip_vision", "image", "weight_type", "noise", "embeds", "unfold_batch")


def file_clip_width(model, info):
    """the file's clip_embeddings_dim: the input width of its image projection"""
    return int(model["image_proj"]["proj_in.weight" if info["is_plus"] else "proj.weight"].shape[1])


def embeds_from_image(clip_vision, image, model, info, noise=0.0):
    """(clip_embed, clip_embed_zeroed) as apply_ipadapter computes them from an image (IPAdapterPlus.py:686-702): plus files take
    penultimate_hidden_states of the image and of a black 224 x 224 image (zeroed_hidden_states), base files image_embeds and zeros.  The image
    and the black image go through the tower in ONE batch.  clip_vision: backend/patcher/clipvision.ClipVisionModel."""
    if (noise or 0) > 0:
        raise NotImplementedError(f"{FEATURE}: noise {noise} > 0: the reference's image_add_noise is torchvision's ElasticTransform on a reseeded "
                                  "generator, which has no counterpart here; pass noise=0")
    if clip_vision is None or image is None:
        raise ValueError(f"{FEATURE}: without embeds= the call needs clip_vision= and image=")
    which = "penultimate_hidden_states" if info["is_plus"] else "image_embeds"
    want, have = file_clip_width(model, info), clip_vision.output_width[which]
    if want != have:
        raise NotImplementedError(f"{FEATURE}: the file's clip_embeddings_dim is {want}, this CLIP-vision tower's {which} are {have} wide: "
                                  "the file was made for another image encoder")
    from .clipvision import clip_preprocess
    image = image.to(clip_vision.load_device)
    rows = clip_preprocess(image)
    if not info["is_plus"]:
        e = clip_vision.encode_pixel_rows(rows)[which]
        return e, torch.zeros_like(e)
    b = image.shape[0]
    black = clip_preprocess(torch.zeros(b, 224, 224, 3, device=image.device))
    both = clip_vision.encode_pixel_rows(torch.cat([rows, black]))[which]
    return both[:b].contiguous(), both[b:].contiguous()


def patch_ipadapter(unet_patcher, ipadapter_sd, embeds=None, weight=1.0, weight_type="original", start_at=0.0, end_at=1.0, attn_mask=None, unfold_batch=False,
                    clip_vision=None, image=None, noise=0.0):
    """-> a clone of `unet_patcher` that applies the IP-Adapter file `ipadapter_sd` (the loaded .bin / .pth / .safetensors state dict) on
    embeds = (clip_embed, clip_embed_zeroed), the reference's own `embeds=` argument of apply_ipadapter: CLIP-vision image_embeds [1, D] for base
    files, penultimate_hidden_states [1, 257, D] for plus files.  With embeds=None they are computed from `image` ([b, h, w, 3] in [0, 1]) by
    `clip_vision` (embeds_from_image); `embeds` may also be the reference's preprocessor dict (clip_vision, image, weight_type, noise, embeds,
    unfold_batch), whose entries then stand for the keyword arguments of the same names.  The clone carries the transformer option "ipadapter" (the native route), or --
    with attn_mask, unfold_batch, more than one reference image, more than 4 units or more than 64 tokens in all -- the same arithmetic as Python
    attn2 replace patches.  Refused (NotImplementedError, before any launch): Flux; FaceID / FaceID-Plus / Portrait / InstantID and 'full' files;
    a file whose to_k_ip count does not fit the UNet; native Perturbed-Attention Guidance or ControlNet-LLLite, or Python block hooks, on the
    same job."""
    from ..modules.k_model import KModelFlux
    if isinstance(unet_patcher.model, KModelFlux):
        raise NotImplementedError(f"{FEATURE}: UNet models only (Flux has no cross-attention against a text context to extend)")
    if isinstance(embeds, dict):
        unknown = sorted(set(embeds) - set(PREPROCESSOR_KEYS))
        if unknown:
            raise ValueError(f"{FEATURE}: the preprocessor dict has keys {unknown}; known: {PREPROCESSOR_KEYS}")
        d = embeds
        clip_vision, image, embeds = d.get("clip_vision", clip_vision), d.get("image", image), d.get("embeds")
        weight_type, noise, unfold_batch = d.get("weight_type", weight_type), d.get("noise", noise), d.get("unfold_batch", unfold_batch)
    model = nets.split_file(ipadapter_sd)
    info = nets.detect(model)
    nets.refuse_unsupported(model, info)
    if embeds is None:
        embeds = embeds_from_image(clip_vision, image, model, info, noise)
    to = unet_patcher.model_options.get("transformer_options", {})
    from .native_call import message
    if unet_patcher.model_options.get("pag") is not None:
        raise NotImplementedError(message("ipadapter", "pag_from"))
    if to.get("lllite") is not None:
        raise NotImplementedError(message("ipadapter", "lllite"))
    if _has_foreign_hooks(to):
        raise NotImplementedError(f"{FEATURE} together with Python block hooks in transformer_options")
    predictor = unet_patcher.model.predictor
    net = unet_patcher.model.diffusion_model
    device = getattr(unet_patcher.model, "device", None) or unet_patcher.load_device or embeds[0].device
    unit = Unit(model, info, net.layout, embeds, weight, weight_type, predictor.percent_to_sigma(start_at), predictor.percent_to_sigma(end_at), device,
                attn_mask=attn_mask, unfold_batch=unfold_batch)
    m = unet_patcher.clone()
    mto = m.model_options["transformer_options"]
    native, python = list(mto.get(OPTION) or []), _python_units(mto)
    units = native + python + [unit]
    if not python and all(u.native_ok() for u in units) and len(units) <= MAX_UNITS and sum(u.tokens_per_image for u in units) <= MAX_TOKENS:
        m.set_transformer_option(OPTION, units)
        return m
    # the Python route: every unit of the job, in the order they were installed (the reference chains them inside one patch object per block)
    mto.pop(OPTION, None)
    rep = dict(mto.get("patches_replace") or {})
    rep["attn2"] = {k: p for k, p in (rep.get("attn2") or {}).items() if not isinstance(p, PythonPatch)}
    mto["patches_replace"] = rep
    return install_python(m, units)


class IPAdapterPatcher:
    """The control-unit entry: built by load_controlnet from a control model file that has ip_adapter keys; before every sampling pass it patches
    the job's UNet with the unit's embeddings, weight and window."""

    @staticmethod
    def try_build_from_state_dict(state_dict, ckpt_path=None):
        if not nets.is_ipadapter_file(state_dict):
            return None
        return IPAdapterPatcher(state_dict)

    def __init__(self, state_dict):
        self.state_dict = state_dict
        self.strength = 1.0
        self.start_percent = 0.0
        self.end_percent = 1.0
        self.weight_type = "original"

    def process_before_every_sampling(self, process, cond, mask=None, *args, **kwargs):
        """cond: the unit's embeddings (clip_embed, clip_embed_zeroed), or the reference's preprocessor dict (clip_vision, image, weight_type,
        noise, embeds, unfold_batch): with embeds=None in it the embeddings are computed from the image (patch_ipadapter)"""
        objs = process.sd_model.forge_objects
        objs.unet = patch_ipadapter(objs.unet, self.state_dict, cond, self.strength, self.weight_type, self.start_percent, self.end_percent,
                                    attn_mask=mask)
