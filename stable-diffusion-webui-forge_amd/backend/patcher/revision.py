"""Revision (reference: extensions-builtin/forge_preprocessor_revision): SDXL conditioned on a CLIP-G image embedding in place of the pooled text
embedding.  It is only a conditioning modifier on SDXL's `y`: the first 1280 of its 2816 columns are the pooled bigG text embedding, and the
modifier overwrites them with sum(image_embeds_u * weight_u) on the cond rows and zeros on the uncond rows; a unit that ignores the prompt also
zeroes the cross-attention context.  `conditioning_modifiers` already run in backend/sampling/sampling_function.py; the embedding comes from
backend/patcher/clipvision.ClipVisionModel.encode_image (ViT-bigG/14).

Refused: a model whose `y` is not 2816 wide (not SDXL), and a model with a `noise_augmentor` (unCLIP checkpoints: not built here).  noise_aug is
carried as the reference carries it and, as there, has no effect without a noise_augmentor."""
import torch

FEATURE = "Revision"
Y_WIDTH, EMBED_WIDTH = 2816, 1280


def revision_conditioning_modifier(model, x, timestep, uncond, cond, cond_scale, model_options, seed):
    units = model_options["revision_conditions"]
    if getattr(model, "noise_augmentor", None) is not None:
        raise NotImplementedError(f"{FEATURE}: the model has a noise_augmentor (an unCLIP checkpoint); only SDXL's plain `y` is supported")
    adm_inputs = [u["cond"]["image_embeds"] * u["weight"] for u in units]     # (the reference skips noise augmentation without a noise_augmentor)
    # one unit: its product; several: the reference's torch.stack(...).sum(0)
    adm_out = torch.stack(adm_inputs).sum(0) if len(adm_inputs) > 1 else adm_inputs[0]
    new_y = adm_out[:, :EMBED_WIDTH]
    ignore_prompt = any(u["ignore_prompt"] for u in units)

    cache = model_options.setdefault("revision_cache", {})      # source tensor -> its replacement: the same tensors step after step, as without the modifier

    def cached(which, src, make):
        hit = cache.get((which, id(src)))
        if hit is None or hit[0] is not src:
            hit = cache[(which, id(src))] = (src, make())
        return hit[1]

    def rebuilt(entries, which, image_part):
        out = []
        for c in entries or []:
            mc = dict(c["model_conds"])
            y = mc["y"].cond if "y" in mc else None
            if y is None or y.shape[-1] != Y_WIDTH:
                raise NotImplementedError(f"{FEATURE}: `y` is {None if y is None else y.shape[-1]} wide, SDXL's is {Y_WIDTH}")

            def new_y_of(y=y):
                t = y.clone()
                t[:, :EMBED_WIDTH] = image_part.to(device=y.device, dtype=y.dtype)
                return t
            mc["y"] = mc["y"].__class__(cached(which + "/y", y, new_y_of))
            if ignore_prompt:
                ctx = mc["c_crossattn"].cond
                mc["c_crossattn"] = mc["c_crossattn"].__class__(cached(which + "/c", ctx, lambda ctx=ctx: torch.zeros_like(ctx)))
            out.append(dict(c, model_conds=mc))
        return out

    cond = rebuilt(cond, "cond", new_y)
    uncond = rebuilt(uncond, "uncond", torch.zeros_like(new_y)) if uncond is not None else None
    return model, x, timestep, uncond, cond, cond_scale, model_options, seed


def patch_revision(unet, clip_vision_output, weight, noise_aug=0.0, ignore_prompt=False):
    """-> a clone of `unet` (a UnetPatcher) with one more Revision unit: clip_vision_output is encode_image's Output (its image_embeds [b, 1280]
    are read).  The modifier is installed once, however many units the job carries."""
    model = unet.model
    adm = getattr(getattr(getattr(model, "diffusion_model", None), "layout", None), "adm_in_channels", None)
    if adm != Y_WIDTH:
        raise NotImplementedError(f"{FEATURE}: the model's `y` is {adm} wide, SDXL's is {Y_WIDTH}: Revision replaces the pooled text embedding of SDXL")
    if getattr(model, "noise_augmentor", None) is not None:
        raise NotImplementedError(f"{FEATURE}: the model has a noise_augmentor (an unCLIP checkpoint); only SDXL's plain `y` is supported")
    embeds = clip_vision_output["image_embeds"]
    if embeds.dim() != 2 or embeds.shape[-1] < EMBED_WIDTH:
        raise ValueError(f"{FEATURE}: image_embeds {tuple(embeds.shape)}; the CLIP-G embedding is [b, {EMBED_WIDTH}]")
    m = unet.clone()
    m.model_options.pop("revision_cache", None)          # (the modifier's memo belongs to one set of units)
    m.model_options["revision_conditions"] = list(m.model_options.get("revision_conditions", [])) + [
        dict(cond=clip_vision_output, weight=float(weight), noise_aug=float(noise_aug), ignore_prompt=bool(ignore_prompt))]
    mods = list(m.model_options.get("conditioning_modifiers", []))
    if revision_conditioning_modifier not in mods:
        mods.append(revision_conditioning_modifier)
    m.model_options["conditioning_modifiers"] = mods
    return m
