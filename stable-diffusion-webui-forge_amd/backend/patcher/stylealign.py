"""Native StyleAlign -- the patcher-level entry (reference: extensions-builtin/sd_forge_stylealign/scripts/forge_stylealign.py, "StyleAlign
Integrated", "Share attention in batch").

The reference installs a Python attn1 replace patch on every transformer block (set_model_replace_all(attn1_proc, "attn1")): per group of the
call (the cond images, the uncond images) the self-attention runs over the tokens of all images of the group joined into one sequence, or is
blended with the ordinary one.  Here the strength travels as the plain transformer option "stylealign", which KModel reads on the fused route and
hands to the UNet executor as `share` (backend/nn/unet.py): a group of consecutive images already is one contiguous sequence in the executor's
[Q | K] and V^T buffers, so the shared attention is the existing kernel with other strides, and the step stays on the captured graph."""
from collections import namedtuple

StyleAlignParams = namedtuple("StyleAlignParams", ["strength"])
Share = namedtuple("Share", ["b", "mode", "strength"])      # what the executor gets: images per group, "aligned" | "blend", the strength

OPTION = "stylealign"
FEATURE = "StyleAlign"


def mode_of(strength):
    """the reference's thresholds (forge_stylealign.py:67-82): "plain" below 0.01, "aligned" above 0.99, else "blend" """
    if strength < 0.01:
        return "plain"
    if strength > 0.99:
        return "aligned"
    return "blend"


def patch_stylealign(unet_patcher, strength=1.0):
    """-> a clone of `unet_patcher` that shares self-attention in the batch (the reference UI's checkbox on, its strength field).  A strength
    below 0.01 is ordinary attention: the clone carries no option at all."""
    from ..modules.k_model import KModelFlux
    if isinstance(unet_patcher.model, KModelFlux):
        raise NotImplementedError(f"{FEATURE}: UNet models only")
    m = unet_patcher.clone()
    if mode_of(float(strength)) != "plain":
        m.set_transformer_option(OPTION, StyleAlignParams(float(strength)))
    return m


def mode(unet_patcher):
    """the mode a patcher runs in: "plain" without the option"""
    opt = unet_patcher.model_options.get("transformer_options", {}).get(OPTION)
    return "plain" if opt is None else mode_of(opt.strength)


def share_for_call(transformer_options, b):
    """-> the Share of a model call whose row groups hold `b` images each, or None: no option, a strength below the reference's threshold, or
    groups of one image, where joining changes nothing (the plain route, the plain graph)"""
    opt = (transformer_options or {}).get(OPTION)
    if opt is None or b <= 1:
        return None
    m = mode_of(opt.strength)
    return None if m == "plain" else Share(int(b), m, float(opt.strength))


def share_graph_key(share):
    """what the option adds to a static-buffer key and a graph key; the blend weights are launch arguments baked into the capture"""
    return (OPTION, share.mode, share.strength)


def group_size_of_call(transformer_options, batch):
    """The images per group of an apply_model call of `batch` rows: the reference's attn1_proc walks transformer_options["cond_or_uncond"] and
    takes ALL cond (or uncond) indices per entry, so a call that carries a value twice (two cond entries batched into one call, from AND-composed
    prompts) makes it return more rows than it was given.  Such calls, and calls without the key, are refused."""
    cou = (transformer_options or {}).get("cond_or_uncond")
    if cou is None:
        raise NotImplementedError(f"{FEATURE}: the model call carries no transformer_options['cond_or_uncond'], so its groups are unknown")
    cou = list(cou)
    if len(set(cou)) != len(cou):
        raise NotImplementedError(f"{FEATURE}: cond_or_uncond = {cou} repeats a value (AND-composed or weighted conditionings batched into one call); "
                                  "the reference's attn1_proc is only well-formed for at most one cond and one uncond entry per call")
    if len(cou) == 0 or batch % len(cou) != 0:
        raise NotImplementedError(f"{FEATURE}: a batch of {batch} rows does not split into the {len(cou)} groups of cond_or_uncond")
    return batch // len(cou)


def check_world(transformer_options, world_size):
    """The sharded entry splits a job's batch over the ranks, which would shrink the groups: refused, before any collective."""
    if (transformer_options or {}).get(OPTION) is not None and world_size > 1:
        raise NotImplementedError(f"{FEATURE} with a batch sharded over {world_size} ranks: the images of a group would no longer share one "
                                  "attention; run the job on one rank")
