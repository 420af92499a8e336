"""What one forward of the LDM UNet executor does natively -- one record (`NativeCall`), resolved once per model call (`resolve_call`), refused
by one table (`RULES`, `check`) and keyed by two functions (`static_key`, `graph_key`).  The per-feature pieces -- windows, parameters, key
tuples -- stay in the feature's own module of this package; this module only composes them.  It imports neither backend/nn/unet.py nor
backend/modules/k_model.py, which both import it."""
from collections import namedtuple

from . import freeu, ipadapter, kohya_hrfix, lllite, pag, stylealign


class NativeCall(namedtuple("NativeCall", ["freeu", "shrink", "pag_from", "share", "lllite", "ipadapter"], defaults=(None,) * 6)):
    """The native options of ONE UNet forward.  None everywhere (`PLAIN`) is the plain call on the plain graph, bit for bit; every field that is
    set runs on the executor's fast path and inside a captured graph, never as a Python hook.

    freeu      a FreeUParams tuple (b1, b2, s1, s2, ...) of freeu.py, the job's transformer_options["freeu_v2"]: FreeU v2 on the inputs of the
               output blocks whose h has 4x / 2x model_channels channels, where the reference's output_block_patch runs when FreeU is the first
               installed patch (Python output-block patches of the same job run after it, eagerly).  Its values are launch arguments of the
               captured kernels: graph key, so the steps inside and outside the FreeU window of one job are two graphs.
    shrink     a KohyaHRFixParams tuple of kohya_hrfix.py, transformer_options["kohya_hrfix"], when the step's host sigma lies inside its window
               (the caller decides; outside, None and the plain graph).  After input block `block_number` h is resized to round(extent / factor)
               -- after the skip is stored, or before it (downscale_after_skip False) -- and at every output block whose popped skip has another
               height h is resized to the skip's size, where the reference's input_block_patch(_after_skip) and output_block_patch run
               (kohya_hrfix.py:13-28).  Other kernels on other shapes: graph key.
    pag_from   the first image of the perturbed group of Perturbed-Attention Guidance (pag.py): KModel stacks [uncond ; cond ; cond] and hands
               over 2b, or b without uncond.  The images from there on get V as the self-attention output of EVERY transformer block of the
               middle block -- the reference's patches_replace key ("middle", 0) carries no block index, so it matches all of them -- and run like
               the others everywhere else.  No key of its own: such a call comes with the "pag" tag in its base key, so its static buffers (one
               more row group) and its graph are its own.
    share      the Share(b, mode, strength) of StyleAlign (stylealign.py), for row groups of b > 1 images: in EVERY transformer block of every
               level the self-attention of each group of b consecutive images runs over the group's joined tokens, or is blended with the
               ordinary one (the reference's set_model_replace_all(attn1_proc, "attn1")); attn2 is untouched.  With `pag_from` the perturbed
               group keeps V in the middle block and is one more group everywhere else.  Other attention launches, and the blend weights are
               launch arguments: static-buffer key (mode, strength).
    lllite     the ControlNet-LLLite unit (lllite.py LLLite) when this MODEL CALL lies inside its window -- the resolver advanced the unit's
               call counter.  The transformer blocks it has modules for adapt the inputs of their q / k / v projections with one launch of
               hipops.lllite_adapt.  The weights and embeddings are captured addresses, the strength a launch argument: static-buffer key
               (unit, strength).
    ipadapter  the prepared ExtraContext of IP-Adapter (ipadapter.py) when the step's host sigma lies inside the window of at least one unit.
               Every cross-attention adds the units' image-token attention to the text attention.  The cached image K / V^T are captured
               addresses, the weights launch arguments: static-buffer key (the active units, each one's identity, weight and weight type, the
               group order)."""
    __slots__ = ()


PLAIN = NativeCall()

# field of the record -> the feature's module: its FEATURE (the name refusals use), its OPTION, and check_world where a sharded batch breaks it
MODULES = {"freeu": freeu, "shrink": kohya_hrfix, "pag_from": pag, "share": stylealign, "lllite": lllite, "ipadapter": ipadapter}

# ---- what cannot run beside what ------------------------------------------------------------------------------------------------------------------
# Besides the record's fields a rule may exclude what the caller knows about the rest of the call:
HOOKS = "hooks"              # Python block hooks in transformer_options (the executor's `_hooks`)
CHAIN = "chain"              # a ControlNet / T2I-Adapter chain on the call
RESIDUALS = "residuals"      # residuals of such a chain that reach the UNet on this step

_IPA, _LLL, _SA, _PAG, _KOHYA = ipadapter.FEATURE, lllite.FEATURE, stylealign.FEATURE, pag.FEATURE, kohya_hrfix.FEATURE
_BESIDE_HOOKS = "{} (native) together with Python block hooks in transformer_options"

# (field, what it excludes, message), in the order they are tested: the first rule that applies is the one raised
RULES = (
    ("ipadapter", HOOKS, _BESIDE_HOOKS.format(_IPA)),
    ("ipadapter", "pag_from", f"{_IPA} with native {_PAG} on the same job: its third row group has no image tokens"),
    ("ipadapter", "lllite", f"{_IPA} with native {_LLL} on the same job"),
    ("lllite", HOOKS, _BESIDE_HOOKS.format(_LLL)),
    ("lllite", "pag_from", f"{_LLL} with native {_PAG} on the same job"),
    ("lllite", "share", f"{_LLL} with native {_SA} on the same job"),
    ("lllite", "shrink", f"{_LLL} with native {_KOHYA} on the same job: the shrunk blocks have other token counts than the cond embedding"),
    ("share", HOOKS, _BESIDE_HOOKS.format(_SA)),
    ("pag_from", HOOKS, _BESIDE_HOOKS.format(_PAG)),
    ("pag_from", "shrink", f"{_PAG} and {_KOHYA} on the same step: the degraded pass of the reference runs through the shrink patches as well; "
                           "that combination has no native route"),
    ("pag_from", CHAIN, f"{_PAG} with a ControlNet / T2I-Adapter chain: the chain has no third group of rows"),
    ("shrink", "freeu", f"{_KOHYA} and native {freeu.FEATURE} on one job: {freeu.FEATURE} needs h and the skip at one size, and the two do not commute"),
    # the reference prints a warning and drops the residuals whose size no longer fits; a silently dropped ControlNet is refused here
    ("shrink", RESIDUALS, f"{_KOHYA} with ControlNet / T2I-Adapter residuals: their sizes do not fit the shrunk hidden state"),
)


def message(field, excluded):
    """the text of one rule, for the patch-time refusals that word it the same way"""
    return next(text for f, e, text in RULES if (f, e) == (field, excluded))


def check(native, hooks=None, chain=False, residuals=False, fields=NativeCall._fields):
    """Refuses (NotImplementedError, before any launch) a call that holds both sides of a rule.  `hooks`: the executor's view of the call's Python
    block hooks or None; `chain`, `residuals`: what the caller knows about a ControlNet chain; `fields`: the rules of these fields only."""
    present = dict(native._asdict(), **{HOOKS: hooks, CHAIN: chain or None, RESIDUALS: residuals or None})
    for field, excluded, text in RULES:
        if field in fields and present[field] is not None and present[excluded] is not None:
            raise NotImplementedError(text)


def refuse_off_unet(transformer_options):
    """a model that is no LDM UNet (Flux) runs none of the transformer options; the reference's scripts decline such models"""
    for field in NativeCall._fields:
        m = MODULES[field]
        # (pag is a model option: sampling_function refuses it; an empty list of IP-Adapter units is no option)
        if m is not pag and (transformer_options or {}).get(m.OPTION):
            raise NotImplementedError(f"{m.FEATURE}: UNet models only")


# ---- keys --------------------------------------------------------------------------------------------------------------------------------------------
def static_key(native):
    """what the call adds to its base key (batch, channels, h, w, row groups[, "pag" | "apply"]), which names its static buffers AND starts its
    graph key: the options that launch other kernels on other captured addresses"""
    key = ()
    if native.share is not None:
        key += stylealign.share_graph_key(native.share)
    if native.lllite is not None:
        key += lllite.lllite_graph_key(native.lllite)
    if native.ipadapter is not None:
        key += native.ipadapter.graph_key()
    return key


def graph_key(native):
    """what the call adds to its graph key only, behind the ControlNet part: the options whose calls share the plain call's static buffers"""
    key = ()
    if native.freeu is not None:
        key += freeu.freeu_graph_key(native.freeu)
    if native.shrink is not None:
        key += kohya_hrfix.shrink_graph_key(native.shrink)
    return key


# ---- one model call -> its record -------------------------------------------------------------------------------------------------------------------
def resolve_call(transformer_options, b, groups, sig_host, cond_or_uncond, net, pag_step=False, chain=False):
    """One model call of KModel -> (its NativeCall, the executor's view of its Python block hooks); a call outside every window resolves to PLAIN.
    `transformer_options`: the job's; `b`: images per row group, `groups`: the row groups of the batch (the perturbed one included);
    `sig_host`: the host's copy of the step's sigmas; `cond_or_uncond`: what each group is, None when the caller does not know;
    `net`: the executor; `pag_step`: the last group is the perturbed one of Perturbed-Attention Guidance; `chain`: see check.
    Everything is refused before any launch, and a refused call does not count for ControlNet-LLLite's call counter."""
    to = transformer_options or {}
    hooks = net._hooks(to)
    pag_from = (groups - 1) * b if pag_step else None
    # 1. what an option's being on the job decides, whatever its window says about this call
    job = NativeCall(shrink=to.get(kohya_hrfix.OPTION), pag_from=pag_from, share=to.get(stylealign.OPTION), lllite=lllite.lllite_of(to),
                     ipadapter=ipadapter.units_of(to))
    check(job, hooks, fields=("ipadapter", "lllite"))
    # 2. the windows, on the host: the step's sigma, and for ControlNet-LLLite the count of model calls
    native = NativeCall(to.get(freeu.OPTION), kohya_hrfix.shrink_for_step(to, sig_host), pag_from, stylealign.share_for_call(to, b))
    check(native, hooks, chain)
    ctx = ipadapter.ipadapter_for_call(to, sig_host[0], cond_or_uncond, groups * b, net)
    lll = lllite.lllite_for_call(to)
    # 3. preparation, outside any capture (ipadapter_for_call prepared its context): the cond embeddings, once per unit
    if lll is not None:
        lll.prepare()
    return native._replace(lllite=lll, ipadapter=ctx), hooks
