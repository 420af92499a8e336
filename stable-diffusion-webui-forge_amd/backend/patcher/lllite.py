"""Native ControlNet-LLLite -- the patcher-level entry (reference: extensions-builtin/sd_forge_controlllite, lib_controllllite.py and the
ControlLLLitePatcher of forge_controllllite.py).

An LLLite file is no second network: per q / k / v projection of a transformer block it holds one small module -- a conditioning chain on the
control image (computed once: the cond embedding [Bc, n, E]) and a 64-wide bottleneck MLP on the rows that feed the projection,
    x + up(relu(mid(cat([cond_emb, relu(down(x))])))) * strength.
The reference installs that as a Python attn1_patch + attn2_patch pair.  Here the loaded modules travel as the plain transformer option "lllite",
which KModel reads on the fused route (window test on the host, per model call) and hands to the UNet executor: a block that has modules computes
its norm unfolded and makes the three operands with one launch of fmxl_lllite_adapt_f16 (hipops.lllite_adapt), and the step stays on the captured
graph.  `python_patch` is the same arithmetic as a Python patch pair, written here: what the hooked executor runs when the native route does not
apply (a token count that is no multiple of 64, a second LLLite unit), and what tests and tools/bench_features.py compare against."""
import math
import re

import torch

OPTION = "lllite"
FEATURE = "ControlNet-LLLite"
HIDDEN, EMBED = 64, 32       # what the kernel is built for, and what every published file uses

_NAME = re.compile(r"lllite_unet_(input_blocks_(\d+)_1|middle_block_1|output_blocks_(\d+)_1)_transformer_blocks_(\d+)_(attn[12])_to_([qkv])")


def split_modules(state_dict):
    """{module name: {weight name: tensor}}: a key's first dotted fragment names the module"""
    out = {}
    for key, value in state_dict.items():
        name, _, rest = key.partition(".")
        out.setdefault(name, {})[rest] = value
    return out


def module_depth(weights):
    """how far the conditioning chain shrinks the control image: a third convolution means 32x (depth 3), a 4 x 4 second one 16x (2), else 8x (1)"""
    if "conditioning1.4.weight" in weights:
        return 3
    return 2 if weights["conditioning1.2.weight"].shape[-1] == 4 else 1


def module_target(name):
    """module name -> (this executor's block name, "attn1" | "attn2", "q" | "k" | "v")"""
    m = _NAME.fullmatch(name)
    if m is None:
        raise ValueError(f"{FEATURE}: module name {name!r} names no transformer block projection")
    if m.group(2) is not None:
        layer = f"input_blocks.{m.group(2)}.1"
    elif m.group(3) is not None:
        layer = f"output_blocks.{m.group(3)}.1"
    else:
        layer = "middle_block.1"
    return f"{layer}.transformer_blocks.{m.group(4)}", m.group(5), m.group(6)


def block_name_of_options(extra_options):
    """the block a transformer patch is called for, in this executor's names, from its extra_options (block = (kind, number), block_index)"""
    kind, number = extra_options["block"][0], extra_options["block"][1]
    layer = {"input": f"input_blocks.{number}.1", "middle": "middle_block.1", "output": f"output_blocks.{number}.1"}.get(kind)
    if layer is None:
        raise ValueError(f"{FEATURE}: a transformer block of {kind!r}")
    return f"{layer}.transformer_blocks.{extra_options['block_index']}"


def step_window(steps, start_percent, end_percent):
    """-> (start_step, end_step): a percentage of 0 means "from the first call" / "to the last" """
    start = math.floor(steps * start_percent) if start_percent > 0 else 0
    end = math.floor(steps * end_percent) if end_percent > 0 else steps
    return start, end


class CallCounter:
    """The reference's per-module counter: it advances once per MODEL CALL, not per sampler step, and starts over at `steps` -- a sampler that
    calls the model twice per step runs through the window twice as fast and wraps.  steps == 0: always on, nothing counted."""

    def __init__(self, steps, start_percent, end_percent):
        self.steps = int(steps)
        self.start, self.end = step_window(self.steps, start_percent, end_percent)
        self.current = 0

    def advance(self):
        """one model call -> whether the adapters apply to it"""
        if self.steps <= 0:
            return True
        now = self.current
        self.current += 1
        if now < self.start:
            return False          # (the reference does not wrap here either: start < steps always ends this branch first)
        if self.current >= self.steps:
            self.current = 0
        return now < self.end

    def reset(self):
        self.current = 0


def _space_to_depth(x, k):
    """NHWC [B, H, W, C] -> [B * (H // k) * (W // k), k * k * C], the rows a kernel = stride = k convolution multiplies (tails cropped)"""
    b, h, w, c = x.shape
    x = x[:, :h // k * k, :w // k * k]
    return x.reshape(b, h // k, k, w // k, k, c).permute(0, 1, 3, 2, 4, 5).reshape(b * (h // k) * (w // k), k * k * c), h // k, w // k


class LLLite:
    """The modules of one LLLite file on one control image.  blocks[block name]["attn1" | "attn2"] = [q, k, v] slots (None: no module), each a dict
    of contiguous tensors (fp16 on the GPU) for hipops.lllite_adapt plus "name" and "conv" (the conditioning chain as [(weight [out, k*k*in] K-padded, bias, k)])."""

    def __init__(self, state_dict, cond_image_bhwc, strength, steps, start_percent, end_percent, device):
        self.strength = float(strength)
        self.steps, self.start_percent, self.end_percent = int(steps), float(start_percent), float(end_percent)
        self.counter = CallCounter(steps, start_percent, end_percent)
        self.device = torch.device(device)
        # fp16 on the GPU, where both routes run; off it (the Python route on the CPU: tests against the reference's fp32 run) the file's own precision
        self.dtype = torch.float16 if self.device.type == "cuda" else torch.float32
        self.blocks, self.modules = {}, {}
        mods = split_modules(state_dict)
        if not mods:
            raise ValueError(f"{FEATURE}: empty state dict")
        for name, w in mods.items():
            block, attn, proj = module_target(name)
            if w["down.0.weight"].ndim == 4:
                raise NotImplementedError(f"{FEATURE}: {name} is a Conv2d module (is_conv2d): only the Linear modules of transformer blocks have a route")
            d, e = int(w["down.0.weight"].shape[0]), int(w["conditioning1.0.weight"].shape[0]) * 2
            if d != HIDDEN or e != EMBED:
                raise NotImplementedError(f"{FEATURE}: {name} has hidden width {d} and cond embedding width {e}; the kernel is built for "
                                          f"{HIDDEN} and {EMBED}")
            if attn == "attn2" and proj != "q":
                raise NotImplementedError(f"{FEATURE}: {name} adapts the {proj} projection of a cross-attention, whose rows are the text tokens: the "
                                          "cond embedding has one row per image token")
            depth = module_depth(w)
            last = 4 if depth == 3 else 2       # the chain's last convolution: conditioning1.{0, 2} or conditioning1.{0, 2, 4}
            if w[f"conditioning1.{last}.weight"].shape[0] != e or w["mid.0.weight"].shape[1] != d + e:
                raise ValueError(f"{FEATURE}: {name}: the conditioning chain ends at {w[f'conditioning1.{last}.weight'].shape[0]} channels, "
                                 f"mid takes {w['mid.0.weight'].shape[1]}")
            t = lambda v: v.detach().to(device=self.device, dtype=self.dtype).contiguous()   # noqa: E731
            conv = []
            for i in range(0, last + 1, 2):
                cw = w[f"conditioning1.{i}.weight"]
                k = int(cw.shape[-1])
                flat = cw.permute(0, 2, 3, 1).reshape(cw.shape[0], -1)               # [out, ky, kx, in]: the order of _space_to_depth's columns
                pad = -flat.shape[1] % 64                                            # the GEMM's K granule
                conv.append((t(torch.nn.functional.pad(flat, (0, pad))), t(w[f"conditioning1.{i}.bias"]), k))
            slot = {"name": name, "depth": depth, "conv": conv, "wd": t(w["down.0.weight"]), "bd": t(w["down.0.bias"]),
                    "wm": t(w["mid.0.weight"]), "bm": t(w["mid.0.bias"]), "wu": t(w["up.0.weight"]), "bu": t(w["up.0.bias"])}
            self.blocks.setdefault(block, {"attn1": [None, None, None], "attn2": [None, None, None]})[attn]["qkv".index(proj)] = slot
            self.modules[name] = slot
        # the control image: [Bc, H, W, 3] in 0 .. 1 -> -1 .. 1 (fp32 here; each route casts it)
        self.cond_image = cond_image_bhwc.detach().to(device=self.device, dtype=torch.float32) * 2.0 - 1.0
        if self.cond_image.dim() != 4 or self.cond_image.shape[-1] != 3:
            raise ValueError(f"{FEATURE}: the control image must be [B, H, W, 3], got {tuple(self.cond_image.shape)}")
        self._emb = {}          # module name -> cond embedding [Bc, n, E] fp16 (native) -- computed once
        self._emb_f32 = {}      # the same in fp32 through torch, for python_patch off the GPU
        self.serial = next(_serials)

    # ---- the cond embedding ---------------------------------------------------------------------------------------------------------------
    def emb_rows(self, slot):
        """rows per image of a module's cond embedding, from the control image's size alone"""
        h, w = int(self.cond_image.shape[1]), int(self.cond_image.shape[2])
        for _, _, k in slot["conv"]:
            h, w = h // k, w // k
        return h * w

    def cond_emb(self, slot):
        """[Bc, n, 32] fp16 on the device, cached: space-to-depth views, the existing GEMM (K padded to 64) and the existing ReLU kernel"""
        emb = self._emb.get(slot["name"])
        if emb is None:
            from ... import hipops as ops
            x = self.cond_image.to(torch.float16)
            bc = x.shape[0]
            for i, (wgt, bias, k) in enumerate(slot["conv"]):
                rows, h, w = _space_to_depth(x, k)
                a = torch.zeros(rows.shape[0], wgt.shape[1], dtype=torch.float16, device=self.device)
                a[:, :rows.shape[1]] = rows
                y = ops.linear(a, wgt, bias, out=torch.empty(rows.shape[0], wgt.shape[0], dtype=torch.float16, device=self.device))
                if i + 1 < len(slot["conv"]):
                    y = ops.act(y, ops.ACT_RELU, out=y)
                x = y.view(bc, h, w, -1)
            emb = self._emb[slot["name"]] = x.reshape(bc, -1, x.shape[-1]).contiguous()
        return emb

    def cond_emb_torch(self, slot, dtype):
        """the same embedding through torch's conv2d in `dtype` (python_patch on the CPU; the tests' yardstick for cond_emb)"""
        key = (slot["name"], dtype)
        emb = self._emb_f32.get(key)
        if emb is None:
            x = self.cond_image.permute(0, 3, 1, 2).to(dtype)
            for i, (wgt, bias, k) in enumerate(slot["conv"]):
                cin = x.shape[1]
                w4 = wgt[:, :k * k * cin].reshape(wgt.shape[0], k, k, cin).permute(0, 3, 1, 2).to(dtype)
                x = torch.nn.functional.conv2d(x, w4, bias.to(dtype), stride=k)
                if i + 1 < len(slot["conv"]):
                    x = torch.relu(x)
            emb = self._emb_f32[key] = x.flatten(2).permute(0, 2, 1).contiguous()
        return emb

    def prepare(self):
        """every module's embedding, outside any capture"""
        for slot in self.modules.values():
            self.cond_emb(slot)

    def check_rows(self, block, n, bu):
        """refusal before any launch: a block whose image has n tokens needs embeddings of n rows, and the batch must tile the cond images"""
        bc = int(self.cond_image.shape[0])
        if bu % bc != 0:
            raise NotImplementedError(f"{FEATURE}: a batch of {bu} images is no multiple of the {bc} control images")
        for slots in self.blocks[block].values():
            for slot in slots:
                if slot is not None and self.emb_rows(slot) != n:
                    raise NotImplementedError(f"{FEATURE}: {slot['name']}: the control image gives a cond embedding of {self.emb_rows(slot)} rows, "
                                              f"the block has {n} tokens per image (the control image must be 8x the latent's size)")

    def native_ok(self):
        """whether every module's embedding has a multiple of 64 rows (what fmxl_lllite_adapt_f16 tiles by)"""
        return all(self.emb_rows(s) % 64 == 0 and self.emb_rows(s) > 0 for s in self.modules.values())

    # ---- the Python route -----------------------------------------------------------------------------------------------------------------
    def python_patch(self):
        """-> one callable for set_model_attn1_patch AND set_model_attn2_patch: (q, k, v, extra_options) -> (q, k, v), the inputs of to_q / to_k /
        to_v each replaced by x + module(x) where the block has a module.  Every module keeps a call counter of its own, as the reference's do."""
        return PythonPatch(self)


_serials = iter(range(1, 1 << 62))


class PythonPatch:
    def __init__(self, lll):
        self.lll = lll
        self.counters = {name: CallCounter(lll.steps, lll.start_percent, lll.end_percent) for name in lll.modules}

    def module(self, slot, x):
        """module(x) * strength in x's dtype, or None outside the window"""
        if not self.counters[slot["name"]].advance():
            return None
        lll = self.lll
        emb = lll.cond_emb(slot) if x.is_cuda else lll.cond_emb_torch(slot, x.dtype)
        emb = emb.to(x.dtype)
        if emb.shape[1] != x.shape[1]:
            raise NotImplementedError(f"{FEATURE}: {slot['name']}: the control image gives a cond embedding of {emb.shape[1]} rows, the block has "
                                      f"{x.shape[1]} tokens per image (the control image must be 8x the latent's size)")
        if x.shape[0] != emb.shape[0]:
            emb = emb.repeat(x.shape[0] // emb.shape[0], 1, 1)        # image i uses embedding i % Bc
        lin = lambda v, w, b: torch.nn.functional.linear(v, slot[w].to(x.dtype), slot[b].to(x.dtype))   # noqa: E731
        d = torch.relu(lin(x, "wd", "bd"))
        m = torch.relu(lin(torch.cat([emb, d], dim=2), "wm", "bm"))
        return lin(m, "wu", "bu") * lll.strength

    def __call__(self, q, k, v, extra_options):
        entry = self.lll.blocks.get(block_name_of_options(extra_options))
        if entry is None:
            return q, k, v
        slots = entry["attn1" if q.shape[-1] == k.shape[-1] else "attn2"]    # a self-attention's three inputs have one width
        out = []
        for x, slot in zip((q, k, v), slots):
            if slot is not None:
                add = self.module(slot, x)
                if add is not None:
                    x = x + add
            out.append(x)
        return tuple(out)


def _refuse_companions(unet_patcher):
    from .native_call import message
    to = unet_patcher.model_options.get("transformer_options", {})
    if unet_patcher.model_options.get("pag") is not None:
        raise NotImplementedError(message("lllite", "pag_from"))
    if to.get("stylealign") is not None:
        raise NotImplementedError(message("lllite", "share"))
    if to.get("kohya_hrfix") is not None:
        raise NotImplementedError(message("lllite", "shrink"))


def _has_foreign_hooks(to):
    """Python block hooks other than LLLite's own patch pairs"""
    from ..nn.unet import IntegratedUNet2DConditionModel as Net
    rest = dict(to)
    patches = {k: [p for p in v if not isinstance(p, PythonPatch)] for k, v in (to.get("patches") or {}).items()}
    rest["patches"] = {k: v for k, v in patches.items() if v}
    return Net._hooks(rest) is not None


def patch_lllite(unet_patcher, state_dict, cond_image_bhwc, strength=1.0, steps=0, start_percent=0.0, end_percent=0.0):
    """-> a clone of `unet_patcher` that applies the LLLite file `state_dict` on the control image `cond_image_bhwc` ([Bc, H, W, 3], 0 .. 1), the
    reference's LLLiteLoader.load_lllite.  The clone carries the transformer option "lllite" (the native route) -- or, where that route does not
    apply (an embedding whose rows are no multiple of 64, a second LLLite unit on the job), the same arithmetic as Python attn1 / attn2 patches.
    Refused (NotImplementedError, before any launch): Flux, Conv2d modules, other widths than 64 / 32, modules on attn2's k / v, native
    Perturbed-Attention Guidance / StyleAlign / Kohya HRFix or Python block hooks on the same job."""
    from ..modules.k_model import KModelFlux
    if isinstance(unet_patcher.model, KModelFlux):
        raise NotImplementedError(f"{FEATURE}: UNet models only")
    _refuse_companions(unet_patcher)
    to = unet_patcher.model_options.get("transformer_options", {})
    if _has_foreign_hooks(to):
        raise NotImplementedError(f"{FEATURE} together with Python block hooks in transformer_options")
    device = getattr(unet_patcher.model, "device", None) or unet_patcher.load_device or cond_image_bhwc.device
    lll = LLLite(state_dict, cond_image_bhwc, strength, steps, start_percent, end_percent, device)
    m = unet_patcher.clone()
    mto = m.model_options["transformer_options"]
    first = mto.get(OPTION)
    python_units = any(isinstance(p, PythonPatch) for p in (mto.get("patches") or {}).get("attn1_patch", []))
    if first is None and not python_units and lll.native_ok():
        m.set_transformer_option(OPTION, lll)
        return m
    # the Python route: this unit, and the unit that was native until now (the reference chains the patches in the order they were installed)
    units = ([first] if first is not None else []) + [lll]
    mto.pop(OPTION, None)
    for unit in units:
        patch = unit.python_patch()
        m.set_model_attn1_patch(patch)
        m.set_model_attn2_patch(patch)
    return m


def lllite_of(transformer_options):
    return (transformer_options or {}).get(OPTION)


def lllite_for_call(transformer_options):
    """One model call on the fused route -> the LLLite whose adapters apply to it, or None (no option, or outside the window: the plain call, the
    plain graph).  Advances the call counter, so it runs once per model call and after the call's refusals (native_call.resolve_call)."""
    lll = lllite_of(transformer_options)
    if lll is None or not lll.counter.advance():
        return None
    return lll


def lllite_graph_key(lll):
    """what the option adds to a static-buffer key and a graph key inside the window: the weights and embeddings are captured addresses (the unit's
    serial stands for them, as id() would, without being reused after the unit is gone), the strength a launch argument"""
    return (OPTION, lll.serial, lll.strength)


def check_world(transformer_options, world_size):
    """The sharded entry splits a job's batch over the ranks; image i of a call uses control image i % Bc, so a shard would pair other images with
    other control images: refused, before any collective."""
    opt = (transformer_options or {}).get(OPTION)
    python_units = any(isinstance(p, PythonPatch) for p in ((transformer_options or {}).get("patches") or {}).get("attn1_patch", []))
    if (opt is not None or python_units) and world_size > 1:
        raise NotImplementedError(f"{FEATURE} with a batch sharded over {world_size} ranks: every rank would pair its images with the control "
                                  "images from the first one on; run the job on one rank")


class ControlLLLitePatcher:
    """The control-unit entry (the reference's ControlLLLitePatcher): built from a control model file whose keys carry 'lllite'; before every
    sampling pass it patches the job's UNet with the unit's image, weight and window."""

    @staticmethod
    def try_build_from_state_dict(state_dict, ckpt_path=None):
        if not any("lllite" in k for k in state_dict.keys()):
            return None
        return ControlLLLitePatcher(state_dict)

    def __init__(self, state_dict):
        self.state_dict = state_dict
        self.strength = 1.0
        self.start_percent = 0.0
        self.end_percent = 1.0

    def process_before_every_sampling(self, process, cond, mask=None, *args, **kwargs):
        """cond: the unit's control image [B, 3, H, W] in 0 .. 1"""
        objs = process.sd_model.forge_objects
        objs.unet = patch_lllite(objs.unet, self.state_dict, cond.movedim(1, -1), self.strength, process.steps, self.start_percent,
                                 self.end_percent)
