"""Storage-quantised checkpoints on the host side: float8 tensors and bitsandbytes 4-bit (NF4 / FP4) tensors of a state dict become
`PackedTensor(scheme, shape, data, state)` wrappers that carry the LOGICAL shape, as `gguf_file.GGUFTensor` does; `loader.dequantize_state_dict`
sends their bytes to the device and expands them there (hipops.fp8_expand / hipops.bnb4_dequant) into the resident 16-bit weights.

The reference keeps fp8 weights and casts them in every forward (backend/operations.py:353-389); it keeps bnb weights packed and calls the
bitsandbytes library in every forward (backend/operations_bnb.py).  Which tensors of a component are stored how follows
backend/memory_management.py:311-337 (`state_dict_dtype`: the bnb marker keys first, else the majority dtype) and backend/loader.py:81-174
(`component_storage` and `mirror_fp8_storage` below).

The bitsandbytes packed format (`QuantState.as_dict(packed=True)` / `from_dict`).  Next to `<p>weight` (uint8, `[(n + 1) / 2, 1]`) the dict holds
  <p>weight.quant_map                           fp32, 16 values
  <p>weight.absmax                              fp32 when not nested, uint8 when nested
  <p>weight.nested_absmax                       fp32, nested only
  <p>weight.nested_quant_map                    fp32, 256 values, nested only
  <p>weight.quant_state.bitsandbytes__nf4|fp4   uint8, the bytes of a UTF-8 JSON object: quant_type, blocksize, dtype, shape and, nested,
                                                nested_blocksize, nested_dtype, nested_offset
Neither the library nor a genuine NF4 file is available where this was written and the reference contains none of the library's arithmetic:
format and arithmetic are parity-UNPINNED against bitsandbytes."""
import json
from collections import namedtuple

import torch

FP8_SCHEMES = {torch.float8_e4m3fn: "fp8_e4m3fn", torch.float8_e5m2: "fp8_e5m2"}
FP8_DTYPES = {v: k for k, v in FP8_SCHEMES.items()}
BNB_SCHEMES = ("nf4", "fp4")
BNB_MARKER = ".quant_state.bitsandbytes__"
BNB_SIDE_KEYS = (".quant_map", ".absmax", ".nested_absmax", ".nested_quant_map")

BnbQuantState = namedtuple("BnbQuantState", "quant_type shape blocksize code absmax nested code2 absmax2 blocksize2 offset dtype")


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


class PackedTensor(namedtuple("PackedTensor", "scheme shape data state")):
    """One storage-quantised tensor: `scheme` 'fp8_e4m3fn' | 'fp8_e5m2' | 'nf4' | 'fp4', `shape` the logical shape (a torch.Size), `data` the stored
    bytes (a flat uint8 host tensor), `state` the BnbQuantState of a 4-bit tensor (None for fp8)."""
    __slots__ = ()

    @property
    def numel(self):
        return _numel(self.shape)

    def dim(self):
        return len(self.shape)

    def size(self, i=None):
        return self.shape if i is None else self.shape[i]

    @property
    def is_fp8(self):
        return self.scheme in FP8_DTYPES

    def host_float(self):
        """fp8 only: the exact fp32 values, on the host (torch's CPU conversion) -- for the few places that read values before the expansion"""
        if not self.is_fp8:
            raise NotImplementedError(f"host values of a {self.scheme} tensor")
        return self.data.view(FP8_DTYPES[self.scheme]).float().reshape(self.shape)


def is_packed(v):
    return isinstance(v, PackedTensor)


def pack_fp8(t):
    """a float8 host / device tensor -> PackedTensor over its bytes"""
    t = t.detach().contiguous()
    return PackedTensor(FP8_SCHEMES[t.dtype], t.shape, t.view(torch.uint8).reshape(-1).cpu(), None)


def round_to_fp8(t, scheme):
    """a wider tensor -> PackedTensor holding it ROUNDED to fp8 with torch's CPU conversion (non-saturating: 500 becomes NaN in e4m3fn), which is
    what `load_state_dict` into an fp8 module does in the reference (backend/loader.py:155-162)"""
    return pack_fp8(t.detach().cpu().to(FP8_DTYPES[scheme]))


def parse_bnb_quant_state(sd, weight_key):
    """-> BnbQuantState of the packed tensor `sd[weight_key]`, read from its side keys.  Malformed input raises ValueError naming the key."""
    marker = next((weight_key + BNB_MARKER + q for q in BNB_SCHEMES if weight_key + BNB_MARKER + q in sd), None)
    if marker is None:
        raise ValueError(f"{weight_key}: no {weight_key}{BNB_MARKER}nf4 / fp4 key beside it")
    try:
        meta = json.loads(bytes(sd[marker].detach().cpu().reshape(-1).to(torch.uint8).tolist()).decode("utf-8"))
    except (ValueError, UnicodeDecodeError) as e:
        raise ValueError(f"{marker}: not UTF-8 JSON ({e})") from e
    if not isinstance(meta, dict):
        raise ValueError(f"{marker}: not a JSON object")
    quant_type = meta.get("quant_type")
    if quant_type not in BNB_SCHEMES or quant_type != marker.rsplit("__", 1)[1]:
        raise ValueError(f"{marker}: unknown quant_type {quant_type!r} (nf4 and fp4 are served, and must match the key)")

    def need(suffix, dtype, numel=None):
        k = weight_key + suffix
        if k not in sd:
            raise ValueError(f"{k}: missing (side key of the bitsandbytes {quant_type} tensor {weight_key})")
        t = sd[k]
        if t.dtype != dtype:
            raise ValueError(f"{k}: stored as {t.dtype}, expected {dtype}")
        if numel is not None and t.numel() != numel:
            raise ValueError(f"{k}: {t.numel()} values, expected {numel}")
        return t.detach().reshape(-1).contiguous()

    for field in ("blocksize", "shape"):
        if field not in meta:
            raise ValueError(f"{marker}: field {field!r} missing")
    shape = torch.Size(int(s) for s in meta["shape"])
    n = _numel(shape)
    packed = sd[weight_key]
    if packed.dtype != torch.uint8 or n <= 0 or packed.numel() != (n + 1) // 2:
        raise ValueError(f"{weight_key}: {packed.numel()} bytes of {packed.dtype} do not hold the shape {tuple(shape)} its quant state gives")
    blocksize = int(meta["blocksize"])
    if blocksize < 64 or blocksize > 4096 or blocksize & (blocksize - 1):
        raise ValueError(f"{marker}: blocksize {blocksize} is not a power of two from 64 to 4096")
    nblocks = (n + blocksize - 1) // blocksize
    code = need(".quant_map", torch.float32, 16)
    nested = (weight_key + ".nested_absmax") in sd or "nested_blocksize" in meta
    dtype = getattr(torch, str(meta.get("dtype", "float16")), None)
    if nested:
        for field in ("nested_blocksize", "nested_offset"):
            if field not in meta:
                raise ValueError(f"{marker}: field {field!r} missing")
        blocksize2 = int(meta["nested_blocksize"])
        if blocksize2 < 64 or blocksize2 & (blocksize2 - 1):
            raise ValueError(f"{marker}: nested_blocksize {blocksize2} is not a power of two of at least 64")
        absmax = need(".absmax", torch.uint8, nblocks)
        absmax2 = need(".nested_absmax", torch.float32, (nblocks + blocksize2 - 1) // blocksize2)
        code2 = need(".nested_quant_map", torch.float32, 256)
        return BnbQuantState(quant_type, shape, blocksize, code, absmax, True, code2, absmax2, blocksize2, float(meta["nested_offset"]), dtype)
    absmax = need(".absmax", torch.float32, nblocks)
    return BnbQuantState(quant_type, shape, blocksize, code, absmax, False, None, None, 0, 0.0, dtype)


def wrap_quantized_state_dict(sd):
    """-> a dict in which every float8 tensor and every bitsandbytes 4-bit tensor of `sd` is a PackedTensor carrying its logical shape; the bnb
    side keys are consumed (they never appear as model keys); everything else passes through.  A dict without such tensors is returned as is."""
    markers = [k for k in sd if BNB_MARKER in k]
    if not markers and not any(isinstance(v, torch.Tensor) and v.dtype in FP8_SCHEMES for v in sd.values()):
        return sd
    out = dict(sd)
    for marker in markers:
        wk = marker[:marker.index(BNB_MARKER)]
        if wk not in sd:
            raise ValueError(f"{marker}: the packed tensor {wk} it describes is missing")
        state = parse_bnb_quant_state(sd, wk)
        out[wk] = PackedTensor(state.quant_type, state.shape, sd[wk].detach().reshape(-1).contiguous(), state)
        for k in [marker] + [wk + s for s in BNB_SIDE_KEYS]:
            out.pop(k, None)
    for k, v in out.items():
        if isinstance(v, torch.Tensor) and v.dtype in FP8_SCHEMES:
            out[k] = pack_fp8(v)
    return out


def component_storage(sd):
    """backend/memory_management.py:311-337 `state_dict_dtype` on one component's (wrapped) dict: 'gguf' / 'nf4' / 'fp4' when such a tensor is
    met, else the dtype most tensors are stored in (counted per tensor; a tie goes to the first seen).  fp8 comes back as its scheme name."""
    from .gguf_file import GGUFTensor
    for v in sd.values():
        if isinstance(v, GGUFTensor):
            return "gguf"
        if is_packed(v) and v.scheme in BNB_SCHEMES:
            return v.scheme
    counts = {}
    for v in sd.values():
        d = v.scheme if is_packed(v) else v.dtype
        counts[d] = counts.get(d, 0) + 1
    major, top = None, 0
    for d, c in counts.items():
        if c > top:
            major, top = d, c
    return major


# Parameters the reference does not build through its operations and that no `.to(dtype)` reaches, so that fp8 storage leaves them fp32 holding the
# stored values exactly: the T5's layer norms (raw nn.Parameter) and its two embeddings (plain nn.Embedding).  The UNet and the Flux transformer
# are moved as a whole (`.to(dtype=fp8)`): nothing is kept.  Recorded from the reference in tests/golden/quant_reference.json (tools/make_quant_fixtures.py).
T5_KEPT_FP32 = ("layer_norm.weight", "relative_attention_bias.weight", "shared.weight")


def fp8_storage_dtype(component, key):
    """the type a parameter of `component` ('flux' | 'unet' | 't5') ends up in when the component's storage type is fp8: 'fp8' or torch.float32"""
    if component == "t5" and key.endswith(T5_KEPT_FP32):
        return torch.float32
    return "fp8"


def mirror_fp8_storage(sd, component):
    """What the reference's fp8 storage does to one component, on the host.  When the component's storage type (`component_storage`) is float8,
    the reference builds the module in that type and `load_state_dict` copies into it: wider-stored tensors are ROUNDED to fp8 (here: torch's CPU
    conversion, then the same device expansion as the stored fp8 tensors), except the parameters `fp8_storage_dtype` lists, which become fp32
    holding the stored values.  Any other storage type: unchanged (stray fp8 tensors are then expanded exactly, as a cast to the module's type is)."""
    storage = component_storage(sd)
    if storage not in FP8_DTYPES:
        return sd
    out = {}
    for k, v in sd.items():
        kept = fp8_storage_dtype(component, k) != "fp8"
        if is_packed(v) and v.is_fp8:
            out[k] = v.host_float() if kept else (v if v.scheme == storage else round_to_fp8(v.host_float(), storage))
        elif isinstance(v, torch.Tensor) and v.is_floating_point():
            out[k] = v.float() if kept else round_to_fp8(v, storage)
        else:
            out[k] = v
    return out
