"""MI355X-native CLIP-vision towers -- transformers' CLIPVisionModelWithProjection as the reference instantiates it (backend/patcher/clipvision.py):
ViT-L/14 (16 heads of 64, quick_gelu), ViT-H/14 (16 x 80) and ViT-bigG/14 (16 x 104), image 224, patch 14, 257 tokens.

Two kernels of their own (include/fmx_clipvision.h) make the front end: `clip_patch_rows` turns the preprocessed image into the [b * 256, 640] matrix
of the patch convolution (the conv weight [C, 3, 14, 14] is used as stored, zero-padded from 588 to 640 columns), one GEMM projects it, and
`clip_embed_ln` assembles class token + patches + position embedding and applies pre_layrnorm.  From there on it is the text tower's layer body
(backend/nn/clip.py) on the kernels the UNet's transformer blocks use -- q|k as one GEMM, V^T by the operand-swapped GEMM, the fused attention
kernel (not causal), out_proj + residual, fc1, activation, fc2 + residual, v_proj.bias folded into out_proj's bias -- with ONE launch each for the
whole batch: tokens live in the padded layout [b, 320, c] from the embed kernel to the last layer, so an image's rows start at a multiple of the
attention's 64-key tile and no op loops over images.

Head width 104 runs at dpad = 128: at load each head's rows of q_proj / k_proj / v_proj (and biases) are laid out 128 apart with 24 zero rows, and
out_proj gets the matching zero columns ([1664, 2048]); scale = 104 ** -0.5 is passed explicitly.  Zero rows of q and k add nothing to q . k, zero
rows of v make zero columns of O, which meet zero columns of out_proj.  Widths 64 and 80 run as they are; any other width is refused by name.

Padding rows (257..319 of every image) are never read by a valid row -- every op but the attention is row-local, and the attention masks keys >= nk
-- but they must stay FINITE: fmx_attention_f16 multiplies V^T columns [nk, nk_pad) by probabilities of exactly 0.  How that is guaranteed:
  * clip_embed_ln writes them as zeros;
  * a row-local op maps a finite row to a finite row (LayerNorm of a constant row is beta), so x, q|k, V^T and the MLP stay finite there as long
    as the attention output O does;
  * fmx_attention_f16 leaves O's rows >= nq as they were, so encode() takes ONE O buffer for all layers and zeroes it once before the first; nothing
    else ever writes it.
Every intermediate comes from `self.allocator(shape, dtype)` (default: torch.empty on the tower's device).  That is the hook tests use to fill
everything the tower computes in with NaN first: whatever a valid output depended on that the tower did not write itself would show."""
import torch

from ... import hipops as ops

P = "vision_model."
TOKENS, T_PAD, PATCHES, PATCH_COLS = 257, 320, 256, 640
HEAD_PAD = {64: 64, 80: 80, 104: 128}
OUTPUTS = ("last_hidden_state", "penultimate_hidden_states", "image_embeds")


def head_dpad(d):
    if d not in HEAD_PAD:
        raise NotImplementedError(f"CLIP-vision: head width {d} is not one of {sorted(HEAD_PAD)} (ViT-L/14, ViT-H/14, ViT-bigG/14)")
    return HEAD_PAD[d]


def pad_head_rows(w, heads, d, dp):
    """[heads * d, ...] -> [heads * dp, ...]: head h's rows at h * dp, zeros behind them"""
    if dp == d:
        return w
    out = w.new_zeros((heads, dp) + tuple(w.shape[1:]))
    out[:, :d] = w.reshape((heads, d) + tuple(w.shape[1:]))
    return out.reshape((heads * dp,) + tuple(w.shape[1:]))


def pad_head_cols(w, heads, d, dp):
    """[n, heads * d] -> [n, heads * dp]: the columns that meet pad_head_rows' rows"""
    return pad_head_rows(w.t(), heads, d, dp).t().contiguous() if dp != d else w


def layer_weights(sd, i, heads, d):
    """Layer i of a transformers-keyed state dict -> fp32 tensors in the executor's layout: qk (weight [2 * heads * dp, c], bias), v [heads * dp, c],
    out (weight [c, heads * dp], bias with W_o b_v folded in), ln1 / ln2 / fc1 / fc2 (weight, bias).  Pure torch, any device."""
    dp = head_dpad(d)
    k = f"{P}encoder.layers.{i}."
    f = lambda n: sd[k + n].float()   # noqa: E731
    rows = lambda n: pad_head_rows(f(n), heads, d, dp)   # noqa: E731
    # softmax rows sum to 1, so V's bias passes through attention unchanged: out_proj(o + b_v) = out_proj(o) + W_o b_v (backend/nn/clip.py)
    bo = f("self_attn.out_proj.bias") + f("self_attn.out_proj.weight") @ f("self_attn.v_proj.bias")
    return {"qk": (torch.cat([rows("self_attn.q_proj.weight"), rows("self_attn.k_proj.weight")], 0), torch.cat([rows("self_attn.q_proj.bias"), rows("self_attn.k_proj.bias")], 0)),
            "v": rows("self_attn.v_proj.weight"), "out": (pad_head_cols(f("self_attn.out_proj.weight"), heads, d, dp), bo),
            "ln1": (f("layer_norm1.weight"), f("layer_norm1.bias")), "ln2": (f("layer_norm2.weight"), f("layer_norm2.bias")),
            "fc1": (f("mlp.fc1.weight"), f("mlp.fc1.bias")), "fc2": (f("mlp.fc2.weight"), f("mlp.fc2.bias"))}


class CLIPVisionTower:
    def __init__(self, config, state_dict, device="cuda"):
        self.config = dict(config)
        self.device = torch.device(device)
        self.hidden, self.heads, self.layers = config["hidden_size"], config["num_attention_heads"], config["num_hidden_layers"]
        self.d = self.hidden // self.heads
        self.dp = head_dpad(self.d)
        if config.get("image_size", 224) != 224 or config.get("patch_size", 14) != 14:
            raise NotImplementedError(f"CLIP-vision: image {config.get('image_size')} / patch {config.get('patch_size')}; the towers are 224 / 14")
        if self.hidden % 64 or config["intermediate_size"] % 64:
            raise NotImplementedError("CLIP-vision: hidden / intermediate sizes must be multiples of 64")
        act = config.get("hidden_act", "quick_gelu")
        if act not in ("quick_gelu", "gelu"):
            raise NotImplementedError(f"CLIP-vision: hidden_act {act!r}")
        self.act = ops.ACT_QUICK_GELU if act == "quick_gelu" else ops.ACT_GELU_ERF
        self.eps = float(config.get("layer_norm_eps", 1e-5))
        self.projection_dim = int(state_dict["visual_projection.weight"].shape[0])
        self.allocator = lambda shape, dtype=torch.float16: torch.empty(shape, dtype=dtype, device=self.device)
        self._load(state_dict)

    def _load(self, sd):
        T = lambda t: t.to(device=self.device, dtype=torch.float16).contiguous()   # noqa: E731
        c = self.hidden
        patch = sd[P + "embeddings.patch_embedding.weight"].float().reshape(c, -1)
        if patch.shape[1] != 588 or tuple(sd[P + "embeddings.position_embedding.weight"].shape) != (TOKENS, c):
            raise NotImplementedError("CLIP-vision: the patch embedding is not [C, 3, 14, 14] or the position embedding not [257, C]")
        w = {"patch": T(torch.nn.functional.pad(patch, (0, PATCH_COLS - 588))), "class": T(sd[P + "embeddings.class_embedding"].reshape(c)),
             "pos": T(sd[P + "embeddings.position_embedding.weight"]), "pre": (T(sd[P + "pre_layrnorm.weight"]), T(sd[P + "pre_layrnorm.bias"])),
             "post": (T(sd[P + "post_layernorm.weight"]), T(sd[P + "post_layernorm.bias"])), "proj": T(sd["visual_projection.weight"])}
        for i in range(self.layers):
            for name, v in layer_weights(sd, i, self.heads, self.d).items():
                w[f"{i}.{name}"] = tuple(T(t) for t in v) if isinstance(v, tuple) else T(v)
        self.w = w
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    @torch.inference_mode()
    def encode(self, pixel_rows):
        """pixel_rows fp16 [b * 256, 640] (hipops.clip_patch_rows) -> {last_hidden_state [b, 257, c] (before post_layernorm), penultimate_hidden_states
        [b, 257, c] (hidden_states[-2]), image_embeds [b, projection_dim]}, fp16: what CLIPVisionModelWithProjection(output_hidden_states=True) returns."""
        c, H, dp, A = self.hidden, self.heads, self.dp, self.allocator
        b = pixel_rows.shape[0] // PATCHES
        if pixel_rows.shape != (b * PATCHES, PATCH_COLS) or b < 1:
            raise ValueError(f"CLIP-vision: pixel rows {tuple(pixel_rows.shape)}, expected [b * {PATCHES}, {PATCH_COLS}]")
        rows, hd = b * T_PAD, H * dp
        patches = ops.linear(pixel_rows, self.w["patch"], out=A((b * PATCHES, c)))
        x = ops.clip_embed_ln(patches, self.w["class"], self.w["pos"], *self.w["pre"], eps=self.eps, rows_per_image=T_PAD, out=A((rows, c)))
        o = A((rows, hd)).zero_()          # rows >= 257 of every image: written here and by nothing else (module docstring)
        hs = [x]
        for i in range(self.layers):
            h = ops.layernorm(x, *self.w[f"{i}.ln1"], eps=self.eps, out=A((rows, c)))
            qk = ops.linear(h, *self.w[f"{i}.qk"], out=A((rows, 2 * hd)))
            vt = ops.conv_gemm(self.w[f"{i}.v"], h, rows, out=A((hd, rows)), ld_out=rows)      # V^T = W_v X^T
            ops.attention(qk, qk[:, hd:], vt, batch=b, heads=H, nq=TOKENS, nk=TOKENS, nk_pad=T_PAD, dpad=dp, scale=self.d ** -0.5,
                          q_bs=T_PAD * 2 * hd, q_rs=2 * hd, k_bs=T_PAD * 2 * hd, k_rs=2 * hd, vt_bs=T_PAD, vt_hs=dp * rows, vt_ds=rows,
                          out=o, o_bs=T_PAD * hd)
            x = ops.linear(o, *self.w[f"{i}.out"], residual=x, out=A((rows, c)))
            h = ops.layernorm(x, *self.w[f"{i}.ln2"], eps=self.eps, out=A((rows, c)))
            f = ops.linear(h, *self.w[f"{i}.fc1"], out=A((rows, self.w[f"{i}.fc1"][0].shape[0])))
            h = ops.act(f, self.act, out=A(tuple(f.shape)))
            x = ops.linear(h, *self.w[f"{i}.fc2"], residual=x, out=A((rows, c)))
            hs.append(x)
        view = lambda t: t.view(b, T_PAD, c)   # noqa: E731
        cls = A((b, c))
        cls.copy_(view(hs[-1])[:, 0])
        pooled = ops.layernorm(cls, *self.w["post"], eps=self.eps, out=A((b, c)))
        embeds = ops.linear(pooled, self.w["proj"], out=A((b, self.projection_dim)))
        return {"last_hidden_state": view(hs[-1])[:, :TOKENS], "penultimate_hidden_states": view(hs[-2])[:, :TOKENS], "image_embeds": embeds}
