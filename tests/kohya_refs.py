"""Shared by the native Kohya HRFix tests: the separable resize in fp64, the kernel cases, the derived bound, and the reference's two patch
functions restated with torch.nn.functional.interpolate (the hooked A/B of tests/test_gpu_kohya.py)."""
import torch

# (n, C, H, W) -> (OH, OW), mode: the kernel cases of tests/test_gpu_kohya.py, which tests/test_kohya_host.py pins the tables on
KERNEL_CASES = [
    ((2, 64, 16, 12), (8, 6), "bicubic"),
    ((1, 128, 8, 6), (16, 12), "bicubic"),            # up
    ((1, 64, 16, 12), (11, 8), "bicubic"),            # non-integer ratio
    ((1, 64, 16, 12), (11, 8), "nearest-exact"),
    ((2, 32, 5, 7), (3, 4), "area"),                  # uneven windows
    ((1, 64, 3, 2), (16, 12), "bilinear"),            # input narrower than the tap count: border folding
    ((1, 320, 33, 31), (17, 16), "bicubic"),          # 40 lane groups per pixel (no power of two), several workgroups
]
MODES = ("bicubic", "bilinear", "nearest-exact", "area")


def case_input(i, shape):
    """seeded fp16-rounded NCHW input of case i, as fp32"""
    g = torch.Generator().manual_seed(5200 + i)
    return torch.randn(*shape, generator=g).half().float()


def tables(h, w, oh, ow, mode):
    from forge_amd.modules.latent_upscale import axis_table
    return axis_table(h, oh, mode, False) + axis_table(w, ow, mode, False)


def _taps(x_nhwc, tabs):
    """-> fp64 [n, oh, ow, c, ky*kx]: every tap's product yweights * xweights * x (the weight product formed in fp64 from the fp32 tables)"""
    ys, yw, xs, xw = tabs
    x = x_nhwc.double()
    (oh, ky), (ow, kx) = yw.shape, xw.shape
    iy = ys.long()[:, None] + torch.arange(ky)[None, :]                   # [oh, ky]
    ix = xs.long()[:, None] + torch.arange(kx)[None, :]                   # [ow, kx]
    assert int(iy.min()) >= 0 and int(iy.max()) < x.shape[1] and int(ix.min()) >= 0 and int(ix.max()) < x.shape[2]
    g = x[:, iy][:, :, :, ix]                                             # [n, oh, ky, ow, kx, c]
    wgt = yw.double()[:, :, None, None] * xw.double()[None, None, :, :]   # [oh, ky, ow, kx]
    t = g * wgt[None, ..., None]
    return t.permute(0, 1, 3, 5, 2, 4).reshape(x.shape[0], oh, ow, x.shape[3], ky * kx)


def resize_ref(x_nhwc16, tabs):
    """out[b, oy, ox, ch] = sum_i sum_j yweights[oy, i] xweights[ox, j] in[b, ystart[oy] + i, xstart[ox] + j, ch] in fp64 on the CPU.
    x_nhwc16: [n, h, w, c] (fp16, or fp32 for the table pin); tabs = (ystart, yweights, xstart, xweights).  -> fp64 [n, oh, ow, c]"""
    return _taps(x_nhwc16, tabs).sum(-1)


def ulp_f16(v):
    """spacing of fp16 at |v| (fp64 in, fp64 out); subnormal spacing 2^-24 below 2^-14"""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 10)


def kernel_bound(x_nhwc16, tabs, ref):
    """|got - ref| <= 1/2 ulp_fp16(ref) + (ky kx + 2) 2^-24 sum |w_y w_x x|: one fp16 rounding of the result plus fp32 accumulation over the
    taps (each tap's weight product rounded once, each multiply-add rounded at most twice -> first-order (ky kx + 2) u on the absolute sum)"""
    k = tabs[1].shape[1] * tabs[3].shape[1]
    return 0.5 * ulp_f16(ref) + (k + 2) * 2.0 ** -24 * _taps(x_nhwc16, tabs).abs().sum(-1)


def torch_resize(x_nchw, size, mode):
    """what the reference's adaptive_resize(samples, width, height, method, "disabled") computes for the four separable methods"""
    return torch.nn.functional.interpolate(x_nchw, size=(int(size[0]), int(size[1])), mode=mode)


def python_patches(block_number, downscale_factor, sigma_start, sigma_end, downscale_method, upscale_method, resized=None):
    """-> (input_block_patch, output_block_patch): the reference's PatchModelAddDownscale closures restated (kohya_hrfix.py:13-28) with
    F.interpolate in fp32; `resized`, a list, receives the ("input" | "output", block) of every resize"""
    def input_block_patch(h, transformer_options):
        if transformer_options["block"][1] == block_number:
            sigma = transformer_options["sigmas"][0].item()
            if sigma <= sigma_start and sigma >= sigma_end:
                h = torch_resize(h.float(), (round(h.shape[-2] * (1.0 / downscale_factor)), round(h.shape[-1] * (1.0 / downscale_factor))), downscale_method)
                if resized is not None:
                    resized.append(tuple(transformer_options["block"]))
        return h

    def output_block_patch(h, hsp, transformer_options):
        if h.shape[2] != hsp.shape[2]:
            h = torch_resize(h.float(), (hsp.shape[-2], hsp.shape[-1]), upscale_method)
            if resized is not None:
                resized.append(tuple(transformer_options["block"]))
        return h, hsp

    return input_block_patch, output_block_patch
