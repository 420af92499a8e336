// 3x3 convolution, 64 -> 64 channels, with the epilogues of the TAESD decoder (modules/sd_vae_taesd.py:16-44): `conv + ReLU`, the Block's
// `fuse(conv(x) + skip(x))` (residual, then ReLU) and `nn.Upsample(scale_factor=2)` + conv(bias=False).  33 of the decoder's 34 layers are this shape, four
// of them at the full image size, where the implicit GEMM would gather every input pixel nine times (fmx_conv_patch.hip is the same finding at 128 channels).
//   * a workgroup (4 waves, ONE per CU: it owns the CU's LDS) is persistent: it loads all nine taps of the weight -- 64 x 9 x 64 x 2 = 73 728 bytes -- into
//     LDS once and then walks output tiles of 8 rows x 32 pixels (tile index blockIdx.x, + gridDim.x, ...), all 64 output channels each;
//   * the 10 x 34-pixel input patch of a tile (128-byte pixels in the swizzled format of fmx_conv_direct.hpp, zeros outside the image) is
//     double-buffered: the global loads of the NEXT tile's patch are issued before the MFMA loop of this one and written to the other LDS buffer after its
//     epilogue, so one barrier per tile; 73 728 + 2 x 43 520 = 160 768 bytes of the CU's 163 840;
//   * with up2x the patch is staged from the half-resolution source, pixel (Y >> 1, X >> 1) for upsampled (Y, X): the upsampled tensor never exists, the layer
//     keeps its own weights (no tap-sum fold: no rounding site the reference network does not have);
//   * the nine taps read their shifted pixels from the patch (MFMA-B operand of v_mfma_f32_16x16x32: 16 neighbouring pixels of a row), the weights are the A
//     operand; a wave owns 2 rows = 64 pixels x 64 channels (4 x 4 accumulator blocks, 8 fragment reads per 16 MFMAs, no barrier inside a tile);
//   * epilogue in the accumulator layout (a lane holds 4 consecutive output channels of a pixel): + bias (+ residual), ReLU, ONE rounding, 8-byte stores.
// Tile, accumulator layout, LDS format, tap step and patch items: fmx_conv_direct.hpp.
#include "fmx_conv_direct.hpp"

namespace {

constexpr int CH = 64;                         // channels in and out: 128-byte pixels in LDS
constexpr int PATCH_BYTES = PH * PW * CH * 2;  // 43 520
constexpr int TAP_BYTES = CH * CH * 2;         // 8 192: one tap, [out channel][in channel]
constexpr int W_BYTES = 9 * TAP_BYTES;         // 73 728
constexpr int SMEM = W_BYTES + 2 * PATCH_BYTES;
constexpr int ITEMS = PH * PW * (CH / 8);      // 16-byte items of a patch
constexpr int ITERS = (ITEMS + 255) / 256;
constexpr int W_ITEMS = CH * 9 * (CH / 8);     // 16-byte items of the weight
static_assert(SMEM <= 160 * 1024, "weights + two patches must fit the CU's LDS");
static_assert(W_ITEMS % 256 == 0, "weight staging loop has no tail");

struct C64Params {
  const f16* x;          // [n][h][w][64]
  const f16* wgt;        // [64][9][64]
  const f16* bias;       // [64] or null
  const f16* res;        // [n*oh*ow][ld_res] or null
  long ld_res;
  f16* out;              // [n*oh*ow][ld_out]
  long ld_out;
  int h, w, oh, ow, up, relu, tiles_x, tiles_y, ntiles;
};

__global__ __launch_bounds__(256, 1) void conv3x3_c64_kernel(const C64Params p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l16 = lane & 15, kg = lane >> 4;
  const int h = p.h, w = p.w, oh = p.oh, ow = p.ow, up = p.up;
  const int tiles_per_img = p.tiles_x * p.tiles_y;

  // ---- weights, once: row o of tap t at t * 8192 + o * 128, swizzled ----------------------------------------------------------------------------------
#pragma unroll
  for (int it = 0; it < W_ITEMS / 256; ++it) {
    const int i = tid + it * 256;
    const int o = i / 72, rem = i - o * 72, t = rem >> 3, c = rem & 7;
    *reinterpret_cast<f16x8*>(smem + t * TAP_BYTES + swz_off(o, o, c)) = *reinterpret_cast<const f16x8*>(p.wgt + (long)i * 8);
  }

  // ---- input patch of a tile: global -> registers (load_patch), registers -> LDS (store_patch) ------------------------------------------------------
  const int cc = tid & 7;                                          // this thread's 16-byte channel octet, in every item
  f16x8 v[ITERS];
  auto load_patch = [&](int tile) __attribute__((always_inline)) {
    const TilePos t = tile_decode(tile, p.tiles_x, tiles_per_img);
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const PatchItem i = patch_item<8>(tid, it, t.ty * TH, t.tx * TW);
      v[it] = zero_octet();                                        // the convolution's zero padding
      if (i.pi < PH * PW && in_image(i, oh, ow)) v[it] = *reinterpret_cast<const f16x8*>(p.x + patch_src_pixel(i, t.img, h, w, up) * CH + cc * 8);
    }
  };
  auto store_patch = [&](char* patch) __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const PatchItem i = patch_item<8>(tid, it, 0, 0);             // its place in the patch only
      if (i.pi < PH * PW) *reinterpret_cast<f16x8*>(patch + swz_off(i.pi, i.q, cc)) = v[it];
    }
  };

  f32x4 bsum[4];
  load_bias(bsum, p.bias, kg);
  const int w_lane = w_frag_off(l16, kg);

  int tile = blockIdx.x;
  if (tile >= p.ntiles) return;
  load_patch(tile);
  store_patch(smem + W_BYTES);
  __syncthreads();

  for (int buf = 0; tile < p.ntiles; tile += gridDim.x, buf ^= 1) {
    const int next = tile + gridDim.x;
    if (next < p.ntiles) load_patch(next);                         // in flight under the MFMA loop
    const char* const patch = smem + W_BYTES + buf * PATCH_BYTES;

    f32x4 acc[4][4];
#pragma unroll
    for (int pb = 0; pb < 4; ++pb)
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) acc[pb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
        tap_mfma(acc, smem, (ky * 3 + kx) * TAP_BYTES + w_lane, patch, p_frag_off(wave, l16, kg, ky, kx));

    // ---- epilogue in the accumulator layout ----
    {
      const TilePos t = tile_decode(tile, p.tiles_x, tiles_per_img);
#pragma unroll
      for (int pb = 0; pb < 4; ++pb) {
        const auto [ok, m] = out_pixel(t, wave, pb, l16, oh, ow);
        f16x4 rv[4];
        if (p.res && ok) {
#pragma unroll
          for (int cb = 0; cb < 4; ++cb) rv[cb] = *reinterpret_cast<const f16x4*>(p.res + m * p.ld_res + acc_chan(cb, kg));
        }
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
          f16x4 o;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float f = acc[pb][cb][r] + bsum[cb][r];
            if (p.res && ok) f += (float)rv[cb][r];
            if (p.relu) f = fmaxf(f, 0.0f);
            o[r] = (f16)f;
          }
          if (ok) *reinterpret_cast<f16x4*>(p.out + m * p.ld_out + acc_chan(cb, kg)) = o;
        }
      }
    }

    // the other buffer was last read in the previous tile's MFMA loop, and every wave has passed the barrier that closed it
    if (next < p.ntiles) store_patch(smem + W_BYTES + (buf ^ 1) * PATCH_BYTES);
    __syncthreads();
  }
}

}  // namespace

extern "C" int fmx_conv3x3_c64_f16(const void* x, int32_t n, int32_t h, int32_t w, int32_t cin, const void* wgt, const void* bias, int32_t cout,
                                   const void* residual, int64_t ld_res, int32_t relu, int32_t up2x, void* out, int64_t ld_out, void* stream) {
  FMX_REQUIRE(x && wgt && out, "conv3x3_c64: null pointer");
  FMX_REQUIRE(cin == CH && cout == CH, "conv3x3_c64: 64 input and 64 output channels (got %d -> %d)", cin, cout);
  FMX_REQUIRE(n > 0 && h > 0 && w > 0, "conv3x3_c64: bad geometry");
  FMX_REQUIRE((relu == 0 || relu == 1) && (up2x == 0 || up2x == 1), "conv3x3_c64: relu and up2x are 0 or 1");
  FMX_REQUIRE(ld_out >= CH && (ld_out % 4) == 0 && (!residual || (ld_res >= CH && (ld_res % 4) == 0)), "conv3x3_c64: bad leading dimensions");
  FMX_REQUIRE(fmx_aligned16(x) && fmx_aligned16(wgt) && aligned8(out) && aligned8(residual) && aligned8(bias), "conv3x3_c64: operand alignment");
  const int oh = h << up2x, ow = w << up2x;
  const TileGrid g = tile_grid(n, oh, ow);
  FMX_REQUIRE(g.one_launch(), "conv3x3_c64: too many tiles for one launch (split the batch)");
  const unsigned grid = persistent_grid(g.ntiles);   // one persistent workgroup per CU
  if (!grid) return fmx_set_error(FMX_E_UNSUPPORTED, "conv3x3_c64: cannot read the device's CU count");
  lds_ceiling_once<&conv3x3_c64_kernel, SMEM>();
  C64Params p;
  p.x = (const f16*)x;
  p.wgt = (const f16*)wgt;
  p.bias = (const f16*)bias;
  p.res = (const f16*)residual;
  p.ld_res = ld_res;
  p.out = (f16*)out;
  p.ld_out = ld_out;
  p.h = h; p.w = w; p.oh = oh; p.ow = ow; p.up = up2x; p.relu = relu; p.tiles_x = g.tiles_x; p.tiles_y = g.tiles_y; p.ntiles = (int)g.ntiles;
  hipLaunchKernelGGL(conv3x3_c64_kernel, dim3(grid), dim3(256), SMEM, (hipStream_t)stream, p);
  FMX_LAUNCH_CHECK("fmx_conv3x3_c64_f16");
  return FMX_OK;
}
