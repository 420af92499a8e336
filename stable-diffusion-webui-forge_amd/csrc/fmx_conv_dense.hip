// 3x3 convolution of the ESRGAN residual dense block (RRDBNet: nf 64, gc 32): cin in {64, 96, 128, 160, 192} -> cout in {32, 64}, with LeakyReLU and up
// to two scaled residuals in the epilogue, reading the first cin channels of pixels with pitch ld_x and writing a column window of pitch ld_out.
//
// In-place window form -- the point of the kernel: a dense block's `torch.cat((x, x1, ...), 1)` never exists.  The block lives in ONE 192-channel buffer
// [x | x1 | x2 | x3 | x4]; conv_k reads columns [0, cin) and writes columns [cin, cin + 32) of the SAME buffer (out = x + cin, ld_out = ld_x).  That is safe
// in any tile order because the written columns are disjoint from the read ones; the residuals may be read-only windows of the same buffer (x's own first
// 64 columns).  conv5 writes the NEXT block's first 64 columns, which other tiles' halos still read: it must go to the OTHER of two such buffers, which
// then ping-pong.  The entry point refuses an `out` that lies inside x's rows and overlaps [0, cin).
//
//   * tile and accumulator layout are those of fmx_conv_direct.hpp, the walk is fmx_conv_c64.hip's: a persistent workgroup (4 waves, ONE per CU) walks 8 x 32-pixel output tiles, a wave owns 2 rows = 64 pixels x all
//     cout channels (4 x cout/16 accumulator blocks of v_mfma_f32_16x16x32, weights the A operand, 16 neighbouring pixels of a patch row the B operand);
//   * the full weight (up to 9 x 192 x 64 x 2 = 221 184 bytes) and a 192-channel 10 x 34 patch (130 560) do not fit the CU's LDS, so the K loop walks the
//     input channels in chunks of 32: a STAGE is (the 10 x 34 x 32-channel patch chunk, the 9 x cout x 32 weight chunk), 22 528 + 36 864 bytes, double
//     buffered.  Stages run over (tile, chunk) as one flat sequence: the global loads of the next stage -- the next chunk, or chunk 0 of the next tile --
//     are issued before the MFMA loop of this one and written to the other buffer after it, one barrier per stage;
//   * LDS images are planes of 16-byte slots, [channel octet kg][pixel] and [tap][kg][out channel]: the 16 lanes of an MFMA fragment that share kg read 16
//     consecutive slots, and the plane pitches (352 and cout slots) are multiples of 16 slots = one bank row, so the 16-lane groups of ds_read_b128
//     (which mix two kg) never meet on a bank;
//   * the accumulators stay in fp32 across all chunks; epilogue in the accumulator layout (a lane holds 4 consecutive output channels of a pixel):
//     + bias, LeakyReLU, alpha * f + res1, beta * f + res2, ONE rounding, 8-byte stores, row / column tails masked.
// The same file carries the two pixel kernels of the upscaler's ends (fmx_esrgan_pack_image, fmx_esrgan_unpack_image).
#include "fmx_conv_direct.hpp"

namespace {

constexpr int CK = 32;                          // input channels per stage: one k-step of the MFMA, 4 octets
constexpr int PLANE = 352;                      // slots per octet plane of the patch: PH * PW = 340 rounded up to a multiple of 16
constexpr int PATCH_BYTES = 4 * PLANE * 16;     // 22 528
constexpr int W_BYTES_MAX = 9 * 4 * 64 * 16;    // 36 864: [tap][octet][out channel] slots at cout 64
constexpr int STAGE_BYTES = PATCH_BYTES + W_BYTES_MAX;
constexpr int SMEM = 2 * STAGE_BYTES;           // 118 784
constexpr int P_ITEMS = PH * PW * 4;            // 16-byte items of a patch chunk
constexpr int P_ITERS = (P_ITEMS + 255) / 256;
static_assert(PLANE >= PH * PW && PLANE % 16 == 0, "patch planes hold the patch and start on a bank row");
static_assert(SMEM <= 160 * 1024, "two stages must fit the CU's LDS");

struct DenseParams {
  const f16* x;          // [n][h][w][ld_x], channels [0, cin) read
  const f16* wgt;        // [cout][9][cin]
  const f16* bias;       // [cout] or null
  const f16* res1;       // [n*oh*ow][ld_res1] or null
  const f16* res2;       // [n*oh*ow][ld_res2] or null
  f16* out;              // [n*oh*ow][ld_out]
  long ld_x, ld_res1, ld_res2, ld_out;
  float slope, alpha, beta;
  int h, w, oh, ow, up, cin, nchunks, tiles_x, tiles_y, ntiles;
};

template <int NCB>       // cout / 16
__global__ __launch_bounds__(256, 1) void conv3x3_dense_kernel(const DenseParams p) {
  constexpr int COUT = NCB * 16;
  constexpr int W_ITEMS = 9 * COUT * 4;
  constexpr int W_ITERS = (W_ITEMS + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l16 = lane & 15, kg = lane >> 4;
  const int h = p.h, w = p.w, oh = p.oh, ow = p.ow, up = p.up;
  const int tiles_per_img = p.tiles_x * p.tiles_y;

  // ---- one stage: global -> registers (load_stage), registers -> LDS (store_stage) ------------------------------------------------------------------
  const int cc = tid & 3;                                          // this thread's channel octet of the chunk, in every patch item
  f16x8 pv[P_ITERS], wv[W_ITERS];
  auto load_stage = [&](int tile, int chunk) __attribute__((always_inline)) {
    const TilePos t = tile_decode(tile, p.tiles_x, tiles_per_img);
    const int y0 = t.ty * TH - 1, x0 = t.tx * TW - 1;
    const int c0 = chunk * CK;
#pragma unroll
    for (int it = 0; it < P_ITERS; ++it) {
      const int pi = (tid >> 2) + it * 64;                         // patch pixel
      const int pr = pi / PW, q = pi - pr * PW;
      const int gy = y0 + pr, gx = x0 + q;                         // in the (upsampled) image the convolution runs on
      const bool ok = pi < PH * PW && gy >= 0 && gy < oh && gx >= 0 && gx < ow;
      pv[it] = zero_octet();                                       // the convolution's zero padding
      if (ok) pv[it] = *reinterpret_cast<const f16x8*>(p.x + (((long)t.img * h + (gy >> up)) * w + (gx >> up)) * p.ld_x + c0 + cc * 8);
    }
#pragma unroll
    for (int it = 0; it < W_ITERS; ++it) {
      const int i = tid + it * 256;
      const int o = i / 36, rem = i - o * 36;                      // rem = tap * 4 + octet
      if (i < W_ITEMS) wv[it] = *reinterpret_cast<const f16x8*>(p.wgt + ((long)o * 9 + (rem >> 2)) * p.cin + c0 + (rem & 3) * 8);
    }
  };
  auto store_stage = [&](char* stage) __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < P_ITERS; ++it) {
      const int pi = (tid >> 2) + it * 64;
      if (pi < PH * PW) *reinterpret_cast<f16x8*>(stage + (cc * PLANE + pi) * 16) = pv[it];
    }
#pragma unroll
    for (int it = 0; it < W_ITERS; ++it) {
      const int i = tid + it * 256;
      const int o = i / 36, rem = i - o * 36;
      if (i < W_ITEMS) *reinterpret_cast<f16x8*>(stage + PATCH_BYTES + (rem * COUT + o) * 16) = wv[it];
    }
  };

  f32x4 bsum[NCB];
  load_bias(bsum, p.bias, kg);

  int tile = blockIdx.x, chunk = 0;
  if (tile >= p.ntiles) return;
  load_stage(tile, 0);
  store_stage(smem);
  __syncthreads();

  f32x4 acc[4][NCB];
#pragma unroll
  for (int pb = 0; pb < 4; ++pb)
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) acc[pb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int buf = 0;; buf ^= 1) {
    int ntile = tile, nchunk = chunk + 1;
    if (nchunk == p.nchunks) {
      nchunk = 0;
      ntile = tile + gridDim.x;
    }
    const bool has_next = ntile < p.ntiles;
    if (has_next) load_stage(ntile, nchunk);                       // in flight under the MFMA loop
    const char* const patch = smem + buf * STAGE_BYTES;
    const char* const wts = patch + PATCH_BYTES;

#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        f16x8 wf[NCB], af[4];
        // weights: slot ((tap * 4 + kg) * COUT + cb * 16 + l16); activations: slot kg * PLANE + row * PW + column, of patch row
        // 2 * wave + (pb >> 1) + ky and column (pb & 1) * 16 + l16 + kx
        const char* wks = wts + (((ky * 3 + kx) * 4 + kg) * COUT + l16) * 16;
        const char* pks = patch + (kg * PLANE + (acc_row(wave, 0) + ky) * PW + l16 + kx) * 16;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) wf[cb] = *reinterpret_cast<const f16x8*>(wks + cb * 256);
#pragma unroll
        for (int pb = 0; pb < 4; ++pb) af[pb] = *reinterpret_cast<const f16x8*>(pks + pb_patch_pixels(pb) * 16);
#pragma unroll
        for (int pb = 0; pb < 4; ++pb)
#pragma unroll
          for (int cb = 0; cb < NCB; ++cb) acc[pb][cb] = FMX_MFMA_16x16x32(wf[cb], af[pb], acc[pb][cb]);
      }

    // ---- epilogue after the last chunk, in the accumulator layout ----
    if (chunk == p.nchunks - 1) {
      const TilePos t = tile_decode(tile, p.tiles_x, tiles_per_img);
#pragma unroll
      for (int pb = 0; pb < 4; ++pb) {
        const auto [ok, m] = out_pixel(t, wave, pb, l16, oh, ow);
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
          const int col = acc_chan(cb, kg);
          f16x4 r1 = {(f16)0.0f, (f16)0.0f, (f16)0.0f, (f16)0.0f}, r2 = r1;
          if (p.res1 && ok) r1 = *reinterpret_cast<const f16x4*>(p.res1 + m * p.ld_res1 + col);
          if (p.res2 && ok) r2 = *reinterpret_cast<const f16x4*>(p.res2 + m * p.ld_res2 + col);
          f16x4 o;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float f = acc[pb][cb][r] + bsum[cb][r];
            f = f >= 0.0f ? f : p.slope * f;
            if (p.res1) f = p.alpha * f + (float)r1[r];
            if (p.res2) f = p.beta * f + (float)r2[r];
            o[r] = (f16)f;
            acc[pb][cb][r] = 0.0f;
          }
          if (ok) *reinterpret_cast<f16x4*>(p.out + m * p.ld_out + col) = o;
        }
      }
    }

    // the other buffer was last read in the previous stage's MFMA loop, and every wave has passed the barrier that closed it
    if (has_next) store_stage(smem + (buf ^ 1) * STAGE_BYTES);
    __syncthreads();
    if (!has_next) break;
    tile = ntile;
    chunk = nchunk;
  }
}

// uint8 RGB [npix][3] -> fp16 [npix][64]: channels 0..2 = lut[B], lut[G], lut[R], the rest zeros; a thread writes one 16-byte octet of a pixel
__global__ void esrgan_pack_kernel(const uint8_t* __restrict__ img, const f16* __restrict__ lut, long npix, f16* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npix * 8) return;
  const long pix = i >> 3;
  f16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (f16)0.0f;
  if ((i & 7) == 0) {
    const uint8_t* s = img + pix * 3;
    v[0] = lut[s[2]];
    v[1] = lut[s[1]];
    v[2] = lut[s[0]];
  }
  *reinterpret_cast<f16x8*>(out + i * 8) = v;
}

// fp16 [npix][ld], channels 0..2 = B, G, R -> uint8 RGB [npix][3] = rint(255 * clamp(v, 0, 1)), ties to even
__global__ void esrgan_unpack_kernel(const f16* __restrict__ y, long ld, long npix, uint8_t* __restrict__ out) {
  const long pix = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= npix) return;
  const f16* s = y + pix * ld;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = fminf(fmaxf((float)s[2 - c], 0.0f), 1.0f);
    out[pix * 3 + c] = (uint8_t)__builtin_rintf(255.0f * v);
  }
}

}  // namespace

extern "C" int fmx_conv3x3_dense_f16(const void* x, int64_t ld_x, int32_t n, int32_t h, int32_t w, int32_t cin, const void* wgt, const void* bias, int32_t cout,
                                     float slope, const void* res1, int64_t ld_res1, float alpha, const void* res2, int64_t ld_res2, float beta, int32_t up2x,
                                     void* out, int64_t ld_out, void* stream) {
  FMX_REQUIRE(x && wgt && out, "conv3x3_dense: null pointer");
  FMX_REQUIRE(cin == 64 || cin == 96 || cin == 128 || cin == 160 || cin == 192, "conv3x3_dense: cin must be 64, 96, 128, 160 or 192 (got %d)", cin);
  FMX_REQUIRE(cout == 32 || cout == 64, "conv3x3_dense: cout must be 32 or 64 (got %d)", cout);
  FMX_REQUIRE(n > 0 && h > 0 && w > 0, "conv3x3_dense: bad geometry");
  FMX_REQUIRE(up2x == 0 || (up2x == 1 && cin == 64 && cout == 64), "conv3x3_dense: up2x is 0 or 1, and 1 only for 64 -> 64 channels");
  FMX_REQUIRE(res1 || !res2, "conv3x3_dense: res2 requires res1");
  FMX_REQUIRE(ld_x >= cin && (ld_x % 8) == 0, "conv3x3_dense: ld_x must be >= cin and a multiple of 8");
  FMX_REQUIRE(ld_out >= cout && (ld_out % 4) == 0 && (!res1 || (ld_res1 >= cout && (ld_res1 % 4) == 0)) && (!res2 || (ld_res2 >= cout && (ld_res2 % 4) == 0)),
              "conv3x3_dense: bad leading dimensions");
  FMX_REQUIRE(fmx_aligned16(x) && fmx_aligned16(wgt) && aligned8(out) && aligned8(res1) && aligned8(res2) && aligned8(bias), "conv3x3_dense: operand alignment");
  const int oh = h << up2x, ow = w << up2x;
  {  // the in-place window form: an `out` inside x's rows must not touch the columns the kernel reads
    const int64_t npx = (int64_t)n * h * w;
    const int64_t d = (static_cast<const char*>(out) - static_cast<const char*>(x)) / 2;      // in elements
    if (out >= x && d < npx * ld_x) {
      const int64_t col = d % ld_x;
      FMX_REQUIRE(ld_out == ld_x && up2x == 0 && col >= cin && col + cout <= ld_x,
                  "conv3x3_dense: out lies inside x: it must be a column window of the same pitch, disjoint from the input columns [0, %d)", cin);
    }
  }
  const TileGrid g = tile_grid(n, oh, ow);
  FMX_REQUIRE(g.one_launch(), "conv3x3_dense: too many tiles for one launch (split the batch)");
  const unsigned grid = persistent_grid(g.ntiles);   // one persistent workgroup per CU
  if (!grid) return fmx_set_error(FMX_E_UNSUPPORTED, "conv3x3_dense: cannot read the device's CU count");
  DenseParams p;
  p.x = (const f16*)x;
  p.wgt = (const f16*)wgt;
  p.bias = (const f16*)bias;
  p.res1 = (const f16*)res1;
  p.res2 = (const f16*)res2;
  p.out = (f16*)out;
  p.ld_x = ld_x; p.ld_res1 = ld_res1; p.ld_res2 = ld_res2; p.ld_out = ld_out;
  p.slope = slope; p.alpha = alpha; p.beta = beta;
  p.h = h; p.w = w; p.oh = oh; p.ow = ow; p.up = up2x; p.cin = cin; p.nchunks = cin / CK;
  p.tiles_x = g.tiles_x; p.tiles_y = g.tiles_y; p.ntiles = (int)g.ntiles;
  if (cout == 32) {
    lds_ceiling_once<&conv3x3_dense_kernel<2>, SMEM>();
    hipLaunchKernelGGL(conv3x3_dense_kernel<2>, dim3(grid), dim3(256), SMEM, (hipStream_t)stream, p);
  } else {
    lds_ceiling_once<&conv3x3_dense_kernel<4>, SMEM>();
    hipLaunchKernelGGL(conv3x3_dense_kernel<4>, dim3(grid), dim3(256), SMEM, (hipStream_t)stream, p);
  }
  FMX_LAUNCH_CHECK("fmx_conv3x3_dense_f16");
  return FMX_OK;
}

extern "C" int fmx_esrgan_pack_image(const void* img, const void* lut, int64_t npix, void* out, void* stream) {
  FMX_REQUIRE(img && lut && out && npix > 0, "esrgan_pack_image: null pointer or no pixels");
  FMX_REQUIRE(fmx_aligned16(out) && (reinterpret_cast<uintptr_t>(lut) & 1u) == 0, "esrgan_pack_image: operand alignment");
  FMX_REQUIRE(npix < (1L << 36), "esrgan_pack_image: too many pixels for one launch");
  const long items = npix * 8;
  hipLaunchKernelGGL(esrgan_pack_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)img, (const f16*)lut, (long)npix,
                     (f16*)out);
  FMX_LAUNCH_CHECK("fmx_esrgan_pack_image");
  return FMX_OK;
}

extern "C" int fmx_esrgan_unpack_image(const void* y, int64_t ld, int64_t npix, void* out, void* stream) {
  FMX_REQUIRE(y && out && npix > 0 && ld >= 3, "esrgan_unpack_image: null pointer, no pixels or ld < 3");
  FMX_REQUIRE((reinterpret_cast<uintptr_t>(y) & 1u) == 0, "esrgan_unpack_image: operand alignment");
  FMX_REQUIRE(npix < (1L << 39), "esrgan_unpack_image: too many pixels for one launch");
  hipLaunchKernelGGL(esrgan_unpack_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const f16*)y, (long)ld, (long)npix, (uint8_t*)out);
  FMX_LAUNCH_CHECK("fmx_esrgan_unpack_image");
  return FMX_OK;
}
