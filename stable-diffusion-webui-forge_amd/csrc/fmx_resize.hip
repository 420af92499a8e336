// Separable resize of a channels-last fp16 activation (include/fmx.h, section "NHWC resize"): what Kohya HRFix / Deep Shrink does to the UNet's
// hidden state.  One HBM-bound pass: every lane owns 8 consecutive channels of one output pixel, reads one 16-byte vector per tap and writes one.
// Lanes run along the channels first, so a wave's loads of one tap are contiguous runs.  fp32 accumulation, rows outer and columns inner, one
// fp16 rounding at the store.  No LDS: the two tables are a few hundred values and stay in cache.
#include "fmx_common.hpp"

namespace {

constexpr int TPB = 256;

__global__ __launch_bounds__(TPB) void resize_nhwc_kernel(const f16* __restrict__ in, f16* __restrict__ out, const int32_t* __restrict__ ystart,
                                                          const float* __restrict__ yweights, const int32_t* __restrict__ xstart,
                                                          const float* __restrict__ xweights, int h, int w, int c, int oh, int ow, int ky, int kx,
                                                          long total) {
  const long gid = (long)blockIdx.x * TPB + threadIdx.x;   // one 8-channel group of one output pixel
  if (gid >= total) return;
  const int cg = c / 8;
  const int g = (int)(gid % cg);
  const long pix = gid / cg;                               // (b * oh + oy) * ow + ox
  const int ox = (int)(pix % ow);
  const long t = pix / ow;
  const int oy = (int)(t % oh);
  const long b = t / oh;
  const int y0 = ystart[oy], x0 = xstart[ox];
  const float* wy = yweights + (long)oy * ky;
  const float* wx = xweights + (long)ox * kx;
  const f16* src = in + ((b * h + y0) * w + x0) * (long)c + g * 8;
  float acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.f;
  for (int i = 0; i < ky; ++i) {
    const float wi = wy[i];
    const f16* row = src + (long)i * w * c;
    for (int j = 0; j < kx; ++j) {
      const float wgt = wi * wx[j];
      const f16x8 v = *reinterpret_cast<const f16x8*>(row + (long)j * c);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] += wgt * (float)v[k];
    }
  }
  f16x8 o;
#pragma unroll
  for (int k = 0; k < 8; ++k) o[k] = (f16)acc[k];
  *reinterpret_cast<f16x8*>(out + pix * c + g * 8) = o;
}

}  // namespace

extern "C" int fmx_resize_nhwc_f16(const void* in, void* out, const int32_t* ystart, const float* yweights, const int32_t* xstart,
                                   const float* xweights, int32_t n, int32_t h, int32_t w, int32_t c, int32_t oh, int32_t ow, int32_t ky, int32_t kx,
                                   void* stream) {
  FMX_REQUIRE(n > 0 && h > 0 && w > 0 && c > 0 && oh > 0 && ow > 0, "resize_nhwc: every extent must be positive");
  FMX_REQUIRE((c % 8) == 0, "resize_nhwc: c must be a multiple of 8 (got %d)", c);
  FMX_REQUIRE(ky >= 1 && kx >= 1 && ky <= h && kx <= w, "resize_nhwc: 1 <= ky <= h and 1 <= kx <= w (got ky %d, kx %d for %d x %d)", ky, kx, h, w);
  FMX_REQUIRE((long)n * h * w * c < (1L << 31) && (long)n * oh * ow * c < (1L << 31), "resize_nhwc: n*h*w*c or n*oh*ow*c overflows 32 bits");
  FMX_REQUIRE(in && out && ystart && yweights && xstart && xweights && (reinterpret_cast<uintptr_t>(in) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(out) & 15) == 0,
              "resize_nhwc: null or misaligned pointer");
  const long total = (long)n * oh * ow * (c / 8);
  hipLaunchKernelGGL(resize_nhwc_kernel, dim3((unsigned)((total + TPB - 1) / TPB)), dim3(TPB), 0, (hipStream_t)stream, (const f16*)in, (f16*)out,
                     ystart, yweights, xstart, xweights, h, w, c, oh, ow, ky, kx, total);
  FMX_LAUNCH_CHECK("fmx_resize_nhwc_f16");
  return FMX_OK;
}
