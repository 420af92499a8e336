// Front end of the CLIP-vision towers (include/fmx_clipvision.h): the quantise / normalise / im2col pass that turns the resized image into the
// patch GEMM's input, and the token assembly + pre_layrnorm pass behind that GEMM.  Both are memory-bound and small (2 images: 0.7 MB in, 0.65 MB
// out; 514 rows of c), so they are plain HIP C++ with 16-byte stores; everything between them is the existing GEMM / attention / LayerNorm kernels.
#include "fmx_common.hpp"
#include "fmx_clipvision.h"

namespace {

constexpr int IMG = FMXV_CLIP_IMAGE, PATCH = FMXV_CLIP_PATCH, GRID = IMG / PATCH, PIX = PATCH * PATCH, COLS = FMXV_CLIP_PATCH_COLS;
constexpr int TOKENS = FMXV_CLIP_TOKENS, PATCHES = GRID * GRID;
constexpr int ROW_OCT = COLS / 8;   // 80 octets per output row
static_assert(GRID == 16 && 3 * PIX == 588 && COLS % 64 == 0 && COLS >= 3 * PIX && TOKENS == PATCHES + 1, "patch geometry");

// One workgroup per (image, patch row py): 16 output rows x 80 octets, 5 octets per thread.  A thread's 8 columns cross (ix, iy, ch) boundaries,
// so the pixel address is worked out per element; the 14-row band of the three planes it reads (3 x 14 x rw floats) stays in L2 / TCP.
__global__ __launch_bounds__(256) void clip_patch_rows_kernel(const float* __restrict__ in, f16* __restrict__ out, int rh, int rw, int top, int left) {
#pragma clang fp contract(off)
  const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f};
  const float stdv[3] = {0.26862954f, 0.26130258f, 0.27577711f};
  const int py = blockIdx.x % GRID;
  const long img = blockIdx.x / GRID;
  const long plane = (long)rh * rw;
  const float* src = in + img * 3 * plane + (long)(top + py * PATCH) * rw + left;
  f16* dst = out + (img * PATCHES + (long)py * GRID) * COLS;
  for (int q = threadIdx.x; q < GRID * ROW_OCT; q += 256) {
    const int px = q / ROW_OCT, col0 = (q % ROW_OCT) * 8;
    f16x8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int col = col0 + e;
      float y = 0.f;
      if (col < 3 * PIX) {
        const int ch = col / PIX, iy = (col % PIX) / PATCH, ix = col % PATCH;
        float t = 255.0f * src[ch * plane + (long)iy * rw + px * PATCH + ix];
        t = t < 0.0f ? 0.0f : (t > 255.0f ? 255.0f : t);          // torch.clip: a NaN fails both comparisons and stays
        const float v = __fdiv_rn(rintf(t), 255.0f);              // torch.round: ties to even
        y = __fdiv_rn(v - mean[ch], stdv[ch]);
      }
      r[e] = (f16)y;
    }
    *reinterpret_cast<f16x8*>(dst + (long)px * COLS + col0) = r;
  }
}

// One wave per output row, the row (class or patch + position) in registers as fp32; MAXOCT octets per lane.
template <int MAXOCT>
__global__ __launch_bounds__(256) void clip_embed_ln_kernel(const f16* __restrict__ patches, const f16* __restrict__ cls, const f16* __restrict__ pos,
                                                             const f16* __restrict__ gamma, const f16* __restrict__ beta, f16* __restrict__ out,
                                                             long rows, int c, int t_pad, float eps) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const long img = row / t_pad;
  const int tok = (int)(row % t_pad);
  const int oct = c >> 3;
  f16* yr = out + row * c;
  if (tok >= TOKENS) {   // padding rows: finite zeros, so the GEMMs and the attention's V^T columns behind them stay finite
    f16x8 z;
#pragma unroll
    for (int e = 0; e < 8; ++e) z[e] = (f16)0.f;
    for (int o = lane; o < oct; o += 64) *reinterpret_cast<f16x8*>(yr + o * 8) = z;
    return;
  }
  const f16* xr = tok == 0 ? cls : patches + (img * PATCHES + (tok - 1)) * c;
  const f16* pr = pos + (long)tok * c;
  float v[MAXOCT][8];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < MAXOCT; ++j) {
    const int o = lane + j * 64;
    if (o < oct) {
      const f16x8 a = *reinterpret_cast<const f16x8*>(xr + o * 8);
      const f16x8 p = *reinterpret_cast<const f16x8*>(pr + o * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        v[j][e] = (float)a[e] + (float)p[e];
        s += v[j][e];
      }
    }
  }
  const float mean = wave_sum(s) / (float)c;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < MAXOCT; ++j) {
    const int o = lane + j * 64;
    if (o < oct) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = v[j][e] - mean;
        q = fmaf(d, d, q);
      }
    }
  }
  const float rstd = rsqrtf(wave_sum(q) / (float)c + eps);
#pragma unroll
  for (int j = 0; j < MAXOCT; ++j) {
    const int o = lane + j * 64;
    if (o < oct) {
      const f16x8 g = *reinterpret_cast<const f16x8*>(gamma + o * 8);
      const f16x8 b = *reinterpret_cast<const f16x8*>(beta + o * 8);
      f16x8 r;
#pragma unroll
      for (int e = 0; e < 8; ++e) r[e] = (f16)fmaf((v[j][e] - mean) * rstd, (float)g[e], (float)b[e]);
      *reinterpret_cast<f16x8*>(yr + o * 8) = r;
    }
  }
}

}  // namespace

extern "C" int fmxv_clip_patch_rows_f16(const void* in, void* out, int32_t b, int32_t rh, int32_t rw, int32_t top, int32_t left, void* stream) {
  FMX_REQUIRE(in && out, "clip_patch_rows: null pointer");
  FMX_REQUIRE((reinterpret_cast<uintptr_t>(in) & 3u) == 0 && fmx_aligned16(out), "clip_patch_rows: `in` must be 4-byte and `out` 16-byte aligned");
  FMX_REQUIRE(b >= 1, "clip_patch_rows: b %d < 1", b);
  FMX_REQUIRE(rh >= IMG && rw >= IMG, "clip_patch_rows: plane %d x %d smaller than %d x %d", rh, rw, IMG, IMG);
  FMX_REQUIRE(top >= 0 && left >= 0 && (long)top + IMG <= rh && (long)left + IMG <= rw,
              "clip_patch_rows: window [%d, %d) x [%d, %d) leaves the %d x %d plane", top, top + IMG, left, left + IMG, rh, rw);
  FMX_REQUIRE((long)b * GRID < (1L << 27), "clip_patch_rows: b %d gives more than 2^31 rows", b);
  hipLaunchKernelGGL(clip_patch_rows_kernel, dim3((unsigned)(b * GRID)), dim3(256), 0, (hipStream_t)stream, (const float*)in, (f16*)out, rh, rw, top, left);
  FMX_LAUNCH_CHECK("fmxv_clip_patch_rows_f16");
  return FMX_OK;
}

extern "C" int fmxv_clip_embed_ln_f16(const void* patches, const void* class_embedding, const void* position_embedding, const void* gamma,
                                      const void* beta, void* out, int32_t b, int32_t c, int32_t rows_per_image, float eps, void* stream) {
  FMX_REQUIRE(patches && class_embedding && position_embedding && gamma && beta && out, "clip_embed_ln: null pointer");
  FMX_REQUIRE(fmx_aligned16(patches) && fmx_aligned16(class_embedding) && fmx_aligned16(position_embedding) && fmx_aligned16(gamma) &&
                  fmx_aligned16(beta) && fmx_aligned16(out), "clip_embed_ln: every pointer must be 16-byte aligned");
  FMX_REQUIRE(b >= 1, "clip_embed_ln: b %d < 1", b);
  FMX_REQUIRE(c >= 8 && (c % 8) == 0 && c <= 4096, "clip_embed_ln: c %d must be a multiple of 8 in 8..4096", c);
  FMX_REQUIRE(rows_per_image >= TOKENS && (rows_per_image % 64) == 0, "clip_embed_ln: rows_per_image %d must be a multiple of 64 and >= %d", rows_per_image, TOKENS);
  const long rows = (long)b * rows_per_image;
  FMX_REQUIRE(rows < (1L << 31), "clip_embed_ln: %ld rows", rows);
  const long blocks = rows / 4;   // rows_per_image % 64 == 0
  hipStream_t st = (hipStream_t)stream;
  const int oct = c >> 3;
#define FMX_CEL(MO)                                                                                                                          \
  hipLaunchKernelGGL((clip_embed_ln_kernel<MO>), dim3((unsigned)blocks), dim3(256), 0, st, (const f16*)patches, (const f16*)class_embedding, \
                     (const f16*)position_embedding, (const f16*)gamma, (const f16*)beta, (f16*)out, rows, c, (int)rows_per_image, eps)
  if (oct <= 64) FMX_CEL(1);
  else if (oct <= 128) FMX_CEL(2);
  else if (oct <= 256) FMX_CEL(4);
  else FMX_CEL(8);
#undef FMX_CEL
  FMX_LAUNCH_CHECK("fmxv_clip_embed_ln_f16");
  return FMX_OK;
}
