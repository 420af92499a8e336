// What the direct 3x3 convolution kernels share -- fmx_conv_patch.hip (GroupNorm + SiLU + conv, 128 output channels), fmx_conv_c64.hip (TAESD, resident
// weights), fmx_conv_dense.hip (ESRGAN, channel-chunk stages) and fmx_conv_narrow.hip (<= 4 output channels, its own 4-row tile): the output tile and its
// accumulator layout, the swizzled 128-byte-pixel LDS format with its per-tap MFMA step, the item geometry of a patch staged through registers, the
// GroupNorm + SiLU arithmetic of the fused forms (the very function gn_apply_kernel in fmx_norm.hip stores with), and the host side of their launches.
// Written against the translation unit's `f16`; everything has internal linkage (the files are compiled once per element type into one library).
#pragma once
#include "fmx_common.hpp"

int fmx_launch_gn_finalize(const float* partial, int32_t nchunks, int32_t c, int32_t n, int32_t groups, int32_t hw, float eps, const void* gamma,
                           const void* beta, float* scale_shift, hipStream_t st);   // fmx_norm.hip

namespace {

// ---- 1. the tile -----------------------------------------------------------------------------------------------------------------------------------
constexpr int TH = 8, TW = 32;                 // output tile of a workgroup (the narrow kernel: 4 rows of TW)
constexpr int PH = TH + 2, PW = TW + 2;        // staged patch (1-pixel halo)

struct TilePos { int img, ty, tx; };
__device__ __forceinline__ TilePos tile_decode(int tile, int tiles_x, int tiles_per_img) {
  const int img = tile / tiles_per_img, tin = tile - img * tiles_per_img;
  const int ty = tin / tiles_x;
  return {img, ty, tin - ty * tiles_x};
}

// Accumulators of an 8 x 32 tile: a wave owns 2 rows = 4 pixel blocks x NCB channel blocks of v_mfma_f32_16x16x32 (weights the A operand, 16 neighbouring
// pixels of a patch row the B operand).  Lane (l16, kg) of block (pb, cb) holds output channels acc_chan(cb, kg) + 0..3 of tile pixel (acc_row(wave, pb),
// acc_col(pb, l16)).
__device__ __forceinline__ constexpr int acc_row(int wave, int pb) { return 2 * wave + (pb >> 1); }
__device__ __forceinline__ constexpr int acc_col(int pb, int l16) { return (pb & 1) * 16 + l16; }
__device__ __forceinline__ constexpr int acc_chan(int cb, int kg) { return cb * 16 + kg * 4; }
// pixels from block 0's fragment to block pb's in a patch of PW-pixel rows
__device__ __forceinline__ constexpr int pb_patch_pixels(int pb) { return acc_row(0, pb) * PW + acc_col(pb, 0); }

struct OutPixel {
  bool ok;   // inside the oh x ow image (row / column tails of the tile are not)
  long m;    // pixel index in [n][oh][ow]
};
__device__ __forceinline__ OutPixel out_pixel(const TilePos& t, int wave, int pb, int l16, int oh, int ow) {
  const int oy = t.ty * TH + acc_row(wave, pb), ox = t.tx * TW + acc_col(pb, l16);
  return {oy < oh && ox < ow, ((long)t.img * oh + oy) * ow + ox};
}

// (`bias` by reference: the kernel argument is read where it is used, not copied ahead of the loop)
template <int NCB>
__device__ __forceinline__ void load_bias(f32x4 (&bsum)[NCB], const f16* const& bias, int kg) {
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) {
    bsum[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (bias) {
      const f16x4 b4 = *reinterpret_cast<const f16x4*>(bias + acc_chan(cb, kg));
#pragma unroll
      for (int r = 0; r < 4; ++r) bsum[cb][r] = (float)b4[r];
    }
  }
}

__device__ __forceinline__ f16x8 zero_octet() {
  f16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (f16)0.0f;
  return v;
}

// ---- 2. the swizzled 128-byte-pixel LDS format (64 channels per pixel / weight row) -----------------------------------------------------------------
// 16-byte chunk c of patch column q sits at chunk c ^ swz_key(q), chunk c of weight row o at c ^ swz_key(o): the 16 neighbouring pixels (rows) of one
// fragment read spread over all bank groups.  The key of 16 + q equals the key of q.
__device__ __forceinline__ constexpr int swz_key(int q) { return (q >> 1) & 7; }
// byte offset of chunk c of 128-byte slot `slot` (a patch pixel, a weight row) whose column (row) number is `q`
__device__ __forceinline__ constexpr int swz_off(int slot, int q, int c) { return slot * 128 + ((c ^ swz_key(q)) << 4); }

// Per-lane fragment offsets of one tap.  Weights: row cb * 16 + l16 (cb * 16 does not change the key); activations: pixel column (pb & 1) * 16 + l16 + kx of
// patch row 2 * wave + (pb >> 1) + ky.  Every term but the chunk bits (4-6) is a multiple of 128, so k-step 1 (logical chunks 4-7) is `^ 64`.
__device__ __forceinline__ int w_frag_off(int l16, int kg) { return swz_off(l16, l16, kg); }
__device__ __forceinline__ int p_frag_off(int wave, int l16, int kg, int ky, int kx) {
  const int q0 = l16 + kx;
  return swz_off((acc_row(wave, 0) + ky) * PW + q0, q0, kg);
}

// One tap of 64 input channels: acc[pb][cb] += W[tap][cb] x patch[pb shifted by the tap]; `wo` / `po` are w_frag_off / p_frag_off plus the multiples of 128
// that select the tap's weights and the patch, from wbase / pbase.
// (the block / pixel-block offsets are multiples of 128 and leave bit 6 alone: one base per k-step, every read an immediate offset)
template <int NCB>
__device__ __forceinline__ void tap_mfma(f32x4 (&acc)[4][NCB], const char* wbase, int wo, const char* pbase, int po) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    f16x8 wf[NCB], af[4];
    const char* wks = wbase + (wo ^ (ks * 64));
    const char* pks = pbase + (po ^ (ks * 64));
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) wf[cb] = *reinterpret_cast<const f16x8*>(wks + cb * 2048);
#pragma unroll
    for (int pb = 0; pb < 4; ++pb) af[pb] = *reinterpret_cast<const f16x8*>(pks + pb_patch_pixels(pb) * 128);
#pragma unroll
    for (int pb = 0; pb < 4; ++pb)
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) acc[pb][cb] = FMX_MFMA_16x16x32(wf[cb], af[pb], acc[pb][cb]);
  }
}

// ---- 3. a patch staged through registers ------------------------------------------------------------------------------------------------------------
// (fmx_conv_patch.hip, fmx_conv_c64.hip; the dense and narrow kernels walk their own octet counts and patch widths with the same scheme, in place: through
// this helper their staging loops compiled to other code, and the widest dense shape measured slower)
// 256 threads walk the 16-byte items of the PH x PW patch with OCT channel octets per pixel: a thread keeps ONE octet (tid % OCT) and takes patch pixel
// tid / OCT + it * (256 / OCT) in iteration `it`.  (y0, x0) is the tile's first output pixel, oh x ow the image the convolution runs on.
struct PatchItem {
  int pi, q;       // patch pixel (past the patch in the tail of the last iteration), its column
  int gy, gx;      // the same pixel in the image
};
template <int OCT>
__device__ __forceinline__ PatchItem patch_item(int tid, int it, int y0, int x0) {
  const int pi = tid / OCT + it * (256 / OCT);
  const int pr = pi / PW, q = pi - pr * PW;
  return {pi, q, y0 - 1 + pr, x0 - 1 + q};
}
// everything outside the oh x ow image is the convolution's zero padding
__device__ __forceinline__ bool in_image(const PatchItem& i, int oh, int ow) { return i.gy >= 0 && i.gy < oh && i.gx >= 0 && i.gx < ow; }
// pixel index of the item's source in [n][h][w]; up = 1: the convolution runs on the 2x nearest-neighbour upsampling of that tensor
__device__ __forceinline__ long patch_src_pixel(const PatchItem& i, int img, int h, int w, int up = 0) {
  return ((long)img * h + (i.gy >> up)) * w + (i.gx >> up);
}

// ---- 4. GroupNorm (+ SiLU) on the way into LDS ------------------------------------------------------------------------------------------------------
// The one place the normalised value is formed: gn_apply_kernel stores it, the fused kernels stage it, so both round the same number.
template <bool SILU = true>
__device__ __forceinline__ float gn_norm_f(float x, float scale, float shift) {
  return SILU ? silu_f(fmaf(x, scale, shift)) : fmaf(x, scale, shift);
}
// {scale, shift} of 8 consecutive channels; `ssp`: the first of them in gn_finalize's [n][channels][2] table.  sv[i] = the pairs of channels 2i, 2i + 1
__device__ __forceinline__ void load_scale_shift(f32x4 (&sv)[4], const float* ssp) {
#pragma unroll
  for (int i = 0; i < 4; ++i) sv[i] = *reinterpret_cast<const f32x4*>(ssp + i * 4);
}
__device__ __forceinline__ f16x8 gn_silu_octet(const f16x8 v, const f32x4 (&sv)[4]) {
  f16x8 r;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const f32x4 s = sv[e >> 1];
    r[e] = (f16)gn_norm_f((float)v[e], s[(e & 1) * 2], s[(e & 1) * 2 + 1]);
  }
  return r;
}
// An item between its global load and its LDS store: -1 = no item; else the LDS byte offset, bit 30 = outside the image (zeros: the convolution pads the
// NORMALISED tensor)
constexpr int ITEM_OUTSIDE = 1 << 30;
__device__ __forceinline__ int gn_item_off(bool in_patch, bool ok, int lds_off) { return in_patch ? (lds_off | (ok ? 0 : ITEM_OUTSIDE)) : -1; }
__device__ __forceinline__ void gn_silu_store(char* patch, int off, const f16x8 v, const f32x4 (&sv)[4]) {
  if (off < 0) return;
  f16x8 r;
  if (off & ITEM_OUTSIDE)
    r = zero_octet();
  else
    r = gn_silu_octet(v, sv);
  *reinterpret_cast<f16x8*>(patch + (off & (ITEM_OUTSIDE - 1))) = r;
}

// ---- 5. host ---------------------------------------------------------------------------------------------------------------------------------------
struct TileGrid {
  int tiles_x, tiles_y;
  long ntiles;
  bool one_launch() const { return ntiles < (1L << 31); }   // the kernels index tiles with an int
};
inline TileGrid tile_grid(int n, int oh, int ow, int th = TH) {
  const int tiles_x = (ow + TW - 1) / TW, tiles_y = (oh + th - 1) / th;
  return {tiles_x, tiles_y, (long)n * tiles_x * tiles_y};
}

// Workgroups of a persistent kernel: one per CU (the count is read once), one per tile where there are fewer.  0: the CU count cannot be read.
inline unsigned persistent_grid(long ntiles) {
  static int cus = 0;
  if (!cus) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) return 0;
    cus = v;
  }
  return (unsigned)(ntiles < cus ? ntiles : cus);
}

// a kernel's dynamic-LDS ceiling is raised once, at its first launch
template <auto KERNEL, int BYTES>
void lds_ceiling_once() {
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, BYTES);
  (void)attr;
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }   // a null (absent) operand passes

}  // namespace
