// The "attention" of Perturbed-Attention Guidance's degraded images (include/fmx.h, section "Perturbed-Attention Guidance"): the reference replaces
// the middle block's self-attention by `lambda q, k, v, to: v`, so O = V.  The executor holds V feature-major (V^T, the attention kernel's operand)
// and O token-major, hence a transposition: a 64 token x 64 feature tile of 16-bit words per workgroup through LDS, 16-byte loads along the tokens,
// 16-byte stores along the features.  Pure data movement on 16-bit words: no arithmetic, no atomics, the same bits on every run.
//
// LDS tile: 64 token rows of 32 dwords (one dword = the features 2p, 2p + 1 of one token) at a pitch of 33 dwords.
//   write, ds_write_b32, banks = dword mod 32 per 32-lane group: a group holds 4 token octets x 8 feature pairs and writes the rows 8 tg + k,
//     dword (8 tg + k) * 33 + pair = 8 tg + pair + const (mod 32), tg < 4, pair < 8: 32 distinct banks.
//   read, ds_read_b32 (x 4 per lane), per 32-lane group: 4 tokens x 8 feature octets, dword t * 33 + 4 fg + j = t + 4 fg + const (mod 32),
//     t in 4 consecutive values from a multiple of 4, fg < 8: 32 distinct banks.
// An unpadded pitch of 32 would put the 4 token octets of a write group on one bank each (4-way).
#include "fmx_common.hpp"

namespace {

constexpr int TPB = 256;
constexpr int TILE = 64;
constexpr int PITCH = 33;   // dwords per token row of the LDS tile

typedef unsigned short u16;
typedef u16 u16x8 __attribute__((ext_vector_type(8)));

// out[b, t, f] = vt[f * vt_ds + b * vt_bs + t], b0 <= b < b0 + gridDim.z, t < n, f < hd.   VEC: every 8-element group of both sides is 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(TPB) void value_rows_kernel(const u16* __restrict__ vt, long vt_bs, long vt_ds, u16* __restrict__ out, long o_rs, long o_bs,
                                                        int hd, int n, int b0) {
  __shared__ uint32_t tile[TILE * PITCH];
  const int tid = threadIdx.x;
  const int t0 = blockIdx.x * TILE, f0 = blockIdx.y * TILE;
  const long b = (long)b0 + blockIdx.z;
  const u16* src = vt + b * vt_bs;
  u16* dst = out + b * o_bs;
  if (VEC) {
    // load: a 32-lane half wave holds the token octets 4 * half .. 4 * half + 3 of 8 feature pairs; a wave 8 pairs, the workgroup all 32
    const int lane = tid & 63, wave = tid >> 6;
    const int tg = (lane & 3) + 4 * (lane >> 5);
    const int pair = ((lane >> 2) & 7) + 8 * wave;
    const int t = t0 + 8 * tg, f = f0 + 2 * pair;
    u16x8 va = {0, 0, 0, 0, 0, 0, 0, 0}, vb = va;
    if (t < n && f < hd) {      // hd is even: f + 1 < hd as well
      const u16* p = src + (long)f * vt_ds + t;
      if (t + 8 <= n) {
        va = *reinterpret_cast<const u16x8*>(p);
        vb = *reinterpret_cast<const u16x8*>(p + vt_ds);
      } else {                  // the last octet of an image: no read past token n - 1
        for (int k = 0; k < n - t; ++k) {
          va[k] = p[k];
          vb[k] = p[vt_ds + k];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) tile[(8 * tg + k) * PITCH + pair] = (uint32_t)va[k] | ((uint32_t)vb[k] << 16);
    __syncthreads();
    // store: 8 lanes write the 128 contiguous bytes of one token's 64 features
    const int fg = tid & 7;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int tt = (tid >> 3) + 32 * pass;
      uint32_t w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = tile[tt * PITCH + 4 * fg + j];
      if (t0 + tt < n && f0 + 8 * fg < hd) {   // hd % 8 == 0: the whole octet is inside
        uint4 v = make_uint4(w[0], w[1], w[2], w[3]);
        *reinterpret_cast<uint4*>(dst + (long)(t0 + tt) * o_rs + f0 + 8 * fg) = v;
      }
    }
  } else {
    u16* th = reinterpret_cast<u16*>(tile);   // [token][feature] at a pitch of 2 * PITCH 16-bit words
    for (int i = tid; i < TILE * TILE; i += TPB) {
      const int fl = i >> 6, tl = i & 63;     // consecutive lanes: consecutive tokens of one feature row
      u16 v = 0;
      if (t0 + tl < n && f0 + fl < hd) v = src[(long)(f0 + fl) * vt_ds + t0 + tl];
      th[tl * (2 * PITCH) + fl] = v;
    }
    __syncthreads();
    for (int i = tid; i < TILE * TILE; i += TPB) {
      const int tl = i >> 6, fl = i & 63;     // consecutive lanes: consecutive features of one token
      if (t0 + tl < n && f0 + fl < hd) dst[(long)(t0 + tl) * o_rs + f0 + fl] = th[tl * (2 * PITCH) + fl];
    }
  }
}

}  // namespace

extern "C" int fmx_attn_value_rows_f16(const void* vt, int64_t vt_bs, int64_t vt_ds, void* out, int64_t o_rs, int64_t o_bs, int32_t hd, int32_t n,
                                       int32_t b0, int32_t nb, void* stream) {
  FMX_REQUIRE(vt && out, "attn_value_rows: null pointer");
  FMX_REQUIRE(hd > 0 && (hd % 8) == 0 && n > 0 && b0 >= 0 && nb > 0 && nb <= 65535, "attn_value_rows: hd %d (multiple of 8), n %d, window [%d, %d + %d)",
              hd, n, b0, b0, nb);
  FMX_REQUIRE(vt_bs >= n && vt_ds >= n && o_rs >= hd && o_bs >= 0, "attn_value_rows: vt_bs %ld / vt_ds %ld below n %d, or row stride %ld below hd %d",
              (long)vt_bs, (long)vt_ds, n, (long)o_rs, hd);
  const dim3 grid((unsigned)((n + TILE - 1) / TILE), (unsigned)((hd + TILE - 1) / TILE), (unsigned)nb);
  FMX_REQUIRE(grid.y <= 65535, "attn_value_rows: hd %d too wide", hd);
  const bool vec = fmx_aligned16(vt) && fmx_aligned16(out) && (vt_bs % 8) == 0 && (vt_ds % 8) == 0 && (o_rs % 8) == 0 && (o_bs % 8) == 0;
  if (vec)
    hipLaunchKernelGGL(value_rows_kernel<true>, grid, dim3(TPB), 0, (hipStream_t)stream, (const u16*)vt, (long)vt_bs, (long)vt_ds, (u16*)out,
                       (long)o_rs, (long)o_bs, hd, n, b0);
  else
    hipLaunchKernelGGL(value_rows_kernel<false>, grid, dim3(TPB), 0, (hipStream_t)stream, (const u16*)vt, (long)vt_bs, (long)vt_ds, (u16*)out,
                       (long)o_rs, (long)o_bs, hd, n, b0);
  FMX_LAUNCH_CHECK("fmx_attn_value_rows_f16");
  return FMX_OK;
}
