// ControlNet-LLLite adapters (include/fmx_lllite.h): per attention, up to three 64-wide bottleneck MLPs on the rows x [M, C] that feed to_q / to_k / to_v,
//   out_s = x + up_s( relu( mid_s( cat(cond_emb, relu(down_s(x))) ) ) ) * multiplier
// in one launch and from one read of x.  A workgroup of four waves owns 64 rows; wave w owns rows 16w .. 16w + 15 through all three stages, so the
// hidden activations in LDS are private to a wave and only the weights are shared.  Every product is computed transposed -- the weights are the A
// operand of v_mfma_f32_16x16x32, 16 rows of activations the B operand -- so a lane ends up with consecutive output CHANNELS of one row:
//   A: lane (l16, kg) holds W[out channel l16 of the block][k = 8 kg .. 8 kg + 7]      B: act[row l16][k = 8 kg .. 8 kg + 7]
//   D: lane (l16, kg) register r = out[row l16][channel 4 kg + r of the block]
//   down:  K loop over C in chunks of 64; the wd chunks of all slots go through LDS (register prefetch of the next chunk), x straight from global into
//          the B fragments (a wave reads whole 128-byte lines of its 16 rows).  + bd, ReLU, fp16 -> hid[slot]           (rounding site 1)
//   mid:   per slot, one K = 96 pass: k 0..31 the slot's cond rows of image (row / n) % Bc (a lane's 16 bytes straight from global: each module has an
//          embedding of its own, and a wave is the only reader of its rows), k 32..95 from hid[slot].  + bm, ReLU, fp16 -> hid[slot] in place (site 2)
//   up:    per slot, 64 output channels at a time.  wu rows are stored into LDS in the order the MFMA rows want them (up_lds_row) so that the two MFMAs
//          of a 32-channel group leave channels 8 kg .. 8 kg + 7 in one lane: (acc + bu) * multiplier + x in fp32, ONE rounding (site 3), a 16-byte store.
// LDS rows are padded to an odd number of 16-byte chunks (64 elements: 9, 96: 13): the 16 lanes of a ds_read_b128 phase read 16 different rows
// at one chunk, and an odd pitch spreads them over all 16 chunk positions.  No atomics, no inter-workgroup traffic, no inline assembly.
#include "fmx_common.hpp"
#include "fmx_lllite.h"

namespace {

constexpr int TPB = 256;
constexpr int TM = 64;          // rows of a workgroup
constexpr int LD = 64, LE = 32; // the adapter's hidden width and the cond embedding's width (fixed)
constexpr int KC = 64;          // K chunk of the down projection, N chunk of the up projection
constexpr int P64 = 144;        // LDS row pitch in bytes of a 64-element row: 8 chunks + 1
constexpr int P96 = 208;        // of a 96-element row (wm): 12 chunks + 1
constexpr int WM_BYTES = LD * P96, W64_BYTES = 64 * P64;
constexpr int MAX_C = 1280;

struct Slot {
  const f16 *cond, *wd, *bd, *wm, *bm, *wu, *bu;
  f16* out;
};
template <int NS>
struct Args {
  const f16* x;
  Slot s[NS];
  int c, n, bc;
  float mult;
};

// the weight region holds the wd chunks of all slots during `down`, then one slot's wm and one wu chunk
template <int NS>
constexpr int wreg_bytes() { return NS * W64_BYTES > WM_BYTES + W64_BYTES ? NS * W64_BYTES : WM_BYTES + W64_BYTES; }
template <int NS>
constexpr int lds_bytes() { return wreg_bytes<NS>() + NS * W64_BYTES; }
static_assert(lds_bytes<3>() <= 64 * 1024, "LLLite: more than 64 KB of LDS");

// LDS row of up-weight row r (0..63, an output channel of the chunk): channel 8 g + 4 a + i of a 32-channel group is row 4 g + i of that group's MFMA a
__device__ __forceinline__ constexpr int up_lds_row(int r) {
  const int r32 = r & 31;
  return (r & 32) + ((r32 >> 2) & 1) * 16 + (r32 >> 3) * 4 + (r32 & 3);
}

__device__ __forceinline__ f16x8 ld8(const char* p) { return *reinterpret_cast<const f16x8*>(p); }

// bias + ReLU + the rounding to fp16 of one 16-channel block of a hidden stage, into the wave's rows of hid
__device__ __forceinline__ void store_hidden(char* hid_row, const f32x4& acc, const f16* bias, int chan) {
  const f16x4 b4 = *reinterpret_cast<const f16x4*>(bias + chan);
  f16x4 o;
#pragma unroll
  for (int r = 0; r < 4; ++r) o[r] = (f16)fmaxf(acc[r] + (float)b4[r], 0.0f);
  *reinterpret_cast<f16x4*>(hid_row + chan * 2) = o;
}

template <int NS>
__global__ __launch_bounds__(TPB) void lllite_kernel(const Args<NS> a) {
  __shared__ __attribute__((aligned(16))) char lds[lds_bytes<NS>()];
  char* const wreg = lds;
  char* const hid = lds + wreg_bytes<NS>();
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, kg = lane >> 4;
  const int C = a.c;
  const long row0 = (long)blockIdx.x * TM;
  const int myrow = wave * 16 + l16;             // the row of the tile this lane feeds into B and gets back in D
  const f16* const xrow = a.x + (row0 + myrow) * C;

  // this lane's 8 cond values: row `myrow` of the tile (n % 64 == 0: a tile lies in one image), columns 8 kg .. 8 kg + 7, as an element offset
  const long img = row0 / a.n;
  const long cond_off = ((img % a.bc) * a.n + (row0 - img * a.n) + myrow) * LE + kg * 8;

  // ---- down: hid[s] = relu(x wd_s^T + bd_s) -------------------------------------------------------------------------------------------------------
  f32x4 acc[NS][4];
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) acc[s][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
  // a thread stages items tid and tid + 256 of each slot's 64 rows x 8 chunks
  const int st_row = tid >> 3, st_ch = tid & 7;
  f16x8 wpre[NS][2], xf[2];
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int i = 0; i < 2; ++i) wpre[s][i] = *reinterpret_cast<const f16x8*>(a.s[s].wd + (long)(st_row + i * 32) * C + st_ch * 8);
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) xf[ks] = *reinterpret_cast<const f16x8*>(xrow + ks * 32 + kg * 8);
  const int nkc = C / KC;
  for (int kc = 0; kc < nkc; ++kc) {
    __syncthreads();   // the previous chunk's fragments have been read
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int i = 0; i < 2; ++i) *reinterpret_cast<f16x8*>(wreg + s * W64_BYTES + (st_row + i * 32) * P64 + st_ch * 16) = wpre[s][i];
    __syncthreads();
    f16x8 xcur[2] = {xf[0], xf[1]};
    if (kc + 1 < nkc) {
      const int k1 = (kc + 1) * KC;
#pragma unroll
      for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int i = 0; i < 2; ++i) wpre[s][i] = *reinterpret_cast<const f16x8*>(a.s[s].wd + (long)(st_row + i * 32) * C + k1 + st_ch * 8);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) xf[ks] = *reinterpret_cast<const f16x8*>(xrow + k1 + ks * 32 + kg * 8);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
          acc[s][cb] = FMX_MFMA_16x16x32(ld8(wreg + s * W64_BYTES + (cb * 16 + l16) * P64 + (ks * 4 + kg) * 16), xcur[ks], acc[s][cb]);
  }
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) store_hidden(hid + s * W64_BYTES + myrow * P64, acc[s][cb], a.s[s].bd, cb * 16 + kg * 4);

  char* const wmb = wreg;
  char* const wub = wreg + WM_BYTES;
  const int nuc = C / KC;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const Slot& sl = a.s[s];
    char* const hrow = hid + s * W64_BYTES + myrow * P64;
    // ---- mid: hid[s] = relu(cat(cond, hid[s]) wm_s^T + bm_s), in place (a wave reads and writes its own 16 rows only) ------------------------------
    f16x8 upre[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) upre[i] = *reinterpret_cast<const f16x8*>(sl.wu + (long)(st_row + i * 32) * LD + st_ch * 8);
    __syncthreads();   // the weight region is free: `down`, or the previous slot's `up`, has read its last fragment
#pragma unroll
    for (int i = 0; i < 3; ++i) {   // 64 rows x 12 chunks
      const int item = tid + i * TPB, r = item / 12, ch = item - r * 12;
      *reinterpret_cast<f16x8*>(wmb + r * P96 + ch * 16) = *reinterpret_cast<const f16x8*>(sl.wm + r * (LE + LD) + ch * 8);
    }
    __syncthreads();
    {
      f16x8 bf[3];
      bf[0] = *reinterpret_cast<const f16x8*>(sl.cond + cond_off);
      bf[1] = ld8(hrow + kg * 16);
      bf[2] = ld8(hrow + (4 + kg) * 16);
      f32x4 macc[4];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) macc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 3; ++ks)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) macc[cb] = FMX_MFMA_16x16x32(ld8(wmb + (cb * 16 + l16) * P96 + (ks * 4 + kg) * 16), bf[ks], macc[cb]);
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) store_hidden(hrow, macc[cb], sl.bm, cb * 16 + kg * 4);
    }
    // ---- up: out_s = (hid[s] wu_s^T + bu_s) * mult + x, 64 channels per pass -----------------------------------------------------------------------
    f16x8 uf[2];
    for (int cc = 0; cc < nuc; ++cc) {
      __syncthreads();   // the previous pass has read the wu chunk (first pass: the wave's mid rows are written)
#pragma unroll
      for (int i = 0; i < 2; ++i) *reinterpret_cast<f16x8*>(wub + up_lds_row(st_row + i * 32) * P64 + st_ch * 16) = upre[i];
      __syncthreads();
      if (cc + 1 < nuc) {
#pragma unroll
        for (int i = 0; i < 2; ++i) upre[i] = *reinterpret_cast<const f16x8*>(sl.wu + ((long)(cc + 1) * KC + st_row + i * 32) * LD + st_ch * 8);
      }
      if (cc == 0) {
        uf[0] = ld8(hrow + kg * 16);
        uf[1] = ld8(hrow + (4 + kg) * 16);
      }
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const int chan = cc * KC + g * 32 + kg * 8;   // this lane's 8 output channels of row `myrow`
        const f16x8 x8 = *reinterpret_cast<const f16x8*>(xrow + chan);
        const f16x8 b8 = *reinterpret_cast<const f16x8*>(sl.bu + chan);
        f32x4 u[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          u[h] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) u[h] = FMX_MFMA_16x16x32(ld8(wub + (g * 32 + h * 16 + l16) * P64 + (ks * 4 + kg) * 16), uf[ks], u[h]);
        }
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (f16)fmaf(u[j >> 2][j & 3] + (float)b8[j], a.mult, (float)x8[j]);
        *reinterpret_cast<f16x8*>(sl.out + (row0 + myrow) * C + chan) = o;
      }
    }
  }
}

template <int NS>
void launch(const Args<NS>& a, long tiles, hipStream_t st) {
  hipLaunchKernelGGL(lllite_kernel<NS>, dim3((unsigned)tiles), dim3(TPB), 0, st, a);
}

bool overlap(const void* p, const void* q, size_t bytes) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + bytes && b < a + bytes;
}

}  // namespace

extern "C" int fmxl_lllite_adapt_f16(const void* x, int64_t m, int32_t c, int32_t d, int32_t e, int32_t rows_per_image,
                                     int32_t cond_images, const fmxl_lllite_slot* q, const fmxl_lllite_slot* k, const fmxl_lllite_slot* v,
                                     float multiplier, void* stream) {
  FMX_REQUIRE(d == LD && e == LE, "lllite_adapt: hidden width %d and cond embedding width %d (the kernel is built for 64 and 32)", d, e);
  FMX_REQUIRE(c >= 64 && c <= MAX_C && c % 64 == 0, "lllite_adapt: c = %d (a multiple of 64, at most %d)", c, MAX_C);
  FMX_REQUIRE(m > 0 && m % TM == 0 && m / TM < (1L << 31), "lllite_adapt: m = %ld rows (a positive multiple of 64)", (long)m);
  FMX_REQUIRE(rows_per_image > 0 && rows_per_image % 64 == 0 && m % rows_per_image == 0,
              "lllite_adapt: rows_per_image = %d (a positive multiple of 64 that divides m = %ld)", rows_per_image, (long)m);
  FMX_REQUIRE(cond_images >= 1, "lllite_adapt: cond_images = %d", cond_images);
  FMX_REQUIRE(x, "lllite_adapt: null pointer (x)");
  FMX_REQUIRE(fmx_aligned16(x), "lllite_adapt: x must be 16-byte aligned");
  const fmxl_lllite_slot* in[3] = {q, k, v};
  const fmxl_lllite_slot* sl[3];
  int ns = 0;
  const size_t bytes = (size_t)m * c * sizeof(f16);
  for (int i = 0; i < 3; ++i) {
    const fmxl_lllite_slot* s = in[i];
    if (!s) continue;
    FMX_REQUIRE(s->cond && s->wd && s->bd && s->wm && s->bm && s->wu && s->bu && s->out, "lllite_adapt: null pointer in slot %d", i);
    FMX_REQUIRE(fmx_aligned16(s->cond) && fmx_aligned16(s->wd) && fmx_aligned16(s->bd) && fmx_aligned16(s->wm) && fmx_aligned16(s->bm) && fmx_aligned16(s->wu) &&
                    fmx_aligned16(s->bu) && fmx_aligned16(s->out),
                "lllite_adapt: the pointers of slot %d must be 16-byte aligned", i);
    FMX_REQUIRE(!overlap(s->out, x, bytes), "lllite_adapt: out of slot %d aliases x", i);
    for (int j = 0; j < ns; ++j) FMX_REQUIRE(!overlap(s->out, sl[j]->out, bytes), "lllite_adapt: out of slot %d aliases another out", i);
    sl[ns++] = s;
  }
  FMX_REQUIRE(ns > 0, "lllite_adapt: no slot (q, k and v are all absent)");
  const long tiles = m / TM;
  auto fill = [&](auto& a) {
    a.x = (const f16*)x;
    a.c = c;
    a.n = rows_per_image;
    a.bc = cond_images;
    a.mult = multiplier;
    for (int i = 0; i < ns; ++i)
      a.s[i] = Slot{(const f16*)sl[i]->cond, (const f16*)sl[i]->wd, (const f16*)sl[i]->bd, (const f16*)sl[i]->wm, (const f16*)sl[i]->bm,
                    (const f16*)sl[i]->wu, (const f16*)sl[i]->bu, (f16*)sl[i]->out};
  };
  if (ns == 1) {
    Args<1> a;
    fill(a);
    launch<1>(a, tiles, (hipStream_t)stream);
  } else if (ns == 2) {
    Args<2> a;
    fill(a);
    launch<2>(a, tiles, (hipStream_t)stream);
  } else {
    Args<3> a;
    fill(a);
    launch<3>(a, tiles, (hipStream_t)stream);
  }
  FMX_LAUNCH_CHECK("fmxl_lllite_adapt_f16");
  return FMX_OK;
}
