// IP-Adapter (lib_ipadapter/IPAdapterPlus.py CrossAttentionPatch.__call__): cross-attention over the text context PLUS up to four independent
// softmaxes over image-token segments of an extra context, O = attention(q, k_text, v_text) + sum_s w_s attention(q, k_ip_s, v_ip_s), in one
// launch (include/fmx_ipadapter.h).
//
// The 77-key cross-attention is a streaming kernel bound by its one read of Q and one write of O; as a second attention launch plus
// an add, the image keys cost a second read of Q and a read-modify-write of O.  Here they ride in the text launch.  The kernel is
// attn_short2_kernel (fmx_attention.hip) with an extra context: persistent workgroups that walk a contiguous range of (batch, head, 128-query
// tile), K / V^T of the (batch, head) staged once in LDS by LDS-DMA, Q one tile ahead and O through per-wave LDS slots in whole lines, the same
// operand layouts (S^T = K Q^T with permuted key rows, O^T = V^T P^T, lane = query).  The text term is computed by the same instructions in the
// same order as there.  fmx_attention.hip is not touched -- its kernels and dispatch stay bit-identical -- so the three small index helpers are
// restated here, not shared through a header.
//
// Extra context: the group's 32 or 64 extra key rows and its 64 V^T rows are staged next to the text tiles.  After the text scores, the extra
// scores (NBX 32-key blocks) are taken from the same Q fragments; each segment's maximum and sum are lane-local over the lane's keys of the
// segment plus one permlane32 swap between the two lane halves that share a query, exactly like the text softmax.  A segment's probabilities
// are scaled by weight / sum in fp32 BEFORE their one rounding to fp16 (the weight is folded into P), so all segments together are ONE further
// chain of MFMAs on top of the text accumulator after that has been multiplied by 1 / (text sum): no second accumulator, no extra pass per
// segment.  Keys outside every segment get P = 0 by a select on the key index, so what xk holds there never matters.
//
// LDS, the decision: short2 holds 64 KiB per workgroup (two text K / V^T stages of 16 KiB, four waves x two 4-KiB Q / O slots) at two workgroups
// per CU.  The extra tiles add NBX * 4 KiB of K rows and 8 KiB of V^T: 76 KiB with up to 32 extra keys, 80 KiB with up to 64.  Two workgroups are
// 152 / 160 KiB of the CU's 160 KiB (workgroups per CU = floor(160 KiB / LDS per workgroup), MI355X_MICROARCH.md "Register files"): both still
// fit two per CU, which is what keeps the walk's latency chain overlapped, so the extra context gets tiles of its own rather than being squeezed
// into the unused tail of the second text stage (13 of its 64 K rows at 77 keys, but its V^T rows are interleaved with the live ones).  The
// extra K tile uses the text K tile's chunk swizzle and the extra V^T tile the text V^T tile's, so every ds_read_b128 is conflict-free as there.
#include <math.h>

#include "fmx_common.hpp"
#include "fmx_ipadapter.h"

namespace {

struct DualParams {
  const f16* q;
  const f16* k;
  const f16* vt;
  f16* o;
  const f16* xk;
  const f16* xvt;
  long q_bs, q_rs, k_bs, k_rs, vt_bs, vt_hs, vt_ds, o_bs, o_rs;
  int batch, heads, nq, nk, qtiles, images_per_group, groups;
  float scale_log2e;
  unsigned q_span, k_span, vt_span, xk_span, xvt_span;
  int nseg;
  int seg_lo[FMXI_MAX_SEGMENTS], seg_hi[FMXI_MAX_SEGMENTS];   // keys [lo, hi)
  float seg_w[FMXI_MAX_SEGMENTS];
};

constexpr int KVB = 64;   // keys per tile

// the 16-byte chunk swizzle of a 128-byte row (eight chunks), its own inverse; and the key-row permutation of the score MFMA (fmx_attention.hip)
__device__ __forceinline__ int chunk8(int row, int c) { return c ^ ((row >> 1) & 7); }
__device__ __forceinline__ int key_perm(int i) { return (i & 3) | (((i >> 3) & 3) << 2) | (((i >> 2) & 1) << 4); }

constexpr int STAGE = KVB * 64 * 2 + 2 * 32 * 128;   // one text K tile + one text V^T tile
constexpr int KV_BYTES = 2 * STAGE;
constexpr int SLOT_BYTES = 4 * 8192;
constexpr int dual_lds(int nbx) { return KV_BYTES + SLOT_BYTES + nbx * 4096 + 8192; }

// NB: 32-key blocks that hold text keys (1..4); NBX: 32-key blocks that hold segment keys (1..2)
template <int NB, int NBX>
__global__ __launch_bounds__(256, 2) void attn_dual_kernel(const DualParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int DP = 64, DSTEPS = 4;
  constexpr int KBYTES = KVB * DP * 2;
  constexpr int NT = (NB + 1) / 2;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, li = lane & 31;
  char* const slots = smem + KV_BYTES + wave * 8192;   // this wave's two Q / O slots
  char* const xks = smem + KV_BYTES + SLOT_BYTES;      // extra K rows [NBX * 32][64]
  char* const xvs = xks + NBX * 4096;                  // extra V^T [64 rows][64 keys]
  // tiles [g0, g1) of the flattened (batch * heads, 128-query tile) list
  const int total = p.batch * p.heads * p.qtiles;
  const int per = (total + (int)gridDim.x - 1) / (int)gridDim.x;
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int g0 = wg * per, g1 = min(total, g0 + per);
  if (g0 >= g1) return;

  const float c2 = p.scale_log2e;
  const int krow = key_perm(li);
  const int r8 = lane >> 3, pc = lane & 7;       // DMA / line pass: row within an 8-row piece, physical 16-byte chunk
  typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

  int bh_cur = -1;
  __amdgpu_buffer_rsrc_t rs_q = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(p.q), 0, 0, 0x00020000);
  auto q_desc = [&](int bh) {
    const int h = bh % p.heads, b = bh / p.heads;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(p.q + (long)b * p.q_bs + (long)h * DP), 0, p.q_span, 0x00020000);
  };
  // Q tile `tile` of the current (batch, head) -> slot: 4 pieces, rows >= nq read as zeros (descriptor bounds)
  auto dma_q = [&](const __amdgpu_buffer_rsrc_t& rs, int tile, int slot) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = e * 8 + r8;
      const unsigned off = (unsigned)(tile * 128 + wave * 32 + row) * (unsigned)p.q_rs * 2u + (unsigned)chunk8(row, pc) * 16u;
      auto* dst = (__attribute__((address_space(3))) void*)(slots + slot * 4096 + e * 1024);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, dst, 16, off, 0, 0, 0);
    }
  };

  int slot = 0;
  for (int g = g0; g < g1; ++g) {
    const int bh = g / p.qtiles, tile = g - bh * p.qtiles;
    const int h = bh % p.heads, b = bh / p.heads;
    if (bh != bh_cur) {
      // new (batch, head): every wave is done with the old K / V^T tiles; stage the new ones, the group's extra tiles and this tile's Q
      if (bh_cur >= 0) {
        wait_vmcnt0();
        __syncthreads();
      }
      bh_cur = bh;
      rs_q = q_desc(bh);
      const f16* kbase = p.k + (long)b * p.k_bs + (long)h * DP;
      const f16* vbase = p.vt + (long)b * p.vt_bs + (long)h * p.vt_hs;
      const __amdgpu_buffer_rsrc_t rs_k = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(kbase), 0, p.k_span, 0x00020000);
      const __amdgpu_buffer_rsrc_t rs_v = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(vbase), 0, p.vt_span, 0x00020000);
#pragma unroll
      for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int kr = (e * 4 + wave) * 8 + r8;
          const unsigned kv = (unsigned)kr * (unsigned)p.k_rs * 2u + (unsigned)chunk8(kr, pc) * 16u;
          auto* dk = (__attribute__((address_space(3))) void*)(smem + kt * STAGE + (e * 4 + wave) * 1024);
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_k, dk, 16, kv, (unsigned)kt * ((unsigned)KVB * (unsigned)p.k_rs * 2u), 0, 0);
          const unsigned vv = (unsigned)kr * (unsigned)p.vt_ds * 2u + (unsigned)chunk8(kr, pc) * 16u;
          auto* dv = (__attribute__((address_space(3))) void*)(smem + kt * STAGE + KBYTES + (e * 4 + wave) * 1024);
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_v, dv, 16, vv, (unsigned)kt * (KVB * 2u), 0, 0);
        }
      // the extra context of this image's group: key rows [0, NBX * 32) and all 64 V^T rows of head h (dense layouts, include/fmx_ipadapter.h)
      const int grp = b / p.images_per_group;
      const unsigned xk_rs = (unsigned)p.heads * DP, xvt_ds = (unsigned)p.groups * KVB;
      const f16* xkbase = p.xk + ((long)grp * KVB * p.heads + h) * DP;
      const f16* xvbase = p.xvt + (long)h * DP * xvt_ds + (long)grp * KVB;
      const __amdgpu_buffer_rsrc_t rs_xk = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(xkbase), 0, p.xk_span, 0x00020000);
      const __amdgpu_buffer_rsrc_t rs_xv = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(xvbase), 0, p.xvt_span, 0x00020000);
#pragma unroll
      for (int e = 0; e < NBX; ++e) {
        const int kr = (e * 4 + wave) * 8 + r8;
        auto* dk = (__attribute__((address_space(3))) void*)(xks + (e * 4 + wave) * 1024);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_xk, dk, 16, (unsigned)kr * xk_rs * 2u + (unsigned)chunk8(kr, pc) * 16u, 0, 0, 0);
      }
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int vr = (e * 4 + wave) * 8 + r8;
        auto* dv = (__attribute__((address_space(3))) void*)(xvs + (e * 4 + wave) * 1024);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_xv, dv, 16, (unsigned)vr * xvt_ds * 2u + (unsigned)chunk8(vr, pc) * 16u, 0, 0, 0);
      }
      dma_q(rs_q, tile, slot);
      wait_vmcnt0();
      __syncthreads();
    } else {
      // this tile's Q was requested a tile ago; behind it in the (in-order) counter are only the 4 line stores of the previous tile's O
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    }
    // ---- Q fragments out of the slot (pre-scaled), then the NEXT tile's Q into the other slot ----
    f16x8 qf[DSTEPS];
    {
      const char* qs = slots + slot * 4096 + li * 128;
#pragma unroll
      for (int ds = 0; ds < DSTEPS; ++ds) {
        const f16x8 raw = *reinterpret_cast<const f16x8*>(qs + (chunk8(li, ds * 2 + hi) << 4));
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[ds][e] = (f16)((float)raw[e] * c2);
      }
    }
    const bool more = g + 1 < g1 && (g + 1) / p.qtiles == bh;   // uniform
    // pinned in program order: the vmcnt(4) above counts on exactly this tile's four O stores being the only memory operations behind it
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (more) dma_q(rs_q, tile + 1, slot ^ 1);
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");

    // ---- text scores ----
    f32x16 sacc[NB];
#pragma unroll
    for (int gk = 0; gk < NB; ++gk) {
#pragma unroll
      for (int r = 0; r < 16; ++r) sacc[gk][r] = 0.f;
      const char* sk = smem + (gk >> 1) * STAGE;
      const int row = (gk & 1) * 32 + krow;
#pragma unroll
      for (int ds = 0; ds < DSTEPS; ++ds) {
        const f16x8 kf = *reinterpret_cast<const f16x8*>(sk + row * (DP * 2) + (chunk8(row, ds * 2 + hi) << 4));
        sacc[gk] = FMX_MFMA_32x32x16(kf, qf[ds], sacc[gk]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---- text softmax (attn_short2_kernel's) ----
#pragma unroll
    for (int gk = 0; gk < NB; ++gk)
      if ((gk + 1) * 32 > p.nk) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (gk * 32 + hi * 16 + r >= p.nk) sacc[gk][r] = -INFINITY;
      }
    float m0 = sacc[0][0];
#pragma unroll
    for (int gk = 0; gk < NB; ++gk)
#pragma unroll
      for (int r = 0; r < 16; ++r) m0 = fmaxf(m0, sacc[gk][r]);
    const u32x2 sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(m0), __float_as_uint(m0), false, false);
    const float mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
    float l = 0.f;
    f16x8 pf[NB][2];
#pragma unroll
    for (int gk = 0; gk < NB; ++gk)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = __builtin_amdgcn_exp2f(sacc[gk][r] - mx);
        l += e;
        pf[gk][r >> 3][r & 7] = (f16)e;
      }
    // ---- the extra scores, from the same Q fragments ----
    f32x16 xacc[NBX];
#pragma unroll
    for (int gk = 0; gk < NBX; ++gk) {
#pragma unroll
      for (int r = 0; r < 16; ++r) xacc[gk][r] = 0.f;
      const int row = gk * 32 + krow;
#pragma unroll
      for (int ds = 0; ds < DSTEPS; ++ds) {
        const f16x8 kf = *reinterpret_cast<const f16x8*>(xks + row * (DP * 2) + (chunk8(row, ds * 2 + hi) << 4));
        xacc[gk] = FMX_MFMA_32x32x16(kf, qf[ds], xacc[gk]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---- the segments: an independent softmax each over the lane's keys [lo, hi) of the extra blocks; P = e * weight / sum, 0 elsewhere ----
    // (a key outside every segment keeps P = 0 whatever its score was)
    f32x16 xp[NBX];
#pragma unroll
    for (int gk = 0; gk < NBX; ++gk)
#pragma unroll
      for (int r = 0; r < 16; ++r) xp[gk][r] = 0.f;
#pragma unroll 1
    for (int s = 0; s < p.nseg; ++s) {   // uniform; not unrolled: the body is 32 or 64 keys' worth of code
      const int lo = p.seg_lo[s] - hi * 16, up = p.seg_hi[s] - hi * 16;   // in the lane's own key numbering: key of (gk, r) = gk * 32 + r
      // the key index is looked at ONCE: scores outside the segment become -inf there, and exp2(-inf - max) = 0 carries that through the sum
      // and the product below without a second select
      f32x16 t[NBX];
      float ms = -INFINITY;
#pragma unroll
      for (int gk = 0; gk < NBX; ++gk)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          t[gk][r] = (gk * 32 + r >= lo && gk * 32 + r < up) ? xacc[gk][r] : -INFINITY;
          ms = fmaxf(ms, t[gk][r]);
        }
      const u32x2 sm = __builtin_amdgcn_permlane32_swap(__float_as_uint(ms), __float_as_uint(ms), false, false);
      const float mxs = fmaxf(__uint_as_float(sm[0]), __uint_as_float(sm[1]));   // count >= 1: one of the two halves holds a key
      float ls = 0.f;
#pragma unroll
      for (int gk = 0; gk < NBX; ++gk)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          t[gk][r] = __builtin_amdgcn_exp2f(t[gk][r] - mxs);
          ls += t[gk][r];
        }
      const u32x2 sl = __builtin_amdgcn_permlane32_swap(__float_as_uint(ls), __float_as_uint(ls), false, false);
      const float f = p.seg_w[s] / (__uint_as_float(sl[0]) + __uint_as_float(sl[1]));
#pragma unroll
      for (int gk = 0; gk < NBX; ++gk)
#pragma unroll
        for (int r = 0; r < 16; ++r) xp[gk][r] = fmaf(t[gk][r], f, xp[gk][r]);   // segments are disjoint: all but one term of a key are 0
    }
    f16x8 xpf[NBX][2];
#pragma unroll
    for (int gk = 0; gk < NBX; ++gk)
#pragma unroll
      for (int r = 0; r < 16; ++r) xpf[gk][r >> 3][r & 7] = (f16)xp[gk][r];

    // ---- O^T = (V^T P^T) / l  +  XV^T XP^T: the extra MFMAs continue the accumulator the text term has been normalised in ----
    const u32x2 lw = __builtin_amdgcn_permlane32_swap(__float_as_uint(l), __float_as_uint(l), false, false);
    const float inv = 1.0f / (__uint_as_float(lw[0]) + __uint_as_float(lw[1]));
    f32x16 oacc[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.f;
      const int row = dt * 32 + li;
      const int swz = (row >> 1) & 7;
#pragma unroll
      for (int gk = 0; gk < NB; ++gk) {
        const char* rp = smem + (gk >> 1) * STAGE + KBYTES + row * 128;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const f16x8 vf = *reinterpret_cast<const f16x8*>(rp + ((((gk & 1) * 4 + hi * 2 + j) ^ swz) << 4));
          oacc[dt] = FMX_MFMA_32x32x16(vf, pf[gk][j], oacc[dt]);
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[dt][r] *= inv;
#pragma unroll
      for (int gk = 0; gk < NBX; ++gk) {
        const char* rp = xvs + row * 128;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const f16x8 vf = *reinterpret_cast<const f16x8*>(rp + (((gk * 4 + hi * 2 + j) ^ swz) << 4));
          oacc[dt] = FMX_MFMA_32x32x16(vf, xpf[gk][j], oacc[dt]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---- O: 16-byte pieces into the slot this tile's Q has left (row = query, chunk-swizzled), then whole lines out ----
    char* os = slots + slot * 4096;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int gq = 0; gq < 4; gq += 2) {
        union { f16x4 h4; unsigned u[2]; } lo, up;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          lo.h4[e] = (f16)oacc[dt][gq * 4 + e];
          up.h4[e] = (f16)oacc[dt][(gq + 1) * 4 + e];
        }
        const u32x2 x = __builtin_amdgcn_permlane32_swap(lo.u[0], up.u[0], false, false);
        const u32x2 y = __builtin_amdgcn_permlane32_swap(lo.u[1], up.u[1], false, false);
        const u32x4 v = {x[0], y[0], x[1], y[1]};
        const int chunk = dt * 4 + gq + hi;   // columns chunk * 8 .. + 7 of query li
        *reinterpret_cast<u32x4*>(os + li * 128 + (chunk8(li, chunk) << 4)) = v;
      }
    // (LDS operations of one wave execute in order: the reads below see the writes above)
    f16* obase = p.o + (long)b * p.o_bs + (long)h * DP;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = e * 8 + r8;
      const u32x4 v = *reinterpret_cast<const u32x4*>(os + row * 128 + (pc << 4));
      const int qg = tile * 128 + wave * 32 + row;
      if (qg < p.nq) *reinterpret_cast<u32x4*>(obase + (long)qg * p.o_rs + chunk8(row, pc) * 8) = v;
    }
    slot ^= 1;
  }
}

template <int NB, int NBX>
int launch_dual(const DualParams& p, int grid, hipStream_t st) {
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(attn_dual_kernel<NB, NBX>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, dual_lds(NBX));
  (void)attr;
  hipLaunchKernelGGL((attn_dual_kernel<NB, NBX>), dim3(grid), dim3(256), dual_lds(NBX), st, p);
  FMX_LAUNCH_CHECK("fmxi_attention_dual_f16");
  return FMX_OK;
}

template <int NBX>
int launch_dual_nb(const DualParams& p, int grid, hipStream_t st) {
  switch ((p.nk + 31) / 32) {   // 32-key blocks that hold text keys
    case 1: return launch_dual<1, NBX>(p, grid, st);
    case 2: return launch_dual<2, NBX>(p, grid, st);
    case 3: return launch_dual<3, NBX>(p, grid, st);
    default: return launch_dual<4, NBX>(p, grid, st);
  }
}

int device_cus() {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) return n;
    return 256;
  }();
  return cus;
}

}  // namespace

extern "C" int fmxi_attention_dual_f16(const fmxi_dual_attn_args* a, void* stream) {
  FMX_REQUIRE(a && a->q && a->k && a->vt && a->o && a->xk && a->xvt, "attention_dual: null pointer");
  FMX_REQUIRE(a->dpad == 64, "attention_dual: dpad %d (the kernel is built for heads of 64; other widths take the composite route)", a->dpad);
  FMX_REQUIRE(a->batch > 0 && a->heads > 0 && a->nq > 0, "attention_dual: bad dims");
  FMX_REQUIRE(a->nk >= 1 && a->nk <= 128, "attention_dual: nk %d not in 1..128", a->nk);
  FMX_REQUIRE(a->nk_pad >= a->nk && (a->nk_pad % 64) == 0, "attention_dual: nk_pad (%d) must be a multiple of 64 >= nk (%d)", a->nk_pad, a->nk);
  FMX_REQUIRE(a->images_per_group >= 1 && a->batch % a->images_per_group == 0, "attention_dual: batch %d is not a multiple of images_per_group %d",
              a->batch, a->images_per_group);
  FMX_REQUIRE(fmx_aligned16(a->q) && fmx_aligned16(a->k) && fmx_aligned16(a->vt) && fmx_aligned16(a->o) && fmx_aligned16(a->xk) &&
                  fmx_aligned16(a->xvt), "attention_dual: 16-byte alignment");
  FMX_REQUIRE((a->q_rs % 8) == 0 && (a->k_rs % 8) == 0 && (a->vt_ds % 8) == 0 && (a->o_rs % 4) == 0 && (a->q_bs % 8) == 0 &&
                  (a->k_bs % 8) == 0 && (a->vt_bs % 8) == 0 && (a->vt_hs % 8) == 0, "attention_dual: strides must be multiples of 8 elements");
  FMX_REQUIRE(a->q_rs > 0 && a->k_rs > 0 && a->vt_ds > 0 && a->o_rs > 0, "attention_dual: row strides must be positive");
  FMX_REQUIRE(a->scale > 0.f && isfinite(a->scale), "attention_dual: scale must be positive and finite");
  FMX_REQUIRE(a->nseg >= 1 && a->nseg <= FMXI_MAX_SEGMENTS, "attention_dual: nseg %d not in 1..%d", a->nseg, FMXI_MAX_SEGMENTS);
  const int32_t start[FMXI_MAX_SEGMENTS] = {a->seg_start0, a->seg_start1, a->seg_start2, a->seg_start3};
  const int32_t count[FMXI_MAX_SEGMENTS] = {a->seg_count0, a->seg_count1, a->seg_count2, a->seg_count3};
  const float weight[FMXI_MAX_SEGMENTS] = {a->seg_weight0, a->seg_weight1, a->seg_weight2, a->seg_weight3};

  DualParams p{};
  int top = 0;
  for (int s = 0; s < a->nseg; ++s) {
    FMX_REQUIRE(start[s] >= 0 && count[s] >= 1 && start[s] <= FMXI_EXTRA_KEYS - count[s] && count[s] <= FMXI_EXTRA_KEYS,
                "attention_dual: segment %d = keys [%d, %d + %d) does not lie inside [0, %d) with at least one key", s, start[s], start[s], count[s],
                FMXI_EXTRA_KEYS);
    FMX_REQUIRE(isfinite(weight[s]), "attention_dual: weight of segment %d is not finite", s);
    for (int t = 0; t < s; ++t)
      FMX_REQUIRE(start[s] >= start[t] + count[t] || start[t] >= start[s] + count[s], "attention_dual: segments %d and %d overlap", t, s);
    p.seg_lo[s] = start[s];
    p.seg_hi[s] = start[s] + count[s];
    p.seg_w[s] = weight[s];
    top = p.seg_hi[s] > top ? p.seg_hi[s] : top;
  }
  p.nseg = a->nseg;
  p.q = (const f16*)a->q; p.k = (const f16*)a->k; p.vt = (const f16*)a->vt; p.o = (f16*)a->o;
  p.xk = (const f16*)a->xk; p.xvt = (const f16*)a->xvt;
  p.q_bs = a->q_bs; p.q_rs = a->q_rs; p.k_bs = a->k_bs; p.k_rs = a->k_rs;
  p.vt_bs = a->vt_bs; p.vt_hs = a->vt_hs; p.vt_ds = a->vt_ds; p.o_bs = a->o_bs; p.o_rs = a->o_rs;
  p.batch = a->batch; p.heads = a->heads; p.nq = a->nq; p.nk = a->nk;
  p.images_per_group = a->images_per_group;
  p.groups = a->batch / a->images_per_group;
  p.scale_log2e = a->scale * 1.44269504088896340736f;
  p.qtiles = (a->nq + 127) / 128;
  // Q rows, K rows 0 .. nk_pad-1 and V^T rows 0 .. 63 with nk_pad keys each are addressed by 32-bit byte offsets from the (batch, head) bases,
  // bounded by buffer descriptors of exactly these spans
  const double q_span = ((double)(a->nq - 1) * a->q_rs + 64) * 2.0, k_span = ((double)(a->nk_pad - 1) * a->k_rs + 64) * 2.0,
               v_span = (63.0 * a->vt_ds + a->nk_pad) * 2.0, xv_span = (63.0 * p.groups * KVB + KVB) * 2.0;
  const long total = (long)a->batch * a->heads * p.qtiles;
  FMX_REQUIRE(q_span < 2.0e9 && k_span < 2.0e9 && v_span < 2.0e9 && xv_span < 2.0e9 && total < (1L << 30),
              "attention_dual: Q, K or V^T of one (batch, head) spans 2 GB or more, or there are 2^30 query tiles or more");
  p.q_span = (unsigned)q_span;
  p.k_span = (unsigned)k_span;
  p.vt_span = (unsigned)v_span;
  p.xk_span = (unsigned)(((double)(KVB - 1) * a->heads * 64 + 64) * 2.0);
  p.xvt_span = (unsigned)xv_span;
  const int cus = device_cus();
  const int grid = (int)(total < 2 * cus ? total : 2 * cus);   // persistent: two workgroups per CU, all resident
  hipStream_t st = (hipStream_t)stream;
  return top <= 32 ? launch_dual_nb<1>(p, grid, st) : launch_dual_nb<2>(p, grid, st);
}
