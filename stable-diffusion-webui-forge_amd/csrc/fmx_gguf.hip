// GGUF block dequantisation on the device (gfx950): packed GGML blocks -> fp16 / bf16 weights, once, at load time.
//
// Contract (include/fmx.h): the value of a weight is what ggml defines in fp32 (the numpy `dequantize_blocks` of the reference's
// packages_3rdparty/gguf/quants.py), rounded ONCE, to nearest-even, to the output type.  The expressions below keep numpy's operation order
// and the file is compiled with floating-point contraction off, so the fp32 value is the same IEEE expression tree as numpy's; for every
// supported type all products are exact in fp32 and at most one addition rounds, so contraction could not change a bit anyway.
//
// Shape: a pure stream (0.33-1.06 bytes in, 2 bytes out per weight, no reuse).  Block sizes (18 .. 210 bytes) are never multiples of 16, so
// a workgroup fetches the 16-byte aligned span that covers its chunk of 8192 weights with 16-byte loads into registers, parks it in LDS
// (at the span's own misalignment, so block offsets stay what they are in memory) and decodes from there; every lane produces 8 consecutive
// weights per store, i.e. one 16-byte store, consecutive lanes consecutive addresses.  The loads of the next chunk are issued before the
// current one is decoded and only waited for when they are written to LDS.  The first and last 16-byte vector of a tensor may straddle its
// bounds: those two are read with guarded 2-byte loads, nothing outside [blocks, blocks + bytes) is ever touched.
#include "fmx_common.hpp"

#pragma clang fp contract(off)

namespace {

enum : int { T_F32 = 0, T_F16 = 1, T_Q4_0 = 2, T_Q4_1 = 3, T_Q5_0 = 6, T_Q5_1 = 7, T_Q8_0 = 8, T_Q2_K = 10, T_Q3_K = 11, T_Q4_K = 12,
             T_Q5_K = 13, T_Q6_K = 14, T_BF16 = 30 };

constexpr int block_weights(int qt) { return qt == T_F32 || qt == T_F16 || qt == T_BF16 ? 1 : (qt >= T_Q2_K && qt <= T_Q6_K ? 256 : 32); }
constexpr int block_bytes(int qt) {
  return qt == T_F32 ? 4 : qt == T_F16 || qt == T_BF16 ? 2 : qt == T_Q4_0 ? 18 : qt == T_Q4_1 ? 20 : qt == T_Q5_0 ? 22 : qt == T_Q5_1 ? 24
       : qt == T_Q8_0 ? 34 : qt == T_Q2_K ? 84 : qt == T_Q3_K ? 110 : qt == T_Q4_K ? 144 : qt == T_Q5_K ? 176 : qt == T_Q6_K ? 210 : 0;
}

constexpr int TPB = 256;
constexpr int CHUNK = 8192;               // weights per workgroup iteration: 4 stores of 8 weights per lane
constexpr int STORES = CHUNK / (TPB * 8);
constexpr int MAX_GRID = 256 * 8;         // 256 CUs x 8 resident workgroups of 4 waves

typedef unsigned short u16;
typedef u16 u16x8 __attribute__((ext_vector_type(8)));

__host__ __device__ __forceinline__ float half_bits_to_float(unsigned bits) { return (float)__builtin_bit_cast(_Float16, (u16)bits); }
__host__ __device__ __forceinline__ float bf16_bits_to_float(unsigned bits) { return __builtin_bit_cast(float, bits << 16); }

// one rounding, to nearest even, as numpy's / torch's conversions do (fp16: the hardware conversion; bf16: the integer form, NaN kept quiet)
template <typename OutT> __host__ __device__ __forceinline__ u16 round_to(float v);
template <> __host__ __device__ __forceinline__ u16 round_to<_Float16>(float v) { return __builtin_bit_cast(u16, (_Float16)v); }
template <> __host__ __device__ __forceinline__ u16 round_to<__bf16>(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u16)((u >> 16) | 0x40u);
  return (u16)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// LDS block accessors.  A block starts at an even byte offset (the tensor is 2-byte aligned and every block size is even), so 16-bit reads
// at even offsets are aligned; nothing wider is.
__host__ __device__ __forceinline__ unsigned ld8(const unsigned char* b, int off) { return b[off]; }
__host__ __device__ __forceinline__ unsigned ld16(const unsigned char* b, int off) { return *reinterpret_cast<const u16*>(b + off); }
__host__ __device__ __forceinline__ unsigned ld32(const unsigned char* b, int off) { return ld16(b, off) | (ld16(b, off + 2) << 16); }
__host__ __device__ __forceinline__ void ld8bytes(const unsigned char* b, int off, unsigned (&q)[8]) {  // off even
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned w = ld16(b, off + 2 * i);
    q[2 * i] = w & 0xffu;
    q[2 * i + 1] = w >> 8;
  }
}

// the 6-bit (scale, min) pairs of Q4_K / Q5_K: 12 bytes at `off`, entry g of 8
__host__ __device__ __forceinline__ void k_scale_min(const unsigned char* b, int off, int g, unsigned& sc, unsigned& mn) {
  if (g < 4) {
    sc = ld8(b, off + g) & 0x3fu;
    mn = ld8(b, off + 4 + g) & 0x3fu;
  } else {
    const unsigned md = ld8(b, off + 4 + g);  // bytes 8..11
    sc = (md & 0x0fu) | ((ld8(b, off + g - 4) >> 2) & 0x30u);
    mn = (md >> 4) | ((ld8(b, off + g) >> 2) & 0x30u);
  }
}

// weights j .. j+7 (j a multiple of 8) of the block at `b`, in fp32, in numpy's operation order
template <int QT> __host__ __device__ __forceinline__ void decode8(const unsigned char* b, int j, float (&v)[8]) {
  unsigned q[8];
  if constexpr (QT == T_Q8_0) {
    const float d = half_bits_to_float(ld16(b, 0));
    ld8bytes(b, 2 + j, q);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)(int)(signed char)q[i] * d;
  } else if constexpr (QT == T_Q4_0 || QT == T_Q4_1) {
    constexpr int QS = QT == T_Q4_0 ? 2 : 4;
    const float d = half_bits_to_float(ld16(b, 0));
    ld8bytes(b, QS + (j & 15), q);
    const int sh = (j >> 4) * 4;
    if constexpr (QT == T_Q4_0) {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = d * (float)((int)((q[i] >> sh) & 15u) - 8);
    } else {
      const float m = half_bits_to_float(ld16(b, 2));
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = d * (float)((q[i] >> sh) & 15u) + m;
    }
  } else if constexpr (QT == T_Q5_0 || QT == T_Q5_1) {
    constexpr int QH = QT == T_Q5_0 ? 2 : 4;
    const float d = half_bits_to_float(ld16(b, 0));
    const unsigned qh = ld32(b, QH) >> j;
    ld8bytes(b, QH + 4 + (j & 15), q);
    const int sh = (j >> 4) * 4;
    if constexpr (QT == T_Q5_0) {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = d * (float)((int)(((q[i] >> sh) & 15u) | (((qh >> i) & 1u) << 4)) - 16);
    } else {
      const float m = half_bits_to_float(ld16(b, 2));
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = d * (float)(((q[i] >> sh) & 15u) | (((qh >> i) & 1u) << 4)) + m;
    }
  } else if constexpr (QT == T_Q2_K) {  // scales[16] qs[64] d dmin
    const unsigned s = ld8(b, j >> 4);
    const float dl = half_bits_to_float(ld16(b, 80)) * (float)(s & 15u);
    const float ml = half_bits_to_float(ld16(b, 82)) * (float)(s >> 4);
    ld8bytes(b, 16 + (j >> 7) * 32 + (j & 31), q);
    const int sh = ((j >> 5) & 3) * 2;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = dl * (float)((q[i] >> sh) & 3u) - ml;
  } else if constexpr (QT == T_Q3_K) {  // hmask[32] qs[64] scales[12] d
    const int g = j >> 4;               // 6-bit scale g of 16: low nibbles in bytes 0..7, 2-bit tops in bytes 8..11
    const unsigned lo = (ld8(b, 96 + (g & 7)) >> ((g >> 3) * 4)) & 15u;
    const unsigned hi = (ld8(b, 104 + (g & 3)) >> ((g >> 2) * 2)) & 3u;
    const float dl = half_bits_to_float(ld16(b, 108)) * (float)((int)(signed char)(lo | (hi << 4)) - 32);
    unsigned h[8];
    ld8bytes(b, 32 + (j >> 7) * 32 + (j & 31), q);
    ld8bytes(b, j & 31, h);
    const int sh = ((j >> 5) & 3) * 2, bit = j >> 5;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = dl * (float)((int)((q[i] >> sh) & 3u) - (int)((((h[i] >> bit) & 1u) ^ 1u) << 2));
  } else if constexpr (QT == T_Q4_K || QT == T_Q5_K) {  // d dmin scales[12] (qh[32]) qs[128]
    unsigned sc, mn;
    k_scale_min(b, 4, j >> 5, sc, mn);
    const float d = half_bits_to_float(ld16(b, 0)) * (float)sc;
    const float dm = half_bits_to_float(ld16(b, 2)) * (float)mn;
    constexpr int QS = QT == T_Q4_K ? 16 : 48;
    ld8bytes(b, QS + (j >> 6) * 32 + (j & 31), q);
    const int sh = ((j >> 5) & 1) * 4;
    if constexpr (QT == T_Q4_K) {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = d * (float)((q[i] >> sh) & 15u) - dm;
    } else {
      unsigned h[8];
      ld8bytes(b, 16 + (j & 31), h);
      const int bit = j >> 5;
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = d * (float)(((q[i] >> sh) & 15u) | (((h[i] >> bit) & 1u) << 4)) - dm;
    }
  } else if constexpr (QT == T_Q6_K) {  // ql[128] qh[64] scales[16] d
    const float d = half_bits_to_float(ld16(b, 208)) * (float)(int)(signed char)ld8(b, 192 + (j >> 4));
    unsigned h[8];
    const int half = j >> 7, r = j & 127;
    ld8bytes(b, half * 64 + (r & 63), q);
    ld8bytes(b, 128 + half * 32 + (r & 31), h);
    const int shl = (r >> 6) * 4, shh = (r >> 5) * 2;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = d * (float)((int)(signed char)(((q[i] >> shl) & 15u) | (((h[i] >> shh) & 3u) << 4)) - 32);
  }
}

template <int QT, typename OutT>
__global__ __launch_bounds__(TPB) void gguf_dequant_kernel(const unsigned char* __restrict__ blocks, u16* __restrict__ out, long long n_elements) {
  constexpr int BW = block_weights(QT), BB = block_bytes(QT);
  constexpr int CBYTES = CHUNK / BW * BB;          // packed bytes of a full chunk
  constexpr int NVEC = (CBYTES + 14 + 15) / 16;    // 16-byte vectors that cover it at the worst (even) misalignment
  constexpr int VPT = (NVEC + TPB - 1) / TPB;
  __shared__ uint4 span[NVEC];

  const uintptr_t begin = reinterpret_cast<uintptr_t>(blocks);
  const long long total_bytes = n_elements / BW * BB;
  const uintptr_t end = begin + (uintptr_t)total_bytes;
  const long long nchunks = (n_elements + CHUNK - 1) / CHUNK;
  const int tid = threadIdx.x;

  uint4 regs[VPT];
  auto fetch = [&](long long c) {
    const uintptr_t g0 = begin + (uintptr_t)(c * (long long)CBYTES);
    const uintptr_t ga = g0 & ~(uintptr_t)15;
    const long long left = total_bytes - c * (long long)CBYTES;
    const int nbytes = left < CBYTES ? (int)left : CBYTES;
    const int nvec = ((int)(g0 - ga) + nbytes + 15) >> 4;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      const int vi = tid + i * TPB;
      if (vi < nvec) {
        const uintptr_t a = ga + (uintptr_t)vi * 16;
        if (a >= begin && a + 16 <= end) {
          regs[i] = *reinterpret_cast<const uint4*>(a);
        } else {  // the tensor's first / last vector: only the 2-byte words inside it
          u16x8 w;
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const uintptr_t p = a + 2 * k;
            w[k] = (p >= begin && p + 2 <= end) ? *reinterpret_cast<const u16*>(p) : (u16)0;
          }
          regs[i] = __builtin_bit_cast(uint4, w);
        }
      } else {
        regs[i] = uint4{0u, 0u, 0u, 0u};
      }
    }
  };

  long long c = blockIdx.x;
  if (c < nchunks) fetch(c);
  for (; c < nchunks; c += gridDim.x) {
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      const int vi = tid + i * TPB;
      if (vi < NVEC) span[vi] = regs[i];
    }
    __syncthreads();
    if (c + gridDim.x < nchunks) fetch(c + gridDim.x);
    const int mis = (int)((begin + (uintptr_t)(c * (long long)CBYTES)) & 15);
    const unsigned char* base = reinterpret_cast<const unsigned char*>(span) + mis;
#pragma unroll
    for (int s = 0; s < STORES; ++s) {
      const int w = (s * TPB + tid) * 8;
      const long long e = c * (long long)CHUNK + w;
      if (e < n_elements) {
        float v[8];
        decode8<QT>(base + (w / BW) * BB, w % BW, v);
        u16x8 o;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = round_to<OutT>(v[i]);
        *reinterpret_cast<u16x8*>(out + e) = o;
      }
    }
    __syncthreads();
  }
}

// F32 / F16 / BF16 tensors (norm scales, biases, unquantised matrices): a cast.  A 16-byte aligned source (every tensor of a GGUF file is: the
// data section is aligned to general.alignment >= 32) goes 8 elements per lane with 16-byte loads and stores; any other 2-byte aligned source,
// and the last n % 8 elements, are read in 16-bit words.
template <int QT> __host__ __device__ __forceinline__ float cast_one(const u16* __restrict__ src, long long i) {
  if constexpr (QT == T_F32) return __builtin_bit_cast(float, (unsigned)src[2 * i] | ((unsigned)src[2 * i + 1] << 16));
  else if constexpr (QT == T_F16) return half_bits_to_float(src[i]);
  else return bf16_bits_to_float(src[i]);
}

template <int QT, typename OutT, bool VEC>
__global__ __launch_bounds__(TPB) void gguf_cast_kernel(const u16* __restrict__ src, u16* __restrict__ out, long long n) {
  const long long stride = (long long)gridDim.x * TPB, t0 = (long long)blockIdx.x * TPB + threadIdx.x;
  const long long n8 = VEC ? n / 8 : 0;
  if constexpr (VEC) {
    for (long long i = t0; i < n8; i += stride) {
      u16x8 o;
      if constexpr (QT == T_F32) {
        const f32x4 a = reinterpret_cast<const f32x4*>(src)[2 * i], b = reinterpret_cast<const f32x4*>(src)[2 * i + 1];
#pragma unroll
        for (int k = 0; k < 4; ++k) { o[k] = round_to<OutT>(a[k]); o[4 + k] = round_to<OutT>(b[k]); }
      } else {
        const u16x8 a = reinterpret_cast<const u16x8*>(src)[i];
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = round_to<OutT>(QT == T_F16 ? half_bits_to_float(a[k]) : bf16_bits_to_float(a[k]));
      }
      reinterpret_cast<u16x8*>(out)[i] = o;
    }
  }
  for (long long i = n8 * 8 + t0; i < n; i += stride) out[i] = round_to<OutT>(cast_one<QT>(src, i));
}

template <int QT, typename OutT> int launch_blocks(const void* blocks, void* out, long long n, hipStream_t stream) {
  const long long nchunks = (n + CHUNK - 1) / CHUNK;
  const unsigned grid = (unsigned)(nchunks < MAX_GRID ? nchunks : MAX_GRID);
  hipLaunchKernelGGL((gguf_dequant_kernel<QT, OutT>), dim3(grid), dim3(TPB), 0, stream, (const unsigned char*)blocks, (u16*)out, n);
  return 0;
}

template <int QT, typename OutT> int launch_cast(const void* blocks, void* out, long long n, hipStream_t stream) {
  const bool vec = fmx_aligned16(blocks);
  const long long nb = ((vec ? (n + 7) / 8 : n) + TPB - 1) / TPB;
  const unsigned grid = (unsigned)(nb < MAX_GRID * 4 ? nb : MAX_GRID * 4);
  if (vec) hipLaunchKernelGGL((gguf_cast_kernel<QT, OutT, true>), dim3(grid), dim3(TPB), 0, stream, (const u16*)blocks, (u16*)out, n);
  else hipLaunchKernelGGL((gguf_cast_kernel<QT, OutT, false>), dim3(grid), dim3(TPB), 0, stream, (const u16*)blocks, (u16*)out, n);
  return 0;
}

template <typename OutT> int dequant(const char* name, int qtype, const void* blocks, void* out, long long n, void* stream) {
  FMX_REQUIRE(blocks && out, "%s: null pointer", name);
  FMX_REQUIRE(n > 0, "%s: n_elements %lld must be positive", name, n);
  const int bw = block_bytes(qtype) ? block_weights(qtype) : 0;
  if (bw == 0) return fmx_set_error(FMX_E_UNSUPPORTED, "%s: GGML type %d is not supported (F32, F16, BF16, Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q2_K .. Q6_K are)", name, qtype);
  FMX_REQUIRE(n % bw == 0, "%s: n_elements %lld is not a multiple of the block size %d of GGML type %d", name, n, bw, qtype);
  FMX_REQUIRE((reinterpret_cast<uintptr_t>(blocks) & 1u) == 0, "%s: blocks must be 2-byte aligned", name);
  FMX_REQUIRE(fmx_aligned16(out), "%s: out must be 16-byte aligned", name);
  hipStream_t st = (hipStream_t)stream;
  switch (qtype) {
    case T_F32: launch_cast<T_F32, OutT>(blocks, out, n, st); break;
    case T_F16: launch_cast<T_F16, OutT>(blocks, out, n, st); break;
    case T_BF16: launch_cast<T_BF16, OutT>(blocks, out, n, st); break;
    case T_Q4_0: launch_blocks<T_Q4_0, OutT>(blocks, out, n, st); break;
    case T_Q4_1: launch_blocks<T_Q4_1, OutT>(blocks, out, n, st); break;
    case T_Q5_0: launch_blocks<T_Q5_0, OutT>(blocks, out, n, st); break;
    case T_Q5_1: launch_blocks<T_Q5_1, OutT>(blocks, out, n, st); break;
    case T_Q8_0: launch_blocks<T_Q8_0, OutT>(blocks, out, n, st); break;
    case T_Q2_K: launch_blocks<T_Q2_K, OutT>(blocks, out, n, st); break;
    case T_Q3_K: launch_blocks<T_Q3_K, OutT>(blocks, out, n, st); break;
    case T_Q4_K: launch_blocks<T_Q4_K, OutT>(blocks, out, n, st); break;
    case T_Q5_K: launch_blocks<T_Q5_K, OutT>(blocks, out, n, st); break;
    case T_Q6_K: launch_blocks<T_Q6_K, OutT>(blocks, out, n, st); break;
    default: return fmx_set_error(FMX_E_UNSUPPORTED, "%s: GGML type %d is not supported", name, qtype);
  }
  FMX_LAUNCH_CHECK(name);
  return FMX_OK;
}

}  // namespace

extern "C" int fmx_gguf_dequant_f16(int32_t qtype, const void* blocks, void* out, int64_t n_elements, void* stream) {
  return dequant<_Float16>("fmx_gguf_dequant_f16", qtype, blocks, out, (long long)n_elements, stream);
}

extern "C" int fmx_gguf_dequant_bf16(int32_t qtype, const void* blocks, void* out, int64_t n_elements, void* stream) {
  return dequant<__bf16>("fmx_gguf_dequant_bf16", qtype, blocks, out, (long long)n_elements, stream);
}
