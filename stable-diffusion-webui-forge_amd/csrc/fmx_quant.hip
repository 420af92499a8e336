// Storage-quantised checkpoints on the device (gfx950): float8 (e4m3fn / e5m2) and bitsandbytes 4-bit (NF4 / FP4) weights -> fp16 / bf16 weights,
// once, at load time.  The resident weights, the GEMMs and the captured step never learn that the file was quantised (include/fmx.h).
//
// Contract.  fp8: the value of a code is what the OCP formats define; all 256 codes of both kinds are exactly representable in fp16 and in
// bf16, so no rounding happens.  NaN codes become a quiet NaN, infinities (e5m2) and signed zeros are kept.  Decoded with bit arithmetic into a
// 256-entry table, never with a hardware fp8 conversion.  bnb4: weight i is nibble (i & 1 ? low : high) of byte i >> 1; its value is
// code16[nibble] * s in ONE fp32 multiply, rounded once, to nearest even, to the output type; s is absmax_f32[i / blocksize], or, nested,
// code256[absmax_u8[i / blocksize]] * absmax2[(i / blocksize) / blocksize2] + offset -- one fp32 multiply, then one fp32 add, each rounded, which
// is why the file is compiled with floating-point contraction off.  The tables are the file's own: no NF4 / FP4 constant lives here.
//
// Shape: pure streams (fp8: 1 byte in, 2 out per weight; bnb4: 0.5 in + the block scales, 2 out).  As in fmx_gguf.hip a workgroup walks chunks
// of 8192 weights, every lane produces 8 consecutive weights per 16-byte store, consecutive lanes consecutive addresses, the grid is capped
// and the rest is grid-strided; all element indices are 64-bit.  A lane's 8 weights start at a multiple of 8 and every block size is a
// multiple of 64, so they never straddle a quantisation block: one scale per store.  The loads of a chunk (8 or 4 bytes per store) are all issued
// before the first is decoded.  Only the tensor's last, partial group of 8 is read and written element by element: nothing outside
// [src, src + bytes) and [out, out + n) is touched.
#include "fmx_common.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int VEC = 8;                     // weights per lane per store: one 16-byte store
constexpr int CHUNK = 8192;                // weights per workgroup iteration: 4 stores per lane
constexpr int STORES = CHUNK / (TPB * VEC);
constexpr int MAX_GRID = 256 * 8;          // 256 CUs x 8 resident workgroups of 4 waves
constexpr int MIN_BLOCK = 64, MAX_BLOCK = 4096;
static_assert(MIN_BLOCK % VEC == 0, "a lane's 8 weights must lie inside one quantisation block");
static_assert(TPB == 256, "one thread fills one entry of the 256-entry tables");

typedef unsigned short u16;
typedef u16 u16x8 __attribute__((ext_vector_type(8)));

// one rounding, to nearest even (fp16: the hardware conversion; bf16: the integer form, NaN kept quiet): as fmx_gguf.hip
template <typename OutT> __host__ __device__ __forceinline__ u16 round_to(float v);
template <> __host__ __device__ __forceinline__ u16 round_to<_Float16>(float v) { return __builtin_bit_cast(u16, (_Float16)v); }
template <> __host__ __device__ __forceinline__ u16 round_to<__bf16>(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const unsigned rounded = (u + 0x7fffu + ((u >> 16) & 1u)) >> 16, quiet = (u >> 16) | 0x40u;
  return (u16)((u & 0x7fffffffu) > 0x7f800000u ? quiet : rounded);   // a select, not a branch: eight of these per store
}

// code * scale as ONE fp32 multiply whose result exists in a register before it is converted.  Without the barrier the compiler folds
// (_Float16)(a * b) into v_fma_mixlo_f16 a, b, +0, and -0 + +0 is +0: a zero scale would lose the sign torch's cast keeps.
__device__ __forceinline__ float mul_f32(float a, float b) {
  float p = a * b;
  asm volatile("" : "+v"(p));
  return p;
}

// the fp32 value of an fp8 code, by bit arithmetic.  E = exponent bits, M = mantissa bits (4, 3: e4m3fn, bias 7; 5, 2: e5m2, bias 15)
template <int E, int M> __host__ __device__ __forceinline__ float fp8_value(unsigned code) {
  constexpr int BIAS = (1 << (E - 1)) - 1;
  const unsigned sign = (code & 0x80u) << 24, e = (code >> M) & ((1u << E) - 1u), m = code & ((1u << M) - 1u);
  unsigned bits;
  if (E == 4 ? (e == 15u && m == 7u) : (e == 31u && m != 0u)) bits = 0x7fc00000u;                 // NaN -> quiet NaN
  else if (E == 5 && e == 31u) bits = 0x7f800000u;                                                 // e5m2 infinity
  else if (e == 0u) return __builtin_bit_cast(float, sign | __builtin_bit_cast(unsigned, (float)m * (1.0f / (float)(1 << (BIAS - 1 + M)))));  // subnormal, +-0
  else bits = ((e + 127u - BIAS) << 23) | (m << (23 - M));
  return __builtin_bit_cast(float, sign | bits);
}

template <typename OutT>
__global__ __launch_bounds__(TPB) void fp8_expand_kernel(int kind, const unsigned char* __restrict__ src, u16* __restrict__ out, long long n) {
  __shared__ u16 table[256];
  table[threadIdx.x] = round_to<OutT>(kind == 0 ? fp8_value<4, 3>(threadIdx.x) : fp8_value<5, 2>(threadIdx.x));   // exact: nothing rounds
  __syncthreads();
  const long long nchunks = (n + CHUNK - 1) / CHUNK;
  for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {
    uint2 raw[STORES];
#pragma unroll
    for (int s = 0; s < STORES; ++s) {
      const long long e = c * (long long)CHUNK + (long long)(s * TPB + (int)threadIdx.x) * VEC;
      raw[s] = e + VEC <= n ? *reinterpret_cast<const uint2*>(src + e) : uint2{0u, 0u};
    }
#pragma unroll
    for (int s = 0; s < STORES; ++s) {
      const long long e = c * (long long)CHUNK + (long long)(s * TPB + (int)threadIdx.x) * VEC;
      if (e + VEC <= n) {
        u16x8 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          o[i] = table[(raw[s].x >> (8 * i)) & 0xffu];
          o[4 + i] = table[(raw[s].y >> (8 * i)) & 0xffu];
        }
        *reinterpret_cast<u16x8*>(out + e) = o;
      } else {
        for (long long i = e; i < n; ++i) out[i] = table[src[i]];      // the tensor's last n % 8 weights
      }
    }
  }
}

struct Bnb4Args {
  const unsigned char* packed;
  const float* code16;
  const float* absmax_f32;       // flat, else null
  const unsigned char* absmax_u8;  // nested, else null
  const float* code256;
  const float* absmax2;
  float offset;
  int shift, shift2;             // log2 of blocksize, blocksize2
  u16* out;
  long long n;
};

template <typename OutT, bool NESTED>
__global__ __launch_bounds__(TPB) void bnb4_dequant_kernel(Bnb4Args a) {
  __shared__ float code16[16];
  __shared__ float code256[NESTED ? 256 : 1];
  if (threadIdx.x < 16) code16[threadIdx.x] = a.code16[threadIdx.x];
  if constexpr (NESTED) code256[threadIdx.x] = a.code256[threadIdx.x];
  __syncthreads();
  const long long n = a.n, nbytes = (n + 1) >> 1;
  const long long nchunks = (n + CHUNK - 1) / CHUNK;
  for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {
    unsigned raw[STORES];
    float scale[STORES];
#pragma unroll
    for (int s = 0; s < STORES; ++s) {
      const long long e = c * (long long)CHUNK + (long long)(s * TPB + (int)threadIdx.x) * VEC;
      raw[s] = 0u;
      scale[s] = 0.0f;
      if (e < n) {
        if (e + VEC <= n) {
          raw[s] = *reinterpret_cast<const unsigned*>(a.packed + (e >> 1));
        } else {  // the tensor's last, partial group: only the bytes that exist
          for (int k = 0; k < 4; ++k)
            if ((e >> 1) + k < nbytes) raw[s] |= (unsigned)a.packed[(e >> 1) + k] << (8 * k);
        }
        const long long b = e >> a.shift;
        if constexpr (NESTED) scale[s] = code256[a.absmax_u8[b]] * a.absmax2[b >> a.shift2] + a.offset;   // multiply, then add: each rounded
        else scale[s] = a.absmax_f32[b];
      }
    }
#pragma unroll
    for (int s = 0; s < STORES; ++s) {
      const long long e = c * (long long)CHUNK + (long long)(s * TPB + (int)threadIdx.x) * VEC;
      if (e >= n) continue;
      u16x8 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned byte = (raw[s] >> (8 * k)) & 0xffu;
        o[2 * k] = round_to<OutT>(mul_f32(code16[byte >> 4], scale[s]));        // even weight: the high nibble
        o[2 * k + 1] = round_to<OutT>(mul_f32(code16[byte & 15u], scale[s]));   // odd weight: the low nibble
      }
      if (e + VEC <= n) {
        *reinterpret_cast<u16x8*>(a.out + e) = o;
      } else {
        for (int i = 0; i < VEC; ++i)
          if (e + i < n) a.out[e + i] = o[i];
      }
    }
  }
}

unsigned grid_for(long long n) {
  const long long nchunks = (n + CHUNK - 1) / CHUNK;
  return (unsigned)(nchunks < MAX_GRID ? nchunks : MAX_GRID);
}

template <typename OutT> int fp8_expand(const char* name, int kind, const void* src, void* out, long long n, void* stream) {
  FMX_REQUIRE(src && out, "%s: null pointer", name);
  FMX_REQUIRE(n > 0, "%s: n %lld must be positive", name, n);
  if (kind != 0 && kind != 1)
    return fmx_set_error(FMX_E_UNSUPPORTED, "%s: kind %d is not supported (0: float8_e4m3fn, 1: float8_e5m2; the fnuz variants are not accepted)", name, kind);
  FMX_REQUIRE((reinterpret_cast<uintptr_t>(src) & 7u) == 0, "%s: src must be 8-byte aligned", name);
  FMX_REQUIRE(fmx_aligned16(out), "%s: out must be 16-byte aligned", name);
  hipLaunchKernelGGL((fp8_expand_kernel<OutT>), dim3(grid_for(n)), dim3(TPB), 0, (hipStream_t)stream, kind, (const unsigned char*)src, (u16*)out, n);
  FMX_LAUNCH_CHECK(name);
  return FMX_OK;
}

int log2_pow2(int v, int lo, int hi) {  // -> log2(v) when v is a power of two in [lo, hi], else -1
  if (v < lo || v > hi || (v & (v - 1)) != 0) return -1;
  int s = 0;
  while ((1 << s) < v) ++s;
  return s;
}

template <typename OutT>
int bnb4_dequant(const char* name, const void* packed, const float* code16, const float* absmax_f32, const uint8_t* absmax_u8, const float* code256,
                 const float* absmax2, float offset, int blocksize2, int blocksize, void* out, long long n, void* stream) {
  FMX_REQUIRE(packed && code16 && out, "%s: null pointer (packed, code16 and out are required)", name);
  FMX_REQUIRE(n > 0, "%s: n %lld must be positive", name, n);
  FMX_REQUIRE((absmax_f32 != nullptr) != (absmax_u8 != nullptr), "%s: exactly one of absmax_f32 (flat) and absmax_u8 (nested) must be given", name);
  const int shift = log2_pow2(blocksize, MIN_BLOCK, MAX_BLOCK);
  FMX_REQUIRE(shift >= 0, "%s: blocksize %d must be a power of two from %d to %d", name, blocksize, MIN_BLOCK, MAX_BLOCK);
  int shift2 = 0;
  if (absmax_u8) {
    FMX_REQUIRE(code256 && absmax2, "%s: nested absmax needs code256 and absmax2", name);
    shift2 = log2_pow2(blocksize2, MIN_BLOCK, 1 << 30);
    FMX_REQUIRE(shift2 >= 0, "%s: blocksize2 %d must be a power of two of at least %d", name, blocksize2, MIN_BLOCK);
  }
  FMX_REQUIRE(fmx_aligned16(packed), "%s: packed must be 16-byte aligned", name);
  FMX_REQUIRE(fmx_aligned16(out), "%s: out must be 16-byte aligned", name);
  const Bnb4Args a{(const unsigned char*)packed, code16, absmax_f32, absmax_u8, code256, absmax2, offset, shift, shift2, (u16*)out, n};
  if (absmax_u8) hipLaunchKernelGGL((bnb4_dequant_kernel<OutT, true>), dim3(grid_for(n)), dim3(TPB), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((bnb4_dequant_kernel<OutT, false>), dim3(grid_for(n)), dim3(TPB), 0, (hipStream_t)stream, a);
  FMX_LAUNCH_CHECK(name);
  return FMX_OK;
}

}  // namespace

extern "C" int fmx_fp8_expand_f16(int32_t kind, const void* src, void* out, int64_t n, void* stream) {
  return fp8_expand<_Float16>("fmx_fp8_expand_f16", kind, src, out, (long long)n, stream);
}

extern "C" int fmx_fp8_expand_bf16(int32_t kind, const void* src, void* out, int64_t n, void* stream) {
  return fp8_expand<__bf16>("fmx_fp8_expand_bf16", kind, src, out, (long long)n, stream);
}

extern "C" int fmx_bnb4_dequant_f16(const void* packed, const float* code16, const float* absmax_f32, const uint8_t* absmax_u8, const float* code256,
                                    const float* absmax2, float offset, int32_t blocksize2, int32_t blocksize, void* out, int64_t n, void* stream) {
  return bnb4_dequant<_Float16>("fmx_bnb4_dequant_f16", packed, code16, absmax_f32, absmax_u8, code256, absmax2, offset, blocksize2, blocksize, out,
                                (long long)n, stream);
}

extern "C" int fmx_bnb4_dequant_bf16(const void* packed, const float* code16, const float* absmax_f32, const uint8_t* absmax_u8, const float* code256,
                                     const float* absmax2, float offset, int32_t blocksize2, int32_t blocksize, void* out, int64_t n, void* stream) {
  return bnb4_dequant<__bf16>("fmx_bnb4_dequant_bf16", packed, code16, absmax_f32, absmax_u8, code256, absmax2, offset, blocksize2, blocksize, out,
                              (long long)n, stream);
}
