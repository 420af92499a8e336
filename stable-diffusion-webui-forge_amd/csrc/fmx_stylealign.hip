// The blend of StyleAlign's two self-attention outputs (include/fmx_ext.h, section "StyleAlign"): the reference computes
//   (1.0 - strength) * original_attention + strength * aligned_attention_result
// on fp16 tensors with Python float scalars, i.e. two fp16 products and one fp16 sum, each evaluated in fp32 and rounded to fp16.  This kernel makes
// the same three roundings in the same places, so the result carries the reference expression's bits:
//   out = h( f(h(f(own) * w_own)) + f(h(f(shared) * w_shared)) )
// The multiplies and the add are spelled with the _rn intrinsics: a contraction into an FMA would skip the rounding of a product.
// Memory bound: 16-byte loads and stores (8 elements per lane), a grid capped at 8 workgroups per CU that strides over the rest, no LDS.  Every lane
// reads its 8 elements of both inputs before it writes them, and no other lane touches them: out may alias own or shared.
#include <hip/hip_fp16.h>

#include "fmx_common.hpp"
#include "fmx_ext.h"

namespace {

constexpr int TPB = 256;
constexpr int BLOCKS_PER_CU = 8;

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));

// The fp32 product has to exist as an fp32 value before it is rounded to fp16: left alone, the compiler folds multiply and conversion into
// v_fma_mixlo_f16, which rounds the exact product ONCE (measured: own 0.89111328125 at strength 0.3, where the product lies 1e-8 below an fp16
// midpoint, fp32 rounding lands on the midpoint and the reference's second rounding goes to even).  The empty asm pins the product in a VGPR.
__device__ inline _Float16 blend1(_Float16 a, _Float16 b, float wa, float wb) {
  float fa = __fmul_rn((float)a, wa);
  float fb = __fmul_rn((float)b, wb);
  asm volatile("" : "+v"(fa), "+v"(fb));
  const _Float16 pa = (_Float16)fa;
  const _Float16 pb = (_Float16)fb;
  return (_Float16)__fadd_rn((float)pa, (float)pb);
}

// own / shared / out are not __restrict__: out may be one of the inputs
__global__ __launch_bounds__(TPB) void attn_blend_kernel(const _Float16* own, const _Float16* shared, _Float16* out, float w_own, float w_shared, long n) {
  const long nvec = n >> 3;
  const long stride = (long)gridDim.x * TPB;
  for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < nvec; i += stride) {
    const h16x8 a = reinterpret_cast<const h16x8*>(own)[i];
    const h16x8 b = reinterpret_cast<const h16x8*>(shared)[i];
    h16x8 r;
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = blend1(a[k], b[k], w_own, w_shared);
    reinterpret_cast<h16x8*>(out)[i] = r;
  }
  // the last partial vector: n % 8 elements, one lane each
  const long tail = nvec << 3;
  if (blockIdx.x == 0 && tail + threadIdx.x < n) {
    const long i = tail + threadIdx.x;
    out[i] = blend1(own[i], shared[i], w_own, w_shared);
  }
}

// the grid's ceiling: BLOCKS_PER_CU workgroups per CU of the current device (the count is read once).  0: the CU count cannot be read.
long max_blocks() {
  static int cus = 0;
  if (!cus) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) return 0;
    cus = v;
  }
  return (long)cus * BLOCKS_PER_CU;
}

}  // namespace

extern "C" int fmxe_attn_blend_f16(const void* own, const void* shared, void* out, float w_own, float w_shared, int64_t n, void* stream) {
  FMX_REQUIRE(own && shared && out, "attn_blend: null pointer");
  FMX_REQUIRE(n > 0, "attn_blend: n %ld", (long)n);
  FMX_REQUIRE(fmx_aligned16(own) && fmx_aligned16(shared) && fmx_aligned16(out), "attn_blend: bases must be 16-byte aligned");
  const long cap = max_blocks();
  FMX_REQUIRE(cap > 0, "attn_blend: cannot read the device's CU count");
  long blocks = ((n >> 3) + TPB - 1) / TPB;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(attn_blend_kernel, dim3((unsigned)blocks), dim3(TPB), 0, (hipStream_t)stream, (const _Float16*)own, (const _Float16*)shared,
                     (_Float16*)out, w_own, w_shared, (long)n);
  FMX_LAUNCH_CHECK("fmxe_attn_blend_f16");
  return FMX_OK;
}
