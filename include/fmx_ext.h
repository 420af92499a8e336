/* Entry points of libfmx_gfx950.so that are not (yet) declared in fmx.h.
 *
 * fmx.h is the home of the C ABI.  tests/test_capi_symbols.py pins the NUMBER of `fmx_*` entry points it declares (97) and ties every exported
 * `fmx_*` symbol and the ctypes binding to exactly that set, so declaring one more there means editing that test in the same change.  A change
 * that leaves the existing tests as they are declares its entry point HERE instead, under the prefix `fmxe_`; whoever next revises that test
 * moves these declarations into fmx.h under their `fmx_` names and raises the count -- nothing else depends on the split.  Same conventions: returns int (FMX_OK or an FMX_E_* code, message through fmx_last_error()), takes the stream last,
 * validates before any launch.  forge_amd/_lib.py derives its ctypes binding from this file exactly as it does from fmx.h (EXT_SIGNATURES), and
 * tests/test_stylealign_host.py holds this file to the rules tests/test_capi_symbols.py and tests/test_kernel_test_coverage.py hold fmx.h to:
 * every exported `fmxe_*` symbol is declared here, the binding lists exactly this set, and each is named in a tests/test_gpu_*.py file.  FMX_ABI_VERSION stays 12: a new symbol moves no existing signature.
 */
#ifndef FMX_EXT_H
#define FMX_EXT_H

#include <stdint.h>

#include "fmx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * StyleAlign ("StyleAlign Integrated", forge_stylealign.py:29-97): every self-attention of the UNet runs over the tokens of all images of a
 * group (the cond images, the uncond images) joined into one sequence.  The executor's layouts make a group of b consecutive images one
 * contiguous sequence of T = b * n tokens in Q, K and V^T, so the shared attention is fmx_attention_f16 with batch = groups, nq = nk = T,
 * q_bs = k_bs = T * row stride, vt_bs = T: no copy, no mask, no attention kernel of its own.  What is new is the blend at 0.01 <= strength <= 0.99.
 *
 * fmxe_attn_blend_f16: elementwise over n contiguous fp16 values, the reference expression `(1.0 - strength) * own + strength * shared` on
 * fp16 tensors with Python float scalars, rounding for rounding:
 *   out[i] = h( f(h(f(own[i]) * w_own)) + f(h(f(shared[i]) * w_shared)) )        f: fp16 -> fp32 (exact), h: fp32 -> fp16 (nearest even)
 * each product an fp32 multiply rounded to fp16, the sum an fp32 add rounded to fp16; the weights are NOT rounded to fp16.  The host passes
 * w_own = (float)(1.0 - strength), the subtraction made in double, and w_shared = (float)strength.
 * out may alias own or shared.  16-byte loads and stores, a grid of at most 8 workgroups per CU striding over the rest, no LDS; the last
 * n % 8 elements with 2-byte accesses.  Nothing behind element n - 1 is read or written.
 * Requirements (FMX_E_BADARG otherwise, before any launch): pointers non-null and 16-byte aligned; n > 0.
 * ---------------------------------------------------------------------------------------------- */
int fmxe_attn_blend_f16(const void* own, const void* shared, void* out, float w_own, float w_shared, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FMX_EXT_H */
