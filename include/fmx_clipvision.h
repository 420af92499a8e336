/* CLIP-vision front-end entry points of libfmx_gfx950.so, not (yet) declared in fmx.h.
 *
 * include/fmx_ipadapter.h says why fmx.h, fmx_ext.h, fmx_lllite.h and fmx_ipadapter.h itself cannot grow while the tests that pin their sets of
 * entry points stay as they are; the two kernels a ViT needs in front of the existing GEMM / attention / LayerNorm kernels are therefore declared
 * HERE under a fifth prefix, `fmxv_`.  Whoever next revises those tests moves them into fmx.h as fmx_clip_patch_rows_f16 / fmx_clip_embed_ln_f16.
 * Same conventions as the other headers: returns int (FMX_OK or an FMX_E_* code, message through fmx_last_error()), takes the stream last,
 * validates before any launch.  forge_amd/_lib.py derives its ctypes binding from this file (CLIPVISION_SIGNATURES), and
 * tests/test_clipvision_host.py holds it to the rules of the others: every exported `fmxv_*` symbol is declared here, the binding lists exactly
 * this set, and each is named in a tests/test_gpu_*.py file.  FMX_ABI_VERSION stays 12: a new symbol moves no existing signature.
 * Both kernels are plain memory-bound passes: no atomics, no traffic between workgroups, the same bits on every run.
 */
#ifndef FMX_CLIPVISION_H
#define FMX_CLIPVISION_H

#include <stdint.h>

#include "fmx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FMXV_CLIP_IMAGE 224      /* side of the crop the towers see (the reference's clip_preprocess fixes it) */
#define FMXV_CLIP_PATCH 14       /* side of a patch: a 16 x 16 grid, 256 patches */
#define FMXV_CLIP_PATCH_COLS 640 /* 3 * 14 * 14 = 588 columns of the patch matrix, zero-padded to the GEMMs' multiple of 64 */
#define FMXV_CLIP_TOKENS 257     /* class token + 256 patches */

/* ------------------------------------------------------------------------------------------------
 * The second half of clip_preprocess (backend/patcher/clipvision.py:77-88: crop, quantise to 8-bit levels, normalise) and the im2col of the
 * 14 x 14 / stride-14 patch convolution, in one pass.
 *   in   : fp32 planes [b][3][rh][rw] (NCHW, dense): the image after the antialiased resize, or the source image when it is 224 x 224 already
 *   crop : the window [top, top + 224) x [left, left + 224) of every plane
 *   out  : fp16 [b * 256][640] dense.  Row b * 256 + py * 16 + px is patch (py, px); column ch * 196 + iy * 14 + ix is pixel
 *          (top + py * 14 + iy, left + px * 14 + ix) of plane ch -- the flattening of the conv weight [C, 3, 14, 14] to [C, 588], so the weight is
 *          used as stored.  Columns 588..639 are written as +0.  Exactly these b * 256 * 640 elements are written.
 * Per element, in fp32 and in this order: t = 255 * x;  t clamped to [0, 255] (a NaN stays a NaN);  v = rint(t) / 255 (ties to even, IEEE
 * division);  (v - mean[ch]) / std[ch] (IEEE division) with mean = {0.48145466, 0.4578275, 0.40821073}, std = {0.26862954, 0.26130258,
 * 0.27577711};  one rounding to fp16.  That is torch's `(clip(255 x, 0, 255).round() / 255 - mean) / std` in fp32, then `.half()`, bit for bit.
 * FMX_E_BADARG before any launch: null pointers; `in` not 4-byte or `out` not 16-byte aligned; b < 1; rh or rw < 224; top / left negative or the
 * window past the plane; b * 256 rows beyond 2^31.
 * ---------------------------------------------------------------------------------------------- */
int fmxv_clip_patch_rows_f16(const void* in, void* out, int32_t b, int32_t rh, int32_t rw, int32_t top, int32_t left, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Token assembly (CLIPVisionEmbeddings: class token first, position embedding added) and pre_layrnorm in one pass.
 *   patches            : fp16 [b * 256][c] dense, the patch GEMM's output
 *   class_embedding    : fp16 [c]
 *   position_embedding : fp16 [257][c] dense
 *   gamma, beta        : fp16 [c]
 *   out                : fp16 [b][rows_per_image][c] dense.  Row 0 of image i = LN(class + pos[0]); row 1 + p = LN(patches[i * 256 + p] + pos[1 + p]);
 *                        rows 257..rows_per_image - 1 are written as +0.  Exactly these b * rows_per_image * c elements are written.
 * Arithmetic: the two fp16 operands are added in fp32 (no rounding of the sum to fp16); mean = sum / c; variance = sum((x - mean)^2) / c, two
 * passes over the row held in registers; y = (x - mean) * rsqrt(variance + eps) * gamma + beta; one rounding to fp16 at the store.  One wave
 * per row: each lane adds its elements in column order (octets lane, lane + 64, ...), then a 6-step xor butterfly.
 * FMX_E_BADARG before any launch: null pointers; any pointer not 16-byte aligned; b < 1; c < 8, c % 8 != 0 or c > 4096 (fmx_layernorm's rules);
 * rows_per_image < 257 or not a multiple of 64; b * rows_per_image rows beyond 2^31.
 * ---------------------------------------------------------------------------------------------- */
int fmxv_clip_embed_ln_f16(const void* patches, const void* class_embedding, const void* position_embedding, const void* gamma, const void* beta,
                           void* out, int32_t b, int32_t c, int32_t rows_per_image, float eps, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FMX_CLIPVISION_H */
