/* IP-Adapter entry point of libfmx_gfx950.so, not (yet) declared in fmx.h.
 *
 * fmx.h is the home of the C ABI, but tests/test_capi_symbols.py pins the number of `fmx_*` entry points it declares (97),
 * tests/test_stylealign_host.py pins include/fmx_ext.h and the exported `fmxe_*` symbols to exactly one entry point, and tests/test_lllite_host.py
 * pins include/fmx_lllite.h and the `fmxl_*` symbols likewise.  A change that leaves those tests as they are can extend none of the three headers,
 * so this entry point is declared HERE under a fourth prefix, `fmxi_`; whoever next revises those tests moves it into fmx.h as
 * fmx_attention_dual_f16 (and its struct as fmx_dual_attn_args) and raises the count -- nothing else depends on the split.
 * Same conventions as the other headers: returns int (FMX_OK or an FMX_E_* code, message through fmx_last_error()), takes the stream last,
 * validates before any launch.  forge_amd/_lib.py derives its ctypes binding from this file as it does from the other three
 * (IPADAPTER_SIGNATURES), and tests/test_ipadapter_host.py holds it to their rules: every exported `fmxi_*` symbol is declared here, the binding
 * lists exactly this set, and each is named in a tests/test_gpu_*.py file.  FMX_ABI_VERSION stays 12: a new symbol moves no existing signature.
 */
#ifndef FMX_IPADAPTER_H
#define FMX_IPADAPTER_H

#include <stdint.h>

#include "fmx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FMXI_MAX_SEGMENTS 4
#define FMXI_EXTRA_KEYS 64

/* ------------------------------------------------------------------------------------------------
 * Cross-attention with an EXTRA CONTEXT (IP-Adapter, lib_ipadapter/IPAdapterPlus.py CrossAttentionPatch.__call__): per query row, in fp32,
 *   O = softmax(Q K^T * scale) V  +  sum over segments s of  weight_s * softmax(Q XK_s^T * scale) XV_s
 * in ONE launch: one read of Q, one write of O.
 *   q, k, vt, o and their strides, batch, heads, nq, nk, nk_pad, scale, zero_page: those of fmx_attn_args, with the same guarantees about what
 *   may lie around the operands (k rows [nk, nk_pad) anything; vt columns [nk, nk_pad) finite; q rows >= nq never used; exactly the elements
 *   (b, i < nq, h, d < 64) of o are written).
 *   xk   : fp16 [groups][64 rows][heads * 64] dense: the extra keys of group g, head h, key j at xk[(g * 64 + j) * heads * 64 + h * 64 + d]
 *   xvt  : fp16 V^T [heads * 64 rows][groups * 64] dense (the text V^T's layout with vt_bs = 64): xvt[(h * 64 + d) * groups * 64 + g * 64 + j].
 *          Every element must be FINITE (zeros beyond the last segment): a key outside the segments is multiplied by a probability of exactly 0.
 *   images_per_group: image b reads group b / images_per_group (cond and uncond rows of a batch use different image tokens); groups =
 *          batch / images_per_group.
 *   nseg in 1..4 segments (start, count, weight), disjoint, inside [0, 64), count >= 1: an independent softmax over the keys
 *          [start, start + count) of the group, the same `scale`.  xk rows outside every segment contribute nothing, whatever they hold (NaN
 *          included: they are masked by a select on the key index).
 * Roundings: the text term is fmx_attention_f16's short-context kernel to the last fp32 operation (probabilities exp2(s - max) rounded to fp16
 * once, the sum of the unrounded ones divided out of the fp32 accumulator).  A segment's probabilities are multiplied by weight_s / (their
 * sum) in fp32 and THEN rounded to fp16 once -- the weight is folded into the probabilities -- so that all segments are one further MFMA
 * accumulation on top of the normalised text accumulator.  O is rounded to fp16 once.  A weight of 0 gives the text-only result bit for bit.
 * No atomics, no traffic between workgroups: the same bits on every run.
 * Scope (FMX_E_BADARG otherwise, before any launch): dpad == 64; 1 <= nk <= 128; nq >= 1; batch % images_per_group == 0; the pointer, alignment
 * and stride rules of fmx_attn_args; xk / xvt non-null and 16-byte aligned; the segment rules above; Q, K and V^T of one (batch, head) within 2 GB
 * of its base (the kernel addresses them by 32-bit byte offsets).  No mask, not causal.
 * ---------------------------------------------------------------------------------------------- */
typedef struct fmxi_dual_attn_args {
  const void* q;
  const void* k;
  const void* vt;
  void* o;
  int64_t q_bs, q_rs;
  int64_t k_bs, k_rs;
  int64_t vt_bs, vt_hs, vt_ds;
  int64_t o_bs, o_rs;
  int32_t batch, heads, nq, nk, nk_pad, dpad;
  float scale;
  int32_t images_per_group;
  const void* zero_page;
  const void* xk;
  const void* xvt;
  int32_t nseg;
  int32_t seg_start0, seg_start1, seg_start2, seg_start3;
  int32_t seg_count0, seg_count1, seg_count2, seg_count3;
  float seg_weight0, seg_weight1, seg_weight2, seg_weight3;
} fmxi_dual_attn_args;

int fmxi_attention_dual_f16(const fmxi_dual_attn_args* args /* host */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FMX_IPADAPTER_H */
