/*
 * flash_attn_mi355x_lsink.h -- C ABI of libflash_attn_mi355x_lsink.so: the TRAINING side of learned attention-sink logits (gpt-oss).
 * The causal sliding-window forward of flash_attn_mi355x_window.h in which one learned fp32 logit per query head joins every row's
 * softmax as an extra column without a value vector, and the gradient of those logits.  The KV-cache calls that generate under the
 * same function are flash_attn_mi355x_decode_lsink.h, in the decode library.  Status codes, dtypes and layouts are
 * flash_attn_mi355x.h's.
 *
 * With tau = softmax_scale, or 1/sqrt(d) when that is 0, the query of row i at position i, its admitted keys A(i) = { j : j <= i and
 * j > i - W }, z_ij = tau * (q_i . k_j) and a = sink_logits[h] for query head h:
 *
 *   lse_i = ln( e^a + sum_{j in A(i)} e^z_ij ),   P_ij = e^(z_ij - lse_i)  (row sums below 1),   out_i = sum_j P_ij v_j
 *
 * The logit is in logit units: not multiplied by tau, not rotated, not masked.  It must be finite (a = +inf would be inf - inf in the
 * row's end; as for the fp8 scales, the kernels do not check).  No finite a and no finite score overflows (the end of a row works in
 * log2 units on max(m c, a log2 e), flash_attn_mi355x_decode_lsink.h).
 *
 * Backward for q, k and v: NO new kernel and no entry point here.  dS = P o (dP - delta) with P = exp2(s c - lse log2 e) and
 * delta_i = rowsum(dO_i o out_i) holds for this P as for the plain softmax (the sink column has no value vector, so it adds nothing
 * to dP . V, and sum_j P_ij dP_ij = dO_i . out_i still), and that is exactly what fa_mi355x_bwd_window computes from the lse and
 * out it is GIVEN.  Call fa_mi355x_bwd_window (sink = 0) with this forward's out and lse.
 *
 * Gradient of the logits: d a_h = - sum_{b,i} e^(a_h - lse_bhi) * delta_bhi, a reduction over all B * N rows of a head.
 *
 * Asynchronous on `stream`, no allocation, no host synchronisation, no atomics, no scratch: a call repeats bit for bit.
 */
#ifndef FLASH_ATTN_MI355X_LSINK_H
#define FLASH_ATTN_MI355X_LSINK_H

#include <stddef.h>

#include "flash_attn_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The message of this thread's last failed call into this library ("" after a successful one). */
const char* fa_mi355x_lsink_last_error(void);

/* The forward.  q [B][N][H][d] (FA_LAYOUT_BNHD) or [B][H][N][d] (FA_LAYOUT_BHND), k and v likewise with Hkv heads (Hkv divides H:
 * query head h reads kv head h / (H / Hkv), in place), out fp32 in q's shape, lse fp32 [B][H][N], sink_logits fp32 [H] on the
 * device (read there: no host copy).  d in {32, 64, 128}; bf16 or fp32; scores are scaled in fp32.  Causal, window >= 1; a window
 * above N is clamped to N, so a call without a window passes window = N.  win_lsink_fwd_kernel: the forward kernel text of the
 * window library built under a name of its own with the sink term in its epilogue.
 * FA_ERR_BAD_ARG before any HIP call: a null pointer (sink_logits included), window < 1, sizes that are not positive, Hkv that does
 * not divide H, an unknown dtype or layout, a bad softmax_scale; FA_ERR_UNSUPPORTED_D does not occur (d is a bad argument here, as in
 * the window library). */
int fa_mi355x_fwd_window_lsink(const void* q, const void* k, const void* v, float* out, float* lse, const float* sink_logits, int B, int H,
                               int Hkv, int N, int d, int layout, float softmax_scale, int window, int dtype, void* stream);

/* Bytes of the workspace of fa_mi355x_sink_logits_grad: one fp32 partial per (head, slice of FA_LSINK_SLICE_ROWS rows).  0 for
 * sizes that are not positive. */
#define FA_LSINK_SLICE_ROWS 512
size_t fa_mi355x_sink_logits_grad_workspace_bytes(int B, int H, int N, int d);

/* The gradient of the logits: sink_grad[h] = - sum_{b,i} exp(sink_logits[h] - lse[b][h][i]) * sum_c out_grad[b,h,i,c] * out[b,h,i,c].
 * out fp32 and out_grad (the call's dtype) in q's shape and layout, lse [B][H][N], sink_logits and sink_grad fp32 [H]; out and
 * out_grad 16-byte aligned (the two that are read with vector loads; checked).  Two launches.  sink_grad_partial_kernel: workgroup (h, s) takes rows s * 512 .. s * 512 + 511 of the B * N rows
 * of head h, forms each row's delta from 16-byte loads of out and out_grad, and writes ONE partial into workspace[h][s]; at B = 2,
 * H = 32, N = 8192 that is 1024 workgroups on 256 CUs (one workgroup per head would leave 7/8 of them idle).  sink_grad_sum_kernel
 * adds each head's partials in slice order.  A fixed order throughout: the same bits on every run. */
int fa_mi355x_sink_logits_grad(const float* out, const void* out_grad, const float* lse, const float* sink_logits, float* sink_grad,
                               void* workspace, int B, int H, int N, int d, int layout, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLASH_ATTN_MI355X_LSINK_H */
