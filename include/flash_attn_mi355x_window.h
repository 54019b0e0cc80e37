/*
 * flash_attn_mi355x_window.h -- C ABI of libflash_attn_mi355x_window.so: the differentiable (training / prefill) attention of the
 * MI355X (gfx950) library under a sliding window, with or without attention-sink tokens.
 *
 * The KV-cache calls (flash_attn_mi355x_decode_window.h, _sink.h) generate under this mask; these two calls train under it, and
 * cost O(N * W) where the causal call costs O(N^2).  The query of row i sits at position i:
 *
 *     row i admits key j   iff   j <= i   and   (j > i - W   or   j < S)          W = window >= 1, S = sink >= 0
 *
 *   A key that is both a sink and inside the window counts once.  lse is taken over the admitted keys.  Causal only: every row
 *   admits its own position, so no row is empty and every lse is finite.
 *
 * A library of its own, as the decode library is: the training library (flash_attn_mi355x.h) keeps its code object.  Same status
 * codes (FA_OK, FA_ERR_*), dtypes (FA_DTYPE_*) and layouts (FA_LAYOUT_*) as there.  Only the FA-2 side output (lse) exists here: no
 * key mask, no dropout, no FA-1 (l, m) outputs.  tau * log2(e) is applied to every score in fp32: no scale guard, no options.
 *
 *   q, out, out_grad, q_grad   H heads:   [B][H][N][d] (FA_LAYOUT_BHND) or [B][N][H][d] (FA_LAYOUT_BNHD)
 *   k, v, k_grad, v_grad       Hkv heads: [B][Hkv][N][d] or [B][N][Hkv][d]; H = G * Hkv, query head h reads kv head h / G in place
 *   q, k, v, out_grad          dtype elements (FA_DTYPE_F32 or FA_DTYPE_BF16); out, lse [B][H][N] and the gradients are fp32
 *   N        any N >= 1.  One (batch*head) matrix and one batch element must stay under 2 GiB, as for fa_mi355x_fwd_gqa.
 *   d        32, 64 or 128; other head sizes through zero-padded columns and softmax_scale = 1/sqrt(d)
 *   softmax_scale   0: sqrt(1/d); otherwise positive and finite, as fa_mi355x_fwd_gqa takes it
 *   window   W >= 1.  W > N is clamped to N: every j <= i is admitted, plain causal attention computed by these kernels.
 *   sink     S >= 0.  S > N is clamped to N, with the same result.
 *
 * window < 1, sink < 0, H not a multiple of Hkv, non-positive sizes, an unsupported d, an unknown dtype or layout, a bad
 * softmax_scale and null pointers are FA_ERR_BAD_ARG with a message (fa_mi355x_window_last_error), before any HIP call.
 * Asynchronous on `stream`, no allocation, no host synchronisation: both calls can be captured in a graph.  No atomics and a fixed
 * summation order: a call repeats bit for bit.
 */
#ifndef FLASH_ATTN_MI355X_WINDOW_H
#define FLASH_ATTN_MI355X_WINDOW_H

#include <stddef.h>

#include "flash_attn_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out = softmax over the admitted keys (scale * q . k) . v and its natural-log logsumexp lse. */
int fa_mi355x_fwd_window(const void* q, const void* k, const void* v, float* out, float* lse, int B, int H, int Hkv, int N, int d,
                         int layout, float softmax_scale, int window, int sink, int dtype, void* stream);

/* Bytes of device workspace fa_mi355x_bwd_window needs: three row-constant vectors of B * H * N floats and, for Hkv < H, the
 * per-query-head dK and dV that the ordered group sum adds (256-byte aligned behind the vectors).  A pure function of its
 * arguments; 0 for sizes it cannot answer. */
size_t fa_mi355x_bwd_window_workspace_bytes(int B, int H, int Hkv, int N, int d);

/* q_grad, k_grad, v_grad from out_grad, the forward's out and lse, under the same window and sink.  workspace: 256-byte aligned
 * device memory of fa_mi355x_bwd_window_workspace_bytes(B, H, Hkv, N, d) bytes.  Launches: the row constants
 * (-lse / scale, -rowsum(out_grad * out)), the key-stationary dK/dV kernel, for Hkv < H the group sum, the query-stationary dQ
 * kernel. */
int fa_mi355x_bwd_window(const void* q, const void* k, const void* v, const float* out, const void* out_grad, float* q_grad,
                         float* k_grad, float* v_grad, const float* lse, void* workspace, int B, int H, int Hkv, int N, int d,
                         int layout, float softmax_scale, int window, int sink, int dtype, void* stream);

/* The message of the calling thread's last failed call into this library ("" after a call that succeeded). */
const char* fa_mi355x_window_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* FLASH_ATTN_MI355X_WINDOW_H */
