/*
 * flash_attn_mi355x_varlen.h -- C ABI of libflash_attn_mi355x_varlen.so: the differentiable causal attention of the MI355X (gfx950)
 * library on a PACKED batch of sequences of different lengths, with or without a sliding window and attention-sink tokens, and the
 * rotary embedding whose positions restart at every sequence.
 *
 *   q, out, out_grad, q_grad   [T][H][d]      token-major, as in the ragged KV-cache calls (flash_attn_mi355x_decode_ragged.h)
 *   k, v, k_grad, v_grad       [T][Hkv][d]    H = G * Hkv, query head h reads kv head h / G in place
 *   q, k, v, out_grad          dtype elements (FA_DTYPE_F32 or FA_DTYPE_BF16); out, lse [H][T] and the gradients are fp32
 *   cu_seqlens                 int32 [nseq + 1] on the device.  Sequence b owns the packed rows s_b .. s_b + n_b - 1 with
 *                              s_b = clamp(cu[b], 0, T) and s_b + n_b = clamp(max(cu[b + 1], s_b), 0, T): whatever the array holds,
 *                              no access leaves the T-row buffers.  n_b may be 0.  It is never read on the host.
 *
 * Row i of sequence b sits at position i and admits key j of the SAME sequence
 *
 *     iff   j <= i   and   (j > i - W   or   j < S)          W = window, S = sink;  window = 0: no window, every j <= i
 *
 * Causal only.  A sink needs a window.  lse is taken over the admitted keys.  Rows that no sequence owns (in front of cu[0], behind
 * cu[nseq]) are ZERO in out, lse and the three gradients after the call.
 *
 * The law that defines the calls: for every sequence with n_b >= 1, rows s_b .. s_b + n_b - 1 of out, lse, q_grad, k_grad and
 * v_grad are, bit for bit, what fa_mi355x_fwd_window / fa_mi355x_bwd_window (flash_attn_mi355x_window.h) return for that sequence
 * alone (B = 1, N = n_b, FA_LAYOUT_BNHD, the same window and sink; window = 2^31 - 1 for "no window").
 *
 *   T        packed rows, >= 1.  T * 128 * 4 and T * H * d * 4 bytes must stay under 2 GiB, the bound of one buffer resource: T
 *            bounds every n_b, so the bound holds for every sequence whatever cu_seqlens says.
 *   nseq     >= 1
 *   d        32, 64 or 128; other head sizes through zero-padded columns and softmax_scale = 1/sqrt(d)
 *   softmax_scale   0: sqrt(1/d); otherwise positive and finite
 *
 * Workspace.  A block map has (T / b + nseq) entries of 16 bytes for block size b: a sequence of n rows has at most n / b + 1
 * blocks, and the floors sum to at most T / b.  With MAP = align256(16 * (T / 128 + nseq)):
 *
 *     fa_mi355x_fwd_varlen_workspace_bytes = MAP
 *     fa_mi355x_bwd_varlen_workspace_bytes = 2 * MAP + 3 * H * T * 4                                     (Hkv == H)
 *                                          = 2 * MAP + align256(3 * H * T * 4) + 2 * H * T * d * 4       (Hkv <  H)
 *
 *   (the map of the query blocks, the map of the key blocks, three row-constant vectors, the per-query-head dK and dV that the
 *   ordered group sum adds).  Both are pure functions of their arguments, 0 for sizes they cannot answer (a non-positive size, Hkv
 *   not dividing H, a result past 2^62).  The workspace must be 256-byte aligned.  The grids depend on the arguments only.
 *
 * Non-positive sizes, nseq < 1, Hkv not dividing H, window < 0, sink < 0, a sink without a window, an unsupported d, an unknown
 * dtype, a bad softmax_scale, null pointers, a misaligned workspace and sizes past the bounds above are FA_ERR_BAD_ARG with a
 * message (fa_mi355x_varlen_last_error), before any HIP call.  Asynchronous on `stream`, no allocation, nothing read back: every
 * call can be captured in a graph.  No atomics and a fixed summation order: a call repeats bit for bit.
 */
#ifndef FLASH_ATTN_MI355X_VARLEN_H
#define FLASH_ATTN_MI355X_VARLEN_H

#include <stddef.h>

#include "flash_attn_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t fa_mi355x_fwd_varlen_workspace_bytes(int nseq, int T, int H, int Hkv, int d);
size_t fa_mi355x_bwd_varlen_workspace_bytes(int nseq, int T, int H, int Hkv, int d);

/* out and lse of every sequence; zeros in the rows no sequence owns.  Launches: the schedule (block map, unowned rows), the
 * query-stationary forward. */
int fa_mi355x_fwd_varlen(const void* q, const void* k, const void* v, float* out, float* lse, const int* cu_seqlens, void* workspace,
                         int nseq, int T, int H, int Hkv, int d, float softmax_scale, int window, int sink, int dtype, void* stream);

/* q_grad, k_grad, v_grad from out_grad, the forward's out and lse, under the same cu_seqlens, window and sink.  Launches: the
 * schedule, the row constants, the key-stationary dK/dV kernel, for Hkv < H the group sum, the query-stationary dQ kernel. */
int fa_mi355x_bwd_varlen(const void* q, const void* k, const void* v, const float* out, const void* out_grad, float* q_grad,
                         float* k_grad, float* v_grad, const float* lse, const int* cu_seqlens, void* workspace, int nseq, int T, int H,
                         int Hkv, int d, float softmax_scale, int window, int sink, int dtype, void* stream);

/* y = x rotated by position, x and y [T][H][d] (y may be x): packed row t of sequence b sits at position t - s_b, clamped to
 * 0 .. max_pos - 1; a row no sequence owns is copied.  cos, sin: fp32 [max_pos][rot / 2]; rot even, 2 <= rot <= d; interleaved: 0
 * NeoX pairs, 1 GPT-J pairs; inverse: 1 rotates back.  The arithmetic is fa_mi355x_rope's (flash_attn_mi355x_decode_rope.h). */
int fa_mi355x_rope_varlen(const void* x, void* y, const float* cos, const float* sin, const int* cu_seqlens, int nseq, int T, int H, int d,
                          int rot, int max_pos, int interleaved, int inverse, int dtype, void* stream);

/* The message of the calling thread's last failed call into this library ("" after a call that succeeded). */
const char* fa_mi355x_varlen_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* FLASH_ATTN_MI355X_VARLEN_H */
