/*
 * flash_attn_mi355x_mla_prefill.h -- C ABI of libflash_attn_mi355x_mla_prefill.so: the PROMPT half of multi-head latent attention
 * (DeepSeek MLA) on the MI355X (gfx950).  A prompt is attended before absorption, as causal attention whose head has 192 score
 * columns, k_nope (128, per head) followed by the rotated k_pe (64, ONE vector per token shared by all heads), and 128 value
 * columns.  Forward and backward, bf16 operands, on a PACKED batch under the two cu_seqlens of the causal two-array packed library: a fresh
 * prompt, a chunk of a long prompt behind its already-processed part and drafted tokens behind a prefix are one call.  The decode
 * half, on the absorbed 576-wide latent cache, is flash_attn_mi355x_mla.h.
 *
 *   q        bf16 [Tq][H][192]   q_nope then the rotated q_pe, contiguous
 *   k_nope   bf16, Tk rows of H heads x 128 columns: element (row t, head h, column c) at k_nope[t * k_ld + h * k_hstride + c]
 *   v        bf16, the same geometry under its own pointer, v_ld and v_hstride
 *   k_pe     bf16 [Tk][64]       contiguous; every head reads the same row
 *   out      fp32 [Tq][H][128], lse fp32 [H][Tq]
 *   cu_seqlens_q, cu_seqlens_k   int32 [nseq + 1] on the device, read there and never on the host, under the clamping rule of
 *            the causal two-array packed library: sequence b owns the rows s_b .. s_b + n_b - 1 of the q buffers with
 *            s_b = clamp(cu_q[b], 0, Tq) and s_b + n_b = clamp(max(cu_q[b + 1], s_b), 0, Tq), likewise of the k buffers (k_nope, k_pe, v) under cu_seqlens_k and
 *            Tk.  Whatever the arrays hold, no access leaves the buffers.  Either count may be 0.  The two pointers may be one array.
 *
 * k_nope and v have strides of their own so that the output of ONE up-projection GEMM, [Tk][H][256] = k_nope | v per head, is read
 * in place through two views (k_ld = v_ld = H * 256, k_hstride = v_hstride = 256, v = k_nope + 128); nothing is concatenated and
 * k_pe is not copied H times.  Strides are in elements, multiples of 8, a head stride >= 128, a row stride >= (H - 1) * head stride
 * + 128; q, k_nope, k_pe, v and out are 16-byte aligned.
 *
 * With D = n_k(b) - n_q(b), query row i of sequence b admits key j of the same sequence iff 0 <= j <= i + D (bottom-right
 * alignment); the score of head h is softmax_scale * (q_nope . k_nope[j][h] + q_pe . k_pe[j]); lse is taken over the admitted keys.
 *
 *   a row that admits no key  (i + D < 0, or n_k(b) = 0) exact ZEROS in out and lse
 *   rows no sequence owns     (in front of cu_q[0], behind cu_q[nseq]) ZEROS in out and lse
 *
 * The law: for every sequence its rows of out and lse are, bit for bit, what the call returns for that sequence alone (nseq = 1).
 * No atomics and a fixed summation order: a call repeats bit for bit.
 *
 *   softmax_scale   0: 192^-1/2; otherwise positive and finite (a YaRN model passes its own).  Every score is scaled in fp32.
 *   Tq, Tk, nseq, H >= 1.  (Tq + 128) * H * 192 * 2, Tq * H * 128 * 4, (Tk + 128) * k_ld * 2 and (Tk + 128) * v_ld * 2 bytes must
 *            stay under 2 GiB, the bound of one buffer resource and of the 32-bit byte offsets under it.
 *
 * How it runs: the schedule kernel of the two-array libraries (block map of 128-row query blocks, zeros in unowned rows), then one
 * query-stationary kernel, a workgroup of 4 waves x 32 rows per (head, block), walking the keys below the block's diagonal in
 * 64-key tiles staged as three LDS images (k_nope, k_pe, v) (csrc/fa_mla_prefill.h).  The grid depends on the arguments only; a
 * block whose rows admit no key walks no tile.
 *
 * Workspace: the query-block map, fa_mi355x_fwd_mla_prefill_workspace_bytes = align256(32 * (Tq / 128 + nseq)); a pure function of
 * its arguments, 0 for a non-positive size.  256-byte aligned.
 *
 * Non-positive sizes, null pointers, a bad softmax_scale, bad strides, offsets past the bounds above, a grid past 2^31 workgroups
 * and misaligned operands or workspace are FA_ERR_BAD_ARG with a message (fa_mi355x_mla_prefill_last_error), before any HIP call.
 * Asynchronous on `stream`, no allocation, nothing read back: the call can be captured in a graph and replayed on other lengths.
 *
 * The backward, fa_mi355x_bwd_mla_prefill: from the forward's operands, its out and lse and dout = dL/dout (bf16 [Tq][H][128]) it
 * writes, in fp32, dq [Tq][H][192], dk_pe [Tk][64] (the SUM over the heads, which all read the one k_pe row), and dk_nope and dv in
 * k_nope's geometry under strides of their own (dk_ld, dk_hstride, dv_ld, dv_hstride: elements, multiples of 4, the same lower
 * bounds), so that the gradient of one [Tk][H][256] up-projection output is written in place through two views.
 *
 *   dq of a row that admits no key; dk_nope, dv and dk_pe of a key that no query admits (n_q(b) = 0 included)   exact ZEROS
 *   every row that no sequence owns (in dq, dk_nope, dk_pe, dv)                                                exact ZEROS
 *
 * The law holds for the four gradients as for out, and a call repeats bit for bit: no atomics, the heads are added into dk_pe in a
 * fixed order that depends on H alone.
 *
 * How it runs (csrc/fa_mla_prefill_bwd.h): the schedule kernel (both block maps, zeros in unowned rows), the row constants
 * -lse / softmax_scale and -rowsum(dout * out), a key-stationary kernel for dk_nope, dv and dk_pe in which a workgroup owns 128 keys
 * and a GROUP of g(H) = clamp(H / 16, 2, 8) heads and keeps k_pe and the dk_pe accumulators across them, a kernel that adds the
 * groups' dk_pe partials when there is more than one group, and a query-stationary kernel for dq.
 *
 * Its workspace, fa_mi355x_bwd_mla_prefill_workspace_bytes = align256(32 * (Tq / 128 + nseq)) + align256(32 * (Tk / 128 + nseq))
 * + align256(3 * H * Tq * 4) + (G > 1 ? G * Tk * 64 * 4 : 0) with G = ceil(H / g(H)) head groups: the two maps, the row constants
 * and the dk_pe partials; a pure function of its arguments, 0 for a non-positive size.  256-byte aligned.
 *
 * Its refusals are the forward's, and: null dout or gradient pointers, bad dk_nope / dv strides, Tq * H * 192 * 4, Tk * dk_ld * 4 or
 * Tk * dv_ld * 4 bytes at or past 2 GiB, dout or a gradient not 16-byte aligned.  Asynchronous, no allocation, nothing read back.
 *
 * Not built: fp32 operands, windows, sinks and a logit cap, the up-projection or its backward fused into the kernels, other head
 * shapes, grouped k/v heads, and reading a cached prefix's keys and values out of the latent cache (the caller up-projects them).
 */
#ifndef FLASH_ATTN_MI355X_MLA_PREFILL_H
#define FLASH_ATTN_MI355X_MLA_PREFILL_H

#include <stddef.h>

#include "flash_attn_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t fa_mi355x_fwd_mla_prefill_workspace_bytes(int nseq, int Tq, int Tk, int H);

/* out and lse of every sequence; zeros in the rows that admit no key and in the rows no sequence owns. */
int fa_mi355x_fwd_mla_prefill(const void* q, const void* k_nope, const void* k_pe, const void* v, float* out, float* lse,
                              const int* cu_seqlens_q, const int* cu_seqlens_k, void* workspace, int nseq, int Tq, int Tk, int H, int k_ld,
                              int k_hstride, int v_ld, int v_hstride, float softmax_scale, void* stream);

size_t fa_mi355x_bwd_mla_prefill_workspace_bytes(int nseq, int Tq, int Tk, int H);

/* dq, dk_nope, dk_pe and dv of every sequence from the forward's operands and results; zeros as listed above. */
int fa_mi355x_bwd_mla_prefill(const void* q, const void* k_nope, const void* k_pe, const void* v, const float* out, const void* dout,
                              const float* lse, float* dq, float* dk_nope, float* dk_pe, float* dv, const int* cu_seqlens_q,
                              const int* cu_seqlens_k, void* workspace, int nseq, int Tq, int Tk, int H, int k_ld, int k_hstride, int v_ld,
                              int v_hstride, int dk_ld, int dk_hstride, int dv_ld, int dv_hstride, float softmax_scale, void* stream);

/* The message of the calling thread's last failed call into this library ("" after a call that succeeded). */
const char* fa_mi355x_mla_prefill_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* FLASH_ATTN_MI355X_MLA_PREFILL_H */
