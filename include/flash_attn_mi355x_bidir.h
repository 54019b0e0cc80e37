/*
 * flash_attn_mi355x_bidir.h -- C ABI of libflash_attn_mi355x_bidir.so: the differentiable BIDIRECTIONAL attention of the MI355X
 * (gfx950) library on a PACKED batch in which sequence b has n_q(b) query rows and n_k(b) key rows: encoder self-attention on packed
 * documents (one array for both) and cross-attention (the decoder's tokens of sequence b attend the encoder's memory of sequence b).
 *
 *   q, out, out_grad, q_grad   [Tq][H][d]      token-major
 *   k, v, k_grad, v_grad       [Tk][Hkv][d]    H = G * Hkv, query head h reads kv head h / G in place
 *   q, k, v, out_grad          dtype elements (FA_DTYPE_F32 or FA_DTYPE_BF16); out, lse [H][Tq] and the gradients are fp32
 *   cu_seqlens_q, cu_seqlens_k int32 [nseq + 1] on the device.  Sequence b owns the rows s_b .. s_b + n_b - 1 of the q buffers with
 *                              s_b = clamp(cu_q[b], 0, Tq) and s_b + n_b = clamp(max(cu_q[b + 1], s_b), 0, Tq), and likewise of the
 *                              k buffers under cu_seqlens_k and Tk (the clamping rule of the packed causal library, applied to each
 *                              array against its own T): whatever the arrays hold, no access leaves the buffers.  Either count may
 *                              be 0.  Neither array is ever read on the host.  The two pointers may be one array.
 *
 * Query row i of sequence b admits EVERY key j of the same sequence, 0 <= j < n_k(b); lse is taken over those keys.
 *
 *   n_k(b) = 0, n_q(b) > 0    the sequence's query rows are exact ZEROS in out, lse and q_grad
 *   n_q(b) = 0, n_k(b) > 0    the sequence's key rows are exact ZEROS in k_grad and v_grad
 *   rows no sequence owns     (in front of cu[0], behind cu[nseq], in either buffer) ZEROS in every output that has the row
 *
 * The law that defines the calls: for every sequence with n_q, n_k >= 1, its rows of out, lse, q_grad, k_grad and v_grad are, bit
 * for bit, what the same entry points return for that sequence alone (nseq = 1, Tq = n_q, Tk = n_k).
 *
 *   Tq, Tk   packed rows, >= 1.  T * 128 * 4, Tq * H * d * 4 and Tk * H * d * 4 bytes must stay under 2 GiB, the bound of one buffer
 *            resource: T bounds every n, so the bound holds for every sequence whatever the arrays say.
 *   nseq     >= 1
 *   d        32, 64 or 128; other head sizes through zero-padded columns and softmax_scale = 1/sqrt(d)
 *   softmax_scale   0: sqrt(1/d); otherwise positive and finite.  Every score is scaled in fp32: no guard, no options.
 *
 * Workspace.  A block map has (T / 128 + nseq) entries of 32 bytes: a sequence of n rows has at most n / 128 + 1 blocks, and the
 * floors sum to at most T / 128.  An entry is eight int32: the first row and the length of the block's sequence in the q buffers,
 * the same in the k buffers, the block within the sequence (-1: unused entry), the sequence, 0, 0.  With
 * MAP(T) = align256(32 * (T / 128 + nseq)):
 *
 *     fa_mi355x_fwd_bidir_workspace_bytes = MAP(Tq)
 *     fa_mi355x_bwd_bidir_workspace_bytes = MAP(Tq) + MAP(Tk) + 3 * H * Tq * 4                                      (Hkv == H)
 *                                         = MAP(Tq) + MAP(Tk) + align256(3 * H * Tq * 4) + 2 * H * Tk * d * 4       (Hkv <  H)
 *
 *   (the map of the query blocks, 128 rows each, from cu_seqlens_q; the map of the key blocks from cu_seqlens_k, whose blocks have
 *   256 keys for bf16 at d < 128 and 128 otherwise and fill the first Tk / block + nseq entries; three row-constant vectors; the
 *   per-query-head dK and dV that the ordered group sum adds).  Both are pure functions of their arguments, 0 for sizes they cannot
 *   answer (a non-positive size, Hkv not dividing H, a result past 2^62).  The workspace must be 256-byte aligned.  The grids depend
 *   on the arguments only.
 *
 * Non-positive sizes, nseq < 1, Hkv not dividing H, an unsupported d, an unknown dtype, a bad softmax_scale, null pointers, a
 * misaligned workspace and sizes past the bounds above are FA_ERR_BAD_ARG with a message (fa_mi355x_bidir_last_error), before any
 * HIP call.  Asynchronous on `stream`, no allocation, nothing read back: every call can be captured in a graph and replayed on other
 * lengths.  No atomics and a fixed summation order: a call repeats bit for bit.
 *
 * Not in this library: a causal mask under two different arrays (bottom-right alignment) and one- or two-sided windows (both are
 * calls of their own: flash_attn_mi355x_local.h has the windows, and the causal mask as its window (-1, 0)); not built anywhere:
 * windows and sinks together, key mask, dropout and FA-1 outputs, fp8, a host-pointer reference ABI, the MFMA-slot pipelines.
 */
#ifndef FLASH_ATTN_MI355X_BIDIR_H
#define FLASH_ATTN_MI355X_BIDIR_H

#include <stddef.h>

#include "flash_attn_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t fa_mi355x_fwd_bidir_workspace_bytes(int nseq, int Tq, int Tk, int H, int Hkv, int d);
size_t fa_mi355x_bwd_bidir_workspace_bytes(int nseq, int Tq, int Tk, int H, int Hkv, int d);

/* out and lse of every sequence; zeros in the rows of keyless sequences and in the rows no sequence owns.  Launches: the schedule
 * (block map, unowned rows), the query-stationary forward. */
int fa_mi355x_fwd_bidir(const void* q, const void* k, const void* v, float* out, float* lse, const int* cu_seqlens_q,
                        const int* cu_seqlens_k, void* workspace, int nseq, int Tq, int Tk, int H, int Hkv, int d, float softmax_scale,
                        int dtype, void* stream);

/* q_grad, k_grad, v_grad from out_grad, the forward's out and lse, under the same two arrays.  Launches: the schedule (both maps,
 * unowned rows), the row constants, the key-stationary dK/dV kernel, for Hkv < H the group sum, the query-stationary dQ kernel. */
int fa_mi355x_bwd_bidir(const void* q, const void* k, const void* v, const float* out, const void* out_grad, float* q_grad,
                        float* k_grad, float* v_grad, const float* lse, const int* cu_seqlens_q, const int* cu_seqlens_k, void* workspace,
                        int nseq, int Tq, int Tk, int H, int Hkv, int d, float softmax_scale, int dtype, void* stream);

/* The message of the calling thread's last failed call into this library ("" after a call that succeeded). */
const char* fa_mi355x_bidir_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* FLASH_ATTN_MI355X_BIDIR_H */
