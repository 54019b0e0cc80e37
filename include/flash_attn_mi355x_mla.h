/*
 * flash_attn_mi355x_mla.h -- C ABI of libflash_attn_mi355x_mla.so: multi-head latent attention (MLA: DeepSeek-V2 / V3 / R1, Kimi-K2)
 * decode on a latent KV cache.  Status codes are flash_attn_mi355x.h's; FA_DECODE_MAX_NQ and FA_PAGE_ROWS are
 * flash_attn_mi355x_decode.h's.  Kernels: csrc/fa_mla.h; host: csrc/fa_mla.hip.
 *
 * The cache of a layer holds ONE row of 576 bf16 columns per token, shared by all heads: the compressed latent c_kv (columns 0..511)
 * followed by the rotated k_pe (columns 512..575).  With the up-projections absorbed into q (q_lat = q_nope . W_UK per head, and
 * out . W_UV per head behind the call) a step is multi-query attention in which, for the query of head h at position p, its admitted
 * keys A = { j < len_b, and j <= p under `causal` } and tau = softmax_scale:
 *
 *   z_j = tau * sum_{c < 576} q[c] kv[j][c],   lse = ln sum_{j in A} e^z_j,   out[c] = sum_{j in A} e^(z_j - lse) kv[j][c],  c < 512
 *
 * bf16 only, d_qk = 576 and d_v = 512 exactly: the widths are not arguments.  Lengths live on the device and are clamped to
 * [0, Ncap] there; under `causal` the Nq queries are the LAST Nq positions of each sequence (query i at len_b - Nq + i).  A row with
 * no admissible key (len_b = 0) gives out = 0 and lse = -inf.  Asynchronous on `stream`, no allocation, no host synchronisation (a
 * call can be captured in a graph), no atomics, no scratch: a call repeats bit for bit, and a paged call returns bit for bit the slab
 * call's result on the gathered cache.
 *
 * How it runs.  mla_decode_split_kernel: 256 threads (one wave per SIMD, the whole register file) per (batch, key chunk, 64-row
 * block), rows in the order i * H + h.  A 64-key x 576-column tile of the cache is staged ONCE, through registers, into one 72 KB LDS
 * image that serves both products: wave (key half, row half) forms one 32 x 32 tile of the scores over all 576 columns (36 MFMAs)
 * against Q fragments held in registers, the two key halves agree on the maximum through LDS, P goes to LDS as a bf16 hi + lo pair,
 * and every wave multiplies it into its own 128 of the 512 output columns for all 64 rows (64 MFMAs): no MFMA is issued twice.
 * Several key chunks leave (o[512], m, l) partials that mla_decode_combine_kernel merges in split order.
 *
 * Not built: a sliding window, sink tokens, a soft cap, learned sink logits, the ragged family, other latent widths, a backward
 * of the absorbed form.  (A prompt is prefilled before absorption by a library of its own, flash_attn_mi355x_mla_prefill.h, which
 * also has the training backward at that head shape.)
 * (Sparse attention over per-query index lists, DeepSeek-V3.2 DSA, is in this library under a header of its own:
 * flash_attn_mi355x_mla_sparse.h; an fp8 latent cache under flash_attn_mi355x_mla_fp8.h.)
 */
#ifndef FLASH_ATTN_MI355X_MLA_H
#define FLASH_ATTN_MI355X_MLA_H

#include <stddef.h>

#include "flash_attn_mi355x_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_MLA_D_QK 576 /* columns of a cache row and of a query row */
#define FA_MLA_D_V 512  /* the leading columns of a cache row that are its value; columns of an output row */

/* The message of this thread's last failed call into this library ("" after a successful one). */
const char* fa_mi355x_mla_last_error(void);

/* One decode step.  q bf16 [B][Nq][H][576]: the absorbed q_nope . W_UK in columns 0..511, the rotated q_pe in columns 512..575.
 * kv_cache bf16 [B][Ncap][576], or, when block_table (int [B][max_pages], on the device) is given, a pool [num_pages][page_size][576]
 * whose logical capacity is max_pages * page_size (Ncap is then ignored); page_size is a multiple of FA_PAGE_ROWS, and page ids are
 * clamped to the pool on the device.  out fp32 [B][Nq][H][512]; lse fp32 [B][H][Nq], may be NULL.  kv_new bf16 [B][Nq][576] or
 * NULL: when given it is appended first (fa_mi355x_mla_append), and cache_seqlens COUNT the new tokens.  cache_seqlens int [B] on the
 * device (NULL: every sequence holds Ncap rows).  1 <= Nq <= FA_DECODE_MAX_NQ, any H >= 1.  softmax_scale is required (positive and
 * finite): 576 is not the model's head dim (DeepSeek: (128 + 64)^-1/2 times its YaRN factor), so there is no default.  workspace:
 * fa_mi355x_decode_mla_workspace_bytes() bytes, 16-byte aligned; NULL when that is 0.  q, kv_new, kv_cache and out are 16-byte aligned.
 * FA_ERR_BAD_ARG with its message, before any HIP call and before the cache is touched: sizes that are not positive, Nq above the
 * bound, a null q, kv_cache or out, a misaligned pointer, a bad softmax_scale, a bad pool geometry, a missing workspace, a cache or
 * q too large for 32-bit byte offsets.  (FA_ERR_UNSUPPORTED_D is what the Python layer's width check reports for other widths.) */
int fa_mi355x_fwd_decode_mla(const void* q, const void* kv_new, void* kv_cache, float* out, float* lse, const int* cache_seqlens,
                             const int* block_table, void* workspace, int B, int H, int Nq, int Ncap, int num_pages, int page_size,
                             int max_pages, float softmax_scale, int causal, void* stream);

/* The append alone: token i of batch element b goes to row len_b - Nq + i (len_b clamped to [0, Ncap]; rows below 0 are not
 * written), slab or paged, in 16-byte moves. */
int fa_mi355x_mla_append(const void* kv_new, void* kv_cache, const int* cache_seqlens, const int* block_table, int B, int Nq, int Ncap,
                         int num_pages, int page_size, int max_pages, void* stream);

/* Sizes: pure functions of their arguments (a paged call passes Ncap = max_pages * page_size).  The split policy is the decode
 * library's rule with one cache head and 64-row blocks: enough (batch, chunk, row block) workgroups for two rounds of the 256 CUs,
 * chunks of whole 128-key super tiles and at least 256 keys.  The workspace is 0 for one split, otherwise
 * B * H * splits * Nq * (512 + 2) floats.  Both are 0 for sizes that are not positive. */
int fa_mi355x_decode_mla_splits(int B, int H, int Nq, int Ncap);
size_t fa_mi355x_decode_mla_workspace_bytes(int B, int H, int Nq, int Ncap);

#ifdef __cplusplus
}
#endif
#endif /* FLASH_ATTN_MI355X_MLA_H */
