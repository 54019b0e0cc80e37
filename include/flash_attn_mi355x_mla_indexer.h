/*
 * flash_attn_mi355x_mla_indexer.h -- the lightning indexer of DeepSeek-V3.2 sparse attention (DSA) in libflash_attn_mi355x_mla.so: it
 * scores every cached position for each new token and picks the top-k index lists that fa_mi355x_fwd_decode_mla_sparse attends.
 * Kernels: csrc/fa_mla_indexer.h; host: csrc/fa_mla.hip.  Status codes are flash_attn_mi355x_mla.h's and errors are reported through
 * fa_mi355x_mla_last_error().
 *
 * q_idx bf16 [B][Nq][HI][128] (1 <= Nq <= 128, 1 <= HI <= 128; DeepSeek-V3.2: HI = 64), weights fp32 [B][Nq][HI] (any sign; the
 * caller folds HI^-1/2 and the softmax scale in), index keys bf16 in a slab kidx_cache [B][Ncap][128], or with block_table
 * [B][max_pages] a pool [num_pages][page_size][128] (page_size a multiple of 128 rows; the latent cache's own table).  cache_seqlens
 * int32 [B] is read on the device and clamped to [0, Ncap] (NULL: Ncap); a paged call's Ncap is max_pages * page_size.
 *
 *   I[b,i,s] = sum_h weights[b,i,h] * max(0, sum_c q_idx[b,i,h,c] * kidx[b,s,c])
 *
 * Position s is ADMITTED iff 0 <= s < len_b and, under `causal`, s <= len_b - Nq + i.  scores fp32 [B][Nq][Ncap]: a position below
 * len_b receives its score, or -inf when it is not admitted; positions at or past len_b are neither read nor written.
 * Selection for row (b, i): the admitted positions by score descending (compared as fp32 values, -0 = +0), equal scores by position
 * ascending; the first min(topk, admitted) of them go to indices[b][i][:] (int32 [B][Nq][topk], topk a positive multiple of 64) in
 * ASCENDING POSITION order and the rest of the row is -1.  -inf and NaN scores are never selected.  The list is a pure function of
 * the score bits: no atomic decides an order and a call repeats bit for bit; a paged call returns the slab call's bits.
 * kidx_new bf16 [B][Nq][128] (may be NULL): written first, inside the call, token i to row len_b - Nq + i (the lengths COUNT the new
 * tokens; a negative row is not written): fa_mi355x_mla_append's rule.  No host synchronisation: every call can be captured in a graph.
 *
 * How it runs.  mla_index_scores_kernel: 256 threads per (batch, group of up to 4 tokens, chunk of keys).  Heads are the MFMA's rows
 * and keys its columns, so a lane owns one key: ReLU and the weighted head sum are in-lane FMAs and one lane <-> lane + 32 add.  A lane
 * streams 128 contiguous bytes of its key's row straight into MFMA fragments (no LDS for keys, the next tile in flight); Q_idx and the
 * weights of the group's tokens lie in LDS and a tile's key fragments serve all of them.  mla_index_topk_kernel: 1024 threads per
 * (b, i) row, a radix select over the order-preserving image of the score in three histogram passes (LDS bins), then a compaction by
 * prefix sums in two more.  mla_index_append_kernel: 16-byte moves.
 *
 * FP8 index keys: flash_attn_mi355x_mla_indexer_fp8.h, the same calls on 144-byte rows.
 * Not built: a fused score + select launch, index dims other than 128, an indexer for prefill / extend, training.
 */
#ifndef FLASH_ATTN_MI355X_MLA_INDEXER_H
#define FLASH_ATTN_MI355X_MLA_INDEXER_H

#include <stddef.h>

#include "flash_attn_mi355x_mla.h"

#ifdef __cplusplus
extern "C" {
#endif

/* FA_ERR_BAD_ARG with its message, before any HIP call and before any buffer is touched, for every entry point that takes the
 * argument: B, HI or Nq not positive, Nq > 128, HI > 128; a pool whose num_pages, page_size or max_pages is not positive, page_size
 * not a multiple of 128, max_pages * page_size past an int; Ncap not positive, a slab batch element of 2 GiB or more; a null pointer
 * (kidx_new and cache_seqlens may be NULL) or one that is not 16-byte aligned (cache_seqlens, block_table, indices: 4-byte); topk not
 * a positive multiple of 64; B * Nq * topk or Ncap at or above 2^30 entries; more workgroups than a launch holds. */

/* scores[b][i][s] for every s < len_b.  kidx_new non-NULL: appended first. */
int fa_mi355x_mla_index_scores(const void* q_idx, const float* weights, const void* kidx_new, void* kidx_cache, float* scores,
                               const int* cache_seqlens, const int* block_table, int B, int HI, int Nq, int Ncap, int num_pages,
                               int page_size, int max_pages, int causal, void* stream);

/* indices[b][i][:] from scores[b][i][0 .. len_b): whatever is not -inf or NaN there is admitted. */
int fa_mi355x_mla_index_topk(const float* scores, int* indices, const int* cache_seqlens, int B, int Nq, int Ncap, int topk,
                             void* stream);

/* The new tokens' index keys into the cache. */
int fa_mi355x_mla_index_append(const void* kidx_new, void* kidx_cache, const int* cache_seqlens, const int* block_table, int B, int Nq,
                               int Ncap, int num_pages, int page_size, int max_pages, void* stream);

/* Append (kidx_new non-NULL), scores and top-k in one call: the three launches above, on `scores` as the caller's buffer of
 * fa_mi355x_mla_indexer_scores_bytes() bytes. */
int fa_mi355x_mla_indexer(const void* q_idx, const float* weights, const void* kidx_new, void* kidx_cache, float* scores, int* indices,
                          const int* cache_seqlens, const int* block_table, int B, int HI, int Nq, int topk, int Ncap, int num_pages,
                          int page_size, int max_pages, int causal, void* stream);

/* Sizes: pure functions of their arguments, 0 for sizes that are not positive.  scores: B * Nq * Ncap floats.  chunks: the key chunks
 * a sequence is cut into by the score launch: B * ceil(Nq / group) groups of workgroups (group = min(Nq, 4, 8 / ceil(HI / 32))
 * tokens), enough chunks for two rounds of two workgroups on each of the 256 CUs, whole 128-key steps and at least 512 keys. */
size_t fa_mi355x_mla_indexer_scores_bytes(int B, int Nq, int Ncap);
int fa_mi355x_mla_index_chunks(int B, int HI, int Nq, int Ncap);

#ifdef __cplusplus
}
#endif
#endif /* FLASH_ATTN_MI355X_MLA_INDEXER_H */
