/*
 * flash_attn_mi355x_mla_sparse.h -- sparse MLA decode (DeepSeek-V3.2 sparse attention, DSA) in libflash_attn_mi355x_mla.so: the
 * latent cache, the absorbed form and the status codes of flash_attn_mi355x_mla.h, but every query token attends only the cache
 * positions its index list names (an indexer's top-k; k = 2048 in the released models).  Kernel: csrc/fa_mla_sparse.h; host:
 * csrc/fa_mla.hip.  Errors are reported through fa_mi355x_mla_last_error().
 *
 * indices: int32 [B][Nq][topk] on the device, contiguous, topk a multiple of 64 and >= 64.  Entry e of query (b, i) names logical
 * position j = indices[b][i][e] of sequence b (through the block table when the cache is paged).  It is ADMITTED iff 0 <= j < len_b,
 * and under `causal` also j <= len_b - Nq + i (len_b clamped to [0, Ncap] on the device).  Any other value is an entry that is not
 * there: -1 padding, any negative value, values >= len_b, values >= Ncap, wherever it sits in the list.  An entry is a key of its
 * own: a position named twice counts twice; nothing deduplicates or sorts.  With A the admitted entries and tau = softmax_scale:
 *
 *   z_e = tau * sum_{c < 576} q[c] kv[j_e][c],   lse = ln sum_{e in A} e^z_e,   out[c] = sum_{e in A} e^(z_e - lse) kv[j_e][c],  c < 512
 *
 * A query with no admitted entry gives out = 0 and lse = -inf.  No cache row and no page id is read for an entry that is not
 * admitted (the compare comes before any address arithmetic, so no index value makes the kernel read outside the cache), and such
 * an entry contributes exactly 0 whatever the memory it would have named holds.  No atomics, no scratch, no host synchronisation
 * (a call can be captured in a graph); a call repeats bit for bit, and a paged call returns the slab call's bits on the gathered cache.
 *
 * How it runs.  mla_sparse_split_kernel: 256 threads per (batch, query token, 64-head block, chunk of the token's list).  All 64
 * rows of a block belong to one token, so the validity of a 64-entry tile is one wave-uniform 64-bit mask (a ballot of the compare):
 * S is masked by bit tests, and a key half, a 16-key step or a whole tile without an admitted entry skips its MFMAs.  The rows of a
 * tile are gathered into the dense kernel's 72 KB image (slab: buffer loads, a row that is not admitted at the resource's size;
 * paged: 64-bit global loads, such a row zeroed in registers), with the chain index -> page id -> row -> LDS pipelined in registers
 * over three tiles.  The products, the partial layout and mla_decode_combine_kernel are flash_attn_mi355x_mla.h's.
 *
 * The indices are the caller's, or the indexer's of flash_attn_mi355x_mla_indexer.h.  Not built: a sparse prefill / extend kernel,
 * other topk granularities than 64, a window, cap or sink beside the indices.
 */
#ifndef FLASH_ATTN_MI355X_MLA_SPARSE_H
#define FLASH_ATTN_MI355X_MLA_SPARSE_H

#include <stddef.h>

#include "flash_attn_mi355x_mla.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One sparse decode step.  q, kv_new, kv_cache, out, lse, cache_seqlens, block_table, the pool geometry, softmax_scale and causal
 * are fa_mi355x_fwd_decode_mla's (kv_new non-NULL: appended first, then attended).  indices int32 [B][Nq][topk] as above, 4-byte
 * aligned.  workspace: fa_mi355x_decode_mla_sparse_workspace_bytes() bytes, 16-byte aligned; NULL when that is 0.
 * FA_ERR_BAD_ARG with its message, before any HIP call and before the cache is touched: every refusal of fa_mi355x_fwd_decode_mla,
 * and null or misaligned indices, topk that is not a positive multiple of 64, B * Nq * topk at or above 2^31, a pool of 2^31 rows
 * or more. */
int fa_mi355x_fwd_decode_mla_sparse(const void* q, const void* kv_new, void* kv_cache, const int* indices, float* out, float* lse,
                                    const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Nq, int topk,
                                    int Ncap, int num_pages, int page_size, int max_pages, float softmax_scale, int causal,
                                    void* stream);

/* Sizes: pure functions of their arguments.  The dense rule applied to the index list: B * Nq * ceil(H / 64) groups of workgroups,
 * enough chunks for two rounds of the 256 CUs, chunks of whole 128-entry multiples and at least 256 entries.  The workspace is 0
 * for one split, otherwise B * H * splits * Nq * (512 + 2) floats.  Both are 0 for sizes that are not positive. */
int fa_mi355x_decode_mla_sparse_splits(int B, int H, int Nq, int topk);
size_t fa_mi355x_decode_mla_sparse_workspace_bytes(int B, int H, int Nq, int topk);

#ifdef __cplusplus
}
#endif
#endif /* FLASH_ATTN_MI355X_MLA_SPARSE_H */
