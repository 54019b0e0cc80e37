/*
 * flash_attn_mi355x_decode_paged.h -- the paged KV-cache entry points of libflash_attn_mi355x_decode.so.  Included by
 * flash_attn_mi355x_decode.h (include that one: it declares the status codes, the layouts, the size queries and
 * fa_mi355x_decode_last_error that these calls share with the contiguous ones).
 */
#ifndef FLASH_ATTN_MI355X_DECODE_PAGED_H
#define FLASH_ATTN_MI355X_DECODE_PAGED_H

#include "flash_attn_mi355x_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The cache of a layer is a POOL of pages shared by every sequence, and a block table says which pages hold a
 * sequence's rows, so a server reserves memory by the page as sequences grow, hands a finished sequence's pages to another one, and
 * lets sequences that share a prefix point at the same pages.
 *   k_pool, v_pool   dtype elements, num_pages pages of page_size rows, contiguous (pages page_size*Hkv*d elements apart): a page is
 *            [page_size][Hkv][d] (FA_LAYOUT_BNHD) or [Hkv][page_size][d] (FA_LAYOUT_BHND).  q, out and lse are exactly as in the
 *            contiguous call of the same layout.
 *   block_table   device int [B][max_pages], row-major: logical cache row j of batch element b is row j % page_size of page
 *            block_table[b][j / page_size].
 *   page_size   a positive multiple of FA_PAGE_ROWS (128), not necessarily a power of two.
 * The logical capacity is Ncap = max_pages * page_size, and everything the contiguous calls say about Ncap and cache_seqlens holds
 * with it: len_b is clamped to [0, Ncap], NULL lengths mean Ncap, causal query i sits at len_b - Nq + i, and rows at or past len_b
 * contribute nothing whatever they hold.  Table entries at or past ceil(len_b / page_size) are never read and may hold anything.  A
 * page id that is read is clamped on the device to [0, num_pages - 1]: a corrupt table gives a meaningless result for that sequence,
 * but no access leaves the pool.  Two table rows, or two entries, may name the same page (a shared prefix); the attention only reads.
 * The APPEND does not guard against writing a shared page: a sequence whose new tokens land in a page another sequence also names
 * overwrites that sequence's rows.  That is the caller's contract (give a sequence its own page from the first row it writes).
 *
 * A paged call uses the contiguous call's split count, chunk size and workspace for the same (B, H, Hkv, Nq, Ncap = max_pages *
 * page_size, d): size the workspace with fa_mi355x_decode_workspace_bytes_gqa / fa_mi355x_extend_workspace_bytes and read the split
 * count from fa_mi355x_decode_splits_gqa / fa_mi355x_extend_splits with that Ncap (there are no paged size queries).  A page boundary
 * only changes where a 128-key tile is fetched from (page_size is a multiple of the tile, and every chunk starts on one), so a paged
 * call returns BIT FOR BIT what the contiguous call returns on the gathered cache, for any table.
 *
 * The six entry points are the _gqa decode / extend forms above with block_table directly after cache_seqlens and (num_pages,
 * page_size, max_pages) where Ncap stood; Hkv = H is the ungrouped call.  They keep the contiguous calls' properties: asynchronous on
 * `stream`, no allocation, no host synchronisation, capturable in a graph, no atomics; the fused forms are the append followed by the
 * attention on the same stream.  Every check of the contiguous form applies with Ncap = max_pages * page_size, except that the 2 GiB
 * bound on a batch element of the cache becomes one on a PAGE (page_size*Hkv*d elements; page addresses are 64-bit, so the pool as a
 * whole may be of any size).  In addition FA_ERR_BAD_ARG, with a message naming the argument, before any HIP call and before the
 * pools are touched: a null block_table; non-positive num_pages, page_size or max_pages; page_size not a multiple of FA_PAGE_ROWS;
 * max_pages * page_size (plus one 128-row tile) not fitting an int. */
#define FA_PAGE_ROWS 128
int fa_mi355x_fwd_decode_paged(const void* q, const void* k_pool, const void* v_pool, float* out, float* lse, const int* cache_seqlens,
                               const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int num_pages, int page_size,
                               int max_pages, int d, int layout, float softmax_scale, int causal, int dtype, void* stream);
int fa_mi355x_decode_append_paged(const void* k_new, const void* v_new, void* k_pool, void* v_pool, const int* cache_seqlens,
                                  const int* block_table, int B, int Hkv, int Nq, int num_pages, int page_size, int max_pages, int d_new,
                                  int d, int layout, int dtype, void* stream);
int fa_mi355x_fwd_decode_append_paged(const void* q, const void* k_new, const void* v_new, void* k_pool, void* v_pool, float* out,
                                      float* lse, const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv,
                                      int Nq, int num_pages, int page_size, int max_pages, int d_new, int d, int layout,
                                      float softmax_scale, int causal, int dtype, void* stream);
int fa_mi355x_fwd_extend_paged(const void* q, const void* k_pool, const void* v_pool, float* out, float* lse, const int* cache_seqlens,
                               const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int num_pages, int page_size,
                               int max_pages, int d, int layout, float softmax_scale, int causal, int dtype, void* stream);
int fa_mi355x_extend_append_paged(const void* k_new, const void* v_new, void* k_pool, void* v_pool, const int* cache_seqlens,
                                  const int* block_table, int B, int Hkv, int Nq, int num_pages, int page_size, int max_pages, int d_new,
                                  int d, int layout, int dtype, void* stream);
int fa_mi355x_fwd_extend_append_paged(const void* q, const void* k_new, const void* v_new, void* k_pool, void* v_pool, float* out,
                                      float* lse, const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv,
                                      int Nq, int num_pages, int page_size, int max_pages, int d_new, int d, int layout,
                                      float softmax_scale, int causal, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLASH_ATTN_MI355X_DECODE_PAGED_H */
