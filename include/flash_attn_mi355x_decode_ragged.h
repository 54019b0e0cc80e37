/*
 * flash_attn_mi355x_decode_ragged.h -- the ragged-batch entry points of libflash_attn_mi355x_decode.so: every sequence brings its own
 * number of new tokens to one call.  Included by flash_attn_mi355x_decode.h (include that one: it declares the status codes, the
 * layouts, FA_PAGE_ROWS and fa_mi355x_decode_last_error that these calls share with the uniform ones).
 */
#ifndef FLASH_ATTN_MI355X_DECODE_RAGGED_H
#define FLASH_ATTN_MI355X_DECODE_RAGGED_H

#include "flash_attn_mi355x_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One step of a serving loop: some sequences decode one token, one is part-way through a chunked prefill, some have nothing to do.
 * The new tokens of all B sequences are PACKED, sequence after sequence, into buffers of T rows, and a device array says where
 * each sequence's rows are; one call appends them and attends, with no host synchronisation (capturable in a graph at fixed T).
 *   q        dtype elements, [T][H][d]; out float [T][H][d]; lse float [H][T], may be NULL
 *   k_new, v_new   dtype elements, [T][Hkv][d_new], 1 <= d_new <= d
 *            The packed buffers are always token-major: `layout` names the caches' layout only.
 *   k_cache, v_cache   as in fa_mi355x_fwd_extend: [B][Hkv][Ncap][d] (FA_LAYOUT_BHND) or [B][Ncap][Hkv][d] (FA_LAYOUT_BNHD); the
 *            paged forms take pools and a block table exactly as flash_attn_mi355x_decode_paged.h describes them
 *   cu_seqlens_q   device int [B + 1].  Sequence b owns the packed rows s_b .. e_b - 1 with s_b = clamp(cu[b], 0, T) and
 *            e_b = clamp(cu[b+1], s_b, T), both clamped on the device: a corrupt array gives a meaningless result for that
 *            sequence, but no access leaves the buffers.  nq_b = e_b - s_b may be 0: a sequence with no tokens in this step is
 *            neither read nor written.  Packed rows at or past e_{B-1} (the unused tail of a fixed-capacity buffer) and in front
 *            of s_0 are neither read nor written, in out, lse and the caches alike.  One more thing a corrupt array can do:
 *            if it is not non-decreasing, an earlier sequence may end past e_{B-1}; a call of several splits then leaves those
 *            rows of out and lse as they were, where a one-split call writes them (meaningless either way, and in bounds).
 *   cache_seqlens  device int [B], as in the extend call: L_b = len_b clamped to [0, Ncap] COUNTS the nq_b new tokens.  NULL: every
 *            L_b = Ncap.
 *
 *   out[s_b + i, h, :] = softmax_j(scale * q[s_b + i, h, :] . k[b, h/G, j, :]) . v[b, h/G, j, :],   j < L_b
 *   causal: token i of sequence b sits at L_b - nq_b + i and sees keys j <= that position
 *   append: token i of sequence b goes to cache row L_b - nq_b + i; rows below 0 are not written; columns d_new .. d-1 are zeroed
 *
 * Everything else is the extend call's: cache rows at or past L_b contribute nothing whatever they hold, nothing past row Ncap - 1 is
 * read, a row with no admissible key returns out = 0 and lse = -inf, every score is scaled in fp32, there are no atomics and the
 * partials are combined in a fixed order (repeated calls are bitwise identical), calls are asynchronous on `stream`, allocate
 * nothing and do not synchronise with the host.  Grouped heads as everywhere: Hkv = H is the ungrouped call; one form only.  A
 * sequence's rows go through the extend kernel's tile loop unchanged, so where both calls run as one split a sequence's result is
 * bit for bit fa_mi355x_fwd_extend's on that sequence alone.
 *
 * How it runs: a small launch in front of the attention turns cu_seqlens_q into a BLOCK MAP in the workspace, one entry (sequence,
 * block within it) per 128-row block of a sequence's G * nq_b rows (row i*G + g, as in the extend call), so a row block never
 * straddles two sequences; a workgroup of the extend kernel reads its entry and is from there on the uniform kernel with nq_b for
 * Nq.  The map and the grid are sized from the arguments alone: B sequences that share T rows have at most
 * floor(G*T/128) + min(B, T) row blocks.  Unused entries are marked and their workgroups return at once.
 *   splits      the extend policy with groups = Hkv * (floor(G*T/128) + min(B, T)): a pure function of (B, H, Hkv, T, Ncap), so
 *               the results, the workspace size and a captured graph do not depend on what the device arrays hold.  KNOWN
 *               WEAKNESS: the bound counts min(B, T) blocks that a step whose tokens all sit in one of many sequences does not
 *               have, so such a step is split less than the extend call would split it.
 *   workspace   fa_mi355x_ragged_workspace_bytes(B, H, Hkv, T, Ncap, d) bytes: the map (floor(G*T/128) + min(B, T) int pairs,
 *               rounded up to 16 bytes) plus H*nsplit*T*(d + 2) floats of partials (a one-split call leaves those untouched).  It
 *               is never 0 bytes and a NULL workspace is always an error.  The pointer must be 16-BYTE ALIGNED (the map is
 *               written as 8-byte pairs, the partials behind it as 16-byte vectors).  0 for sizes the query cannot answer.
 *   paged       a paged call takes the contiguous policy and workspace at Ncap = max_pages * page_size, and returns bit for bit
 *               the contiguous ragged call's result on the gathered cache.
 * A step in which every sequence decodes one token is better served by fa_mi355x_fwd_decode_gqa, whose waves split the keys
 * of a 32-row block; here a block with few live rows leaves three of its four waves idle (measured, profiles/ragged_bench.txt:
 * B = 32 at length 4096, d = 128, 8 of 32 heads cached: 0.122 against 0.111 ms in bf16, 0.623 against 0.260 ms in fp32).
 *
 * FA_ERR_BAD_ARG / FA_ERR_UNSUPPORTED_D, with a message naming the argument, before any HIP call and before the caches are
 * touched: everything fa_mi355x_fwd_extend and fa_mi355x_extend_append reject, with T in the place of Nq (non-positive sizes,
 * H not a multiple of Hkv, an unknown layout or dtype, null pointers, d not 32 / 64 / 128, d_new outside 1 .. d, a bad
 * softmax_scale, G*T >= 2^25 rows, q as a whole (T*H*d elements) or a batch element or page of the cache of 2 GiB or more, workgroup
 * counts that do not fit an unsigned int); the paged checks; a null cu_seqlens_q; a null workspace. */
int fa_mi355x_ragged_splits(int B, int H, int Hkv, int T, int Ncap, int d, int dtype);
size_t fa_mi355x_ragged_workspace_bytes(int B, int H, int Hkv, int T, int Ncap, int d);
int fa_mi355x_fwd_ragged(const void* q, const void* k_cache, const void* v_cache, float* out, float* lse, const int* cu_seqlens_q,
                         const int* cache_seqlens, void* workspace, int B, int H, int Hkv, int T, int Ncap, int d, int layout,
                         float softmax_scale, int causal, int dtype, void* stream);
int fa_mi355x_ragged_append(const void* k_new, const void* v_new, void* k_cache, void* v_cache, const int* cu_seqlens_q,
                            const int* cache_seqlens, int B, int Hkv, int T, int Ncap, int d_new, int d, int layout, int dtype,
                            void* stream);
/* fa_mi355x_ragged_append followed, on the same stream, by exactly fa_mi355x_fwd_ragged with the same arguments. */
int fa_mi355x_fwd_ragged_append(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                                const int* cu_seqlens_q, const int* cache_seqlens, void* workspace, int B, int H, int Hkv, int T,
                                int Ncap, int d_new, int d, int layout, float softmax_scale, int causal, int dtype, void* stream);

/* The paged forms: block_table directly after cache_seqlens, (num_pages, page_size, max_pages) where Ncap stood. */
int fa_mi355x_fwd_ragged_paged(const void* q, const void* k_pool, const void* v_pool, float* out, float* lse, const int* cu_seqlens_q,
                               const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv, int T,
                               int num_pages, int page_size, int max_pages, int d, int layout, float softmax_scale, int causal,
                               int dtype, void* stream);
int fa_mi355x_ragged_append_paged(const void* k_new, const void* v_new, void* k_pool, void* v_pool, const int* cu_seqlens_q,
                                  const int* cache_seqlens, const int* block_table, int B, int Hkv, int T, int num_pages, int page_size,
                                  int max_pages, int d_new, int d, int layout, int dtype, void* stream);
int fa_mi355x_fwd_ragged_append_paged(const void* q, const void* k_new, const void* v_new, void* k_pool, void* v_pool, float* out,
                                      float* lse, const int* cu_seqlens_q, const int* cache_seqlens, const int* block_table,
                                      void* workspace, int B, int H, int Hkv, int T, int num_pages, int page_size, int max_pages,
                                      int d_new, int d, int layout, float softmax_scale, int causal, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLASH_ATTN_MI355X_DECODE_RAGGED_H */
