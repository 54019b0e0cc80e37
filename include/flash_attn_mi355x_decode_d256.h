/*
 * flash_attn_mi355x_decode_d256.h -- the head-dim-256 entry points of libflash_attn_mi355x_decode.so: the decode and extend calls, and
 * the append, on KV caches whose rows hold d = 256 bf16 elements (Gemma-2 2B / 9B, most of Gemma-3).  Included by
 * flash_attn_mi355x_decode.h (include that one: it declares the status codes, the layouts, FA_PAGE_ROWS and
 * fa_mi355x_decode_last_error that these calls share with the others).
 */
#ifndef FLASH_ATTN_MI355X_DECODE_D256_H
#define FLASH_ATTN_MI355X_DECODE_D256_H

#include "flash_attn_mi355x_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The semantics are those of the calls in flash_attn_mi355x_decode_softcap.h, argument by argument: optional k_new / v_new (both NULL:
 * attend only; both given: appended first, rows of d_new <= 256 elements, zeros in columns d_new .. 255), block_table NULL (slabs of
 * Ncap rows) or a table (a pool of pages, page_size a multiple of FA_PAGE_ROWS; Ncap is then ignored), `window` (0: none; needs
 * causal), `softcap` (0: none; finite and not negative), grouped-query heads (H a multiple of Hkv), lengths on the device.
 *
 *   d        256 exactly (FA_ERR_UNSUPPORTED_D otherwise); d_new in 1 .. 256.
 *   dtype    FA_DTYPE_BF16 only (FA_DTYPE_F32: FA_ERR_BAD_ARG).
 *   Every bad argument is answered before any HIP call and before the caches are touched, with its message in
 *   fa_mi355x_decode_last_error.  window = 0 or >= Ncap and softcap = 0 make the launches and the bits of the call without them.
 *   A paged call returns bit for bit the slab call's result on the gathered cache; a call repeats bit for bit (no atomics).
 *   Not built at d = 256: the ragged family, fp8 caches, sink tokens, learned sink logits, fused rotary embeddings, fp32 caches,
 *   other d in (128, 256) (pad the rows to 256 with zero columns and pass softmax_scale), and the training forward / backward.
 *
 * How it runs (csrc/fa_decode_d256.h).  The 128-key super tile, the page walk, the chunk rounding and the split policy are the other
 * calls'.  decode_split_d256_kernel: 512 threads per (batch * kv head, key chunk, 32-row block); wave w takes key quarter w & 3 of a
 * staged tile for S over the full d and the output columns 128 (w >> 2) .. + 127 for P.V; the eight partials merge through LDS in a
 * fixed order.  extend_split_d256_kernel: 256 threads per 128-row block, a wave owns 32 rows and all 256 columns, K / V staged as
 * 64-key halves of the super tile.  Several splits meet in decode_combine_d256_kernel in a fixed order. */

/* The decode family: 1 <= Nq <= FA_DECODE_MAX_NQ. */
int fa_mi355x_fwd_decode_d256(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                              const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int Ncap,
                              int num_pages, int page_size, int max_pages, int d_new, int d, int layout, float softmax_scale, int causal,
                              int window, float softcap, int dtype, void* stream);

/* The extend family: any Nq >= 1. */
int fa_mi355x_fwd_extend_d256(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                              const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int Ncap,
                              int num_pages, int page_size, int max_pages, int d_new, int d, int layout, float softmax_scale, int causal,
                              int window, float softcap, int dtype, void* stream);

/* The append alone, any Nq >= 1, slab (block_table NULL) or paged: fa_mi355x_extend_append's placement and zero columns. */
int fa_mi355x_append_d256(const void* k_new, const void* v_new, void* k_cache, void* v_cache, const int* cache_seqlens,
                          const int* block_table, int B, int Hkv, int Nq, int Ncap, int num_pages, int page_size, int max_pages,
                          int d_new, int d, int layout, int dtype, void* stream);

/* Sizes: the split policy of the other calls on d = 256 (the _window queries' prototypes; window = 0: none).  The workspace does not
 * depend on the cap.  0 for arguments the policy cannot answer, d != 256 included. */
int fa_mi355x_decode_d256_splits(int B, int H, int Hkv, int Nq, int Ncap, int d, int dtype, int window);
size_t fa_mi355x_decode_d256_workspace_bytes(int B, int H, int Hkv, int Nq, int Ncap, int d, int window);
int fa_mi355x_extend_d256_splits(int B, int H, int Hkv, int Nq, int Ncap, int d, int dtype, int window);
size_t fa_mi355x_extend_d256_workspace_bytes(int B, int H, int Hkv, int Nq, int Ncap, int d, int window);

#ifdef __cplusplus
}
#endif
#endif /* FLASH_ATTN_MI355X_DECODE_D256_H */
