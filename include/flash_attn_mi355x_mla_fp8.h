/*
 * flash_attn_mi355x_mla_fp8.h -- MLA decode on an FP8 latent cache in libflash_attn_mi355x_mla.so: the dense step of
 * flash_attn_mi355x_mla.h, the sparse step of flash_attn_mi355x_mla_sparse.h and the append, on the cache format V3.2-class models
 * are served with.  Kernels: csrc/fa_mla_fp8.h; host: csrc/fa_mla.hip.  Errors are reported through fa_mi355x_mla_last_error().
 *
 * THE FORMAT (part of the contract).  A cache row is 656 bytes.  The cache is a byte array: a slab [B][Ncap][656], or under a block
 * table a pool [num_pages][page_size][656].
 *
 *   bytes   0 .. 511   512 OCP e4m3fn codes (gfx950's fp8 format): latent columns 0..511
 *   bytes 512 .. 527   four fp32 scales s_0..s_3; s_t belongs to columns 128 t .. 128 t + 127
 *   bytes 528 .. 655   the 64 rotated k_pe columns, bf16, not quantised
 *
 * The value of latent column c is s_{c >> 7} * e4m3(code_c).  Scales are POWERS OF TWO in [2^-100, 2^120]: the append writes only
 * such scales, and a caller who fills a cache by other means keeps to this (the caller's contract, as positive finite scales are in
 * flash_attn_mi355x_decode_fp8.h).  A violation gives wrong numbers, never a bad address.  Within that range every dequantised value
 * is exactly a bf16 value, so the kernels widen the codes to bf16 in front of LDS without rounding, and the MFMAs, the masks, the
 * softmax, the partials and the combine are the bf16 kernels' own.
 *
 * THE LAW.  An fp8 call returns BIT FOR BIT what the bf16 call (fa_mi355x_fwd_decode_mla, fa_mi355x_fwd_decode_mla_sparse) returns
 * on the cache dequantised to bf16, with the same arguments.  A paged call returns the slab call's bits; a call repeats bit for bit.
 *
 * THE APPEND.  kv_new stays bf16 [B][Nq][576].  For each new token and each tile t of its 512 latent columns:
 *   a    = the largest |x| of the tile, in fp32 (a NaN is ignored; an infinity counts)
 *   s_t  = the smallest power of two with a <= 448 s_t, clamped to [2^-100, 2^120]
 *          (an all-zero tile gets 2^-100, a tile holding an infinity 2^120; there is no special case)
 *   code = rne_e4m3(clamp(x * (1 / s_t), -448, 448)), the clamp in front of the conversion; a NaN input stores 0x7F
 * and k_pe is copied.  Placement is fa_mi355x_mla_append's: row len_b - Nq + i, nothing below row 0, page ids clamped to the pool.
 * (For a host-side restatement: with a = m 2^e, m in [0.5, 1) from frexp, s_t = 2^(e - 9) if m <= 0.875, else 2^(e - 8).)
 *
 * The split policy, fa_mi355x_decode_mla_splits / _workspace_bytes and their sparse forms answer for these calls too.
 *
 * (FP8 index keys for the indexer: flash_attn_mi355x_mla_indexer_fp8.h.)
 * Not built: fp8 queries or fp8 MFMAs for the attention itself, e5m2, scales that are not powers of two, other tile widths
 * than 128, a window, sink or cap, an extend kernel.
 */
#ifndef FLASH_ATTN_MI355X_MLA_FP8_H
#define FLASH_ATTN_MI355X_MLA_FP8_H

#include "flash_attn_mi355x_mla.h"
#include "flash_attn_mi355x_mla_sparse.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FA_MLA_FP8_ROW_BYTES 656 /* bytes of a cache row: 512 codes, 16 of scales, 128 of k_pe */

/* fa_mi355x_fwd_decode_mla on an fp8 cache: kv_cache is the byte array above, every other argument is that call's (q and kv_new
 * bf16, kv_new appended first as by fa_mi355x_mla_append_fp8).  Its refusals, with the 2 GiB bounds counted at 656 bytes per row. */
int fa_mi355x_fwd_decode_mla_fp8(const void* q, const void* kv_new, void* kv_cache, float* out, float* lse, const int* cache_seqlens,
                                 const int* block_table, void* workspace, int B, int H, int Nq, int Ncap, int num_pages, int page_size,
                                 int max_pages, float softmax_scale, int causal, void* stream);

/* fa_mi355x_fwd_decode_mla_sparse on an fp8 cache, likewise.  No byte of a row is read for an entry that is not admitted. */
int fa_mi355x_fwd_decode_mla_sparse_fp8(const void* q, const void* kv_new, void* kv_cache, const int* indices, float* out, float* lse,
                                        const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Nq,
                                        int topk, int Ncap, int num_pages, int page_size, int max_pages, float softmax_scale,
                                        int causal, void* stream);

/* The quantising append alone (THE APPEND above): kv_new bf16 [B][Nq][576] into the byte cache. */
int fa_mi355x_mla_append_fp8(const void* kv_new, void* kv_cache, const int* cache_seqlens, const int* block_table, int B, int Nq,
                             int Ncap, int num_pages, int page_size, int max_pages, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLASH_ATTN_MI355X_MLA_FP8_H */
