/*
 * flash_attn_mi355x_decode_fp8.h -- the fp8 entry points of libflash_attn_mi355x_decode.so: the decode and extend calls on a KV cache
 * of 8-bit (e4m3) elements, and the append that quantises into it.  Included by flash_attn_mi355x_decode.h (include that one: it
 * declares the status codes, the layouts, FA_PAGE_ROWS and fa_mi355x_decode_last_error that these calls share with the others).
 */
#ifndef FLASH_ATTN_MI355X_DECODE_FP8_H
#define FLASH_ATTN_MI355X_DECODE_FP8_H

#include "flash_attn_mi355x_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

/* An 8-bit KV cache: half the HBM traffic of every decode and extend call and twice the tokens in a pool of pages.
 *
 *   format      The caches (slab or page pool, either layout) hold OCP e4m3fn bytes: 1 sign, 4 exponent (bias 7) and 3 mantissa bits,
 *               no infinity, 0x7F / 0xFF are NaN, the largest finite value is 448.  This is gfx950's format (torch.float8_e4m3fn),
 *               not the e4m3fnuz of MI300.
 *   queries     q, k_new, v_new, out, lse and the workspace are what they are in the other calls.  Queries and new tokens are bf16
 *               ONLY: dtype = FA_DTYPE_F32 is FA_ERR_BAD_ARG.  `dtype` is the type of q / k_new / v_new.
 *   scales      k_scale, v_scale: device arrays of Hkv floats; the real value of a cache element of kv head h is
 *               scale[h] * e4m3_value.  NULL: all ones.  They are read on the device, so a captured graph can be replayed after a
 *               recalibration.  A scale must be positive and finite: the kernels do not check it, it is the caller's contract (as a
 *               non-decreasing cu_seqlens_q is in the ragged calls).
 *   attention   exactly the family's call on K = k_scale * k8, V = v_scale * v8.  The scales never touch an element:
 *               k_scale[hkv] multiplies the softmax scale once per workgroup (the exp2 constant, the lse, the combine kernel's
 *               weights) and v_scale[hkv] multiplies the final 1 / l (in the one-split store and in the combine kernel).  The
 *               partials in the workspace stay unscaled.
 *   bit for bit Every e4m3 value is a bf16 value, and the kernels widen a staged tile to the bf16 image the bf16 kernels compute on.
 *               An fp8 call therefore returns, with scales that are powers of two, bit for bit what the bf16 call returns on the
 *               cache cast to bf16 with softmax_scale * k_scale, times v_scale; a paged call returns the slab call's bits.
 *   bounds      Rows at or past len_b read as zero through the buffer resource, as everywhere (a zero byte is +0).  The 2 GiB bounds
 *               on one batch element of the cache, and on one page, count ONE byte per element.
 *   sizes       d in {32, 64, 128}; page_size a multiple of FA_PAGE_ROWS.
 *   splits      and the workspace are the bf16 call's for the same arguments: fa_mi355x_decode_splits_gqa /
 *               fa_mi355x_decode_workspace_bytes_gqa and fa_mi355x_extend_splits / fa_mi355x_extend_workspace_bytes answer for the
 *               fp8 calls too.
 *   append      code = rne_e4m3(clamp(fp32(x) * (1.0f / scale[h]), -448, 448)), the reciprocal and the product each correctly
 *               rounded in fp32.  The clamp sits in front of the conversion: overflow saturates to +-448 (0x7E / 0xFE), never to
 *               the NaN code.  A NaN input stores 0x7F.  Columns d_new .. d-1 of a written row are zero bytes.  Placement (row
 *               L_b - Nq + i), the rule for rows below 0 and the paged lookup with clamped ids are the other appends'.
 *   not built   a sliding window on an fp8 cache, the ragged calls on one, fp32 queries, e5m2, per-token or per-block scales, fp8 in
 *               the training forward and backward.
 *
 * One entry point per family.  Each takes, beyond the arguments of its family (flash_attn_mi355x_decode.h):
 *   k_new, v_new   both NULL: attend only.  Both given: the quantising append in front of the attention, one call (d_new as there;
 *                  ignored when they are NULL).  One of the two NULL: FA_ERR_BAD_ARG.
 *   block_table    NULL: slab caches [B][Hkv][Ncap][d] / [B][Ncap][Hkv][d] of bytes; num_pages, page_size and max_pages are
 *                  ignored.  Otherwise a paged cache exactly as flash_attn_mi355x_decode_paged.h describes it: k_cache / v_cache
 *                  are the pools, Ncap is ignored and max_pages * page_size stands for it.
 *   k_scale, v_scale   as above.
 * Every argument check of the family's unfused, fused and paged forms applies, all before any HIP call and before the caches are
 * touched.
 */
/* The decode family: 1 <= Nq <= FA_DECODE_MAX_NQ. */
int fa_mi355x_fwd_decode_fp8(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, const float* k_scale,
                             const float* v_scale, float* out, float* lse, const int* cache_seqlens, const int* block_table, void* workspace,
                             int B, int H, int Hkv, int Nq, int Ncap, int num_pages, int page_size, int max_pages, int d_new, int d,
                             int layout, float softmax_scale, int causal, int dtype, void* stream);
/* The extend family: any Nq >= 1. */
int fa_mi355x_fwd_extend_fp8(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, const float* k_scale,
                             const float* v_scale, float* out, float* lse, const int* cache_seqlens, const int* block_table, void* workspace,
                             int B, int H, int Hkv, int Nq, int Ncap, int num_pages, int page_size, int max_pages, int d_new, int d,
                             int layout, float softmax_scale, int causal, int dtype, void* stream);
/* The append alone: any Nq >= 1. */
int fa_mi355x_append_fp8(const void* k_new, const void* v_new, void* k_cache, void* v_cache, const float* k_scale, const float* v_scale,
                         const int* cache_seqlens, const int* block_table, int B, int Hkv, int Nq, int Ncap, int num_pages, int page_size,
                         int max_pages, int d_new, int d, int layout, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLASH_ATTN_MI355X_DECODE_FP8_H */
