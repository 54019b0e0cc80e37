/*
 * flash_attn_mi355x_decode_softcap.h -- the logit soft-capping entry points of libflash_attn_mi355x_decode.so: the decode, extend and
 * ragged calls in which every score passes through softcap * tanh(score / softcap).  Included by flash_attn_mi355x_decode.h (include
 * that one: it declares the status codes, the layouts, FA_PAGE_ROWS and fa_mi355x_decode_last_error that these calls share with the
 * others).
 */
#ifndef FLASH_ATTN_MI355X_DECODE_SOFTCAP_H
#define FLASH_ATTN_MI355X_DECODE_SOFTCAP_H

#include "flash_attn_mi355x_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Logit soft-capping against a KV cache (Gemma-2's attn_logit_softcapping = 50, Grok-1's 30, `softcap` of the flash-attention
 * interface).  With tau = softmax_scale, or 1/sqrt(d) when that is 0, and the admitted keys j of query i as the other calls define
 * them (the cache length, the causal mask, the window):
 *
 *   z_ij = softcap * tanh(tau * (q_i . k_j) / softcap)
 *   P    = softmax of z over the admitted keys,    out = P . V,    lse = ln sum_j exp(z_ij)
 *
 * The cap acts on every score BEFORE the masks: a key that is not admitted stays out, whatever the cap (a mask applied first would
 * come out of the cap as -softcap, an admitted key).  |z| <= softcap, so lse <= softcap + ln(keys).
 *
 *   softcap = 0      the _window call exactly: the same launches, splits, workspace and bits.
 *   softcap < 0, NaN or infinite   FA_ERR_BAD_ARG, checked with the window checks: before any HIP call and before the caches are
 *                    touched.
 *   causal           a cap does not need the causal mask (window = 0 with causal = 0 is a valid capped call); a window still does.
 *   empty rows       a row with no admissible key gives out = 0 and lse = -inf, as everywhere.
 *   append           is untouched.  A fused call appends first, then attends.
 *   Not built: a cap beside attention-sink tokens and a cap on an fp8 cache (there is no such entry point).  The training forward
 *   and backward under a cap are flash_attn_mi355x_window_softcap.h, in another library.  Rotary embeddings need nothing new: fa_mi355x_rope_append in front, then the attend-only form of these
 *   calls on q_rot.
 *
 * One entry point per call family.  Each is its family's _window prototype (flash_attn_mi355x_decode_window.h: k_new / v_new both
 * NULL or both given, block_table NULL or a table, window = 0 for no window) with `float softcap` behind `int window`, and every
 * argument check of that form applies.
 *
 * Sizes.  The splits and the workspace do not depend on the cap.  fa_mi355x_{decode,extend,ragged}_window_splits and
 * fa_mi355x_{decode,extend,ragged}_window_workspace_bytes answer for these calls, with window = 0 giving the unwindowed figures;
 * there are no size queries of their own.
 *
 * How it runs (decode_split_softcap_kernel, extend_split_softcap_kernel: the SOFTCAP builds of the split and extend kernels'
 * bodies).  With k2 = 2 log2(e) tau / softcap, computed once per workgroup, a score s becomes
 *     t = exp2(s * k2),    z = softcap - 2 softcap / (t + 1)
 * right after the QK products: one v_exp_f32 and one v_rcp_f32 per score (gfx950 has no tanh instruction).  It saturates without a
 * special case (t = inf: z = +softcap; t = 0: z = -softcap) and no finite score gives a NaN.  From there on the scores are the
 * logits: the online softmax runs with tau = 1, the partial maxima of a split call are in capped-logit units, and the combine launch
 * is the existing decode_combine_kernel with tau = 1 in its argument.  Key ranges, tiles, the page walk and the window edges are the
 * other builds'; a paged capped call returns bit for bit the slab capped call's result on the gathered cache.
 */
/* The decode family: 1 <= Nq <= FA_DECODE_MAX_NQ. */
int fa_mi355x_fwd_decode_softcap(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                                 const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int Ncap,
                                 int num_pages, int page_size, int max_pages, int d_new, int d, int layout, float softmax_scale, int causal,
                                 int window, float softcap, int dtype, void* stream);

/* The extend family: any Nq >= 1. */
int fa_mi355x_fwd_extend_softcap(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                                 const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int Ncap,
                                 int num_pages, int page_size, int max_pages, int d_new, int d, int layout, float softmax_scale, int causal,
                                 int window, float softcap, int dtype, void* stream);

/* The ragged family: q, out, k_new and v_new packed into T rows, cu_seqlens_q as in flash_attn_mi355x_decode_ragged.h. */
int fa_mi355x_fwd_ragged_softcap(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                                 const int* cu_seqlens_q, const int* cache_seqlens, const int* block_table, void* workspace, int B, int H,
                                 int Hkv, int T, int Ncap, int num_pages, int page_size, int max_pages, int d_new, int d, int layout,
                                 float softmax_scale, int causal, int window, float softcap, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLASH_ATTN_MI355X_DECODE_SOFTCAP_H */
