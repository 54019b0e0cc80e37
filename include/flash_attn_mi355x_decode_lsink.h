/*
 * flash_attn_mi355x_decode_lsink.h -- the learned-sink-logit entry points of libflash_attn_mi355x_decode.so: the decode, extend and
 * ragged calls in which one learned fp32 logit per query head joins every row's softmax as an extra column that has no value vector.
 * Included by flash_attn_mi355x_decode.h (include that one: it declares the status codes, the layouts, FA_PAGE_ROWS and
 * fa_mi355x_decode_last_error that these calls share with the others).
 */
#ifndef FLASH_ATTN_MI355X_DECODE_LSINK_H
#define FLASH_ATTN_MI355X_DECODE_LSINK_H

#include "flash_attn_mi355x_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Learned attention-sink logits against a KV cache (gpt-oss's `sinks` parameter; not the sink TOKENS of
 * flash_attn_mi355x_decode_sink.h, which are keys).  With tau = softmax_scale, or 1/sqrt(d) when that is 0, the admitted keys A(i) of
 * query i as the other calls define them (the cache length, the causal mask, the window), z_ij = tau * (q_i . k_j) and
 * a = sink_logits[h] for query head h:
 *
 *   lse_i = ln( e^a + sum_{j in A(i)} e^z_ij )
 *   P_ij  = e^(z_ij - lse_i)      (a row of P sums to less than 1: the rest went to the sink)
 *   out_i = sum_j P_ij v_j
 *
 * The logit is in logit units: it is not multiplied by tau, not rotated and no mask applies to it.  With (out0, lse0) the same call
 * without the logits, out = out0 * sigmoid(lse0 - a) and lse = lse0 + softplus(a - lse0).
 *
 *   sink_logits      fp32, one entry per QUERY head (H of them), on the device.  Every entry must be FINITE: the kernels do not check
 *                    (a = +inf would be inf - inf in the row's end), as they do not check the fp8 scales.  The kernels read it on the device where a row is
 *                    finished: no host copy, no synchronisation, so a captured call replays with the values the array holds then.
 *                    NULL: the _window call exactly, the same launches, splits, workspace and bits.
 *   empty rows       a row with no admitted key (a sequence of length 0, a row at a negative position) gives out = 0 and
 *                    lse = a, the logit itself.  Rows that the other calls neither read nor write (the unused tail of a ragged
 *                    buffer, a sequence without new tokens) stay so.
 *   causal           the logits do not need the causal mask (window = 0 with causal = 0 is a valid call); a window still does.
 *   range            no finite a and no finite score overflows: the end of a row works in log2 units on M = max(m c, a log2 e)
 *                    (m: the row's highest score, c = tau log2 e), wa = 2^(m c - M), ws = 2^(a log2 e - M), denom = l wa + ws >= 1,
 *                    out = O wa / denom, lse = M ln 2 + ln denom.
 *   append           is untouched.  A fused call appends first, then attends.
 *   Not built: logits beside attention-sink tokens, beside a soft cap and on an fp8 cache (there is no such entry point).  Rotary
 *   embeddings need nothing new: fa_mi355x_rope_append in front, then the attend-only form of these calls on q_rot.
 *
 * One entry point per call family.  Each is its family's _window prototype (flash_attn_mi355x_decode_window.h: k_new / v_new both
 * NULL or both given, block_table NULL or a table, window = 0 for no window) with `const float* sink_logits` behind `int window`, and
 * every argument check of that form applies, before any HIP call.
 *
 * Sizes.  The splits and the workspace do not depend on the logits.  fa_mi355x_{decode,extend,ragged}_window_splits and
 * fa_mi355x_{decode,extend,ragged}_window_workspace_bytes answer for these calls, with window = 0 giving the unwindowed figures;
 * there are no size queries of their own.
 *
 * How it runs (decode_split_lsink_kernel, extend_split_lsink_kernel, decode_combine_lsink_kernel: the LSINK builds of the split,
 * extend and combine kernels' bodies).  Key ranges, tiles, the page walk, the window edges, the online softmax and the partials in
 * the workspace (unnormalised, without the logit) are the other builds'.  The logit enters once per row, where the row's 1 / l is
 * formed: in the one-split store of a split kernel, or in the combine kernel behind its reduction over the splits.  A call makes
 * the launches of the same call without the logits: no pass over out, no extra launch, no atomics.  A paged call returns bit for bit
 * the slab call's result on the gathered cache.
 */
/* The decode family: 1 <= Nq <= FA_DECODE_MAX_NQ. */
int fa_mi355x_fwd_decode_lsink(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                               const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int Ncap,
                               int num_pages, int page_size, int max_pages, int d_new, int d, int layout, float softmax_scale, int causal,
                               int window, const float* sink_logits, int dtype, void* stream);

/* The extend family: any Nq >= 1. */
int fa_mi355x_fwd_extend_lsink(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                               const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int Ncap,
                               int num_pages, int page_size, int max_pages, int d_new, int d, int layout, float softmax_scale, int causal,
                               int window, const float* sink_logits, int dtype, void* stream);

/* The ragged family: q, out, k_new and v_new packed into T rows, cu_seqlens_q as in flash_attn_mi355x_decode_ragged.h. */
int fa_mi355x_fwd_ragged_lsink(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                               const int* cu_seqlens_q, const int* cache_seqlens, const int* block_table, void* workspace, int B, int H,
                               int Hkv, int T, int Ncap, int num_pages, int page_size, int max_pages, int d_new, int d, int layout,
                               float softmax_scale, int causal, int window, const float* sink_logits, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLASH_ATTN_MI355X_DECODE_LSINK_H */
