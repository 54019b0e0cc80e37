/*
 * flash_attn_mi355x_decode_window.h -- the sliding-window entry points of libflash_attn_mi355x_decode.so: the decode, extend and
 * ragged calls in which every token sees only the last W positions.  Included by flash_attn_mi355x_decode.h (include that one: it
 * declares the status codes, the layouts, FA_PAGE_ROWS and fa_mi355x_decode_last_error that these calls share with the others).
 */
#ifndef FLASH_ATTN_MI355X_DECODE_WINDOW_H
#define FLASH_ATTN_MI355X_DECODE_WINDOW_H

#include "flash_attn_mi355x_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sliding-window (local) causal attention against a KV cache, for models whose layers see the last W positions only (Mistral's
 * `sliding_window` in every layer, alternating layers elsewhere).  Positions are the ones the other calls use: query i of batch
 * element b sits at p_i = L_b - Nq + i (ragged: L_b - nq_b + i), L_b = len_b clamped to [0, Ncap].
 *
 *   window = W >= 1:  query i admits key j  iff  p_i - W < j <= p_i        (W keys, the query's own position included: the meaning
 *                                                                          of Mistral's sliding_window)
 *
 *   causal only  window > 0 with causal = 0 is FA_ERR_BAD_ARG (a window ends at the query's position: it needs the causal mask).
 *   window < 0   FA_ERR_BAD_ARG.
 *   window = 0   the unwindowed call: the same launches, the same bits.
 *   window >= Ncap   admits every key of every row (a position is at most Ncap - 1) and IS the unwindowed call as well: the same
 *                launches, splits, workspace and bits.  The device therefore only ever computes with 1 <= W < Ncap, and no
 *                expression on it can overflow whatever the caller passes.
 *   empty rows   a row with no admissible key (p_i < 0) gives out = 0 and lse = -inf, as everywhere.
 *   lse          is taken over the admitted keys only.
 *   append       is untouched: new token i goes to row L_b - Nq + i.  A fused call appends first, then attends through the window.
 *   A ring-buffer cache of W rows is NOT what this is: the cache keeps logical rows 0 .. L_b - 1; memory is saved by releasing pages
 *   (below).  Attention-sink tokens beside the window are flash_attn_mi355x_decode_sink.h.  A window on an fp8 cache is out of
 *   scope.  The training forward and backward under this mask: flash_attn_mi355x_window.h (a library of its own).
 *
 * One entry point per call family.  Each takes, beyond the arguments of its family (flash_attn_mi355x_decode.h, _ragged.h):
 *   k_new, v_new   both NULL: attend only.  Both given: the family's append in front of the attention, one call (d_new as there;
 *                  ignored when they are NULL).  One of the two NULL: FA_ERR_BAD_ARG.
 *   block_table    NULL: slab caches [B][Hkv][Ncap][d] / [B][Ncap][Hkv][d]; num_pages, page_size and max_pages are ignored.
 *                  Otherwise a paged cache exactly as flash_attn_mi355x_decode_paged.h describes it: k_cache / v_cache are the
 *                  pools, Ncap is ignored and max_pages * page_size stands for it.
 *   window         as above.
 * Every argument check of the family's unwindowed, fused and paged forms applies, and the two window checks, all before any HIP
 * call and before the caches are touched.
 *
 * How it runs (the WINDOW builds of the split and extend kernels).  A workgroup owns a row block (32 rows of a kv head's G * Nq in
 * the decode call, 128 in the extend and ragged calls) and a key chunk.  The block's key range starts at
 *     lo = max(p_first - W + 1, 0) rounded DOWN to a multiple of 128,      p_first: the position of the block's first row
 * and split s covers [lo + s * chunk, lo + (s + 1) * chunk) below L_b (and, as before, below the block's last position + 1 in the
 * extend kernels).  lo belongs to the BLOCK, in all three calls, and is derived from len_b on the device: no host
 * synchronisation, capturable in a graph.  No 128-key tile is loaded that no row of the block can see.  Inside the first tile the
 * rows below the block's window edge are replaced by zeros before they reach LDS, a wave skips a 32-key sub-tile wholly below its
 * rows' windows, and per-element masking happens only in sub-tiles that straddle a window edge.  The admitted keys go through the
 * same products in the same order as in the unwindowed kernels.  Because lo is a multiple of 128 a tile never straddles two pages,
 * and a paged windowed call returns bit for bit the slab windowed call's result on the gathered cache.
 *
 *   span        the keys one row block can need:  span = min(Ncap, W + min(Nq, R) - 1 + 127),  R = 32 (decode) or 128 (extend;
 *               ragged with T for Nq): W keys for the first row, one more per further position of the block, at most 127 for the
 *               rounding of lo.
 *   splits      the family's own policy with span in the place of Ncap: chunk from span, nsplit = ceil(span / chunk).  A pure
 *               function of the arguments; at fixed W independent of Ncap once Ncap >= span; the unwindowed figures exactly for
 *               window = 0 and window >= Ncap.  0 for sizes the query cannot answer and for window < 0.
 *   workspace   the family's formula with that nsplit (decode / extend: B*H*nsplit*Nq*(d + 2) floats, 0 for one split; ragged: the
 *               block map plus H*nsplit*T*(d + 2) floats, never 0, 16-byte aligned).
 *
 * Page release.  With a paged cache, a page whose LAST logical row is <= n_b - W, where n_b is the number of rows sequence b holds
 * now (so that every later query sits at a position >= n_b), is below the window of every later query of b: it is then wholly
 * below lo, is never loaded, and its table entry is never read.  The caller may hand such a page to another sequence and leave
 * the entry stale or invalid; a long-running windowed sequence so holds O(W) pages, not O(length).
 */
int fa_mi355x_decode_window_splits(int B, int H, int Hkv, int Nq, int Ncap, int d, int dtype, int window);
size_t fa_mi355x_decode_window_workspace_bytes(int B, int H, int Hkv, int Nq, int Ncap, int d, int window);
/* The decode family: 1 <= Nq <= FA_DECODE_MAX_NQ. */
int fa_mi355x_fwd_decode_window(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                                const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int Ncap,
                                int num_pages, int page_size, int max_pages, int d_new, int d, int layout, float softmax_scale, int causal,
                                int window, int dtype, void* stream);

int fa_mi355x_extend_window_splits(int B, int H, int Hkv, int Nq, int Ncap, int d, int dtype, int window);
size_t fa_mi355x_extend_window_workspace_bytes(int B, int H, int Hkv, int Nq, int Ncap, int d, int window);
/* The extend family: any Nq >= 1. */
int fa_mi355x_fwd_extend_window(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                                const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int Ncap,
                                int num_pages, int page_size, int max_pages, int d_new, int d, int layout, float softmax_scale, int causal,
                                int window, int dtype, void* stream);

int fa_mi355x_ragged_window_splits(int B, int H, int Hkv, int T, int Ncap, int d, int dtype, int window);
size_t fa_mi355x_ragged_window_workspace_bytes(int B, int H, int Hkv, int T, int Ncap, int d, int window);
/* The ragged family: q, out, k_new and v_new packed into T rows, cu_seqlens_q as in flash_attn_mi355x_decode_ragged.h. */
int fa_mi355x_fwd_ragged_window(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                                const int* cu_seqlens_q, const int* cache_seqlens, const int* block_table, void* workspace, int B, int H,
                                int Hkv, int T, int Ncap, int num_pages, int page_size, int max_pages, int d_new, int d, int layout,
                                float softmax_scale, int causal, int window, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLASH_ATTN_MI355X_DECODE_WINDOW_H */
