/*
 * flash_attn_mi355x_decode_sink.h -- the attention-sink entry points of libflash_attn_mi355x_decode.so: the sliding-window decode,
 * extend and ragged calls in which every token also keeps the first S positions of its sequence.  Included by
 * flash_attn_mi355x_decode.h (include that one: it declares the status codes, the layouts, FA_PAGE_ROWS and
 * fa_mi355x_decode_last_error that these calls share with the others).
 */
#ifndef FLASH_ATTN_MI355X_DECODE_SINK_H
#define FLASH_ATTN_MI355X_DECODE_SINK_H

#include "flash_attn_mi355x_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A pure sliding window loses the first positions of a sequence, which every later token leans on (the attention sinks of
 * StreamingLLM); a long-running windowed generation keeps them visible for good.  `sink` = S >= 0 is a second integer beside
 * `window` = W of flash_attn_mi355x_decode_window.h; positions are the ones every call uses: query i of batch element b sits at
 * p = L_b - Nq + i (ragged: L_b - nq_b + i), L_b = len_b clamped to [0, Ncap].
 *
 *   query at p admits key j   iff   j <= p   and   (j > p - W   or   j < S)
 *
 *   A key that is both a sink and inside the window counts once.  lse is taken over the admitted keys.  A row with p < 0 is empty
 *   (out = 0, lse = -inf), as everywhere.  The append is untouched: a fused call appends first, then attends.
 *   sink < 0     FA_ERR_BAD_ARG (the size queries return 0).
 *   sink = 0     the windowed call exactly: the same launches, splits, workspace and bits.
 *   window = 0, window >= Ncap or sink >= Ncap   every j <= p is admitted: the unwindowed call exactly, the same launches, splits,
 *                workspace and bits.  The device therefore only ever computes with 1 <= W < Ncap and 1 <= S < Ncap.
 *   causal only  window > 0 with causal = 0 is FA_ERR_BAD_ARG, the window's own check.
 *   Sinks are a mask on the logical rows of the cache.  NOT built: sinks on an fp8 cache; learned sink logits (gpt-oss); a
 *   re-assignment of positions inside the cache (StreamingLLM's other half: the rotary calls of _rope.h keep a token's position); a ring-buffer cache;
 *   (The training forward and backward under this mask are flash_attn_mi355x_window.h, a library of its own.)
 *
 * One entry point per call family, each with the arguments of its windowed form and `sink` directly after `window`; k_new / v_new
 * (both NULL: attend only) and block_table (NULL: slab caches) are optional as there.  Every argument check of the windowed forms
 * applies, and the check of sink, all before any HIP call and before the caches are touched.
 *
 * How it runs (the sink builds of the split and extend kernels: kernels of their own, the others are the code they were).  A row
 * block's key range is two ranges walked as one, in ascending key order.  With lo the start of the window's range (_window.h):
 *     n_s = min(ceil(S / 128), lo / 128) sink tiles: the 128-key tiles 0 .. n_s - 1, those that hold a sink key and lie wholly
 *           below lo; then the window's tiles from lo on.
 * A tile at or above lo that holds keys below S admits them through the mask (early in a sequence, while the window still reaches
 * down to the sinks), so no key is counted twice.  The splits cut the VIRTUAL axis on which the two ranges are adjacent: split s
 * covers the virtual keys [s * chunk, (s + 1) * chunk), so the splits stay balanced, the jump from the last sink tile to lo may
 * fall inside a chunk or on a chunk boundary, and a split past the end leaves the empty partial.  Staged rows j with
 * S <= j < the block's window edge, which no row of the block admits and which may hold anything (a released page), become zeros
 * before they reach LDS: the tail of the last sink tile and the head of the first window tile.  A paged call reads no table entry
 * strictly between the last sink tile's page and lo's page, and returns bit for bit the slab call's result on the gathered cache.
 *
 *   span        span = min(Ncap, ceil(S / 128) * 128 + W + min(Nq, R) - 1 + 127),  R = 32 (decode) or 128 (extend; ragged with T
 *               for Nq): the window's span plus the sink tiles; Ncap in the cases that are the unwindowed call.
 *   splits      the family's own policy with span in the place of Ncap, as in _window.h.  A pure function of the arguments; the
 *               windowed figures for sink = 0, the unwindowed ones in the cases above.  0 for sizes the query cannot answer and for
 *               window < 0 or sink < 0.
 *   workspace   the family's formula with that nsplit, as in _window.h.
 *
 * Page release.  The pages that hold the first S rows (the first ceil(S / page_size) table entries) must stay; every other page
 * wholly below the window of every later query may be released as _window.h describes, its entry left stale or invalid.
 */
int fa_mi355x_decode_sink_splits(int B, int H, int Hkv, int Nq, int Ncap, int d, int dtype, int window, int sink);
size_t fa_mi355x_decode_sink_workspace_bytes(int B, int H, int Hkv, int Nq, int Ncap, int d, int window, int sink);
/* The decode family: 1 <= Nq <= FA_DECODE_MAX_NQ. */
int fa_mi355x_fwd_decode_sink(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                              const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int Ncap,
                              int num_pages, int page_size, int max_pages, int d_new, int d, int layout, float softmax_scale, int causal,
                              int window, int sink, int dtype, void* stream);

int fa_mi355x_extend_sink_splits(int B, int H, int Hkv, int Nq, int Ncap, int d, int dtype, int window, int sink);
size_t fa_mi355x_extend_sink_workspace_bytes(int B, int H, int Hkv, int Nq, int Ncap, int d, int window, int sink);
/* The extend family: any Nq >= 1. */
int fa_mi355x_fwd_extend_sink(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                              const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int Ncap,
                              int num_pages, int page_size, int max_pages, int d_new, int d, int layout, float softmax_scale, int causal,
                              int window, int sink, int dtype, void* stream);

int fa_mi355x_ragged_sink_splits(int B, int H, int Hkv, int T, int Ncap, int d, int dtype, int window, int sink);
size_t fa_mi355x_ragged_sink_workspace_bytes(int B, int H, int Hkv, int T, int Ncap, int d, int window, int sink);
/* The ragged family: q, out, k_new and v_new packed into T rows, cu_seqlens_q as in flash_attn_mi355x_decode_ragged.h. */
int fa_mi355x_fwd_ragged_sink(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                              const int* cu_seqlens_q, const int* cache_seqlens, const int* block_table, void* workspace, int B, int H,
                              int Hkv, int T, int Ncap, int num_pages, int page_size, int max_pages, int d_new, int d, int layout,
                              float softmax_scale, int causal, int window, int sink, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLASH_ATTN_MI355X_DECODE_SINK_H */
