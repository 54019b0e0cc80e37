/*
 * flash_attn_mi355x_decode.h -- C ABI of the MI355X (gfx950) KV-cache decode attention library, libflash_attn_mi355x_decode.so.
 *
 * The decode step of token-by-token generation: a few new queries against a cache that already holds the earlier keys and values.
 * The reference model's generate() re-runs the whole model over the full prefix for every new token and keeps the last row
 * (project/run_machine_translation.py:276-292 there); with a cache, a step costs one pass over the cached K and V instead.
 *
 *   out[b,h,i,:] = softmax_j(scale * q[b,h,i,:] . k[b,h,j,:]) . v[b,h,j,:],   j < len_b
 *
 * A library of its own: the training library (flash_attn_mi355x.h) keeps its code object, and inference users can ship only this.
 * Same status codes (FA_OK, FA_ERR_*), dtypes (FA_DTYPE_*) and layouts (FA_LAYOUT_*) as the training library.
 */
#ifndef FLASH_ATTN_MI355X_DECODE_H
#define FLASH_ATTN_MI355X_DECODE_H

#include <stddef.h>

#include "flash_attn_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Largest number of new queries per decode call; more is prefill (fa_mi355x_fwd_layout / fa_mi355x_fwd_scaled) or, against a
 * cache, the extend entry points at the end of this header. */
#define FA_DECODE_MAX_NQ 128

/* Bytes of device workspace fa_mi355x_fwd_decode needs for these sizes: 0 when the call runs as one split, else
 * B*H*nsplit*Nq*(d + 2) floats (one partial O, m, l per query row and split).  A pure function of its arguments (no device query);
 * 0 for non-positive sizes. */
size_t fa_mi355x_decode_workspace_bytes(int B, int H, int Nq, int Ncap, int d);

/* The number of key chunks (splits) a call with these sizes uses: 1 = one launch that writes out and lse directly; more = a split
 * launch into the workspace and a combine launch.  The policy assumes a 256-CU chip (as fa_mi355x_plan does), so the split count,
 * the workspace size and the results do not depend on the GPU that runs the call.  0 for non-positive sizes. */
int fa_mi355x_decode_splits(int B, int H, int Nq, int Ncap, int d, int dtype);

/* Decode attention on device pointers, asynchronous on `stream`, no allocation, no host synchronisation (capturable in a graph).
 *   q        dtype elements, [B][H][Nq][d] (FA_LAYOUT_BHND) or [B][Nq][H][d] (FA_LAYOUT_BNHD), 1 <= Nq <= FA_DECODE_MAX_NQ
 *   k_cache, v_cache   dtype elements, [B][H][Ncap][d] or [B][Ncap][H][d] (the same layout family as q)
 *   out      float, q's shape and layout
 *   lse      float [B][H][Nq]: natural-log logsumexp of the scaled scores (the FA-2 l of the training library); may be NULL
 *   cache_seqlens  device int [B]: len_b, the valid cache rows of batch element b, counting the Nq new tokens (the caller writes
 *            their k / v into the cache first); clamped to [0, Ncap] in the kernel.  NULL: every len_b = Ncap.  Cache rows at or past
 *            len_b contribute nothing whatever they hold, and no cache row past Ncap - 1 is read.
 *   workspace  device memory of fa_mi355x_decode_workspace_bytes(B, H, Nq, Ncap, d) bytes (may be NULL when that is 0)
 *   d        32, 64 or 128 (FA_ERR_UNSUPPORTED_D otherwise).  Other head sizes run through a cache padded with zero columns to
 *            the next of them, with q padded likewise and softmax_scale = 1/sqrt(d).
 *   softmax_scale  0: 1/sqrt(d); otherwise positive and finite.  Applied in fp32 to every score (no folded operand, no guard).
 *   causal   queries are the LAST Nq positions: query i sits at len_b - Nq + i and sees keys j <= len_b - Nq + i.  Otherwise a
 *            query sees all len_b keys.
 *   dtype    FA_DTYPE_F32 or FA_DTYPE_BF16 (q and the cache alike); out and lse are fp32.
 * A row with no admissible key (len_b = 0, or a causal row at a position below 0) returns out = 0 and lse = -inf, as
 * fa_mi355x_fwd_masked does.  No atomics: the split boundaries and the combine order depend only on the arguments, so repeated
 * calls are bitwise identical.  Every bad argument is answered with FA_ERR_BAD_ARG / FA_ERR_UNSUPPORTED_D before any HIP call. */
int fa_mi355x_fwd_decode(const void* q, const void* k_cache, const void* v_cache, float* out, float* lse, const int* cache_seqlens,
                         void* workspace, int B, int H, int Nq, int Ncap, int d, int layout, float softmax_scale, int causal,
                         int dtype, void* stream);

/* Grouped-query (GQA) and multi-query (MQA) caches: q and out have H heads, the caches Hkv heads, H a multiple of Hkv, and query
 * head h reads kv head h / G with G = H / Hkv (Hkv = 1: multi-query).
 *
 *   out[b,h,i,:] = softmax_j(scale * q[b,h,i,:] . k[b,h/G,j,:]) . v[b,h/G,j,:],   j < len_b
 *
 * The G heads of a group share one pass over their kv head's K and V: the G*Nq (query, head) pairs of a kv head are the rows of
 * the kernel's 32-row tiles (row i*G + g: query i, head hkv*G + g), so a call reads B*Hkv*len*d elements of K and of V whatever G.
 * The three functions below are the general form of the three above, with Hkv directly after H; the ones above are their Hkv = H
 * case (the same code: identical splits, workspace and bits).  Everything said there holds here, with these differences:
 *   k_cache, v_cache   [B][Hkv][Ncap][d] (FA_LAYOUT_BHND) or [B][Ncap][Hkv][d] (FA_LAYOUT_BNHD)
 *   q, out, lse        H heads, as above: lse is [B][H][Nq]
 *   workspace          fa_mi355x_decode_workspace_bytes_gqa(B, H, Hkv, Nq, Ncap, d) bytes: B*H*nsplit*Nq*(d + 2) floats or 0 (the
 *                      partials are per QUERY head); the split policy counts B*Hkv*ceil(G*Nq/32) row blocks
 *   Hkv <= 0, or H not a multiple of Hkv: FA_ERR_BAD_ARG (the size queries return 0).  The 2 GiB bound per batch element applies to
 *   the cache with its Hkv heads, and to q. */
size_t fa_mi355x_decode_workspace_bytes_gqa(int B, int H, int Hkv, int Nq, int Ncap, int d);
int fa_mi355x_decode_splits_gqa(int B, int H, int Hkv, int Nq, int Ncap, int d, int dtype);
int fa_mi355x_fwd_decode_gqa(const void* q, const void* k_cache, const void* v_cache, float* out, float* lse, const int* cache_seqlens,
                             void* workspace, int B, int H, int Hkv, int Nq, int Ncap, int d, int layout, float softmax_scale,
                             int causal, int dtype, void* stream);

/* Append the Nq new tokens' k and v to the caches, on the device: one launch writes both, asynchronous on `stream`, no allocation, no
 * host synchronisation (capturable in a graph).  The call that makes "the caller writes their k / v into the cache first" above.
 *   k_new, v_new   dtype elements, [B][Nq][Hkv][d_new] (FA_LAYOUT_BNHD) or [B][Hkv][Nq][d_new] (FA_LAYOUT_BHND), 1 <= d_new <= d;
 *            they must not alias the caches (not checked)
 *   k_cache, v_cache   as fa_mi355x_fwd_decode_gqa: rows of d in {32, 64, 128} (FA_ERR_UNSUPPORTED_D otherwise)
 *   cache_seqlens  as above, with the same meaning: len_b COUNTS the Nq new tokens.  With L_b = len_b clamped to [0, Ncap] on the
 *            device, new token i goes to row L_b - Nq + i, the position the causal mask gives query i, so a token's key always lands
 *            on its own position.  A row below 0 (len_b < Nq) is not written; no row reaches Ncap.  NULL: every L_b = Ncap, the new
 *            tokens go to the last Nq rows.
 * Columns d_new .. d-1 of a written row are set to zero (the caller neither pads nor keeps stale columns clean); every other row of
 * the caches is left untouched.  Stores are 16 bytes per lane when d_new * sizeof(element) is a multiple of 16 and all four pointers
 * are 16-byte aligned, element by element otherwise.  Null k_new, v_new or caches, d_new outside 1 .. d, Nq > FA_DECODE_MAX_NQ,
 * non-positive sizes, an unknown layout or dtype: FA_ERR_BAD_ARG before any HIP call. */
int fa_mi355x_decode_append(const void* k_new, const void* v_new, void* k_cache, void* v_cache, const int* cache_seqlens, int B, int Hkv,
                            int Nq, int Ncap, int d_new, int d, int layout, int dtype, void* stream);

/* fa_mi355x_decode_append followed, on the same stream, by exactly what fa_mi355x_fwd_decode_gqa does with the same arguments: by
 * definition the result is what fa_mi355x_fwd_decode_gqa returns on the caches after the append (same splits, same workspace size
 * from fa_mi355x_decode_workspace_bytes_gqa, same bits).  q has d columns (padded by the caller when d_new < d, as above).  Every
 * argument either of the two rejects is rejected here, before any HIP call and before the caches are touched. */
int fa_mi355x_fwd_decode_append(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                                const int* cache_seqlens, void* workspace, int B, int H, int Hkv, int Nq, int Ncap, int d_new, int d,
                                int layout, float softmax_scale, int causal, int dtype, void* stream);

/* Extend: ANY number Nq >= 1 of new queries against the cache -- a long input that follows a cached prefix (a second chat turn, a
 * user message after a cached system prompt, re-scoring more than 128 tokens) and chunked prefill (the same call from an empty
 * cache, piece by piece).  The semantics, arguments and their order are those of the _gqa decode entry points above (Hkv = H is the
 * ungrouped call; there is one form only), with no upper bound on Nq:
 *
 *   out[b,h,i,:] = softmax_j(scale * q[b,h,i,:] . k[b,h/G,j,:]) . v[b,h/G,j,:],   j < len_b;   causal: query i sits at len_b - Nq + i
 *
 * Kernels of their own: a workgroup owns a 128-row block of a kv head's G*Nq rows (row i*G + g, as above) and a key chunk; its four
 * waves take 32 rows each and share every staged 128-key tile of K and V, each wave keeps its own online softmax, and under `causal`
 * a workgroup loads no tile above its block's last position.  Everything said of fa_mi355x_fwd_decode_gqa holds: len_b clamped to
 * [0, Ncap] on the device, rows at or past len_b contribute nothing whatever they hold and nothing past row Ncap - 1 is read, a row
 * with no admissible key returns out = 0 and lse = -inf, fp32 scaling of every score, no atomics (repeated calls are bitwise
 * identical), asynchronous on `stream`, no allocation, no host synchronisation (capturable in a graph).  For Nq <= 128 the result
 * agrees with fa_mi355x_fwd_decode_gqa to rounding, not bitwise (another summation order).
 *   workspace   fa_mi355x_extend_workspace_bytes(B, H, Hkv, Nq, Ncap, d) bytes: B*H*nsplit*Nq*(d + 2) floats, 0 for one split
 *   splits      the decode policy with 128-row blocks: B*Hkv*ceil(G*Nq/128) groups, aimed at 512 workgroups (two per CU of an
 *               assumed 256-CU chip), chunks a multiple of 256 keys and at least 256; a pure function of the arguments (0 for sizes the size queries
 *               cannot answer, as above)
 * FA_ERR_BAD_ARG / FA_ERR_UNSUPPORTED_D before any HIP call for every argument fa_mi355x_fwd_decode_gqa rejects but Nq > 128, and
 * for G*Nq >= 2^25 rows per kv head, a batch element of q or of the cache of 2 GiB or more, and launches whose workgroup counts
 * (B*Hkv*nsplit*ceil(G*Nq/128) rounded up to 8 items, and B*H*Nq for the combine) do not fit an unsigned int. */
int fa_mi355x_extend_splits(int B, int H, int Hkv, int Nq, int Ncap, int d, int dtype);
size_t fa_mi355x_extend_workspace_bytes(int B, int H, int Hkv, int Nq, int Ncap, int d);
int fa_mi355x_fwd_extend(const void* q, const void* k_cache, const void* v_cache, float* out, float* lse, const int* cache_seqlens,
                         void* workspace, int B, int H, int Hkv, int Nq, int Ncap, int d, int layout, float softmax_scale, int causal,
                         int dtype, void* stream);

/* fa_mi355x_decode_append without its bound on Nq (the same kernel, the same placement: new token i at row L_b - Nq + i), and that
 * launch followed on the same stream by exactly fa_mi355x_fwd_extend, as fa_mi355x_fwd_decode_append is for the decode call: every
 * argument either of the two rejects is rejected before any HIP call and before the caches are touched. */
int fa_mi355x_extend_append(const void* k_new, const void* v_new, void* k_cache, void* v_cache, const int* cache_seqlens, int B, int Hkv,
                            int Nq, int Ncap, int d_new, int d, int layout, int dtype, void* stream);
int fa_mi355x_fwd_extend_append(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                                const int* cache_seqlens, void* workspace, int B, int H, int Hkv, int Nq, int Ncap, int d_new, int d,
                                int layout, float softmax_scale, int causal, int dtype, void* stream);

/* Message of the last FA_ERR_* of this library on this thread ("" if none). */
const char* fa_mi355x_decode_last_error(void);

#ifdef __cplusplus
}
#endif

/* Paged KV caches (a pool of pages and a block table instead of one slab per sequence): the six _paged forms of the entry points
 * above, part of this library and of this header, kept in a file of their own. */
#include "flash_attn_mi355x_decode_paged.h"

/* Ragged batches (packed new tokens, a per-sequence count of them in a device array, contiguous or paged caches): the eight
 * ragged entry points, part of this library and of this header, kept in a file of their own. */
#include "flash_attn_mi355x_decode_ragged.h"

/* Sliding-window attention (each token sees the last W positions only) for the decode, extend and ragged calls, slab or paged, fused
 * with the append or not: nine entry points, part of this library and of this header, kept in a file of their own. */
#include "flash_attn_mi355x_decode_window.h"

/* FP8 (e4m3) KV caches with per-kv-head scales for the decode and extend calls, slab or paged, and the quantising append: three
 * entry points, part of this library and of this header, kept in a file of their own. */
#include "flash_attn_mi355x_decode_fp8.h"

/* Attention-sink tokens (the first S positions stay visible beside the sliding window) for the windowed decode, extend and ragged
 * calls: nine entry points, part of this library and of this header, kept in a file of their own. */
#include "flash_attn_mi355x_decode_sink.h"

/* Rotary position embeddings: a tensor rotated by position, and the fused rotate-and-append that goes in front of the attend-only
 * entry points above, uniform and ragged: three entry points, part of this library and of this header, kept in a file of their own. */
#include "flash_attn_mi355x_decode_rope.h"

/* Logit soft-capping (every score becomes softcap * tanh(score / softcap) between the two products) for the decode, extend and
 * ragged calls, slab or paged, windowed or not: three entry points, part of this library and of this header, kept in a file of
 * their own. */
#include "flash_attn_mi355x_decode_softcap.h"

/* Learned attention-sink logits (gpt-oss: one fp32 logit per query head joins every softmax as a column without a value vector) for
 * the decode, extend and ragged calls, slab or paged, windowed or not: three entry points, part of this library and of this header,
 * kept in a file of their own. */
#include "flash_attn_mi355x_decode_lsink.h"

#endif /* FLASH_ATTN_MI355X_DECODE_H */
