/*
 * flash_attn_mi355x_decode_rope.h -- the rotary-embedding (RoPE) entry points of libflash_attn_mi355x_decode.so: a tensor rotated by
 * position, and the fused rotate-and-append that stands in front of the attention of a roped KV-cache call.  Included by
 * flash_attn_mi355x_decode.h (include that one: it declares the status codes, the layouts, FA_PAGE_ROWS and
 * fa_mi355x_decode_last_error that these calls share with the others).
 */
#ifndef FLASH_ATTN_MI355X_DECODE_ROPE_H
#define FLASH_ATTN_MI355X_DECODE_ROPE_H

#include "flash_attn_mi355x_decode.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Semantics: one definition, used by all three calls.
 *   tables     cos and sin are fp32 device arrays [max_pos][rot / 2], supplied by the caller (any base, any scaling).
 *   rot        the rotary dimension: even, 2 <= rot <= the row length.  Columns >= rot are copied as bits.
 *   pairs      interleaved = 0 (NeoX / Llama): pair j is (x[j], x[j + rot/2]);  interleaved = 1 (GPT-J): pair j is (x[2j], x[2j+1]).
 *   rotation   for a row at position p, c = cos[p][j], s = sin[p][j]:   y1 = x1 * c - x2 * s,   y2 = x2 * c + x1 * s.
 *              Evaluated in fp32 (one product and one fused multiply-add per result, the same device function in every build) and
 *              rounded once, to nearest even, to the tensor's type.  inverse = 1 uses -s: the backward of the rotation.
 *   position   new token i of batch element b sits where the append puts it: p = L_b - Nq + i (ragged: L_b - nq_b + i),
 *              L_b = len_b clamped to [0, Ncap]; its query row has the same p.  The index into the tables is
 *              clamp(p, 0, max_pos - 1), on the device: no access leaves the tables.
 *   V          is never rotated.
 *
 * fa_mi355x_rope: y = rotate(x) for x, y [B][N][H][d] (FA_LAYOUT_BNHD) or [B][H][N][d] (FA_LAYOUT_BHND), any d >= 2; row i of batch
 * element b sits at pos_offsets[b] + i (pos_offsets: an int32 device array [B], or NULL: all zero).  y may be x (a lane owns both
 * members of its pairs).
 *
 * fa_mi355x_rope_append, in ONE launch: q rotated into q_rot (same shape and type; q_rot may be q), k_new rotated and written into
 * the K cache, v_new copied into the V cache.  Placement is exactly the append's (fa_mi355x_extend_append and its paged form): row
 * L_b - Nq + i, nothing below row 0, zeros in columns d_new .. d-1, a paged row looked up with the page id clamped to the pool.  A
 * q row with p < 0 is still written, rotated at the clamped position (the attention gives it an empty row anyway).  Any Nq >= 1.
 *   q / q_rot both NULL           append only.
 *   k_new / v_new both NULL       rotate q only (the caches are not touched and may be NULL).
 *   one of a pair NULL, all NULL  FA_ERR_BAD_ARG.
 *   block_table NULL              slab caches of Ncap rows; otherwise the pool's geometry stands for Ncap, as in _paged.h.
 *   cache_fp8 = 1                 caches of e4m3 bytes with k_scale / v_scale (NULL: ones) as in _fp8.h; dtype must be FA_DTYPE_BF16.
 *                                 The rotated k is rounded to bf16, then quantised by fa_mi355x_append_fp8's rule; v as there.
 * fa_mi355x_rope_append_ragged: the same for packed q, q_rot [T][H][d] and k_new, v_new [T][Hkv][d_new] with cu_seqlens_q as in
 * _ragged.h; packed rows that no sequence owns are neither read nor written, in the caches and in q_rot.
 *
 * The attention then goes through the EXISTING attend-only entry points on q_rot (plain, _paged, _window, _sink, _fp8, _ragged...):
 * two asynchronous calls on one stream, capturable in a graph, and the launch count of the fused call: append, split, combine.
 *
 * Checks, all before any HIP call and before the caches are touched: every check of the family's append and of the paged form;
 * cos / sin non-null; rot even and 2 <= rot <= min(d_new, d) (d alone when there is no k_new); interleaved and inverse in {0, 1};
 * max_pos >= Ncap in the two append forms (the logical capacity of a paged cache), since every row the cache can hold must have
 * an angle; cache_fp8 in {0, 1} and only with FA_DTYPE_BF16.
 *
 * Bit for bit:
 *   1. rope_append = rope on q and on k_new with pos_offsets[b] = L_b - Nq, then the family's plain append (fa_mi355x_append_fp8
 *      for an fp8 cache): the same q_rot, and the same K and V caches in every byte.
 *   2. hence a roped attention (rope_append, then an attend-only call on q_rot) returns the out and lse, and leaves the caches, of
 *      the unroped fused call on the rotated q and k_new.
 * Against exact arithmetic on the same inputs and tables: |err| <= u * |exact| + 2^-22 * (|x1| + |x2|), u = 2^-8 (bf16) or 0 (fp32).
 *
 * How it runs.  A lane moves 16 bytes of one row where rot, d_new and the pointers allow it (the pairs or their halves fall on whole
 * vectors, every row and table row starts on 16 bytes), one element otherwise; the host picks the build.  In the NeoX form a lane
 * loads the matching 16 bytes of both halves.  Lanes walk the sources in memory order; no LDS, no scratch.
 *
 * NOT built: rotation inside the attention kernels; a re-assignment of positions inside the cache (StreamingLLM); scaled and YaRN
 * tables (the caller supplies any table); rotary on a ragged fp8 cache (ragged fp8 does not exist); rotary in the host-pointer
 * reference ABI.
 */
int fa_mi355x_rope(const void* x, void* y, const float* cos, const float* sin, const int* pos_offsets, int B, int N, int H, int d, int rot,
                   int max_pos, int layout, int interleaved, int inverse, int dtype, void* stream);

int fa_mi355x_rope_append(const void* q, void* q_rot, const void* k_new, const void* v_new, void* k_cache, void* v_cache, const float* k_scale,
                          const float* v_scale, const float* cos, const float* sin, const int* cache_seqlens, const int* block_table, int B,
                          int H, int Hkv, int Nq, int Ncap, int num_pages, int page_size, int max_pages, int d_new, int d, int rot,
                          int max_pos, int layout, int interleaved, int cache_fp8, int dtype, void* stream);

int fa_mi355x_rope_append_ragged(const void* q, void* q_rot, const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                                 const float* cos, const float* sin, const int* cu_seqlens_q, const int* cache_seqlens,
                                 const int* block_table, int B, int H, int Hkv, int T, int Ncap, int num_pages, int page_size, int max_pages,
                                 int d_new, int d, int rot, int max_pos, int layout, int interleaved, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLASH_ATTN_MI355X_DECODE_ROPE_H */
