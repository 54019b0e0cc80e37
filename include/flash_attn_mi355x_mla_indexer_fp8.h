/*
 * flash_attn_mi355x_mla_indexer_fp8.h -- the lightning indexer of libflash_attn_mi355x_mla.so on FP8 index keys, the format in which
 * DeepSeek-V3.2 runs its indexer: e4m3 keys with one scale per token, e4m3 queries whose scale is folded into the head weights.
 * Kernels: csrc/fa_mla_indexer_fp8.h; host: csrc/fa_mla.hip.  Everything that is not said here is flash_attn_mi355x_mla_indexer.h's:
 * the definition of a score, the admission rule, the -inf rule, the selection, the chunk policy (fa_mi355x_mla_index_chunks answers
 * for both formats), the status codes and fa_mi355x_mla_last_error().
 *
 * THE FORMAT.  An index-key row is 144 bytes:
 *   bytes   0..127   128 OCP e4m3fn codes, one per column
 *   bytes 128..131   one fp32 scale s for the row: a power of two in [2^-100, 2^120]
 *   bytes 132..143   reserved: the append writes zeros, the kernels ignore them
 * and the value of column c is s * e4m3(code_c).  The cache is a byte array: a slab kidx_cache [B][Ncap][144], or with block_table
 * [B][max_pages] a pool [num_pages][page_size][144] (page_size a multiple of 128 rows, page ids clamped to the pool; the latent
 * cache's own table).  144 bytes and not 132: every row stays 16-byte aligned, so a lane streams its key as whole 16-byte loads and a
 * row never straddles more cache lines than it must.  A scale that is no power of two in that range gives wrong numbers, never a
 * bad address.
 *
 * THE APPEND.  kidx_new bf16 [B][Nq][128]; token i goes to row len_b - Nq + i (nothing below row 0), quantised as ONE 128-column tile
 * by the fp8 latent cache's rule (flash_attn_mi355x_mla_fp8.h): a = max |x| in fp32 (a NaN is ignored, an infinity counts); s = the
 * smallest power of two with a <= 448 s, clamped to [2^-100, 2^120]; code = rne_e4m3(clamp(x / s, -448, 448)); a NaN input stores 0x7F.
 *
 * THE SCORES.  q_idx stays bf16 [B][Nq][HI][128].  The kernel quantises each (token, head) row of 128 columns by the append's rule
 * while it stages Q, and folds that row's scale s_q into the head's weight:
 *
 *   I[b,i,s] = s_k[s] * sum_h (weights[b,i,h] * s_q[b,i,h]) * max(0, sum_c qcode[b,i,h,c] * kcode[b,s,c])
 *
 * Every scale is a positive power of two, so this is the bf16 header's definition on the dequantised queries and keys; products of
 * e4m3 values are exact in fp32.  Positions at or past len_b are neither read nor written; a paged call returns the slab call's
 * bits and a call repeats bit for bit.  scores stay fp32 [B][Nq][Ncap] and fa_mi355x_mla_index_topk selects from them as it does.
 *
 * How it runs.  mla_index_scores_fp8_kernel: the bf16 kernel's split (a lane owns one key, a wave a 32-key tile of each 128-key step,
 * no barrier in the key loop) on v_mfma_f32_32x32x64_f8f6f4 at unit scales, two per 32-head tile and key tile.  A lane streams 64
 * contiguous bytes of its key's row straight into the B operands; Q lies in LDS as codes (32 KB) in the matching column order.  The
 * key's scale multiplies the finished head sum once.  mla_index_append_fp8_kernel: 16 lanes per row.  No scratch, no atomics, no host
 * synchronisation: every call can be captured in a graph.
 *
 * Not built: e5m2, scales that are not powers of two, fp8 q_idx supplied by the caller, a fused score + select launch.
 */
#ifndef FLASH_ATTN_MI355X_MLA_INDEXER_FP8_H
#define FLASH_ATTN_MI355X_MLA_INDEXER_FP8_H

#include "flash_attn_mi355x_mla_indexer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Each call takes its bf16 twin's arguments, with kidx_cache as the byte array, and refuses what the twin refuses, before any HIP call
 * and before any buffer is touched; a slab batch element is counted at 144 bytes per row against 2 GiB. */

int fa_mi355x_mla_index_scores_fp8(const void* q_idx, const float* weights, const void* kidx_new, void* kidx_cache, float* scores,
                                   const int* cache_seqlens, const int* block_table, int B, int HI, int Nq, int Ncap, int num_pages,
                                   int page_size, int max_pages, int causal, void* stream);

int fa_mi355x_mla_index_append_fp8(const void* kidx_new, void* kidx_cache, const int* cache_seqlens, const int* block_table, int B,
                                   int Nq, int Ncap, int num_pages, int page_size, int max_pages, void* stream);

/* Append (kidx_new non-NULL), scores and fa_mi355x_mla_index_topk's launch in one call. */
int fa_mi355x_mla_indexer_fp8(const void* q_idx, const float* weights, const void* kidx_new, void* kidx_cache, float* scores,
                              int* indices, const int* cache_seqlens, const int* block_table, int B, int HI, int Nq, int topk, int Ncap,
                              int num_pages, int page_size, int max_pages, int causal, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLASH_ATTN_MI355X_MLA_INDEXER_FP8_H */
