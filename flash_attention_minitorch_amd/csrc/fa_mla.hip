// C ABI of libflash_attn_mi355x_mla.so (include/flash_attn_mi355x_mla.h): multi-head latent attention decode on a latent KV cache.
// The kernels are fa_mla.h's.  Every entry point fills one MlaCall, check() answers every bad argument before any HIP call, and the
// split policy is stated once (split_rule(), under policy() and sparse_policy()): the size queries and the launches answer from it.
// The sparse call (include/flash_attn_mi355x_mla_sparse.h, kernel in fa_mla_sparse.h) is an MlaCall with an index list.
// The indexer that produces such lists (include/flash_attn_mi355x_mla_indexer.h, kernels in fa_mla_indexer.h) fills one IndexCall,
// which check_index() answers the same way; its chunking is index_policy(), under the split policies.
// The fp8 latent cache (include/flash_attn_mi355x_mla_fp8.h, kernels in fa_mla_fp8.h) is an MlaCall with the fp8 flag: rows of 656
// bytes in the bounds and the strides, the fp8 builds in the launches, the same policies.
// FP8 index keys (include/flash_attn_mi355x_mla_indexer_fp8.h, kernels in fa_mla_indexer_fp8.h) are an IndexCall with the fp8 flag:
// rows of 144 bytes in the slab bound, the fp8 append and score kernels in the launches, the same chunks, the same top-k.
#include "../../include/flash_attn_mi355x_mla.h"
#include "../../include/flash_attn_mi355x_mla_fp8.h"
#include "../../include/flash_attn_mi355x_mla_indexer.h"
#include "../../include/flash_attn_mi355x_mla_indexer_fp8.h"
#include "../../include/flash_attn_mi355x_mla_sparse.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "fa_mla.h"
#include "fa_mla_fp8.h"
#include "fa_mla_indexer.h"
#include "fa_mla_indexer_fp8.h"
#include "fa_mla_sparse.h"

namespace {

thread_local char g_err[512] = "";

int set_err(int code, const char* what) {
  snprintf(g_err, sizeof(g_err), "%s", what);
  return code;
}

int hip_err(const char* what, hipError_t e) {
  snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
  return FA_ERR_HIP;
}

struct MlaCall {
  const void* q = nullptr;
  const void* kv_new = nullptr;
  void* kv_cache = nullptr;
  float *out = nullptr, *lse = nullptr;
  const int *seqlens = nullptr, *table = nullptr;
  const int* indices = nullptr;   // the sparse call: [B][Nq][topk]
  void* workspace = nullptr;
  int B = 0, H = 1, Nq = 0, topk = 0, Ncap = 0, num_pages = 0, page_size = 0, max_pages = 0;
  float softmax_scale = 0.f;
  int causal = 0;
  bool attend = false, append = false, sparse = false;
  bool fp8 = false;   // the cache holds 656-byte rows (e4m3 codes, tile scales, bf16 k_pe)
  long row_bytes() const { return fp8 ? fa::MLA_FP8_ROW_BYTES : fa::MLA_ROW_BYTES; }
  hipStream_t stream = nullptr;
};

// Split policy: the decode library's rule (fa_decode.hip: policy) with one cache head and the 64-row block.  A workgroup holds a
// CU alone (88 KB of LDS, the whole register file), so the aim is two rounds of (batch, chunk, row block) workgroups on the 256 CUs:
// the second round levels sequences of unequal length.  Chunks are whole 128-key super tiles (a page is a whole number of them) and
// at least 256 keys.  The chip size is assumed, not queried: the split count is a function of the arguments alone.
constexpr int MLA_CUS = 256, MLA_ROUNDS = 2, MLA_SUPER = 128, MLA_MIN_CHUNK = 256;
static_assert(FA_PAGE_ROWS % MLA_SUPER == 0 && MLA_SUPER % fa::MLA_TILE == 0, "a page is whole super tiles, a super tile whole tiles");

struct Policy {
  long nqb;     // 64-row blocks of the H * Nq rows
  int chunk, nsplit;
  long items;   // (batch element, split) pairs
  size_t workspace_bytes;
};

// The rule itself: `groups` sets of workgroups walk `n` keys (dense: the cache's capacity; sparse: the entries of an index list).
void split_rule(Policy& p, long groups, int n, int B, int H, int Nq) {
  const long want = std::max(1L, (MLA_CUS * MLA_ROUNDS + groups - 1) / groups);
  const long per = (n + want - 1) / want;
  p.chunk = (int)std::max((long)MLA_MIN_CHUNK, (per + MLA_SUPER - 1) / MLA_SUPER * MLA_SUPER);
  p.nsplit = (int)(((long)n + p.chunk - 1) / p.chunk);
  p.workspace_bytes = p.nsplit == 1 ? 0 : (size_t)B * H * p.nsplit * Nq * (size_t)(fa::MLA_DV + 2) * sizeof(float);
}

Policy policy(int B, int H, int Nq, int Ncap) {
  Policy p;
  p.nqb = ((long)H * Nq + fa::MLA_BLOCK - 1) / fa::MLA_BLOCK;
  split_rule(p, (long)B * p.nqb, Ncap, B, H, Nq);
  p.items = (long)B * p.nsplit;
  return p;
}

// The sparse call: a block holds 64 heads of ONE query token, and the chunks cut that token's list.
Policy sparse_policy(int B, int H, int Nq, int topk) {
  Policy p;
  p.nqb = ((long)H + fa::MLA_BLOCK - 1) / fa::MLA_BLOCK;
  split_rule(p, (long)B * Nq * p.nqb, topk, B, H, Nq);
  p.items = (long)B * Nq * p.nsplit;
  return p;
}

Policy query(int B, int H, int Nq, int n, bool sparse = false) {
  return B > 0 && H > 0 && Nq > 0 && n > 0 ? (sparse ? sparse_policy(B, H, Nq, n) : policy(B, H, Nq, n)) : Policy{};
}

long split_grid(long items, long nqb) { return (items + 7) / 8 * 8 * nqb; }

// The indexer's score launch: a workgroup = (batch element, group of tokens, chunk of keys) streams its chunk once for the group's
// tokens.  A group is as many tokens as the 64 KB of Q in LDS hold (8 blocks of 32 heads), 4 at the most.  Two workgroups share a
// CU (66 KB of LDS each), so the aim is two rounds of two workgroups on each of the 256 CUs; chunks are whole 128-key steps (a page
// is a whole number of them) and at least 512 keys, which keeps the 16 KB of Q per token a small part of what a workgroup reads.
constexpr int IDX_WGS_PER_CU = 2, IDX_MIN_CHUNK = 512;
static_assert(FA_PAGE_ROWS % fa::MLA_IDX_STEP == 0 && IDX_MIN_CHUNK % fa::MLA_IDX_STEP == 0, "a page and a chunk are whole steps");

struct IndexPolicy {
  int group = 0, ngroups = 0, chunk = 0, nchunk = 0;
};

IndexPolicy index_policy(int B, int HI, int Nq, int Ncap) {
  IndexPolicy p;
  if (B <= 0 || HI <= 0 || Nq <= 0 || Ncap <= 0) return p;
  const int tiles = (HI + 31) / 32;
  p.group = std::min(Nq, std::min(fa::MLA_IDX_MAX_GROUP, std::max(1, fa::MLA_IDX_QBLOCKS / tiles)));
  p.ngroups = (Nq + p.group - 1) / p.group;
  const long groups = (long)B * p.ngroups;
  const long want = std::max(1L, ((long)MLA_CUS * IDX_WGS_PER_CU * MLA_ROUNDS + groups - 1) / groups);
  const long per = (Ncap + want - 1) / want;
  p.chunk = (int)std::max((long)IDX_MIN_CHUNK, (per + fa::MLA_IDX_STEP - 1) / fa::MLA_IDX_STEP * fa::MLA_IDX_STEP);
  p.nchunk = (int)(((long)Ncap + p.chunk - 1) / p.chunk);
  return p;
}

bool misaligned(const void* p) { return (uintptr_t)p % 16 != 0; }

// Every check of a call, in one order, before any HIP call.  A paged call's Ncap becomes max_pages * page_size.
int check(MlaCall& c, Policy* out) {
  g_err[0] = 0;
  if (c.B <= 0 || c.H <= 0 || c.Nq <= 0) return set_err(FA_ERR_BAD_ARG, "B, H and Nq must be positive");
  if (c.Nq > FA_DECODE_MAX_NQ)
    return set_err(FA_ERR_BAD_ARG, "Nq > 128 is prefill: a prompt is prefilled un-absorbed, through the forward entry points");
  if (c.table) {
    if (c.num_pages <= 0 || c.page_size <= 0 || c.max_pages <= 0)
      return set_err(FA_ERR_BAD_ARG, "num_pages, page_size and max_pages must be positive");
    if (c.page_size % FA_PAGE_ROWS != 0) {
      snprintf(g_err, sizeof(g_err), "page_size = %d must be a multiple of %d rows", c.page_size, FA_PAGE_ROWS);
      return FA_ERR_BAD_ARG;
    }
    if ((long)c.max_pages * c.page_size + MLA_SUPER > 0x7fffffffL)
      return set_err(FA_ERR_BAD_ARG, "max_pages * page_size (the logical capacity) must fit an int");
    if ((long)c.page_size * c.row_bytes() >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "one page of the pool must stay under 2 GiB");
    if (c.sparse && (long)c.num_pages * c.page_size >= (1L << 31))
      return set_err(FA_ERR_BAD_ARG, "num_pages * page_size (the pool's rows) must stay under 2^31 for the sparse call");
    c.Ncap = c.max_pages * c.page_size;
  } else {
    if (c.Ncap <= 0) return set_err(FA_ERR_BAD_ARG, "Ncap must be positive");
    // (a buffer load's row offset is a 32-bit byte count: a slab, plus a tile of rows past its end)
    if (((long)c.Ncap + fa::MLA_TILE) * c.row_bytes() >= (1L << 31))
      return set_err(FA_ERR_BAD_ARG, "one batch element of the cache must stay under 2 GiB");
  }
  if (!c.kv_cache) return set_err(FA_ERR_BAD_ARG, "null pointer argument: kv_cache");
  if (c.append && !c.kv_new) return set_err(FA_ERR_BAD_ARG, "null pointer argument: kv_new");
  if (misaligned(c.kv_cache) || misaligned(c.kv_new)) return set_err(FA_ERR_BAD_ARG, "kv_cache and kv_new must be 16-byte aligned");
  if ((long)c.B * c.Nq * fa::MlaStager::CPR / 256 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "too many new rows for one append launch");
  if (!c.attend) return FA_OK;
  if (!c.q || !c.out) return set_err(FA_ERR_BAD_ARG, "null pointer argument: q and out");
  if (misaligned(c.q) || misaligned(c.out) || misaligned(c.workspace))
    return set_err(FA_ERR_BAD_ARG, "q, out and the workspace must be 16-byte aligned");
  if (!(c.softmax_scale > 0.f) || !std::isfinite(c.softmax_scale))
    return set_err(FA_ERR_BAD_ARG, "softmax_scale must be positive and finite: it is required (576 is not the model's head dim)");
  if ((long)c.H * c.Nq >= (1L << 25)) return set_err(FA_ERR_BAD_ARG, "H * Nq rows must stay under 2^25");
  if ((long)c.Nq * c.H * fa::MLA_ROW_BYTES >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "one batch element of q must stay under 2 GiB");
  if (c.sparse) {
    if (!c.indices) return set_err(FA_ERR_BAD_ARG, "null pointer argument: indices");
    if ((uintptr_t)c.indices % 4 != 0) return set_err(FA_ERR_BAD_ARG, "indices must be 4-byte aligned");
    if (c.topk <= 0 || c.topk % fa::MLA_TILE != 0) {
      snprintf(g_err, sizeof(g_err), "topk = %d must be a positive multiple of %d entries", c.topk, fa::MLA_TILE);
      return FA_ERR_BAD_ARG;
    }
    if ((long)c.B * c.Nq * c.topk >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "B * Nq * topk index entries must stay under 2^31");
  }
  const Policy p = c.sparse ? sparse_policy(c.B, c.H, c.Nq, c.topk) : policy(c.B, c.H, c.Nq, c.Ncap);
  if (split_grid(p.items, p.nqb) >= (1L << 32) || p.items >= (1L << 31) || (long)c.B * c.H * c.Nq >= (1L << 32))
    return set_err(FA_ERR_BAD_ARG, "too many workgroups for one launch: B * splits * row blocks and B * H * Nq must fit an unsigned int");
  if (p.nsplit > 1 && !c.workspace)
    return set_err(FA_ERR_BAD_ARG, "null workspace: this call needs fa_mi355x_decode_mla_workspace_bytes() bytes");
  *out = p;
  return FA_OK;
}

int launch_append(const MlaCall& c) {
  fa::MlaAppendArgs a;
  a.kv_new = c.kv_new;
  a.kv = c.kv_cache;
  a.seqlens = c.seqlens;
  a.table = c.table;
  a.lanes = (long)c.B * c.Nq * fa::MlaStager::CPR;
  a.Nq = c.Nq, a.Ncap = c.Ncap, a.page_size = c.page_size, a.num_pages = c.num_pages, a.max_pages = c.max_pages;
  if (c.fp8) {   // (a wave per new row, four to a workgroup: `lanes` counts rows)
    a.lanes = (long)c.B * c.Nq;
    hipLaunchKernelGGL(fa::mla_fp8_append_kernel, dim3((unsigned)((a.lanes + 3) / 4)), dim3(256), 0, c.stream, a);
  } else {
    hipLaunchKernelGGL(fa::mla_append_kernel, dim3((unsigned)((a.lanes + 255) / 256)), dim3(256), 0, c.stream, a);
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? FA_OK : hip_err(c.fp8 ? "mla_fp8_append_kernel launch" : "mla_append_kernel launch", e);
}

int launch_attend(const MlaCall& c, const Policy& p) {
  constexpr int D = fa::MLA_DQK, DV = fa::MLA_DV;
  fa::DecodeArgs a{};
  a.q = c.q, a.k = c.kv_cache, a.v = c.kv_cache;
  a.out = c.out, a.lse = c.lse;
  a.part_o = (float*)c.workspace;
  a.part_ml = a.part_o ? a.part_o + (size_t)c.B * c.H * p.nsplit * c.Nq * DV : nullptr;
  a.seqlens = c.seqlens;
  a.H = c.H, a.Hkv = 1, a.G = c.H, a.Nq = c.Nq, a.Ncap = c.Ncap;
  a.nsplit = p.nsplit, a.chunk = p.chunk, a.nqb = (int)p.nqb, a.items = (int)p.items;
  a.inv_G = 1.0f / (float)c.H;
  a.q_ld = c.H * D, a.q_hstride = D, a.q_bstride = (long)c.Nq * c.H * D;
  const int KD = (int)(c.row_bytes() / 2);   // a cache row in the 2-byte units of the argument's strides: 576, or 328 for fp8
  a.kv_ld = KD, a.kv_hstride = 0, a.kv_bstride = (long)c.Ncap * KD;
  a.causal = c.causal ? 1 : 0;
  a.tau = c.softmax_scale;
  a.table = c.table;
  a.page_size = c.page_size, a.num_pages = c.num_pages, a.max_pages = c.max_pages;
  a.page_stride = (long)c.page_size * KD;
  const unsigned grid = (unsigned)split_grid(p.items, p.nqb);
  hipError_t e;
  if (c.sparse) {   // (the same argument and the list; G = H is not read: a block's rows are heads of one token)
    fa::MlaSparseArgs sa{};
    static_cast<fa::DecodeArgs&>(sa) = a;
    sa.indices = c.indices, sa.topk = c.topk;
    if (c.fp8 && c.table) hipLaunchKernelGGL(fa::mla_fp8_sparse_split_kernel<true>, dim3(grid), dim3(256), 0, c.stream, sa);
    else if (c.fp8) hipLaunchKernelGGL(fa::mla_fp8_sparse_split_kernel<false>, dim3(grid), dim3(256), 0, c.stream, sa);
    else if (c.table) hipLaunchKernelGGL(fa::mla_sparse_split_kernel<true>, dim3(grid), dim3(256), 0, c.stream, sa);
    else hipLaunchKernelGGL(fa::mla_sparse_split_kernel<false>, dim3(grid), dim3(256), 0, c.stream, sa);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_err("mla_sparse_split_kernel launch", e);
  } else {
    if (c.fp8 && c.table) hipLaunchKernelGGL(fa::mla_fp8_split_kernel<true>, dim3(grid), dim3(256), 0, c.stream, a);
    else if (c.fp8) hipLaunchKernelGGL(fa::mla_fp8_split_kernel<false>, dim3(grid), dim3(256), 0, c.stream, a);
    else if (c.table) hipLaunchKernelGGL(fa::mla_decode_split_kernel<true>, dim3(grid), dim3(256), 0, c.stream, a);
    else hipLaunchKernelGGL(fa::mla_decode_split_kernel<false>, dim3(grid), dim3(256), 0, c.stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_err("mla_decode_split_kernel launch", e);
  }
  if (p.nsplit == 1) return FA_OK;
  // (the combine body addresses out through q's strides: out's stand in their place)
  a.q_ld = c.H * DV, a.q_hstride = DV, a.q_bstride = (long)c.Nq * c.H * DV;
  hipLaunchKernelGGL(fa::mla_decode_combine_kernel<false>, dim3((unsigned)((long)c.B * c.H * c.Nq)), dim3(256), 0, c.stream, a);
  e = hipGetLastError();
  return e == hipSuccess ? FA_OK : hip_err("mla_decode_combine_kernel launch", e);
}

int run(MlaCall& c) {
  Policy p{};
  if (int rc = check(c, &p)) return rc;
  if (c.append)
    if (int rc = launch_append(c)) return rc;
  return c.attend ? launch_attend(c, p) : FA_OK;
}

// ---- the indexer ----
struct IndexCall {
  const void* q_idx = nullptr;
  const float* weights = nullptr;
  const void* kidx_new = nullptr;
  void* kidx_cache = nullptr;
  float* scores = nullptr;
  int* indices = nullptr;
  const int *seqlens = nullptr, *table = nullptr;
  int B = 0, HI = 1, Nq = 0, topk = 0, Ncap = 0, num_pages = 0, page_size = 0, max_pages = 0, causal = 0;
  bool append = false, score = false, select = false;
  bool fp8 = false;   // the index-key cache holds 144-byte rows (e4m3 codes, one scale)
  long row_bytes() const { return fp8 ? fa::MLA_IDX8_ROW_BYTES : fa::MLA_IDX_ROW_BYTES; }
  hipStream_t stream = nullptr;
};

bool misaligned4(const void* p) { return (uintptr_t)p % 4 != 0; }

// Every check of an indexer call, in one order, before any HIP call.  A paged call's Ncap becomes max_pages * page_size.
int check_index(IndexCall& c, IndexPolicy* out) {
  g_err[0] = 0;
  if (c.B <= 0 || c.HI <= 0 || c.Nq <= 0) return set_err(FA_ERR_BAD_ARG, "B, HI and Nq must be positive");
  if (c.Nq > FA_DECODE_MAX_NQ) return set_err(FA_ERR_BAD_ARG, "Nq > 128 is prefill: an indexer for prefill is not built");
  if (c.HI > fa::MLA_IDX_MAX_HI) return set_err(FA_ERR_BAD_ARG, "HI must be in 1 .. 128 index heads");
  if (c.table) {
    if (c.num_pages <= 0 || c.page_size <= 0 || c.max_pages <= 0)
      return set_err(FA_ERR_BAD_ARG, "num_pages, page_size and max_pages must be positive");
    if (c.page_size % FA_PAGE_ROWS != 0) {
      snprintf(g_err, sizeof(g_err), "page_size = %d must be a multiple of %d rows", c.page_size, FA_PAGE_ROWS);
      return FA_ERR_BAD_ARG;
    }
    if ((long)c.max_pages * c.page_size + fa::MLA_IDX_STEP > 0x7fffffffL)
      return set_err(FA_ERR_BAD_ARG, "max_pages * page_size (the logical capacity) must fit an int");
    c.Ncap = c.max_pages * c.page_size;
  } else {
    if (c.Ncap <= 0) return set_err(FA_ERR_BAD_ARG, "Ncap must be positive");
    // (a buffer load's row offset is a 32-bit byte count: a slab, plus a step of rows past its end)
    if (!c.select || c.score || c.append)
      if (((long)c.Ncap + fa::MLA_IDX_STEP) * c.row_bytes() >= (1L << 31))
        return set_err(FA_ERR_BAD_ARG, "one batch element of the index-key cache must stay under 2 GiB");
  }
  if (misaligned4(c.seqlens) || misaligned4(c.table)) return set_err(FA_ERR_BAD_ARG, "cache_seqlens and block_table must be 4-byte aligned");
  if (c.append || c.score) {
    if (!c.kidx_cache) return set_err(FA_ERR_BAD_ARG, "null pointer argument: kidx_cache");
    if (c.append && !c.kidx_new) return set_err(FA_ERR_BAD_ARG, "null pointer argument: kidx_new");
    if (misaligned(c.kidx_cache) || misaligned(c.kidx_new)) return set_err(FA_ERR_BAD_ARG, "kidx_cache and kidx_new must be 16-byte aligned");
  }
  if (c.score) {
    if (!c.q_idx || !c.weights) return set_err(FA_ERR_BAD_ARG, "null pointer argument: q_idx and weights");
    if (misaligned(c.q_idx) || misaligned(c.weights)) return set_err(FA_ERR_BAD_ARG, "q_idx and weights must be 16-byte aligned");
  }
  if (c.score || c.select) {
    if (!c.scores) return set_err(FA_ERR_BAD_ARG, "null pointer argument: scores");
    if (misaligned(c.scores)) return set_err(FA_ERR_BAD_ARG, "scores must be 16-byte aligned");
  }
  if (c.select) {
    if (!c.indices) return set_err(FA_ERR_BAD_ARG, "null pointer argument: indices");
    if (misaligned4(c.indices)) return set_err(FA_ERR_BAD_ARG, "indices must be 4-byte aligned");
    if (c.topk <= 0 || c.topk % fa::MLA_TILE != 0) {
      snprintf(g_err, sizeof(g_err), "topk = %d must be a positive multiple of %d entries", c.topk, fa::MLA_TILE);
      return FA_ERR_BAD_ARG;
    }
    if ((long)c.B * c.Nq * c.topk >= (1L << 30)) return set_err(FA_ERR_BAD_ARG, "B * Nq * topk index entries must stay under 2^30");
    if (c.Ncap >= (1 << 30)) return set_err(FA_ERR_BAD_ARG, "a row of scores (Ncap) must stay under 2^30 entries");
  }
  const IndexPolicy p = index_policy(c.B, c.HI, c.Nq, c.Ncap);
  if ((long)c.B * p.ngroups * p.nchunk >= (1L << 31) || (long)c.B * c.Nq * (fa::MLA_IDX_D / 8) / 256 >= (1L << 31))
    return set_err(FA_ERR_BAD_ARG, "too many workgroups for one launch");
  *out = p;
  return FA_OK;
}

int run_index(IndexCall& c) {
  IndexPolicy p;
  if (int rc = check_index(c, &p)) return rc;
  hipError_t e;
  if (c.append) {
    fa::MlaAppendArgs a;
    a.kv_new = c.kidx_new, a.kv = c.kidx_cache, a.seqlens = c.seqlens, a.table = c.table;
    a.lanes = (long)c.B * c.Nq * (fa::MLA_IDX_D / 8);
    a.Nq = c.Nq, a.Ncap = c.Ncap, a.page_size = c.page_size, a.num_pages = c.num_pages, a.max_pages = c.max_pages;
    const dim3 grid((unsigned)((a.lanes + 255) / 256));
    if (c.fp8) hipLaunchKernelGGL(fa::mla_index_append_fp8_kernel, grid, dim3(256), 0, c.stream, a);
    else hipLaunchKernelGGL(fa::mla_index_append_kernel, grid, dim3(256), 0, c.stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return hip_err(c.fp8 ? "mla_index_append_fp8_kernel launch" : "mla_index_append_kernel launch", e);
  }
  if (c.score) {
    fa::MlaIndexArgs a;
    a.q = c.q_idx, a.w = c.weights, a.k = c.kidx_cache, a.scores = c.scores, a.seqlens = c.seqlens, a.table = c.table;
    a.HI = c.HI, a.Nq = c.Nq, a.Ncap = c.Ncap, a.chunk = p.chunk, a.nchunk = p.nchunk, a.group = p.group, a.ngroups = p.ngroups;
    a.page_size = c.page_size, a.num_pages = c.num_pages, a.max_pages = c.max_pages, a.causal = c.causal ? 1 : 0;
    const dim3 grid((unsigned)((long)c.B * p.ngroups * p.nchunk));
    if (c.fp8 && c.table) hipLaunchKernelGGL(fa::mla_index_scores_fp8_kernel<true>, grid, dim3(256), 0, c.stream, a);
    else if (c.fp8) hipLaunchKernelGGL(fa::mla_index_scores_fp8_kernel<false>, grid, dim3(256), 0, c.stream, a);
    else if (c.table) hipLaunchKernelGGL(fa::mla_index_scores_kernel<true>, grid, dim3(256), 0, c.stream, a);
    else hipLaunchKernelGGL(fa::mla_index_scores_kernel<false>, grid, dim3(256), 0, c.stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return hip_err(c.fp8 ? "mla_index_scores_fp8_kernel launch" : "mla_index_scores_kernel launch", e);
  }
  if (c.select) {
    fa::MlaTopkArgs a;
    a.scores = c.scores, a.indices = c.indices, a.seqlens = c.seqlens, a.Nq = c.Nq, a.Ncap = c.Ncap, a.topk = c.topk;
    hipLaunchKernelGGL(fa::mla_index_topk_kernel, dim3((unsigned)(c.B * c.Nq)), dim3(fa::MLA_TOPK_THREADS), 0, c.stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return hip_err("mla_index_topk_kernel launch", e);
  }
  return FA_OK;
}

}  // namespace

extern "C" {

const char* fa_mi355x_mla_last_error(void) { return g_err; }

static int decode_mla(bool fp8, const void* q, const void* kv_new, void* kv_cache, float* out, float* lse, const int* cache_seqlens,
                      const int* block_table, void* workspace, int B, int H, int Nq, int Ncap, int num_pages, int page_size,
                      int max_pages, float softmax_scale, int causal, void* stream) {
  MlaCall c;
  c.fp8 = fp8;
  c.q = q, c.kv_new = kv_new, c.kv_cache = kv_cache, c.out = out, c.lse = lse, c.seqlens = cache_seqlens, c.table = block_table;
  c.workspace = workspace, c.B = B, c.H = H, c.Nq = Nq, c.Ncap = Ncap, c.num_pages = num_pages, c.page_size = page_size;
  c.max_pages = max_pages, c.softmax_scale = softmax_scale, c.causal = causal, c.stream = static_cast<hipStream_t>(stream);
  c.attend = true, c.append = kv_new != nullptr;
  return run(c);
}

int fa_mi355x_fwd_decode_mla(const void* q, const void* kv_new, void* kv_cache, float* out, float* lse, const int* cache_seqlens,
                             const int* block_table, void* workspace, int B, int H, int Nq, int Ncap, int num_pages, int page_size,
                             int max_pages, float softmax_scale, int causal, void* stream) {
  return decode_mla(false, q, kv_new, kv_cache, out, lse, cache_seqlens, block_table, workspace, B, H, Nq, Ncap, num_pages, page_size,
                    max_pages, softmax_scale, causal, stream);
}

int fa_mi355x_fwd_decode_mla_fp8(const void* q, const void* kv_new, void* kv_cache, float* out, float* lse, const int* cache_seqlens,
                                 const int* block_table, void* workspace, int B, int H, int Nq, int Ncap, int num_pages, int page_size,
                                 int max_pages, float softmax_scale, int causal, void* stream) {
  return decode_mla(true, q, kv_new, kv_cache, out, lse, cache_seqlens, block_table, workspace, B, H, Nq, Ncap, num_pages, page_size,
                    max_pages, softmax_scale, causal, stream);
}

static int decode_mla_sparse(bool fp8, const void* q, const void* kv_new, void* kv_cache, const int* indices, float* out, float* lse,
                             const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Nq, int topk,
                             int Ncap, int num_pages, int page_size, int max_pages, float softmax_scale, int causal, void* stream) {
  MlaCall c;
  c.fp8 = fp8;
  c.q = q, c.kv_new = kv_new, c.kv_cache = kv_cache, c.out = out, c.lse = lse, c.seqlens = cache_seqlens, c.table = block_table;
  c.workspace = workspace, c.B = B, c.H = H, c.Nq = Nq, c.Ncap = Ncap, c.num_pages = num_pages, c.page_size = page_size;
  c.max_pages = max_pages, c.softmax_scale = softmax_scale, c.causal = causal, c.stream = static_cast<hipStream_t>(stream);
  c.indices = indices, c.topk = topk;
  c.attend = true, c.append = kv_new != nullptr, c.sparse = true;
  return run(c);
}

int fa_mi355x_fwd_decode_mla_sparse(const void* q, const void* kv_new, void* kv_cache, const int* indices, float* out, float* lse,
                                    const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Nq, int topk,
                                    int Ncap, int num_pages, int page_size, int max_pages, float softmax_scale, int causal,
                                    void* stream) {
  return decode_mla_sparse(false, q, kv_new, kv_cache, indices, out, lse, cache_seqlens, block_table, workspace, B, H, Nq, topk, Ncap,
                           num_pages, page_size, max_pages, softmax_scale, causal, stream);
}

int fa_mi355x_fwd_decode_mla_sparse_fp8(const void* q, const void* kv_new, void* kv_cache, const int* indices, float* out, float* lse,
                                        const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Nq,
                                        int topk, int Ncap, int num_pages, int page_size, int max_pages, float softmax_scale,
                                        int causal, void* stream) {
  return decode_mla_sparse(true, q, kv_new, kv_cache, indices, out, lse, cache_seqlens, block_table, workspace, B, H, Nq, topk, Ncap,
                           num_pages, page_size, max_pages, softmax_scale, causal, stream);
}

static int mla_append(bool fp8, const void* kv_new, void* kv_cache, const int* cache_seqlens, const int* block_table, int B, int Nq,
                      int Ncap, int num_pages, int page_size, int max_pages, void* stream) {
  MlaCall c;
  c.fp8 = fp8;
  c.kv_new = kv_new, c.kv_cache = kv_cache, c.seqlens = cache_seqlens, c.table = block_table, c.B = B, c.Nq = Nq, c.Ncap = Ncap;
  c.num_pages = num_pages, c.page_size = page_size, c.max_pages = max_pages, c.stream = static_cast<hipStream_t>(stream);
  c.append = true;
  return run(c);
}

int fa_mi355x_mla_append(const void* kv_new, void* kv_cache, const int* cache_seqlens, const int* block_table, int B, int Nq, int Ncap,
                         int num_pages, int page_size, int max_pages, void* stream) {
  return mla_append(false, kv_new, kv_cache, cache_seqlens, block_table, B, Nq, Ncap, num_pages, page_size, max_pages, stream);
}

int fa_mi355x_mla_append_fp8(const void* kv_new, void* kv_cache, const int* cache_seqlens, const int* block_table, int B, int Nq,
                             int Ncap, int num_pages, int page_size, int max_pages, void* stream) {
  return mla_append(true, kv_new, kv_cache, cache_seqlens, block_table, B, Nq, Ncap, num_pages, page_size, max_pages, stream);
}

int fa_mi355x_decode_mla_splits(int B, int H, int Nq, int Ncap) { return query(B, H, Nq, Ncap).nsplit; }

size_t fa_mi355x_decode_mla_workspace_bytes(int B, int H, int Nq, int Ncap) { return query(B, H, Nq, Ncap).workspace_bytes; }

int fa_mi355x_decode_mla_sparse_splits(int B, int H, int Nq, int topk) { return query(B, H, Nq, topk, true).nsplit; }

size_t fa_mi355x_decode_mla_sparse_workspace_bytes(int B, int H, int Nq, int topk) {
  return query(B, H, Nq, topk, true).workspace_bytes;
}

static int index_scores(bool fp8, const void* q_idx, const float* weights, const void* kidx_new, void* kidx_cache, float* scores,
                        const int* cache_seqlens, const int* block_table, int B, int HI, int Nq, int Ncap, int num_pages, int page_size,
                        int max_pages, int causal, void* stream) {
  IndexCall c;
  c.fp8 = fp8;
  c.q_idx = q_idx, c.weights = weights, c.kidx_new = kidx_new, c.kidx_cache = kidx_cache, c.scores = scores, c.seqlens = cache_seqlens;
  c.table = block_table, c.B = B, c.HI = HI, c.Nq = Nq, c.Ncap = Ncap, c.num_pages = num_pages, c.page_size = page_size;
  c.max_pages = max_pages, c.causal = causal, c.stream = static_cast<hipStream_t>(stream);
  c.append = kidx_new != nullptr, c.score = true;
  return run_index(c);
}

int fa_mi355x_mla_index_scores(const void* q_idx, const float* weights, const void* kidx_new, void* kidx_cache, float* scores,
                               const int* cache_seqlens, const int* block_table, int B, int HI, int Nq, int Ncap, int num_pages,
                               int page_size, int max_pages, int causal, void* stream) {
  return index_scores(false, q_idx, weights, kidx_new, kidx_cache, scores, cache_seqlens, block_table, B, HI, Nq, Ncap, num_pages,
                      page_size, max_pages, causal, stream);
}

int fa_mi355x_mla_index_scores_fp8(const void* q_idx, const float* weights, const void* kidx_new, void* kidx_cache, float* scores,
                                   const int* cache_seqlens, const int* block_table, int B, int HI, int Nq, int Ncap, int num_pages,
                                   int page_size, int max_pages, int causal, void* stream) {
  return index_scores(true, q_idx, weights, kidx_new, kidx_cache, scores, cache_seqlens, block_table, B, HI, Nq, Ncap, num_pages,
                      page_size, max_pages, causal, stream);
}

int fa_mi355x_mla_index_topk(const float* scores, int* indices, const int* cache_seqlens, int B, int Nq, int Ncap, int topk,
                             void* stream) {
  IndexCall c;
  c.scores = const_cast<float*>(scores), c.indices = indices, c.seqlens = cache_seqlens, c.B = B, c.Nq = Nq, c.Ncap = Ncap, c.topk = topk;
  c.stream = static_cast<hipStream_t>(stream);
  c.select = true;
  return run_index(c);
}

static int index_append(bool fp8, const void* kidx_new, void* kidx_cache, const int* cache_seqlens, const int* block_table, int B, int Nq,
                        int Ncap, int num_pages, int page_size, int max_pages, void* stream) {
  IndexCall c;
  c.fp8 = fp8;
  c.kidx_new = kidx_new, c.kidx_cache = kidx_cache, c.seqlens = cache_seqlens, c.table = block_table, c.B = B, c.Nq = Nq, c.Ncap = Ncap;
  c.num_pages = num_pages, c.page_size = page_size, c.max_pages = max_pages, c.stream = static_cast<hipStream_t>(stream);
  c.append = true;
  return run_index(c);
}

int fa_mi355x_mla_index_append(const void* kidx_new, void* kidx_cache, const int* cache_seqlens, const int* block_table, int B, int Nq,
                               int Ncap, int num_pages, int page_size, int max_pages, void* stream) {
  return index_append(false, kidx_new, kidx_cache, cache_seqlens, block_table, B, Nq, Ncap, num_pages, page_size, max_pages, stream);
}

int fa_mi355x_mla_index_append_fp8(const void* kidx_new, void* kidx_cache, const int* cache_seqlens, const int* block_table, int B,
                                   int Nq, int Ncap, int num_pages, int page_size, int max_pages, void* stream) {
  return index_append(true, kidx_new, kidx_cache, cache_seqlens, block_table, B, Nq, Ncap, num_pages, page_size, max_pages, stream);
}

static int indexer(bool fp8, const void* q_idx, const float* weights, const void* kidx_new, void* kidx_cache, float* scores, int* indices,
                   const int* cache_seqlens, const int* block_table, int B, int HI, int Nq, int topk, int Ncap, int num_pages,
                   int page_size, int max_pages, int causal, void* stream) {
  IndexCall c;
  c.fp8 = fp8;
  c.q_idx = q_idx, c.weights = weights, c.kidx_new = kidx_new, c.kidx_cache = kidx_cache, c.scores = scores, c.indices = indices;
  c.seqlens = cache_seqlens, c.table = block_table, c.B = B, c.HI = HI, c.Nq = Nq, c.topk = topk, c.Ncap = Ncap, c.num_pages = num_pages;
  c.page_size = page_size, c.max_pages = max_pages, c.causal = causal, c.stream = static_cast<hipStream_t>(stream);
  c.append = kidx_new != nullptr, c.score = true, c.select = true;
  return run_index(c);
}

int fa_mi355x_mla_indexer(const void* q_idx, const float* weights, const void* kidx_new, void* kidx_cache, float* scores, int* indices,
                          const int* cache_seqlens, const int* block_table, int B, int HI, int Nq, int topk, int Ncap, int num_pages,
                          int page_size, int max_pages, int causal, void* stream) {
  return indexer(false, q_idx, weights, kidx_new, kidx_cache, scores, indices, cache_seqlens, block_table, B, HI, Nq, topk, Ncap,
                 num_pages, page_size, max_pages, causal, stream);
}

int fa_mi355x_mla_indexer_fp8(const void* q_idx, const float* weights, const void* kidx_new, void* kidx_cache, float* scores,
                              int* indices, const int* cache_seqlens, const int* block_table, int B, int HI, int Nq, int topk, int Ncap,
                              int num_pages, int page_size, int max_pages, int causal, void* stream) {
  return indexer(true, q_idx, weights, kidx_new, kidx_cache, scores, indices, cache_seqlens, block_table, B, HI, Nq, topk, Ncap,
                 num_pages, page_size, max_pages, causal, stream);
}

size_t fa_mi355x_mla_indexer_scores_bytes(int B, int Nq, int Ncap) {
  return B > 0 && Nq > 0 && Ncap > 0 ? (size_t)B * Nq * Ncap * sizeof(float) : 0;
}

int fa_mi355x_mla_index_chunks(int B, int HI, int Nq, int Ncap) { return index_policy(B, HI, Nq, Ncap).nchunk; }

}  // extern "C"
