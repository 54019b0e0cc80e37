// C ABI of the MI355X KV-cache decode library (declared in include/flash_attn_mi355x_decode.h, its _paged.h and its _ragged.h):
// argument checks, the split policies (decode: 32-row blocks, at most 128 queries; extend: 128-row blocks, any number; ragged: the
// extend policy on an upper bound of the row blocks) and the launches of the kernels of fa_decode.h.  A paged call (a pool and a
// block table) takes the contiguous call's policy at Ncap = max_pages * page_size.  A windowed call (_window.h) takes the three
// policies on its window span (span_keys) instead of Ncap, a sink call (_sink.h) on that span plus its sink tiles.  An fp8 call (_fp8.h: caches of e4m3 bytes, per-kv-head scales) takes the
// bf16 call's policy and workspace for the same arguments; its cache bounds count one byte per element.  The rotary calls (_rope.h)
// launch the kernels of fa_rope.h in front of the attend-only entry points.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <stdio.h>

#include "../../include/flash_attn_mi355x_decode.h"
#include "fa_decode.h"
#include "fa_rope.h"

namespace {

thread_local char g_err[512] = "";

int set_err(int code, const char* what, hipError_t e = hipSuccess) {
  if (e != hipSuccess)
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
  else
    snprintf(g_err, sizeof(g_err), "%s", what);
  return code;
}

// Split policy (DESIGN.md "Decode"): enough (batch*kv head, chunk, row block) workgroups to cover a 256-CU chip four times, chunks a
// multiple of 256 keys (two super tiles) and at least 256 keys.  A kv head has G*Nq rows (G = H / Hkv query heads per kv head), 32 to
// a block.  Launches that already have 1024 workgroups without splitting run as one split.  The chip size is assumed, not queried,
// so the split count is a function of the arguments alone.
constexpr int DEC_CUS = 256, DEC_WAVES = 4, DEC_MIN_CHUNK = 256;

// (positive sizes and H a multiple of Hkv: what the two size queries need to answer at all)
bool sizes_ok(int B, int H, int Hkv, int Nq, int Ncap, int d) {
  return B > 0 && H > 0 && Hkv > 0 && Nq > 0 && Ncap > 0 && d > 0 && H % Hkv == 0;
}

int row_blocks(int H, int Hkv, int Nq) { return (int)(((long)(H / Hkv) * Nq + 31) / 32); }

int chunk_keys(int B, int H, int Hkv, int Nq, int Ncap) {
  const long groups = (long)B * Hkv * row_blocks(H, Hkv, Nq);
  const long want = std::max(1L, (DEC_CUS * DEC_WAVES + groups - 1) / groups);
  const long per = (Ncap + want - 1) / want;
  return (int)std::max((long)DEC_MIN_CHUNK, (per + DEC_MIN_CHUNK - 1) / DEC_MIN_CHUNK * DEC_MIN_CHUNK);
}

int splits(int B, int H, int Hkv, int Nq, int Ncap) {
  const int ch = chunk_keys(B, H, Hkv, Nq, Ncap);
  return (int)(((long)Ncap + ch - 1) / ch);
}

size_t workspace_bytes(int B, int H, int Hkv, int Nq, int Ncap, int d) {
  const int ns = splits(B, H, Hkv, Nq, Ncap);
  return ns == 1 ? 0 : (size_t)B * H * ns * Nq * (size_t)(d + 2) * sizeof(float);
}

// Extend policy: the same with 128-row blocks (a workgroup of extend_split_kernel owns 128 rows): groups = B * Hkv * ceil(G*Nq / 128),
// and TWO workgroups per CU as the target: a workgroup here lives for a long key loop, so a second round of workgroups buys nothing,
// while every split costs a partial per row and the combine launch over B*H*Nq rows (measured: profiles/extend_bench.txt).
constexpr int EXT_WAVES = 2;
int ext_row_blocks(int H, int Hkv, int Nq) { return (int)(((long)(H / Hkv) * Nq + fa::EXT_BLOCK - 1) / fa::EXT_BLOCK); }

int ext_chunk_for(long groups, int Ncap) {
  const long want = std::max(1L, (DEC_CUS * EXT_WAVES + groups - 1) / groups);
  const long per = (Ncap + want - 1) / want;
  return (int)std::max((long)DEC_MIN_CHUNK, (per + DEC_MIN_CHUNK - 1) / DEC_MIN_CHUNK * DEC_MIN_CHUNK);
}

int ext_chunk_keys(int B, int H, int Hkv, int Nq, int Ncap) { return ext_chunk_for((long)B * Hkv * ext_row_blocks(H, Hkv, Nq), Ncap); }

int ext_splits(int B, int H, int Hkv, int Nq, int Ncap) {
  const int ch = ext_chunk_keys(B, H, Hkv, Nq, Ncap);
  return (int)(((long)Ncap + ch - 1) / ch);
}

size_t ext_workspace_bytes(int B, int H, int Hkv, int Nq, int Ncap, int d) {
  const int ns = ext_splits(B, H, Hkv, Nq, Ncap);
  return ns == 1 ? 0 : (size_t)B * H * ns * Nq * (size_t)(d + 2) * sizeof(float);
}

// Sliding window (include/flash_attn_mi355x_decode_window.h).  A window of W >= Ncap keys admits every key of every row (a row's
// position is at most len - 1 <= Ncap - 1): such a call IS the unwindowed call, the same launches and the same bits, and so is
// W = 0.  This also bounds what the device computes with: W < Ncap.
// Sinks (include/flash_attn_mi355x_decode_sink.h): S >= Ncap first positions admit every key of every row as well, and S = 0 is
// the windowed call; sinks without a window mean nothing.  The device computes with 1 <= W < Ncap and 0 <= S < Ncap.
int win_of(int window, int Ncap, int sink = 0) { return window >= Ncap || sink >= Ncap ? 0 : window; }
int sink_of(int window, int sink, int Ncap) { return win_of(window, Ncap, sink) == 0 ? 0 : sink; }

// The window SPAN: the keys one row block can need, which is what the three policies split where they split Ncap.  A block's rows
// sit at positions p_first .. p_last with p_last - p_first <= min(Nq, block_rows) - 1 (row i * G + g: block_rows rows span at most
// block_rows positions, and no more than the call has).  Its key range starts at lo = (p_first - W + 1, clamped to 0) rounded DOWN
// to a super tile, at most 127 keys below the edge, and ends at p_last:
//   p_last - lo + 1 <= (p_last - p_first) + W + 127 <= W + min(Nq, block_rows) - 1 + 127
// and never more than the cache holds.  nsplit * chunk >= span, so the splits of every block cover [lo, p_last].
// With S sinks a block walks, in front of that range, the super tiles that hold a sink key and lie wholly below lo: at most
// ceil(S / 128) of them, which the span counts in full.
int span_keys(int window, int Ncap, int Nq, int block_rows, int sink = 0) {
  const int W = win_of(window, Ncap, sink);
  if (W == 0) return Ncap;
  const long sink_keys = ((long)sink + fa::DEC_ROWS - 1) / fa::DEC_ROWS * fa::DEC_ROWS;
  return (int)std::min((long)Ncap, sink_keys + W + std::min(Nq, block_rows) - 1 + fa::DEC_ROWS - 1);
}

// workgroups of the split launch: the items rounded up to 8, times the row blocks (the kernels' workgroup -> (item, row block) map)
long split_grid(long items, long nqb) { return (items + 7) / 8 * 8 * nqb; }

// Ragged policy: the extend policy on what the ARGUMENTS say about the row blocks, never the device arrays: a sequence's G * nq_b rows
// round up to 128 at most once, so B sequences that share T packed rows have at most floor(G * T / 128) + min(B, T) row blocks.  That
// bound sizes the block map and the grid and stands for the row blocks in the policy, so the split count, the workspace and a
// captured graph do not depend on cu_seqlens_q.  (It under-splits a step whose tokens all sit in one of many sequences.)
long rag_blocks(int B, int H, int Hkv, int T) { return (long)(H / Hkv) * T / fa::EXT_BLOCK + std::min(B, T); }
int rag_chunk_keys(int B, int H, int Hkv, int T, int Ncap) { return ext_chunk_for((long)Hkv * rag_blocks(B, H, Hkv, T), Ncap); }

int rag_splits(int B, int H, int Hkv, int T, int Ncap) {
  const int ch = rag_chunk_keys(B, H, Hkv, T, Ncap);
  return (int)(((long)Ncap + ch - 1) / ch);
}

// the workspace: the block map ((sequence, block) int pairs, rounded up to 16 bytes), then the partials of H * ns * T rows
size_t rag_map_bytes(int B, int H, int Hkv, int T) { return ((size_t)rag_blocks(B, H, Hkv, T) * 2 * sizeof(int) + 15) / 16 * 16; }

size_t rag_workspace_bytes(int B, int H, int Hkv, int T, int Ncap, int d) {
  return rag_map_bytes(B, H, Hkv, T) + (size_t)H * rag_splits(B, H, Hkv, T, Ncap) * T * (size_t)(d + 2) * sizeof(float);
}

template <typename T, int D> int launch_extend(fa::DecodeArgs a, int BH, int sink, hipStream_t st) {
  if (sink) {   // (the sink builds: their own kernels and argument; a.window >= 1)
    fa::SinkArgs sa;
    static_cast<fa::DecodeArgs&>(sa) = a;
    sa.sink = sink;
    if (a.table)
      hipLaunchKernelGGL((fa::extend_split_sink_kernel<T, D, true, false>), dim3((unsigned)split_grid(a.items, a.nqb)), dim3(256), 0, st, sa);
    else
      hipLaunchKernelGGL((fa::extend_split_sink_kernel<T, D, false, false>), dim3((unsigned)split_grid(a.items, a.nqb)), dim3(256), 0, st, sa);
  } else if (a.window && a.table)
    hipLaunchKernelGGL((fa::extend_split_kernel<T, D, true, false, true>), dim3((unsigned)split_grid(a.items, a.nqb)), dim3(256), 0, st, a);
  else if (a.window)
    hipLaunchKernelGGL((fa::extend_split_kernel<T, D, false, false, true>), dim3((unsigned)split_grid(a.items, a.nqb)), dim3(256), 0, st, a);
  else if (a.table)
    hipLaunchKernelGGL((fa::extend_split_kernel<T, D, true>), dim3((unsigned)split_grid(a.items, a.nqb)), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((fa::extend_split_kernel<T, D>), dim3((unsigned)split_grid(a.items, a.nqb)), dim3(256), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_err(FA_ERR_HIP, "extend_split_kernel launch", e);
  if (a.nsplit > 1) {
    hipLaunchKernelGGL((fa::decode_combine_kernel<D>), dim3((unsigned)((long)BH * a.Nq)), dim3(256), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return set_err(FA_ERR_HIP, "decode_combine_kernel launch", e);
  }
  return FA_OK;
}

template <typename T> int launch_extend_d(const fa::DecodeArgs& a, int BH, int d, int sink, hipStream_t st) {
  switch (d) {
    case 32: return launch_extend<T, 32>(a, BH, sink, st);
    case 64: return launch_extend<T, 64>(a, BH, sink, st);
    default: return launch_extend<T, 128>(a, BH, sink, st);
  }
}

template <typename T, int D> int launch(fa::DecodeArgs a, int BH, int sink, hipStream_t st) {
  const int grid = ((a.items + 7) / 8) * 8 * a.nqb;
  if (sink) {   // (the sink builds: their own kernels and argument; grouped, as the windowed builds are; a.window >= 1)
    fa::SinkArgs sa;
    static_cast<fa::DecodeArgs&>(sa) = a;
    sa.sink = sink;
    if (a.table)
      hipLaunchKernelGGL((fa::decode_split_sink_kernel<T, D, true>), dim3(grid), dim3(256), 0, st, sa);
    else
      hipLaunchKernelGGL((fa::decode_split_sink_kernel<T, D, false>), dim3(grid), dim3(256), 0, st, sa);
  } else if (a.window && a.table)   // (the windowed builds: grouped, as the paged one is)
    hipLaunchKernelGGL((fa::decode_split_kernel<T, D, true, true, true>), dim3(grid), dim3(256), 0, st, a);
  else if (a.window)
    hipLaunchKernelGGL((fa::decode_split_kernel<T, D, true, false, true>), dim3(grid), dim3(256), 0, st, a);
  else if (a.table)   // (one paged build, the grouped one: G = 1 computes the same rows, and a paged workgroup looks up its page anyway)
    hipLaunchKernelGGL((fa::decode_split_kernel<T, D, true, true>), dim3(grid), dim3(256), 0, st, a);
  else if (a.G > 1)
    hipLaunchKernelGGL((fa::decode_split_kernel<T, D, true>), dim3(grid), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((fa::decode_split_kernel<T, D, false>), dim3(grid), dim3(256), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_err(FA_ERR_HIP, "decode_split_kernel launch", e);
  if (a.nsplit > 1) {
    hipLaunchKernelGGL((fa::decode_combine_kernel<D>), dim3((unsigned)(BH * a.Nq)), dim3(256), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return set_err(FA_ERR_HIP, "decode_combine_kernel launch", e);
  }
  return FA_OK;
}

template <typename T> int launch_d(const fa::DecodeArgs& a, int BH, int d, int sink, hipStream_t st) {
  switch (d) {
    case 32: return launch<T, 32>(a, BH, sink, st);
    case 64: return launch<T, 64>(a, BH, sink, st);
    default: return launch<T, 128>(a, BH, sink, st);
  }
}

// An fp8 call's scales (null: a bf16 or fp32 cache).
struct Fp8 {
  const float* k_scale;
  const float* v_scale;
};

// The FP8 builds: bf16 queries, the grouped form of the split kernel (as the paged build takes it for G = 1), slab or paged.
template <int D> int launch_fp8(fa::Fp8Args a, int BH, bool extend, hipStream_t st) {
  using T = fa::bf16_t;
  const dim3 grid((unsigned)split_grid(a.items, a.nqb));
  if (extend && a.table)
    hipLaunchKernelGGL((fa::extend_split_kernel<T, D, true, false, false, true>), grid, dim3(256), 0, st, a);
  else if (extend)
    hipLaunchKernelGGL((fa::extend_split_kernel<T, D, false, false, false, true>), grid, dim3(256), 0, st, a);
  else if (a.table)
    hipLaunchKernelGGL((fa::decode_split_kernel<T, D, true, true, false, true>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((fa::decode_split_kernel<T, D, true, false, false, true>), grid, dim3(256), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_err(FA_ERR_HIP, extend ? "extend_split_kernel (fp8) launch" : "decode_split_kernel (fp8) launch", e);
  if (a.nsplit > 1) {
    hipLaunchKernelGGL((fa::decode_combine_kernel<D, false, true>), dim3((unsigned)((long)BH * a.Nq)), dim3(256), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return set_err(FA_ERR_HIP, "decode_combine_kernel (fp8) launch", e);
  }
  return FA_OK;
}

int launch_fp8_d(const fa::Fp8Args& a, int BH, int d, bool extend, hipStream_t st) {
  switch (d) {
    case 32: return launch_fp8<32>(a, BH, extend, st);
    case 64: return launch_fp8<64>(a, BH, extend, st);
    default: return launch_fp8<128>(a, BH, extend, st);
  }
}

// A paged call's block table and pool geometry (null: the contiguous call).
struct Paging {
  const int* table;
  int num_pages, page_size, max_pages;
};

// The checks a paged call makes first: FA_OK with the logical capacity max_pages * page_size in *Ncap, or the error.
int check_pages(const Paging& p, int* Ncap) {
  g_err[0] = 0;
  if (!p.table) return set_err(FA_ERR_BAD_ARG, "null block_table");
  if (p.num_pages <= 0) return set_err(FA_ERR_BAD_ARG, "num_pages must be positive");
  if (p.page_size <= 0) return set_err(FA_ERR_BAD_ARG, "page_size must be positive");
  if (p.max_pages <= 0) return set_err(FA_ERR_BAD_ARG, "max_pages must be positive");
  if (p.page_size % FA_PAGE_ROWS != 0) {
    snprintf(g_err, sizeof(g_err), "page_size = %d must be a multiple of %d rows", p.page_size, FA_PAGE_ROWS);
    return FA_ERR_BAD_ARG;
  }
  // (the kernels count logical rows in an int, a super tile past the capacity included)
  if ((long)p.max_pages * p.page_size + fa::DEC_ROWS > 0x7fffffffL)
    return set_err(FA_ERR_BAD_ARG, "max_pages * page_size (the logical capacity) must fit an int");
  *Ncap = p.max_pages * p.page_size;
  return FA_OK;
}

// (a buffer load's row offset is a 32-bit byte count inside one page; page base addresses are 64-bit, so the pool may be any size)
// (fp8: the pool holds one byte per element whatever dtype, the queries' type, says)
int check_page_bytes(int page_size, int Hkv, int d, int dtype, bool fp8 = false) {
  const long esz = fp8 ? 1 : dtype == FA_DTYPE_BF16 ? 2 : 4;
  if ((long)page_size * Hkv * d * esz >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "one page of the pool must stay under 2 GiB");
  return FA_OK;
}

// The argument checks of fa_mi355x_fwd_decode_gqa, or (extend) of fa_mi355x_fwd_extend: FA_OK, or the error with its message set.
// page_size > 0: a paged call with Ncap = max_pages * page_size, where the bound on a batch element of the cache is one on a page.
// window, sink: the splits are those of the window span.  fp8: the caches hold one byte per element and the queries are bf16.
int check_decode(const void* q, const void* k_cache, const void* v_cache, const float* out, const void* workspace, int B, int H, int Hkv,
                 int Nq, int Ncap, int d, int layout, float softmax_scale, int dtype, bool extend = false, int page_size = 0,
                 int window = 0, bool fp8 = false, int sink = 0) {
  g_err[0] = 0;
  if (B <= 0 || H <= 0 || Nq <= 0 || Ncap <= 0 || d <= 0) return set_err(FA_ERR_BAD_ARG, "B, H, Nq, Ncap and d must be positive");
  if (Hkv <= 0) return set_err(FA_ERR_BAD_ARG, "Hkv must be positive");
  if (H % Hkv != 0) {
    snprintf(g_err, sizeof(g_err), "H = %d query heads must be a multiple of Hkv = %d cache heads", H, Hkv);
    return FA_ERR_BAD_ARG;
  }
  if (!extend && Nq > FA_DECODE_MAX_NQ)
    return set_err(FA_ERR_BAD_ARG, "Nq > 128 is prefill: use fa_mi355x_fwd_layout or fa_mi355x_fwd_scaled (the forward entry points)");
  if (dtype != FA_DTYPE_F32 && dtype != FA_DTYPE_BF16) return set_err(FA_ERR_BAD_ARG, "unknown dtype");
  if (layout != FA_LAYOUT_BHND && layout != FA_LAYOUT_BNHD) return set_err(FA_ERR_BAD_ARG, "unknown layout");
  if (!q || !k_cache || !v_cache || !out) return set_err(FA_ERR_BAD_ARG, "null pointer argument");
  if (d != 32 && d != 64 && d != 128)
    return set_err(FA_ERR_UNSUPPORTED_D, "decode supports d in {32, 64, 128}: pad the cache with zero columns for other d <= 128");
  if (softmax_scale != 0.f && (!(softmax_scale > 0.f) || !std::isfinite(softmax_scale)))
    return set_err(FA_ERR_BAD_ARG, "softmax_scale must be positive and finite (0: 1/sqrt(d))");
  // (row_query is exact for rows below 2^25)
  if (extend && (long)(H / Hkv) * Nq >= (1L << 25)) return set_err(FA_ERR_BAD_ARG, "G * Nq rows per kv head must stay under 2^25");
  const long esz = dtype == FA_DTYPE_BF16 ? 2 : 4;
  // (a buffer load's row offset is a 32-bit byte count: one batch element, plus a super tile of rows past its end, stays under 2 GiB;
  // q's (head, query) offset within its batch element likewise)
  if (page_size > 0) {
    if (check_page_bytes(page_size, Hkv, d, dtype, fp8) != FA_OK) return FA_ERR_BAD_ARG;
  } else if (((long)Ncap + fa::DEC_ROWS) * Hkv * d * (fp8 ? 1 : esz) >= (1L << 31)) {
    return set_err(FA_ERR_BAD_ARG, "one batch element of the cache must stay under 2 GiB");
  }
  if ((long)Nq * H * d * esz >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "one batch element of q must stay under 2 GiB");
  if (extend) {
    // (the workgroup counts of the split and the combine launch are unsigned ints, the items an int)
    const int ens = ext_splits(B, H, Hkv, Nq, span_keys(window, Ncap, Nq, fa::EXT_BLOCK, sink));
    if (split_grid((long)B * Hkv * ens, ext_row_blocks(H, Hkv, Nq)) >= (1L << 32) || (long)B * Hkv * ens >= (1L << 31) ||
        (long)B * H * Nq >= (1L << 32))
      return set_err(FA_ERR_BAD_ARG, "too many workgroups for one launch: B * Hkv * splits * row blocks and B * H * Nq must fit an unsigned int");
    if (ens > 1 && !workspace) return set_err(FA_ERR_BAD_ARG, "null workspace: this call needs fa_mi355x_extend_workspace_bytes() bytes");
    return FA_OK;
  }
  const int ns = splits(B, H, Hkv, Nq, span_keys(window, Ncap, Nq, 32, sink));
  if (ns > 1 && !workspace) return set_err(FA_ERR_BAD_ARG, "null workspace: this call needs fa_mi355x_decode_workspace_bytes() bytes");
  return FA_OK;
}

// The split (and combine) launches of a checked call: the decode kernels, or (extend) the extend kernels under their own policy.
int run_decode(const void* q, const void* k_cache, const void* v_cache, float* out, float* lse, const int* cache_seqlens, void* workspace,
               int B, int H, int Hkv, int Nq, int Ncap, int d, int layout, float softmax_scale, int causal, int dtype, void* stream,
               bool extend = false, const Paging* pg = nullptr, int window = 0, const Fp8* f8 = nullptr, int sink = 0) {
  const int span = span_keys(window, Ncap, Nq, extend ? fa::EXT_BLOCK : 32, sink);   // (no window: Ncap)
  const int ns = extend ? ext_splits(B, H, Hkv, Nq, span) : splits(B, H, Hkv, Nq, span);
  fa::Fp8Args a;   // (the other builds take its DecodeArgs part)
  a.k_scale = f8 ? f8->k_scale : nullptr;
  a.v_scale = f8 ? f8->v_scale : nullptr;
  a.q = q;
  a.k = k_cache;
  a.v = v_cache;
  a.out = out;
  a.lse = lse;
  a.part_o = static_cast<float*>(workspace);
  a.part_ml = ns > 1 ? a.part_o + (size_t)B * H * ns * Nq * d : nullptr;
  a.seqlens = cache_seqlens;
  a.H = H;
  a.Hkv = Hkv;
  a.G = H / Hkv;
  a.inv_G = 1.0f / (float)a.G;
  a.Nq = Nq;
  a.Ncap = Ncap;
  a.nsplit = ns;
  a.chunk = extend ? ext_chunk_keys(B, H, Hkv, Nq, span) : chunk_keys(B, H, Hkv, Nq, span);
  a.window = win_of(window, Ncap, sink);
  sink = sink_of(window, sink, Ncap);
  a.nqb = extend ? ext_row_blocks(H, Hkv, Nq) : row_blocks(H, Hkv, Nq);
  a.items = B * Hkv * ns;
  const bool bnhd = layout == FA_LAYOUT_BNHD;
  a.q_ld = bnhd ? H * d : d;
  a.kv_ld = bnhd ? Hkv * d : d;
  a.q_bstride = (long)Nq * H * d;
  a.kv_bstride = (long)Ncap * Hkv * d;
  a.q_hstride = bnhd ? d : (long)Nq * d;
  a.kv_hstride = bnhd ? d : (long)Ncap * d;
  a.causal = causal ? 1 : 0;
  a.tau = softmax_scale > 0.f ? softmax_scale : sqrtf(1.0f / (float)d);
  a.table = nullptr;
  a.page_size = a.num_pages = a.max_pages = 0;
  a.page_stride = 0;
  if (pg) {   // the pools: pages of [page_size][Hkv][d] or [Hkv][page_size][d]
    a.table = pg->table;
    a.page_size = pg->page_size;
    a.num_pages = pg->num_pages;
    a.max_pages = pg->max_pages;
    a.page_stride = (long)pg->page_size * Hkv * d;
    a.kv_bstride = 0;
    a.kv_hstride = bnhd ? d : (long)pg->page_size * d;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (f8) return launch_fp8_d(a, B * H, d, extend, st);
  if (extend) return dtype == FA_DTYPE_BF16 ? launch_extend_d<fa::bf16_t>(a, B * H, d, sink, st) : launch_extend_d<float>(a, B * H, d, sink, st);
  return dtype == FA_DTYPE_BF16 ? launch_d<fa::bf16_t>(a, B * H, d, sink, st) : launch_d<float>(a, B * H, d, sink, st);
}

// The argument checks of the append: FA_OK, or the error with its message set.
int check_append(const void* k_new, const void* v_new, const void* k_cache, const void* v_cache, int B, int Hkv, int Nq, int Ncap,
                 int d_new, int d, int layout, int dtype, bool extend = false) {
  g_err[0] = 0;
  if (B <= 0 || Hkv <= 0 || Nq <= 0 || Ncap <= 0 || d <= 0) return set_err(FA_ERR_BAD_ARG, "B, Hkv, Nq, Ncap and d must be positive");
  if (!extend && Nq > FA_DECODE_MAX_NQ) return set_err(FA_ERR_BAD_ARG, "Nq > 128 new tokens per call: fill the cache of a prompt directly");
  if (dtype != FA_DTYPE_F32 && dtype != FA_DTYPE_BF16) return set_err(FA_ERR_BAD_ARG, "unknown dtype");
  if (layout != FA_LAYOUT_BHND && layout != FA_LAYOUT_BNHD) return set_err(FA_ERR_BAD_ARG, "unknown layout");
  if (!k_new || !v_new || !k_cache || !v_cache) return set_err(FA_ERR_BAD_ARG, "null pointer argument (k_new, v_new and the caches)");
  if (d != 32 && d != 64 && d != 128) return set_err(FA_ERR_UNSUPPORTED_D, "decode supports cache rows of d in {32, 64, 128}");
  if (d_new < 1 || d_new > d) {
    snprintf(g_err, sizeof(g_err), "d_new = %d must be in 1 .. d = %d", d_new, d);
    return FA_ERR_BAD_ARG;
  }
  // (one lane per element at the most, 256 lanes to a workgroup, the workgroup count an int)
  if ((long)B * Nq * Hkv * d / 256 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "too many new elements for one append launch");
  return FA_OK;
}

template <typename T, int E> int launch_append(fa::RaggedAppendArgs a, int d, hipStream_t st) {
  a.ch_shift = __builtin_ctz(d / E);
  a.lanes <<= a.ch_shift;   // (rows on entry)
  const dim3 grid((unsigned)((a.lanes + 255) / 256));
  if (a.cu && a.table)
    hipLaunchKernelGGL((fa::decode_append_kernel<T, E, true, true>), grid, dim3(256), 0, st, a);
  else if (a.cu)
    hipLaunchKernelGGL((fa::decode_append_kernel<T, E, false, true>), grid, dim3(256), 0, st, a);
  else if (a.table)
    hipLaunchKernelGGL((fa::decode_append_kernel<T, E, true>), grid, dim3(256), 0, st, static_cast<const fa::AppendArgs&>(a));
  else
    hipLaunchKernelGGL((fa::decode_append_kernel<T, E>), grid, dim3(256), 0, st, static_cast<const fa::AppendArgs&>(a));
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? FA_OK : set_err(FA_ERR_HIP, "decode_append_kernel launch", e);
}

template <typename T> int launch_append_e(const fa::RaggedAppendArgs& a, int d, bool vec, hipStream_t st) {
  return vec ? launch_append<T, 16 / sizeof(T)>(a, d, st) : launch_append<T, 1>(a, d, st);
}

template <int E> int launch_append_fp8(fa::Fp8AppendArgs a, int d, hipStream_t st) {
  a.ch_shift = __builtin_ctz(d / E);
  a.lanes <<= a.ch_shift;   // (rows on entry)
  const dim3 grid((unsigned)((a.lanes + 255) / 256));
  if (a.table)
    hipLaunchKernelGGL((fa::append_fp8_kernel<E, true>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((fa::append_fp8_kernel<E>), grid, dim3(256), 0, st, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? FA_OK : set_err(FA_ERR_HIP, "append_fp8_kernel launch", e);
}

// The append launch of a checked call.  cu: the ragged append of Nq = T packed rows shared by the B sequences.
int run_append(const void* k_new, const void* v_new, void* k_cache, void* v_cache, const int* cache_seqlens, int B, int Hkv, int Nq,
               int Ncap, int d_new, int d, int layout, int dtype, void* stream, const Paging* pg = nullptr, const int* cu = nullptr,
               const Fp8* f8 = nullptr) {
  fa::RaggedAppendArgs a;
  a.k_new = k_new;
  a.v_new = v_new;
  a.k = k_cache;
  a.v = v_cache;
  a.seqlens = cache_seqlens;
  a.lanes = cu ? (long)Nq * Hkv : (long)B * Nq * Hkv;
  a.cu = cu;
  a.nseq = B;
  a.ntok = Nq;
  a.Hkv = Hkv;
  a.Nq = Nq;
  a.Ncap = Ncap;
  a.d_new = d_new;
  a.bnhd = layout == FA_LAYOUT_BNHD;
  a.kv_ld = a.bnhd ? Hkv * d : d;
  a.kv_bstride = (long)Ncap * Hkv * d;
  a.kv_hstride = a.bnhd ? d : (long)Ncap * d;
  a.table = nullptr;
  a.page_size = a.num_pages = a.max_pages = 0;
  a.page_stride = 0;
  if (pg) {
    a.table = pg->table;
    a.page_size = pg->page_size;
    a.num_pages = pg->num_pages;
    a.max_pages = pg->max_pages;
    a.page_stride = (long)pg->page_size * Hkv * d;
    a.kv_bstride = 0;
    a.kv_hstride = a.bnhd ? d : (long)pg->page_size * d;
  }
  const size_t esz = dtype == FA_DTYPE_BF16 ? 2 : 4;
  // 16-byte lanes where every row of the source starts on 16 bytes, as every row of the cache does once its base is
  const bool vec = (d_new * esz) % 16 == 0 &&
                   (((uintptr_t)k_new | (uintptr_t)v_new | (uintptr_t)k_cache | (uintptr_t)v_cache) & 15) == 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (f8) {   // bf16 sources into byte caches: eight elements to a lane where every source row starts on 16 bytes and every cache row on 8
    fa::Fp8AppendArgs fa8;
    static_cast<fa::AppendArgs&>(fa8) = a;
    fa8.k_scale = f8->k_scale;
    fa8.v_scale = f8->v_scale;
    const bool vec8 = d_new % 8 == 0 && (((uintptr_t)k_new | (uintptr_t)v_new) & 15) == 0 && (((uintptr_t)k_cache | (uintptr_t)v_cache) & 7) == 0;
    return vec8 ? launch_append_fp8<8>(fa8, d, st) : launch_append_fp8<1>(fa8, d, st);
  }
  return dtype == FA_DTYPE_BF16 ? launch_append_e<fa::bf16_t>(a, d, vec, st) : launch_append_e<float>(a, d, vec, st);
}

// ---- ragged batches (include/flash_attn_mi355x_decode_ragged.h) ----
// The argument checks of fa_mi355x_fwd_ragged: those of fa_mi355x_fwd_extend with T in the place of Nq, a null cu_seqlens_q, and
// a null workspace (the block map lives there: every ragged call needs one).  page_size > 0: a paged call, as in check_decode.
int check_ragged(const void* q, const void* k_cache, const void* v_cache, const float* out, const int* cu, const void* workspace, int B,
                 int H, int Hkv, int T, int Ncap, int d, int layout, float softmax_scale, int dtype, int page_size = 0, int window = 0,
                 int sink = 0) {
  g_err[0] = 0;
  if (B <= 0 || H <= 0 || T <= 0 || Ncap <= 0 || d <= 0) return set_err(FA_ERR_BAD_ARG, "B, H, T, Ncap and d must be positive");
  if (Hkv <= 0) return set_err(FA_ERR_BAD_ARG, "Hkv must be positive");
  if (H % Hkv != 0) {
    snprintf(g_err, sizeof(g_err), "H = %d query heads must be a multiple of Hkv = %d cache heads", H, Hkv);
    return FA_ERR_BAD_ARG;
  }
  if (dtype != FA_DTYPE_F32 && dtype != FA_DTYPE_BF16) return set_err(FA_ERR_BAD_ARG, "unknown dtype");
  if (layout != FA_LAYOUT_BHND && layout != FA_LAYOUT_BNHD) return set_err(FA_ERR_BAD_ARG, "unknown layout");
  if (!q || !k_cache || !v_cache || !out) return set_err(FA_ERR_BAD_ARG, "null pointer argument");
  if (!cu) return set_err(FA_ERR_BAD_ARG, "null cu_seqlens_q");
  if (d != 32 && d != 64 && d != 128)
    return set_err(FA_ERR_UNSUPPORTED_D, "decode supports d in {32, 64, 128}: pad the cache with zero columns for other d <= 128");
  if (softmax_scale != 0.f && (!(softmax_scale > 0.f) || !std::isfinite(softmax_scale)))
    return set_err(FA_ERR_BAD_ARG, "softmax_scale must be positive and finite (0: 1/sqrt(d))");
  // (row_query is exact for rows below 2^25; a sequence has at most G * T of them)
  if ((long)(H / Hkv) * T >= (1L << 25)) return set_err(FA_ERR_BAD_ARG, "G * T rows per kv head must stay under 2^25");
  const long esz = dtype == FA_DTYPE_BF16 ? 2 : 4;
  if (page_size > 0) {
    if (check_page_bytes(page_size, Hkv, d, dtype) != FA_OK) return FA_ERR_BAD_ARG;
  } else if (((long)Ncap + fa::DEC_ROWS) * Hkv * d * esz >= (1L << 31)) {
    return set_err(FA_ERR_BAD_ARG, "one batch element of the cache must stay under 2 GiB");
  }
  // (a sequence may own every packed row: its q resource and the (head, query) offsets inside it are 32-bit byte counts)
  if ((long)T * H * d * esz >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "q (T * H * d elements) must stay under 2 GiB");
  const int ns = rag_splits(B, H, Hkv, T, span_keys(window, Ncap, T, fa::EXT_BLOCK, sink));
  if (split_grid((long)Hkv * ns, rag_blocks(B, H, Hkv, T)) >= (1L << 32) || (long)Hkv * ns >= (1L << 31) || (long)H * T >= (1L << 32))
    return set_err(FA_ERR_BAD_ARG, "too many workgroups for one launch: Hkv * splits * row blocks and H * T must fit an unsigned int");
  if (!workspace)
    return set_err(FA_ERR_BAD_ARG, "null workspace: a ragged call always needs fa_mi355x_ragged_workspace_bytes() bytes (the block map)");
  return FA_OK;
}

// ... of fa_mi355x_ragged_append: those of fa_mi355x_extend_append with T in the place of B * Nq, and a null cu_seqlens_q.
int check_ragged_append(const void* k_new, const void* v_new, const void* k_cache, const void* v_cache, const int* cu, int B, int Hkv, int T,
                        int Ncap, int d_new, int d, int layout, int dtype) {
  g_err[0] = 0;
  if (B <= 0 || Hkv <= 0 || T <= 0 || Ncap <= 0 || d <= 0) return set_err(FA_ERR_BAD_ARG, "B, Hkv, T, Ncap and d must be positive");
  if (dtype != FA_DTYPE_F32 && dtype != FA_DTYPE_BF16) return set_err(FA_ERR_BAD_ARG, "unknown dtype");
  if (layout != FA_LAYOUT_BHND && layout != FA_LAYOUT_BNHD) return set_err(FA_ERR_BAD_ARG, "unknown layout");
  if (!k_new || !v_new || !k_cache || !v_cache) return set_err(FA_ERR_BAD_ARG, "null pointer argument (k_new, v_new and the caches)");
  if (!cu) return set_err(FA_ERR_BAD_ARG, "null cu_seqlens_q");
  if (d != 32 && d != 64 && d != 128) return set_err(FA_ERR_UNSUPPORTED_D, "decode supports cache rows of d in {32, 64, 128}");
  if (d_new < 1 || d_new > d) {
    snprintf(g_err, sizeof(g_err), "d_new = %d must be in 1 .. d = %d", d_new, d);
    return FA_ERR_BAD_ARG;
  }
  // (the kernel counts packed rows in an int; one lane per element at the most, the workgroup count an int)
  if ((long)T * Hkv * d / 256 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "too many new elements for one append launch");
  return FA_OK;
}

template <typename T, int D> int launch_ragged(fa::RaggedArgs a, int sink, hipStream_t st) {
  hipLaunchKernelGGL(fa::ragged_schedule_kernel, dim3(1), dim3(256), 0, st, a.cu, const_cast<int*>(a.map), a.nseq, a.ntok, a.G, a.nqb);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_err(FA_ERR_HIP, "ragged_schedule_kernel launch", e);
  const dim3 grid((unsigned)split_grid(a.items, a.nqb));
  if (sink) {   // (the sink builds: their own kernels and argument; a.window >= 1)
    fa::RaggedSinkArgs sa;
    static_cast<fa::RaggedArgs&>(sa) = a;
    sa.sink = sink;
    if (a.table)
      hipLaunchKernelGGL((fa::extend_split_sink_kernel<T, D, true, true>), grid, dim3(256), 0, st, sa);
    else
      hipLaunchKernelGGL((fa::extend_split_sink_kernel<T, D, false, true>), grid, dim3(256), 0, st, sa);
  } else if (a.window && a.table)
    hipLaunchKernelGGL((fa::extend_split_kernel<T, D, true, true, true>), grid, dim3(256), 0, st, a);
  else if (a.window)
    hipLaunchKernelGGL((fa::extend_split_kernel<T, D, false, true, true>), grid, dim3(256), 0, st, a);
  else if (a.table)
    hipLaunchKernelGGL((fa::extend_split_kernel<T, D, true, true>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((fa::extend_split_kernel<T, D, false, true>), grid, dim3(256), 0, st, a);
  e = hipGetLastError();
  if (e != hipSuccess) return set_err(FA_ERR_HIP, "extend_split_kernel (ragged) launch", e);
  if (a.nsplit > 1) {
    hipLaunchKernelGGL((fa::decode_combine_kernel<D, true>), dim3((unsigned)((long)a.H * a.ntok)), dim3(256), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return set_err(FA_ERR_HIP, "decode_combine_kernel (ragged) launch", e);
  }
  return FA_OK;
}

template <typename T> int launch_ragged_d(const fa::RaggedArgs& a, int d, int sink, hipStream_t st) {
  switch (d) {
    case 32: return launch_ragged<T, 32>(a, sink, st);
    case 64: return launch_ragged<T, 64>(a, sink, st);
    default: return launch_ragged<T, 128>(a, sink, st);
  }
}

// The schedule, split (and combine) launches of a checked ragged call.
int run_ragged(const void* q, const void* k_cache, const void* v_cache, float* out, float* lse, const int* cu, const int* cache_seqlens,
               void* workspace, int B, int H, int Hkv, int T, int Ncap, int d, int layout, float softmax_scale, int causal, int dtype,
               void* stream, const Paging* pg, int window = 0, int sink = 0) {
  const int span = span_keys(window, Ncap, T, fa::EXT_BLOCK, sink);   // (no window: Ncap; a sequence may own all T rows)
  const int ns = rag_splits(B, H, Hkv, T, span);
  fa::RaggedArgs a;
  a.q = q;
  a.k = k_cache;
  a.v = v_cache;
  a.out = out;
  a.lse = lse;
  a.map = static_cast<const int*>(workspace);
  a.part_o = reinterpret_cast<float*>(static_cast<char*>(workspace) + rag_map_bytes(B, H, Hkv, T));
  a.part_ml = a.part_o + (size_t)H * ns * T * d;
  a.seqlens = cache_seqlens;
  a.cu = cu;
  a.nseq = B;
  a.ntok = T;
  a.H = H;
  a.Hkv = Hkv;
  a.G = H / Hkv;
  a.inv_G = 1.0f / (float)a.G;
  a.Nq = T;   // (the combine kernel's view: one batch element of T queries)
  a.Ncap = Ncap;
  a.nsplit = ns;
  a.chunk = rag_chunk_keys(B, H, Hkv, T, span);
  a.window = win_of(window, Ncap, sink);
  sink = sink_of(window, sink, Ncap);
  a.nqb = (int)rag_blocks(B, H, Hkv, T);
  a.items = Hkv * ns;
  const bool bnhd = layout == FA_LAYOUT_BNHD;
  a.q_ld = H * d;   // (the packed buffers are token-major whatever the caches' layout)
  a.q_hstride = d;
  a.q_bstride = (long)T * H * d;
  a.kv_ld = bnhd ? Hkv * d : d;
  a.kv_bstride = (long)Ncap * Hkv * d;
  a.kv_hstride = bnhd ? d : (long)Ncap * d;
  a.causal = causal ? 1 : 0;
  a.tau = softmax_scale > 0.f ? softmax_scale : sqrtf(1.0f / (float)d);
  a.table = nullptr;
  a.page_size = a.num_pages = a.max_pages = 0;
  a.page_stride = 0;
  if (pg) {
    a.table = pg->table;
    a.page_size = pg->page_size;
    a.num_pages = pg->num_pages;
    a.max_pages = pg->max_pages;
    a.page_stride = (long)pg->page_size * Hkv * d;
    a.kv_bstride = 0;
    a.kv_hstride = bnhd ? d : (long)pg->page_size * d;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dtype == FA_DTYPE_BF16 ? launch_ragged_d<fa::bf16_t>(a, d, sink, st) : launch_ragged_d<float>(a, d, sink, st);
}

// One ragged call: the attention (attend), the append (append), or the append then the attention; pg: the paged form.
int ragged_call(bool attend, bool append, const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out,
                float* lse, const int* cu, const int* cache_seqlens, const Paging* pg, void* workspace, int B, int H, int Hkv, int T, int Ncap,
                int d_new, int d, int layout, float softmax_scale, int causal, int dtype, void* stream, int window = 0, int sink = 0) {
  int rc = pg ? check_pages(*pg, &Ncap) : FA_OK;
  if (rc == FA_OK && attend)
    rc = check_ragged(q, k_cache, v_cache, out, cu, workspace, B, H, Hkv, T, Ncap, d, layout, softmax_scale, dtype, pg ? pg->page_size : 0,
                      window, sink);
  if (rc == FA_OK && append) rc = check_ragged_append(k_new, v_new, k_cache, v_cache, cu, B, Hkv, T, Ncap, d_new, d, layout, dtype);
  if (rc == FA_OK && append && pg) rc = check_page_bytes(pg->page_size, Hkv, d, dtype);
  if (rc != FA_OK) return rc;
  if (append) {
    rc = run_append(k_new, v_new, k_cache, v_cache, cache_seqlens, B, Hkv, T, Ncap, d_new, d, layout, dtype, stream, pg, cu);
    if (rc != FA_OK || !attend) return rc;
  }
  return run_ragged(q, k_cache, v_cache, out, lse, cu, cache_seqlens, workspace, B, H, Hkv, T, Ncap, d, layout, softmax_scale, causal, dtype,
                    stream, pg, window, sink);
}

}  // namespace

extern "C" {

size_t fa_mi355x_decode_workspace_bytes_gqa(int B, int H, int Hkv, int Nq, int Ncap, int d) {
  if (!sizes_ok(B, H, Hkv, Nq, Ncap, d)) return 0;
  return workspace_bytes(B, H, Hkv, Nq, Ncap, d);
}

int fa_mi355x_decode_splits_gqa(int B, int H, int Hkv, int Nq, int Ncap, int d, int dtype) {
  (void)dtype;
  if (!sizes_ok(B, H, Hkv, Nq, Ncap, d)) return 0;
  return splits(B, H, Hkv, Nq, Ncap);
}

int fa_mi355x_fwd_decode_gqa(const void* q, const void* k_cache, const void* v_cache, float* out, float* lse, const int* cache_seqlens,
                             void* workspace, int B, int H, int Hkv, int Nq, int Ncap, int d, int layout, float softmax_scale,
                             int causal, int dtype, void* stream) {
  const int rc = check_decode(q, k_cache, v_cache, out, workspace, B, H, Hkv, Nq, Ncap, d, layout, softmax_scale, dtype);
  if (rc != FA_OK) return rc;
  return run_decode(q, k_cache, v_cache, out, lse, cache_seqlens, workspace, B, H, Hkv, Nq, Ncap, d, layout, softmax_scale, causal, dtype,
                    stream);
}

int fa_mi355x_decode_append(const void* k_new, const void* v_new, void* k_cache, void* v_cache, const int* cache_seqlens, int B, int Hkv,
                            int Nq, int Ncap, int d_new, int d, int layout, int dtype, void* stream) {
  const int rc = check_append(k_new, v_new, k_cache, v_cache, B, Hkv, Nq, Ncap, d_new, d, layout, dtype);
  if (rc != FA_OK) return rc;
  return run_append(k_new, v_new, k_cache, v_cache, cache_seqlens, B, Hkv, Nq, Ncap, d_new, d, layout, dtype, stream);
}

int fa_mi355x_fwd_decode_append(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                                const int* cache_seqlens, void* workspace, int B, int H, int Hkv, int Nq, int Ncap, int d_new, int d,
                                int layout, float softmax_scale, int causal, int dtype, void* stream) {
  int rc = check_decode(q, k_cache, v_cache, out, workspace, B, H, Hkv, Nq, Ncap, d, layout, softmax_scale, dtype);
  if (rc == FA_OK) rc = check_append(k_new, v_new, k_cache, v_cache, B, Hkv, Nq, Ncap, d_new, d, layout, dtype);
  if (rc != FA_OK) return rc;
  rc = run_append(k_new, v_new, k_cache, v_cache, cache_seqlens, B, Hkv, Nq, Ncap, d_new, d, layout, dtype, stream);
  if (rc != FA_OK) return rc;
  return run_decode(q, k_cache, v_cache, out, lse, cache_seqlens, workspace, B, H, Hkv, Nq, Ncap, d, layout, softmax_scale, causal, dtype,
                    stream);
}

// The extend entry points: any Nq, the extend kernels and their policy; the append is the decode library's own.
size_t fa_mi355x_extend_workspace_bytes(int B, int H, int Hkv, int Nq, int Ncap, int d) {
  if (!sizes_ok(B, H, Hkv, Nq, Ncap, d)) return 0;
  return ext_workspace_bytes(B, H, Hkv, Nq, Ncap, d);
}

int fa_mi355x_extend_splits(int B, int H, int Hkv, int Nq, int Ncap, int d, int dtype) {
  (void)dtype;
  if (!sizes_ok(B, H, Hkv, Nq, Ncap, d)) return 0;
  return ext_splits(B, H, Hkv, Nq, Ncap);
}

int fa_mi355x_fwd_extend(const void* q, const void* k_cache, const void* v_cache, float* out, float* lse, const int* cache_seqlens,
                         void* workspace, int B, int H, int Hkv, int Nq, int Ncap, int d, int layout, float softmax_scale, int causal,
                         int dtype, void* stream) {
  const int rc = check_decode(q, k_cache, v_cache, out, workspace, B, H, Hkv, Nq, Ncap, d, layout, softmax_scale, dtype, true);
  if (rc != FA_OK) return rc;
  return run_decode(q, k_cache, v_cache, out, lse, cache_seqlens, workspace, B, H, Hkv, Nq, Ncap, d, layout, softmax_scale, causal, dtype,
                    stream, true);
}

int fa_mi355x_extend_append(const void* k_new, const void* v_new, void* k_cache, void* v_cache, const int* cache_seqlens, int B, int Hkv,
                            int Nq, int Ncap, int d_new, int d, int layout, int dtype, void* stream) {
  const int rc = check_append(k_new, v_new, k_cache, v_cache, B, Hkv, Nq, Ncap, d_new, d, layout, dtype, true);
  if (rc != FA_OK) return rc;
  return run_append(k_new, v_new, k_cache, v_cache, cache_seqlens, B, Hkv, Nq, Ncap, d_new, d, layout, dtype, stream);
}

int fa_mi355x_fwd_extend_append(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                                const int* cache_seqlens, void* workspace, int B, int H, int Hkv, int Nq, int Ncap, int d_new, int d,
                                int layout, float softmax_scale, int causal, int dtype, void* stream) {
  int rc = check_decode(q, k_cache, v_cache, out, workspace, B, H, Hkv, Nq, Ncap, d, layout, softmax_scale, dtype, true);
  if (rc == FA_OK) rc = check_append(k_new, v_new, k_cache, v_cache, B, Hkv, Nq, Ncap, d_new, d, layout, dtype, true);
  if (rc != FA_OK) return rc;
  rc = run_append(k_new, v_new, k_cache, v_cache, cache_seqlens, B, Hkv, Nq, Ncap, d_new, d, layout, dtype, stream);
  if (rc != FA_OK) return rc;
  return run_decode(q, k_cache, v_cache, out, lse, cache_seqlens, workspace, B, H, Hkv, Nq, Ncap, d, layout, softmax_scale, causal, dtype,
                    stream, true);
}

// The paged entry points: the _gqa / extend forms above on a pool of pages read through a block table.
namespace {

// One decode or extend call, fused with the append or not, on a pool (pg: Ncap comes from its geometry) or on slabs of Ncap rows
// (pg null), windowed or not.
int attend(bool extend, bool fused, const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
           const int* cache_seqlens, const Paging* pg, void* workspace, int B, int H, int Hkv, int Nq, int Ncap, int d_new, int d, int layout,
           float softmax_scale, int causal, int dtype, void* stream, int window = 0, const Fp8* f8 = nullptr, int sink = 0) {
  int rc = pg ? check_pages(*pg, &Ncap) : FA_OK;
  if (rc == FA_OK)
    rc = check_decode(q, k_cache, v_cache, out, workspace, B, H, Hkv, Nq, Ncap, d, layout, softmax_scale, dtype, extend, pg ? pg->page_size : 0,
                      window, f8 != nullptr, sink);
  if (rc == FA_OK && fused) rc = check_append(k_new, v_new, k_cache, v_cache, B, Hkv, Nq, Ncap, d_new, d, layout, dtype, extend);
  if (rc != FA_OK) return rc;
  if (fused) {
    rc = run_append(k_new, v_new, k_cache, v_cache, cache_seqlens, B, Hkv, Nq, Ncap, d_new, d, layout, dtype, stream, pg, nullptr, f8);
    if (rc != FA_OK) return rc;
  }
  return run_decode(q, k_cache, v_cache, out, lse, cache_seqlens, workspace, B, H, Hkv, Nq, Ncap, d, layout, softmax_scale, causal, dtype,
                    stream, extend, pg, window, f8, sink);
}

// The check an fp8 call makes first: the queries and the new tokens are bf16.
int check_fp8(int dtype) {
  g_err[0] = 0;
  if (dtype == FA_DTYPE_F32)
    return set_err(FA_ERR_BAD_ARG, "an fp8 cache takes bf16 queries and new tokens: FA_DTYPE_F32 is not supported (dtype must be FA_DTYPE_BF16)");
  if (dtype != FA_DTYPE_BF16) return set_err(FA_ERR_BAD_ARG, "unknown dtype");
  return FA_OK;
}

// The checks a windowed call makes first (sink: 0 in the calls that have none).
int check_window(int window, int causal, int sink = 0) {
  g_err[0] = 0;
  if (sink < 0) return set_err(FA_ERR_BAD_ARG, "sink must not be negative (0: no sink tokens)");
  if (window < 0) return set_err(FA_ERR_BAD_ARG, "window must not be negative (0: no window)");
  if (window > 0 && !causal)
    return set_err(FA_ERR_BAD_ARG, "a sliding window needs the causal mask: window > 0 with causal = 0 (the window ends at the query's position)");
  return FA_OK;
}

int append_paged(bool extend, const void* k_new, const void* v_new, void* k_pool, void* v_pool, const int* cache_seqlens, const Paging& pg,
                 int B, int Hkv, int Nq, int d_new, int d, int layout, int dtype, void* stream) {
  int Ncap = 0;
  int rc = check_pages(pg, &Ncap);
  if (rc == FA_OK) rc = check_append(k_new, v_new, k_pool, v_pool, B, Hkv, Nq, Ncap, d_new, d, layout, dtype, extend);
  if (rc == FA_OK) rc = check_page_bytes(pg.page_size, Hkv, d, dtype);
  if (rc != FA_OK) return rc;
  return run_append(k_new, v_new, k_pool, v_pool, cache_seqlens, B, Hkv, Nq, Ncap, d_new, d, layout, dtype, stream, &pg);
}

}  // namespace

int fa_mi355x_fwd_decode_paged(const void* q, const void* k_pool, const void* v_pool, float* out, float* lse, const int* cache_seqlens,
                               const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int num_pages, int page_size,
                               int max_pages, int d, int layout, float softmax_scale, int causal, int dtype, void* stream) {
  const Paging pg = {block_table, num_pages, page_size, max_pages};
  return attend(false, false, q, nullptr, nullptr, const_cast<void*>(k_pool), const_cast<void*>(v_pool), out, lse, cache_seqlens, &pg,
                workspace, B, H, Hkv, Nq, 0, d, d, layout, softmax_scale, causal, dtype, stream);
}

int fa_mi355x_fwd_extend_paged(const void* q, const void* k_pool, const void* v_pool, float* out, float* lse, const int* cache_seqlens,
                               const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int num_pages, int page_size,
                               int max_pages, int d, int layout, float softmax_scale, int causal, int dtype, void* stream) {
  const Paging pg = {block_table, num_pages, page_size, max_pages};
  return attend(true, false, q, nullptr, nullptr, const_cast<void*>(k_pool), const_cast<void*>(v_pool), out, lse, cache_seqlens, &pg,
                workspace, B, H, Hkv, Nq, 0, d, d, layout, softmax_scale, causal, dtype, stream);
}

int fa_mi355x_decode_append_paged(const void* k_new, const void* v_new, void* k_pool, void* v_pool, const int* cache_seqlens,
                                  const int* block_table, int B, int Hkv, int Nq, int num_pages, int page_size, int max_pages, int d_new,
                                  int d, int layout, int dtype, void* stream) {
  const Paging pg = {block_table, num_pages, page_size, max_pages};
  return append_paged(false, k_new, v_new, k_pool, v_pool, cache_seqlens, pg, B, Hkv, Nq, d_new, d, layout, dtype, stream);
}

int fa_mi355x_extend_append_paged(const void* k_new, const void* v_new, void* k_pool, void* v_pool, const int* cache_seqlens,
                                  const int* block_table, int B, int Hkv, int Nq, int num_pages, int page_size, int max_pages, int d_new,
                                  int d, int layout, int dtype, void* stream) {
  const Paging pg = {block_table, num_pages, page_size, max_pages};
  return append_paged(true, k_new, v_new, k_pool, v_pool, cache_seqlens, pg, B, Hkv, Nq, d_new, d, layout, dtype, stream);
}

int fa_mi355x_fwd_decode_append_paged(const void* q, const void* k_new, const void* v_new, void* k_pool, void* v_pool, float* out,
                                      float* lse, const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv,
                                      int Nq, int num_pages, int page_size, int max_pages, int d_new, int d, int layout,
                                      float softmax_scale, int causal, int dtype, void* stream) {
  const Paging pg = {block_table, num_pages, page_size, max_pages};
  return attend(false, true, q, k_new, v_new, k_pool, v_pool, out, lse, cache_seqlens, &pg, workspace, B, H, Hkv, Nq, 0, d_new, d, layout,
                softmax_scale, causal, dtype, stream);
}

int fa_mi355x_fwd_extend_append_paged(const void* q, const void* k_new, const void* v_new, void* k_pool, void* v_pool, float* out,
                                      float* lse, const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv,
                                      int Nq, int num_pages, int page_size, int max_pages, int d_new, int d, int layout,
                                      float softmax_scale, int causal, int dtype, void* stream) {
  const Paging pg = {block_table, num_pages, page_size, max_pages};
  return attend(true, true, q, k_new, v_new, k_pool, v_pool, out, lse, cache_seqlens, &pg, workspace, B, H, Hkv, Nq, 0, d_new, d, layout,
                softmax_scale, causal, dtype, stream);
}

// The ragged entry points (include/flash_attn_mi355x_decode_ragged.h): the new tokens of all sequences packed into T rows, the
// sequences' boundaries in cu_seqlens_q on the device.
int fa_mi355x_ragged_splits(int B, int H, int Hkv, int T, int Ncap, int d, int dtype) {
  (void)dtype;
  if (!sizes_ok(B, H, Hkv, T, Ncap, d)) return 0;
  return rag_splits(B, H, Hkv, T, Ncap);
}

size_t fa_mi355x_ragged_workspace_bytes(int B, int H, int Hkv, int T, int Ncap, int d) {
  if (!sizes_ok(B, H, Hkv, T, Ncap, d)) return 0;
  return rag_workspace_bytes(B, H, Hkv, T, Ncap, d);
}

int fa_mi355x_fwd_ragged(const void* q, const void* k_cache, const void* v_cache, float* out, float* lse, const int* cu_seqlens_q,
                         const int* cache_seqlens, void* workspace, int B, int H, int Hkv, int T, int Ncap, int d, int layout,
                         float softmax_scale, int causal, int dtype, void* stream) {
  return ragged_call(true, false, q, nullptr, nullptr, const_cast<void*>(k_cache), const_cast<void*>(v_cache), out, lse, cu_seqlens_q,
                     cache_seqlens, nullptr, workspace, B, H, Hkv, T, Ncap, d, d, layout, softmax_scale, causal, dtype, stream);
}

int fa_mi355x_ragged_append(const void* k_new, const void* v_new, void* k_cache, void* v_cache, const int* cu_seqlens_q,
                            const int* cache_seqlens, int B, int Hkv, int T, int Ncap, int d_new, int d, int layout, int dtype,
                            void* stream) {
  return ragged_call(false, true, nullptr, k_new, v_new, k_cache, v_cache, nullptr, nullptr, cu_seqlens_q, cache_seqlens, nullptr, nullptr, B,
                     Hkv, Hkv, T, Ncap, d_new, d, layout, 0.f, 0, dtype, stream);
}

int fa_mi355x_fwd_ragged_append(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                                const int* cu_seqlens_q, const int* cache_seqlens, void* workspace, int B, int H, int Hkv, int T,
                                int Ncap, int d_new, int d, int layout, float softmax_scale, int causal, int dtype, void* stream) {
  return ragged_call(true, true, q, k_new, v_new, k_cache, v_cache, out, lse, cu_seqlens_q, cache_seqlens, nullptr, workspace, B, H, Hkv, T,
                     Ncap, d_new, d, layout, softmax_scale, causal, dtype, stream);
}

int fa_mi355x_fwd_ragged_paged(const void* q, const void* k_pool, const void* v_pool, float* out, float* lse, const int* cu_seqlens_q,
                               const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv, int T,
                               int num_pages, int page_size, int max_pages, int d, int layout, float softmax_scale, int causal,
                               int dtype, void* stream) {
  const Paging pg = {block_table, num_pages, page_size, max_pages};
  return ragged_call(true, false, q, nullptr, nullptr, const_cast<void*>(k_pool), const_cast<void*>(v_pool), out, lse, cu_seqlens_q,
                     cache_seqlens, &pg, workspace, B, H, Hkv, T, 0, d, d, layout, softmax_scale, causal, dtype, stream);
}

int fa_mi355x_ragged_append_paged(const void* k_new, const void* v_new, void* k_pool, void* v_pool, const int* cu_seqlens_q,
                                  const int* cache_seqlens, const int* block_table, int B, int Hkv, int T, int num_pages, int page_size,
                                  int max_pages, int d_new, int d, int layout, int dtype, void* stream) {
  const Paging pg = {block_table, num_pages, page_size, max_pages};
  return ragged_call(false, true, nullptr, k_new, v_new, k_pool, v_pool, nullptr, nullptr, cu_seqlens_q, cache_seqlens, &pg, nullptr, B, Hkv,
                     Hkv, T, 0, d_new, d, layout, 0.f, 0, dtype, stream);
}

int fa_mi355x_fwd_ragged_append_paged(const void* q, const void* k_new, const void* v_new, void* k_pool, void* v_pool, float* out,
                                      float* lse, const int* cu_seqlens_q, const int* cache_seqlens, const int* block_table,
                                      void* workspace, int B, int H, int Hkv, int T, int num_pages, int page_size, int max_pages,
                                      int d_new, int d, int layout, float softmax_scale, int causal, int dtype, void* stream) {
  const Paging pg = {block_table, num_pages, page_size, max_pages};
  return ragged_call(true, true, q, k_new, v_new, k_pool, v_pool, out, lse, cu_seqlens_q, cache_seqlens, &pg, workspace, B, H, Hkv, T, 0,
                     d_new, d, layout, softmax_scale, causal, dtype, stream);
}

// The windowed entry points (include/flash_attn_mi355x_decode_window.h): one per call family.  k_new / v_new null: attend only;
// block_table null: slabs of Ncap rows, otherwise the pool's geometry stands for Ncap.
int fa_mi355x_decode_window_splits(int B, int H, int Hkv, int Nq, int Ncap, int d, int dtype, int window) {
  (void)dtype;
  if (!sizes_ok(B, H, Hkv, Nq, Ncap, d) || window < 0) return 0;
  return splits(B, H, Hkv, Nq, span_keys(window, Ncap, Nq, 32));
}

size_t fa_mi355x_decode_window_workspace_bytes(int B, int H, int Hkv, int Nq, int Ncap, int d, int window) {
  if (!sizes_ok(B, H, Hkv, Nq, Ncap, d) || window < 0) return 0;
  return workspace_bytes(B, H, Hkv, Nq, span_keys(window, Ncap, Nq, 32), d);
}

int fa_mi355x_extend_window_splits(int B, int H, int Hkv, int Nq, int Ncap, int d, int dtype, int window) {
  (void)dtype;
  if (!sizes_ok(B, H, Hkv, Nq, Ncap, d) || window < 0) return 0;
  return ext_splits(B, H, Hkv, Nq, span_keys(window, Ncap, Nq, fa::EXT_BLOCK));
}

size_t fa_mi355x_extend_window_workspace_bytes(int B, int H, int Hkv, int Nq, int Ncap, int d, int window) {
  if (!sizes_ok(B, H, Hkv, Nq, Ncap, d) || window < 0) return 0;
  return ext_workspace_bytes(B, H, Hkv, Nq, span_keys(window, Ncap, Nq, fa::EXT_BLOCK), d);
}

int fa_mi355x_ragged_window_splits(int B, int H, int Hkv, int T, int Ncap, int d, int dtype, int window) {
  (void)dtype;
  if (!sizes_ok(B, H, Hkv, T, Ncap, d) || window < 0) return 0;
  return rag_splits(B, H, Hkv, T, span_keys(window, Ncap, T, fa::EXT_BLOCK));
}

size_t fa_mi355x_ragged_window_workspace_bytes(int B, int H, int Hkv, int T, int Ncap, int d, int window) {
  if (!sizes_ok(B, H, Hkv, T, Ncap, d) || window < 0) return 0;
  return rag_workspace_bytes(B, H, Hkv, T, span_keys(window, Ncap, T, fa::EXT_BLOCK), d);
}

int fa_mi355x_fwd_decode_window(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                                const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int Ncap,
                                int num_pages, int page_size, int max_pages, int d_new, int d, int layout, float softmax_scale, int causal,
                                int window, int dtype, void* stream) {
  const int rc = check_window(window, causal);
  if (rc != FA_OK) return rc;
  const Paging pg = {block_table, num_pages, page_size, max_pages};
  return attend(false, k_new || v_new, q, k_new, v_new, k_cache, v_cache, out, lse, cache_seqlens, block_table ? &pg : nullptr, workspace, B, H,
                Hkv, Nq, Ncap, d_new, d, layout, softmax_scale, causal, dtype, stream, window);
}

int fa_mi355x_fwd_extend_window(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                                const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int Ncap,
                                int num_pages, int page_size, int max_pages, int d_new, int d, int layout, float softmax_scale, int causal,
                                int window, int dtype, void* stream) {
  const int rc = check_window(window, causal);
  if (rc != FA_OK) return rc;
  const Paging pg = {block_table, num_pages, page_size, max_pages};
  return attend(true, k_new || v_new, q, k_new, v_new, k_cache, v_cache, out, lse, cache_seqlens, block_table ? &pg : nullptr, workspace, B, H,
                Hkv, Nq, Ncap, d_new, d, layout, softmax_scale, causal, dtype, stream, window);
}

int fa_mi355x_fwd_ragged_window(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                                const int* cu_seqlens_q, const int* cache_seqlens, const int* block_table, void* workspace, int B, int H,
                                int Hkv, int T, int Ncap, int num_pages, int page_size, int max_pages, int d_new, int d, int layout,
                                float softmax_scale, int causal, int window, int dtype, void* stream) {
  const int rc = check_window(window, causal);
  if (rc != FA_OK) return rc;
  const Paging pg = {block_table, num_pages, page_size, max_pages};
  return ragged_call(true, k_new || v_new, q, k_new, v_new, k_cache, v_cache, out, lse, cu_seqlens_q, cache_seqlens,
                     block_table ? &pg : nullptr, workspace, B, H, Hkv, T, Ncap, d_new, d, layout, softmax_scale, causal, dtype, stream, window);
}

// The sink entry points (include/flash_attn_mi355x_decode_sink.h): the windowed ones with `sink` first positions kept beside the window.
int fa_mi355x_decode_sink_splits(int B, int H, int Hkv, int Nq, int Ncap, int d, int dtype, int window, int sink) {
  (void)dtype;
  if (!sizes_ok(B, H, Hkv, Nq, Ncap, d) || window < 0 || sink < 0) return 0;
  return splits(B, H, Hkv, Nq, span_keys(window, Ncap, Nq, 32, sink));
}

size_t fa_mi355x_decode_sink_workspace_bytes(int B, int H, int Hkv, int Nq, int Ncap, int d, int window, int sink) {
  if (!sizes_ok(B, H, Hkv, Nq, Ncap, d) || window < 0 || sink < 0) return 0;
  return workspace_bytes(B, H, Hkv, Nq, span_keys(window, Ncap, Nq, 32, sink), d);
}

int fa_mi355x_extend_sink_splits(int B, int H, int Hkv, int Nq, int Ncap, int d, int dtype, int window, int sink) {
  (void)dtype;
  if (!sizes_ok(B, H, Hkv, Nq, Ncap, d) || window < 0 || sink < 0) return 0;
  return ext_splits(B, H, Hkv, Nq, span_keys(window, Ncap, Nq, fa::EXT_BLOCK, sink));
}

size_t fa_mi355x_extend_sink_workspace_bytes(int B, int H, int Hkv, int Nq, int Ncap, int d, int window, int sink) {
  if (!sizes_ok(B, H, Hkv, Nq, Ncap, d) || window < 0 || sink < 0) return 0;
  return ext_workspace_bytes(B, H, Hkv, Nq, span_keys(window, Ncap, Nq, fa::EXT_BLOCK, sink), d);
}

int fa_mi355x_ragged_sink_splits(int B, int H, int Hkv, int T, int Ncap, int d, int dtype, int window, int sink) {
  (void)dtype;
  if (!sizes_ok(B, H, Hkv, T, Ncap, d) || window < 0 || sink < 0) return 0;
  return rag_splits(B, H, Hkv, T, span_keys(window, Ncap, T, fa::EXT_BLOCK, sink));
}

size_t fa_mi355x_ragged_sink_workspace_bytes(int B, int H, int Hkv, int T, int Ncap, int d, int window, int sink) {
  if (!sizes_ok(B, H, Hkv, T, Ncap, d) || window < 0 || sink < 0) return 0;
  return rag_workspace_bytes(B, H, Hkv, T, span_keys(window, Ncap, T, fa::EXT_BLOCK, sink), d);
}

int fa_mi355x_fwd_decode_sink(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                              const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int Ncap,
                              int num_pages, int page_size, int max_pages, int d_new, int d, int layout, float softmax_scale, int causal,
                              int window, int sink, int dtype, void* stream) {
  const int rc = check_window(window, causal, sink);
  if (rc != FA_OK) return rc;
  const Paging pg = {block_table, num_pages, page_size, max_pages};
  return attend(false, k_new || v_new, q, k_new, v_new, k_cache, v_cache, out, lse, cache_seqlens, block_table ? &pg : nullptr, workspace, B, H,
                Hkv, Nq, Ncap, d_new, d, layout, softmax_scale, causal, dtype, stream, window, nullptr, sink);
}

int fa_mi355x_fwd_extend_sink(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                              const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int Ncap,
                              int num_pages, int page_size, int max_pages, int d_new, int d, int layout, float softmax_scale, int causal,
                              int window, int sink, int dtype, void* stream) {
  const int rc = check_window(window, causal, sink);
  if (rc != FA_OK) return rc;
  const Paging pg = {block_table, num_pages, page_size, max_pages};
  return attend(true, k_new || v_new, q, k_new, v_new, k_cache, v_cache, out, lse, cache_seqlens, block_table ? &pg : nullptr, workspace, B, H,
                Hkv, Nq, Ncap, d_new, d, layout, softmax_scale, causal, dtype, stream, window, nullptr, sink);
}

int fa_mi355x_fwd_ragged_sink(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                              const int* cu_seqlens_q, const int* cache_seqlens, const int* block_table, void* workspace, int B, int H,
                              int Hkv, int T, int Ncap, int num_pages, int page_size, int max_pages, int d_new, int d, int layout,
                              float softmax_scale, int causal, int window, int sink, int dtype, void* stream) {
  const int rc = check_window(window, causal, sink);
  if (rc != FA_OK) return rc;
  const Paging pg = {block_table, num_pages, page_size, max_pages};
  return ragged_call(true, k_new || v_new, q, k_new, v_new, k_cache, v_cache, out, lse, cu_seqlens_q, cache_seqlens,
                     block_table ? &pg : nullptr, workspace, B, H, Hkv, T, Ncap, d_new, d, layout, softmax_scale, causal, dtype, stream, window,
                     sink);
}

// The fp8 entry points (include/flash_attn_mi355x_decode_fp8.h): caches of e4m3 bytes with per-kv-head scales.  k_new / v_new null:
// attend only; block_table null: slabs of Ncap rows.
int fa_mi355x_fwd_decode_fp8(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, const float* k_scale,
                             const float* v_scale, float* out, float* lse, const int* cache_seqlens, const int* block_table, void* workspace,
                             int B, int H, int Hkv, int Nq, int Ncap, int num_pages, int page_size, int max_pages, int d_new, int d,
                             int layout, float softmax_scale, int causal, int dtype, void* stream) {
  const int rc = check_fp8(dtype);
  if (rc != FA_OK) return rc;
  const Paging pg = {block_table, num_pages, page_size, max_pages};
  const Fp8 f8 = {k_scale, v_scale};
  return attend(false, k_new || v_new, q, k_new, v_new, k_cache, v_cache, out, lse, cache_seqlens, block_table ? &pg : nullptr, workspace, B, H,
                Hkv, Nq, Ncap, d_new, d, layout, softmax_scale, causal, dtype, stream, 0, &f8);
}

int fa_mi355x_fwd_extend_fp8(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, const float* k_scale,
                             const float* v_scale, float* out, float* lse, const int* cache_seqlens, const int* block_table, void* workspace,
                             int B, int H, int Hkv, int Nq, int Ncap, int num_pages, int page_size, int max_pages, int d_new, int d,
                             int layout, float softmax_scale, int causal, int dtype, void* stream) {
  const int rc = check_fp8(dtype);
  if (rc != FA_OK) return rc;
  const Paging pg = {block_table, num_pages, page_size, max_pages};
  const Fp8 f8 = {k_scale, v_scale};
  return attend(true, k_new || v_new, q, k_new, v_new, k_cache, v_cache, out, lse, cache_seqlens, block_table ? &pg : nullptr, workspace, B, H,
                Hkv, Nq, Ncap, d_new, d, layout, softmax_scale, causal, dtype, stream, 0, &f8);
}

int fa_mi355x_append_fp8(const void* k_new, const void* v_new, void* k_cache, void* v_cache, const float* k_scale, const float* v_scale,
                         const int* cache_seqlens, const int* block_table, int B, int Hkv, int Nq, int Ncap, int num_pages, int page_size,
                         int max_pages, int d_new, int d, int layout, int dtype, void* stream) {
  int rc = check_fp8(dtype);
  const Paging pg = {block_table, num_pages, page_size, max_pages};
  if (rc == FA_OK && block_table) rc = check_pages(pg, &Ncap);
  if (rc == FA_OK) rc = check_append(k_new, v_new, k_cache, v_cache, B, Hkv, Nq, Ncap, d_new, d, layout, dtype, true);
  if (rc == FA_OK) {   // (a store's row offset is added to a 64-bit address: the bound is the attention's, whose loads read these rows)
    if (block_table)
      rc = check_page_bytes(page_size, Hkv, d, dtype, true);
    else if (((long)Ncap + fa::DEC_ROWS) * Hkv * d >= (1L << 31))
      rc = set_err(FA_ERR_BAD_ARG, "one batch element of the cache must stay under 2 GiB");
  }
  if (rc != FA_OK) return rc;
  const Fp8 f8 = {k_scale, v_scale};
  return run_append(k_new, v_new, k_cache, v_cache, cache_seqlens, B, Hkv, Nq, Ncap, d_new, d, layout, dtype, stream, block_table ? &pg : nullptr,
                    nullptr, &f8);
}

// The rotary entry points (include/flash_attn_mi355x_decode_rope.h): a tensor rotated by position, and the roped append that goes
// in front of the EXISTING attend-only entry points (rope_kernel and rope_append_kernel of fa_rope.h; no attention kernel changes).
}  // extern "C"  (the launchers below are templates)

namespace {

// The checks of the tables and the rotary dimension; row_len: the shortest row that is rotated.
int check_rope(const void* cos, const void* sin, int rot, int row_len, int max_pos, int interleaved, int inverse) {
  if (!cos || !sin) return set_err(FA_ERR_BAD_ARG, "null cos or sin (the rotary tables, fp32 [max_pos][rot / 2])");
  if (interleaved != 0 && interleaved != 1) return set_err(FA_ERR_BAD_ARG, "interleaved must be 0 (NeoX pairs) or 1 (GPT-J pairs)");
  if (inverse != 0 && inverse != 1) return set_err(FA_ERR_BAD_ARG, "inverse must be 0 or 1");
  if (rot < 2 || rot % 2 != 0 || rot > row_len) {
    snprintf(g_err, sizeof(g_err), "rot = %d must be even and in 2 .. %d (the rotated rows' length: min(d_new, d) with new tokens)", rot, row_len);
    return FA_ERR_BAD_ARG;
  }
  if (max_pos <= 0) return set_err(FA_ERR_BAD_ARG, "max_pos must be positive");
  return FA_OK;
}

// 16-byte lanes (E elements): the pairs' halves (NeoX) or the pairs (interleaved) fall on whole vectors, which also aligns the
// E (E / 2) table entries a lane reads; every row and every pointer on 16 bytes (align: an fp8 cache's rows on 8).
bool rope_vec(int E, int rot, int interleaved, int len_a, int len_b, uintptr_t ptrs, uintptr_t caches, uintptr_t cache_align) {
  if ((interleaved ? rot : rot / 2) % E != 0 || len_a % E != 0 || len_b % E != 0) return false;
  return (ptrs & 15) == 0 && (caches & (cache_align - 1)) == 0;
}

template <typename T, int E> int launch_rope(fa::RopeArgs a, bool il, hipStream_t st) {
  a.cpr = a.d / E;
  a.lanes *= a.cpr;   // (rows on entry)
  const dim3 grid((unsigned)((a.lanes + 255) / 256));
  if (il)
    hipLaunchKernelGGL((fa::rope_kernel<T, E, true>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((fa::rope_kernel<T, E, false>), grid, dim3(256), 0, st, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? FA_OK : set_err(FA_ERR_HIP, "rope_kernel launch", e);
}

template <typename T, int E, bool IL, bool FP8> void launch_rope_append_il(const fa::RopeAppendArgs& a, dim3 grid, hipStream_t st) {
  if constexpr (FP8) {
    if (a.table)
      hipLaunchKernelGGL((fa::rope_append_kernel<T, E, IL, true, false, true>), grid, dim3(256), 0, st, a);
    else
      hipLaunchKernelGGL((fa::rope_append_kernel<T, E, IL, false, false, true>), grid, dim3(256), 0, st, a);
  } else if (a.cu && a.table)
    hipLaunchKernelGGL((fa::rope_append_kernel<T, E, IL, true, true>), grid, dim3(256), 0, st, a);
  else if (a.cu)
    hipLaunchKernelGGL((fa::rope_append_kernel<T, E, IL, false, true>), grid, dim3(256), 0, st, a);
  else if (a.table)
    hipLaunchKernelGGL((fa::rope_append_kernel<T, E, IL, true>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((fa::rope_append_kernel<T, E, IL>), grid, dim3(256), 0, st, a);
}

template <typename T, int E, bool FP8 = false> int launch_rope_append(fa::RopeAppendArgs a, bool il, hipStream_t st) {
  a.ch_shift = __builtin_ctz(a.d / E);
  a.lanes <<= a.ch_shift;     // (rows on entry)
  a.q_lanes <<= a.ch_shift;
  const dim3 grid((unsigned)((a.q_lanes + a.lanes + 255) / 256));
  if (il)
    launch_rope_append_il<T, E, true, FP8>(a, grid, st);
  else
    launch_rope_append_il<T, E, false, FP8>(a, grid, st);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? FA_OK : set_err(FA_ERR_HIP, "rope_append_kernel launch", e);
}

// One roped append, uniform (cu null: Nq new tokens per batch element) or ragged (cu: Nq = T packed rows); q / q_rot or
// k_new / v_new may be absent (both null).  Every check comes first; then the one launch.
int rope_append_call(const void* q, void* q_rot, const void* k_new, const void* v_new, void* k_cache, void* v_cache, const Fp8* f8,
                     const float* cos, const float* sin, const int* cu, bool ragged, const int* cache_seqlens, const Paging* pg, int B, int H,
                     int Hkv, int Nq, int Ncap, int d_new, int d, int rot, int max_pos, int layout, int interleaved, int dtype,
                     void* stream) {
  g_err[0] = 0;
  int rc = f8 ? check_fp8(dtype) : FA_OK;
  if (rc != FA_OK) return rc;
  if ((q == nullptr) != (q_rot == nullptr)) return set_err(FA_ERR_BAD_ARG, "q and q_rot go together: give both, or neither (append only)");
  if ((k_new == nullptr) != (v_new == nullptr))
    return set_err(FA_ERR_BAD_ARG, "k_new and v_new go together: give both, or neither (rotate q only)");
  if (!q && !k_new) return set_err(FA_ERR_BAD_ARG, "nothing to do: q / q_rot and k_new / v_new are all null");
  if (pg) rc = check_pages(*pg, &Ncap);
  if (rc != FA_OK) return rc;
  if (k_new) {
    rc = ragged ? check_ragged_append(k_new, v_new, k_cache, v_cache, cu, B, Hkv, Nq, Ncap, d_new, d, layout, dtype)
                : check_append(k_new, v_new, k_cache, v_cache, B, Hkv, Nq, Ncap, d_new, d, layout, dtype, true);
    if (rc == FA_OK && pg) rc = check_page_bytes(pg->page_size, Hkv, d, dtype, f8 != nullptr);
    if (rc == FA_OK && f8 && !pg && ((long)Ncap + fa::DEC_ROWS) * Hkv * d >= (1L << 31))
      rc = set_err(FA_ERR_BAD_ARG, "one batch element of the cache must stay under 2 GiB");
    if (rc != FA_OK) return rc;
  } else {
    if (B <= 0 || Nq <= 0 || Ncap <= 0 || d <= 0) return set_err(FA_ERR_BAD_ARG, "B, Nq (T), Ncap and d must be positive");
    if (dtype != FA_DTYPE_F32 && dtype != FA_DTYPE_BF16) return set_err(FA_ERR_BAD_ARG, "unknown dtype");
    if (layout != FA_LAYOUT_BHND && layout != FA_LAYOUT_BNHD) return set_err(FA_ERR_BAD_ARG, "unknown layout");
    if (ragged && !cu) return set_err(FA_ERR_BAD_ARG, "null cu_seqlens_q");
    if (d != 32 && d != 64 && d != 128) return set_err(FA_ERR_UNSUPPORTED_D, "decode supports rows of d in {32, 64, 128}");
    d_new = d;
  }
  if (q) {
    if (H <= 0) return set_err(FA_ERR_BAD_ARG, "H must be positive");
    // (one lane per element at the most, the workgroup count of q's and the new rows' lanes together an unsigned int)
    if ((long)(ragged ? 1 : B) * Nq * H * d / 256 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "too many q elements for one rope_append launch");
  }
  rc = check_rope(cos, sin, rot, std::min(d_new, d), max_pos, interleaved, 0);
  if (rc != FA_OK) return rc;
  if (max_pos < Ncap) {
    snprintf(g_err, sizeof(g_err), "max_pos = %d table rows do not cover the cache's capacity of %d rows: every row needs an angle", max_pos, Ncap);
    return FA_ERR_BAD_ARG;
  }
  fa::RopeAppendArgs a;
  a.k_new = k_new;
  a.v_new = v_new;
  a.k = k_cache;
  a.v = v_cache;
  a.seqlens = cache_seqlens;
  const long seqs = ragged ? 1 : B;
  a.lanes = k_new ? seqs * Nq * Hkv : 0;
  a.q_lanes = q ? seqs * Nq * H : 0;
  a.Hkv = Hkv;
  a.Nq = Nq;
  a.Ncap = Ncap;
  a.d_new = d_new;
  a.bnhd = layout == FA_LAYOUT_BNHD;
  a.kv_ld = a.bnhd ? Hkv * d : d;
  a.kv_bstride = (long)Ncap * Hkv * d;
  a.kv_hstride = a.bnhd ? d : (long)Ncap * d;
  a.table = nullptr;
  a.page_size = a.num_pages = a.max_pages = 0;
  a.page_stride = 0;
  if (pg) {
    a.table = pg->table;
    a.page_size = pg->page_size;
    a.num_pages = pg->num_pages;
    a.max_pages = pg->max_pages;
    a.page_stride = (long)pg->page_size * Hkv * d;
    a.kv_bstride = 0;
    a.kv_hstride = a.bnhd ? d : (long)pg->page_size * d;
  }
  a.q = q;
  a.q_rot = q_rot;
  a.cos = cos;
  a.sin = sin;
  a.k_scale = f8 ? f8->k_scale : nullptr;
  a.v_scale = f8 ? f8->v_scale : nullptr;
  a.H = H;
  a.d = d;
  a.rot = rot;
  a.max_pos = max_pos;
  a.cu = ragged ? cu : nullptr;
  a.nseq = B;
  a.ntok = Nq;
  const int esz = dtype == FA_DTYPE_BF16 ? 2 : 4;
  const uintptr_t ptrs = (uintptr_t)q | (uintptr_t)q_rot | (uintptr_t)k_new | (uintptr_t)v_new | (uintptr_t)cos | (uintptr_t)sin;
  const uintptr_t caches = k_new ? (uintptr_t)k_cache | (uintptr_t)v_cache : 0;
  const bool vec = rope_vec(16 / esz, rot, interleaved, d_new, d, ptrs, caches, f8 ? 8 : 16);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool il = interleaved != 0;
  if (f8) return vec ? launch_rope_append<fa::bf16_t, 8, true>(a, il, st) : launch_rope_append<fa::bf16_t, 1, true>(a, il, st);
  if (dtype == FA_DTYPE_BF16) return vec ? launch_rope_append<fa::bf16_t, 8>(a, il, st) : launch_rope_append<fa::bf16_t, 1>(a, il, st);
  return vec ? launch_rope_append<float, 4>(a, il, st) : launch_rope_append<float, 1>(a, il, st);
}

}  // namespace

extern "C" {

int fa_mi355x_rope(const void* x, void* y, const float* cos, const float* sin, const int* pos_offsets, int B, int N, int H, int d, int rot,
                   int max_pos, int layout, int interleaved, int inverse, int dtype, void* stream) {
  g_err[0] = 0;
  if (B <= 0 || N <= 0 || H <= 0 || d <= 0) return set_err(FA_ERR_BAD_ARG, "B, N, H and d must be positive");
  if (dtype != FA_DTYPE_F32 && dtype != FA_DTYPE_BF16) return set_err(FA_ERR_BAD_ARG, "unknown dtype");
  if (layout != FA_LAYOUT_BHND && layout != FA_LAYOUT_BNHD) return set_err(FA_ERR_BAD_ARG, "unknown layout");
  if (!x || !y) return set_err(FA_ERR_BAD_ARG, "null pointer argument (x and y)");
  const int rc = check_rope(cos, sin, rot, d, max_pos, interleaved, inverse);
  if (rc != FA_OK) return rc;
  // (one lane per element at the most, 256 lanes to a workgroup, the workgroup count an int)
  if ((long)B * N * H * d / 256 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "too many elements for one rope launch");
  fa::RopeArgs a;
  a.x = x;
  a.y = y;
  a.cos = cos;
  a.sin = sin;
  a.offsets = pos_offsets;
  a.lanes = (long)B * N * H;
  a.N = N;
  a.H = H;
  a.d = d;
  a.rot = rot;
  a.max_pos = max_pos;
  a.bnhd = layout == FA_LAYOUT_BNHD;
  a.inverse = inverse;
  const int esz = dtype == FA_DTYPE_BF16 ? 2 : 4;
  const bool vec = rope_vec(16 / esz, rot, interleaved, d, d, (uintptr_t)x | (uintptr_t)y | (uintptr_t)cos | (uintptr_t)sin, 0, 16);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool il = interleaved != 0;
  if (dtype == FA_DTYPE_BF16) return vec ? launch_rope<fa::bf16_t, 8>(a, il, st) : launch_rope<fa::bf16_t, 1>(a, il, st);
  return vec ? launch_rope<float, 4>(a, il, st) : launch_rope<float, 1>(a, il, st);
}

int fa_mi355x_rope_append(const void* q, void* q_rot, const void* k_new, const void* v_new, void* k_cache, void* v_cache, const float* k_scale,
                          const float* v_scale, const float* cos, const float* sin, const int* cache_seqlens, const int* block_table, int B,
                          int H, int Hkv, int Nq, int Ncap, int num_pages, int page_size, int max_pages, int d_new, int d, int rot,
                          int max_pos, int layout, int interleaved, int cache_fp8, int dtype, void* stream) {
  if (cache_fp8 != 0 && cache_fp8 != 1) {
    g_err[0] = 0;
    return set_err(FA_ERR_BAD_ARG, "cache_fp8 must be 0 or 1");
  }
  const Paging pg = {block_table, num_pages, page_size, max_pages};
  const Fp8 f8 = {k_scale, v_scale};
  return rope_append_call(q, q_rot, k_new, v_new, k_cache, v_cache, cache_fp8 ? &f8 : nullptr, cos, sin, nullptr, false, cache_seqlens,
                          block_table ? &pg : nullptr, B, H, Hkv, Nq, Ncap, d_new, d, rot, max_pos, layout, interleaved, dtype, stream);
}

int fa_mi355x_rope_append_ragged(const void* q, void* q_rot, const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                                 const float* cos, const float* sin, const int* cu_seqlens_q, const int* cache_seqlens,
                                 const int* block_table, int B, int H, int Hkv, int T, int Ncap, int num_pages, int page_size, int max_pages,
                                 int d_new, int d, int rot, int max_pos, int layout, int interleaved, int dtype, void* stream) {
  const Paging pg = {block_table, num_pages, page_size, max_pages};
  return rope_append_call(q, q_rot, k_new, v_new, k_cache, v_cache, nullptr, cos, sin, cu_seqlens_q, true, cache_seqlens,
                          block_table ? &pg : nullptr, B, H, Hkv, T, Ncap, d_new, d, rot, max_pos, layout, interleaved, dtype, stream);
}

// The ungrouped entry points: Hkv = H.
size_t fa_mi355x_decode_workspace_bytes(int B, int H, int Nq, int Ncap, int d) {
  return fa_mi355x_decode_workspace_bytes_gqa(B, H, H, Nq, Ncap, d);
}

int fa_mi355x_decode_splits(int B, int H, int Nq, int Ncap, int d, int dtype) {
  return fa_mi355x_decode_splits_gqa(B, H, H, Nq, Ncap, d, dtype);
}

int fa_mi355x_fwd_decode(const void* q, const void* k_cache, const void* v_cache, float* out, float* lse, const int* cache_seqlens,
                         void* workspace, int B, int H, int Nq, int Ncap, int d, int layout, float softmax_scale, int causal,
                         int dtype, void* stream) {
  return fa_mi355x_fwd_decode_gqa(q, k_cache, v_cache, out, lse, cache_seqlens, workspace, B, H, H, Nq, Ncap, d, layout, softmax_scale,
                                  causal, dtype, stream);
}

const char* fa_mi355x_decode_last_error(void) { return g_err; }

}  // extern "C"
