// C ABI of the MI355X KV-cache decode library (declared in include/flash_attn_mi355x_decode.h and its _paged.h, _ragged.h,
// _window.h, _sink.h, _fp8.h, _softcap.h, _lsink.h and _rope.h).  Every entry point fills one KvCall (the call as it was received) and hands it to run():
// the entry point's prelude (check_fp8 or check_window), the page geometry (check_pages), the attention's checks (check_attend, which
// also returns the call's Policy), the append's (check_append), then the append launch (run_append) and the attention's launches
// (run_attend -> launch_split).  policy() is the one split policy: the three families (decode: 32-row blocks, at most 128 queries;
// extend: 128-row blocks, any number; ragged: the extend policy on an upper bound of the row blocks) differ by the data of FAMILIES.
// A paged call (a pool and a block table) takes the contiguous call's policy at Ncap = max_pages * page_size.  A windowed call takes
// the policy on its window span (span_keys) instead of Ncap, a sink call on that span plus its sink tiles.  An fp8 call (caches of
// e4m3 bytes, per-kv-head scales) takes the bf16 call's policy and workspace for the same arguments; its cache bounds count one byte
// per element.  A soft-capped call (softcap > 0) takes the policy and workspace of the same call without the cap, the softcap builds
// of the split kernels and the existing combine kernels with tau = 1.  A call with learned sink logits (sink_logits not null) takes
// the policy and workspace of the same call without them, the lsink builds of the split kernels and of the combine kernel.  The rotary calls launch the kernels of fa_rope.h in front of the attend-only entry points.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <stdio.h>
#include <type_traits>

#include "../../include/flash_attn_mi355x_decode.h"
#include "fa_decode.h"
#include "fa_rope.h"

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

// What the three call families do differently, as data: the split policy's two figures, and the messages that name a family's
// arguments or its size query (null: the family has no such check).
enum Family { DECODE, EXTEND, RAGGED };

struct FamilyRule {
  int block_rows, waves;   // rows of a workgroup's row block; workgroups per CU the split aims at
  const char *sizes, *append_sizes, *rows, *q_bytes, *grid, *workspace, *split_launch, *combine_launch;
};

// Extend: a workgroup of extend_split_kernel owns 128 rows, and TWO workgroups per CU are the target: a workgroup there lives for a
// long key loop, so a second round of workgroups buys nothing, while every split costs a partial per row and the combine launch
// over B*H*Nq rows (measured: profiles/extend_bench.txt).
constexpr FamilyRule FAMILIES[3] = {
    {32, 4, "B, H, Nq, Ncap and d must be positive", "B, Hkv, Nq, Ncap and d must be positive", nullptr,
     "one batch element of q must stay under 2 GiB", nullptr, "null workspace: this call needs fa_mi355x_decode_workspace_bytes() bytes",
     "decode_split_kernel launch", "decode_combine_kernel launch"},
    {fa::EXT_BLOCK, 2, "B, H, Nq, Ncap and d must be positive", "B, Hkv, Nq, Ncap and d must be positive",
     "G * Nq rows per kv head must stay under 2^25", "one batch element of q must stay under 2 GiB",
     "too many workgroups for one launch: B * Hkv * splits * row blocks and B * H * Nq must fit an unsigned int",
     "null workspace: this call needs fa_mi355x_extend_workspace_bytes() bytes", "extend_split_kernel launch",
     "decode_combine_kernel launch"},
    {fa::EXT_BLOCK, 2, "B, H, T, Ncap and d must be positive", "B, Hkv, T, Ncap and d must be positive",
     "G * T rows per kv head must stay under 2^25", "q (T * H * d elements) must stay under 2 GiB",
     "too many workgroups for one launch: Hkv * splits * row blocks and H * T must fit an unsigned int",
     "null workspace: a ragged call always needs fa_mi355x_ragged_workspace_bytes() bytes (the block map)",
     "extend_split_kernel (ragged) launch", "decode_combine_kernel (ragged) launch"},
};

// A paged call's block table and pool geometry (all zero in the contiguous call).
struct Paging {
  const int* table;
  int num_pages, page_size, max_pages;
};

// An fp8 call's scales (either may be null: all ones); on false: a bf16 or fp32 cache.
struct Fp8 {
  bool on;
  const float* k_scale;
  const float* v_scale;
};

// One KV-cache call as its entry point received it.  The setters group the arguments the prototypes group; what an entry point does
// not set keeps the value here.  Nq is T, the packed rows, in the ragged family; Ncap is overwritten by the pool's capacity in a
// paged call.
struct KvCall {
  Family family;
  bool attend = false, append = false;   // what to do: the attention, the append, or the append then the attention
  const void *q = nullptr, *k_new = nullptr, *v_new = nullptr;
  void *k_cache = nullptr, *v_cache = nullptr;
  float *out = nullptr, *lse = nullptr;
  const int *cu = nullptr, *seqlens = nullptr;
  void* workspace = nullptr;
  // a pool and a block table (pg) in the place of slabs of Ncap rows.  (A flag beside pg.table: the _paged entry points answer a null
  // table with an error, the later forms take it for slabs.)
  bool paged = false;
  Paging pg = {nullptr, 0, 0, 0};
  Fp8 f8 = {false, nullptr, nullptr};
  int B = 0, H = 0, Hkv = 0, Nq = 0, Ncap = 0, d_new = 0, d = 0;
  int layout = 0, causal = 0, window = 0, sink = 0, dtype = 0;
  float softmax_scale = 0.f;
  float softcap = 0.f;   // logit soft-capping (_softcap.h); 0: none
  const float* sink_logits = nullptr;   // learned sink logits (_lsink.h), fp32 [H] on the device; null: none
  hipStream_t stream = nullptr;

  explicit KvCall(Family f) : family(f) {}
  KvCall& attention(const void* q_, float* out_, float* lse_, void* workspace_, float softmax_scale_, int causal_) {
    attend = true;
    q = q_, out = out_, lse = lse_, workspace = workspace_, softmax_scale = softmax_scale_, causal = causal_;
    return *this;
  }
  KvCall& new_tokens(const void* k_new_, const void* v_new_, int d_new_) {
    append = true;
    k_new = k_new_, v_new = v_new_, d_new = d_new_;
    return *this;
  }
  // (the attend-only prototypes take the caches const: only an append writes them)
  KvCall& cache(const void* k_, const void* v_, const int* seqlens_, int Ncap_) {
    k_cache = const_cast<void*>(k_), v_cache = const_cast<void*>(v_), seqlens = seqlens_, Ncap = Ncap_;
    return *this;
  }
  KvCall& pool(const int* table, int num_pages, int page_size, int max_pages) {
    paged = true;
    pg = {table, num_pages, page_size, max_pages};
    return *this;
  }
  // (the forms that take both kinds of cache: a null block_table means slabs of Ncap rows)
  KvCall& pool_or_slabs(const int* table, int num_pages, int page_size, int max_pages) {
    return table ? pool(table, num_pages, page_size, max_pages) : *this;
  }
  KvCall& heads(int B_, int H_, int Hkv_, int Nq_, int d_) {
    B = B_, H = H_, Hkv = Hkv_, Nq = Nq_, d = d_;
    return *this;
  }
  KvCall& format(int layout_, int dtype_, void* stream_) {
    layout = layout_, dtype = dtype_, stream = static_cast<hipStream_t>(stream_);
    return *this;
  }
  bool bnhd() const { return layout == FA_LAYOUT_BNHD; }
  long seqs() const { return family == RAGGED ? 1 : B; }   // batch elements that own Nq rows each: the ragged ones share T
  long esz() const { return dtype == FA_DTYPE_BF16 ? 2 : 4; }
};

// Sliding window (include/flash_attn_mi355x_decode_window.h).  A window of W >= Ncap keys admits every key of every row (a row's
// position is at most len - 1 <= Ncap - 1): such a call IS the unwindowed call, the same launches and the same bits, and so is
// W = 0.  This also bounds what the device computes with: W < Ncap.
// Sinks (include/flash_attn_mi355x_decode_sink.h): S >= Ncap first positions admit every key of every row as well, and S = 0 is
// the windowed call; sinks without a window mean nothing.  The device computes with 1 <= W < Ncap and 0 <= S < Ncap.
int win_of(int window, int sink, int Ncap) { return window >= Ncap || sink >= Ncap ? 0 : window; }
int sink_of(int window, int sink, int Ncap) { return win_of(window, sink, Ncap) == 0 ? 0 : sink; }

// The window SPAN: the keys one row block can need, which is what the policy splits where it splits Ncap.  A block's rows
// sit at positions p_first .. p_last with p_last - p_first <= min(Nq, block_rows) - 1 (row i * G + g: block_rows rows span at most
// block_rows positions, and no more than the call has).  Its key range starts at lo = (p_first - W + 1, clamped to 0) rounded DOWN
// to a super tile, at most 127 keys below the edge, and ends at p_last:
//   p_last - lo + 1 <= (p_last - p_first) + W + 127 <= W + min(Nq, block_rows) - 1 + 127
// and never more than the cache holds.  nsplit * chunk >= span, so the splits of every block cover [lo, p_last].
// With S sinks a block walks, in front of that range, the super tiles that hold a sink key and lie wholly below lo: at most
// ceil(S / 128) of them, which the span counts in full.
int span_keys(int window, int sink, int Ncap, int Nq, int block_rows) {
  const int W = win_of(window, sink, Ncap);
  if (W == 0) return Ncap;
  const long sink_keys = ((long)sink + fa::DEC_ROWS - 1) / fa::DEC_ROWS * fa::DEC_ROWS;
  return (int)std::min((long)Ncap, sink_keys + W + std::min(Nq, block_rows) - 1 + fa::DEC_ROWS - 1);
}

// workgroups of the split launch: the items rounded up to 8, times the row blocks (the kernels' workgroup -> (item, row block) map)
long split_grid(long items, long nqb) { return (items + 7) / 8 * 8 * nqb; }

// Split policy (DESIGN.md "Decode"): enough (batch*kv head, chunk, row block) workgroups to cover a 256-CU chip `waves` times, chunks
// a multiple of 256 keys (two super tiles) and at least 256 keys.  A kv head has G*Nq rows (G = H / Hkv query heads per kv head),
// block_rows to a block.  Launches that already have that many workgroups without splitting run as one split.  The chip size is
// assumed, not queried, so the split count is a function of the arguments alone.
// Ragged: the policy on what the ARGUMENTS say about the row blocks, never the device arrays: a sequence's G * nq_b rows round up to
// 128 at most once, so B sequences that share T packed rows have at most floor(G * T / 128) + min(B, T) row blocks.  That bound
// sizes the block map and the grid and stands for the row blocks in the policy, so the split count, the workspace and a captured
// graph do not depend on cu_seqlens_q.  (It under-splits a step whose tokens all sit in one of many sequences.)  Its figures are per
// call, not per batch element.
constexpr int DEC_CUS = 256, DEC_MIN_CHUNK = 256;

struct Policy {
  int span;      // the keys that are split: Ncap, or the window span
  long nqb;      // row blocks per kv head (ragged: entries of the block map)
  int chunk, nsplit;
  long items;    // (batch element, kv head, split) triples; ragged: (kv head, split) pairs
  // the workspace: (ragged) the block map, (sequence, block) int pairs rounded up to 16 bytes, then the partials of all rows and
  // splits; a decode or extend call of one split needs none
  size_t map_bytes, workspace_bytes;
};

Policy policy(Family f, int B, int H, int Hkv, int Nq, int Ncap, int d, int window, int sink) {
  const FamilyRule& r = FAMILIES[f];
  const long G = H / Hkv, seqs = f == RAGGED ? 1 : B;
  Policy p;
  p.span = span_keys(window, sink, Ncap, Nq, r.block_rows);
  p.nqb = f == RAGGED ? G * Nq / r.block_rows + std::min(B, Nq) : (G * Nq + r.block_rows - 1) / r.block_rows;
  const long groups = seqs * Hkv * p.nqb;
  const long want = std::max(1L, (DEC_CUS * r.waves + groups - 1) / groups);
  const long per = (p.span + want - 1) / want;
  p.chunk = (int)std::max((long)DEC_MIN_CHUNK, (per + DEC_MIN_CHUNK - 1) / DEC_MIN_CHUNK * DEC_MIN_CHUNK);
  p.nsplit = (int)(((long)p.span + p.chunk - 1) / p.chunk);
  p.items = seqs * Hkv * p.nsplit;
  p.map_bytes = f == RAGGED ? ((size_t)p.nqb * 2 * sizeof(int) + 15) / 16 * 16 : 0;
  const size_t partials = (size_t)seqs * H * p.nsplit * Nq * (size_t)(d + 2) * sizeof(float);
  p.workspace_bytes = f == RAGGED ? p.map_bytes + partials : p.nsplit == 1 ? 0 : partials;
  return p;
}

Policy policy(const KvCall& c) { return policy(c.family, c.B, c.H, c.Hkv, c.Nq, c.Ncap, c.d, c.window, c.sink); }

// The size queries: all zero unless the sizes are positive, H is a multiple of Hkv and window and sink are not negative (what the
// policy needs to answer at all).
Policy query(Family f, int B, int H, int Hkv, int Nq, int Ncap, int d, int window, int sink) {
  const bool ok = B > 0 && H > 0 && Hkv > 0 && Nq > 0 && Ncap > 0 && d > 0 && H % Hkv == 0 && window >= 0 && sink >= 0;
  return ok ? policy(f, B, H, Hkv, Nq, Ncap, d, window, sink) : Policy{};
}

// ---- the checks ----
// The check an fp8 call makes first: the queries and the new tokens are bf16.
int check_fp8(int dtype) {
  g_err[0] = 0;
  if (dtype == FA_DTYPE_F32)
    return set_err(FA_ERR_BAD_ARG, "an fp8 cache takes bf16 queries and new tokens: FA_DTYPE_F32 is not supported (dtype must be FA_DTYPE_BF16)");
  if (dtype != FA_DTYPE_BF16) return set_err(FA_ERR_BAD_ARG, "unknown dtype");
  return FA_OK;
}

// The checks a windowed call makes first (sink and softcap: 0 in the calls that have none; a call without a window passes).  A cap
// does not need the causal mask; a window still does.
int check_window(int window, int causal, int sink, float softcap) {
  g_err[0] = 0;
  if (!(softcap >= 0.f) || !std::isfinite(softcap))
    return set_err(FA_ERR_BAD_ARG, "softcap must be finite and not negative (0: no soft-capping)");
  if (sink < 0) return set_err(FA_ERR_BAD_ARG, "sink must not be negative (0: no sink tokens)");
  if (window < 0) return set_err(FA_ERR_BAD_ARG, "window must not be negative (0: no window)");
  if (window > 0 && !causal)
    return set_err(FA_ERR_BAD_ARG, "a sliding window needs the causal mask: window > 0 with causal = 0 (the window ends at the query's position)");
  return FA_OK;
}

// The checks a paged call makes next: FA_OK with the logical capacity max_pages * page_size in *Ncap, or the error.
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

// A buffer load's row offset is a 32-bit byte count: one batch element of a slab, plus a super tile of rows past its end, stays
// under 2 GiB; in a pool the bound is on one page (page base addresses are 64-bit, so the pool may be any size).  An fp8 cache
// holds one byte per element whatever dtype, the queries' type, says.
int check_cache_bytes(const KvCall& c) {
  const long esz = c.f8.on ? 1 : c.esz();
  if (c.paged) {
    if ((long)c.pg.page_size * c.Hkv * c.d * esz >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "one page of the pool must stay under 2 GiB");
  } else if (((long)c.Ncap + fa::DEC_ROWS) * c.Hkv * c.d * esz >= (1L << 31)) {
    return set_err(FA_ERR_BAD_ARG, "one batch element of the cache must stay under 2 GiB");
  }
  return FA_OK;
}

// The argument checks of the attention: FA_OK with the call's policy in *out, or the error with its message set.  The families
// differ in the Nq <= 128 of decode, the null cu_seqlens_q of ragged, the names in the messages and the bounds of FAMILIES.
int check_attend(const KvCall& c, Policy* out) {
  const FamilyRule& r = FAMILIES[c.family];
  g_err[0] = 0;
  if (c.B <= 0 || c.H <= 0 || c.Nq <= 0 || c.Ncap <= 0 || c.d <= 0) return set_err(FA_ERR_BAD_ARG, r.sizes);
  if (c.Hkv <= 0) return set_err(FA_ERR_BAD_ARG, "Hkv must be positive");
  if (c.H % c.Hkv != 0) {
    snprintf(g_err, sizeof(g_err), "H = %d query heads must be a multiple of Hkv = %d cache heads", c.H, c.Hkv);
    return FA_ERR_BAD_ARG;
  }
  if (c.family == DECODE && c.Nq > FA_DECODE_MAX_NQ)
    return set_err(FA_ERR_BAD_ARG, "Nq > 128 is prefill: use fa_mi355x_fwd_layout or fa_mi355x_fwd_scaled (the forward entry points)");
  if (c.dtype != FA_DTYPE_F32 && c.dtype != FA_DTYPE_BF16) return set_err(FA_ERR_BAD_ARG, "unknown dtype");
  if (c.layout != FA_LAYOUT_BHND && c.layout != FA_LAYOUT_BNHD) return set_err(FA_ERR_BAD_ARG, "unknown layout");
  if (!c.q || !c.k_cache || !c.v_cache || !c.out) return set_err(FA_ERR_BAD_ARG, "null pointer argument");
  if (c.family == RAGGED && !c.cu) return set_err(FA_ERR_BAD_ARG, "null cu_seqlens_q");
  if (c.d != 32 && c.d != 64 && c.d != 128)
    return set_err(FA_ERR_UNSUPPORTED_D, "decode supports d in {32, 64, 128}: pad the cache with zero columns for other d <= 128");
  if (c.softmax_scale != 0.f && (!(c.softmax_scale > 0.f) || !std::isfinite(c.softmax_scale)))
    return set_err(FA_ERR_BAD_ARG, "softmax_scale must be positive and finite (0: 1/sqrt(d))");
  // (row_query is exact for rows below 2^25; a ragged sequence has at most G * T of them)
  if (r.rows && (long)(c.H / c.Hkv) * c.Nq >= (1L << 25)) return set_err(FA_ERR_BAD_ARG, r.rows);
  if (check_cache_bytes(c) != FA_OK) return FA_ERR_BAD_ARG;
  // (q's (head, query) offset within its batch element is a 32-bit byte count as well; a ragged sequence may own every packed row)
  if ((long)c.Nq * c.H * c.d * c.esz() >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, r.q_bytes);
  const Policy p = policy(c);
  // (the workgroup counts of the split and the combine launch are unsigned ints, the items an int)
  if (r.grid && (split_grid(p.items, p.nqb) >= (1L << 32) || p.items >= (1L << 31) || c.seqs() * c.H * c.Nq >= (1L << 32)))
    return set_err(FA_ERR_BAD_ARG, r.grid);
  // (the ragged block map lives in the workspace: every ragged call needs one)
  if ((p.nsplit > 1 || c.family == RAGGED) && !c.workspace) return set_err(FA_ERR_BAD_ARG, r.workspace);
  *out = p;
  return FA_OK;
}

// The argument checks of the append: FA_OK, or the error with its message set.  Ragged: T packed rows in the place of B * Nq, and
// a null cu_seqlens_q.  An append without the attention also makes the attention's check of the cache's size.
int check_append(const KvCall& c) {
  g_err[0] = 0;
  if (c.B <= 0 || c.Hkv <= 0 || c.Nq <= 0 || c.Ncap <= 0 || c.d <= 0) return set_err(FA_ERR_BAD_ARG, FAMILIES[c.family].append_sizes);
  if (c.family == DECODE && c.Nq > FA_DECODE_MAX_NQ)
    return set_err(FA_ERR_BAD_ARG, "Nq > 128 new tokens per call: fill the cache of a prompt directly");
  if (c.dtype != FA_DTYPE_F32 && c.dtype != FA_DTYPE_BF16) return set_err(FA_ERR_BAD_ARG, "unknown dtype");
  if (c.layout != FA_LAYOUT_BHND && c.layout != FA_LAYOUT_BNHD) return set_err(FA_ERR_BAD_ARG, "unknown layout");
  if (!c.k_new || !c.v_new || !c.k_cache || !c.v_cache)
    return set_err(FA_ERR_BAD_ARG, "null pointer argument (k_new, v_new and the caches)");
  if (c.family == RAGGED && !c.cu) return set_err(FA_ERR_BAD_ARG, "null cu_seqlens_q");
  if (c.d != 32 && c.d != 64 && c.d != 128) return set_err(FA_ERR_UNSUPPORTED_D, "decode supports cache rows of d in {32, 64, 128}");
  if (c.d_new < 1 || c.d_new > c.d) {
    snprintf(g_err, sizeof(g_err), "d_new = %d must be in 1 .. d = %d", c.d_new, c.d);
    return FA_ERR_BAD_ARG;
  }
  // (one lane per element at the most, 256 lanes to a workgroup, the workgroup count an int; the ragged kernel counts packed rows in
  // an int)
  if (c.seqs() * c.Nq * c.Hkv * c.d / 256 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "too many new elements for one append launch");
  // (a store's row offset is added to a 64-bit address: the bound is the attention's, whose loads read these rows.  A page of any
  // pool, and the slabs an fp8 append fills; a fused call's attention has checked it already)
  if (!c.attend && (c.paged || c.f8.on)) return check_cache_bytes(c);
  return FA_OK;
}

// ---- the kernel arguments ----
// The one place that writes cache geometry, into a DecodeArgs, RaggedArgs, AppendArgs or RopeAppendArgs: slabs of Ncap rows per batch
// element, or (a block table) pool pages of [page_size][Hkv][d] or [Hkv][page_size][d] rows.
template <typename A> void set_cache_geometry(A& a, const KvCall& c) {
  const long rows = c.paged ? c.pg.page_size : c.Ncap;   // rows of one slab or page
  a.kv_ld = c.bnhd() ? c.Hkv * c.d : c.d;
  a.kv_hstride = c.bnhd() ? c.d : rows * c.d;
  a.kv_bstride = c.paged ? 0 : (long)c.Ncap * c.Hkv * c.d;
  a.table = c.pg.table;
  a.page_size = c.pg.page_size;
  a.num_pages = c.pg.num_pages;
  a.max_pages = c.pg.max_pages;
  a.page_stride = (long)c.pg.page_size * c.Hkv * c.d;
}

// The AppendArgs part of every append's argument (lanes: rows on entry, which the launchers turn into lanes).
void set_append(fa::AppendArgs& a, const KvCall& c) {
  a.k_new = c.k_new;
  a.v_new = c.v_new;
  a.k = c.k_cache;
  a.v = c.v_cache;
  a.seqlens = c.seqlens;
  a.lanes = c.k_new ? c.seqs() * c.Nq * c.Hkv : 0;
  a.Hkv = c.Hkv;
  a.Nq = c.Nq;
  a.Ncap = c.Ncap;
  a.d_new = c.d_new;
  a.bnhd = c.bnhd();
  set_cache_geometry(a, c);
}

// The host's view of a split launch: every build's argument is a part of it (DecodeArgs, RaggedArgs) or a copy of such a part with
// the scales or the sink count behind it (Fp8Args, SinkArgs, RaggedSinkArgs), which the leg that launches such a build makes.
struct SplitArgs : fa::RaggedArgs {
  Fp8 f8;
  int sink;        // S >= 1: a sink reaches the device
  float softcap;   // > 0: the softcap builds (SoftcapArgs, RaggedSoftcapArgs), and tau = 1 for the combine kernel
  const float* sink_logits;   // not null: the lsink builds (LsinkArgs, RaggedLsinkArgs) and the lsink build of the combine kernel
};

template <typename S, typename Base> S with_lsink(const SplitArgs& a) {
  S s;
  static_cast<Base&>(s) = a;
  s.sink_logits = a.sink_logits;
  return s;
}

template <typename S, typename Base> S with_softcap(const SplitArgs& a) {
  S s;
  static_cast<Base&>(s) = a;
  s.softcap = a.softcap;
  return s;
}

template <typename S, typename Base> S with_sink(const SplitArgs& a) {
  S s;
  static_cast<Base&>(s) = a;
  s.sink = a.sink;
  return s;
}

fa::Fp8Args with_scales(const SplitArgs& a) {
  fa::Fp8Args f;
  static_cast<fa::DecodeArgs&>(f) = a;
  f.k_scale = a.f8.k_scale;
  f.v_scale = a.f8.v_scale;
  return f;
}

// ---- the launches ----
template <typename A, typename B> void launch256(void (*kernel)(A), long grid, hipStream_t st, const B& a) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(256), 0, st, static_cast<const A&>(a));
}

// The launches of a checked attention: (ragged) the schedule, the split build of the table below, and the combine if nsplit > 1.
// Which instance serves which call:
//   decode  the ungrouped build for exactly the slab, unwindowed, non-fp8, G == 1 call; the grouped build for every other (one paged
//           build: G = 1 computes the same rows, and a paged workgroup looks up its page anyway; the windowed, sink and fp8 builds
//           likewise)
//   extend, ragged  PAGED x WINDOW as the call has them; ragged is the RAGGED flag of the extend kernels
//   sink    kernels and an argument of their own, only when a sink reaches the device (a.sink >= 1, which implies a.window >= 1)
//   fp8     bf16 queries, slab or paged, no window (the Python layer refuses the combination by name)
//   softcap kernels and an argument of their own, only when a cap reaches the device (a.softcap > 0): PAGED x WINDOW as the call has
//           them, the grouped build in the decode family; the combine launch is the existing instance with tau = 1
//   lsink   kernels and an argument of their own, only when the logits reach the device (a.sink_logits not null): the softcap
//           legs' choice of builds, and the lsink build of the combine kernel; as many launches as the call without the logits
template <typename T, int D> int launch_split(const SplitArgs& a, Family f, hipStream_t st) {
  constexpr bool BF16 = std::is_same<T, fa::bf16_t>::value;
  const bool paged = a.table != nullptr, window = a.window != 0;
  const long grid = split_grid(a.items, a.nqb);
  if (f == RAGGED) {
    hipLaunchKernelGGL(fa::ragged_schedule_kernel, dim3(1), dim3(256), 0, st, a.cu, const_cast<int*>(a.map), a.nseq, a.ntok, a.G, a.nqb);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_err("ragged_schedule_kernel launch", e);
  }
  const char* what = FAMILIES[f].split_launch;
  if (a.f8.on) {
    what = f == EXTEND ? "extend_split_kernel (fp8) launch" : "decode_split_kernel (fp8) launch";
    if constexpr (BF16) {   // (check_fp8: never fp32 queries)
      const fa::Fp8Args fa8 = with_scales(a);
      if (f == EXTEND && paged) launch256(fa::extend_split_kernel<T, D, true, false, false, true>, grid, st, fa8);
      else if (f == EXTEND) launch256(fa::extend_split_kernel<T, D, false, false, false, true>, grid, st, fa8);
      else if (paged) launch256(fa::decode_split_kernel<T, D, true, true, false, true>, grid, st, fa8);
      else launch256(fa::decode_split_kernel<T, D, true, false, false, true>, grid, st, fa8);
    }
  } else if (a.softcap > 0.f) {   // (no sinks and no fp8 cache beside a cap: the softcap entry points have neither argument)
    if (f == RAGGED) {
      what = "extend_split_softcap_kernel (ragged) launch";
      const fa::RaggedSoftcapArgs ca = with_softcap<fa::RaggedSoftcapArgs, fa::RaggedArgs>(a);
      if (window && paged) launch256(fa::extend_split_softcap_kernel<T, D, true, true, true>, grid, st, ca);
      else if (window) launch256(fa::extend_split_softcap_kernel<T, D, false, true, true>, grid, st, ca);
      else if (paged) launch256(fa::extend_split_softcap_kernel<T, D, true, true, false>, grid, st, ca);
      else launch256(fa::extend_split_softcap_kernel<T, D, false, true, false>, grid, st, ca);
    } else {
      what = f == EXTEND ? "extend_split_softcap_kernel launch" : "decode_split_softcap_kernel launch";
      const fa::SoftcapArgs ca = with_softcap<fa::SoftcapArgs, fa::DecodeArgs>(a);
      if (f == EXTEND && window && paged) launch256(fa::extend_split_softcap_kernel<T, D, true, false, true>, grid, st, ca);
      else if (f == EXTEND && window) launch256(fa::extend_split_softcap_kernel<T, D, false, false, true>, grid, st, ca);
      else if (f == EXTEND && paged) launch256(fa::extend_split_softcap_kernel<T, D, true, false, false>, grid, st, ca);
      else if (f == EXTEND) launch256(fa::extend_split_softcap_kernel<T, D, false, false, false>, grid, st, ca);
      else if (window && paged) launch256(fa::decode_split_softcap_kernel<T, D, true, true>, grid, st, ca);
      else if (window) launch256(fa::decode_split_softcap_kernel<T, D, false, true>, grid, st, ca);
      else if (paged) launch256(fa::decode_split_softcap_kernel<T, D, true, false>, grid, st, ca);
      else launch256(fa::decode_split_softcap_kernel<T, D, false, false>, grid, st, ca);
    }
  } else if (a.sink_logits) {   // (no sink tokens, no cap and no fp8 cache beside the logits: the lsink entry points have none of them)
    if (f == RAGGED) {
      what = "extend_split_lsink_kernel (ragged) launch";
      const fa::RaggedLsinkArgs la = with_lsink<fa::RaggedLsinkArgs, fa::RaggedArgs>(a);
      if (window && paged) launch256(fa::extend_split_lsink_kernel<T, D, true, true, true>, grid, st, la);
      else if (window) launch256(fa::extend_split_lsink_kernel<T, D, false, true, true>, grid, st, la);
      else if (paged) launch256(fa::extend_split_lsink_kernel<T, D, true, true, false>, grid, st, la);
      else launch256(fa::extend_split_lsink_kernel<T, D, false, true, false>, grid, st, la);
    } else {
      what = f == EXTEND ? "extend_split_lsink_kernel launch" : "decode_split_lsink_kernel launch";
      const fa::LsinkArgs la = with_lsink<fa::LsinkArgs, fa::DecodeArgs>(a);
      if (f == EXTEND && window && paged) launch256(fa::extend_split_lsink_kernel<T, D, true, false, true>, grid, st, la);
      else if (f == EXTEND && window) launch256(fa::extend_split_lsink_kernel<T, D, false, false, true>, grid, st, la);
      else if (f == EXTEND && paged) launch256(fa::extend_split_lsink_kernel<T, D, true, false, false>, grid, st, la);
      else if (f == EXTEND) launch256(fa::extend_split_lsink_kernel<T, D, false, false, false>, grid, st, la);
      else if (window && paged) launch256(fa::decode_split_lsink_kernel<T, D, true, true>, grid, st, la);
      else if (window) launch256(fa::decode_split_lsink_kernel<T, D, false, true>, grid, st, la);
      else if (paged) launch256(fa::decode_split_lsink_kernel<T, D, true, false>, grid, st, la);
      else launch256(fa::decode_split_lsink_kernel<T, D, false, false>, grid, st, la);
    }
  } else if (f == DECODE) {
    if (a.sink) {
      const fa::SinkArgs sa = with_sink<fa::SinkArgs, fa::DecodeArgs>(a);
      if (paged) launch256(fa::decode_split_sink_kernel<T, D, true>, grid, st, sa);
      else launch256(fa::decode_split_sink_kernel<T, D, false>, grid, st, sa);
    } else if (window && paged) launch256(fa::decode_split_kernel<T, D, true, true, true>, grid, st, a);
    else if (window) launch256(fa::decode_split_kernel<T, D, true, false, true>, grid, st, a);
    else if (paged) launch256(fa::decode_split_kernel<T, D, true, true>, grid, st, a);
    else if (a.G > 1) launch256(fa::decode_split_kernel<T, D, true>, grid, st, a);
    else launch256(fa::decode_split_kernel<T, D, false>, grid, st, a);
  } else if (f == EXTEND) {
    if (a.sink) {
      const fa::SinkArgs sa = with_sink<fa::SinkArgs, fa::DecodeArgs>(a);
      if (paged) launch256(fa::extend_split_sink_kernel<T, D, true, false>, grid, st, sa);
      else launch256(fa::extend_split_sink_kernel<T, D, false, false>, grid, st, sa);
    } else if (window && paged) launch256(fa::extend_split_kernel<T, D, true, false, true>, grid, st, a);
    else if (window) launch256(fa::extend_split_kernel<T, D, false, false, true>, grid, st, a);
    else if (paged) launch256(fa::extend_split_kernel<T, D, true>, grid, st, a);
    else launch256(fa::extend_split_kernel<T, D>, grid, st, a);
  } else {
    if (a.sink) {
      const fa::RaggedSinkArgs sa = with_sink<fa::RaggedSinkArgs, fa::RaggedArgs>(a);
      if (paged) launch256(fa::extend_split_sink_kernel<T, D, true, true>, grid, st, sa);
      else launch256(fa::extend_split_sink_kernel<T, D, false, true>, grid, st, sa);
    } else if (window && paged) launch256(fa::extend_split_kernel<T, D, true, true, true>, grid, st, a);
    else if (window) launch256(fa::extend_split_kernel<T, D, false, true, true>, grid, st, a);
    else if (paged) launch256(fa::extend_split_kernel<T, D, true, true>, grid, st, a);
    else launch256(fa::extend_split_kernel<T, D, false, true>, grid, st, a);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_err(what, e);
  if (a.nsplit > 1) {
    const long rows = (f == RAGGED ? 1L : a.nseq) * a.H * a.Nq;   // one workgroup per output row
    // (softcap: the partials' m are capped logits already, so the EXISTING combine instances run with tau = 1; the softmax scale
    // left there would weigh the splits wrongly)
    SplitArgs one = a;
    one.tau = 1.0f;
    const SplitArgs& ca = a.softcap > 0.f ? one : a;
    if (a.f8.on) launch256(fa::decode_combine_kernel<D, false, true>, rows, st, with_scales(a));
    else if (a.sink_logits && f == RAGGED)   // (the logits: the lsink build, which adds the sink column behind its reduction)
      launch256(fa::decode_combine_lsink_kernel<D, true>, rows, st, with_lsink<fa::RaggedLsinkArgs, fa::RaggedArgs>(a));
    else if (a.sink_logits) launch256(fa::decode_combine_lsink_kernel<D, false>, rows, st, with_lsink<fa::LsinkArgs, fa::DecodeArgs>(a));
    else if (f == RAGGED) launch256(fa::decode_combine_kernel<D, true>, rows, st, ca);
    else launch256(fa::decode_combine_kernel<D>, rows, st, ca);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_err(a.f8.on ? "decode_combine_kernel (fp8) launch" : FAMILIES[f].combine_launch, e);
  }
  return FA_OK;
}

template <typename T> int launch_split_d(const SplitArgs& a, Family f, int d, hipStream_t st) {
  switch (d) {
    case 32: return launch_split<T, 32>(a, f, st);
    case 64: return launch_split<T, 64>(a, f, st);
    default: return launch_split<T, 128>(a, f, st);
  }
}

// The launches of a checked attention under the policy its check returned.
int run_attend(const KvCall& c, const Policy& p) {
  const bool ragged = c.family == RAGGED;
  SplitArgs a;
  a.q = c.q;
  a.k = c.k_cache;
  a.v = c.v_cache;
  a.out = c.out;
  a.lse = c.lse;
  a.map = static_cast<const int*>(c.workspace);   // (ragged: the block map, then the partials)
  a.part_o = reinterpret_cast<float*>(static_cast<char*>(c.workspace) + p.map_bytes);
  a.part_ml = p.nsplit > 1 || ragged ? a.part_o + (size_t)c.seqs() * c.H * p.nsplit * c.Nq * c.d : nullptr;
  a.seqlens = c.seqlens;
  a.cu = c.cu;
  a.nseq = c.B;
  a.ntok = c.Nq;
  a.H = c.H;
  a.Hkv = c.Hkv;
  a.G = c.H / c.Hkv;
  a.inv_G = 1.0f / (float)a.G;
  a.Nq = c.Nq;   // (ragged: the combine kernel's view, one batch element of T queries)
  a.Ncap = c.Ncap;
  a.nsplit = p.nsplit;
  a.chunk = p.chunk;
  a.window = win_of(c.window, c.sink, c.Ncap);
  a.sink = sink_of(c.window, c.sink, c.Ncap);
  a.nqb = (int)p.nqb;
  a.items = (int)p.items;
  const bool q_bnhd = c.bnhd() || ragged;   // (the packed buffers are token-major whatever the caches' layout)
  a.q_ld = q_bnhd ? c.H * c.d : c.d;
  a.q_bstride = (long)c.Nq * c.H * c.d;
  a.q_hstride = q_bnhd ? c.d : (long)c.Nq * c.d;
  set_cache_geometry(a, c);
  a.causal = c.causal ? 1 : 0;
  a.tau = c.softmax_scale > 0.f ? c.softmax_scale : sqrtf(1.0f / (float)c.d);
  a.f8 = c.f8;
  a.softcap = c.softcap;
  a.sink_logits = c.sink_logits;
  return c.dtype == FA_DTYPE_BF16 ? launch_split_d<fa::bf16_t>(a, c.family, c.d, c.stream) : launch_split_d<float>(a, c.family, c.d, c.stream);
}

template <typename T, int E> int launch_append(fa::RaggedAppendArgs a, int d, hipStream_t st) {
  a.ch_shift = __builtin_ctz(d / E);
  a.lanes <<= a.ch_shift;   // (rows on entry)
  const long grid = (a.lanes + 255) / 256;
  if (a.cu && a.table) launch256(fa::decode_append_kernel<T, E, true, true>, grid, st, a);
  else if (a.cu) launch256(fa::decode_append_kernel<T, E, false, true>, grid, st, a);
  else if (a.table) launch256(fa::decode_append_kernel<T, E, true>, grid, st, a);
  else launch256(fa::decode_append_kernel<T, E>, grid, st, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? FA_OK : hip_err("decode_append_kernel launch", e);
}

template <int E> int launch_append_fp8(fa::Fp8AppendArgs a, int d, hipStream_t st) {
  a.ch_shift = __builtin_ctz(d / E);
  a.lanes <<= a.ch_shift;   // (rows on entry)
  const long grid = (a.lanes + 255) / 256;
  if (a.table) launch256(fa::append_fp8_kernel<E, true>, grid, st, a);
  else launch256(fa::append_fp8_kernel<E>, grid, st, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? FA_OK : hip_err("append_fp8_kernel launch", e);
}

// The append launch of a checked call.  Ragged: the append of T packed rows shared by the B sequences.
int run_append(const KvCall& c) {
  const uintptr_t news = (uintptr_t)c.k_new | (uintptr_t)c.v_new, caches = (uintptr_t)c.k_cache | (uintptr_t)c.v_cache;
  if (c.f8.on) {   // bf16 sources into byte caches: eight elements to a lane where every source row starts on 16 bytes and every cache row on 8
    fa::Fp8AppendArgs a;
    set_append(a, c);
    a.k_scale = c.f8.k_scale;
    a.v_scale = c.f8.v_scale;
    const bool vec8 = c.d_new % 8 == 0 && (news & 15) == 0 && (caches & 7) == 0;
    return vec8 ? launch_append_fp8<8>(a, c.d, c.stream) : launch_append_fp8<1>(a, c.d, c.stream);
  }
  fa::RaggedAppendArgs a;
  set_append(a, c);
  a.cu = c.cu;
  a.nseq = c.B;
  a.ntok = c.Nq;
  // 16-byte lanes where every row of the source starts on 16 bytes, as every row of the cache does once its base is
  const bool vec = (c.d_new * c.esz()) % 16 == 0 && ((news | caches) & 15) == 0;
  if (c.dtype == FA_DTYPE_BF16) return vec ? launch_append<fa::bf16_t, 8>(a, c.d, c.stream) : launch_append<fa::bf16_t, 1>(a, c.d, c.stream);
  return vec ? launch_append<float, 4>(a, c.d, c.stream) : launch_append<float, 1>(a, c.d, c.stream);
}

// The one path of every attention and append entry point: every check, in the order in which errors win, then the launches.
int run(KvCall c) {
  int rc = c.f8.on ? check_fp8(c.dtype) : check_window(c.window, c.causal, c.sink, c.softcap);
  if (rc == FA_OK && c.paged) rc = check_pages(c.pg, &c.Ncap);
  Policy p{};
  if (rc == FA_OK && c.attend) rc = check_attend(c, &p);
  if (rc == FA_OK && c.append) rc = check_append(c);
  if (rc == FA_OK && c.append) rc = run_append(c);
  if (rc == FA_OK && c.attend) rc = run_attend(c, p);
  return rc;
}

// ---- rotary embeddings (include/flash_attn_mi355x_decode_rope.h) ----
// A tensor rotated by position, and the roped append that goes in front of the EXISTING attend-only entry points (rope_kernel and
// rope_append_kernel of fa_rope.h; no attention kernel changes).
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
  const long grid = (a.lanes + 255) / 256;
  if (il) launch256(fa::rope_kernel<T, E, true>, grid, st, a);
  else launch256(fa::rope_kernel<T, E, false>, grid, st, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? FA_OK : hip_err("rope_kernel launch", e);
}

template <typename T, int E, bool IL, bool FP8> void launch_rope_append_il(const fa::RopeAppendArgs& a, long grid, hipStream_t st) {
  if constexpr (FP8) {
    if (a.table) launch256(fa::rope_append_kernel<T, E, IL, true, false, true>, grid, st, a);
    else launch256(fa::rope_append_kernel<T, E, IL, false, false, true>, grid, st, a);
  } else if (a.cu && a.table) launch256(fa::rope_append_kernel<T, E, IL, true, true>, grid, st, a);
  else if (a.cu) launch256(fa::rope_append_kernel<T, E, IL, false, true>, grid, st, a);
  else if (a.table) launch256(fa::rope_append_kernel<T, E, IL, true>, grid, st, a);
  else launch256(fa::rope_append_kernel<T, E, IL>, grid, st, a);
}

template <typename T, int E, bool FP8> int launch_rope_append(fa::RopeAppendArgs a, bool il, hipStream_t st) {
  a.ch_shift = __builtin_ctz(a.d / E);
  a.lanes <<= a.ch_shift;     // (rows on entry)
  a.q_lanes <<= a.ch_shift;
  const long grid = (a.q_lanes + a.lanes + 255) / 256;
  if (il)
    launch_rope_append_il<T, E, true, FP8>(a, grid, st);
  else
    launch_rope_append_il<T, E, false, FP8>(a, grid, st);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? FA_OK : hip_err("rope_append_kernel launch", e);
}

// What a roped append takes beside the cache call: where the rotated q goes, the tables and the rotary dimension.
struct Rope {
  void* q_rot;
  const float *cos, *sin;
  int rot, max_pos, interleaved;
};

// One roped append, uniform (the extend family: Nq new tokens per batch element, any number) or ragged (Nq = T packed rows); q / q_rot
// or k_new / v_new may be absent (both null).  Every check comes first; then the one launch.
int rope_append_call(KvCall c, const Rope& r) {
  const bool ragged = c.family == RAGGED;
  g_err[0] = 0;
  int rc = c.f8.on ? check_fp8(c.dtype) : FA_OK;
  if (rc != FA_OK) return rc;
  if ((c.q == nullptr) != (r.q_rot == nullptr)) return set_err(FA_ERR_BAD_ARG, "q and q_rot go together: give both, or neither (append only)");
  if ((c.k_new == nullptr) != (c.v_new == nullptr))
    return set_err(FA_ERR_BAD_ARG, "k_new and v_new go together: give both, or neither (rotate q only)");
  if (!c.q && !c.k_new) return set_err(FA_ERR_BAD_ARG, "nothing to do: q / q_rot and k_new / v_new are all null");
  if (c.paged) rc = check_pages(c.pg, &c.Ncap);
  if (rc != FA_OK) return rc;
  if (c.k_new) {
    rc = check_append(c);
    if (rc != FA_OK) return rc;
  } else {
    if (c.B <= 0 || c.Nq <= 0 || c.Ncap <= 0 || c.d <= 0) return set_err(FA_ERR_BAD_ARG, "B, Nq (T), Ncap and d must be positive");
    if (c.dtype != FA_DTYPE_F32 && c.dtype != FA_DTYPE_BF16) return set_err(FA_ERR_BAD_ARG, "unknown dtype");
    if (c.layout != FA_LAYOUT_BHND && c.layout != FA_LAYOUT_BNHD) return set_err(FA_ERR_BAD_ARG, "unknown layout");
    if (ragged && !c.cu) return set_err(FA_ERR_BAD_ARG, "null cu_seqlens_q");
    if (c.d != 32 && c.d != 64 && c.d != 128) return set_err(FA_ERR_UNSUPPORTED_D, "decode supports rows of d in {32, 64, 128}");
    c.d_new = c.d;
  }
  if (c.q) {
    if (c.H <= 0) return set_err(FA_ERR_BAD_ARG, "H must be positive");
    // (one lane per element at the most, the workgroup count of q's and the new rows' lanes together an unsigned int)
    if (c.seqs() * c.Nq * c.H * c.d / 256 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "too many q elements for one rope_append launch");
  }
  rc = check_rope(r.cos, r.sin, r.rot, std::min(c.d_new, c.d), r.max_pos, r.interleaved, 0);
  if (rc != FA_OK) return rc;
  if (r.max_pos < c.Ncap) {
    snprintf(g_err, sizeof(g_err), "max_pos = %d table rows do not cover the cache's capacity of %d rows: every row needs an angle", r.max_pos,
             c.Ncap);
    return FA_ERR_BAD_ARG;
  }
  fa::RopeAppendArgs a;
  set_append(a, c);
  a.q = c.q;
  a.q_rot = r.q_rot;
  a.cos = r.cos;
  a.sin = r.sin;
  a.k_scale = c.f8.k_scale;
  a.v_scale = c.f8.v_scale;
  a.q_lanes = c.q ? c.seqs() * c.Nq * c.H : 0;
  a.H = c.H;
  a.d = c.d;
  a.rot = r.rot;
  a.max_pos = r.max_pos;
  a.cu = c.cu;
  a.nseq = c.B;
  a.ntok = c.Nq;
  const uintptr_t ptrs = (uintptr_t)c.q | (uintptr_t)r.q_rot | (uintptr_t)c.k_new | (uintptr_t)c.v_new | (uintptr_t)r.cos | (uintptr_t)r.sin;
  const uintptr_t caches = c.k_new ? (uintptr_t)c.k_cache | (uintptr_t)c.v_cache : 0;
  const bool vec = rope_vec(16 / (int)c.esz(), r.rot, r.interleaved, c.d_new, c.d, ptrs, caches, c.f8.on ? 8 : 16);
  const bool il = r.interleaved != 0;
  if (c.f8.on)
    return vec ? launch_rope_append<fa::bf16_t, 8, true>(a, il, c.stream) : launch_rope_append<fa::bf16_t, 1, true>(a, il, c.stream);
  if (c.dtype == FA_DTYPE_BF16)
    return vec ? launch_rope_append<fa::bf16_t, 8, false>(a, il, c.stream) : launch_rope_append<fa::bf16_t, 1, false>(a, il, c.stream);
  return vec ? launch_rope_append<float, 4, false>(a, il, c.stream) : launch_rope_append<float, 1, false>(a, il, c.stream);
}

}  // namespace

extern "C" {

// ---- the size queries: the policy's split count and workspace on (window, sink), 0 and 0 in the forms that have none ----
int fa_mi355x_decode_splits_gqa(int B, int H, int Hkv, int Nq, int Ncap, int d, int dtype) {
  (void)dtype;
  return query(DECODE, B, H, Hkv, Nq, Ncap, d, 0, 0).nsplit;
}

size_t fa_mi355x_decode_workspace_bytes_gqa(int B, int H, int Hkv, int Nq, int Ncap, int d) {
  return query(DECODE, B, H, Hkv, Nq, Ncap, d, 0, 0).workspace_bytes;
}

int fa_mi355x_extend_splits(int B, int H, int Hkv, int Nq, int Ncap, int d, int dtype) {
  (void)dtype;
  return query(EXTEND, B, H, Hkv, Nq, Ncap, d, 0, 0).nsplit;
}

size_t fa_mi355x_extend_workspace_bytes(int B, int H, int Hkv, int Nq, int Ncap, int d) {
  return query(EXTEND, B, H, Hkv, Nq, Ncap, d, 0, 0).workspace_bytes;
}

int fa_mi355x_ragged_splits(int B, int H, int Hkv, int T, int Ncap, int d, int dtype) {
  (void)dtype;
  return query(RAGGED, B, H, Hkv, T, Ncap, d, 0, 0).nsplit;
}

size_t fa_mi355x_ragged_workspace_bytes(int B, int H, int Hkv, int T, int Ncap, int d) {
  return query(RAGGED, B, H, Hkv, T, Ncap, d, 0, 0).workspace_bytes;
}

int fa_mi355x_decode_window_splits(int B, int H, int Hkv, int Nq, int Ncap, int d, int dtype, int window) {
  (void)dtype;
  return query(DECODE, B, H, Hkv, Nq, Ncap, d, window, 0).nsplit;
}

size_t fa_mi355x_decode_window_workspace_bytes(int B, int H, int Hkv, int Nq, int Ncap, int d, int window) {
  return query(DECODE, B, H, Hkv, Nq, Ncap, d, window, 0).workspace_bytes;
}

int fa_mi355x_extend_window_splits(int B, int H, int Hkv, int Nq, int Ncap, int d, int dtype, int window) {
  (void)dtype;
  return query(EXTEND, B, H, Hkv, Nq, Ncap, d, window, 0).nsplit;
}

size_t fa_mi355x_extend_window_workspace_bytes(int B, int H, int Hkv, int Nq, int Ncap, int d, int window) {
  return query(EXTEND, B, H, Hkv, Nq, Ncap, d, window, 0).workspace_bytes;
}

int fa_mi355x_ragged_window_splits(int B, int H, int Hkv, int T, int Ncap, int d, int dtype, int window) {
  (void)dtype;
  return query(RAGGED, B, H, Hkv, T, Ncap, d, window, 0).nsplit;
}

size_t fa_mi355x_ragged_window_workspace_bytes(int B, int H, int Hkv, int T, int Ncap, int d, int window) {
  return query(RAGGED, B, H, Hkv, T, Ncap, d, window, 0).workspace_bytes;
}

int fa_mi355x_decode_sink_splits(int B, int H, int Hkv, int Nq, int Ncap, int d, int dtype, int window, int sink) {
  (void)dtype;
  return query(DECODE, B, H, Hkv, Nq, Ncap, d, window, sink).nsplit;
}

size_t fa_mi355x_decode_sink_workspace_bytes(int B, int H, int Hkv, int Nq, int Ncap, int d, int window, int sink) {
  return query(DECODE, B, H, Hkv, Nq, Ncap, d, window, sink).workspace_bytes;
}

int fa_mi355x_extend_sink_splits(int B, int H, int Hkv, int Nq, int Ncap, int d, int dtype, int window, int sink) {
  (void)dtype;
  return query(EXTEND, B, H, Hkv, Nq, Ncap, d, window, sink).nsplit;
}

size_t fa_mi355x_extend_sink_workspace_bytes(int B, int H, int Hkv, int Nq, int Ncap, int d, int window, int sink) {
  return query(EXTEND, B, H, Hkv, Nq, Ncap, d, window, sink).workspace_bytes;
}

int fa_mi355x_ragged_sink_splits(int B, int H, int Hkv, int T, int Ncap, int d, int dtype, int window, int sink) {
  (void)dtype;
  return query(RAGGED, B, H, Hkv, T, Ncap, d, window, sink).nsplit;
}

size_t fa_mi355x_ragged_sink_workspace_bytes(int B, int H, int Hkv, int T, int Ncap, int d, int window, int sink) {
  return query(RAGGED, B, H, Hkv, T, Ncap, d, window, sink).workspace_bytes;
}

// ---- decode and extend on slabs of Ncap rows: the attention, the append, and the append then the attention ----
int fa_mi355x_fwd_decode_gqa(const void* q, const void* k_cache, const void* v_cache, float* out, float* lse, const int* cache_seqlens,
                             void* workspace, int B, int H, int Hkv, int Nq, int Ncap, int d, int layout, float softmax_scale,
                             int causal, int dtype, void* stream) {
  KvCall c(DECODE);
  c.attention(q, out, lse, workspace, softmax_scale, causal).cache(k_cache, v_cache, cache_seqlens, Ncap);
  return run(c.heads(B, H, Hkv, Nq, d).format(layout, dtype, stream));
}

int fa_mi355x_decode_append(const void* k_new, const void* v_new, void* k_cache, void* v_cache, const int* cache_seqlens, int B, int Hkv,
                            int Nq, int Ncap, int d_new, int d, int layout, int dtype, void* stream) {
  KvCall c(DECODE);
  c.new_tokens(k_new, v_new, d_new).cache(k_cache, v_cache, cache_seqlens, Ncap);
  return run(c.heads(B, Hkv, Hkv, Nq, d).format(layout, dtype, stream));
}

int fa_mi355x_fwd_decode_append(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                                const int* cache_seqlens, void* workspace, int B, int H, int Hkv, int Nq, int Ncap, int d_new, int d,
                                int layout, float softmax_scale, int causal, int dtype, void* stream) {
  KvCall c(DECODE);
  c.attention(q, out, lse, workspace, softmax_scale, causal).new_tokens(k_new, v_new, d_new).cache(k_cache, v_cache, cache_seqlens, Ncap);
  return run(c.heads(B, H, Hkv, Nq, d).format(layout, dtype, stream));
}

int fa_mi355x_fwd_extend(const void* q, const void* k_cache, const void* v_cache, float* out, float* lse, const int* cache_seqlens,
                         void* workspace, int B, int H, int Hkv, int Nq, int Ncap, int d, int layout, float softmax_scale, int causal,
                         int dtype, void* stream) {
  KvCall c(EXTEND);
  c.attention(q, out, lse, workspace, softmax_scale, causal).cache(k_cache, v_cache, cache_seqlens, Ncap);
  return run(c.heads(B, H, Hkv, Nq, d).format(layout, dtype, stream));
}

int fa_mi355x_extend_append(const void* k_new, const void* v_new, void* k_cache, void* v_cache, const int* cache_seqlens, int B, int Hkv,
                            int Nq, int Ncap, int d_new, int d, int layout, int dtype, void* stream) {
  KvCall c(EXTEND);
  c.new_tokens(k_new, v_new, d_new).cache(k_cache, v_cache, cache_seqlens, Ncap);
  return run(c.heads(B, Hkv, Hkv, Nq, d).format(layout, dtype, stream));
}

int fa_mi355x_fwd_extend_append(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                                const int* cache_seqlens, void* workspace, int B, int H, int Hkv, int Nq, int Ncap, int d_new, int d,
                                int layout, float softmax_scale, int causal, int dtype, void* stream) {
  KvCall c(EXTEND);
  c.attention(q, out, lse, workspace, softmax_scale, causal).new_tokens(k_new, v_new, d_new).cache(k_cache, v_cache, cache_seqlens, Ncap);
  return run(c.heads(B, H, Hkv, Nq, d).format(layout, dtype, stream));
}

// ---- the paged entry points: the forms above on a pool of pages read through a block table, whose geometry stands for Ncap ----
int fa_mi355x_fwd_decode_paged(const void* q, const void* k_pool, const void* v_pool, float* out, float* lse, const int* cache_seqlens,
                               const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int num_pages, int page_size,
                               int max_pages, int d, int layout, float softmax_scale, int causal, int dtype, void* stream) {
  KvCall c(DECODE);
  c.attention(q, out, lse, workspace, softmax_scale, causal).cache(k_pool, v_pool, cache_seqlens, 0);
  c.pool(block_table, num_pages, page_size, max_pages);
  return run(c.heads(B, H, Hkv, Nq, d).format(layout, dtype, stream));
}

int fa_mi355x_fwd_extend_paged(const void* q, const void* k_pool, const void* v_pool, float* out, float* lse, const int* cache_seqlens,
                               const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int num_pages, int page_size,
                               int max_pages, int d, int layout, float softmax_scale, int causal, int dtype, void* stream) {
  KvCall c(EXTEND);
  c.attention(q, out, lse, workspace, softmax_scale, causal).cache(k_pool, v_pool, cache_seqlens, 0);
  c.pool(block_table, num_pages, page_size, max_pages);
  return run(c.heads(B, H, Hkv, Nq, d).format(layout, dtype, stream));
}

int fa_mi355x_decode_append_paged(const void* k_new, const void* v_new, void* k_pool, void* v_pool, const int* cache_seqlens,
                                  const int* block_table, int B, int Hkv, int Nq, int num_pages, int page_size, int max_pages, int d_new,
                                  int d, int layout, int dtype, void* stream) {
  KvCall c(DECODE);
  c.new_tokens(k_new, v_new, d_new).cache(k_pool, v_pool, cache_seqlens, 0);
  c.pool(block_table, num_pages, page_size, max_pages);
  return run(c.heads(B, Hkv, Hkv, Nq, d).format(layout, dtype, stream));
}

int fa_mi355x_extend_append_paged(const void* k_new, const void* v_new, void* k_pool, void* v_pool, const int* cache_seqlens,
                                  const int* block_table, int B, int Hkv, int Nq, int num_pages, int page_size, int max_pages, int d_new,
                                  int d, int layout, int dtype, void* stream) {
  KvCall c(EXTEND);
  c.new_tokens(k_new, v_new, d_new).cache(k_pool, v_pool, cache_seqlens, 0);
  c.pool(block_table, num_pages, page_size, max_pages);
  return run(c.heads(B, Hkv, Hkv, Nq, d).format(layout, dtype, stream));
}

int fa_mi355x_fwd_decode_append_paged(const void* q, const void* k_new, const void* v_new, void* k_pool, void* v_pool, float* out,
                                      float* lse, const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv,
                                      int Nq, int num_pages, int page_size, int max_pages, int d_new, int d, int layout,
                                      float softmax_scale, int causal, int dtype, void* stream) {
  KvCall c(DECODE);
  c.attention(q, out, lse, workspace, softmax_scale, causal).new_tokens(k_new, v_new, d_new).cache(k_pool, v_pool, cache_seqlens, 0);
  c.pool(block_table, num_pages, page_size, max_pages);
  return run(c.heads(B, H, Hkv, Nq, d).format(layout, dtype, stream));
}

int fa_mi355x_fwd_extend_append_paged(const void* q, const void* k_new, const void* v_new, void* k_pool, void* v_pool, float* out,
                                      float* lse, const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv,
                                      int Nq, int num_pages, int page_size, int max_pages, int d_new, int d, int layout,
                                      float softmax_scale, int causal, int dtype, void* stream) {
  KvCall c(EXTEND);
  c.attention(q, out, lse, workspace, softmax_scale, causal).new_tokens(k_new, v_new, d_new).cache(k_pool, v_pool, cache_seqlens, 0);
  c.pool(block_table, num_pages, page_size, max_pages);
  return run(c.heads(B, H, Hkv, Nq, d).format(layout, dtype, stream));
}

// ---- the ragged entry points (include/flash_attn_mi355x_decode_ragged.h): the new tokens of all sequences packed into T rows, the
// sequences' boundaries in cu_seqlens_q on the device ----
int fa_mi355x_fwd_ragged(const void* q, const void* k_cache, const void* v_cache, float* out, float* lse, const int* cu_seqlens_q,
                         const int* cache_seqlens, void* workspace, int B, int H, int Hkv, int T, int Ncap, int d, int layout,
                         float softmax_scale, int causal, int dtype, void* stream) {
  KvCall c(RAGGED);
  c.attention(q, out, lse, workspace, softmax_scale, causal).cache(k_cache, v_cache, cache_seqlens, Ncap);
  c.cu = cu_seqlens_q;
  return run(c.heads(B, H, Hkv, T, d).format(layout, dtype, stream));
}

int fa_mi355x_ragged_append(const void* k_new, const void* v_new, void* k_cache, void* v_cache, const int* cu_seqlens_q,
                            const int* cache_seqlens, int B, int Hkv, int T, int Ncap, int d_new, int d, int layout, int dtype,
                            void* stream) {
  KvCall c(RAGGED);
  c.new_tokens(k_new, v_new, d_new).cache(k_cache, v_cache, cache_seqlens, Ncap);
  c.cu = cu_seqlens_q;
  return run(c.heads(B, Hkv, Hkv, T, d).format(layout, dtype, stream));
}

int fa_mi355x_fwd_ragged_append(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                                const int* cu_seqlens_q, const int* cache_seqlens, void* workspace, int B, int H, int Hkv, int T,
                                int Ncap, int d_new, int d, int layout, float softmax_scale, int causal, int dtype, void* stream) {
  KvCall c(RAGGED);
  c.attention(q, out, lse, workspace, softmax_scale, causal).new_tokens(k_new, v_new, d_new).cache(k_cache, v_cache, cache_seqlens, Ncap);
  c.cu = cu_seqlens_q;
  return run(c.heads(B, H, Hkv, T, d).format(layout, dtype, stream));
}

int fa_mi355x_fwd_ragged_paged(const void* q, const void* k_pool, const void* v_pool, float* out, float* lse, const int* cu_seqlens_q,
                               const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv, int T,
                               int num_pages, int page_size, int max_pages, int d, int layout, float softmax_scale, int causal,
                               int dtype, void* stream) {
  KvCall c(RAGGED);
  c.attention(q, out, lse, workspace, softmax_scale, causal).cache(k_pool, v_pool, cache_seqlens, 0);
  c.cu = cu_seqlens_q;
  c.pool(block_table, num_pages, page_size, max_pages);
  return run(c.heads(B, H, Hkv, T, d).format(layout, dtype, stream));
}

int fa_mi355x_ragged_append_paged(const void* k_new, const void* v_new, void* k_pool, void* v_pool, const int* cu_seqlens_q,
                                  const int* cache_seqlens, const int* block_table, int B, int Hkv, int T, int num_pages, int page_size,
                                  int max_pages, int d_new, int d, int layout, int dtype, void* stream) {
  KvCall c(RAGGED);
  c.new_tokens(k_new, v_new, d_new).cache(k_pool, v_pool, cache_seqlens, 0);
  c.cu = cu_seqlens_q;
  c.pool(block_table, num_pages, page_size, max_pages);
  return run(c.heads(B, Hkv, Hkv, T, d).format(layout, dtype, stream));
}

int fa_mi355x_fwd_ragged_append_paged(const void* q, const void* k_new, const void* v_new, void* k_pool, void* v_pool, float* out,
                                      float* lse, const int* cu_seqlens_q, const int* cache_seqlens, const int* block_table,
                                      void* workspace, int B, int H, int Hkv, int T, int num_pages, int page_size, int max_pages,
                                      int d_new, int d, int layout, float softmax_scale, int causal, int dtype, void* stream) {
  KvCall c(RAGGED);
  c.attention(q, out, lse, workspace, softmax_scale, causal).new_tokens(k_new, v_new, d_new).cache(k_pool, v_pool, cache_seqlens, 0);
  c.cu = cu_seqlens_q;
  c.pool(block_table, num_pages, page_size, max_pages);
  return run(c.heads(B, H, Hkv, T, d).format(layout, dtype, stream));
}

// ---- the windowed, sink and fp8 entry points (_window.h, _sink.h, _fp8.h): one per call family.  k_new / v_new both null: attend
// only; block_table null: slabs of Ncap rows, otherwise the pool's geometry stands for Ncap ----
int fa_mi355x_fwd_decode_window(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                                const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int Ncap,
                                int num_pages, int page_size, int max_pages, int d_new, int d, int layout, float softmax_scale, int causal,
                                int window, int dtype, void* stream) {
  return fa_mi355x_fwd_decode_sink(q, k_new, v_new, k_cache, v_cache, out, lse, cache_seqlens, block_table, workspace, B, H, Hkv, Nq, Ncap,
                                   num_pages, page_size, max_pages, d_new, d, layout, softmax_scale, causal, window, 0, dtype, stream);
}

int fa_mi355x_fwd_extend_window(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                                const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int Ncap,
                                int num_pages, int page_size, int max_pages, int d_new, int d, int layout, float softmax_scale, int causal,
                                int window, int dtype, void* stream) {
  return fa_mi355x_fwd_extend_sink(q, k_new, v_new, k_cache, v_cache, out, lse, cache_seqlens, block_table, workspace, B, H, Hkv, Nq, Ncap,
                                   num_pages, page_size, max_pages, d_new, d, layout, softmax_scale, causal, window, 0, dtype, stream);
}

int fa_mi355x_fwd_ragged_window(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                                const int* cu_seqlens_q, const int* cache_seqlens, const int* block_table, void* workspace, int B, int H,
                                int Hkv, int T, int Ncap, int num_pages, int page_size, int max_pages, int d_new, int d, int layout,
                                float softmax_scale, int causal, int window, int dtype, void* stream) {
  return fa_mi355x_fwd_ragged_sink(q, k_new, v_new, k_cache, v_cache, out, lse, cu_seqlens_q, cache_seqlens, block_table, workspace, B, H,
                                   Hkv, T, Ncap, num_pages, page_size, max_pages, d_new, d, layout, softmax_scale, causal, window, 0, dtype,
                                   stream);
}

int fa_mi355x_fwd_decode_sink(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                              const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int Ncap,
                              int num_pages, int page_size, int max_pages, int d_new, int d, int layout, float softmax_scale, int causal,
                              int window, int sink, int dtype, void* stream) {
  KvCall c(DECODE);
  c.attention(q, out, lse, workspace, softmax_scale, causal).cache(k_cache, v_cache, cache_seqlens, Ncap);
  c.pool_or_slabs(block_table, num_pages, page_size, max_pages).heads(B, H, Hkv, Nq, d).format(layout, dtype, stream);
  if (k_new || v_new) c.new_tokens(k_new, v_new, d_new);
  c.window = window, c.sink = sink;
  return run(c);
}

int fa_mi355x_fwd_extend_sink(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                              const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int Ncap,
                              int num_pages, int page_size, int max_pages, int d_new, int d, int layout, float softmax_scale, int causal,
                              int window, int sink, int dtype, void* stream) {
  KvCall c(EXTEND);
  c.attention(q, out, lse, workspace, softmax_scale, causal).cache(k_cache, v_cache, cache_seqlens, Ncap);
  c.pool_or_slabs(block_table, num_pages, page_size, max_pages).heads(B, H, Hkv, Nq, d).format(layout, dtype, stream);
  if (k_new || v_new) c.new_tokens(k_new, v_new, d_new);
  c.window = window, c.sink = sink;
  return run(c);
}

int fa_mi355x_fwd_ragged_sink(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                              const int* cu_seqlens_q, const int* cache_seqlens, const int* block_table, void* workspace, int B, int H,
                              int Hkv, int T, int Ncap, int num_pages, int page_size, int max_pages, int d_new, int d, int layout,
                              float softmax_scale, int causal, int window, int sink, int dtype, void* stream) {
  KvCall c(RAGGED);
  c.attention(q, out, lse, workspace, softmax_scale, causal).cache(k_cache, v_cache, cache_seqlens, Ncap);
  c.pool_or_slabs(block_table, num_pages, page_size, max_pages).heads(B, H, Hkv, T, d).format(layout, dtype, stream);
  if (k_new || v_new) c.new_tokens(k_new, v_new, d_new);
  c.cu = cu_seqlens_q;
  c.window = window, c.sink = sink;
  return run(c);
}

// ---- logit soft-capping (_softcap.h): the windowed forms with the cap behind the window; softcap = 0 is the _window call ----
int fa_mi355x_fwd_decode_softcap(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                                 const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int Ncap,
                                 int num_pages, int page_size, int max_pages, int d_new, int d, int layout, float softmax_scale, int causal,
                                 int window, float softcap, int dtype, void* stream) {
  KvCall c(DECODE);
  c.attention(q, out, lse, workspace, softmax_scale, causal).cache(k_cache, v_cache, cache_seqlens, Ncap);
  c.pool_or_slabs(block_table, num_pages, page_size, max_pages).heads(B, H, Hkv, Nq, d).format(layout, dtype, stream);
  if (k_new || v_new) c.new_tokens(k_new, v_new, d_new);
  c.window = window, c.softcap = softcap;
  return run(c);
}

int fa_mi355x_fwd_extend_softcap(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                                 const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int Ncap,
                                 int num_pages, int page_size, int max_pages, int d_new, int d, int layout, float softmax_scale, int causal,
                                 int window, float softcap, int dtype, void* stream) {
  KvCall c(EXTEND);
  c.attention(q, out, lse, workspace, softmax_scale, causal).cache(k_cache, v_cache, cache_seqlens, Ncap);
  c.pool_or_slabs(block_table, num_pages, page_size, max_pages).heads(B, H, Hkv, Nq, d).format(layout, dtype, stream);
  if (k_new || v_new) c.new_tokens(k_new, v_new, d_new);
  c.window = window, c.softcap = softcap;
  return run(c);
}

int fa_mi355x_fwd_ragged_softcap(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                                 const int* cu_seqlens_q, const int* cache_seqlens, const int* block_table, void* workspace, int B, int H,
                                 int Hkv, int T, int Ncap, int num_pages, int page_size, int max_pages, int d_new, int d, int layout,
                                 float softmax_scale, int causal, int window, float softcap, int dtype, void* stream) {
  KvCall c(RAGGED);
  c.attention(q, out, lse, workspace, softmax_scale, causal).cache(k_cache, v_cache, cache_seqlens, Ncap);
  c.pool_or_slabs(block_table, num_pages, page_size, max_pages).heads(B, H, Hkv, T, d).format(layout, dtype, stream);
  if (k_new || v_new) c.new_tokens(k_new, v_new, d_new);
  c.cu = cu_seqlens_q;
  c.window = window, c.softcap = softcap;
  return run(c);
}

// ---- learned sink logits (_lsink.h): the windowed forms with the logits behind the window; null sink_logits is the _window call ----
int fa_mi355x_fwd_decode_lsink(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                               const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int Ncap,
                               int num_pages, int page_size, int max_pages, int d_new, int d, int layout, float softmax_scale, int causal,
                               int window, const float* sink_logits, int dtype, void* stream) {
  KvCall c(DECODE);
  c.attention(q, out, lse, workspace, softmax_scale, causal).cache(k_cache, v_cache, cache_seqlens, Ncap);
  c.pool_or_slabs(block_table, num_pages, page_size, max_pages).heads(B, H, Hkv, Nq, d).format(layout, dtype, stream);
  if (k_new || v_new) c.new_tokens(k_new, v_new, d_new);
  c.window = window, c.sink_logits = sink_logits;
  return run(c);
}

int fa_mi355x_fwd_extend_lsink(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                               const int* cache_seqlens, const int* block_table, void* workspace, int B, int H, int Hkv, int Nq, int Ncap,
                               int num_pages, int page_size, int max_pages, int d_new, int d, int layout, float softmax_scale, int causal,
                               int window, const float* sink_logits, int dtype, void* stream) {
  KvCall c(EXTEND);
  c.attention(q, out, lse, workspace, softmax_scale, causal).cache(k_cache, v_cache, cache_seqlens, Ncap);
  c.pool_or_slabs(block_table, num_pages, page_size, max_pages).heads(B, H, Hkv, Nq, d).format(layout, dtype, stream);
  if (k_new || v_new) c.new_tokens(k_new, v_new, d_new);
  c.window = window, c.sink_logits = sink_logits;
  return run(c);
}

int fa_mi355x_fwd_ragged_lsink(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, float* out, float* lse,
                               const int* cu_seqlens_q, const int* cache_seqlens, const int* block_table, void* workspace, int B, int H,
                               int Hkv, int T, int Ncap, int num_pages, int page_size, int max_pages, int d_new, int d, int layout,
                               float softmax_scale, int causal, int window, const float* sink_logits, int dtype, void* stream) {
  KvCall c(RAGGED);
  c.attention(q, out, lse, workspace, softmax_scale, causal).cache(k_cache, v_cache, cache_seqlens, Ncap);
  c.pool_or_slabs(block_table, num_pages, page_size, max_pages).heads(B, H, Hkv, T, d).format(layout, dtype, stream);
  if (k_new || v_new) c.new_tokens(k_new, v_new, d_new);
  c.cu = cu_seqlens_q;
  c.window = window, c.sink_logits = sink_logits;
  return run(c);
}

int fa_mi355x_fwd_decode_fp8(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, const float* k_scale,
                             const float* v_scale, float* out, float* lse, const int* cache_seqlens, const int* block_table, void* workspace,
                             int B, int H, int Hkv, int Nq, int Ncap, int num_pages, int page_size, int max_pages, int d_new, int d,
                             int layout, float softmax_scale, int causal, int dtype, void* stream) {
  KvCall c(DECODE);
  c.attention(q, out, lse, workspace, softmax_scale, causal).cache(k_cache, v_cache, cache_seqlens, Ncap);
  c.pool_or_slabs(block_table, num_pages, page_size, max_pages).heads(B, H, Hkv, Nq, d).format(layout, dtype, stream);
  if (k_new || v_new) c.new_tokens(k_new, v_new, d_new);
  c.f8 = {true, k_scale, v_scale};
  return run(c);
}

int fa_mi355x_fwd_extend_fp8(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, const float* k_scale,
                             const float* v_scale, float* out, float* lse, const int* cache_seqlens, const int* block_table, void* workspace,
                             int B, int H, int Hkv, int Nq, int Ncap, int num_pages, int page_size, int max_pages, int d_new, int d,
                             int layout, float softmax_scale, int causal, int dtype, void* stream) {
  KvCall c(EXTEND);
  c.attention(q, out, lse, workspace, softmax_scale, causal).cache(k_cache, v_cache, cache_seqlens, Ncap);
  c.pool_or_slabs(block_table, num_pages, page_size, max_pages).heads(B, H, Hkv, Nq, d).format(layout, dtype, stream);
  if (k_new || v_new) c.new_tokens(k_new, v_new, d_new);
  c.f8 = {true, k_scale, v_scale};
  return run(c);
}

// (the append's checks are the extend family's: any Nq >= 1)
int fa_mi355x_append_fp8(const void* k_new, const void* v_new, void* k_cache, void* v_cache, const float* k_scale, const float* v_scale,
                         const int* cache_seqlens, const int* block_table, int B, int Hkv, int Nq, int Ncap, int num_pages, int page_size,
                         int max_pages, int d_new, int d, int layout, int dtype, void* stream) {
  KvCall c(EXTEND);
  c.new_tokens(k_new, v_new, d_new).cache(k_cache, v_cache, cache_seqlens, Ncap);
  c.pool_or_slabs(block_table, num_pages, page_size, max_pages).heads(B, Hkv, Hkv, Nq, d).format(layout, dtype, stream);
  c.f8 = {true, k_scale, v_scale};
  return run(c);
}

// ---- the rotary entry points (include/flash_attn_mi355x_decode_rope.h) ----
// (no cache call: its own few checks, then the one launch)
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
  KvCall c(EXTEND);   // (the append's checks are the extend family's: any Nq >= 1)
  c.new_tokens(k_new, v_new, d_new).cache(k_cache, v_cache, cache_seqlens, Ncap);
  c.pool_or_slabs(block_table, num_pages, page_size, max_pages).heads(B, H, Hkv, Nq, d).format(layout, dtype, stream);
  c.q = q;
  c.f8 = {cache_fp8 != 0, k_scale, v_scale};
  return rope_append_call(c, {q_rot, cos, sin, rot, max_pos, interleaved});
}

int fa_mi355x_rope_append_ragged(const void* q, void* q_rot, const void* k_new, const void* v_new, void* k_cache, void* v_cache,
                                 const float* cos, const float* sin, const int* cu_seqlens_q, const int* cache_seqlens,
                                 const int* block_table, int B, int H, int Hkv, int T, int Ncap, int num_pages, int page_size, int max_pages,
                                 int d_new, int d, int rot, int max_pos, int layout, int interleaved, int dtype, void* stream) {
  KvCall c(RAGGED);
  c.new_tokens(k_new, v_new, d_new).cache(k_cache, v_cache, cache_seqlens, Ncap);
  c.pool_or_slabs(block_table, num_pages, page_size, max_pages).heads(B, H, Hkv, T, d).format(layout, dtype, stream);
  c.q = q;
  c.cu = cu_seqlens_q;
  return rope_append_call(c, {q_rot, cos, sin, rot, max_pos, interleaved});
}

// ---- the ungrouped entry points: Hkv = H ----
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
