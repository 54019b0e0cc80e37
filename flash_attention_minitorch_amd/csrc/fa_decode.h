// KV-cache decode attention for MI355X (gfx950): Nq = 1..128 new queries against a cache of up to Ncap keys per (batch, kv head), with
// per-batch valid lengths on the device.  Declared in include/flash_attn_mi355x_decode.h, dispatched by fa_decode.hip; the training
// kernels (fa_kernels.h) are not part of this unit.
//
// Grouped-query heads: the cache holds Hkv heads and q holds H = G * Hkv; query head h reads kv head h / G.  The G * Nq (query, head)
// pairs of one kv head are the ROWS of that head, row rho = i * G + g for query i and head hkv * G + g, so the G heads of a group fill
// the 32-row MFMA tile that a single query leaves empty and share one pass over the kv head's K and V.  Query-major order keeps the
// causal positions of a block compact (row rho sits at len - Nq + rho / G), and in [B][Nq][H][d] a block's rows are contiguous.
// G = 1 is the ungrouped call: rho = i.
//
// Split kernel: a workgroup = one (batch*kv head, key chunk, 32-row block).  Its four waves stage 128-key super tiles of K and V through
// LDS together (register staging: the next super tile's loads are in flight under this one's products) and each wave takes 32 keys of
// the super tile: S^T = K Q^T with the ROW on the lane, the online softmax of fwd_splitk_f32_kernel, O^T += V^T P^T from registers.
// At the end the four partial (O, m, l) meet in LDS and wave 0 combines them in wave order.  The result is either final (one split:
// out and lse written directly) or one fp32 partial (unnormalised O, m, l) per row in the workspace.
// Output, lse and the partials are indexed by QUERY head and query row, whatever G.
// Combine kernel: one workgroup per (batch*head, query row) reduces the partials of its row in a fixed order (no atomics: bitwise
// repeatable).
//
// Extend kernel (extend_split_kernel, behind the split kernel): the same call for ANY Nq (a long input after a cached prefix, chunked
// prefill), a workgroup = one (batch*kv head, key chunk, 128-row block) whose waves each own 32 rows and share the staged tiles.
// Append kernel (decode_append_kernel, at the end of this file): writes the Nq new tokens' k and v into the caches in front of the
// kernels above, at the rows where the split kernel's causal mask places the queries.
//
// Bounds: every K / V load goes through a buffer resource of its (batch, kv head) sized to the valid rows (len_b clamped to
// [0, Ncap]), with the row offset in the per-lane voffset, so rows at or past len_b read as zero in hardware: whatever they hold (NaN
// included) reaches neither a score nor the P.V product, and no load goes past row Ncap - 1.  Q goes through a resource of its batch
// element with (head, query) in the voffset; rows rho >= G * Nq get the resource's size as their offset, read as zero and store nothing.
//
// Paged caches (the PAGED builds of the split, extend and append kernels; include/flash_attn_mi355x_decode_paged.h): the cache is a
// pool of pages of page_size rows and a block table [B][max_pages] names each batch element's pages.  page_size is a multiple of the
// 128-key super tile and every chunk starts on a multiple of it, so a staged tile never straddles two pages: paging costs one
// wave-uniform table entry and one resource per super tile (PageWalk), and the tile loop, the LDS image and the MFMA work are those
// of the contiguous builds, which is why a paged call returns the contiguous call's bits on the gathered cache.  The PAGED = false
// builds are the code they were (same registers, LDS and instructions: DESIGN.md "Paged").
//
// Ragged batches (the RAGGED builds of the extend, combine and append kernels; include/flash_attn_mi355x_decode_ragged.h): the new
// tokens of all sequences are PACKED into buffers of T rows, [T][H][d], and cu[b] .. cu[b+1] - 1 are the rows of sequence b, so every
// sequence brings its own number nq_b of new tokens.  ragged_schedule_kernel turns cu into a block map in front of the attention:
// one entry (sequence, row block in it) per 128-row block of a sequence's G * nq_b rows, so a row block never straddles two sequences
// and a workgroup of the extend kernel reads its entry, then its sequence's first packed row and nq_b, and is from there on the
// uniform build with nq_b for Nq.  All of these are wave-uniform (readfirstlane): the resources stay in SGPRs.  Outputs, lse and the
// partials are indexed by packed row.  The RAGGED = false builds are the code they were (DESIGN.md "Ragged").
//
// Sliding window (the WINDOW builds of the split and extend kernels; include/flash_attn_mi355x_decode_window.h): a causal call in
// which the query at position p admits the W keys p - W < j <= p.  A workgroup's key range starts at its row block's lowest window
// EDGE (the lowest key its first row admits, clamped to 0) rounded down to a super tile, split s covers [lo + s * chunk,
// lo + (s + 1) * chunk), and the host sizes the splits on the W + block + 127 keys a block can need instead of on Ncap: the work and
// the HBM traffic follow the window, not the cache.  lo is a multiple of 128, so a super tile still lies inside one page and the
// staging, the LDS image and the order of the products on the admitted keys are those of the other builds.  No tile wholly below
// the edge is loaded; the rows below it in the first tile are zeroed in the staging registers (they may hold anything: a released
// page); a wave skips a 32-key sub-tile wholly below its rows' lowest edge and masks per element only where a sub-tile straddles
// an edge.  Everything is wave-uniform and derived from len on the device.  The WINDOW = false builds are the code they were
// (DESIGN.md "Window").
//
// Attention sinks (decode_split_sink_kernel, extend_split_sink_kernel; include/flash_attn_mi355x_decode_sink.h): a windowed call in
// which every query also admits the first S positions, j < S.  A row block's key range is two ranges walked as one loop in ascending
// key order: the super tiles 0 .. vs - 128 that hold a sink key and lie wholly below lo (vs = min(S rounded up to a tile, lo)), then
// the window's tiles from lo on; a tile at or above lo that holds keys below S admits them through the mask, so no key counts
// twice.  The splits cut the virtual axis on which the two ranges are adjacent (sink_chunk), so they stay balanced wherever the
// jump from vs to lo falls; a paged walk re-initialises at lo and reads no table entry in between.  The staged rows S <= j < wedge
// become zeros (zero_rows: the tail of the last sink tile, the head of the first window tile).  The sink kernels share their body
// with the other builds as TEXT (fa_decode_split_body.h, fa_decode_extend_body.h), so the other builds are the code they were
// (DESIGN.md "Sinks").
//
// FP8 caches (the FP8 builds of the split, extend and combine kernels, and append_fp8_kernel; include/flash_attn_mi355x_decode_fp8.h):
// the caches hold OCP e4m3fn bytes and the real value of an element of kv head h is scale[h] * e4m3 (k_scale / v_scale, fp32 arrays
// of Hkv entries read on the device).  Every e4m3 value is a bf16 value, so a tile goes HBM -> registers as bytes and is widened to
// the bf16 LDS image on its way from the staging registers to LDS (Fp8Stager): the image, the fragments, the MFMAs, the softmax and
// the split / combine are those of the bf16 builds, which is why an fp8 call returns bit for bit what the bf16 call returns on the
// cache cast to bf16.  The scales never touch an element: k_scale[hkv] multiplies tau once per workgroup (the exp2 constant, the
// lse, the combine kernel's weights), v_scale[hkv] multiplies the final 1 / l (the one-split store and the combine kernel); the
// partials in the workspace stay unscaled.  bf16 queries only, no window, no ragged form.  The FP8 = false builds are the code
// they were (DESIGN.md "FP8 cache").
//
// Logit soft-capping (decode_split_softcap_kernel, extend_split_softcap_kernel; include/flash_attn_mi355x_decode_softcap.h): every
// score becomes z = softcap * tanh(tau * s / softcap) right after the QK products and BEFORE the -inf masks (cap_score below; a mask
// applied first would come out of the cap as -softcap, an admitted key).  From there on the scores are the logits: the softmax runs
// with tau = 1, m_run and the partial m are in capped-logit units, lse = m + ln l, and the host hands the EXISTING combine kernels
// tau = 1.  Key ranges, staging, page walk, window edges and the P.V products are the body's as they are.  No sinks and no fp8
// cache beside a cap.  The softcap kernels share their body with the other builds as text, as the sink kernels do, so the other
// builds are the code they were (DESIGN.md "Softcap").
//
// Learned sink logits (decode_split_lsink_kernel, extend_split_lsink_kernel, decode_combine_lsink_kernel;
// include/flash_attn_mi355x_decode_lsink.h): gpt-oss's one fp32 logit per QUERY head, a column of every row's softmax that has no
// value vector: lse = ln(e^a + sum_j e^z_j), P_j = e^(z_j - lse), out = P . V.  The logit is not scaled by tau and no mask touches
// it.  Key ranges, staging, the online softmax and the partials are the body's as they are; the logit enters where a row is
// FINISHED (lsink_finish): the one-split store of the split kernels, or the combine kernel behind its reduction, so it counts once
// however many splits a row has, and the workspace holds what it held.  The array is read on the device at that point, one load
// per row.  No sink tokens, no cap and no fp8 cache beside it.  Body shared as text, as above (DESIGN.md "Learned sinks").
#pragma once
#include "fa_common.h"

namespace fa {

constexpr int DEC_ROWS = 128;   // keys per super tile: 32 per wave

struct DecodeArgs {
  const void* q;
  const void* k;
  const void* v;
  float* out;          // final output (nsplit == 1) in q's layout
  float* lse;          // [BH][Nq], may be null
  float* part_o;       // [BH][nsplit][Nq][D] unnormalised partial O (nsplit > 1)
  float* part_ml;      // [BH][nsplit][Nq][2] partial (m, l), m in raw score units
  const int* seqlens;  // [B] or null (= Ncap)
  int H, Hkv, G, Nq, Ncap, nsplit, chunk, nqb, items;   // H = G * Hkv query heads; nqb row blocks per kv head; items = B * Hkv * nsplit
  float inv_G;         // 1.0f / G (row_query)
  int q_ld, kv_ld;     // elements between consecutive rows of one head (D or H*D for q, D or Hkv*D for the cache)
  long q_bstride, q_hstride, kv_bstride, kv_hstride;
  int causal;
  float tau;
  // paged builds only (a pool of pages and a block table instead of one slab per batch element; Ncap = max_pages * page_size)
  const int* table;    // [B][max_pages] page ids
  int page_size, num_pages, max_pages;   // rows per page (a multiple of DEC_ROWS), pages in the pool, table entries per batch element
  int window;          // window builds only: W >= 1 (in the four bytes that padded page_stride: no other field moves)
  long page_stride;    // elements between consecutive pages: page_size * Hkv * D
};

// The argument of the ragged builds (a type of its own: the other builds keep the kernel argument they had).  Nq = ntok: the combine
// kernel sees one batch element of ntok queries; nqb = entries of the block map; items = Hkv * nsplit; q is token-major: q_ld =
// H * D, q_hstride = D.
struct RaggedArgs : DecodeArgs {
  const int* cu;       // [nseq + 1] boundaries of the sequences in the packed buffers
  const int* map;      // [nqb][2] (sequence or -1: unused, row block within the sequence), written by ragged_schedule_kernel
  int nseq, ntok;      // sequences; rows of the packed buffers
};
// The argument of the FP8 builds, as RaggedArgs: the two per-kv-head scales (null: all ones).
struct Fp8Args : DecodeArgs {
  const float* k_scale;   // [Hkv] or null
  const float* v_scale;   // [Hkv] or null
};
// The arguments of the SINK builds, likewise: S, the number of leading positions every later query keeps (1 <= S < Ncap).
struct SinkArgs : DecodeArgs {
  int sink;
};
struct RaggedSinkArgs : RaggedArgs {
  int sink;
};
template <bool RAGGED> using SinkArgsOf = typename std::conditional<RAGGED, RaggedSinkArgs, SinkArgs>::type;
// The arguments of the SOFTCAP builds, likewise: the cap, positive and finite (the host checks it).
struct SoftcapArgs : DecodeArgs {
  float softcap;
};
struct RaggedSoftcapArgs : RaggedArgs {
  float softcap;
};
template <bool RAGGED> using SoftcapArgsOf = typename std::conditional<RAGGED, RaggedSoftcapArgs, SoftcapArgs>::type;
// The arguments of the LSINK builds, likewise: one learned logit per QUERY head, fp32 [H], read on the device (never null here: the
// host sends a call without them to the other builds).
struct LsinkArgs : DecodeArgs {
  const float* sink_logits;
};
struct RaggedLsinkArgs : RaggedArgs {
  const float* sink_logits;
};
template <bool RAGGED> using LsinkArgsOf = typename std::conditional<RAGGED, RaggedLsinkArgs, LsinkArgs>::type;
template <bool RAGGED, bool FP8 = false>
using DecodeArgsOf = typename std::conditional<FP8, Fp8Args, typename std::conditional<RAGGED, RaggedArgs, DecodeArgs>::type>::type;
// (positive and finite is the caller's contract: the kernels do not check a scale)
FA_DEV float scale_of(const float* scale, int hkv) { return scale ? scale[hkv] : 1.0f; }

// (Soft-capping: cap_score and cap_k2 are in fa_common.h, which the training kernels of fa_window.h share.)

// (Learned sink logits: lsink_finish, the end of a row, is in fa_common.h, which the training forward of fa_window.h shares.)

FA_DEV int clamp_len(const int* seqlens, int Ncap, int b) {
  const int len = seqlens ? seqlens[b] : Ncap;
  return min(max(len, 0), Ncap);
}

FA_DEV int clamp_len(const DecodeArgs& a, int b) { return clamp_len(a.seqlens, a.Ncap, b); }

// (Ragged: seq_rows, which packed rows a sequence owns, is in fa_common.h, which the packed training libraries share.)

// rho / G for a row index 0 <= rho < 2^25 without the integer division's long dependent chain in front of the workgroup's first
// loads: the float quotient is off by at most one, which the remainder corrects.  (G = 1: exact at once.)
FA_DEV int row_query(const DecodeArgs& a, int rho) {
  int qi = (int)(((float)rho + 0.5f) * a.inv_G);
  const int rem = rho - qi * a.G;
  qi += (rem >= a.G) - (rem < 0);
  return qi;
}

// Row n of the loader's matrix at byte voffset n*ldb: TileStager's (row, chunk) map and LDS image, with the tile's row offset added to
// the voffset instead of the scalar offset, so that the resource's range check covers it.
template <typename S> FA_DEV void load_rows(S& st, rsrc_t rs, int row0) {
#pragma unroll
  for (int i = 0; i < S::PER; ++i) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if (S::NCH % 256 == 0 || st.live)
      v = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, st.voff + (row0 + i * S::RSTEP) * st.ldb, 0, 0));
    st.regs[i] = v;
  }
}

// Window builds: the first tile of a block's key range starts up to 127 rows below the block's window edge.  No row of the block
// admits those keys, and they may hold anything (NaN included: P = 0 times a NaN of V is a NaN), so they become zeros in the staging
// registers, as the hardware makes the rows at or past len.  n: the rows of the staged tile below the edge.  (A thread's first row
// is voff / ldb: voff = row * ldb + a column offset below ldb.  Once per workgroup, in front of its tile loop.)
template <typename S> FA_DEV void zero_below(S& st, int n) {
  const int row = st.voff / st.ldb;
#pragma unroll
  for (int i = 0; i < S::PER; ++i)
    if (row + i * S::RSTEP < n) st.regs[i] = u32x4{0u, 0u, 0u, 0u};
}

// Sink builds: the range form.  The staged rows n0 <= row < n1 become zeros (n0 may be negative, n1 past the tile): the rows at or
// past the last sink key and below the block's window edge, in the last sink tile and in the first tile of the window's range.
template <typename S> FA_DEV void zero_rows(S& st, int n0, int n1) {
  const int row = st.voff / st.ldb;
#pragma unroll
  for (int i = 0; i < S::PER; ++i)
    if (row + i * S::RSTEP >= n0 && row + i * S::RSTEP < n1) st.regs[i] = u32x4{0u, 0u, 0u, 0u};
}

// FP8 builds: TileStager<bf16_t, D, DEC_ROWS, 256> for rows of one byte per element.  The thread -> (row, 16-byte bf16 chunk) map and
// lds_off are that stager's own (init runs it and halves its byte offsets: row * ld + 8 * ch); a chunk is loaded as the 8 cache
// bytes that become it, stays 8 bytes until store, and is widened there: v_cvt_scalef32_pk_bf16_fp8 with a scale of 1, one
// instruction per pair of elements, exact for all 256 codes (every e4m3 value is a bf16 value; both NaN codes give a bf16 NaN).
template <int D> struct Fp8Stager {
  using B16 = TileStager<bf16_t, D, DEC_ROWS, 256>;
  static constexpr int NCH = B16::NCH, PER = B16::PER, RSTEP = B16::RSTEP;
  static_assert(NCH % 256 == 0, "every thread has a chunk");
  typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
  u32x2 regs[PER];
  int voff, lds_off, ldb;   // as TileStager's, in cache bytes
  static constexpr bool live = true;
  FA_DEV void init(int tid, int ld) {
    B16 b;
    b.init(tid, ld);
    voff = b.voff >> 1;
    lds_off = b.lds_off;
    ldb = ld;
  }
  FA_DEV void store(lds_char* tile) const {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const u32x4 w = {__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(regs[i][0], 1.0f, false)),
                       __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(regs[i][0], 1.0f, true)),
                       __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(regs[i][1], 1.0f, false)),
                       __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(regs[i][1], 1.0f, true))};
      *FA_LDS(u32x4, tile + lds_off + Atom<bf16_t>::template off<D>(i * RSTEP, 0)) = w;
    }
  }
};

// load_rows for the byte rows of an fp8 cache: 8 bytes per chunk, the same row offsets under the resource's range check
template <int D> FA_DEV void load_rows(Fp8Stager<D>& st, rsrc_t rs, int row0) {
#pragma unroll
  for (int i = 0; i < Fp8Stager<D>::PER; ++i)
    st.regs[i] = __builtin_bit_cast(typename Fp8Stager<D>::u32x2,
                                    __builtin_amdgcn_raw_buffer_load_b64(rs, st.voff + (row0 + i * Fp8Stager<D>::RSTEP) * st.ldb, 0, 0));
}

// Paged cache: logical row j of batch element b is row j % page_size of page table[b][j / page_size].  page_size is a multiple of
// DEC_ROWS and every chunk starts on a multiple of it, so a super tile lies inside one page: the tile at logical row t0 goes through
// a resource of its page's (kv head) slice sized to the page's valid rows, min(page_size, len - page start), with the tile's row
// inside the page in the voffset, exactly as load_rows does for the slab.  Rows at or past len_b read as zero as before, and a page
// id is clamped to the pool, so no access leaves it whatever the table holds.  (slot, off) walk forward by additions; the id of the
// tile after the one being loaded is fetched a tile ahead, so the table's latency sits under a tile's products.  Everything here is
// wave-uniform: the table is read through a workgroup-uniform index and the id passes readfirstlane, so the resources stay in SGPRs.
struct PageWalk {
  const int* row;   // the table row of this batch element
  int slot, off;    // of the next tile to load: its entry in the row and its first row inside that page
  int next;         // that tile's page id (clamped)
  FA_DEV int id(const DecodeArgs& a) const { return __builtin_amdgcn_readfirstlane(min(max(row[slot], 0), a.num_pages - 1)); }
  // t0: the first tile of the workgroup's chunk
  FA_DEV void init(const DecodeArgs& a, int b, int t0) {
    row = a.table + (size_t)b * a.max_pages;
    slot = t0 / a.page_size;
    off = t0 - slot * a.page_size;
    next = id(a);
  }
  // loads the tile at (slot, off) and steps to the one after it, fetching its id if there is one (more); T: the CACHE's element
  template <typename T, int D, typename S> FA_DEV void load(const DecodeArgs& a, S& sk, S& sv, size_t hoff, int len, bool more) {
    const int rows = min(a.page_size, len - slot * a.page_size);
    const uint32_t bytes = ((uint32_t)(rows - 1) * a.kv_ld + D) * (uint32_t)sizeof(T);
    const size_t base = (size_t)next * a.page_stride + hoff;
    load_rows(sk, make_rsrc(reinterpret_cast<const T*>(a.k) + base, bytes), off);
    load_rows(sv, make_rsrc(reinterpret_cast<const T*>(a.v) + base, bytes), off);
    off += DEC_ROWS;
    if (off == a.page_size) {
      off = 0;
      ++slot;
    }
    if (more) next = id(a);
  }
};

// Sink builds (include/flash_attn_mi355x_decode_sink.h): a row block walks the super tiles 0 .. vs - 128 that hold a sink key and
// lie wholly below lo, the start of its window range, and then the tiles from lo on: one loop in ascending key order.
// The tile behind the one at t on that walk (t + DEC_ROWS == vs is the jump; vs == lo: the two ranges are adjacent).
FA_DEV int sink_next(int t, int vs, int lo) { return t + DEC_ROWS == vs ? lo : t + DEC_ROWS; }
// The bounds of split `split` of that walk in logical keys.  The splits cut the VIRTUAL axis on which the two ranges are adjacent
// (virtual key v is key v below vs and key v + lo - vs from there on), so they stay balanced, and a split past the end is empty.
FA_DEV void sink_chunk(int split, int chunk, int len, int vs, int lo, int& c0, int& c1) {
  const int jump = lo - vs, v0 = split * chunk, v1 = min(v0 + chunk, len - jump);
  c0 = v0 + (v0 >= vs ? jump : 0);   // (a split that starts at the jump starts at lo)
  c1 = v1 + (v1 > vs ? jump : 0);    // (one that ends at it ends at vs: c1 is never inside (vs, lo])
}
// PageWalk::load for the tile at t, which leaves the walk at sink_next(t) if that tile lies below `end`: at the jump by an init
// at lo, so that the table entries between the last sink tile's page and lo's page are never read.
template <typename C, int D, typename S>
FA_DEV void sink_load(PageWalk& pw, const DecodeArgs& a, int b, S& sk, S& sv, size_t hoff, int len, int t, int vs, int lo, int end) {
  const int t2 = sink_next(t, vs, lo);
  const bool more = t2 < end, jump = t2 != t + DEC_ROWS;
  pw.template load<C, D>(a, sk, sv, hoff, len, more && !jump);
  if (more && jump) pw.init(a, b, t2);
}

// GROUPED = false is the G = 1 build: rho = i with no row arithmetic in front of the workgroup's first loads (a workgroup lives for a
// few super tiles, so its prologue is not free: DESIGN.md "Decode").  PAGED: the cache is a pool read through a block table (PageWalk).
// WINDOW: a sliding window of a.window keys (causal).  The key range belongs to the 32-row BLOCK, not to the call: wedge is the
// lowest key the block's first row admits, so every block walks about W + 32 + 127 keys whatever Nq.
// FP8: the caches hold e4m3 bytes (C, the cache's element type, is a byte) and a carries the two scales; T, the queries' type and
// the type of the LDS image, is bf16.  tau8 = tau * k_scale[hkv] stands for tau wherever the kernel uses it.
// SINK (with WINDOW; a.sink = S): the first S positions stay admitted beside the window; the key range becomes the sink tiles, then
// the window's (above).  The sink builds are kernels of their own, decode_split_sink_kernel below, with the same body: it is
// fa_decode_split_body.h, included as text in both (that file says why it is not a function).
template <typename T, int D, bool GROUPED, bool PAGED = false, bool WINDOW = false, bool FP8 = false>
__global__ void __launch_bounds__(256) decode_split_kernel(DecodeArgsOf<false, FP8> a) {
  constexpr bool SINK = false;
  constexpr bool SOFTCAP = false;
  constexpr bool LSINK = false;
#include "fa_decode_split_body.h"
}

// The SINK builds: grouped and windowed, slab or paged.  (The argument is SinkArgs, spelled as a type that depends on a template
// parameter: the body's FP8 statements name fields it does not have, and are discarded unchecked only under a dependent type.)
template <typename T, int D, bool PAGED>
__global__ void __launch_bounds__(256) decode_split_sink_kernel(SinkArgsOf<PAGED && false> a) {
  constexpr bool GROUPED = true, WINDOW = true, FP8 = false, SINK = true;
  constexpr bool SOFTCAP = false;
  constexpr bool LSINK = false;
#include "fa_decode_split_body.h"
}

// The SOFTCAP builds (a.softcap: the cap): grouped, slab or paged, windowed or not.  (The argument's type depends on a template
// parameter for the reason above.)
template <typename T, int D, bool PAGED, bool WINDOW>
__global__ void __launch_bounds__(256) decode_split_softcap_kernel(SoftcapArgsOf<PAGED && false> a) {
  constexpr bool GROUPED = true, FP8 = false, SINK = false, SOFTCAP = true;
  constexpr bool LSINK = false;
#include "fa_decode_split_body.h"
}

// The LSINK builds (a.sink_logits: one learned logit per query head): grouped, slab or paged, windowed or not.  They differ from
// the other builds in the one-split store alone (lsink_finish); a partial in the workspace is the other builds' partial.
template <typename T, int D, bool PAGED, bool WINDOW>
__global__ void __launch_bounds__(256) decode_split_lsink_kernel(LsinkArgsOf<PAGED && false> a) {
  constexpr bool GROUPED = true, FP8 = false, SINK = false, SOFTCAP = false, LSINK = true;
#include "fa_decode_split_body.h"
}

// ---- extend: any number of new queries against the cache ---------------------------------------------------------------------------
// The split kernel's semantics for any Nq >= 1 with the roles of its waves swapped: a workgroup = one (batch*kv head, key chunk,
// 128-ROW block), wave w owns rows 128 * qb + 32 * w .. + 31 (its own Q fragments, acc_o, m_run, l_run), the four waves stage the
// 128-key super tiles together as above, and every wave walks all four 32-key sub-tiles of a staged tile for its own rows.  A staged
// tile serves 128 rows instead of 32 and there is no cross-wave merge: each wave writes its 32 rows, final (one split) or as a
// partial in the layout decode_combine_kernel reads.  DecodeArgs as above with nqb = ceil(G * Nq / 128).
// Causal: the workgroup's key loop ends at the block's highest position + 1 (workgroup-uniform: every wave reaches every barrier, and
// no tile is loaded that no row of the block can see); inside it a wave skips the sub-tiles wholly above its own pos_hi and masks
// only those that straddle pos_lo .. pos_hi.  A wave whose rows are all >= G * Nq stages, meets the barriers and stores nothing.
constexpr int EXT_BLOCK = 128;   // rows per workgroup: 32 per wave

// RAGGED: the row block is entry `slot % nqb` of the block map, which names its sequence b and its block qb within b's G * nq_b
// rows; the items are (kv head, split) alone.  nq_ below is nq_b, row0 the sequence's first packed row.
// WINDOW: a sliding window of a.window keys (causal).  wedge, the lowest key the 128-row block's first row admits, is to the
// start of the block's key range what blk_hi is to its end: a block walks about W + 128 + 127 keys wherever it sits in a long
// input.  Each wave then skips and masks by its own 32 rows' edges.
// FP8: as in decode_split_kernel (C: a byte; tau8 for tau; v_scale on the final 1 / l).
// SINK: as in decode_split_kernel, per 128-row block; the body is fa_decode_extend_body.h, included as text in both kernels.
template <typename T, int D, bool PAGED = false, bool RAGGED = false, bool WINDOW = false, bool FP8 = false>
__global__ void __launch_bounds__(256) extend_split_kernel(DecodeArgsOf<RAGGED, FP8> a) {
  constexpr bool SINK = false;
  constexpr bool SOFTCAP = false;
  constexpr bool LSINK = false;
#include "fa_decode_extend_body.h"
}

// The SINK builds: windowed, slab or paged, uniform or ragged.
template <typename T, int D, bool PAGED, bool RAGGED>
__global__ void __launch_bounds__(256) extend_split_sink_kernel(SinkArgsOf<RAGGED> a) {
  constexpr bool WINDOW = true, FP8 = false, SINK = true;
  constexpr bool SOFTCAP = false;
  constexpr bool LSINK = false;
#include "fa_decode_extend_body.h"
}

// The SOFTCAP builds: slab or paged, uniform or ragged, windowed or not.
template <typename T, int D, bool PAGED, bool RAGGED, bool WINDOW>
__global__ void __launch_bounds__(256) extend_split_softcap_kernel(SoftcapArgsOf<RAGGED> a) {
  constexpr bool FP8 = false, SINK = false, SOFTCAP = true;
  constexpr bool LSINK = false;
#include "fa_decode_extend_body.h"
}

// The LSINK builds: slab or paged, uniform or ragged, windowed or not (as in decode_split_lsink_kernel: the one-split store).
template <typename T, int D, bool PAGED, bool RAGGED, bool WINDOW>
__global__ void __launch_bounds__(256) extend_split_lsink_kernel(LsinkArgsOf<RAGGED> a) {
  constexpr bool FP8 = false, SINK = false, SOFTCAP = false, LSINK = true;
#include "fa_decode_extend_body.h"
}

// out[row] = sum_s O_s 2^(c (m_s - M)) / sum_s l_s 2^(c (m_s - M)), M = max_s m_s.  A workgroup = one (bh, row): thread (g, j) takes
// columns 4g .. 4g+3 of the splits j, j + S, j + 2S, ... and the S partial sums of a column group are added in the order j = 0 .. S-1
// (a fixed order: bitwise repeatable).
// RAGGED: one batch element of Nq = ntok packed rows; a row in front of the first sequence or behind the last one (the unused tail
// of the packed buffers) has no partials and is neither read nor written.  (A cu that is not non-decreasing can make an earlier
// sequence end past the last one's end: its rows there are then left as they were, where a one-split call writes them.)
// FP8: the row's kv head is hd / a.G; its k_scale multiplies tau (the weights and the lse), its v_scale the final 1 / l.
template <int D, bool RAGGED = false, bool FP8 = false>
__global__ void __launch_bounds__(256) decode_combine_kernel(DecodeArgsOf<RAGGED, FP8> a) {
  constexpr bool LSINK = false;
#include "fa_decode_combine_body.h"
}

// The LSINK build of the combine kernel (uniform and ragged): the partials are the other builds' (unnormalised, without the logit),
// and the row's sink column joins once, behind the reduction (lsink_finish).  The body is fa_decode_combine_body.h, included as
// text in both kernels.
template <int D, bool RAGGED>
__global__ void __launch_bounds__(256) decode_combine_lsink_kernel(LsinkArgsOf<RAGGED> a) {
  constexpr bool FP8 = false, LSINK = true;
#include "fa_decode_combine_body.h"
}

// ---- ragged: the block map -------------------------------------------------------------------------------------------------------
// One workgroup turns cu into the block map of the ragged extend kernel: for b = 0, 1, ... in order, one entry (b, qb) for each of
// the ceil(G * nq_b / 128) row blocks of sequence b (none for nq_b = 0), then (-1, 0) up to the map's `cap` entries.  For a cu that
// is non-decreasing the blocks number at most floor(G * ntok / 128) + min(nseq, ntok) = cap (every non-empty sequence rounds up at
// most once); for any other cu the counts saturate at cap and the entries past it are dropped, so the map is never overrun.
// Thread t takes the sequences t * per .. t * per + per - 1: its block count, an exclusive prefix over the 256 counts in LDS, then
// its entries.  Integer work in a fixed order: the map is a function of cu alone.  The map is written as int pairs (8 bytes) at the
// workspace's base and the partials behind it as 16-byte vectors: the workspace is 16-byte aligned (the header says so).
__global__ void __launch_bounds__(256) ragged_schedule_kernel(const int* cu, int* map, int nseq, int ntok, int G, int cap) {
  __shared__ int counts[256];
  const int tid = threadIdx.x;
  const int per = (int)(((long)nseq + 255) / 256);
  const int b0 = (int)min((long)tid * per, (long)nseq), b1 = (int)min((long)b0 + per, (long)nseq);
  int n = 0;
  for (int b = b0; b < b1; ++b) {
    int s, nq;
    seq_rows(cu, ntok, b, s, nq);
    n = min(n + (G * nq + EXT_BLOCK - 1) / EXT_BLOCK, cap);
  }
  counts[tid] = n;
  __syncthreads();
  int off = 0, total = 0;
  for (int u = 0; u < 256; ++u) {
    if (u == tid) off = total;
    total = min(total + counts[u], cap);
  }
  for (int b = b0; b < b1; ++b) {
    int s, nq;
    seq_rows(cu, ntok, b, s, nq);
    const int nb = (G * nq + EXT_BLOCK - 1) / EXT_BLOCK;
    for (int qb = 0; qb < nb && off < cap; ++qb, ++off) *reinterpret_cast<int2*>(map + 2 * (size_t)off) = make_int2(b, qb);
  }
  for (int i = total + tid; i < cap; i += 256) *reinterpret_cast<int2*>(map + 2 * (size_t)i) = make_int2(-1, 0);
}

// ---- append: the new tokens' k and v into the caches ------------------------------------------------------------------------------
// k_new / v_new hold rows of d_new <= D elements, [B][Nq][Hkv] (bnhd) or [B][Hkv][Nq] of them, contiguous.  With L_b = len_b clamped
// to [0, Ncap] (the length COUNTS the new tokens, as the split kernel reads it), token i goes to cache row L_b - Nq + i: the position
// the causal mask gives query i, so a key always lands on its own query's position.  Rows below 0 (len_b < Nq) are not written; no
// row reaches Ncap.  Columns d_new .. D-1 of a written row are set to zero: the caller neither pads nor keeps stale columns clean.
struct AppendArgs {
  const void* k_new;
  const void* v_new;
  void* k;
  void* v;
  const int* seqlens;   // [B] or null (= Ncap)
  long lanes;           // B * Nq * Hkv * (D / E)
  int Hkv, Nq, Ncap, d_new, bnhd;
  int ch_shift;         // log2(D / E): lanes per row
  int kv_ld;            // elements between consecutive rows of one head of the cache (D or Hkv*D)
  long kv_bstride, kv_hstride;
  // paged builds only, as in DecodeArgs (Ncap = max_pages * page_size)
  const int* table;
  int page_size, num_pages, max_pages;
  long page_stride;
};

// The argument of the ragged builds, as RaggedArgs: k_new / v_new are [ntok][Hkv][d_new] and lanes = ntok * Hkv * (D / E).
struct RaggedAppendArgs : AppendArgs {
  const int* cu;
  int nseq, ntok;
};

// A lane = E consecutive elements of one new row, of K and of V: E = 16 bytes' worth (one vector load and store each; the host picks
// it when d_new * sizeof(T) is a multiple of 16 and all four pointers are 16-byte aligned) or E = 1.  Consecutive lanes walk the
// source in memory order.  The elements are copied as bits; the cache's row length D (a power of two) is a run-time argument.
// PAGED: row pos is row pos % page_size of page table[b][pos / page_size], the id clamped to the pool as the split kernels do.
// RAGGED: the source is packed, row (t, hkv); the lane finds the sequence that owns packed row t by a binary search of cu (the first
// b whose clamped end is above t) and places token i = t - s_b of nq_b as above.  A row that no sequence owns (in front of the first
// one, or the unused tail) is not copied.
template <typename T, int E, bool PAGED = false, bool RAGGED = false>
__global__ void __launch_bounds__(256) decode_append_kernel(typename std::conditional<RAGGED, RaggedAppendArgs, AppendArgs>::type a) {
  typedef typename std::conditional<sizeof(T) == 2, uint16_t, uint32_t>::type U;
  typedef __attribute__((ext_vector_type(E))) U vec;
  static_assert(E == 1 || E * sizeof(T) == 16, "a lane moves one element or 16 bytes");
  const long lane = (long)blockIdx.x * 256 + threadIdx.x;
  if (lane >= a.lanes) return;
  const long row = lane >> a.ch_shift;           // source row (b, i, hkv) or (b, hkv, i)
  const int col = (int)(lane - (row << a.ch_shift)) * E;
  int b_, i_, hkv_, nq_ = a.Nq;
  if constexpr (RAGGED) {
    const int t = (int)(row / a.Hkv);
    hkv_ = (int)(row - (long)t * a.Hkv);
    int lo = 0, hi = a.nseq;   // the first b in [0, nseq) with clamp(cu[b + 1]) > t, or nseq: none
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (min(max(a.cu[mid + 1], 0), a.ntok) > t) hi = mid; else lo = mid + 1;
    }
    if (lo == a.nseq) return;
    int s;
    seq_rows(a.cu, a.ntok, lo, s, nq_);
    if (t < s || t >= s + nq_) return;
    b_ = lo;
    i_ = t - s;
  } else {
    const int inner = a.bnhd ? a.Hkv : a.Nq;
    const long outer = row / inner;
    const int in = (int)(row - outer * inner);
    const int mid = a.bnhd ? a.Nq : a.Hkv;
    b_ = (int)(outer / mid);
    const int md = (int)(outer - (long)b_ * mid);
    i_ = a.bnhd ? md : in;
    hkv_ = a.bnhd ? in : md;
  }
  const int b = b_, i = i_, hkv = hkv_;
  const int pos = clamp_len(a.seqlens, a.Ncap, b) - nq_ + i;
  if (pos < 0) return;
  const size_t src = (size_t)row * a.d_new + col;
  size_t dst;
  if constexpr (PAGED) {
    const int slot = pos / a.page_size;
    const int page = min(max(a.table[(size_t)b * a.max_pages + slot], 0), a.num_pages - 1);
    dst = (size_t)page * a.page_stride + (size_t)hkv * a.kv_hstride + (size_t)(pos - slot * a.page_size) * a.kv_ld + col;
  } else {
    dst = (size_t)b * a.kv_bstride + (size_t)hkv * a.kv_hstride + (size_t)pos * a.kv_ld + col;
  }
  vec kk = {}, vv = {};
  if (col < a.d_new) {   // (E > 1: d_new is a multiple of E, so the whole lane is inside the row)
    kk = *reinterpret_cast<const vec*>(reinterpret_cast<const U*>(a.k_new) + src);
    vv = *reinterpret_cast<const vec*>(reinterpret_cast<const U*>(a.v_new) + src);
  }
  *reinterpret_cast<vec*>(reinterpret_cast<U*>(a.k) + dst) = kk;
  *reinterpret_cast<vec*>(reinterpret_cast<U*>(a.v) + dst) = vv;
}

// ---- append into an fp8 cache: quantise on the way -----------------------------------------------------------------------------
// The uniform append above for bf16 sources and caches of e4m3 bytes: the same placement (row L_b - Nq + i, nothing below row 0, the
// paged lookup with clamped ids), zero BYTES in columns d_new .. D-1, and for an element x of kv head h
//     code = rne_e4m3(clamp(fp32(x) * (1.0f / scale[h]), -448, 448))
// with the reciprocal and the product each correctly rounded in fp32 (an IEEE division: the build has no fast-math).  The clamp
// sits in front of the conversion, so overflow saturates to +-448 (0x7E / 0xFE) and never reaches the NaN code; a NaN input stores
// 0x7F.  v_cvt_pk_fp8_f32 rounds to nearest even, denormals included.
struct Fp8AppendArgs : AppendArgs {
  const float* k_scale;   // [Hkv] or null (all ones)
  const float* v_scale;
};

FA_DEV float fp8_prescale(float x, float rcp) {
  return (x != x) ? x : __builtin_fminf(__builtin_fmaxf(x * rcp, -448.0f), 448.0f);   // (a NaN stays one: min / max would drop it)
}
// two elements -> two codes in the low (hi = false) or high half of `old`
FA_DEV uint32_t fp8_pack2(float x0, float x1, float rcp, uint32_t old, bool hi) {
  const float p0 = fp8_prescale(x0, rcp), p1 = fp8_prescale(x1, rcp);
  uint32_t w = hi ? (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(p0, p1, (int)old, true)
                  : (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(p0, p1, (int)old, false);
  const int sh = hi ? 16 : 0;   // (the conversion gives a NaN the code 0xFF: the format's canonical NaN byte is stored instead)
  if (p0 != p0) w = (w & ~(0xffu << sh)) | (0x7fu << sh);
  if (p1 != p1) w = (w & ~(0xff00u << sh)) | (0x7f00u << sh);
  return w;
}

// A lane = E consecutive elements of one new row, of K and of V: E = 8 (one 16-byte load and one 8-byte store each; the host picks it
// when d_new is a multiple of 8, the sources are 16-byte aligned and the caches 8-byte aligned) or E = 1.
template <int E, bool PAGED = false>
__global__ void __launch_bounds__(256) append_fp8_kernel(Fp8AppendArgs a) {
  static_assert(E == 1 || E == 8, "a lane moves one element or eight");
  const long lane = (long)blockIdx.x * 256 + threadIdx.x;
  if (lane >= a.lanes) return;
  const long row = lane >> a.ch_shift;           // source row (b, i, hkv) or (b, hkv, i)
  const int col = (int)(lane - (row << a.ch_shift)) * E;
  const int inner = a.bnhd ? a.Hkv : a.Nq;
  const long outer = row / inner;
  const int in = (int)(row - outer * inner);
  const int mid = a.bnhd ? a.Nq : a.Hkv;
  const int b = (int)(outer / mid);
  const int md = (int)(outer - (long)b * mid);
  const int i = a.bnhd ? md : in, hkv = a.bnhd ? in : md;
  const int pos = clamp_len(a.seqlens, a.Ncap, b) - a.Nq + i;
  if (pos < 0) return;
  const size_t src = (size_t)row * a.d_new + col;
  size_t dst;
  if constexpr (PAGED) {
    const int slot = pos / a.page_size;
    const int page = min(max(a.table[(size_t)b * a.max_pages + slot], 0), a.num_pages - 1);
    dst = (size_t)page * a.page_stride + (size_t)hkv * a.kv_hstride + (size_t)(pos - slot * a.page_size) * a.kv_ld + col;
  } else {
    dst = (size_t)b * a.kv_bstride + (size_t)hkv * a.kv_hstride + (size_t)pos * a.kv_ld + col;
  }
  const float rk = 1.0f / scale_of(a.k_scale, hkv), rv = 1.0f / scale_of(a.v_scale, hkv);
  uint8_t* kd = reinterpret_cast<uint8_t*>(a.k) + dst;
  uint8_t* vd = reinterpret_cast<uint8_t*>(a.v) + dst;
  if constexpr (E == 8) {
    typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
    u32x2 kk = {0u, 0u}, vv = {0u, 0u};
    if (col < a.d_new) {   // (d_new is a multiple of 8, so the whole lane is inside the row)
      const bf16x8 ks = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const bf16_t*>(a.k_new) + src);
      const bf16x8 vs = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const bf16_t*>(a.v_new) + src);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        kk[j] = fp8_pack2((float)ks[4 * j], (float)ks[4 * j + 1], rk, 0u, false);
        kk[j] = fp8_pack2((float)ks[4 * j + 2], (float)ks[4 * j + 3], rk, kk[j], true);
        vv[j] = fp8_pack2((float)vs[4 * j], (float)vs[4 * j + 1], rv, 0u, false);
        vv[j] = fp8_pack2((float)vs[4 * j + 2], (float)vs[4 * j + 3], rv, vv[j], true);
      }
    }
    *reinterpret_cast<u32x2*>(kd) = kk;
    *reinterpret_cast<u32x2*>(vd) = vv;
  } else {
    uint8_t kk = 0, vv = 0;
    if (col < a.d_new) {
      const float xk = (float)reinterpret_cast<const bf16_t*>(a.k_new)[src], xv = (float)reinterpret_cast<const bf16_t*>(a.v_new)[src];
      kk = (uint8_t)fp8_pack2(xk, xk, rk, 0u, false);
      vv = (uint8_t)fp8_pack2(xv, xv, rv, 0u, false);
    }
    *kd = kk;
    *vd = vv;
  }
}

}  // namespace fa
