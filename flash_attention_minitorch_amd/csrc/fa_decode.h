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
// FP8 caches (the FP8 builds of the split, extend and combine kernels, and append_fp8_kernel; include/flash_attn_mi355x_decode_fp8.h):
// the caches hold OCP e4m3fn bytes and the real value of an element of kv head h is scale[h] * e4m3 (k_scale / v_scale, fp32 arrays
// of Hkv entries read on the device).  Every e4m3 value is a bf16 value, so a tile goes HBM -> registers as bytes and is widened to
// the bf16 LDS image on its way from the staging registers to LDS (Fp8Stager): the image, the fragments, the MFMAs, the softmax and
// the split / combine are those of the bf16 builds, which is why an fp8 call returns bit for bit what the bf16 call returns on the
// cache cast to bf16.  The scales never touch an element: k_scale[hkv] multiplies tau once per workgroup (the exp2 constant, the
// lse, the combine kernel's weights), v_scale[hkv] multiplies the final 1 / l (the one-split store and the combine kernel); the
// partials in the workspace stay unscaled.  bf16 queries only, no window, no ragged form.  The FP8 = false builds are the code
// they were (DESIGN.md "FP8 cache").
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
template <bool RAGGED, bool FP8 = false>
using DecodeArgsOf = typename std::conditional<FP8, Fp8Args, typename std::conditional<RAGGED, RaggedArgs, DecodeArgs>::type>::type;
// (positive and finite is the caller's contract: the kernels do not check a scale)
FA_DEV float scale_of(const float* scale, int hkv) { return scale ? scale[hkv] : 1.0f; }

FA_DEV int clamp_len(const int* seqlens, int Ncap, int b) {
  const int len = seqlens ? seqlens[b] : Ncap;
  return min(max(len, 0), Ncap);
}

FA_DEV int clamp_len(const DecodeArgs& a, int b) { return clamp_len(a.seqlens, a.Ncap, b); }

// Ragged: sequence b owns the packed rows s .. s + nq - 1, s = clamp(cu[b], 0, ntok) and s + nq = clamp(cu[b+1], s, ntok): whatever
// the array holds, no row leaves the ntok-row buffers.  nq may be 0.
FA_DEV void seq_rows(const int* cu, int ntok, int b, int& s, int& nq) {
  s = min(max(cu[b], 0), ntok);
  nq = min(max(cu[b + 1], s), ntok) - s;
}

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

// GROUPED = false is the G = 1 build: rho = i with no row arithmetic in front of the workgroup's first loads (a workgroup lives for a
// few super tiles, so its prologue is not free: DESIGN.md "Decode").  PAGED: the cache is a pool read through a block table (PageWalk).
// WINDOW: a sliding window of a.window keys (causal).  The key range belongs to the 32-row BLOCK, not to the call: wedge is the
// lowest key the block's first row admits, so every block walks about W + 32 + 127 keys whatever Nq.
// FP8: the caches hold e4m3 bytes (C, the cache's element type, is a byte) and a carries the two scales; T, the queries' type and
// the type of the LDS image, is bf16.  tau8 = tau * k_scale[hkv] stands for tau wherever the kernel uses it.
template <typename T, int D, bool GROUPED, bool PAGED = false, bool WINDOW = false, bool FP8 = false>
__global__ void __launch_bounds__(256) decode_split_kernel(DecodeArgsOf<false, FP8> a) {
  static_assert(!FP8 || (std::is_same<T, bf16_t>::value && GROUPED && !WINDOW), "fp8 caches: bf16 queries, the grouped form, no window");
  using A = Atom<T>;
  typedef typename std::conditional<FP8, uint8_t, T>::type C;
  typedef typename A::frag frag;
  constexpr int KC = D / 16, DT = D / 32;
  constexpr int TB = A::template tile_bytes<D>(DEC_ROWS);
  constexpr int PW = (16 * DT + 2) * 64 * 4;   // one wave's partial: [lane][16*DT accumulator registers, m, l]
  static_assert(3 * PW <= 2 * TB, "the partials of waves 1-3 must fit the tile images");
  __shared__ __attribute__((aligned(16))) char smem_raw[2 * TB];
  lds_char* tk = (lds_char*)smem_raw;
  lds_char* tv = tk + TB;

  // workgroup -> (item = (b * Hkv + kv head) * nsplit + split, row block): the row blocks of one item are 8 workgroup ids apart, so
  // they share an XCD's L2 under round-robin dispatch and the chunk is fetched from HBM once (speed only)
  const int id = blockIdx.x, slot = id >> 3;
  const int qb = slot % a.nqb, item = (slot / a.nqb) * 8 + (id & 7);
  if (item >= a.items) return;
  const int bh = item / a.nsplit, split = item - bh * a.nsplit;
  const int b = bh / a.Hkv, hkv = bh - b * a.Hkv;
  const int len = __builtin_amdgcn_readfirstlane(clamp_len(a, b));
  int wedge = 0;   // (window builds) the block's window edge; the key range starts at the super tile that holds it
  if constexpr (WINDOW) wedge = max(len - a.Nq + (GROUPED ? row_query(a, qb * 32) : qb * 32) - a.window + 1, 0);
  const int c0 = (WINDOW ? wedge & ~(DEC_ROWS - 1) : 0) + split * a.chunk, c1 = min(c0 + a.chunk, len);

  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the lane's row rho = qi * G + g: query qi of head hd = hkv * G + g
  const int G = GROUPED ? a.G : 1;
  const int q0 = qb * 32, rho = q0 + r, qi = GROUPED ? row_query(a, rho) : rho, hd = hkv * G + (rho - qi * G);
  const bool live = rho < G * a.Nq;
  // (a macro, as FA_NQ below: the other builds read a.tau where they always did)
  float tau8 = 0.f;
  if constexpr (FP8) tau8 = a.tau * scale_of(a.k_scale, hkv);
#define FA_TAU (FP8 ? tau8 : a.tau)
  const float c = FA_TAU * LOG2E;

  f32x16 acc_o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc_o[dt] = zero16();
  float m_run = -INFINITY, l_run = 0.f;

  if (c0 < c1) {   // (a chunk wholly past len_b loads nothing and leaves the empty partial m = -inf, l = 0)
    const size_t kvoff = (PAGED ? 0 : (size_t)b * a.kv_bstride) + (size_t)hkv * a.kv_hstride;   // (paged: inside a page)
    const uint32_t esz = sizeof(T);
    const uint32_t q_bytes = (uint32_t)a.q_bstride * esz;
    const rsrc_t qrs = make_rsrc(reinterpret_cast<const T*>(a.q) + (size_t)b * a.q_bstride, q_bytes);
    const uint32_t kv_bytes = ((uint32_t)(len - 1) * a.kv_ld + D) * (uint32_t)sizeof(C);
    const rsrc_t krs = make_rsrc(reinterpret_cast<const C*>(a.k) + kvoff, kv_bytes);   // (the slab's: unused by a paged build)
    const rsrc_t vrs = make_rsrc(reinterpret_cast<const C*>(a.v) + kvoff, kv_bytes);
    PageWalk pw;

    frag qf[KC];
    const int qoff = live ? (hd * (int)a.q_hstride + qi * a.q_ld + 8 * h) * (int)esz : (int)q_bytes;
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) qf[kc] = load_frag_buf<T>(qrs, qoff + 16 * kc * (int)esz);

    const LaneAddr ra = A::template row_addr<D>(lane);
    const LaneAddr ta = A::template tr_addr<D>(lane);
    typename std::conditional<FP8, Fp8Stager<D>, TileStager<T, D, DEC_ROWS, 256>>::type sk, sv;
    sk.init(tid, a.kv_ld);
    sv.init(tid, a.kv_ld);
    // causal: query i sits at position len - Nq + i and sees keys j <= len - Nq + i (bottom-right aligned); the block's rows span
    // the positions pos_lo .. pos_hi (wave-uniform; pos_hi may count rows past G * Nq, which only keeps a tile that masks to nothing)
    const int qpos = len - a.Nq + qi;
    const int pos_lo = len - a.Nq + (GROUPED ? row_query(a, q0) : q0), pos_hi = len - a.Nq + (GROUPED ? row_query(a, q0 + 31) : q0 + 31);
    if constexpr (PAGED) {
      pw.init(a, b, c0);
      pw.template load<C, D>(a, sk, sv, kvoff, len, c0 + DEC_ROWS < c1);
    } else {
      load_rows(sk, krs, c0);
      load_rows(sv, vrs, c0);
    }
    if constexpr (WINDOW) {
      if (c0 < wedge) {   // (split 0 of a block whose edge is inside a super tile)
        zero_below(sk, wedge - c0);
        zero_below(sv, wedge - c0);
      }
    }
    for (int t0 = c0; t0 < c1; t0 += DEC_ROWS) {
      __syncthreads();   // (the previous super tile's reads are done)
      sk.store(tk);
      sv.store(tv);
      if (t0 + DEC_ROWS < c1) {
        if constexpr (PAGED) {
          pw.template load<C, D>(a, sk, sv, kvoff, len, t0 + 2 * DEC_ROWS < c1);
        } else {
          load_rows(sk, krs, t0 + DEC_ROWS);
          load_rows(sv, vrs, t0 + DEC_ROWS);
        }
      }
      __syncthreads();
      const int kbase = t0 + 32 * w;
      if (kbase >= c1 || (a.causal && kbase > pos_hi)) continue;   // wave-uniform: no admissible key in the wave's 32
      if constexpr (WINDOW) {
        if (kbase + 31 <= pos_lo - a.window) continue;   // wave-uniform: the 32 keys are below every row's window
      }
      f32x16 s = zero16();
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) A::mma(s, A::template row_frag<D>(tk, ra, 32 * w, kc), qf[kc]);
      // (window: only the sub-tiles that hold a key at or below the highest row's edge - 1 mask for it)
      if (kbase + 32 > c1 || (a.causal && kbase + 31 > pos_lo) || (WINDOW && kbase <= pos_hi - a.window)) {   // wave-uniform
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int key = kbase + acc_row(i, h);
          if (key >= c1 || (a.causal && key > qpos) || (WINDOW && key <= qpos - a.window)) s[i] = -INFINITY;
        }
      }
      float mx = s[0];
#pragma unroll
      for (int i = 1; i < 16; ++i) mx = fmaxf(mx, s[i]);
      const float m_new = fmaxf(m_run, xhalf_max(mx));
      const float nm = (m_new == -INFINITY) ? 0.f : -m_new * c;   // (every key so far masked: any finite reference, P = 0)
      const float alpha = __builtin_amdgcn_exp2f(__builtin_fmaf(m_run, c, nm));
      float rs = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        s[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[i], c, nm));
        rs += s[i];
      }
      if (__any(alpha != 1.0f)) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
          for (int i = 0; i < 16; ++i) acc_o[dt][i] *= alpha;
      }
      l_run = l_run * alpha + rs;
      m_run = m_new;
      // bf16: P goes in at 16 significant bits (pack + pack_lo): a row with few admissible keys holds P of order 1, whose 2^-9
      // rounding would not average out (the decode step's first tokens, causal rows near position 0)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const frag p_hi = A::pack(s, s2);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const frag vt = A::template tr_frag<D>(tv, ta, 32 * w + 16 * s2, dt);
          A::mma(acc_o[dt], vt, p_hi);
          if constexpr (A::SPLITS) A::mma(acc_o[dt], vt, A::pack_lo(s, s2, p_hi));
        }
      }
    }
  }
  const float l_w = xhalf_sum(l_run);

  // the partials of waves 1-3 meet in LDS (over the tile images), wave 0 adds them in wave order
  __syncthreads();
  if (w != 0) {
    lds_char* mine = tk + (w - 1) * PW + lane * (16 * DT + 2) * 4;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int i = 0; i < 16; ++i) *FA_LDS(float, mine + (16 * dt + i) * 4) = acc_o[dt][i];
    *FA_LDS(float, mine + 16 * DT * 4) = m_run;
    *FA_LDS(float, mine + (16 * DT + 1) * 4) = l_w;
  }
  __syncthreads();
  if (w != 0) return;
  float m_all = m_run;
#pragma unroll
  for (int u = 0; u < 3; ++u) m_all = fmaxf(m_all, *FA_LDS(float, tk + u * PW + (lane * (16 * DT + 2) + 16 * DT) * 4));
  float wgt = (m_run == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f((m_run - m_all) * c);
  float l_tot = l_w * wgt;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc_o[dt][i] *= wgt;
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    lds_char* pu = tk + u * PW + lane * (16 * DT + 2) * 4;
    const float mu = *FA_LDS(float, pu + 16 * DT * 4);
    wgt = (mu == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f((mu - m_all) * c);
    l_tot += *FA_LDS(float, pu + (16 * DT + 1) * 4) * wgt;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc_o[dt][i] += *FA_LDS(float, pu + (16 * dt + i) * 4) * wgt;
  }
  if (!live) return;
  const size_t bhq = (size_t)b * a.H + hd;
  if (a.nsplit == 1) {   // final: out = O / l, lse = m * tau + ln l; a row without an admissible key: out = 0, lse = -inf
    float inv = (l_tot > 0.f) ? 1.0f / l_tot : 0.f;
    if constexpr (FP8) inv *= scale_of(a.v_scale, hkv);   // (the scale of V: once per row, on 1 / l)
    float* orow = a.out + (size_t)b * a.q_bstride + (size_t)hd * a.q_hstride + (size_t)qi * a.q_ld;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 val = {acc_o[dt][4 * g] * inv, acc_o[dt][4 * g + 1] * inv, acc_o[dt][4 * g + 2] * inv, acc_o[dt][4 * g + 3] * inv};
        *reinterpret_cast<f32x4*>(orow + 32 * dt + 8 * g + 4 * h) = val;
      }
    if (h == 0 && a.lse) a.lse[bhq * a.Nq + qi] = (l_tot > 0.f) ? m_all * FA_TAU + __logf(l_tot) : -INFINITY;
  } else {
    const size_t pr = (bhq * a.nsplit + split) * a.Nq + qi;
    float* prow = a.part_o + pr * D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 val = {acc_o[dt][4 * g], acc_o[dt][4 * g + 1], acc_o[dt][4 * g + 2], acc_o[dt][4 * g + 3]};
        *reinterpret_cast<f32x4*>(prow + 32 * dt + 8 * g + 4 * h) = val;
      }
    if (h == 0) *reinterpret_cast<f32x2*>(a.part_ml + 2 * pr) = f32x2{m_all, l_tot};
  }
}
#undef FA_TAU

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
template <typename T, int D, bool PAGED = false, bool RAGGED = false, bool WINDOW = false, bool FP8 = false>
__global__ void __launch_bounds__(256) extend_split_kernel(DecodeArgsOf<RAGGED, FP8> a) {
  static_assert(!FP8 || (std::is_same<T, bf16_t>::value && !RAGGED && !WINDOW), "fp8 caches: bf16 queries, no ragged form, no window");
  using A = Atom<T>;
  typedef typename std::conditional<FP8, uint8_t, T>::type C;
  typedef typename A::frag frag;
  constexpr int KC = D / 16, DT = D / 32;
  constexpr int TB = A::template tile_bytes<D>(DEC_ROWS);
  __shared__ __attribute__((aligned(16))) char smem_raw[2 * TB];
  lds_char* tk = (lds_char*)smem_raw;
  lds_char* tv = tk + TB;

  // workgroup -> (item, row block) as in decode_split_kernel: the row blocks of one item share an XCD's L2
  const int id = blockIdx.x, slot = id >> 3;
  const int entry = slot % a.nqb, item = (slot / a.nqb) * 8 + (id & 7);
  if (item >= a.items) return;
  const int bh = item / a.nsplit, split = item - bh * a.nsplit;
  int b_ = bh / a.Hkv, hkv_ = bh - b_ * a.Hkv, qb_ = entry, row0_ = 0, nq_ = 0;
  if constexpr (RAGGED) {
    b_ = __builtin_amdgcn_readfirstlane(a.map[2 * entry]);
    if (b_ < 0) return;   // (an unused entry: the map is sized for the worst case)
    qb_ = __builtin_amdgcn_readfirstlane(a.map[2 * entry + 1]);
    hkv_ = bh;
    seq_rows(a.cu, a.ntok, b_, row0_, nq_);
    row0_ = __builtin_amdgcn_readfirstlane(row0_);
    nq_ = __builtin_amdgcn_readfirstlane(nq_);
  }
  const int b = b_, hkv = hkv_, qb = qb_, row0 = row0_;
  // The sequence's own count, or the call's.  A macro, not a local `const int Nq`: a local reads a.Nq once at the top of the uniform
  // build, which moved two of its fp32 builds from 58 to 59 SGPRs; with a.Nq read where it always was, the uniform builds compile to
  // the code they were (DESIGN.md "Ragged").  Do not fold it into a variable without comparing the resource report.
#define FA_NQ (RAGGED ? nq_ : a.Nq)
  const int len = __builtin_amdgcn_readfirstlane(clamp_len(a, b));
  int wedge = 0;   // (window builds) the block's window edge; the key range starts at the super tile that holds it
  if constexpr (WINDOW) wedge = max(len - FA_NQ + row_query(a, qb * EXT_BLOCK) - a.window + 1, 0);
  const int c0 = (WINDOW ? wedge & ~(DEC_ROWS - 1) : 0) + split * a.chunk, c1 = min(c0 + a.chunk, len);

  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rows = a.G * FA_NQ;
  const int q0 = qb * EXT_BLOCK + 32 * w, rho = q0 + r, qi = row_query(a, rho), hd = hkv * a.G + (rho - qi * a.G);
  const bool live = rho < rows;
  const bool wave_live = q0 < rows;   // (wave-uniform)
  float tau8 = 0.f;
  if constexpr (FP8) tau8 = a.tau * scale_of(a.k_scale, hkv);
#define FA_TAU (FP8 ? tau8 : a.tau)
  const float c = FA_TAU * LOG2E;
  // causal: the last key any row of the block sees is the position of its last row (of its last REAL row: rows >= G * Nq see nothing)
  const int blk_hi = len - FA_NQ + row_query(a, min(qb * EXT_BLOCK + EXT_BLOCK, rows) - 1);
  const int cend = a.causal ? min(c1, blk_hi + 1) : c1;

  f32x16 acc_o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc_o[dt] = zero16();
  float m_run = -INFINITY, l_run = 0.f;

  if (c0 < cend) {   // (a chunk past len_b, or past every position of the block, loads nothing and leaves m = -inf, l = 0)
    const size_t kvoff = (PAGED ? 0 : (size_t)b * a.kv_bstride) + (size_t)hkv * a.kv_hstride;   // (paged: inside a page)
    const uint32_t esz = sizeof(T);
    // (ragged: the resource of the sequence's own nq_b * H * D elements of the packed q)
    const uint32_t q_bytes = RAGGED ? (uint32_t)nq_ * (uint32_t)a.q_ld * esz : (uint32_t)a.q_bstride * esz;
    const rsrc_t qrs = make_rsrc(reinterpret_cast<const T*>(a.q) + (RAGGED ? (size_t)row0 * a.q_ld : (size_t)b * a.q_bstride), q_bytes);
    const uint32_t kv_bytes = ((uint32_t)(len - 1) * a.kv_ld + D) * (uint32_t)sizeof(C);
    const rsrc_t krs = make_rsrc(reinterpret_cast<const C*>(a.k) + kvoff, kv_bytes);   // (the slab's: unused by a paged build)
    const rsrc_t vrs = make_rsrc(reinterpret_cast<const C*>(a.v) + kvoff, kv_bytes);
    PageWalk pw;

    frag qf[KC];
    const int qoff = live ? (hd * (int)a.q_hstride + qi * a.q_ld + 8 * h) * (int)esz : (int)q_bytes;
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) qf[kc] = load_frag_buf<T>(qrs, qoff + 16 * kc * (int)esz);

    const LaneAddr ra = A::template row_addr<D>(lane);
    const LaneAddr ta = A::template tr_addr<D>(lane);
    typename std::conditional<FP8, Fp8Stager<D>, TileStager<T, D, DEC_ROWS, 256>>::type sk, sv;
    sk.init(tid, a.kv_ld);
    sv.init(tid, a.kv_ld);
    // the wave's rows span the positions pos_lo .. pos_hi (wave-uniform; rows past G * Nq may push pos_hi up, which only keeps a
    // sub-tile that masks to nothing for the real rows' lanes)
    const int qpos = len - FA_NQ + qi;
    const int pos_lo = len - FA_NQ + row_query(a, q0), pos_hi = len - FA_NQ + row_query(a, q0 + 31);
    if constexpr (PAGED) {
      pw.init(a, b, c0);
      pw.template load<C, D>(a, sk, sv, kvoff, len, c0 + DEC_ROWS < cend);
    } else {
      load_rows(sk, krs, c0);
      load_rows(sv, vrs, c0);
    }
    if constexpr (WINDOW) {
      if (c0 < wedge) {   // (split 0 of a block whose edge is inside a super tile)
        zero_below(sk, wedge - c0);
        zero_below(sv, wedge - c0);
      }
    }
    for (int t0 = c0; t0 < cend; t0 += DEC_ROWS) {
      __syncthreads();   // (the previous super tile's reads are done)
      sk.store(tk);
      sv.store(tv);
      if (t0 + DEC_ROWS < cend) {
        if constexpr (PAGED) {
          pw.template load<C, D>(a, sk, sv, kvoff, len, t0 + 2 * DEC_ROWS < cend);
        } else {
          load_rows(sk, krs, t0 + DEC_ROWS);
          load_rows(sv, vrs, t0 + DEC_ROWS);
        }
      }
      __syncthreads();
      if (!wave_live) continue;
#pragma unroll
      for (int st = 0; st < DEC_ROWS / 32; ++st) {
        const int kbase = t0 + 32 * st;
        if (kbase >= cend || (a.causal && kbase > pos_hi)) break;   // wave-uniform: no admissible key here or further on
        if constexpr (WINDOW) {
          if (kbase + 31 <= pos_lo - a.window) continue;   // wave-uniform: the 32 keys are below every window of the wave's rows
        }
        f32x16 s = zero16();
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) A::mma(s, A::template row_frag<D>(tk, ra, 32 * st, kc), qf[kc]);
        // (window: only the sub-tiles that hold a key at or below the wave's highest edge - 1 mask for it)
        if (kbase + 32 > c1 || (a.causal && kbase + 31 > pos_lo) || (WINDOW && kbase <= pos_hi - a.window)) {   // wave-uniform
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int key = kbase + acc_row(i, h);
            if (key >= c1 || (a.causal && key > qpos) || (WINDOW && key <= qpos - a.window)) s[i] = -INFINITY;
          }
        }
        float mx = s[0];
#pragma unroll
        for (int i = 1; i < 16; ++i) mx = fmaxf(mx, s[i]);
        const float m_new = fmaxf(m_run, xhalf_max(mx));
        const float nm = (m_new == -INFINITY) ? 0.f : -m_new * c;   // (every key so far masked: any finite reference, P = 0)
        const float alpha = __builtin_amdgcn_exp2f(__builtin_fmaf(m_run, c, nm));
        float rs = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          s[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[i], c, nm));
          rs += s[i];
        }
        if (__any(alpha != 1.0f)) {
#pragma unroll
          for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc_o[dt][i] *= alpha;
        }
        l_run = l_run * alpha + rs;
        m_run = m_new;
        // bf16: P at 16 significant bits (pack + pack_lo), as in decode_split_kernel
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const frag p_hi = A::pack(s, s2);
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            const frag vt = A::template tr_frag<D>(tv, ta, 32 * st + 16 * s2, dt);
            A::mma(acc_o[dt], vt, p_hi);
            if constexpr (A::SPLITS) A::mma(acc_o[dt], vt, A::pack_lo(s, s2, p_hi));
          }
        }
      }
    }
  }
  const float l_tot = xhalf_sum(l_run);
  if (!live) return;   // (no barrier follows)
  // (ragged: out, lse and the partials by packed row row0 + qi, as one batch element of a.Nq = ntok queries)
  const size_t bhq = RAGGED ? (size_t)hd : (size_t)b * a.H + hd;
  if (a.nsplit == 1) {   // final: out = O / l, lse = m * tau + ln l; a row without an admissible key: out = 0, lse = -inf
    float inv = (l_tot > 0.f) ? 1.0f / l_tot : 0.f;
    if constexpr (FP8) inv *= scale_of(a.v_scale, hkv);   // (the scale of V: once per row, on 1 / l)
    float* orow = a.out + (RAGGED ? 0 : (size_t)b * a.q_bstride) + (size_t)hd * a.q_hstride + (size_t)(RAGGED ? row0 + qi : qi) * a.q_ld;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 val = {acc_o[dt][4 * g] * inv, acc_o[dt][4 * g + 1] * inv, acc_o[dt][4 * g + 2] * inv, acc_o[dt][4 * g + 3] * inv};
        *reinterpret_cast<f32x4*>(orow + 32 * dt + 8 * g + 4 * h) = val;
      }
    if (h == 0 && a.lse) a.lse[bhq * a.Nq + (RAGGED ? row0 + qi : qi)] = (l_tot > 0.f) ? m_run * FA_TAU + __logf(l_tot) : -INFINITY;
  } else {
    const size_t pr = (bhq * a.nsplit + split) * a.Nq + (RAGGED ? row0 + qi : qi);
    float* prow = a.part_o + pr * D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 val = {acc_o[dt][4 * g], acc_o[dt][4 * g + 1], acc_o[dt][4 * g + 2], acc_o[dt][4 * g + 3]};
        *reinterpret_cast<f32x4*>(prow + 32 * dt + 8 * g + 4 * h) = val;
      }
    if (h == 0) *reinterpret_cast<f32x2*>(a.part_ml + 2 * pr) = f32x2{m_run, l_tot};
  }
}
#undef FA_NQ
#undef FA_TAU

// out[row] = sum_s O_s 2^(c (m_s - M)) / sum_s l_s 2^(c (m_s - M)), M = max_s m_s.  A workgroup = one (bh, row): thread (g, j) takes
// columns 4g .. 4g+3 of the splits j, j + S, j + 2S, ... and the S partial sums of a column group are added in the order j = 0 .. S-1
// (a fixed order: bitwise repeatable).
// RAGGED: one batch element of Nq = ntok packed rows; a row in front of the first sequence or behind the last one (the unused tail
// of the packed buffers) has no partials and is neither read nor written.  (A cu that is not non-decreasing can make an earlier
// sequence end past the last one's end: its rows there are then left as they were, where a one-split call writes them.)
// FP8: the row's kv head is hd / a.G; its k_scale multiplies tau (the weights and the lse), its v_scale the final 1 / l.
template <int D, bool RAGGED = false, bool FP8 = false>
__global__ void __launch_bounds__(256) decode_combine_kernel(DecodeArgsOf<RAGGED, FP8> a) {
  constexpr int G = D / 4, S = 256 / G;
  __shared__ f32x4 red_o[256];
  __shared__ float red_m[256], red_l[256];
  const int tid = threadIdx.x, g = tid % G, j = tid / G;
  const int row = blockIdx.x % a.Nq, bh = blockIdx.x / a.Nq;
  if constexpr (RAGGED) {   // (workgroup-uniform: in front of the barriers)
    int s0, n0, sl, nl;
    seq_rows(a.cu, a.ntok, 0, s0, n0);
    seq_rows(a.cu, a.ntok, a.nseq - 1, sl, nl);
    if (row < s0 || row >= sl + nl) return;
  }
  const int b = bh / a.H, hd = bh - b * a.H;
  float tau8 = 0.f;
  if constexpr (FP8) tau8 = a.tau * scale_of(a.k_scale, hd / a.G);
#define FA_TAU (FP8 ? tau8 : a.tau)
  const float c = FA_TAU * LOG2E;
  const size_t p0 = (size_t)bh * a.nsplit * a.Nq + row;   // partial row of split s: p0 + s * Nq
  float m = -INFINITY;
  for (int s = j; s < a.nsplit; s += S) m = fmaxf(m, a.part_ml[2 * (p0 + (size_t)s * a.Nq)]);
  red_m[tid] = m;
  __syncthreads();
  float m_all = -INFINITY;
  for (int u = 0; u < S; ++u) m_all = fmaxf(m_all, red_m[u * G + g]);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float l = 0.f;
  if (m_all != -INFINITY) {
    for (int s = j; s < a.nsplit; s += S) {
      const size_t p = p0 + (size_t)s * a.Nq;
      const f32x2 ml = *reinterpret_cast<const f32x2*>(a.part_ml + 2 * p);
      if (ml[0] == -INFINITY) continue;
      const float wgt = __builtin_amdgcn_exp2f((ml[0] - m_all) * c);
      l += ml[1] * wgt;
      acc += *reinterpret_cast<const f32x4*>(a.part_o + p * D + 4 * g) * wgt;
    }
  }
  red_o[tid] = acc;
  red_l[tid] = l;
  __syncthreads();
  if (j != 0) return;
  for (int u = 1; u < S; ++u) {
    acc += red_o[u * G + g];
    l += red_l[u * G + g];
  }
  float inv = (l > 0.f) ? 1.0f / l : 0.f;
  if constexpr (FP8) inv *= scale_of(a.v_scale, hd / a.G);
  float* orow = a.out + (size_t)b * a.q_bstride + (size_t)hd * a.q_hstride + (size_t)row * a.q_ld;
  *reinterpret_cast<f32x4*>(orow + 4 * g) = acc * inv;
  if (g == 0 && a.lse) a.lse[(size_t)bh * a.Nq + row] = (l > 0.f) ? m_all * FA_TAU + __logf(l) : -INFINITY;
}
#undef FA_TAU

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
