// Multi-head latent attention (DeepSeek-V2 / V3 / R1, Kimi-K2) decode on a latent KV cache, for MI355X (gfx950): bf16, one cache row of
// 576 columns per token shared by ALL heads -- the compressed latent c_kv (512 columns) followed by the rotated k_pe (64).  With the
// up-projections absorbed into q a step is multi-query attention in which the score product runs over all 576 columns, the value is
// the first 512 columns of the SAME row, and the result is (H, 512) per token.  Declared in include/flash_attn_mi355x_mla.h,
// dispatched by fa_mla.hip; the atoms, make_rsrc, clamp_len, row_query and the page walk are fa_atoms.h's and fa_decode.h's, used as
// they are (this unit changes no shared definition: every other library's code object stays what it is).
//
// mla_decode_split_kernel<PAGED>: 256 threads, one wave per SIMD on the whole 512-entry register file; a workgroup = one (batch, key
// chunk, 64-row block).  Rows run in the decode kernels' order with G = H: rho = i * H + h for query i and head h; rows >= H * Nq read
// as zero and store nothing, and a 32-row half without a live row is skipped wave-uniformly in both products.
//   * The cache is walked in 64-key tiles of 576 columns (72 KB) in the image Atom<bf16_t>::off<576>, staged through registers
//     (MlaStager: 18 x 16 bytes per thread, the next tile's loads issued in front of this tile's MFMAs).  ONE image serves both
//     products: S reads row fragments over all 36 k-chunks, P.V reads transposed fragments of columns 0..511 of the same image, so a
//     cache row crosses HBM once and LDS once per workgroup.
//   * S: wave w = (key half kh = w & 1, row half rh = w >> 1) forms ONE 32 x 32 tile of S^T = K Q^T over the full 576 columns, 36 MFMAs
//     against its 32 rows of Q held as 144 registers of fragments (loaded once per workgroup).  The two key halves of a row half
//     exchange their tile maxima through LDS and form the same m_new and the same alpha; P = exp2(s c - m_new c) goes to LDS as the
//     bf16 pair pack + pack_lo (16 KB for 64 x 64, in the lanes' own fragment order: a reader's fragment is the writer's), alpha per
//     row beside it.  Each wave keeps the row sums of its own key half; the two halves are added once, at the end.
//   * P.V: every wave takes the output columns 128 w .. 128 w + 127 of all 64 rows over all 64 keys: 8 accumulator tiles (128
//     registers), per staged tile 4 k-steps x 8 tiles x 2 (hi, lo) = 64 MFMAs, rescaled by the alpha read from LDS.  So a tile costs
//     every wave 36 + 64 MFMAs and none of them is issued twice in the workgroup (decode_split_d256_kernel forms S once per column
//     half: free when the cache stream is the limit, not at H = 128 where the MFMAs are).
//   * One split stores out = O / l and lse = m tau + ln l; several splits store (o[512], m, l) partials, which
//     mla_decode_combine_kernel merges in split order (decode_combine_kernel's body text at 512 columns).  No atomics: a call repeats
//     bit for bit.  Chunks are whole multiples of 128 keys and a page a multiple of FA_PAGE_ROWS rows, so a tile lies inside one page
//     and a paged call returns the slab call's bits on the gathered cache.  Resources end at len_b or at the page.
// mla_append_kernel: token i of batch element b goes to row len_b - Nq + i, slab or paged, in 16-byte moves.
//
// Not built: window, sink tokens, soft cap, learned sink logits, the ragged family, other latent widths, the training backward.
// (A prompt is prefilled before absorption by a kernel of its own: fa_mla_prefill.h.  Attention over per-query index lists, DeepSeek-V3.2's sparse attention, is a kernel
// of its own on this image and these products: fa_mla_sparse.h.  An fp8 latent cache: fa_mla_fp8.h.)
#pragma once
#include "fa_atoms.h"
#include "fa_common.h"
#include "fa_decode.h"

namespace fa {

constexpr int MLA_DQK = 576, MLA_DV = 512;   // columns of a cache row (and of q); columns of it that are the value (and of out)
constexpr int MLA_TILE = 64;                 // keys per staged tile: 32 per key half
constexpr int MLA_BLOCK = 64;                // rows per workgroup: 32 per row half
constexpr int MLA_ROW_BYTES = MLA_DQK * 2;
// An fp8 cache row (fa_mla_fp8.h, whose kernels share this header's body text): 512 e4m3 codes, four fp32 tile scales, 64 bf16 k_pe.
constexpr int MLA_FP8_SCALE_OFF = MLA_DV, MLA_FP8_PE_OFF = MLA_DV + 16, MLA_FP8_ROW_BYTES = MLA_FP8_PE_OFF + (MLA_DQK - MLA_DV) * 2;
struct MlaFp8Stager;

// The register-staged copy of one 64 x 576 bf16 tile by 256 threads: 72 chunks of 16 bytes per row, which TileStager cannot tile
// (256 % 72 != 0).  Pass i = 2 * sp + rph of 18 moves, for lane group g = tid >> 3, the rows 2 * (g >> 1) + 32 * rph (+ 1 for the
// odd half of the group) at the four chunks of the 32-column subtile 2 * sp + (g & 1).  Eight consecutive lanes cover two adjacent
// rows x four chunks of one subtile (the image's ds_write_b128 rule, as TileStager), sixteen cover 128 contiguous bytes of each of
// two cache rows, and a row step of 32 keeps the swizzle phase: a thread's 18 global offsets and 18 LDS offsets are one register
// each plus compile-time constants.
struct MlaStager {
  static constexpr int CPR = MLA_DQK / 8, NCH = MLA_TILE * CPR, PER = NCH / 256;
  static_assert(NCH % 256 == 0 && PER == 18, "every thread moves 18 chunks");
  static constexpr int row_of(int tid, int i) { return 2 * (tid >> 4) + ((tid >> 2) & 1) + 32 * (i & 1); }
  static constexpr int chunk_of(int tid, int i) { return 4 * (2 * (i >> 1) + ((tid >> 3) & 1)) + (tid & 3); }
  static constexpr int src_step(int i) { return 32 * MLA_ROW_BYTES * (i & 1) + 128 * (i >> 1); }
  static constexpr int lds_step(int i) { return Atom<bf16_t>::off<MLA_DQK>(32 * (i & 1), 8 * (i >> 1)); }
  // every (row, chunk) of the tile exactly once, at the offsets init and the two steps form; eight lanes: two adjacent rows, one subtile
  static constexpr bool covers_image() {
    bool seen[NCH] = {};
    for (int tid = 0; tid < 256; ++tid)
      for (int i = 0; i < PER; ++i) {
        const int row = row_of(tid, i), ch = chunk_of(tid, i);
        if (row >= MLA_TILE || ch >= CPR || seen[row * CPR + ch]) return false;
        seen[row * CPR + ch] = true;
        if (Atom<bf16_t>::off<MLA_DQK>(row, ch) != Atom<bf16_t>::off<MLA_DQK>(row_of(tid, 0), chunk_of(tid, 0)) + lds_step(i)) return false;
        if (row * MLA_ROW_BYTES + ch * 16 != row_of(tid, 0) * MLA_ROW_BYTES + chunk_of(tid, 0) * 16 + src_step(i)) return false;
        const int t0 = tid & ~7;
        if ((row >> 1) != (row_of(t0, i) >> 1) || (ch >> 2) != (chunk_of(t0, i) >> 2)) return false;
      }
    return true;
  }
  u32x4 regs[PER];
  int voff, lds_off;
  FA_DEV void init(int tid) {
    voff = row_of(tid, 0) * MLA_ROW_BYTES + chunk_of(tid, 0) * 16;
    lds_off = Atom<bf16_t>::off<MLA_DQK>(row_of(tid, 0), chunk_of(tid, 0));
  }
  // The tile whose first row is row0 of the matrix the resource covers.  The row offset rides in the voffset, so the resource's
  // range check covers it: rows at or past the resource's end (len_b, or the page's valid rows) read as zero.
  FA_DEV void load(rsrc_t rs, int row0) {
#pragma unroll
    for (int i = 0; i < PER; ++i)
      regs[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff + row0 * MLA_ROW_BYTES + src_step(i), 0, 0));
  }
  FA_DEV void store(lds_char* tile) const {
#pragma unroll
    for (int i = 0; i < PER; ++i) *FA_LDS(u32x4, tile + lds_off + lds_step(i)) = regs[i];
  }
};
static_assert(MlaStager::covers_image(), "the stager's lane-to-chunk map must tile the 64 x 576 image once, by the image's write rule");

// The kernels' argument is fa_decode.h's DecodeArgs with Hkv = 1 and G = H (row_query, clamp_len and PageWalk read it as it is):
// q [B][Nq][H][576] (q_ld = H * 576, q_hstride = 576, q_bstride = Nq * H * 576), k = the latent cache (kv_ld = 576, kv_hstride = 0,
// kv_bstride = Ncap * 576, page_stride = page_size * 576; v is not read), items = B * nsplit, nqb = ceil(H * Nq / 64).
// out is [B][Nq][H][512], lse [B][H][Nq], the partials [B * H][nsplit][Nq][512] and [..][2] as decode_combine_kernel reads them.
// The body is TEXT, fa_mla_split_body.h, shared with the fp8 cache's kernel of fa_mla_fp8.h (FP8 there picks the stager and the
// bytes of a cache row; as text this kernel keeps its name, its one template parameter and its code).
template <bool PAGED>
__global__ void __launch_bounds__(256) mla_decode_split_kernel(DecodeArgs a) {
  constexpr bool FP8 = false;
#include "fa_mla_split_body.h"
}

// The combine kernel at 512 columns: decode_combine_kernel's body text (thread (g, j): columns 4g .. 4g+3 of the splits j, j + 2,
// ...; the two partial sums of a column group added in the order j = 0, 1; in log2 units).  It addresses out through q's strides, so
// the host hands it the argument with OUT's strides in their place (q itself is not read here).
// (RAGGED is never true: it makes the argument's type depend on a template parameter, for the reason decode_split_sink_kernel gives.)
template <bool RAGGED>
__global__ void __launch_bounds__(256) mla_decode_combine_kernel(DecodeArgsOf<RAGGED> a) {
  constexpr int D = MLA_DV;
  constexpr bool FP8 = false, LSINK = false;
#include "fa_decode_combine_body.h"
}

// Append: kv_new [B][Nq][576] into the cache.  With L_b = len_b clamped to [0, Ncap] (the length COUNTS the new tokens), token i goes
// to row L_b - Nq + i, the position the causal mask gives query i; rows below 0 are not written and no row reaches Ncap.  A lane moves
// one 16-byte chunk; page ids are clamped to the pool as the split kernel's.
struct MlaAppendArgs {
  const void* kv_new;
  void* kv;
  const int* seqlens;   // [B] or null (= Ncap)
  const int* table;     // [B][max_pages] or null: slabs of Ncap rows
  long lanes;           // B * Nq * 72
  int Nq, Ncap, page_size, num_pages, max_pages;
};

__global__ void __launch_bounds__(256) mla_append_kernel(MlaAppendArgs a) {
  constexpr int CPR = MlaStager::CPR;
  const long lane = (long)blockIdx.x * 256 + threadIdx.x;
  if (lane >= a.lanes) return;
  const long row = lane / CPR;   // source row (b, i)
  const int ch = (int)(lane - row * CPR), b = (int)(row / a.Nq), i = (int)(row - (long)b * a.Nq);
  const int pos = clamp_len(a.seqlens, a.Ncap, b) - a.Nq + i;
  if (pos < 0) return;
  size_t dst_row;
  if (a.table) {
    const int slot = pos / a.page_size;
    const int page = min(max(a.table[(size_t)b * a.max_pages + slot], 0), a.num_pages - 1);
    dst_row = (size_t)page * a.page_size + (pos - slot * a.page_size);
  } else {
    dst_row = (size_t)b * a.Ncap + pos;
  }
  reinterpret_cast<u32x4*>(a.kv)[dst_row * CPR + ch] = reinterpret_cast<const u32x4*>(a.kv_new)[lane];
}

}  // namespace fa
