// Sparse MLA decode (DeepSeek-V3.2 sparse attention, DSA) on the latent KV cache of fa_mla.h, for MI355X (gfx950): every query token
// brings a list of topk cache positions (an indexer's top-k: fa_mla_indexer.h's, or the caller's) and all heads of that token attend those
// rows alone.  Declared in include/flash_attn_mi355x_mla_sparse.h, dispatched by fa_mla.hip into the same library.  The tile image,
// its swizzle, MlaStager's lane-to-chunk map, the two fragment readers, the P buffer, the row constants, the partial layout and
// mla_decode_combine_kernel are fa_mla.h's, used as they are: this header changes no definition of it.
//
// An entry e of query (b, i) names position j = indices[b][i][e].  It is ADMITTED iff 0 <= j < len_b, and under `causal` also
// j <= len_b - Nq + i: one unsigned compare, j < lim, with lim = min(len_b, len_b - Nq + i + 1) uniform for the workgroup.  Every
// other value (-1 padding, any negative, anything at or past len_b or Ncap) is an entry that is not there.  The compare comes
// before any address arithmetic: no cache row and no page id is read for an entry that is not admitted, and its row of the tile is
// zeros.  An entry is a key of its own: a position named twice counts twice.
//
// mla_sparse_split_kernel<PAGED>: 256 threads, one wave per SIMD; a workgroup = (batch b, query token i, 64-HEAD block, chunk of
// that token's index list).  All 64 rows of a block belong to one token, so every row sees the same 64 keys of a tile with the same
// validity (the dense kernel's rows rho = i * H + h mix tokens in a block, and two tokens read different rows here).
//   * Validity of a tile is ONE wave-uniform 64-bit mask: lane e of every wave holds entry e of the tile, and the mask is the ballot
//     of its compare.  Masking S is a bit test on 32 kh + acc_row(i, h).  A key half whose 32 bits are clear skips its 36 score MFMAs
//     and joins as -inf; a 16-key k-step whose bits are clear skips its P.V MFMAs; a tile whose mask is 0 is neither loaded nor
//     stored nor multiplied and passes no barrier (every wave holds the same mask, so the barriers stay workgroup-uniform).
//   * Gather staging.  MlaStager gives a thread two rows of a tile (row_of(tid, 0) and that + 32) at nine 16-byte chunks each; a
//     row's 1152 bytes stay contiguous, so eight lanes still cover full 128-byte segments.  The thread takes its two source rows
//     from the lanes that hold those entries (two ds_bpermute).  Slab: buffer loads whose voffset is j * 1152 for an admitted row
//     and the resource's size for any other, which the hardware answers with zeros.  Paged: a pool may exceed 4 GiB and a resource
//     must be wave-uniform, so rows go through 64-bit global loads; the lane that holds an admitted entry reads its page id
//     (clamped to the pool), any other row is aimed at row 0 of the pool and its registers become zeros before the LDS store.
//   * The chain index -> (page id) -> row -> LDS is pipelined in registers, one register per stage: while tile t is in the MFMAs the
//     rows of tile t + 1 are in flight, the entries of tile t + 2 have been compared and (paged) their page ids requested, and the
//     entries of tile t + 3 are requested.  (A chunk's list has no bound, so it is not staged in LDS.)
//   * Everything behind the image is the dense kernel's: the 32 x 32 score tile over 36 k-chunks against Q fragments in registers,
//     the key halves' maximum exchange, P as the bf16 hi + lo pair, each wave's 128 output columns for all 64 rows, alpha through
//     LDS, the final or the partial store.  topk is a multiple of 64: there is no partial tile.
//
// Not built: a sparse prefill / extend kernel, other topk granularities than 64, a window, cap or sink beside the
// indices.  (The indexer is fa_mla_indexer.h; an fp8 latent cache is fa_mla_fp8.h.)
#pragma once
#include "fa_mla.h"

namespace fa {

// DecodeArgs as mla_decode_split_kernel reads it (H, Nq, nsplit, chunk, nqb = ceil(H / 64), items = B * Nq * nsplit, q's strides,
// the partials, the table), and the lists.  mla_decode_combine_kernel is launched on the DecodeArgs part.
struct MlaSparseArgs : DecodeArgs {
  const int* indices;   // [B][Nq][topk]
  int topk;
};

// The gather of one 64-entry tile: MlaStager's map with a source row per thread row instead of one row offset per tile.
template <bool PAGED>
struct MlaGather {
  using S = MlaStager;
  u32x4 regs[S::PER];
  int lds_off, coff, r0;   // LDS offset and byte offset inside a cache row of the thread's first chunk; its first row of the tile
  FA_DEV void init(int tid) {
    r0 = S::row_of(tid, 0);
    coff = S::chunk_of(tid, 0) * 16;
    lds_off = Atom<bf16_t>::off<MLA_DQK>(r0, S::chunk_of(tid, 0));
  }
  // src: on lane e the source of entry e.  Slab: its byte offset in the resource (the resource's size: not admitted).  Paged: its
  // row in the pool (0: not admitted; such a row is cleared in store()).
  FA_DEV void load(rsrc_t rs, const char* pool, int src) {
    const int s[2] = {__shfl(src, r0), __shfl(src, r0 + 32)};
#pragma unroll
    for (int i = 0; i < S::PER; ++i) {
      if constexpr (PAGED)
        regs[i] = *reinterpret_cast<const u32x4*>(pool + (size_t)(uint32_t)s[i & 1] * MLA_ROW_BYTES + coff + 128 * (i >> 1));
      else
        regs[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, s[i & 1] + coff + 128 * (i >> 1), 0, 0));
    }
  }
  FA_DEV void store(lds_char* tile, uint64_t mask) {
    if constexpr (PAGED) {   // (slab: the hardware returned zeros)
      const bool keep[2] = {(bool)((mask >> r0) & 1), (bool)((mask >> (r0 + 32)) & 1)};
#pragma unroll
      for (int i = 0; i < S::PER; ++i)
        if (!keep[i & 1]) regs[i] = u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int i = 0; i < S::PER; ++i) *FA_LDS(u32x4, tile + lds_off + S::lds_step(i)) = regs[i];
  }
};

template <bool PAGED> struct MlaFp8Gather;   // (fa_mla_fp8.h)

// The body is TEXT, fa_mla_sparse_split_body.h, shared with the fp8 cache's kernel of fa_mla_fp8.h (FP8 there picks the gather and
// the bytes of a cache row).
template <bool PAGED>
__global__ void __launch_bounds__(256) mla_sparse_split_kernel(MlaSparseArgs a) {
  constexpr bool FP8 = false;
#include "fa_mla_sparse_split_body.h"
}

}  // namespace fa
