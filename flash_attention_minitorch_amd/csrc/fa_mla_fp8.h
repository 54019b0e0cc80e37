// MLA decode on an FP8 latent cache (the deployment format of DeepSeek-V3.2-class models), dense and sparse, and the quantising append,
// for MI355X (gfx950).  Declared in include/flash_attn_mi355x_mla_fp8.h (the format is stated there), dispatched by fa_mla.hip into
// the same library.  A cache row is 656 bytes: 512 e4m3fn codes of the latent columns, four fp32 scales (one per 128 columns, powers
// of two in [2^-100, 2^120]), then the 64 rotated k_pe columns as bf16.  The value of latent column c is s_{c >> 7} * e4m3(code_c),
// which is exactly a bf16 value, so the codes are widened to bf16 ON THE WAY from the staging registers to LDS
// (v_cvt_scalef32_pk_bf16_fp8 carrying the tile's scale: one instruction per pair of columns) and the LDS image is the bf16 kernels'
// image.  Everything behind it is their text (fa_mla_split_body.h, fa_mla_sparse_split_body.h): an fp8 call returns bit for bit
// what the bf16 call returns on the cache dequantised to bf16.
//
// mla_fp8_split_kernel<PAGED> / mla_fp8_sparse_split_kernel<PAGED>: the bodies with FP8 = true, i.e. with MlaFp8Stager / MlaFp8Gather.
//   * The lane map is MlaStager's (row_of, chunk_of, lds_step: the image's ds_write_b128 rule holds as it stands).  An image chunk
//     (row, ch) of 8 columns is, for ch < 64, the 8 code bytes at row * 656 + 8 ch: one 8-byte load, four conversions, one 16-byte
//     LDS store; for ch >= 64 the 16 bytes of k_pe at row * 656 + 528 + 16 (ch - 64), stored as they are.  Passes 0..15 of a thread
//     are code passes, 16 and 17 are k_pe.
//   * The scale tile of pass i is i >> 2, a compile-time constant (chunk_of(tid, i) >> 4 == i >> 2 for every thread), so a thread
//     needs the four scales of its two rows and nothing else: one 16-byte load per row and tile image.
//   * Staging registers: 16 x 2 (codes) + 2 x 4 (k_pe) + 2 x 4 (scales) = 48, against the bf16 stager's 72.
//   * A row at or past the end of its resource (len_b, a page's valid rows, a sparse entry that is not admitted) reads as zero
//     bytes, scales included: code 0 under scale +0.0f widens to +0 (0 * 0; under an exponent-only reading of the scale, 0 * 2^-127).
//     The paged sparse gather reads row 0 of the pool for such an entry and clears codes, scales and k_pe in registers.
// mla_fp8_append_kernel: one wave per new row.  Lane l holds latent columns 8 l .. 8 l + 7 (one 16-byte load), the maximum of a
// 128-column tile is a reduction over 16 lanes, the scale comes from the maximum's exponent and mantissa bits alone (no division by
// 448), the codes are fa_decode.h's fp8_prescale / fp8_pack2 (clamp in front of the conversion, NaN -> 0x7F); one 8-byte store per
// lane, one lane stores the 16 bytes of scales, eight lanes copy k_pe.  Placement is mla_append_kernel's.
//
// (FP8 index keys for the indexer, with fp8 MFMAs, are fa_mla_indexer_fp8.h's.)
// Not built: fp8 queries or fp8 MFMAs for the attention itself, e5m2, scales that are not powers of two, other tile widths
// than 128, window / sink / cap, an extend kernel.
#pragma once
#include "fa_mla_sparse.h"

namespace fa {

typedef __attribute__((ext_vector_type(2))) uint32_t mla_u32x2;

// 8 e4m3 codes under one scale -> 8 bf16, in column order (as Fp8Stager::store, with the tile's scale in the place of 1.0f)
FA_DEV u32x4 mla_fp8_widen(mla_u32x2 c, float s) {
  return u32x4{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[0], s, false)),
               __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[0], s, true)),
               __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[1], s, false)),
               __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[1], s, true))};
}

// MlaStager for 656-byte rows.  Pass i < 16: codes at voff + code_step(i); the two k_pe passes and the two scale loads sit at
// fixed offsets of the thread's two rows.  covers_image() walks the map as MlaStager::covers_image does.
struct MlaFp8Stager {
  using S = MlaStager;
  static constexpr int PER = S::PER, NCODE = 16, ROWB = MLA_FP8_ROW_BYTES;
  static constexpr int code_step(int i) { return 32 * ROWB * (i & 1) + 64 * (i >> 1); }
  static constexpr bool covers_image() {
    bool seen[S::NCH] = {};
    for (int tid = 0; tid < 256; ++tid) {
      const int row0 = S::row_of(tid, 0), ch0 = S::chunk_of(tid, 0);
      for (int i = 0; i < PER; ++i) {
        const int row = S::row_of(tid, i), ch = S::chunk_of(tid, i);
        if (row >= MLA_TILE || ch >= S::CPR || seen[row * S::CPR + ch]) return false;
        seen[row * S::CPR + ch] = true;
        if (Atom<bf16_t>::off<MLA_DQK>(row, ch) != Atom<bf16_t>::off<MLA_DQK>(row0, ch0) + S::lds_step(i)) return false;
        if (row != row0 + 32 * (i & 1)) return false;   // (the scales and k_pe of a pass are those of row0 or row0 + 32)
        if (i < NCODE) {   // 8 code bytes, and the pass's scale tile
          if ((ch >= MLA_DV / 8) || (ch >> 4) != (i >> 2)) return false;
          if (row * ROWB + 8 * ch != row0 * ROWB + 8 * ch0 + code_step(i)) return false;
        } else if (row * ROWB + MLA_FP8_PE_OFF + 16 * (ch - MLA_DV / 8) != row0 * ROWB + 32 * ROWB * (i & 1) + MLA_FP8_PE_OFF + 16 * ch0) {
          return false;
        }
        const int t0 = tid & ~7;
        if ((row >> 1) != (S::row_of(t0, i) >> 1) || (ch >> 2) != (S::chunk_of(t0, i) >> 2)) return false;
      }
    }
    return true;
  }
  mla_u32x2 codes[NCODE];
  u32x4 pe[2];
  f32x4 scale[2];   // the four tile scales of row0 and of row0 + 32
  int voff, ch8, lds_off;
  FA_DEV void init(int tid) {
    ch8 = S::chunk_of(tid, 0) * 8;
    voff = S::row_of(tid, 0) * ROWB + ch8;
    lds_off = Atom<bf16_t>::off<MLA_DQK>(S::row_of(tid, 0), S::chunk_of(tid, 0));
  }
  // As MlaStager::load: the row offset rides in the voffset, so rows at or past the resource's end read as zero -- codes, scales, k_pe.
  FA_DEV void load(rsrc_t rs, int row0) {
    const int base = voff + row0 * ROWB;
#pragma unroll
    for (int i = 0; i < NCODE; ++i)
      codes[i] = __builtin_bit_cast(mla_u32x2, __builtin_amdgcn_raw_buffer_load_b64(rs, base + code_step(i), 0, 0));
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      scale[r] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, base - ch8 + 32 * ROWB * r + MLA_FP8_SCALE_OFF, 0, 0));
      pe[r] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, base + ch8 + 32 * ROWB * r + MLA_FP8_PE_OFF, 0, 0));
    }
  }
  FA_DEV void store(lds_char* tile) const {
#pragma unroll
    for (int i = 0; i < NCODE; ++i) *FA_LDS(u32x4, tile + lds_off + S::lds_step(i)) = mla_fp8_widen(codes[i], scale[i & 1][i >> 2]);
#pragma unroll
    for (int r = 0; r < 2; ++r) *FA_LDS(u32x4, tile + lds_off + S::lds_step(NCODE + r)) = pe[r];
  }
};
static_assert(MlaFp8Stager::covers_image(), "the fp8 stager must tile the 64 x 576 image once, from the right bytes of a 656-byte row");

// MlaGather for 656-byte rows: the same passes with a source per thread row.  src as MlaGather::load takes it.
template <bool PAGED>
struct MlaFp8Gather {
  using S = MlaStager;
  using F = MlaFp8Stager;
  mla_u32x2 codes[F::NCODE];
  u32x4 pe[2];
  f32x4 scale[2];
  int lds_off, ch8, r0;
  FA_DEV void init(int tid) {
    r0 = S::row_of(tid, 0);
    ch8 = S::chunk_of(tid, 0) * 8;
    lds_off = Atom<bf16_t>::off<MLA_DQK>(r0, S::chunk_of(tid, 0));
  }
  FA_DEV void load(rsrc_t rs, const char* pool, int src) {
    const int s[2] = {__shfl(src, r0), __shfl(src, r0 + 32)};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if constexpr (PAGED) {
        const char* row = pool + (size_t)(uint32_t)s[r] * F::ROWB;
#pragma unroll
        for (int sp = 0; sp < F::NCODE / 2; ++sp) codes[2 * sp + r] = *reinterpret_cast<const mla_u32x2*>(row + ch8 + 64 * sp);
        scale[r] = *reinterpret_cast<const f32x4*>(row + MLA_FP8_SCALE_OFF);
        pe[r] = *reinterpret_cast<const u32x4*>(row + MLA_FP8_PE_OFF + 2 * ch8);
      } else {
#pragma unroll
        for (int sp = 0; sp < F::NCODE / 2; ++sp)
          codes[2 * sp + r] = __builtin_bit_cast(mla_u32x2, __builtin_amdgcn_raw_buffer_load_b64(rs, s[r] + ch8 + 64 * sp, 0, 0));
        scale[r] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, s[r] + MLA_FP8_SCALE_OFF, 0, 0));
        pe[r] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, s[r] + MLA_FP8_PE_OFF + 2 * ch8, 0, 0));
      }
    }
  }
  FA_DEV void store(lds_char* tile, uint64_t mask) {
    if constexpr (PAGED) {   // (slab: the hardware returned zeros.  The scales too: row 0 of the pool may hold anything)
#pragma unroll
      for (int r = 0; r < 2; ++r)
        if (!((mask >> (r0 + 32 * r)) & 1)) {
#pragma unroll
          for (int sp = 0; sp < F::NCODE / 2; ++sp) codes[2 * sp + r] = mla_u32x2{0u, 0u};
          scale[r] = f32x4{0.f, 0.f, 0.f, 0.f};
          pe[r] = u32x4{0u, 0u, 0u, 0u};
        }
    }
#pragma unroll
    for (int i = 0; i < F::NCODE; ++i) *FA_LDS(u32x4, tile + lds_off + S::lds_step(i)) = mla_fp8_widen(codes[i], scale[i & 1][i >> 2]);
#pragma unroll
    for (int r = 0; r < 2; ++r) *FA_LDS(u32x4, tile + lds_off + S::lds_step(F::NCODE + r)) = pe[r];
  }
};

// DecodeArgs as mla_decode_split_kernel reads it, with the cache strides of a 656-byte row in 2-byte units: kv_ld = 328,
// kv_bstride = Ncap * 328, page_stride = page_size * 328.
template <bool PAGED>
__global__ void __launch_bounds__(256) mla_fp8_split_kernel(DecodeArgs a) {
  constexpr bool FP8 = true;
#include "fa_mla_split_body.h"
}

template <bool PAGED>
__global__ void __launch_bounds__(256) mla_fp8_sparse_split_kernel(MlaSparseArgs a) {
  constexpr bool FP8 = true;
#include "fa_mla_sparse_split_body.h"
}

// Append: MlaAppendArgs with lanes = B * Nq ROWS (a wave per row, four rows per workgroup); kv_new is bf16 [B][Nq][576].  Per
// 128-column tile: a = max |x| in fp32 (v_max drops a NaN, keeps an infinity), s = the smallest power of two with a <= 448 s,
// clamped to [2^-100, 2^120].  With a = 1.f * 2^(E - 127), 448 = 1.75 * 2^8: the biased exponent of s is E - 8, or E - 7 when
// 1.f > 1.75; zero and the clamp need no case of their own.  1 / s is the power of two with biased exponent 254 - that.
__global__ void __launch_bounds__(256) mla_fp8_append_kernel(MlaAppendArgs a) {
  constexpr int CPR = MlaStager::CPR;
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);   // source row (b, i)
  if (row >= a.lanes) return;
  const int b = (int)(row / a.Nq), i = (int)(row - (long)b * a.Nq);
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
  const u32x4* src = reinterpret_cast<const u32x4*>(a.kv_new) + row * CPR;
  char* dst = reinterpret_cast<char*>(a.kv) + dst_row * MLA_FP8_ROW_BYTES;
  const bf16x8 x = __builtin_bit_cast(bf16x8, src[lane]);
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) amax = __builtin_fmaxf(amax, __builtin_fabsf((float)x[j]));
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) amax = __builtin_fmaxf(amax, __shfl_xor(amax, m));
  const uint32_t bits = __builtin_bit_cast(uint32_t, amax);
  const int e = min(max((int)(bits >> 23) - 8 + ((bits & 0x7fffffu) > 0x600000u ? 1 : 0), 127 - 100), 127 + 120);
  const float rcp = __builtin_bit_cast(float, (uint32_t)(254 - e) << 23);
  mla_u32x2 c;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    c[j] = fp8_pack2((float)x[4 * j], (float)x[4 * j + 1], rcp, 0u, false);
    c[j] = fp8_pack2((float)x[4 * j + 2], (float)x[4 * j + 3], rcp, c[j], true);
  }
  *reinterpret_cast<mla_u32x2*>(dst + 8 * lane) = c;
  const uint32_t sb = (uint32_t)e << 23;
  const u32x4 scales = {(uint32_t)__shfl((int)sb, 0), (uint32_t)__shfl((int)sb, 16), (uint32_t)__shfl((int)sb, 32), (uint32_t)__shfl((int)sb, 48)};
  if (lane == 0) *reinterpret_cast<u32x4*>(dst + MLA_FP8_SCALE_OFF) = scales;
  if (lane < 8) *reinterpret_cast<u32x4*>(dst + MLA_FP8_PE_OFF + 16 * lane) = src[MLA_DV / 8 + lane];
}

}  // namespace fa
