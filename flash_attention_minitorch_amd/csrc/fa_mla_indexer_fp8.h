// The lightning indexer on FP8 index keys (the deployment format of DeepSeek-V3.2's indexer) for MI355X (gfx950): the score kernel on
// fp8 matrix instructions and the quantising append.  Declared in include/flash_attn_mi355x_mla_indexer_fp8.h (the format is stated
// there), dispatched by fa_mla.hip into the same library.  MlaIndexArgs, MlaAppendArgs, the chunk and group policy, the top-k kernel and
// the definition of a score are fa_mla_indexer.h's, used as they are: this header changes no definition of theirs.
//
// An index-key row is 144 bytes: 128 e4m3fn codes, one fp32 power-of-two scale, 12 zero bytes.  The value of column c is
// s * e4m3(code_c).  q_idx stays bf16 in the interface and is quantised by the append's rule, row by row, on its way into LDS:
//   I[b,i,s] = s_k[s] * sum_h (w[b,i,h] * s_q[b,i,h]) * max(0, sum_c qcode[b,i,h,c] * kcode[s,c])
// which is the bf16 definition on the dequantised operands, since every scale is a positive power of two.
//
// mla_index_scores_fp8_kernel<PAGED>: the bf16 kernel's split (256 threads per (batch, token group, chunk); heads are the MFMA's M rows,
// keys its N columns, a lane owns ONE key, a wave a 32-key tile of each 128-key step; nothing is shared between waves but Q, so the
// key loop has no barrier), on v_mfma_f32_32x32x64_f8f6f4 at unit scales: 2 MFMAs of 16 passes per 32-head tile and key tile against
// the 8 MFMAs of 8 passes of either 32x32x16 form (bf16, or fp8_fp8, which gfx950 runs at the bf16 rate).
//   * Keys bypass LDS.  An MFMA's K index is some fixed function of (lane half, byte of the 32-byte operand), the same for A and B; a
//     dot product does not care which, as long as Q follows the keys.  Lane half h streams bytes 64 h .. 64 h + 63 of its key's row
//     as four 16-byte loads: loads 0, 1 are the B operand of MFMA 0, loads 2, 3 of MFMA 1.  Lane half 0, which stores the scores,
//     also loads the row's scale (a fifth, 4-byte load of the same cache line); the next step's loads are issued in front of this
//     step's MFMAs.  Slab: buffer loads whose resource ends at len_b (rows past it read as zero, scale included).  Paged: global
//     loads through the step's page id, clamped to the pool; a lane whose key is at or past len_b loads nothing.
//   * Q: the staging loop gives 16 lanes one (token, head) row of 128 bf16 columns, 8 columns each: the row's maximum is a 16-lane
//     reduction, the scale comes from its exponent and mantissa (mla_fp8_append_kernel's rule), the 8 codes are one 8-byte LDS store,
//     and the lane of chunk 0 stores w * s_q as the head's weight.  LDS holds Q in fragment order: block (token, 32-head tile) of 4 KB
//     = 4 pieces of 64 lanes x 16 bytes, piece p of lane (r, h) = columns 64 h + 16 p .. + 15 of head r.  An MFMA reads its A
//     operand with two conflict-free ds_read_b128.  32 KB of Q (8 blocks: the bf16 kernel's token groups) + 2 KB of weights.
//   * The 32 x 32 accumulator gives a lane 16 heads of its key: ReLU and the weighted head sum are 16 in-lane FMAs per head tile, one
//     lane <-> lane + 32 add finishes the sum, and the key's scale multiplies it once.  The add order is the same in both builds:
//     a paged call returns the slab call's bits.
// mla_index_append_fp8_kernel: 16 lanes per new row, 8 columns each; the maximum is a 16-lane reduction, codes by fa_decode.h's
// fp8_pack2 (clamp in front of the conversion, NaN -> 0x7F); one 8-byte store per lane, and the lane of chunk 0 stores the 16 bytes
// {scale, 0, 0, 0}.  Placement is mla_index_append_kernel's.
//
// Not built: e5m2, scales that are not powers of two, fp8 q_idx supplied by the caller, a fused score + select launch.
#pragma once
#include "fa_mla_fp8.h"
#include "fa_mla_indexer.h"

namespace fa {

constexpr int MLA_IDX8_ROW_BYTES = 144, MLA_IDX8_SCALE_OFF = MLA_IDX_D;
constexpr int MLA_IDX8_QBLOCK = 32 * MLA_IDX_D;   // bytes of one 32-head block of Q codes
static_assert(MLA_IDX8_ROW_BYTES % 16 == 0 && MLA_IDX8_SCALE_OFF + 4 <= MLA_IDX8_ROW_BYTES, "rows keep 16-byte alignment and hold their scale");

typedef __attribute__((ext_vector_type(8))) int mla_i32x8;

// 8 bf16 columns of a 128-column row that 16 consecutive lanes hold -> their 8 e4m3 codes, and the row's scale as fp32 bits.
// a = max |x| (v_max drops a NaN, keeps an infinity); with a = 1.f * 2^(E - 127) and 448 = 1.75 * 2^8 the biased exponent of the
// smallest power of two s with a <= 448 s is E - 8, or E - 7 when 1.f > 1.75, clamped to [2^-100, 2^120].  Called by whole groups.
FA_DEV mla_u32x2 idx8_quantise(const bf16x8& x, uint32_t& scale_bits) {
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
  scale_bits = (uint32_t)e << 23;
  return c;
}

template <bool PAGED>
__global__ void __launch_bounds__(256) mla_index_scores_fp8_kernel(MlaIndexArgs a) {
  constexpr int QB = MLA_IDX_QBLOCKS * MLA_IDX8_QBLOCK, WB = MLA_IDX_MAX_GROUP * MLA_IDX_MAX_HI * 4, ROWB = MLA_IDX8_ROW_BYTES;
  __shared__ __attribute__((aligned(16))) char smem_raw[QB + WB];
  lds_char* qs = (lds_char*)smem_raw;   // [token][head tile][piece][lane] 16-byte pieces of codes
  lds_char* ws = qs + QB;               // [token][128] weights, the heads' scales folded in

  const int id = blockIdx.x;
  const int chunk = id % a.nchunk, rest = id / a.nchunk, grp = rest % a.ngroups, b = rest / a.ngroups;
  const int len = __builtin_amdgcn_readfirstlane(clamp_len(a.seqlens, a.Ncap, b));
  const int c0 = chunk * a.chunk, c1 = min(c0 + a.chunk, len);
  if (c0 >= c1) return;   // (a chunk wholly past len_b reads and writes nothing; workgroup-uniform, in front of the barrier)

  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int NT = (a.HI + 31) >> 5, hpad = 32 * NT;
  const int i0 = grp * a.group, nt = min(a.group, a.Nq - i0);

  // Q of the group's tokens, quantised row by row, into fragment order.  16 consecutive lanes hold the 16 chunks of one head's row
  // (nt * hpad * 16 is a multiple of 512: every trip is whole); chunk c = 8 hh + 2 p + o goes to piece p, lane 32 hh + (hl & 31),
  // byte 8 o.  Heads past HI get the resource's size as their offset, read as zero and weigh nothing.
  const uint32_t q_bytes = (uint32_t)a.Nq * a.HI * MLA_IDX_ROW_BYTES;
  const rsrc_t qrs = make_rsrc(reinterpret_cast<const char*>(a.q) + (size_t)b * q_bytes, q_bytes);
  for (int idx = tid; idx < nt * hpad * 16; idx += 256) {
    const int c = idx & 15, row = idx >> 4, t = row / hpad, hl = row - t * hpad;
    const int off = hl < a.HI ? (((i0 + t) * a.HI + hl) * 16 + c) * 16 : (int)q_bytes;
    const bf16x8 x = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(qrs, off, 0, 0));
    uint32_t sb;
    const mla_u32x2 codes = idx8_quantise(x, sb);
    *FA_LDS(mla_u32x2, qs + (t * NT + (hl >> 5)) * MLA_IDX8_QBLOCK + ((c & 7) >> 1) * 1024 + (32 * (c >> 3) + (hl & 31)) * 16 + 8 * (c & 1)) = codes;
    if (c == 0)
      *FA_LDS(float, ws + (t * MLA_IDX_MAX_HI + hl) * 4) =
          hl < a.HI ? a.w[((size_t)b * a.Nq + i0 + t) * a.HI + hl] * __builtin_bit_cast(float, sb) : 0.f;
  }
  __syncthreads();   // (the key loop reads the weights of heads below hpad alone)

  // the slab's resource ends at len_b (unused by a paged build)
  const rsrc_t krs = make_rsrc(reinterpret_cast<const char*>(a.k) + (PAGED ? 0 : (size_t)b * a.Ncap * ROWB), (uint32_t)len * ROWB);
  const char* pool = reinterpret_cast<const char*>(a.k);
  const int* trow = a.table + (PAGED ? (size_t)b * a.max_pages : 0);
  const int kl = 32 * w + r;   // the lane's key inside a step

  // The wave's tile of the step at key t_ into dst and sc_: the lane's key row, bytes 64 h ..; lane half 0 takes the row's scale.
#define FA_IDX8_LOAD(dst, sc_, t_, page_)                                                                                \
  {                                                                                                                      \
    const int key_ = (t_) + kl;                                                                                          \
    sc_ = 0.f;                                                                                                           \
    if constexpr (PAGED) {                                                                                               \
      if (key_ < len) {                                                                                                  \
        const char* p_ = pool + ((size_t)(page_) * a.page_size + ((t_) % a.page_size + kl)) * ROWB;                      \
        _Pragma("unroll") for (int p = 0; p < 4; ++p) dst[p] = *reinterpret_cast<const u32x4*>(p_ + 64 * h + 16 * p);    \
        if (h == 0) sc_ = *reinterpret_cast<const float*>(p_ + MLA_IDX8_SCALE_OFF);                                      \
      } else {                                                                                                           \
        _Pragma("unroll") for (int p = 0; p < 4; ++p) dst[p] = u32x4{0u, 0u, 0u, 0u};                                    \
      }                                                                                                                  \
    } else {                                                                                                             \
      _Pragma("unroll") for (int p = 0; p < 4; ++p)                                                                      \
        dst[p] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(krs, key_ * ROWB + 64 * h + 16 * p, 0, 0)); \
      if (h == 0) sc_ = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(krs, key_ * ROWB + MLA_IDX8_SCALE_OFF, 0, 0)); \
    }                                                                                                                    \
  }
#define FA_IDX8_PAGE(t_) (PAGED ? min(max(trow[(t_) / a.page_size], 0), a.num_pages - 1) : 0)

  u32x4 kf[4], kn[4];
  float ks, ksn;
  int page_nxt = FA_IDX8_PAGE(c0);
  FA_IDX8_LOAD(kn, ksn, c0, page_nxt)
  if (c0 + MLA_IDX_STEP < c1) page_nxt = FA_IDX8_PAGE(c0 + MLA_IDX_STEP);
  for (int t0 = c0; t0 < c1; t0 += MLA_IDX_STEP) {
#pragma unroll
    for (int p = 0; p < 4; ++p) kf[p] = kn[p];
    ks = ksn;
    if (t0 + MLA_IDX_STEP < c1) {
      FA_IDX8_LOAD(kn, ksn, t0 + MLA_IDX_STEP, page_nxt)
      if (t0 + 2 * MLA_IDX_STEP < c1) page_nxt = FA_IDX8_PAGE(t0 + 2 * MLA_IDX_STEP);
    }
    if (t0 + 32 * w >= c1) continue;   // wave-uniform: the wave's 32 keys lie past len_b (no barrier in this loop)
    const int key = t0 + kl;
    const mla_i32x8 kb0 = __builtin_bit_cast(mla_i32x8, __builtin_shufflevector(kf[0], kf[1], 0, 1, 2, 3, 4, 5, 6, 7));
    const mla_i32x8 kb1 = __builtin_bit_cast(mla_i32x8, __builtin_shufflevector(kf[2], kf[3], 0, 1, 2, 3, 4, 5, 6, 7));
    for (int t = 0; t < nt; ++t) {
      float sum = 0.f;
      for (int ht = 0; ht < NT; ++ht) {
        lds_char* qp = qs + (t * NT + ht) * MLA_IDX8_QBLOCK + lane * 16;
        const u32x4 q0 = *FA_LDS(u32x4, qp), q1 = *FA_LDS(u32x4, qp + 1024), q2 = *FA_LDS(u32x4, qp + 2048), q3 = *FA_LDS(u32x4, qp + 3072);
        const mla_i32x8 qa0 = __builtin_bit_cast(mla_i32x8, __builtin_shufflevector(q0, q1, 0, 1, 2, 3, 4, 5, 6, 7));
        const mla_i32x8 qa1 = __builtin_bit_cast(mla_i32x8, __builtin_shufflevector(q2, q3, 0, 1, 2, 3, 4, 5, 6, 7));
        // (cbsz = blgp = 0: both operands e4m3; scale operands 0: the instruction's form without block scales)
        f32x16 acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(qa0, kb0, zero16(), 0, 0, 0, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(qa1, kb1, acc, 0, 0, 0, 0, 0, 0);
        lds_char* wp = ws + (t * MLA_IDX_MAX_HI + 32 * ht + 4 * h) * 4;
#pragma unroll
        for (int g = 0; g < 4; ++g) {   // registers 4 g .. 4 g + 3 are the heads 32 ht + 8 g + 4 h .. + 3 (acc_row)
          const f32x4 wv = *FA_LDS(f32x4, wp + 32 * g);
#pragma unroll
          for (int j = 0; j < 4; ++j) sum = __builtin_fmaf(wv[j], fmaxf(acc[4 * g + j], 0.f), sum);
        }
      }
      sum = xhalf_sum(sum) * ks;
      const int i = i0 + t;
      if (h == 0 && key < len)
        a.scores[((size_t)b * a.Nq + i) * a.Ncap + key] = (a.causal && key > len - a.Nq + i) ? -INFINITY : sum;
    }
  }
#undef FA_IDX8_LOAD
#undef FA_IDX8_PAGE
}

// Append: kidx_new bf16 [B][Nq][128] into 144-byte rows (MlaAppendArgs with lanes = B * Nq * 16, as mla_index_append_kernel).  A
// row's 16 lanes sit in one wave and leave together, so the reduction runs among live lanes.
__global__ void __launch_bounds__(256) mla_index_append_fp8_kernel(MlaAppendArgs a) {
  constexpr int CPR = MLA_IDX_D / 8;
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
  char* dst = reinterpret_cast<char*>(a.kv) + dst_row * MLA_IDX8_ROW_BYTES;
  uint32_t sb;
  const mla_u32x2 codes = idx8_quantise(__builtin_bit_cast(bf16x8, reinterpret_cast<const u32x4*>(a.kv_new)[lane]), sb);
  *reinterpret_cast<mla_u32x2*>(dst + 8 * ch) = codes;
  if (ch == 0) *reinterpret_cast<u32x4*>(dst + MLA_IDX8_SCALE_OFF) = u32x4{sb, 0u, 0u, 0u};
}

}  // namespace fa
