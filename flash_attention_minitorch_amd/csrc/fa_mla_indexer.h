// The lightning indexer of DeepSeek-V3.2 sparse attention (DSA) for MI355X (gfx950): it produces the per-query top-k index lists that
// fa_mla_sparse.h attends.  Declared in include/flash_attn_mi355x_mla_indexer.h, dispatched by fa_mla.hip into the same library.  The
// atoms, make_rsrc, clamp_len and MlaAppendArgs are fa_atoms.h's, fa_decode.h's and fa_mla.h's, used as they are: this header changes
// no definition of theirs.
//
// Index keys are bf16 rows of 128 columns, one per cached token, in a slab [B][Ncap][128] or a pool [num_pages][page_size][128] under
// the latent cache's block table.  With q_idx [B][Nq][HI][128] bf16 and weights [B][Nq][HI] fp32 the score of token (b, i) for
// position s is  I[b,i,s] = sum_h w[b,i,h] * max(0, q_idx[b,i,h,:] . kidx[b,s,:]);  s is ADMITTED iff 0 <= s < len_b and, under
// `causal`, s <= len_b - Nq + i.  scores [B][Nq][Ncap] fp32: a position below len_b gets its score, or -inf when it is not admitted;
// positions at or past len_b are neither read nor written.
//
// mla_index_scores_kernel<PAGED>: 256 threads; a workgroup = (batch b, group of up to 4 query tokens, chunk of keys); its four waves
// take the four 32-key tiles of each 128-key step of the chunk.  Nothing is shared between waves but Q, so the loop has no barrier.
//   * Orientation: heads are the MFMA's M rows (A operand = Q_idx), keys its N columns (B operand).  In the 32 x 32 accumulator a
//     lane owns ONE key and 16 heads, so ReLU and the weighted head sum are 16 in-lane FMAs per 32-head tile, the tiles accumulate
//     in-lane, and one lane <-> lane + 32 add per token finishes the sum (the same add order in every build: paged = slab in bits).
//   * Keys need no LDS.  A dot product does not care about the order of its 128 terms: lane half h takes columns 64 h .. 64 h + 63 of
//     its key's row (k-step kc = columns 64 h + 8 kc .. + 7), and Q is permuted the same way.  A lane streams 128 contiguous bytes of
//     one row as eight 16-byte loads straight into MFMA fragments; the next tile's eight loads are issued in front of this tile's
//     MFMAs.  Slab: buffer loads whose resource ends at len_b, so rows past it read as zero.  Paged: 64-bit global loads through the
//     tile's page id (requested one tile further ahead, clamped to the pool); a lane whose key is at or past len_b loads nothing.
//   * Q_idx of the group's tokens lies in LDS in fragment order (64 KB: 8 blocks of 32 heads x 128 columns; HI <= 64: 4 tokens,
//     HI <= 128: 2), the weights beside it (2 KB); heads past HI are zero rows with zero weights.  Every MFMA reads its A fragment with
//     one ds_read_b128 and a tile's key fragments are reused by every token of the group.  More tokens than a group holds: further
//     workgroups, which read the keys again.
//   * The causal bound turns a score into -inf on the store; lane half 0 stores 32 consecutive floats per token.
// mla_index_topk_kernel: one workgroup of 1024 threads per (b, i) row; a radix select over the order-preserving unsigned image of the
// fp32 score (-0 counts as +0; NaN and -inf are never selected).  Three histogram passes (11, 11 and 10 bits, LDS bins, integer
// atomics whose result does not depend on order) find the k-th largest image T and how many entries equal to T still fit; `admitted
// <= topk` is seen after the first pass and takes everything.  Then two passes compact by prefix sums alone: wave w owns a contiguous
// span of the row, the spans' counts are summed in wave order, and each wave walks its span again, placing the entries above T and
// the first ties in ascending position by a wave-level scan.  The list is ascending, the rest is -1, and it is a pure function of
// the score bits.  The row (128 KB at 32768 entries) is read five times, from L2.
// mla_index_append_kernel: mla_append_kernel's rule on 128-wide rows (token i of batch element b goes to row len_b - Nq + i).
//
// FP8 index keys (144-byte rows, fp8 matrix instructions) are fa_mla_indexer_fp8.h's kernels, under this header's policy and top-k.
// Not built: a fused score + select launch, index dims other than 128, an indexer for prefill / extend, training.
#pragma once
#include "fa_mla.h"

namespace fa {

constexpr int MLA_IDX_D = 128, MLA_IDX_ROW_BYTES = MLA_IDX_D * 2;
constexpr int MLA_IDX_STEP = 128;         // keys per workgroup step: four waves of 32
constexpr int MLA_IDX_MAX_HI = 128;
constexpr int MLA_IDX_QBLOCKS = 8;        // 32-head blocks of Q (8 KB each) a workgroup holds: tokens per group * ceil(HI / 32)
constexpr int MLA_IDX_MAX_GROUP = 4;      // tokens per group at most

struct MlaIndexArgs {
  const void* q;        // [B][Nq][HI][128] bf16
  const float* w;       // [B][Nq][HI]
  const void* k;        // slab [B][Ncap][128] or pool [num_pages][page_size][128]
  float* scores;        // [B][Nq][Ncap]
  const int* seqlens;   // [B] or null (= Ncap)
  const int* table;     // [B][max_pages] (paged builds)
  int HI, Nq, Ncap, chunk, nchunk, group, ngroups, page_size, num_pages, max_pages, causal;
};

template <bool PAGED>
__global__ void __launch_bounds__(256) mla_index_scores_kernel(MlaIndexArgs a) {
  using A = Atom<bf16_t>;
  typedef A::frag frag;
  constexpr int QB = MLA_IDX_QBLOCKS * 8 * 1024, WB = MLA_IDX_MAX_GROUP * MLA_IDX_MAX_HI * 4;
  __shared__ __attribute__((aligned(16))) char smem_raw[QB + WB];
  lds_char* qs = (lds_char*)smem_raw;   // [token][head tile][k-step][lane] fragments
  lds_char* ws = qs + QB;               // [token][128] weights

  const int id = blockIdx.x;
  const int chunk = id % a.nchunk, rest = id / a.nchunk, grp = rest % a.ngroups, b = rest / a.ngroups;
  const int len = __builtin_amdgcn_readfirstlane(clamp_len(a.seqlens, a.Ncap, b));
  const int c0 = chunk * a.chunk, c1 = min(c0 + a.chunk, len);
  if (c0 >= c1) return;   // (a chunk wholly past len_b reads and writes nothing; workgroup-uniform, in front of the barrier)

  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int NT = (a.HI + 31) >> 5, hpad = 32 * NT;
  const int i0 = grp * a.group, nt = min(a.group, a.Nq - i0);

  // Q of the group's tokens into fragment order: 16-byte chunk c = 8 h + kc of head hl goes to block (t, hl >> 5), k-step kc, lane
  // 32 h + (hl & 31).  Heads past HI get the resource's size as their offset and read as zero.
  const uint32_t q_bytes = (uint32_t)a.Nq * a.HI * MLA_IDX_ROW_BYTES;
  const rsrc_t qrs = make_rsrc(reinterpret_cast<const char*>(a.q) + (size_t)b * q_bytes, q_bytes);
  for (int idx = tid; idx < nt * hpad * 16; idx += 256) {
    const int c = idx & 15, row = idx >> 4, t = row / hpad, hl = row - t * hpad;
    const int off = hl < a.HI ? (((i0 + t) * a.HI + hl) * 16 + c) * 16 : (int)q_bytes;
    const u32x4 v = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(qrs, off, 0, 0));
    *FA_LDS(u32x4, qs + ((((t * NT + (hl >> 5)) * 8 + (c & 7)) * 64) + 32 * (c >> 3) + (hl & 31)) * 16) = v;
  }
  for (int idx = tid; idx < nt * MLA_IDX_MAX_HI; idx += 256) {
    const int t = idx >> 7, hl = idx & 127;
    *FA_LDS(float, ws + idx * 4) = hl < a.HI ? a.w[((size_t)b * a.Nq + i0 + t) * a.HI + hl] : 0.f;
  }
  __syncthreads();

  // the slab's resource ends at len_b (unused by a paged build)
  const rsrc_t krs = make_rsrc(reinterpret_cast<const char*>(a.k) + (PAGED ? 0 : (size_t)b * a.Ncap * MLA_IDX_ROW_BYTES),
                               (uint32_t)len * MLA_IDX_ROW_BYTES);
  const char* pool = reinterpret_cast<const char*>(a.k);
  const int* trow = a.table + (PAGED ? (size_t)b * a.max_pages : 0);
  const int kl = 32 * w + r;   // the lane's key inside a step

  // The wave's tile of the step at key t_ into dst: the lane's key row, columns 64 h ..; page_: the step's page id (paged builds).
#define FA_IDX_LOAD(dst, t_, page_)                                                                                       \
  {                                                                                                                       \
    const int key_ = (t_) + kl;                                                                                           \
    if constexpr (PAGED) {                                                                                                \
      if (key_ < len) {                                                                                                   \
        const char* p_ = pool + ((size_t)(page_) * a.page_size + ((t_) % a.page_size + kl)) * MLA_IDX_ROW_BYTES + 128 * h; \
        _Pragma("unroll") for (int kc = 0; kc < 8; ++kc) dst[kc] = *reinterpret_cast<const frag*>(p_ + 16 * kc);          \
      } else {                                                                                                            \
        _Pragma("unroll") for (int kc = 0; kc < 8; ++kc) dst[kc] = A::zero();                                             \
      }                                                                                                                   \
    } else {                                                                                                              \
      _Pragma("unroll") for (int kc = 0; kc < 8; ++kc)                                                                    \
        dst[kc] = load_frag_buf<bf16_t>(krs, key_ * MLA_IDX_ROW_BYTES + 128 * h + 16 * kc);                               \
    }                                                                                                                     \
  }
#define FA_IDX_PAGE(t_) (PAGED ? min(max(trow[(t_) / a.page_size], 0), a.num_pages - 1) : 0)

  frag kf[8], kn[8];
  int page_nxt = FA_IDX_PAGE(c0);
  FA_IDX_LOAD(kn, c0, page_nxt)
  if (c0 + MLA_IDX_STEP < c1) page_nxt = FA_IDX_PAGE(c0 + MLA_IDX_STEP);
  for (int t0 = c0; t0 < c1; t0 += MLA_IDX_STEP) {
#pragma unroll
    for (int kc = 0; kc < 8; ++kc) kf[kc] = kn[kc];
    if (t0 + MLA_IDX_STEP < c1) {
      FA_IDX_LOAD(kn, t0 + MLA_IDX_STEP, page_nxt)
      if (t0 + 2 * MLA_IDX_STEP < c1) page_nxt = FA_IDX_PAGE(t0 + 2 * MLA_IDX_STEP);
    }
    if (t0 + 32 * w >= c1) continue;   // wave-uniform: the wave's 32 keys lie past len_b (no barrier in this loop)
    const int key = t0 + kl;
    for (int t = 0; t < nt; ++t) {
      float sum = 0.f;
      for (int ht = 0; ht < NT; ++ht) {
        f32x16 acc = zero16();
        lds_char* qp = qs + (t * NT + ht) * 8 * 1024 + lane * 16;
#pragma unroll
        for (int kc = 0; kc < 8; ++kc) {
          const frag qa = *FA_LDS(frag, qp + kc * 1024);
          A::mma(acc, qa, kf[kc]);
        }
        lds_char* wp = ws + (t * MLA_IDX_MAX_HI + 32 * ht + 4 * h) * 4;
#pragma unroll
        for (int g = 0; g < 4; ++g) {   // registers 4 g .. 4 g + 3 are the heads 32 ht + 8 g + 4 h .. + 3 (acc_row)
          const f32x4 wv = *FA_LDS(f32x4, wp + 32 * g);
#pragma unroll
          for (int j = 0; j < 4; ++j) sum = __builtin_fmaf(wv[j], fmaxf(acc[4 * g + j], 0.f), sum);
        }
      }
      sum = xhalf_sum(sum);
      const int i = i0 + t;
      if (h == 0 && key < len)
        a.scores[((size_t)b * a.Nq + i) * a.Ncap + key] = (a.causal && key > len - a.Nq + i) ? -INFINITY : sum;
    }
  }
#undef FA_IDX_LOAD
#undef FA_IDX_PAGE
}

// ---- top-k ----
constexpr int MLA_TOPK_THREADS = 1024, MLA_TOPK_WAVES = MLA_TOPK_THREADS / 64, MLA_TOPK_BINS = 2048;

struct MlaTopkArgs {
  const float* scores;   // [B][Nq][Ncap]
  int* indices;          // [B][Nq][topk]
  const int* seqlens;
  int Nq, Ncap, topk;
};

// The order-preserving unsigned image of a score (larger score, larger image; -0 is +0), and which scores can be selected at all.
FA_DEV uint32_t score_image(float x) {
  const uint32_t b = __float_as_uint(x), u = (b & 0x7fffffffu) == 0 ? 0u : b;
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
// (on the bits: neither a NaN, whatever the compiler may assume about float compares, nor -inf)
FA_DEV bool score_valid(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x7fffffffu) <= 0x7f800000u && u != 0xff800000u;
}

// Four consecutive entries of a row from position p; positions at or past n read as -inf (never selected).  vec: rows are 16-byte aligned.
FA_DEV void topk_load4(const float* row, int p, int n, bool vec, float (&x)[4]) {
  if (vec && p + 4 <= n) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + p);
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = v[e];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = p + e < n ? row[p + e] : -INFINITY;
  }
}

// One count into an LDS bin per active lane.  Scores cluster, so the first digits of a wave's 64 entries fall into a few bins, and
// atomics on one address serialise: up to four rounds in which the first remaining lane's bin is counted once for all its lanes,
// then plain atomics for what is left.  Called by whole waves.
FA_DEV void hist_add(int* hist, int bin, bool active, int lane) {
  uint64_t rem = __ballot(active);
  for (int it = 0; it < 4 && rem != 0; ++it) {
    const int leader = __ffsll((long long)rem) - 1;
    const int lb = __shfl(bin, leader);
    const uint64_t m = __ballot(active && bin == lb) & rem;
    if (lane == leader) atomicAdd(&hist[lb], __popcll(m));
    rem &= ~m;
  }
  if ((rem >> lane) & 1) atomicAdd(&hist[bin], 1);
}

FA_DEV int wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d);
    if (lane >= d) v += o;
  }
  return v;
}

// Exclusive prefix sum of v over the workgroup's threads, and the total.  wsum: MLA_TOPK_WAVES ints of LDS.
FA_DEV int block_excl_scan(int v, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int inc = wave_incl_scan(v, lane);
  __syncthreads();   // (an earlier use of wsum is over)
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  int before = 0;
  total = 0;
  for (int j = 0; j < MLA_TOPK_WAVES; ++j) {
    const int s = wsum[j];
    before += j < w ? s : 0;
    total += s;
  }
  return before + inc - v;
}

__global__ void __launch_bounds__(MLA_TOPK_THREADS) mla_index_topk_kernel(MlaTopkArgs a) {
  __shared__ int hist[MLA_TOPK_BINS];
  __shared__ int wsum[MLA_TOPK_WAVES], wsum2[MLA_TOPK_WAVES], res[2];
  const int row = blockIdx.x, b = row / a.Nq;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n = clamp_len(a.seqlens, a.Ncap, b);
  const float* src = a.scores + (size_t)row * a.Ncap;
  int* dst = a.indices + (size_t)row * a.topk;
  const bool vec = (a.Ncap & 3) == 0;
  // wave w owns the positions [w0, w1): whole 256-entry steps, in which lane l reads the entries 4 l .. 4 l + 3 of the step
  const int span = ((n + MLA_TOPK_WAVES - 1) / MLA_TOPK_WAVES + 255) / 256 * 256;
  const int w0 = min(w * span, n), w1 = min(w0 + span, n);

  // ---- the k-th largest image T, most significant digit first; `need` entries equal to T are taken ----
  uint32_t prefix = 0;
  int need = a.topk;
  bool all = false;   // admitted <= topk: every selectable entry is taken
  for (int pass = 0; pass < 3 && !all; ++pass) {
    const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0, bits = pass == 2 ? 10 : 11, nb = 1 << bits;
    for (int j = tid; j < MLA_TOPK_BINS; j += MLA_TOPK_THREADS) hist[j] = 0;
    __syncthreads();
    for (int base = w0; base < w1; base += 256) {
      float x[4];
      topk_load4(src, base + 4 * lane, n, vec, x);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t u = score_image(x[e]);
        const bool ok = score_valid(x[e]) && (uint32_t)((uint64_t)u >> (shift + bits)) == prefix;
        hist_add(hist, (int)((u >> shift) & (nb - 1)), ok, lane);
      }
    }
    __syncthreads();
    // thread t owns the bins nb - 1 - 2 t and the one below: a prefix sum in thread order counts the entries in higher bins
    const int j0 = nb - 1 - 2 * tid;
    const int n0 = j0 >= 0 ? hist[j0] : 0, n1 = j0 >= 1 ? hist[j0 - 1] : 0;
    int total;
    const int above = block_excl_scan(n0 + n1, wsum, total);
    if (pass == 0 && total <= a.topk) {   // (workgroup-uniform)
      all = true;
      break;
    }
    if (above < need && need <= above + n0) res[0] = j0, res[1] = need - above;
    else if (above + n0 < need && need <= above + n0 + n1) res[0] = j0 - 1, res[1] = need - above - n0;
    __syncthreads();
    prefix = (prefix << bits) | (uint32_t)res[0];
    need = res[1];
    __syncthreads();   // (res and hist are read; the next pass clears hist)
  }
  const uint32_t T = prefix;
  if (all) need = 0;

  // ---- compaction by prefix sums: the spans' counts in wave order, then each wave's walk over its span ----
  int cg = 0, ce = 0;
  for (int base = w0; base < w1; base += 256) {
    float x[4];
    topk_load4(src, base + 4 * lane, n, vec, x);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t u = score_image(x[e]);
      const bool ok = score_valid(x[e]);
      cg += ok && (all || u > T);
      ce += ok && !all && u == T;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    cg += __shfl_xor(cg, d);
    ce += __shfl_xor(ce, d);
  }
  __syncthreads();   // (the last scan's reads of wsum are over)
  if (lane == 0) wsum[w] = cg, wsum2[w] = ce;
  __syncthreads();
  int run_g = 0, run_e = 0, tot_g = 0, tot_e = 0;   // entries above T and ties in front of this wave's span; in the whole row
  for (int j = 0; j < MLA_TOPK_WAVES; ++j) {
    run_g += j < w ? wsum[j] : 0;
    run_e += j < w ? wsum2[j] : 0;
    tot_g += wsum[j];
    tot_e += wsum2[j];
  }
  for (int base = w0; base < w1; base += 256) {
    float x[4];
    topk_load4(src, base + 4 * lane, n, vec, x);
    bool g[4], q[4];
    int packed = 0;   // entries above T in the low half, ties in the high half (at most 256 of either in a step)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t u = score_image(x[e]);
      const bool ok = score_valid(x[e]);
      g[e] = ok && (all || u > T);
      q[e] = ok && !all && u == T;
      packed += (int)g[e] + ((int)q[e] << 16);
    }
    const int inc = wave_incl_scan(packed, lane), excl = inc - packed;
    int rank = run_e + (excl >> 16);                               // ties in front of the lane's entries
    int out = run_g + (excl & 0xffff) + min(rank, need);           // selected entries in front of them
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if ((g[e] || (q[e] && rank < need)) && out < a.topk) dst[out++] = base + 4 * lane + e;
      rank += q[e];
    }
    const int tot = __shfl(inc, 63);
    run_g += tot & 0xffff;
    run_e += tot >> 16;
  }
  for (int j = tot_g + min(tot_e, need) + tid; j < a.topk; j += MLA_TOPK_THREADS) dst[j] = -1;
}

// Append: kidx_new [B][Nq][128] into the index-key cache by mla_append_kernel's rule (its argument, with lanes = B * Nq * 16).
__global__ void __launch_bounds__(256) mla_index_append_kernel(MlaAppendArgs a) {
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
  reinterpret_cast<u32x4*>(a.kv)[dst_row * CPR + ch] = reinterpret_cast<const u32x4*>(a.kv_new)[lane];
}

}  // namespace fa
