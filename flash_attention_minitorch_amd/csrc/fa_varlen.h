// Packed variable-length batches for the training forward and backward on MI355X (gfx950): the kernels of
// libflash_attn_mi355x_varlen.so (include/flash_attn_mi355x_varlen.h).  q / out / dO / dq are [T][H][d], k / v / dk / dv [T][Hkv][d];
// cu_seqlens (int32, nseq + 1 entries, on the device) says which packed rows a sequence owns (seq_rows of fa_common.h).
//
// The attention kernels are the three of fa_window.h, built here under names of their own (varlen_fwd_kernel, varlen_dq_kernel,
// varlen_dkdv_kernel) through that file's hooks.  A workgroup takes (head, map entry) where a window workgroup takes (head, block);
// the entry says which sequence's which block it is.  Everything the body then does, it does to the sequence alone: the bases are
// advanced to the sequence's first row, N is the sequence's length (so the buffer resources end with the sequence and its last tile
// reads zeros, never a neighbour's rows), W and S are clamped to it, positions count from its first row.  A block never straddles
// two sequences.  Hence the law of the header: a sequence's rows are the bits of the window library's call on that sequence alone.
// What the hooks add is wave-uniform: three scalars loaded from the map, folded into the base pointers and the resources.
//
// varlen_schedule_kernel writes the maps (workgroup 0) and zeroes the rows no sequence owns (the other workgroups) in one launch.
#pragma once
#include "fa_rope.h"

namespace fa {

constexpr int VARLEN_QBLOCK = 128;      // query rows per block of the forward and of dQ
constexpr int VARLEN_FILL_BLOCKS = 64;  // workgroups of the schedule launch that zero unowned rows

}  // namespace fa

// A map entry is an int4 (first packed row of the sequence, its length, the block within it, 0); block -1: unused, the workgroup
// returns before its first barrier.  The entry's index depends on blockIdx alone: the load is scalar, and readfirstlane says so.
#ifdef FA_WIN_KERNEL
#error "fa_varlen.h must be included before fa_window.h: it builds that file's kernels under its own hooks"
#endif
#define FA_WIN_KERNEL(stem) varlen_##stem##_kernel
#define FA_WIN_GEOM_PARAMS const int4* __restrict__ map, int Trows, int nblk, int BH
#define FA_WIN_MASK_PARAMS int W_call, int S_call
#define FA_WIN_LOCATE(blk, nb)                                                                       \
  int entry_;                                                                                        \
  map_block(blockIdx.x, BH, nb, bh, entry_);                                                         \
  const int4 ent_ = map[entry_];                                                                     \
  blk = __builtin_amdgcn_readfirstlane(ent_.z);                                                      \
  if (blk < 0) return;                                                                               \
  const int row0_ = __builtin_amdgcn_readfirstlane(ent_.x), N = __builtin_amdgcn_readfirstlane(ent_.y); \
  const int W = min(W_call, N), S = min(S_call, N);
#define FA_WIN_LOCATE_KEYS(blk, nb) FA_WIN_LOCATE(blk, nb)
#define FA_WIN_ROW0 (size_t)row0_
#define FA_WIN_ROWCONST0 ((size_t)bh * Trows + row0_)
#include "fa_window.h"

namespace fa {

// ---- the schedule launch ----------------------------------------------------------------------------------------------------------
// One map for block size bs: for b = 0, 1, ... in order, one entry (s_b, n_b, blk) for each of the ceil(n_b / bs) blocks of
// sequence b (none for n_b = 0), then unused entries up to `cap` = T / bs + nseq.  A sequence of n rows has at most floor(n / bs) + 1
// blocks and, for a non-decreasing cu, the floors sum to at most floor(T / bs): the map holds them all.  For any other cu the
// counts saturate at cap and the entries past it are dropped, so the map is never overrun (ragged_schedule_kernel's rule, whose
// thread-per-run-of-sequences scan this is).  Integer work in a fixed order: the map is a function of cu alone.
FA_DEV void varlen_build_map(const int* cu, int nseq, int T, int4* map, int bs, int cap, int* counts) {
  const int tid = threadIdx.x;
  const int per = (int)(((long)nseq + 255) / 256);
  const int b0 = (int)min((long)tid * per, (long)nseq), b1 = (int)min((long)b0 + per, (long)nseq);
  int n = 0;
  for (int b = b0; b < b1; ++b) {
    int s, nq;
    seq_rows(cu, T, b, s, nq);
    n = min(n + (nq + bs - 1) / bs, cap);
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
    seq_rows(cu, T, b, s, nq);
    const int nb = (nq + bs - 1) / bs;
    for (int blk = 0; blk < nb && off < cap; ++blk, ++off) map[off] = make_int4(s, nq, blk, 0);
  }
  for (int i = total + tid; i < cap; i += 256) map[i] = make_int4(0, 0, -1, 0);
  __syncthreads();   // (counts is used again)
}

// What the launch zeroes: up to three [T][ld] fp32 matrices (rows of ld floats, ld a multiple of 4) and one [H][T] array.
struct VarlenFill {
  float* mat[3];
  int ld[3];
  float* rowc;
  int H;
};

// Rows no sequence owns: those in front of sequence 0 and those behind the last one (consecutive sequences leave no gap: each
// begins at or before the end of the one before it).  u counts them: 0 .. lead - 1, then the tail.
__global__ void __launch_bounds__(256) varlen_schedule_kernel(const int* cu, int nseq, int T, int4* map_q, int cap_q, int4* map_k,
                                                              int bk, int cap_k, VarlenFill f) {
  if (blockIdx.x == 0) {
    __shared__ int counts[256];
    varlen_build_map(cu, nseq, T, map_q, VARLEN_QBLOCK, cap_q, counts);
    if (map_k) varlen_build_map(cu, nseq, T, map_k, bk, cap_k, counts);
    return;
  }
  int lead, n0, sl, nl;
  seq_rows(cu, T, 0, lead, n0);
  seq_rows(cu, T, nseq - 1, sl, nl);
  const int tail0 = sl + nl;
  const long count = (long)lead + (T - tail0);
  if (count <= 0) return;
  const long start = (long)(blockIdx.x - 1) * 256 + threadIdx.x, step = (long)(gridDim.x - 1) * 256;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    if (!f.mat[j]) continue;
    const int vpr = f.ld[j] >> 2;
    for (long i = start; i < count * vpr; i += step) {
      const long u = i / vpr;
      const int col = (int)(i - u * vpr), row = u < lead ? (int)u : tail0 + (int)(u - lead);
      *reinterpret_cast<f32x4*>(f.mat[j] + (size_t)row * f.ld[j] + 4 * col) = zero;
    }
  }
  if (f.rowc)
    for (long i = start; i < count * f.H; i += step) {
      const long hd = i / count, u = i - hd * count;
      const int row = u < lead ? (int)u : tail0 + (int)(u - lead);
      f.rowc[(size_t)hd * T + row] = 0.f;
    }
}

// ---- rope_varlen_kernel: y = rotate(x), x and y [T][H][d]; packed row t of sequence b sits at clamp(t - s_b, 0, max_pos - 1) ----------
// rope_kernel's lanes (RopeLane) under another position rule; a row's sequence is found by the binary search the ragged append
// makes.  A row no sequence owns is copied as bits (RopeLane with nothing to rotate).
struct RopeVarlenArgs {
  const void* x;
  void* y;
  const float* cos;
  const float* sin;
  const int* cu;
  long lanes;   // T * H * (d / E)
  int nseq, T, H, d, rot, max_pos, inverse;
  int cpr;      // d / E: lanes per row
};

template <typename T, int E, bool IL> __global__ void __launch_bounds__(256) rope_varlen_kernel(RopeVarlenArgs a) {
  typedef RopeLane<T, E, IL> L;
  static_assert(E == 1 || E * sizeof(T) == 16, "a lane moves one element or 16 bytes");
  const long lane = (long)blockIdx.x * 256 + threadIdx.x;
  if (lane >= a.lanes) return;
  const long row = lane / a.cpr;   // t * H + h
  const int col = (int)(lane - row * a.cpr) * E;
  const int t = (int)(row / a.H);
  int lo = 0, hi = a.nseq;   // the first b in [0, nseq) with clamp(cu[b + 1]) > t, or nseq: none
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (min(max(a.cu[mid + 1], 0), a.T) > t) hi = mid; else lo = mid + 1;
  }
  int pos = 0;
  bool owned = false;
  if (lo < a.nseq) {
    int s, n;
    seq_rows(a.cu, a.T, lo, s, n);
    owned = t >= s && t < s + n;
    pos = t - s;
  }
  const int p = owned ? min(max(pos, 0), a.max_pos - 1) : 0;
  const size_t tab = (size_t)p * (a.rot >> 1);
  typename L::vec va, vb;
  int gap;
  const size_t off = (size_t)row * a.d;
  const int n = L::run(reinterpret_cast<const typename L::U*>(a.x) + off, col, owned ? a.rot : 0, a.cos + tab, a.sin + tab, a.inverse != 0,
                       va, vb, gap);
  typename L::U* dst = reinterpret_cast<typename L::U*>(a.y) + off + col;
  if (n >= 1) *reinterpret_cast<typename L::vec*>(dst) = va;
  if (n == 2) *reinterpret_cast<typename L::vec*>(dst + gap) = vb;
}

}  // namespace fa
