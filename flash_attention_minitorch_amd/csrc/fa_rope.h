// Rotary position embeddings (RoPE) for the KV-cache calls (include/flash_attn_mi355x_decode_rope.h): rope_kernel rotates a tensor,
// rope_append_kernel does in ONE launch what a roped fused call needs in front of the attention: q rotated into q_rot, k_new rotated
// into the K cache, v_new copied into the V cache.  The attention kernels are not touched: a roped call runs them on q_rot.
//
// One definition, used by every build (rope_rotate): for a row at position p and pair j, c = cos[p][j], s = sin[p][j] (fp32 tables
// [max_pos][rot / 2]; the index is clamp(p, 0, max_pos - 1), on the device),
//     y1 = x1 * c - x2 * s,   y2 = x2 * c + x1 * s        (inverse: -s)
// evaluated in fp32 as ONE product and ONE fused multiply-add each, written out, so that contraction cannot differ between builds, and
// rounded once (to nearest even) to the tensor's type.  Pair j of a row is (x[j], x[j + rot/2]) (NeoX / Llama) or (x[2j], x[2j+1])
// (interleaved: GPT-J).  Columns >= rot are copied as bits.
//
// Lanes.  A lane = E consecutive elements of one row: E = 16 bytes' worth (the host picks it when rot, the row lengths and the
// pointers allow: RopeLane below) or E = 1.  A lane owns BOTH members of its pairs, so y may alias x: interleaved with E > 1 both
// sit in its vector; otherwise the lane at column c < gap of the rotary part also loads and stores the matching vector at c + gap
// (gap = rot / 2, NeoX; gap = 1 for the interleaved element build, where the odd columns' lanes have nothing to do) and the lane
// at c + gap leaves K alone.  Consecutive lanes walk the sources in memory order.  No LDS, no scratch, 256-thread workgroups.
#pragma once
#include "fa_decode.h"

namespace fa {

// THE rotation: two roundings per result in fp32 (the product, then the fused multiply-add).
FA_DEV void rope_rotate(float x1, float x2, float c, float s, float& y1, float& y2) {
  const float x2s = x2 * s, x1s = x1 * s;
  y1 = __builtin_fmaf(x1, c, -x2s);
  y2 = __builtin_fmaf(x2, c, x1s);
}

// an element as its bits, and the one rounding to its type
template <typename T> struct RopeElem;
template <> struct RopeElem<bf16_t> {
  typedef uint16_t U;
  static FA_DEV float up(uint16_t u) { return __builtin_bit_cast(float, (uint32_t)u << 16); }
  static FA_DEV uint16_t down(float f) { return __builtin_bit_cast(uint16_t, (bf16_t)f); }
};
template <> struct RopeElem<float> {
  typedef uint32_t U;
  static FA_DEV float up(uint32_t u) { return __builtin_bit_cast(float, u); }
  static FA_DEV uint32_t down(float f) { return __builtin_bit_cast(uint32_t, f); }
};

// NT consecutive table entries (the host has checked their alignment where NT > 1)
template <int NT> FA_DEV void rope_table(const float* p, float (&o)[NT]) {
  if constexpr (NT % 4 == 0) {
#pragma unroll
    for (int i = 0; i < NT / 4; ++i) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(p + 4 * i);
      o[4 * i] = v[0], o[4 * i + 1] = v[1], o[4 * i + 2] = v[2], o[4 * i + 3] = v[3];
    }
  } else if constexpr (NT == 2) {
    const f32x2 v = *reinterpret_cast<const f32x2*>(p);
    o[0] = v[0], o[1] = v[1];
  } else {
    static_assert(NT == 1, "a lane reads 1, 2, 4 or 8 table entries");
    o[0] = p[0];
  }
}

// One lane's share of one source row (src: the row's first element): the E elements at column col, rotated or (col >= rot) copied.
// Returns the number of vectors the lane owns: 0 (a column whose pair another lane owns), 1 (`a`, for column col) or 2 (`a`, and
// `b` for column col + gap).  cs / sn: the table rows of the row's position.  The caller has col + E <= the row's length.
template <typename T, int E, bool IL> struct RopeLane {
  typedef RopeElem<T> R;
  typedef typename R::U U;
  typedef __attribute__((ext_vector_type(E))) U vec;
  static FA_DEV int run(const void* src_row, int col, int rot, const float* cs, const float* sn, bool inverse, vec& a, vec& b, int& gap) {
    const U* s = reinterpret_cast<const U*>(src_row);
    gap = 0;
    if (col >= rot) {
      a = *reinterpret_cast<const vec*>(s + col);
      return 1;
    }
    if constexpr (IL && E > 1) {   // E / 2 whole pairs inside the vector
      a = *reinterpret_cast<const vec*>(s + col);
      float c[E / 2], sg[E / 2];
      rope_table<E / 2>(cs + (col >> 1), c);
      rope_table<E / 2>(sn + (col >> 1), sg);
#pragma unroll
      for (int e = 0; e < E / 2; ++e) {
        float y1, y2;
        rope_rotate(R::up(a[2 * e]), R::up(a[2 * e + 1]), c[e], inverse ? -sg[e] : sg[e], y1, y2);
        a[2 * e] = R::down(y1);
        a[2 * e + 1] = R::down(y2);
      }
      return 1;
    } else {
      gap = IL ? 1 : rot >> 1;
      if (IL ? (col & 1) != 0 : col >= gap) return 0;
      const int j = IL ? col >> 1 : col;
      a = *reinterpret_cast<const vec*>(s + col);
      b = *reinterpret_cast<const vec*>(s + col + gap);
      float c[E], sg[E];
      rope_table<E>(cs + j, c);
      rope_table<E>(sn + j, sg);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        float y1, y2;
        rope_rotate(R::up(a[e]), R::up(b[e]), c[e], inverse ? -sg[e] : sg[e], y1, y2);
        a[e] = R::down(y1);
        b[e] = R::down(y2);
      }
      return 2;
    }
  }
};

// ---- rope_kernel: y = rotate(x), x and y [B][N][H][d] (bnhd) or [B][H][N][d]; row (b, i) sits at clamp(off_b + i, 0, max_pos - 1) ----
struct RopeArgs {
  const void* x;
  void* y;
  const float* cos;
  const float* sin;
  const int* offsets;   // [B] or null (all zero)
  long lanes;           // B * N * H * (d / E)
  int N, H, d, rot, max_pos, bnhd, inverse;
  int cpr;              // d / E: lanes per row
};

template <typename T, int E, bool IL> __global__ void __launch_bounds__(256) rope_kernel(RopeArgs a) {
  typedef RopeLane<T, E, IL> L;
  static_assert(E == 1 || E * sizeof(T) == 16, "a lane moves one element or 16 bytes");
  const long lane = (long)blockIdx.x * 256 + threadIdx.x;
  if (lane >= a.lanes) return;
  const long row = lane / a.cpr;
  const int col = (int)(lane - row * a.cpr) * E;
  const long outer = a.bnhd ? row / a.H : row;             // b * N + i, or (b * H + h) * N + i
  const int i = (int)(outer % a.N);
  const int b = (int)(row / ((long)a.N * a.H));
  const long pos = (long)(a.offsets ? a.offsets[b] : 0) + i;
  const int p = pos < 0 ? 0 : pos >= a.max_pos ? a.max_pos - 1 : (int)pos;
  const size_t tab = (size_t)p * (a.rot >> 1);
  typename L::vec va, vb;
  int gap;
  const size_t off = (size_t)row * a.d;
  const int n = L::run(reinterpret_cast<const typename L::U*>(a.x) + off, col, a.rot, a.cos + tab, a.sin + tab, a.inverse != 0, va, vb, gap);
  typename L::U* dst = reinterpret_cast<typename L::U*>(a.y) + off + col;
  if (n >= 1) *reinterpret_cast<typename L::vec*>(dst) = va;
  if (n == 2) *reinterpret_cast<typename L::vec*>(dst + gap) = vb;
}

// ---- rope_append_kernel: q -> q_rot, k_new -> K cache (both rotated), v_new -> V cache (copied) ----
// The AppendArgs part is the append's own (lanes: those of the new k / v rows, 0 without them); the first q_lanes lanes take q.
struct RopeAppendArgs : AppendArgs {
  const void* q;          // [B][Nq][H][d] / [B][H][Nq][d], ragged [ntok][H][d]; null: append only
  void* q_rot;
  const float* cos;
  const float* sin;
  const float* k_scale;   // FP8 builds: [Hkv] or null (all ones)
  const float* v_scale;
  long q_lanes;           // q rows * (d / E)
  int H, d, rot, max_pos;
  const int* cu;          // RAGGED builds, as RaggedAppendArgs
  int nseq, ntok;
};

// E elements of bf16 bits into the e4m3 bytes at dst, by append_fp8_kernel's rule
template <int E, typename V> FA_DEV void rope_store_fp8(uint8_t* dst, const V& v, float rcp) {
  typedef RopeElem<bf16_t> R;
  if constexpr (E == 8) {
    typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
    u32x2 w;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      w[j] = fp8_pack2(R::up(v[4 * j]), R::up(v[4 * j + 1]), rcp, 0u, false);
      w[j] = fp8_pack2(R::up(v[4 * j + 2]), R::up(v[4 * j + 3]), rcp, w[j], true);
    }
    *reinterpret_cast<u32x2*>(dst) = w;
  } else {
    const float x = R::up(v[0]);
    *dst = (uint8_t)fp8_pack2(x, x, rcp, 0u, false);
  }
}

// Placement is decode_append_kernel's: token i of batch element b goes to cache row L_b - nq + i (nothing below row 0), columns
// d_new .. d-1 of a written row become zeros, a paged row is looked up with the page id clamped to the pool; RAGGED: the sources are
// packed and a row's sequence is found by the binary search of cu that the ragged append makes; rows no sequence owns are neither
// read nor written, in the caches and in q_rot.  The same position serves the token's query row, which is written even where
// L_b - nq + i < 0 (rotated at the clamped position).  FP8 (bf16 sources, byte caches): the rotated k is rounded to bf16, then
// quantised as append_fp8_kernel quantises; v as there.
template <typename T, int E, bool IL, bool PAGED = false, bool RAGGED = false, bool FP8 = false>
__global__ void __launch_bounds__(256) rope_append_kernel(RopeAppendArgs a) {
  typedef RopeLane<T, E, IL> L;
  typedef typename L::U U;
  typedef typename L::vec vec;
  static_assert(E == 1 || E * sizeof(T) == 16, "a lane moves one element or 16 bytes");
  static_assert(!FP8 || (sizeof(T) == 2 && !RAGGED), "fp8 caches: bf16 sources, uniform batches");
  long lane = (long)blockIdx.x * 256 + threadIdx.x;
  if (lane >= a.q_lanes + a.lanes) return;
  const bool isq = lane < a.q_lanes;
  if (!isq) lane -= a.q_lanes;
  const long row = lane >> a.ch_shift;           // source row (b, i, h) or (b, h, i); ragged (t, h)
  const int col = (int)(lane - (row << a.ch_shift)) * E;
  const int heads = isq ? a.H : a.Hkv;
  int b_, i_, h_, nq_ = a.Nq;
  if constexpr (RAGGED) {
    const int t = (int)(row / heads);
    h_ = (int)(row - (long)t * heads);
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
    const int inner = a.bnhd ? heads : a.Nq;
    const long outer = row / inner;
    const int in = (int)(row - outer * inner);
    const int mid = a.bnhd ? a.Nq : heads;
    b_ = (int)(outer / mid);
    const int md = (int)(outer - (long)b_ * mid);
    i_ = a.bnhd ? md : in;
    h_ = a.bnhd ? in : md;
  }
  const int b = b_, i = i_, h = h_;
  const int pos = clamp_len(a.seqlens, a.Ncap, b) - nq_ + i;
  const size_t tab = (size_t)min(max(pos, 0), a.max_pos - 1) * (a.rot >> 1);
  vec va = {}, vb = {};
  int gap = 0;
  if (isq) {
    const size_t off = (size_t)row * a.d;
    const int n = L::run(reinterpret_cast<const U*>(a.q) + off, col, a.rot, a.cos + tab, a.sin + tab, false, va, vb, gap);
    U* dst = reinterpret_cast<U*>(a.q_rot) + off + col;
    if (n >= 1) *reinterpret_cast<vec*>(dst) = va;
    if (n == 2) *reinterpret_cast<vec*>(dst + gap) = vb;
    return;
  }
  if (pos < 0) return;
  size_t dst;
  if constexpr (PAGED) {
    const int slot = pos / a.page_size;
    const int page = min(max(a.table[(size_t)b * a.max_pages + slot], 0), a.num_pages - 1);
    dst = (size_t)page * a.page_stride + (size_t)h * a.kv_hstride + (size_t)(pos - slot * a.page_size) * a.kv_ld + col;
  } else {
    dst = (size_t)b * a.kv_bstride + (size_t)h * a.kv_hstride + (size_t)pos * a.kv_ld + col;
  }
  vec vv = {};
  int n = 1;   // (a lane at or past d_new owns the zeros of its columns)
  if (col < a.d_new) {   // (E > 1: d_new is a multiple of E, so the whole lane is inside the row)
    const size_t src = (size_t)row * a.d_new;
    n = L::run(reinterpret_cast<const U*>(a.k_new) + src, col, a.rot, a.cos + tab, a.sin + tab, false, va, vb, gap);
    vv = *reinterpret_cast<const vec*>(reinterpret_cast<const U*>(a.v_new) + src + col);
  }
  if constexpr (FP8) {
    const float rk = 1.0f / scale_of(a.k_scale, h), rv = 1.0f / scale_of(a.v_scale, h);
    uint8_t* kd = reinterpret_cast<uint8_t*>(a.k) + dst;
    uint8_t* vd = reinterpret_cast<uint8_t*>(a.v) + dst;
    if (col < a.d_new) {
      if (n >= 1) rope_store_fp8<E>(kd, va, rk);
      if (n == 2) rope_store_fp8<E>(kd + gap, vb, rk);
      rope_store_fp8<E>(vd, vv, rv);
    } else if constexpr (E == 8) {   // (zero BYTES, whatever the scales)
      *reinterpret_cast<uint2*>(kd) = make_uint2(0u, 0u);
      *reinterpret_cast<uint2*>(vd) = make_uint2(0u, 0u);
    } else {
      *kd = 0;
      *vd = 0;
    }
  } else {
    U* kd = reinterpret_cast<U*>(a.k) + dst;
    if (n >= 1) *reinterpret_cast<vec*>(kd) = va;
    if (n == 2) *reinterpret_cast<vec*>(kd + gap) = vb;
    *reinterpret_cast<vec*>(reinterpret_cast<U*>(a.v) + dst) = vv;
  }
}

}  // namespace fa
