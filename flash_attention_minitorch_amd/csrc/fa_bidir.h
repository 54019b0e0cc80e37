// Bidirectional packed attention with one cu_seqlens for the queries and one for the keys, forward and backward, on MI355X (gfx950):
// the kernels of libflash_attn_mi355x_bidir.so (include/flash_attn_mi355x_bidir.h), written against fa_atoms.h.  q / out / dO / dq are
// [Tq][H][d], k / v / dk / dv [Tk][Hkv][d]; sequence b owns n_q rows of the first buffers and n_k rows of the second, and every query
// of it admits every key of it: encoder self-attention on packed documents (the two arrays are one) and cross-attention.
//
// The three attention kernels have the phased structure of fa_window.h's: the query (forward, dQ) or the key (dK/dV) on the lane, the
// other operand staged through LDS in double-buffered tiles, tau*log2(e) applied to every score in fp32.  What differs:
//   * A workgroup takes (head, map entry); the entry names its sequence's rows in BOTH buffers.  The Q / dO / row-constant resources
//     end with the sequence's n_q rows and the K / V resources with its n_k rows.  Every tile's row offset rides in the VECTOR offset
//     of its loads, which the resource's range check covers (the scalar offset is not checked): a last tile reads zeros, never a
//     neighbour's rows, and no access leaves the buffers whatever the arrays hold.
//   * No diagonal and no window: a query block walks all ceil(n_k / BN) key tiles, a key block sweeps all ceil(n_q / QS) query slices.
//     Only the sub-tile that holds the key tail j >= n_k is masked per element, by a wave-uniform test.  (dK/dV needs no mask at all:
//     a key is a lane there, and the lanes at or past n_k are not stored; query rows at or past n_q are zeros in Q and dO and add
//     nothing.)
//   * bf16: a sequence with n_k < 64 takes P and dS into the second product as two bf16 fragments (Atom::pack_lo), the project's rule
//     for rows that admit fewer than 64 keys; wave-uniform, since a block never straddles sequences.  dK/dV does the same for a
//     sequence with many queries on few keys, G * n_q > n_k^2 / 32 (see there).
//   * n_k = 0: the forward and dQ walk no tile and store zeros (out, lse, dq).  n_q = 0: dK/dV sweeps no slice and stores zeros.
// No atomics, a fixed summation order.  bidir_schedule_kernel writes both maps and zeroes the rows no sequence owns, in one launch.
#pragma once
#include "fa_common.h"

namespace fa {

constexpr int BIDIR_QBLOCK = 128;      // query rows per block of the forward and of dQ
constexpr int BIDIR_FILL_BLOCKS = 64;  // workgroups of the schedule launch that zero unowned rows
constexpr float BIDIR_DEFER_SUM = 64.0f;   // as fa_fwd.h's MAX_DEFER_SUM: bound on a lane's partial row sum while the reference stands

// A map entry: two int4, (first q row, q rows, first k row, k rows) of the block's sequence and (block within it, sequence, 0, 0);
// block -1: unused, the workgroup returns before its first barrier.
constexpr int BIDIR_ENTRY_BYTES = 32;

// bytes of a buffer resource over n rows of ld elements whose last row ends after D of them (n = 0: no byte, every load reads zero)
template <typename T, int D> FA_DEV uint32_t bidir_bytes(int n, int ld) {
  return n > 0 ? ((uint32_t)(n - 1) * (uint32_t)ld + D) * (uint32_t)sizeof(T) : 0u;
}

// TileStager::load with the tile's row offset in the voffset, under the resource's range check (fa_decode.h's load_rows)
template <typename S> FA_DEV void bidir_load(S& st, rsrc_t rs, int row0) {
#pragma unroll
  for (int i = 0; i < S::PER; ++i) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if (S::NCH % S::THREADS == 0 || st.live)
      v = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                        rs, (int)((uint32_t)st.voff + (uint32_t)(row0 + i * S::RSTEP) * (uint32_t)st.ldb), 0, 0));
    st.regs[i] = v;
  }
}
template <typename T, int D, int ROWS, int NT> struct BidirStager : TileStager<T, D, ROWS, NT> {
  static constexpr int THREADS = NT;
};

// sets bh, blk and the sequence's rows sq_, nq, sk_, nk from the map entry of this workgroup; scalar loads, and readfirstlane says so
#define FA_BIDIR_LOCATE(blk)                                                                         \
  int entry_;                                                                                        \
  map_block(blockIdx.x, BH, nblk, bh, entry_);                                                       \
  const int4 ea_ = map[2 * entry_], eb_ = map[2 * entry_ + 1];                                       \
  blk = __builtin_amdgcn_readfirstlane(eb_.x);                                                       \
  if (blk < 0) return;                                                                               \
  const int sq_ = __builtin_amdgcn_readfirstlane(ea_.x), nq = __builtin_amdgcn_readfirstlane(ea_.y); \
  const int sk_ = __builtin_amdgcn_readfirstlane(ea_.z), nk = __builtin_amdgcn_readfirstlane(ea_.w);

// ---------------------------------------------------------------------------------------------
// Forward, query-stationary: a workgroup = 4 waves = 128 query rows.  P = exp2(c*s - c*m_ref) against a per-row reference that only
// moves when a lane's partial row sum would pass 2^6 (fa_fwd.h).  Every row meets key 0 in tile 0, which takes the classic step (tile
// maximum, reference moved, O and l rescaled) since no row has a reference before it.
// ---------------------------------------------------------------------------------------------
template <typename T, int D, int BN>
__global__ void __launch_bounds__(256)
bidir_fwd_kernel(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, float* __restrict__ o,
                 float* __restrict__ lse, const int4* __restrict__ map, int Tq, int Tk, int nblk, int BH, Layout lay, float tau) {
  using A = Atom<T>;
  typedef typename A::frag frag;
  constexpr int KC = D / 16, KT = BN / 32, DT = D / 32;
  constexpr int TB = A::template tile_bytes<D>(BN);
  __shared__ __attribute__((aligned(16))) char smem_raw[4 * TB];
  lds_char* smem = (lds_char*)smem_raw;

  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int bh, qb;
  FA_BIDIR_LOCATE(qb)
  const int q0 = qb * 128 + w * 32, qrow = q0 + r;
  const bool qvalid = qrow < nq;
  const bool careful = A::SPLITS && nk < 64;   // wave-uniform: the sequence's rows admit fewer than 64 keys
  const int ld = lay.ld;
  const size_t base = head_base(lay, bh) + (size_t)sq_ * ld;
  const rsrc_t qrs = make_rsrc(q + base, bidir_bytes<T, D>(nq, ld));
  const int ldk = lay.ldk;
  const size_t kvb = kv_base<D>(lay, bh, Tk) + (size_t)sk_ * ldk;
  const uint32_t kv_bytes = bidir_bytes<T, D>(nk, ldk);
  const rsrc_t krs = make_rsrc(k + kvb, kv_bytes);
  const rsrc_t vrs = make_rsrc(v + kvb, kv_bytes);
  const float c = tau * LOG2E;

  frag qf[KC];
#pragma unroll
  for (int kc = 0; kc < KC; ++kc)
    qf[kc] = load_frag_buf<T>(qrs, (qrow * ld + 16 * kc + 8 * h) * (int)sizeof(T));

  f32x16 acc_o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc_o[dt] = zero16();
  float m_ref = -INFINITY, nmc = 0.f, l_run = 0.f;   // raw score units; nmc = -m_ref * c; m_ref = -inf: the row has no reference yet

  const LaneAddr ra = A::template row_addr<D>(lane);
  const LaneAddr ta = A::template tr_addr<D>(lane);
  const int nt = (nk + BN - 1) / BN;
  BidirStager<T, D, BN, 256> sk, sv;
  sk.init(tid, ldk);
  sv.init(tid, ldk);
  bidir_load(sk, krs, 0);
  bidir_load(sv, vrs, 0);
  sk.store(smem);
  sv.store(smem + 2 * TB);
  __syncthreads();

  auto tile = [&](auto par, int t) {
    constexpr int PAR = decltype(par)::value;
    const int kbase = t * BN;
    const bool more = t + 1 < nt;
    if (more) {
      bidir_load(sk, krs, kbase + BN);
      bidir_load(sv, vrs, kbase + BN);
    }
    lds_char* tk = smem + PAR * TB;
    lds_char* tv = smem + (2 + PAR) * TB;
    if (q0 < nq) {   // wave-uniform
      f32x16 s[KT];
      auto scores = [&]() {   // S^T tile of this wave (raw units), the key tail masked
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
          s[kt] = zero16();
#pragma unroll
          for (int kc = 0; kc < KC; ++kc) A::mma(s[kt], A::template row_frag<D>(tk, ra, 32 * kt, kc), qf[kc]);
          if (kbase + 32 * kt + 31 >= nk) {   // wave-uniform
#pragma unroll
            for (int i = 0; i < 16; ++i)
              if (kbase + 32 * kt + acc_row(i, h) >= nk) s[kt][i] = -INFINITY;
          }
        }
      };
      auto tile_max = [&]() {
        float mx = s[0][0];
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
          for (int i = 0; i < 16; ++i) mx = fmaxf(mx, s[kt][i]);
        return xhalf_max(mx);
      };
      auto exps = [&]() {   // s <- P = exp2(c*s - c*m_ref); returns this lane's partial row sum
        float rowsum = 0.f;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kt][i], c, nmc));
            s[kt][i] = p;
            rowsum += p;
          }
        return rowsum;
      };
      scores();
      float rowsum = 0.f;
      bool classic = t == 0;   // no row has a reference yet
      if (!classic) {
        rowsum = exps();
        if (__any(!(rowsum < BIDIR_DEFER_SUM))) {   // rare: some row outgrew its reference
          classic = true;
          scores();
        }
      }
      if (classic) {
        const float m_new = fmaxf(m_ref, tile_max());   // finite: key kbase is admitted (kbase < nk)
        const float alpha = (m_ref == -INFINITY) ? 1.0f : __builtin_amdgcn_exp2f((m_ref - m_new) * c);   // (no reference: O = l = 0)
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
          for (int i = 0; i < 16; ++i) acc_o[dt][i] *= alpha;
        l_run *= alpha;
        m_ref = m_new;
        nmc = -m_new * c;
        rowsum = exps();
      }
      l_run += rowsum;
      frag pf[KT][2];
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        pf[kt][0] = A::pack(s[kt], 0);
        pf[kt][1] = A::pack(s[kt], 1);
      }
      if (!careful) {
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
              A::mma(acc_o[dt], A::template tr_frag<D>(tv, ta, 32 * kt + 16 * s2, dt), pf[kt][s2]);
      } else {   // few keys: P.V also takes what the bf16 rounding of P dropped
        frag pl[KT][2];
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
          pl[kt][0] = A::pack_lo(s[kt], 0, pf[kt][0]);
          pl[kt][1] = A::pack_lo(s[kt], 1, pf[kt][1]);
        }
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
              const frag vt = A::template tr_frag<D>(tv, ta, 32 * kt + 16 * s2, dt);
              A::mma(acc_o[dt], vt, pf[kt][s2]);
              A::mma(acc_o[dt], vt, pl[kt][s2]);
            }
      }
    }
    if (more) {
      sk.store(smem + (PAR ^ 1) * TB);
      sv.store(smem + (2 + (PAR ^ 1)) * TB);
    }
    __syncthreads();
  };
  int t = 0;
  for (; t + 1 < nt; t += 2) {
    tile(ic<0>{}, t);
    tile(ic<1>{}, t + 1);
  }
  if (t < nt) tile(ic<0>{}, t);

  const float l_tot = xhalf_sum(l_run);   // > 0 for every real row of a sequence with a key
  if (qvalid) {
    const bool keyless = nk == 0;   // the rows come back as zeros, as rows no sequence owns
    const float inv = keyless ? 0.f : 1.0f / l_tot;
    float* orow = o + base + (size_t)qrow * ld;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 val = {acc_o[dt][4 * g] * inv, acc_o[dt][4 * g + 1] * inv, acc_o[dt][4 * g + 2] * inv, acc_o[dt][4 * g + 3] * inv};
        *reinterpret_cast<f32x4*>(orow + 32 * dt + 8 * g + 4 * h) = val;
      }
    if (h == 0) lse[(size_t)bh * Tq + sq_ + qrow] = keyless ? 0.f : m_ref * tau + __logf(l_tot);
  }
}

// ---------------------------------------------------------------------------------------------
// Backward dQ, query-stationary: NWQ waves x 32 query rows, K / V tiles of 32 keys, all of the sequence's.
// nlc = -L / tau and ndelta = -rowsum(dO * O) come from bwd_prep_kernel (fa_bwd_dkdv.h).
// ---------------------------------------------------------------------------------------------
template <typename T, int D, int NWQ>
__global__ void __launch_bounds__(64 * NWQ)
bidir_dq_kernel(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, const T* __restrict__ dout,
                const float* __restrict__ nlc, const float* __restrict__ ndelta, float* __restrict__ dq, const int4* __restrict__ map,
                int Tq, int Tk, int nblk, int BH, Layout lay, float tau) {
  using A = Atom<T>;
  typedef typename A::frag frag;
  constexpr int BN = 32, KC = D / 16, DT = D / 32, QB = 32 * NWQ;
  constexpr int TB = A::template tile_bytes<D>(BN);
  __shared__ __attribute__((aligned(16))) char smem_raw[4 * TB];
  lds_char* smem = (lds_char*)smem_raw;

  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int bh, qb;
  FA_BIDIR_LOCATE(qb)
  const int q0 = qb * QB + w * 32, qrow = q0 + r;
  const bool qvalid = qrow < nq;
  const bool careful = A::SPLITS && nk < 64;   // wave-uniform: see bidir_fwd_kernel
  const int ld = lay.ld;
  const size_t base = head_base(lay, bh) + (size_t)sq_ * ld;
  const uint32_t mat_bytes = bidir_bytes<T, D>(nq, ld);
  const rsrc_t qrs = make_rsrc(q + base, mat_bytes);
  const rsrc_t dors = make_rsrc(dout + base, mat_bytes);
  const int ldk = lay.ldk;
  const size_t kvb = kv_base<D>(lay, bh, Tk) + (size_t)sk_ * ldk;
  const uint32_t kv_bytes = bidir_bytes<T, D>(nk, ldk);
  const rsrc_t krs = make_rsrc(k + kvb, kv_bytes);
  const rsrc_t vrs = make_rsrc(v + kvb, kv_bytes);
  const float c = tau * LOG2E;

  frag qf[KC], dof[KC];
#pragma unroll
  for (int kc = 0; kc < KC; ++kc) {
    const int off = (qrow * ld + 16 * kc + 8 * h) * (int)sizeof(T);
    qf[kc] = load_frag_buf<T>(qrs, off);
    dof[kc] = load_frag_buf<T>(dors, off);
  }
  // this lane's row constants; -delta, in every register, is the accumulator input of the dP^T tiles
  const size_t rc0 = (size_t)bh * Tq + sq_;
  const float nlq = qvalid ? nlc[rc0 + qrow] * c : 0.f;   // -L * log2(e)
  const float ndq = qvalid ? ndelta[rc0 + qrow] : 0.f;
  f32x16 nd16;
#pragma unroll
  for (int i = 0; i < 16; ++i) nd16[i] = ndq;

  f32x16 acc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc[dt] = zero16();

  const LaneAddr ra = A::template row_addr<D>(lane);
  const LaneAddr ta = A::template tr_addr<D>(lane);
  const int nt = (nk + BN - 1) / BN;
  BidirStager<T, D, BN, 64 * NWQ> sk, sv;
  sk.init(tid, ldk);
  sv.init(tid, ldk);
  bidir_load(sk, krs, 0);
  bidir_load(sv, vrs, 0);
  sk.store(smem);
  sv.store(smem + 2 * TB);
  __syncthreads();

  auto tile = [&](auto par, int t) {
    constexpr int PAR = decltype(par)::value;
    const int kbase = t * BN;
    const bool more = t + 1 < nt;
    if (more) {
      bidir_load(sk, krs, kbase + BN);
      bidir_load(sv, vrs, kbase + BN);
    }
    lds_char* tk = smem + PAR * TB;
    lds_char* tv = smem + (2 + PAR) * TB;
    if (q0 < nq) {   // wave-uniform
      f32x16 s, dp;
      A::mma_c(s, A::template row_frag<D>(tk, ra, 0, 0), qf[0], zero16());
      A::mma_c(dp, A::template row_frag<D>(tv, ra, 0, 0), dof[0], nd16);
#pragma unroll
      for (int kc = 1; kc < KC; ++kc) {
        A::mma(s, A::template row_frag<D>(tk, ra, 0, kc), qf[kc]);
        A::mma(dp, A::template row_frag<D>(tv, ra, 0, kc), dof[kc]);
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) s[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[i], c, nlq));
      if (kbase + 31 >= nk) {   // wave-uniform: the key tail
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (kbase + acc_row(i, h) >= nk) s[i] = 0.f;
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) dp[i] = s[i] * dp[i];
      frag dsf[2];
      dsf[0] = A::pack(dp, 0);
      dsf[1] = A::pack(dp, 1);
      if (!careful) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) A::mma(acc[dt], A::template tr_frag<D>(tk, ta, 16 * s2, dt), dsf[s2]);
      } else {   // few keys: K^T dS^T also takes what the bf16 rounding of dS dropped
        frag dl[2];
        dl[0] = A::pack_lo(dp, 0, dsf[0]);
        dl[1] = A::pack_lo(dp, 1, dsf[1]);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) {
            const frag kt_ = A::template tr_frag<D>(tk, ta, 16 * s2, dt);
            A::mma(acc[dt], kt_, dsf[s2]);
            A::mma(acc[dt], kt_, dl[s2]);
          }
      }
    }
    if (more) {
      sk.store(smem + (PAR ^ 1) * TB);
      sv.store(smem + (2 + (PAR ^ 1)) * TB);
    }
    __syncthreads();
  };
  int t = 0;
  for (; t + 1 < nt; t += 2) {
    tile(ic<0>{}, t);
    tile(ic<1>{}, t + 1);
  }
  if (t < nt) tile(ic<0>{}, t);

  if (qvalid) {   // (a keyless sequence walked no tile: zeros)
    float* row = dq + base + (size_t)qrow * ld;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 val = {acc[dt][4 * g] * tau, acc[dt][4 * g + 1] * tau, acc[dt][4 * g + 2] * tau, acc[dt][4 * g + 3] * tau};
        *reinterpret_cast<f32x4*>(row + 32 * dt + 8 * g + 4 * h) = val;
      }
  }
}

// ---------------------------------------------------------------------------------------------
// Backward dK / dV, key-stationary: a workgroup = NW waves = NW * 32 keys of one (head, sequence); each wave keeps the K, V fragments
// and the dK^T, dV^T accumulators of its 32 keys while the workgroup sweeps all QS-query slices of the sequence (Q, dO and their row
// constants staged in LDS, double buffered).  Stores one dK and one dV per QUERY head, rows of ld = H * d floats (a grouped call
// points dk, dv at the workspace; group_sum_kernel adds the groups).
// ---------------------------------------------------------------------------------------------
template <typename T, int D, int NW, int QS>
__global__ void __launch_bounds__(NW * 64)
bidir_dkdv_kernel(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, const T* __restrict__ dout,
                  const float* __restrict__ nlc, const float* __restrict__ ndelta, float* __restrict__ dk, float* __restrict__ dv,
                  const int4* __restrict__ map, int Tq, int Tk, int nblk, int BH, Layout lay, float tau) {
  using A = Atom<T>;
  typedef typename A::frag frag;
  constexpr int KC = D / 16, DT = D / 32, BK = NW * 32, NT = NW * 64, NSUB = QS / 32;
  constexpr int TB = A::template tile_bytes<D>(QS);
  constexpr int BUF = 2 * TB + 8 * QS;   // Q tile, dO tile, QS x nlc, QS x -delta
  __shared__ __attribute__((aligned(16))) char smem_raw[2 * BUF];
  lds_char* smem = (lds_char*)smem_raw;

  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int bh, kb;
  FA_BIDIR_LOCATE(kb)
  const int kw0 = kb * BK + w * 32, key = kw0 + r;
  // wave-uniform: see bidir_fwd_kernel; and MANY queries on FEW keys (cross-attention against a short memory).  A key collects P and
  // dS of all G * n_q queries, terms of order 1 / n_k whose bf16 rounding (2^-9 / sqrt(3) relative rms) adds up with sqrt(G * n_q):
  // for U(-1, 1) operands an entry of dV is off by about 6.5e-4 * sqrt(G * n_q) / n_k rms.  Four of those stay under half the
  // project's 1e-3 envelope while G * n_q <= n_k^2 / 32; past that the split operands, as for the sink keys of fa_window.h.
  const bool thin = A::SPLITS && (nk < 64 || 32L * lay.G * nq > (long)nk * nk);
  const int ld = lay.ld;
  const size_t hb = head_base(lay, bh);
  const size_t base = hb + (size_t)sq_ * ld;        // Q, dO
  const size_t gbase = hb + (size_t)sk_ * ld;       // the per-query-head dK, dV
  const uint32_t mat_bytes = bidir_bytes<T, D>(nq, ld);
  const rsrc_t qrs = make_rsrc(q + base, mat_bytes);
  const rsrc_t dors = make_rsrc(dout + base, mat_bytes);
  const int ldk = lay.ldk;
  const size_t kvb = kv_base<D>(lay, bh, Tk) + (size_t)sk_ * ldk;
  const uint32_t kv_bytes = bidir_bytes<T, D>(nk, ldk);
  const rsrc_t krs = make_rsrc(k + kvb, kv_bytes);
  const rsrc_t vrs = make_rsrc(v + kvb, kv_bytes);
  const float* nlg = nlc + (size_t)bh * Tq + sq_;
  const float* deg = ndelta + (size_t)bh * Tq + sq_;
  const float c = tau * LOG2E;

  frag kf[KC], vf[KC];
#pragma unroll
  for (int kc = 0; kc < KC; ++kc) {
    const int off = (key * ldk + 16 * kc + 8 * h) * (int)sizeof(T);   // rows >= nk read as zero
    kf[kc] = load_frag_buf<T>(krs, off);
    vf[kc] = load_frag_buf<T>(vrs, off);
  }
  f32x16 acc_dk[DT], acc_dv[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    acc_dk[dt] = zero16();
    acc_dv[dt] = zero16();
  }

  const LaneAddr ra = A::template row_addr<D>(lane);
  const LaneAddr ta = A::template tr_addr<D>(lane);
  const int nqi = (nq + QS - 1) / QS;   // the sweep: slices 0 .. nqi - 1 (none for a sequence without queries)
  // Stage copies of Q and dO, as bwd_dkdv_kernel: LDS-DMA for bf16 at d >= 64, registers otherwise
  constexpr bool DMA = sizeof(T) == 2 && D >= 64;
  constexpr int PPG = D >= 128 ? 2 : 1;
  BidirStager<T, D, QS, NT> sq, sdo;
  if constexpr (!DMA) {
    sq.init(tid, ld);
    sdo.init(tid, ld);
  }
  const raw_rsrc_t qraw = make_raw_rsrc(q + base, mat_bytes), doraw = make_raw_rsrc(dout + base, mat_bytes);
  const uint32_t smem_addr = (uint32_t)(uintptr_t)smem;
  FA_DMA_VOFF(dma_voff, PPG, lane, w, ld, (int)sizeof(T));
  float st_nl = 0.f, st_de = 0.f;
  auto stage_load = [&](int qi, int dst /* LDS byte offset of the stage buffer */) {
    if constexpr (DMA) {
      using RG = StageRing<D, QS, NW>;
      static_assert(RG::PPG == PPG && RG::dma_matches_image(), "LDS-DMA source swizzle vs Atom::off");
#pragma unroll
      for (int i = 0; i < RG::NPW; ++i) {
        const int piece = w + NW * i, g = piece / PPG;
        // (the slice's row offset in the vector offset, under the range check: rows >= nq land as zeros)
        const int voff = (int)((uint32_t)dma_voff + (uint32_t)(qi * QS + 8 * g) * (uint32_t)ld * (uint32_t)sizeof(T));
        dma16(qraw, smem_addr + dst + 1024 * piece, voff, 0);
        dma16(doraw, smem_addr + dst + TB + 1024 * piece, voff, 0);
      }
    } else {
      bidir_load(sq, qrs, qi * QS);
      bidir_load(sdo, dors, qi * QS);
    }
    if (tid < QS) {
      const int row = qi * QS + tid;
      st_nl = row < nq ? nlg[row] : 0.f;
      st_de = row < nq ? deg[row] : 0.f;
    }
  };
  auto stage_store = [&](lds_char* b) {
    if constexpr (DMA) {
      dma_wait_all();   // this wave's pieces have landed (the barrier that follows publishes them)
    } else {
      sq.store(b);
      sdo.store(b + TB);
    }
    if (tid < QS) {
      *FA_LDS(float, b + 2 * TB + 4 * tid) = st_nl;
      *FA_LDS(float, b + 2 * TB + 4 * QS + 4 * tid) = st_de;
    }
  };
  if (nqi > 0) {   // wave-uniform, the whole workgroup
    stage_load(0, 0);
    stage_store(smem);
    __syncthreads();
  }

  auto slice = [&](auto par, int qi) {
    constexpr int PAR = decltype(par)::value;
    const bool more = qi + 1 < nqi;
    if (more) stage_load(qi + 1, (PAR ^ 1) * BUF);
    lds_char* buf = smem + PAR * BUF;
    lds_char* tq = buf;
    lds_char* tdo = buf + TB;
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub) {
      const int qi0 = qi * QS + 32 * sub;
      if (kw0 < nk && qi0 < nq) {   // wave-uniform
        // register i of lane half h is query qi0 + acc_row(i, h): its nlc / -delta come from LDS (broadcast reads) and ride in as
        // the accumulator inputs: S' = S - L/tau, dP' = dP - delta
        f32x16 nl16, nd16;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 a = *FA_LDS(f32x4, buf + 2 * TB + 128 * sub + 16 * h + 32 * g);
          const f32x4 b = *FA_LDS(f32x4, buf + 2 * TB + 4 * QS + 128 * sub + 16 * h + 32 * g);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            nl16[4 * g + j] = a[j];
            nd16[4 * g + j] = b[j];
          }
        }
        f32x16 s, dp;
        A::mma_c(s, A::template row_frag<D>(tq, ra, 32 * sub, 0), kf[0], nl16);
        A::mma_c(dp, A::template row_frag<D>(tdo, ra, 32 * sub, 0), vf[0], nd16);
#pragma unroll
        for (int kc = 1; kc < KC; ++kc) {
          A::mma(s, A::template row_frag<D>(tq, ra, 32 * sub, kc), kf[kc]);
          A::mma(dp, A::template row_frag<D>(tdo, ra, 32 * sub, kc), vf[kc]);
        }
        // (query rows >= nq: Q, dO and the constants are zeros, P = 1 meets dO = 0 and dS = 0: nothing is added.  Keys >= nk are
        // lanes that are not stored.)
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = __builtin_amdgcn_exp2f(s[i] * c);
#pragma unroll
        for (int i = 0; i < 16; ++i) dp[i] = s[i] * dp[i];
        frag pf[2], dsf[2];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          pf[s2] = A::pack(s, s2);
          dsf[s2] = A::pack(dp, s2);
        }
        if (!thin) {
#pragma unroll
          for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
              A::mma(acc_dv[dt], A::template tr_frag<D>(tdo, ta, 32 * sub + 16 * s2, dt), pf[s2]);
              A::mma(acc_dk[dt], A::template tr_frag<D>(tq, ta, 32 * sub + 16 * s2, dt), dsf[s2]);
            }
        } else {   // few keys: both products also take what the bf16 rounding of P, dS dropped
          frag pl[2], dl[2];
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) {
            pl[s2] = A::pack_lo(s, s2, pf[s2]);
            dl[s2] = A::pack_lo(dp, s2, dsf[s2]);
          }
#pragma unroll
          for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
              const frag adoT = A::template tr_frag<D>(tdo, ta, 32 * sub + 16 * s2, dt);
              const frag aqT = A::template tr_frag<D>(tq, ta, 32 * sub + 16 * s2, dt);
              A::mma(acc_dv[dt], adoT, pf[s2]);
              A::mma(acc_dv[dt], adoT, pl[s2]);
              A::mma(acc_dk[dt], aqT, dsf[s2]);
              A::mma(acc_dk[dt], aqT, dl[s2]);
            }
        }
      }
    }
    if (more) stage_store(smem + (PAR ^ 1) * BUF);
    __syncthreads();
  };
  int qi = 0;
  for (; qi + 1 < nqi; qi += 2) {
    slice(ic<0>{}, qi);
    slice(ic<1>{}, qi + 1);
  }
  if (qi < nqi) slice(ic<0>{}, qi);

  if (key < nk) {   // (a sequence without queries swept no slice: zeros)
    float* dkrow = dk + gbase + (size_t)key * ld;
    float* dvrow = dv + gbase + (size_t)key * ld;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 a = {acc_dk[dt][4 * g] * tau, acc_dk[dt][4 * g + 1] * tau, acc_dk[dt][4 * g + 2] * tau, acc_dk[dt][4 * g + 3] * tau};
        f32x4 b = {acc_dv[dt][4 * g], acc_dv[dt][4 * g + 1], acc_dv[dt][4 * g + 2], acc_dv[dt][4 * g + 3]};
        *reinterpret_cast<f32x4*>(dkrow + 32 * dt + 8 * g + 4 * h) = a;
        *reinterpret_cast<f32x4*>(dvrow + 32 * dt + 8 * g + 4 * h) = b;
      }
  }
}

// ---- the schedule launch ----------------------------------------------------------------------------------------------------------
// One map over the array `cu` (T rows, block size bs): for b = 0, 1, ... in order, one entry for each of the ceil(n_b / bs) blocks of
// sequence b (none for n_b = 0), then unused entries up to `cap` = T / bs + nseq.  A sequence of n rows has at most floor(n / bs) + 1
// blocks and, for a non-decreasing cu, the floors sum to at most floor(T / bs): the map holds them all.  For any other cu the counts
// saturate at cap and the entries past it are dropped, so the map is never overrun.  An entry carries the sequence's rows in the q
// buffer and in the k buffer, whichever array the blocks count.  Integer work in a fixed order: a function of the two arrays alone.
FA_DEV void bidir_build_map(const int* cu, int T, const int* cu_q, int Tq, const int* cu_k, int Tk, int nseq, int4* map, int bs,
                            int cap, int* counts) {
  const int tid = threadIdx.x;
  const int per = (int)(((long)nseq + 255) / 256);
  const int b0 = (int)min((long)tid * per, (long)nseq), b1 = (int)min((long)b0 + per, (long)nseq);
  int n = 0;
  for (int b = b0; b < b1; ++b) {
    int s, nb;
    seq_rows(cu, T, b, s, nb);
    n = min(n + (nb + bs - 1) / bs, cap);
  }
  counts[tid] = n;
  __syncthreads();
  int off = 0, total = 0;
  for (int u = 0; u < 256; ++u) {
    if (u == tid) off = total;
    total = min(total + counts[u], cap);
  }
  for (int b = b0; b < b1; ++b) {
    int s, nb, sq, nq, sk, nk;
    seq_rows(cu, T, b, s, nb);
    seq_rows(cu_q, Tq, b, sq, nq);
    seq_rows(cu_k, Tk, b, sk, nk);
    const int blocks = (nb + bs - 1) / bs;
    for (int blk = 0; blk < blocks && off < cap; ++blk, ++off) {
      map[2 * off] = make_int4(sq, nq, sk, nk);
      map[2 * off + 1] = make_int4(blk, b, 0, 0);
    }
  }
  for (int i = total + tid; i < cap; i += 256) {
    map[2 * i] = make_int4(0, 0, 0, 0);
    map[2 * i + 1] = make_int4(-1, 0, 0, 0);
  }
  __syncthreads();   // (counts is used again)
}

// What the launch zeroes in the rows no sequence owns: in the q buffers up to one [Tq][ld] fp32 matrix (out or dq) and one [H][Tq]
// array (lse), in the k buffers up to two [Tk][ld] matrices (dk, dv, per query head or not); ld a multiple of 4.
struct BidirFill {
  float* qmat;
  float* rowc;
  float* kmat[2];
  int ldq, ldk, H;
};

// Rows of a T-row buffer that no sequence owns: those in front of sequence 0 and those behind the last one (consecutive sequences
// leave no gap: each begins at or before the end of the one before it).  u counts them: 0 .. lead - 1, then the tail.
FA_DEV void bidir_fill_unowned(const int* cu, int nseq, int T, float* m0, float* m1, int ld, float* rowc, int H, long start, long step) {
  int lead, n0, sl, nl;
  seq_rows(cu, T, 0, lead, n0);
  seq_rows(cu, T, nseq - 1, sl, nl);
  const int tail0 = sl + nl;
  const long count = (long)lead + (T - tail0);
  if (count <= 0) return;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const int vpr = ld >> 2;
  for (long i = start; i < count * vpr; i += step) {
    const long u = i / vpr;
    const int col = (int)(i - u * vpr), row = u < lead ? (int)u : tail0 + (int)(u - lead);
    if (m0) *reinterpret_cast<f32x4*>(m0 + (size_t)row * ld + 4 * col) = zero;
    if (m1) *reinterpret_cast<f32x4*>(m1 + (size_t)row * ld + 4 * col) = zero;
  }
  if (rowc)
    for (long i = start; i < count * H; i += step) {
      const long hd = i / count, u = i - hd * count;
      const int row = u < lead ? (int)u : tail0 + (int)(u - lead);
      rowc[(size_t)hd * T + row] = 0.f;
    }
}

// map_k = nullptr: the forward (no key-block map)
__global__ void __launch_bounds__(256) bidir_schedule_kernel(const int* cu_q, const int* cu_k, int nseq, int Tq, int Tk, int4* map_q,
                                                             int cap_q, int4* map_k, int bk, int cap_k, BidirFill f) {
  if (blockIdx.x == 0) {
    __shared__ int counts[256];
    bidir_build_map(cu_q, Tq, cu_q, Tq, cu_k, Tk, nseq, map_q, BIDIR_QBLOCK, cap_q, counts);
    if (map_k) bidir_build_map(cu_k, Tk, cu_q, Tq, cu_k, Tk, nseq, map_k, bk, cap_k, counts);
    return;
  }
  const long start = (long)(blockIdx.x - 1) * 256 + threadIdx.x, step = (long)(gridDim.x - 1) * 256;
  if (f.qmat || f.rowc) bidir_fill_unowned(cu_q, nseq, Tq, f.qmat, nullptr, f.ldq, f.rowc, f.H, start, step);
  if (f.kmat[0]) bidir_fill_unowned(cu_k, nseq, Tk, f.kmat[0], f.kmat[1], f.ldk, nullptr, 0, start, step);
}

}  // namespace fa
