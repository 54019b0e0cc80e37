// Packed attention under a two-sided sliding window (a band), one cu_seqlens for the queries and one for the keys, forward and
// backward, on MI355X (gfx950): the kernels of libflash_attn_mi355x_local.so (include/flash_attn_mi355x_local.h), written against
// fa_atoms.h.  q / out / dO / dq are [Tq][H][d], k / v / dk / dv [Tk][Hkv][d]; sequence b owns n_q rows of the first buffers and n_k
// rows of the second, and its queries are the LAST n_q positions of its n_k keys: with D = n_k - n_q (DELTA below), query row i sits
// at key position p = i + D and admits key j iff 0 <= j < n_k and p - WL <= j <= p + WR.  The host hands an unbounded side over as a
// bound no sequence reaches (LOCAL_UNBOUNDED), so both edges are plain integer compares here.
//
// The geometry is fa_bidir.h's (its map, loads and schedule kernel are used as they are): a workgroup takes (head, map entry), the
// entry names its sequence's rows in both buffers, the resources end with the sequence's rows, every tile's row offset rides in the
// vector offset under the resource's range check, a block never straddles sequences.  The diagonal is fa_prefix.h's, with two edges:
//   * Forward and dQ: a query block with rows i_first .. i_last walks the key tiles that meet [max(0, i_first + D - WL),
//     min(n_k, i_last + D + WR + 1)); with an empty range it stores zeros and touches no LDS.  A wave skips the compute of a tile
//     wholly outside the band of its own rows (it still stages and meets the barriers), and masks per element only the 32 x 32
//     sub-tiles that straddle the lower edge, the upper edge or the key tail j >= n_k (which the right side can reach).  The lanes of
//     a wave past n_q take the wave's last real row's position, so that they never hold a wave back.
//   * A row has no softmax reference until the first tile in which it admits a key, and a tile in which some row of the wave lacks one
//     takes the classic step; a row that never admits one (p + WR < 0, or n_k = 0) keeps l = 0 and stores zeros in out and lse.  In
//     the backward such a row has lse = 0, and P outside the band is forced to 0 (it would be exp2(s * c)).
//   * dK/dV: a key block with keys j_first .. j_last sweeps the query slices that meet [max(0, j_first - WR - D),
//     min(n_q, j_last + WL - D + 1)); a wave skips the sub-slices wholly outside its keys' band and forces P and dS to 0 per element
//     where a sub-slice straddles an edge.  A block none of whose keys is admitted sweeps nothing and stores zeros.
//   * bf16: rows that admit fewer than 64 keys take P and dS into the second product as two bf16 fragments (Atom::pack_lo).  A row
//     at position p admits local_count(p) keys, a concave function of p, so the least count of a run of rows is at one of its ends:
//     the decision is wave-uniform and covers a band of WL + WR + 1 < 64, n_k < 64, and the rows next to a sequence end on a bounded
//     side.  dK/dV decides per sub-slice, and keeps fa_bidir.h's rule for many queries on few keys, counted within the band.
// No atomics, a fixed summation order.  Grids and workspace are functions of the shapes alone, never of WL, WR or the arrays.
#pragma once
#include "fa_bidir.h"

namespace fa {

constexpr int LOCAL_UNBOUNDED = 1 << 29;   // a window side no sequence reaches (T < 2^22: sums of a position and this stay in an int)

// keys admitted by a row at position p of a sequence with nk keys: concave in p (0 or less: none)
FA_DEV int local_count(int p, int nk, int WL, int WR) { return min(nk - 1, p + WR) - max(0, p - WL) + 1; }

// ---------------------------------------------------------------------------------------------
// Forward, query-stationary: a workgroup = 4 waves = 128 query rows.  P = exp2(c*s - c*m_ref) against a per-row reference that only
// moves when a lane's partial row sum would pass 2^6 (fa_fwd.h).
// ---------------------------------------------------------------------------------------------
template <typename T, int D, int BN>
__global__ void __launch_bounds__(256)
local_fwd_kernel(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, float* __restrict__ o,
                 float* __restrict__ lse, const int4* __restrict__ map, int Tq, int Tk, int nblk, int BH, Layout lay, float tau, int WL,
                 int WR) {
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
  const int DELTA = nk - nq;   // wave-uniform
  const int q0 = qb * 128 + w * 32, qrow = q0 + r;
  const bool qvalid = qrow < nq;
  const int p0 = q0 + DELTA, p1 = min(q0 + 31, nq - 1) + DELTA;   // wave-uniform: the positions of the wave's first and last real row
  const int pos = min(qrow, nq - 1) + DELTA;                      // this lane's (a lane past n_q: the last real row's)
  const bool careful = A::SPLITS && (local_count(p0, nk, WL, WR) < 64 || local_count(p1, nk, WL, WR) < 64);   // wave-uniform
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
  // the walk: the key tiles that meet the band of the block's rows (none: the block's rows admit no key)
  const int klo = max(0, qb * 128 + DELTA - WL), khi = min(nk, min(nq, qb * 128 + 128) + DELTA + WR);
  const int t0 = klo / BN, nt = khi > klo ? (khi + BN - 1) / BN : t0;
  BidirStager<T, D, BN, 256> sk, sv;
  sk.init(tid, ldk);
  sv.init(tid, ldk);
  if (t0 < nt) {   // wave-uniform, the whole workgroup
    bidir_load(sk, krs, t0 * BN);
    bidir_load(sv, vrs, t0 * BN);
    sk.store(smem);
    sv.store(smem + 2 * TB);
    __syncthreads();
  }

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
    if (q0 < nq && kbase <= p1 + WR && kbase + BN - 1 >= p0 - WL) {   // wave-uniform: some row of the wave admits a key of this tile
      f32x16 s[KT];
      auto scores = [&]() {   // S^T tile of this wave (raw units), masked outside the band and past the key tail
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
          s[kt] = zero16();
#pragma unroll
          for (int kc = 0; kc < KC; ++kc) A::mma(s[kt], A::template row_frag<D>(tk, ra, 32 * kt, kc), qf[kc]);
          const int k32 = kbase + 32 * kt;
          if (k32 + 31 > p0 + WR || k32 < p1 - WL || k32 + 31 >= nk) {   // wave-uniform: not wholly inside every row's band
#pragma unroll
            for (int i = 0; i < 16; ++i) {
              const int j = k32 + acc_row(i, h);
              if (j > pos + WR || j < pos - WL || j >= nk) s[kt][i] = -INFINITY;
            }
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
      bool classic = __any(m_ref == -INFINITY);   // some row has no reference yet
      if (!classic) {
        rowsum = exps();
        if (__any(!(rowsum < BIDIR_DEFER_SUM))) {   // rare: some row outgrew its reference
          classic = true;
          scores();
        }
      }
      if (classic) {
        const float m_new = fmaxf(m_ref, tile_max());
        const float alpha = (m_ref == -INFINITY) ? 1.0f : __builtin_amdgcn_exp2f((m_ref - m_new) * c);   // (no reference: O = l = 0)
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
          for (int i = 0; i < 16; ++i) acc_o[dt][i] *= alpha;
        l_run *= alpha;
        m_ref = m_new;
        nmc = (m_new == -INFINITY) ? 0.f : -m_new * c;   // (still no key: every score is -inf, P = 0 against any reference)
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
      } else {   // rows with few admissible keys: P.V also takes what the bf16 rounding of P dropped
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
  int t = t0;
  for (; t + 1 < nt; t += 2) {
    tile(ic<0>{}, t);
    tile(ic<1>{}, t + 1);
  }
  if (t < nt) tile(ic<0>{}, t);

  const float l_tot = xhalf_sum(l_run);   // 0 for a row that admits no key: it comes back as zeros, as rows no sequence owns
  if (qvalid) {
    const bool empty = !(l_tot > 0.f);
    const float inv = empty ? 0.f : 1.0f / l_tot;
    float* orow = o + base + (size_t)qrow * ld;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 val = {acc_o[dt][4 * g] * inv, acc_o[dt][4 * g + 1] * inv, acc_o[dt][4 * g + 2] * inv, acc_o[dt][4 * g + 3] * inv};
        *reinterpret_cast<f32x4*>(orow + 32 * dt + 8 * g + 4 * h) = val;
      }
    if (h == 0) lse[(size_t)bh * Tq + sq_ + qrow] = empty ? 0.f : m_ref * tau + __logf(l_tot);
  }
}

// ---------------------------------------------------------------------------------------------
// Backward dQ, query-stationary: NWQ waves x 32 query rows, K / V tiles of 32 keys, the forward's walk over them.
// nlc = -L / tau and ndelta = -rowsum(dO * O) come from bwd_prep_kernel (fa_bwd_dkdv.h).
// ---------------------------------------------------------------------------------------------
template <typename T, int D, int NWQ>
__global__ void __launch_bounds__(64 * NWQ)
local_dq_kernel(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, const T* __restrict__ dout,
                const float* __restrict__ nlc, const float* __restrict__ ndelta, float* __restrict__ dq, const int4* __restrict__ map,
                int Tq, int Tk, int nblk, int BH, Layout lay, float tau, int WL, int WR) {
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
  const int DELTA = nk - nq;   // wave-uniform
  const int q0 = qb * QB + w * 32, qrow = q0 + r;
  const bool qvalid = qrow < nq;
  const int p0 = q0 + DELTA, p1 = min(q0 + 31, nq - 1) + DELTA;   // wave-uniform: see local_fwd_kernel
  const int pos = min(qrow, nq - 1) + DELTA;
  const bool careful = A::SPLITS && (local_count(p0, nk, WL, WR) < 64 || local_count(p1, nk, WL, WR) < 64);   // wave-uniform
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
  const int klo = max(0, qb * QB + DELTA - WL), khi = min(nk, min(nq, qb * QB + QB) + DELTA + WR);   // the forward's walk
  const int t0 = klo / BN, nt = khi > klo ? (khi + BN - 1) / BN : t0;
  BidirStager<T, D, BN, 64 * NWQ> sk, sv;
  sk.init(tid, ldk);
  sv.init(tid, ldk);
  if (t0 < nt) {   // wave-uniform, the whole workgroup
    bidir_load(sk, krs, t0 * BN);
    bidir_load(sv, vrs, t0 * BN);
    sk.store(smem);
    sv.store(smem + 2 * TB);
    __syncthreads();
  }

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
    if (q0 < nq && kbase <= p1 + WR && kbase + BN - 1 >= p0 - WL) {   // wave-uniform
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
      if (kbase + 31 > p0 + WR || kbase < p1 - WL || kbase + 31 >= nk) {   // wave-uniform: an edge of the band, or the key tail
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int j = kbase + acc_row(i, h);
          if (j > pos + WR || j < pos - WL || j >= nk) s[i] = 0.f;
        }
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
      } else {   // rows with few admissible keys: K^T dS^T also takes what the bf16 rounding of dS dropped
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
  int t = t0;
  for (; t + 1 < nt; t += 2) {
    tile(ic<0>{}, t);
    tile(ic<1>{}, t + 1);
  }
  if (t < nt) tile(ic<0>{}, t);

  if (qvalid) {   // (a row that admits no key added nothing: zeros)
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
// and the dK^T, dV^T accumulators of its 32 keys while the workgroup sweeps the QS-query slices that admit a key of the block (Q, dO
// and their row constants staged in LDS, double buffered).  Key j is admitted by the queries j - WR - D <= i <= j + WL - D.  Stores
// one dK and one dV per QUERY head, rows of ld = H * d floats (a grouped call points dk, dv at the workspace; group_sum_kernel adds
// the groups).
// ---------------------------------------------------------------------------------------------
template <typename T, int D, int NW, int QS>
__global__ void __launch_bounds__(NW * 64)
local_dkdv_kernel(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, const T* __restrict__ dout,
                  const float* __restrict__ nlc, const float* __restrict__ ndelta, float* __restrict__ dk, float* __restrict__ dv,
                  const int4* __restrict__ map, int Tq, int Tk, int nblk, int BH, Layout lay, float tau, int WL, int WR) {
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
  const int DELTA = nk - nq;   // wave-uniform
  const int kb0 = kb * BK, kw0 = kb0 + w * 32, key = kw0 + r;
  const int kw1 = min(kw0 + 31, nk - 1);   // wave-uniform: the wave's last real key
  // wave-uniform: fa_bidir.h's rule for few keys, and for many queries on few keys, with the counts the band leaves: a key collects
  // P and dS of at most G * min(n_q, WL + WR + 1) queries, each a term of order 1 / min(n_k, WL + WR + 1).  (At the bound itself it
  // splits: a band of exactly 64 keys under G = 2 measured 9.9e-4 on dV unsplit at d = 128, where P is far from uniform.)  The rows
  // that admit fewer than 64 keys are found per sub-slice below
  const long band = (long)WL + WR + 1, per_key = min((long)nq, band), per_row = min((long)nk, band);
  const bool thin = A::SPLITS && (nk < 64 || 32L * lay.G * per_key >= per_row * per_row);
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
  // the sweep: the slices that meet the queries that admit a key of the block (none: no query does)
  const int qlo = max(0, kb0 - WR - DELTA), qhi = min(nq, min(nk, kb0 + BK) + WL - DELTA);
  const int qi_begin = qlo / QS, nqi = qhi > qlo ? (qhi + QS - 1) / QS : qi_begin;
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
  if (qi_begin < nqi) {   // wave-uniform, the whole workgroup
    stage_load(qi_begin, 0);
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
      const int pa = qi0 + DELTA, pb = min(qi0 + 31, nq - 1) + DELTA;   // the positions of the sub-slice's first and last real query
      if (kw0 < nk && qi0 < nq && kw0 <= pb + WR && kw1 >= pa - WL) {   // wave-uniform: some query of the sub-slice admits a key of the wave
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
        if (kw0 + 31 > pa + WR || kw0 < qi0 + 31 + DELTA - WL) {   // wave-uniform: the unmasked path only where every pair is admitted
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int pq = qi0 + acc_row(i, h) + DELTA;
            if (key > pq + WR || key < pq - WL) s[i] = 0.f;
          }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) dp[i] = s[i] * dp[i];
        frag pf[2], dsf[2];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          pf[s2] = A::pack(s, s2);
          dsf[s2] = A::pack(dp, s2);
        }
        // (the sub-slice's rows admit at least 64 keys)
        if (!(thin || (A::SPLITS && (local_count(pa, nk, WL, WR) < 64 || local_count(pb, nk, WL, WR) < 64)))) {
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
  int qi = qi_begin;
  for (; qi + 1 < nqi; qi += 2) {
    slice(ic<0>{}, qi);
    slice(ic<1>{}, qi + 1);
  }
  if (qi < nqi) slice(ic<0>{}, qi);

  if (key < nk) {   // (a block no query admits swept no slice: zeros)
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

}  // namespace fa
