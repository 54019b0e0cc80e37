// MLA prefill: causal packed attention at the head shape of a DeepSeek multi-head-latent-attention layer BEFORE absorption, 192 score
// columns and 128 value columns, on MI355X (gfx950): the kernel of libflash_attn_mi355x_mla_prefill.so
// (include/flash_attn_mi355x_mla_prefill.h), written against fa_atoms.h.  bf16, forward only.
//
// The operands are the tensors the layer has, not a 192-wide K with k_pe copied H times:
//   q       [Tq][H][192]   q_nope (128) then the rotated q_pe (64)
//   k_nope  rows of H heads x 128 columns: row stride k_ld, head stride k_hs (elements, multiples of 8)
//   k_pe    [Tk][64]       the rotated rope key, ONE vector per token read by every head
//   v       the geometry of k_nope under its own pointer and strides (v_ld, v_hs): the two are usually the two views of one
//           [Tk][H][256] up-projection output
//   out     fp32 [Tq][H][128], lse fp32 [H][Tq]
// Semantics, map, loads and schedule kernel are fa_prefix.h's and fa_bidir.h's, used as they are: a workgroup takes (head, map
// entry), the entry names its sequence's rows in both buffers, with D = n_k - n_q row i admits key j iff 0 <= j <= i + D, every
// resource ends with the sequence's rows and every tile's row offset rides in the vector offset under its range check.
//
//   * Workgroup: 256 threads = 4 waves x 32 query rows (BIDIR_QBLOCK = 128).  Q is 12 bf16x8 fragments per lane, loaded once.
//   * Keys come in 64-row tiles as THREE LDS images, double buffered (80 KB): k_nope in Atom::off<128> (16 KB), k_pe in
//     Atom::off<64> (8 KB) and v in Atom::off<128> (16 KB, read transposed).  One 192-wide image is not an option: 256 threads do
//     not tile rows of 24 chunks (TileStager), and k_pe has another pointer and no head stride anyway.
//   * Per wave and tile: S^T = 2 x (8 + 4) 32x32x16 MFMAs, the score accumulating over the nope image and then over the pe image
//     into one tile; P.V = 4 output tiles x 4 k-steps = 16 MFMAs into 64 accumulator registers.
//   * The softmax is prefix_fwd_kernel's: P = exp2(c*s - c*m_ref) against a per-row reference that moves only when a lane's partial
//     row sum would pass BIDIR_DEFER_SUM; a row has no reference until the first tile in which it admits a key; a wave skips the
//     compute of a tile wholly above its last row's diagonal and masks per element only the 32 x 32 sub-tiles that are not wholly
//     below its first row's.  Rows that admit fewer than 64 keys take P into the second product as pack + pack_lo.
//   * Grid order: FA_BIDIR_LOCATE's (map_block): the blocks of one head are neighbours and, for H a multiple of 8, on one XCD, so
//     that a head's k_nope and v (512 bytes per key) are served from that XCD's L2 to every block of the head.  k_pe (128 bytes per
//     key, the same for all heads) then lives in every XCD's L2 once.  Putting the heads of one block side by side instead would
//     share k_pe and the map entry and stream H heads of k_nope and v through the L2 at a time.  A supposition either way: neither
//     order has been profiled.
// No atomics, a fixed summation order.
#pragma once
#include "fa_bidir.h"

namespace fa {

constexpr int MLAP_DN = 128, MLAP_DR = 64, MLAP_DQ = MLAP_DN + MLAP_DR, MLAP_DV = 128, MLAP_BN = 64;

__global__ void __launch_bounds__(256)
mla_prefill_fwd_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k_nope, const bf16_t* __restrict__ k_pe,
                       const bf16_t* __restrict__ v, float* __restrict__ o, float* __restrict__ lse, const int4* __restrict__ map, int Tq,
                       int nblk, int BH, int k_ld, int k_hs, int v_ld, int v_hs, float tau) {
  using T = bf16_t;
  using A = Atom<T>;
  typedef A::frag frag;
  constexpr int DN = MLAP_DN, DR = MLAP_DR, DQ = MLAP_DQ, DV = MLAP_DV, BN = MLAP_BN;
  constexpr int KCN = DN / 16, KCR = DR / 16, KT = BN / 32, DT = DV / 32;
  constexpr int TBN = A::tile_bytes<DN>(BN), TBR = A::tile_bytes<DR>(BN), TBV = A::tile_bytes<DV>(BN);
  constexpr int OFF_R = 2 * TBN, OFF_V = OFF_R + 2 * TBR;
  __shared__ __attribute__((aligned(16))) char smem_raw[OFF_V + 2 * TBV];
  lds_char* smem = (lds_char*)smem_raw;

  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int bh, qb;   // bh: the head (a packed batch is one batch element)
  FA_BIDIR_LOCATE(qb)
  const int DELTA = nk - nq;   // wave-uniform
  const int q0 = qb * 128 + w * 32, qrow = q0 + r;
  const bool qvalid = qrow < nq;
  const bool careful = q0 + DELTA < 63 || nk < 64;   // wave-uniform: the wave's rows may admit fewer than 64 keys
  const int ldq = BH * DQ, ldo = BH * DV;
  const rsrc_t qrs = make_rsrc(q + (size_t)sq_ * ldq + (size_t)bh * DQ, bidir_bytes<T, DQ>(nq, ldq));
  const rsrc_t knrs = make_rsrc(k_nope + (size_t)sk_ * k_ld + (size_t)bh * k_hs, bidir_bytes<T, DN>(nk, k_ld));
  const rsrc_t krrs = make_rsrc(k_pe + (size_t)sk_ * DR, bidir_bytes<T, DR>(nk, DR));
  const rsrc_t vrs = make_rsrc(v + (size_t)sk_ * v_ld + (size_t)bh * v_hs, bidir_bytes<T, DV>(nk, v_ld));
  const float c = tau * LOG2E;

  frag qf[KCN + KCR];
#pragma unroll
  for (int kc = 0; kc < KCN + KCR; ++kc)
    qf[kc] = load_frag_buf<T>(qrs, (qrow * ldq + 16 * kc + 8 * h) * (int)sizeof(T));

  f32x16 acc_o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc_o[dt] = zero16();
  float m_ref = -INFINITY, nmc = 0.f, l_run = 0.f;   // raw score units; nmc = -m_ref * c; m_ref = -inf: the row has no reference yet

  const LaneAddr ran = A::row_addr<DN>(lane);
  const LaneAddr rar = A::row_addr<DR>(lane);
  const LaneAddr ta = A::tr_addr<DV>(lane);
  // the walk: the keys below the diagonal of the block's last row (at most n_k of them; none: the block's rows admit no key)
  const int kend = max(0, min(nq, qb * 128 + 128) + DELTA);
  const int nt = (kend + BN - 1) / BN;
  BidirStager<T, DN, BN, 256> skn;
  BidirStager<T, DR, BN, 256> skr;
  BidirStager<T, DV, BN, 256> sv;
  skn.init(tid, k_ld);
  skr.init(tid, DR);
  sv.init(tid, v_ld);
  if (nt > 0) {   // wave-uniform, the whole workgroup
    bidir_load(skn, knrs, 0);
    bidir_load(skr, krrs, 0);
    bidir_load(sv, vrs, 0);
    skn.store(smem);
    skr.store(smem + OFF_R);
    sv.store(smem + OFF_V);
    __syncthreads();
  }

  auto tile = [&](auto par, int t) {
    constexpr int PAR = decltype(par)::value;
    const int kbase = t * BN;
    const bool more = t + 1 < nt;
    if (more) {
      bidir_load(skn, knrs, kbase + BN);
      bidir_load(skr, krrs, kbase + BN);
      bidir_load(sv, vrs, kbase + BN);
    }
    lds_char* tkn = smem + PAR * TBN;
    lds_char* tkr = smem + OFF_R + PAR * TBR;
    lds_char* tv = smem + OFF_V + PAR * TBV;
    if (q0 < nq && kbase <= q0 + 31 + DELTA) {   // wave-uniform: some row of the wave admits a key of this tile
      f32x16 s[KT];
      auto scores = [&]() {   // S^T tile of this wave (raw units): the nope columns, then the pe columns; masked above the diagonal
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
          s[kt] = zero16();
#pragma unroll
          for (int kc = 0; kc < KCN; ++kc) A::mma(s[kt], A::row_frag<DN>(tkn, ran, 32 * kt, kc), qf[kc]);
#pragma unroll
          for (int kc = 0; kc < KCR; ++kc) A::mma(s[kt], A::row_frag<DR>(tkr, rar, 32 * kt, kc), qf[KCN + kc]);
          if (kbase + 32 * kt + 31 > q0 + DELTA) {   // wave-uniform: not wholly below the first row's diagonal
#pragma unroll
            for (int i = 0; i < 16; ++i)
              if (kbase + 32 * kt + acc_row(i, h) > qrow + DELTA) s[kt][i] = -INFINITY;
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
              A::mma(acc_o[dt], A::tr_frag<DV>(tv, ta, 32 * kt + 16 * s2, dt), pf[kt][s2]);
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
              const frag vt = A::tr_frag<DV>(tv, ta, 32 * kt + 16 * s2, dt);
              A::mma(acc_o[dt], vt, pf[kt][s2]);
              A::mma(acc_o[dt], vt, pl[kt][s2]);
            }
      }
    }
    if (more) {
      skn.store(smem + (PAR ^ 1) * TBN);
      skr.store(smem + OFF_R + (PAR ^ 1) * TBR);
      sv.store(smem + OFF_V + (PAR ^ 1) * TBV);
    }
    __syncthreads();
  };
  int t = 0;
  for (; t + 1 < nt; t += 2) {
    tile(ic<0>{}, t);
    tile(ic<1>{}, t + 1);
  }
  if (t < nt) tile(ic<0>{}, t);

  const float l_tot = xhalf_sum(l_run);   // 0 for a row that admits no key: it comes back as zeros, as rows no sequence owns
  if (qvalid) {
    const bool empty = !(l_tot > 0.f);
    const float inv = empty ? 0.f : 1.0f / l_tot;
    float* orow = o + (size_t)(sq_ + qrow) * ldo + (size_t)bh * DV;
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

}  // namespace fa
