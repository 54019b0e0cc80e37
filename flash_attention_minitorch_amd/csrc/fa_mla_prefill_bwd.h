// MLA prefill backward: dQ, dK_nope, dK_pe and dV of fa_mla_prefill.h's attention (192 score columns = k_nope per head | k_pe per
// token, 128 value columns) on MI355X (gfx950): the backward kernels of libflash_attn_mi355x_mla_prefill.so, written against
// fa_atoms.h.  bf16 operands, fp32 gradients.  Semantics, block maps, loads and schedule kernel are the forward's (fa_prefix.h's and
// fa_bidir.h's, used as they are); the walks, the masking, the row constants (bwd_prep_kernel<bf16, 128> of fa_bwd_dkdv.h on out and
// dO, both 128 wide) and the pack + pack_lo path for rows with few admissible keys are prefix_dq_kernel's and prefix_dkdv_kernel's.
// What is new is the split operand and the head-shared k_pe:
//
//   * mla_prefill_dq_kernel, query-stationary: a workgroup = 4 waves x 32 rows of one (head, 128-row map entry).  A lane holds its
//     row of Q as 12 fragments and of dO as 8.  Keys come in tiles of MLAP_BWD_BN = 32 rows as three LDS images (k_nope, k_pe, v),
//     double buffered.  S^T accumulates over the nope image and then the pe image (12 k-steps), dP^T over the v image (8 k-steps,
//     seeded with -delta), dS = P * dP, and dQ^T[192] += [k_nope | k_pe]^T dS^T through transposed reads of the k_nope and k_pe
//     images: 6 accumulator tiles, 4 + 2.
//     The key tile is 32 rows (prefix_dq_kernel's), not the forward's 64: 40 KB of LDS instead of 80, one S and one dP tile and 20
//     staging registers instead of two of each and 40.  Operands and accumulators are 12 * 4 + 8 * 4 + 6 * 16 + 16 = 192 registers
//     and the compiler's allocation is 362 (256 + 106 accumulator registers), so a SIMD holds one wave either way; a 64-key tile
//     would halve the barriers per key for about 50 registers more.  Chosen from the budget, not profiled.
//
//   * mla_prefill_dkdv_kernel, key-stationary: a workgroup = 4 waves x 32 keys of one 128-key map entry and a GROUP of heads.  Every
//     head reads the same k_pe row, so dK_pe is a sum over heads: a wave keeps the 4 k_pe fragments of its keys and the 2 dK_pe^T
//     accumulator tiles for the whole group, and for the current head the 8 k_nope and 8 v fragments and the 4 + 4 dK_nope^T / dV^T
//     tiles (240 registers of operands and accumulators by the count; the v fragments are parked in a wave-private piece of LDS, see
//     there: 502 registers, 72.5 KB of LDS).  The workgroup sweeps, head after head, the 32-query slices that admit a key of the
//     block (64-query slices cost 20 more staging registers and ended in scratch): Q as a 128-wide and a 64-wide LDS image, dO as a
//     128-wide one and the slice's two row constants, double buffered ACROSS the head change (the last slice of a head prefetches the first of the next).  At a head change the wave stores
//     dk_nope and dv of the finished head, zeroes those tiles and reloads k_nope and v; k_pe and the dK_pe tiles stay.  After its
//     last head it stores ONE dK_pe partial: into [group][Tk][64] of the workspace, or straight into dk_pe when H fits one group.
//     The walk crosses heads, so the stage buffer's parity is a run-time value here (a dozen address adds per slice against 40
//     MFMAs; the two-copy form with a compile-time parity spilled more), not a template argument as in the kernels above.
//
//   * mla_prefill_dkpe_sum_kernel adds the group partials in group order into the rows of dk_pe that a sequence owns (more than one
//     group only), and mla_prefill_bwd_fill_kernel zeroes the rows of dk_nope and dv that no sequence owns (the schedule kernel's
//     fill writes whole rows of one stride; these two have strides of their own and may be views of one buffer).
//
// Heads per group, mla_prefill_heads_per_group(H) = clamp(H / 16, 2, 8): a function of H alone, so that the order in which the heads
// are summed into dK_pe depends on neither Tk nor nseq (the per-sequence bit law).  A SUPPOSITION, nothing here has been profiled.
// What it trades: a larger group reads k_pe and writes a dK_pe partial (256 bytes per key) once per more heads, and shrinks the grid
// by as much.  H / 16 keeps 16 groups from H = 32 to 128: a 4096-token prompt is 32 key blocks, 512 workgroups on 256 CUs, and the
// partials are 16 * 256 bytes per key against H * 1024 bytes of dk_nope and dv.  Below H = 32 two heads still share every k_pe load
// and partial (12.5% of the dk_nope + dv bytes); H = 16 then has 8 groups, 256 workgroups at 4096 tokens, of which the causal sweep
// makes the later blocks short: it may underfill the machine.  Past H = 128 the group stays at 8 heads and the grid grows.
// No atomics, a fixed summation order.
#pragma once
#include "fa_mla_prefill.h"

namespace fa {

constexpr int MLAP_BWD_BN = 32;                   // key rows per tile of the dQ kernel
constexpr int MLAP_BWD_NW = 4, MLAP_BWD_QS = 32;  // dK/dV: waves (x 32 keys) per block, query rows per slice
constexpr int MLAP_BWD_BK = 32 * MLAP_BWD_NW;
__host__ __device__ constexpr int mla_prefill_heads_per_group(int H) { return H >= 128 ? 8 : H >= 32 ? H / 16 : 2; }

// ---------------------------------------------------------------------------------------------
// Backward dQ, query-stationary.  nlc = -L / tau and ndelta = -rowsum(dO * O), [H][Tq] each.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
mla_prefill_dq_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k_nope, const bf16_t* __restrict__ k_pe,
                      const bf16_t* __restrict__ v, const bf16_t* __restrict__ dout, const float* __restrict__ nlc,
                      const float* __restrict__ ndelta, float* __restrict__ dq, const int4* __restrict__ map, int Tq, int nblk, int BH,
                      int k_ld, int k_hs, int v_ld, int v_hs, float tau) {
  using T = bf16_t;
  using A = Atom<T>;
  typedef A::frag frag;
  constexpr int DN = MLAP_DN, DR = MLAP_DR, DQ = MLAP_DQ, DV = MLAP_DV, BN = MLAP_BWD_BN;
  constexpr int KCN = DN / 16, KCR = DR / 16, KCV = DV / 16, DTN = DN / 32, DTR = DR / 32;
  constexpr int TBN = A::tile_bytes<DN>(BN), TBR = A::tile_bytes<DR>(BN), TBV = A::tile_bytes<DV>(BN);
  constexpr int OFF_R = 2 * TBN, OFF_V = OFF_R + 2 * TBR;
  static_assert(BN == 32, "one S^T and one dP^T tile per key tile");
  __shared__ __attribute__((aligned(16))) char smem_raw[OFF_V + 2 * TBV];
  lds_char* smem = (lds_char*)smem_raw;

  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int bh, qb;   // bh: the head
  FA_BIDIR_LOCATE(qb)
  const int DELTA = nk - nq;   // wave-uniform
  const int q0 = qb * 128 + w * 32, qrow = q0 + r;
  const bool qvalid = qrow < nq;
  const bool careful = q0 + DELTA < 63 || nk < 64;   // wave-uniform: see mla_prefill_fwd_kernel
  const int ldq = BH * DQ, ldo = BH * DV;
  const rsrc_t qrs = make_rsrc(q + (size_t)sq_ * ldq + (size_t)bh * DQ, bidir_bytes<T, DQ>(nq, ldq));
  const rsrc_t dors = make_rsrc(dout + (size_t)sq_ * ldo + (size_t)bh * DV, bidir_bytes<T, DV>(nq, ldo));
  const rsrc_t knrs = make_rsrc(k_nope + (size_t)sk_ * k_ld + (size_t)bh * k_hs, bidir_bytes<T, DN>(nk, k_ld));
  const rsrc_t krrs = make_rsrc(k_pe + (size_t)sk_ * DR, bidir_bytes<T, DR>(nk, DR));
  const rsrc_t vrs = make_rsrc(v + (size_t)sk_ * v_ld + (size_t)bh * v_hs, bidir_bytes<T, DV>(nk, v_ld));
  const float c = tau * LOG2E;

  frag qf[KCN + KCR], dof[KCV];
#pragma unroll
  for (int kc = 0; kc < KCN + KCR; ++kc)
    qf[kc] = load_frag_buf<T>(qrs, (qrow * ldq + 16 * kc + 8 * h) * (int)sizeof(T));
#pragma unroll
  for (int kc = 0; kc < KCV; ++kc)
    dof[kc] = load_frag_buf<T>(dors, (qrow * ldo + 16 * kc + 8 * h) * (int)sizeof(T));
  // this lane's row constants; -delta, in every register, is the accumulator input of the dP^T tile
  const size_t rc0 = (size_t)bh * Tq + sq_;
  const float nlq = qvalid ? nlc[rc0 + qrow] * c : 0.f;   // -L * log2(e)
  const float ndq = qvalid ? ndelta[rc0 + qrow] : 0.f;
  f32x16 nd16;
#pragma unroll
  for (int i = 0; i < 16; ++i) nd16[i] = ndq;

  f32x16 acc_n[DTN], acc_r[DTR];   // dQ^T: the nope columns, the pe columns
#pragma unroll
  for (int dt = 0; dt < DTN; ++dt) acc_n[dt] = zero16();
#pragma unroll
  for (int dt = 0; dt < DTR; ++dt) acc_r[dt] = zero16();

  const LaneAddr ran = A::row_addr<DN>(lane);   // (k_nope and v: both 128 wide)
  const LaneAddr rar = A::row_addr<DR>(lane);
  const LaneAddr ta = A::tr_addr<DN>(lane);     // (the same for every width)
  const int kend = max(0, min(nq, qb * 128 + 128) + DELTA);   // the forward's walk
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
      f32x16 s, dp;
      A::mma_c(s, A::row_frag<DN>(tkn, ran, 0, 0), qf[0], zero16());
      A::mma_c(dp, A::row_frag<DV>(tv, ran, 0, 0), dof[0], nd16);
#pragma unroll
      for (int kc = 1; kc < KCN; ++kc) {
        A::mma(s, A::row_frag<DN>(tkn, ran, 0, kc), qf[kc]);
        A::mma(dp, A::row_frag<DV>(tv, ran, 0, kc), dof[kc]);
      }
#pragma unroll
      for (int kc = 0; kc < KCR; ++kc) A::mma(s, A::row_frag<DR>(tkr, rar, 0, kc), qf[KCN + kc]);
#pragma unroll
      for (int i = 0; i < 16; ++i) s[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[i], c, nlq));
      if (kbase + 31 > q0 + DELTA) {   // wave-uniform: the diagonal (keys past n_k lie above every real row's)
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (kbase + acc_row(i, h) > qrow + DELTA) s[i] = 0.f;
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) dp[i] = s[i] * dp[i];
      frag dsf[2];
      dsf[0] = A::pack(dp, 0);
      dsf[1] = A::pack(dp, 1);
      if (!careful) {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
#pragma unroll
          for (int dt = 0; dt < DTN; ++dt) A::mma(acc_n[dt], A::tr_frag<DN>(tkn, ta, 16 * s2, dt), dsf[s2]);
#pragma unroll
          for (int dt = 0; dt < DTR; ++dt) A::mma(acc_r[dt], A::tr_frag<DR>(tkr, ta, 16 * s2, dt), dsf[s2]);
        }
      } else {   // rows with few admissible keys: K^T dS^T also takes what the bf16 rounding of dS dropped
        frag dl[2];
        dl[0] = A::pack_lo(dp, 0, dsf[0]);
        dl[1] = A::pack_lo(dp, 1, dsf[1]);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
#pragma unroll
          for (int dt = 0; dt < DTN; ++dt) {
            const frag kt_ = A::tr_frag<DN>(tkn, ta, 16 * s2, dt);
            A::mma(acc_n[dt], kt_, dsf[s2]);
            A::mma(acc_n[dt], kt_, dl[s2]);
          }
#pragma unroll
          for (int dt = 0; dt < DTR; ++dt) {
            const frag kt_ = A::tr_frag<DR>(tkr, ta, 16 * s2, dt);
            A::mma(acc_r[dt], kt_, dsf[s2]);
            A::mma(acc_r[dt], kt_, dl[s2]);
          }
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

  if (qvalid) {   // (a row that admits no key added nothing: zeros)
    float* row = dq + (size_t)(sq_ + qrow) * ldq + (size_t)bh * DQ;
    auto store = [&](const f32x16& a, float* dst) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 val = {a[4 * g] * tau, a[4 * g + 1] * tau, a[4 * g + 2] * tau, a[4 * g + 3] * tau};
        *reinterpret_cast<f32x4*>(dst + 8 * g + 4 * h) = val;
      }
    };
#pragma unroll
    for (int dt = 0; dt < DTN; ++dt) store(acc_n[dt], row + 32 * dt);
#pragma unroll
    for (int dt = 0; dt < DTR; ++dt) store(acc_r[dt], row + DN + 32 * dt);
  }
}

// ---------------------------------------------------------------------------------------------
// Backward dK_nope / dK_pe / dV, key-stationary over a group of heads.  BH: the number of head groups (FA_BIDIR_LOCATE's "heads"),
// hpg heads each, the last one maybe fewer.  Key j is admitted by the queries i >= j - D.  dk_pe: where this launch's partials go,
// [group][Tk][64].
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64 * MLAP_BWD_NW)
mla_prefill_dkdv_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k_nope, const bf16_t* __restrict__ k_pe,
                        const bf16_t* __restrict__ v, const bf16_t* __restrict__ dout, const float* __restrict__ nlc,
                        const float* __restrict__ ndelta, float* __restrict__ dk_nope, float* __restrict__ dk_pe, float* __restrict__ dv,
                        const int4* __restrict__ map, int Tq, int Tk, int nblk, int BH, int H, int hpg, int k_ld, int k_hs, int v_ld,
                        int v_hs, int dk_ld, int dk_hs, int dv_ld, int dv_hs, float tau) {
  using T = bf16_t;
  using A = Atom<T>;
  typedef A::frag frag;
  constexpr int DN = MLAP_DN, DR = MLAP_DR, DQ = MLAP_DQ, DV = MLAP_DV, QS = MLAP_BWD_QS, BK = MLAP_BWD_BK, NT = 64 * MLAP_BWD_NW;
  constexpr int KCN = DN / 16, KCR = DR / 16, KCV = DV / 16, DTN = DN / 32, DTR = DR / 32, DTV = DV / 32, NSUB = QS / 32;
  constexpr int TBN = A::tile_bytes<DN>(QS), TBR = A::tile_bytes<DR>(QS), TBO = A::tile_bytes<DV>(QS);
  constexpr int OFF_R = TBN, OFF_O = OFF_R + TBR, OFF_C = OFF_O + TBO;
  constexpr int BUF = OFF_C + 8 * QS;   // Q's nope columns, Q's pe columns, dO, QS x nlc, QS x -delta
  constexpr int OFF_VF = 2 * BUF, VFB = KCV * 64 * 16;   // behind the stage buffers: each wave's V fragments, lane-linear
  __shared__ __attribute__((aligned(16))) char smem_raw[OFF_VF + MLAP_BWD_NW * VFB];
  lds_char* smem = (lds_char*)smem_raw;

  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int bh, kb;   // bh: the head group
  FA_BIDIR_LOCATE(kb)
  const int DELTA = nk - nq;   // wave-uniform
  const int kb0 = kb * BK, kw0 = kb0 + w * 32, key = kw0 + r;
  const int h0 = bh * hpg, h1 = min(H, h0 + hpg);   // the group's heads
  // wave-uniform: prefix_dkdv_kernel's rule for few keys, and for many queries on few keys
  const bool thin = nk < 64 || 32L * nq > (long)nk * nk;
  const int ldq = H * DQ, ldo = H * DV;
  const float c = tau * LOG2E;

  frag kpf[KCR];   // the keys' k_pe: every head's
  {
    const rsrc_t krrs = make_rsrc(k_pe + (size_t)sk_ * DR, bidir_bytes<T, DR>(nk, DR));
#pragma unroll
    for (int kc = 0; kc < KCR; ++kc) kpf[kc] = load_frag_buf<T>(krrs, (key * DR + 16 * kc + 8 * h) * (int)sizeof(T));   // rows >= nk: zero
  }
  // The V fragments live in a wave-private piece of LDS that only their own lane writes and reads (no barrier): with them in
  // registers the allocation ends in scratch, since every MFMA tile of this library is held in arch VGPRs and 12 tiles are.
  lds_char* vfl = smem + OFF_VF + w * VFB + 16 * lane;
  frag knf[KCN];
  auto load_head = [&](int hd) __attribute__((always_inline)) {
    const rsrc_t knrs = make_rsrc(k_nope + (size_t)sk_ * k_ld + (size_t)hd * k_hs, bidir_bytes<T, DN>(nk, k_ld));
    const rsrc_t vrs = make_rsrc(v + (size_t)sk_ * v_ld + (size_t)hd * v_hs, bidir_bytes<T, DV>(nk, v_ld));
#pragma unroll
    for (int kc = 0; kc < KCN; ++kc) knf[kc] = load_frag_buf<T>(knrs, (key * k_ld + 16 * kc + 8 * h) * (int)sizeof(T));
#pragma unroll
    for (int kc = 0; kc < KCV; ++kc) *FA_LDS(frag, vfl + 1024 * kc) = load_frag_buf<T>(vrs, (key * v_ld + 16 * kc + 8 * h) * (int)sizeof(T));
  };
  f32x16 acc_pe[DTR], acc_dk[DTN], acc_dv[DTV];
#pragma unroll
  for (int dt = 0; dt < DTR; ++dt) acc_pe[dt] = zero16();
#pragma unroll
  for (int dt = 0; dt < DTN; ++dt) {
    acc_dk[dt] = zero16();
    acc_dv[dt] = zero16();
  }

  const LaneAddr ran = A::row_addr<DN>(lane);   // (Q's nope columns and dO: both 128 wide)
  const LaneAddr rar = A::row_addr<DR>(lane);
  const LaneAddr ta = A::tr_addr<DN>(lane);     // (the same for every width)
  // the sweep of every head: slices qi_begin .. nqi - 1, from the first query that admits the block's first key (none: no query does)
  const int qi_begin = max(0, kb0 - DELTA) / QS, nqi = (nq + QS - 1) / QS;
  BidirStager<T, DN, QS, NT> sqn;
  BidirStager<T, DR, QS, NT> sqr;
  BidirStager<T, DV, QS, NT> sdo;
  sqn.init(tid, ldq);
  sqr.init(tid, ldq);
  sdo.init(tid, ldo);
  float st_nl = 0.f, st_de = 0.f;
  auto stage_load = [&](int hd, int qi) {   // (rows >= nq land as zeros)
    const bf16_t* qh = q + (size_t)sq_ * ldq + (size_t)hd * DQ;
    bidir_load(sqn, make_rsrc(qh, bidir_bytes<T, DQ>(nq, ldq)), qi * QS);
    bidir_load(sqr, make_rsrc(qh + DN, bidir_bytes<T, DR>(nq, ldq)), qi * QS);
    bidir_load(sdo, make_rsrc(dout + (size_t)sq_ * ldo + (size_t)hd * DV, bidir_bytes<T, DV>(nq, ldo)), qi * QS);
    if (tid < QS) {
      const int row = qi * QS + tid;
      const size_t rc = (size_t)hd * Tq + sq_ + row;
      st_nl = row < nq ? nlc[rc] : 0.f;
      st_de = row < nq ? ndelta[rc] : 0.f;
    }
  };
  auto stage_store = [&](lds_char* b) {
    sqn.store(b);
    sqr.store(b + OFF_R);
    sdo.store(b + OFF_O);
    if (tid < QS) {
      *FA_LDS(float, b + OFF_C + 4 * tid) = st_nl;
      *FA_LDS(float, b + OFF_C + 4 * QS + 4 * tid) = st_de;
    }
  };

  auto slice = [&](lds_char* buf, int qi) __attribute__((always_inline)) {
    lds_char* tqn = buf;
    lds_char* tqr = buf + OFF_R;
    lds_char* tdo = buf + OFF_O;
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub) {
      const int qi0 = qi * QS + 32 * sub;
      if (kw0 < nk && qi0 < nq && kw0 <= qi0 + 31 + DELTA) {   // wave-uniform: some query of the sub-slice admits a key of the wave
        // register i of lane half h is query qi0 + acc_row(i, h): its nlc / -delta come from LDS (broadcast reads) and ride in as
        // the accumulator inputs: S' = S - L/tau, dP' = dP - delta
        f32x16 nl16, nd16;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 a = *FA_LDS(f32x4, buf + OFF_C + 128 * sub + 16 * h + 32 * g);
          const f32x4 b = *FA_LDS(f32x4, buf + OFF_C + 4 * QS + 128 * sub + 16 * h + 32 * g);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            nl16[4 * g + j] = a[j];
            nd16[4 * g + j] = b[j];
          }
        }
        f32x16 s, dp;
        A::mma_c(s, A::row_frag<DN>(tqn, ran, 32 * sub, 0), knf[0], nl16);
        A::mma_c(dp, A::row_frag<DV>(tdo, ran, 32 * sub, 0), frag(*FA_LDS(frag, vfl)), nd16);
#pragma unroll
        for (int kc = 1; kc < KCN; ++kc) {
          A::mma(s, A::row_frag<DN>(tqn, ran, 32 * sub, kc), knf[kc]);
          A::mma(dp, A::row_frag<DV>(tdo, ran, 32 * sub, kc), frag(*FA_LDS(frag, vfl + 1024 * kc)));
        }
#pragma unroll
        for (int kc = 0; kc < KCR; ++kc) A::mma(s, A::row_frag<DR>(tqr, rar, 32 * sub, kc), kpf[kc]);
        // (query rows >= nq: Q, dO and the constants are zeros, P = 1 meets dO = 0 and dS = 0: nothing is added.  Keys >= nk are
        // lanes that are not stored.)
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = __builtin_amdgcn_exp2f(s[i] * c);
        if (kw0 + 31 > qi0 + DELTA) {   // wave-uniform: the unmasked path is taken only where every (query, key) pair is admitted
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (key > qi0 + acc_row(i, h) + DELTA) s[i] = 0.f;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) dp[i] = s[i] * dp[i];
        frag pf[2], dsf[2];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          pf[s2] = A::pack(s, s2);
          dsf[s2] = A::pack(dp, s2);
        }
        if (!(thin || qi0 + DELTA < 63)) {   // (the sub-slice's rows admit at least 64 keys)
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) {
#pragma unroll
            for (int dt = 0; dt < DTV; ++dt) {
              A::mma(acc_dv[dt], A::tr_frag<DV>(tdo, ta, 32 * sub + 16 * s2, dt), pf[s2]);
              A::mma(acc_dk[dt], A::tr_frag<DN>(tqn, ta, 32 * sub + 16 * s2, dt), dsf[s2]);
            }
#pragma unroll
            for (int dt = 0; dt < DTR; ++dt) A::mma(acc_pe[dt], A::tr_frag<DR>(tqr, ta, 32 * sub + 16 * s2, dt), dsf[s2]);
          }
        } else {   // few keys: the products also take what the bf16 rounding of P, dS dropped
          frag pl[2], dl[2];
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) {
            pl[s2] = A::pack_lo(s, s2, pf[s2]);
            dl[s2] = A::pack_lo(dp, s2, dsf[s2]);
          }
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) {
#pragma unroll
            for (int dt = 0; dt < DTV; ++dt) {
              const frag adoT = A::tr_frag<DV>(tdo, ta, 32 * sub + 16 * s2, dt);
              const frag aqT = A::tr_frag<DN>(tqn, ta, 32 * sub + 16 * s2, dt);
              A::mma(acc_dv[dt], adoT, pf[s2]);
              A::mma(acc_dv[dt], adoT, pl[s2]);
              A::mma(acc_dk[dt], aqT, dsf[s2]);
              A::mma(acc_dk[dt], aqT, dl[s2]);
            }
#pragma unroll
            for (int dt = 0; dt < DTR; ++dt) {
              const frag aqT = A::tr_frag<DR>(tqr, ta, 32 * sub + 16 * s2, dt);
              A::mma(acc_pe[dt], aqT, dsf[s2]);
              A::mma(acc_pe[dt], aqT, dl[s2]);
            }
          }
        }
      }
    }
  };
  auto store_tile = [&](const f32x16& a, float* dst, float f) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x4 val = {a[4 * g] * f, a[4 * g + 1] * f, a[4 * g + 2] * f, a[4 * g + 3] * f};
      *reinterpret_cast<f32x4*>(dst + 8 * g + 4 * h) = val;
    }
  };

  auto store_head = [&](int hd) __attribute__((always_inline)) {   // dk_nope and dv of one head
    if (key < nk) {
      float* dkrow = dk_nope + (size_t)(sk_ + key) * dk_ld + (size_t)hd * dk_hs;
      float* dvrow = dv + (size_t)(sk_ + key) * dv_ld + (size_t)hd * dv_hs;
#pragma unroll
      for (int dt = 0; dt < DTN; ++dt) {
        store_tile(acc_dk[dt], dkrow + 32 * dt, tau);
        store_tile(acc_dv[dt], dvrow + 32 * dt, 1.0f);
      }
    }
  };
  const bool sweeps = qi_begin < nqi;   // wave-uniform, the whole workgroup (no slice: every gradient of the block is zero)
  int par = 0;
  if (sweeps) {
    load_head(h0);
    stage_load(h0, qi_begin);
    stage_store(smem);
    __syncthreads();
  }
  for (int hd = h0; hd < h1; ++hd) {
    if (sweeps) {
      for (int qi = qi_begin; qi < nqi; ++qi) {
        const bool last = qi + 1 == nqi;
        const bool more = !last || hd + 1 < h1;   // the next slice: this head's, or the first of the next head
        if (more) stage_load(last ? hd + 1 : hd, last ? qi_begin : qi + 1);
        slice(smem + par * BUF, qi);
        if (more) stage_store(smem + (par ^ 1) * BUF);
        __syncthreads();
        par ^= 1;
      }
    }
    store_head(hd);
    if (sweeps && hd + 1 < h1) {   // the head change: k_pe and the dK_pe tiles stay
#pragma unroll
      for (int dt = 0; dt < DTN; ++dt) {
        acc_dk[dt] = zero16();
        acc_dv[dt] = zero16();
      }
      load_head(hd + 1);
    }
  }
  if (key < nk) {
    float* prow = dk_pe + ((size_t)bh * Tk + sk_ + key) * DR;
#pragma unroll
    for (int dt = 0; dt < DTR; ++dt) store_tile(acc_pe[dt], prow + 32 * dt, tau);
  }
}

// dk_pe's owned rows = the group partials added in group order; one lane per 16 bytes.  (The unowned rows are the schedule
// kernel's: zeros.  Consecutive sequences leave no gap, so the owned rows are one range.)
__global__ void __launch_bounds__(256)
mla_prefill_dkpe_sum_kernel(const float* __restrict__ part, float* __restrict__ dk_pe, const int* __restrict__ cu_k, int nseq, int Tk,
                            int groups) {
  int lead, n0, sl, nl;
  seq_rows(cu_k, Tk, 0, lead, n0);
  seq_rows(cu_k, Tk, nseq - 1, sl, nl);
  constexpr int VPR = MLAP_DR / 4;
  const long i = (long)blockIdx.x * 256 + threadIdx.x + (long)lead * VPR;
  if (i >= (long)(sl + nl) * VPR) return;
  f32x4 sum = *reinterpret_cast<const f32x4*>(part + 4 * i);
  for (int g = 1; g < groups; ++g) sum += *reinterpret_cast<const f32x4*>(part + (size_t)g * Tk * MLAP_DR + 4 * i);
  *reinterpret_cast<f32x4*>(dk_pe + 4 * i) = sum;
}

// zeros in the rows of dk_nope and dv that no sequence owns: H heads x 128 columns under each one's strides
__global__ void __launch_bounds__(256)
mla_prefill_bwd_fill_kernel(const int* __restrict__ cu_k, int nseq, int Tk, int H, float* __restrict__ dk_nope, int dk_ld, int dk_hs,
                            float* __restrict__ dv, int dv_ld, int dv_hs) {
  int lead, n0, sl, nl;
  seq_rows(cu_k, Tk, 0, lead, n0);
  seq_rows(cu_k, Tk, nseq - 1, sl, nl);
  const int tail0 = sl + nl;
  constexpr int VPH = MLAP_DN / 4;
  const long total = ((long)lead + (Tk - tail0)) * H * VPH;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long u = i / (H * VPH);
    const int rest = (int)(i - u * (H * VPH)), hd = rest / VPH, col = 4 * (rest % VPH);
    const int row = u < lead ? (int)u : tail0 + (int)(u - lead);
    *reinterpret_cast<f32x4*>(dk_nope + (size_t)row * dk_ld + (size_t)hd * dk_hs + col) = zero;
    *reinterpret_cast<f32x4*>(dv + (size_t)row * dv_ld + (size_t)hd * dv_hs + col) = zero;
  }
}

}  // namespace fa
