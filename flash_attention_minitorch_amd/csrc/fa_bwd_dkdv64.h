// FlashAttention backward for MI355X (gfx950): the 64-keys-per-wave build of the tiled dK / dV slot kernel.
// Part of the kernel set described in fa_kernels.h (included from there, inside its include order).
#pragma once
#include "fa_common.h"

namespace fa {

// ---------------------------------------------------------------------------------------------
// Backward dK / dV, continuous slot pipeline, 4 waves x 64 keys (bf16, d = 64, non-causal, N a multiple of 256): what
// bwd_dkdv_slot_kernel<T, 64, false, true> computes, bit for bit, with HALF the LDS reads per MFMA.  The 256-key block, the 128-query
// stages, the three-slot LDS-DMA ring, the barrier per stage and the head-to-head hand-over are that kernel's; a workgroup is four
// waves, one per SIMD, and wave w owns keys 64 w .. 64 w + 63 of the block as two 32-key groups.  Every Q / dO row fragment, every
// transposed fragment and every row-constant register that comes out of LDS feeds the MFMAs of BOTH groups, back to back: one
// ds_read_b128 or one pair of ds_read_b64_tr_b16 per two MFMAs.  The per-key arithmetic and the order of the sum over queries are
// unchanged; only which wave owns a key differs.
// Registers (one wave per SIMD: the whole 512-entry file): dK^T, dV^T of both groups (128) and the K, V fragments (64) live in AGPRs
// for the whole sweep, through the explicit-class MFMA of fa_atoms.h (MfmaRC); S', dP', P, dS, the LDS fragments and all softmax
// VALU stay in arch VGPRs.
// A period is 32 slots: slot 2k + g holds the MFMA of slot k of bwd_dkdv_slot_kernel's period for key group g (one MFMA per
// sched_barrier-pinned slot).  The fillers are spread so that a slot of the folded-scale sweep carries at most one v_exp pair and 24
// issue cycles of VALU + LDS (exp 8, others 4): the dS' = P * dP' multiplies ride in the exp slots, a transposed fragment is requested
// again in the slot after the second MFMA that read it, and the next sub-slice's operands come in the last slots, which carry little
// else.  The fp32-scaling sweep has two more multiplies in each exp slot (32 cycles), as the 8-wave build has.
// hipcc pads nothing around an asm MFMA (MfmaRC), so the schedule itself keeps the distances: a fragment packed by VALU is consumed two
// slots later, S' / dP' tiles are read by VALU a period after their chain, the row constants stay allocated for two slots behind the
// MFMAs that read them as accumulator input, and the accumulators are read after the sweep behind mma_drain.
// A workgroup takes key block kb of up to lay.tiles consecutive heads; the last head group of a launch may be partial.
// ---------------------------------------------------------------------------------------------
template <typename T, int D>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
bwd_dkdv_slot64_kernel(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, const T* __restrict__ dout,
                       const float* __restrict__ nl2, const float* __restrict__ ndelta, float* __restrict__ dk,
                       float* __restrict__ dv, int N, int nkb, int BH, Layout lay, float tau) {
  if (guard_skip(lay)) return;   // guarded call: this launch is not the chosen one of its pair
  static_assert(D == 64 && sizeof(T) == 2, "slot schedule is laid out for bf16, d = 64");
  using A = Atom<T>;
  using M = MfmaRC;
  typedef typename A::frag frag;
  constexpr int KC = 4, QS = 128, NW = 4, KG = 2, KPW = 32 * KG, BK = NW * KPW;
  constexpr int TB = A::template tile_bytes<D>(QS);   // 16 KiB
  constexpr int BUF = 2 * TB + 8 * QS;                // Q tile, dO tile, QS x (-L), QS x (-delta)
  using RG = StageRing<D, QS, NW>;                    // DMA pieces and readers of a stage (fa_atoms.h): four pieces per wave and tensor
  static_assert(RG::dma_matches_image() && RG::NPW == 4, "LDS-DMA source swizzle vs Atom::off");
  __shared__ __attribute__((aligned(16))) char smem_raw[3 * BUF];
  lds_char* smem = (lds_char*)smem_raw;

  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tiles = max(lay.tiles, 1);   // heads per workgroup (the launcher sizes the grid with ceil(BH / tiles) head groups)
  int bh, kb;
  map_block(blockIdx.x, (BH + tiles - 1) / tiles, nkb, bh, kb);
  bh *= tiles;
  const int heads = min(tiles, BH - bh);   // (the last head group may be partial)
  size_t base = head_base(lay, bh);
  const int ld = lay.ld;
  const uint32_t mat_bytes = ((uint32_t)(N - 1) * ld + D) * (uint32_t)sizeof(T);
  // (ungrouped calls only, as every tiled build: K and V live where q does)
  rsrc_t krs = make_rsrc(k + base, mat_bytes), vrs = make_rsrc(v + base, mat_bytes);
  raw_rsrc_t qraw = make_raw_rsrc(q + base, mat_bytes), doraw = make_raw_rsrc(dout + base, mat_bytes);
  // Both scalings in one launch (Layout::scale_sel), as in bwd_dkdv_slot_kernel
  const bool exact = scale_exact(lay);   // wave-uniform
  const float* nlv = exact ? nl2 - 2 * (size_t)BH * N : nl2;
  raw_rsrc_t nlraw = make_raw_rsrc(nlv + (size_t)bh * N, (uint32_t)N * 4u);
  raw_rsrc_t ndraw = make_raw_rsrc(ndelta + (size_t)bh * N, (uint32_t)N * 4u);
  const float c = tau * LOG2E;
  const int kw0 = kb * BK + w * KPW;   // (N is a multiple of 256: every key of every wave exists)

  frag kl[KG][KC], vl[KG][KC];   // the tracked loads' landing registers (VGPRs), live from a head's request to its move into AGPRs
  auto load_kv = [&]() {
#pragma unroll
    for (int g = 0; g < KG; ++g)
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) {
        const int off = ((kw0 + 32 * g + r) * ld + 16 * kc + 8 * h) * (int)sizeof(T);
        kl[g][kc] = load_frag_buf<T>(krs, off);
        vl[g][kc] = load_frag_buf<T>(vrs, off);
      }
  };

  const LaneAddr ra = A::template row_addr<D>(lane);
  const LaneAddr ta = A::template tr_addr<D>(lane);
  const int nst = N / QS;
  const uint32_t smem_addr = (uint32_t)(uintptr_t)smem;
  // LDS-DMA: wave w moves pieces w, w + 4, w + 8, w + 12 (1 KiB = one 8-row group) of the Q and of the dO tile, and a half of one
  // row-constant vector
  FA_DMA_VOFF(dma_voff, RG::PPG, lane, w, ld, (int)sizeof(T));
  auto stage_dma = [&](int st, int dst) {
#pragma unroll
    for (int i = 0; i < RG::NPW; ++i) {
      const int g = w + NW * i;
      const int soff = (st * QS + 8 * g) * ld * (int)sizeof(T);
      dma16(qraw, smem_addr + dst + 1024 * g, dma_voff, soff);
      dma16(doraw, smem_addr + dst + TB + 1024 * g, dma_voff, soff);
    }
    const int half = w & 1;
    dma4((w < 2) ? nlraw : ndraw, smem_addr + dst + 2 * TB + ((w < 2) ? 0 : 4 * QS) + 256 * half, 4 * lane, (st * QS + 64 * half) * 4);
  };
  int roff = 0;   // ring position of the current head's stage 0
  auto slot_of = [&](int st) { return ring_slot<3, BUF>(st, roff); };

  // (two copies of the sweep, one per scaling: the fp32 multiply of the exact one exists in its own instruction stream only)
  auto sweep = [&](auto ex_c) {
  constexpr bool EX = decltype(ex_c)::value != 0;
  frag ka[KG][KC], va[KG][KC];          // AGPRs
  f32x16 acc_dk[KG][2], acc_dv[KG][2];  // AGPRs
  f32x16 sA[KG], dpA[KG], sB[KG], dpB[KG], cS, cD;
  frag pf0[KG], pf1[KG], df0[KG], df1[KG], rq[4], rdo[4], tf[4];
  auto SB = [&]() { __builtin_amdgcn_sched_barrier(0); };
  auto ld_c = [&](f32x16& x, int hb /* stage base + 16 * h */, int off, int sub) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 a = *FA_LDS(f32x4, smem + hb + 2 * TB + off + 128 * sub + 32 * g);
#pragma unroll
      for (int j = 0; j < 4; ++j) x[4 * g + j] = a[j];
    }
  };
  auto me = [&](f32x16& x, int i) { x[i] = EX ? __builtin_amdgcn_exp2f(x[i] * c) : __builtin_amdgcn_exp2f(x[i]); };
  // One period.  SN: sub-slice whose S', dP' are produced, rows at (nr0, nr1) [its dO rows 1..3 are requested here]; SC: sub-slice in
  // the softmax / dV, dK stream, transposed reads at (ct0, ct1); SP: the sub-slice after SN, whose Q rows, row constants and first
  // dO row are requested in slots 24-30 at (pr0, pr1, ph16).  HC = false: the pipeline fills (S', dP' alone).
  auto period = [&](auto hc_c, auto subn_c, auto subc_c, auto subp_c, int nr0, int nr1, int ct0, int ct1, int pr0, int pr1, int ph16,
                    f32x16(&ns)[KG], f32x16(&ndp)[KG], f32x16(&cs)[KG], f32x16(&cdp)[KG]) {
    constexpr bool HC = decltype(hc_c)::value != 0;
    constexpr int SN = decltype(subn_c)::value, SC = decltype(subc_c)::value, SP = decltype(subp_c)::value;
    auto mu = [&](int g, int i) { cdp[g][i] = cs[g][i] * cdp[g][i]; };   // dS' = P * dP'
#pragma unroll
    for (int kq = 0; kq < 4; ++kq)   // slots 0-7: S' chains | exp of scores 0..7, dS' 1..3 | dO rows 1..3
#pragma unroll
      for (int g = 0; g < KG; ++g) {
        if (kq == 0) M::vs_c(ns[g], rq[0], ka[g][0], cS);
        else M::vs(ns[g], rq[kq], ka[g][kq]);
        SB();
        if (g == 0 && kq < 3) rdo[kq + 1] = RG::row(smem, nr0, nr1, SN, kq + 1, TB);
        if constexpr (HC) {
          me(cs[g], 2 * kq); me(cs[g], 2 * kq + 1);
          if (kq) mu(g, kq);
        }
        if (kq == 1 && g == KG - 1) asm volatile("" ::"v"(cS));   // (see cD below)
        SB();
      }
#pragma unroll
    for (int g = 0; g < KG; ++g) {   // slots 8, 9: dP' chains open | P fragment 0 | first transposed dO fragment
      M::vs_c(ndp[g], rdo[0], va[g][0], cD);
      SB();
      if constexpr (HC) {
        pf0[g] = A::pack(cs[g], 0);
        if (g == 0) tf[0] = RG::tr(smem, ct0, ct1, SC, 0, 0, TB);
        else { mu(0, 0); mu(1, 0); }
      }
      SB();
    }
#pragma unroll
    for (int kq = 1; kq < 4; ++kq)   // slots 10-15: | exp of scores 8..13, dS' 4..6 | transposed dO fragments
#pragma unroll
      for (int g = 0; g < KG; ++g) {
        M::vs(ndp[g], rdo[kq], va[g][kq]);
        SB();
        if constexpr (HC) {
          me(cs[g], 6 + 2 * kq); me(cs[g], 7 + 2 * kq);
          if (g == 0) tf[kq] = RG::tr(smem, ct0, ct1, SC, kq >> 1, kq & 1, TB);
          else { mu(0, 3 + kq); mu(1, 3 + kq); }
        }
        // an MFMA reads its accumulator input over its passes: the row constants stay allocated for two slots behind the chain
        // heads that read them, so no VALU result can land in their registers meanwhile (hipcc does not see the asm MFMA's hazard)
        if (kq == 1 && g == KG - 1) asm volatile("" ::"v"(cD));
        SB();
      }
    // slots 16-31: dV^T += dO^T P, dK^T += Q^T dS of both groups; a transposed fragment is requested again (Q for dO) in the slot
    // after the second MFMA that read it; the operands of sub-slice SP in the slots that carry little VALU
#pragma unroll
    for (int g = 0; g < KG; ++g) {   // slots 16, 17
      if constexpr (HC) {
        M::ag(acc_dv[g][0], tf[0], pf0[g]);
        SB();
        me(cs[g], 14); me(cs[g], 15);
        mu(g, 7);
      }
      SB();
    }
#pragma unroll
    for (int g = 0; g < KG; ++g) {   // slots 18, 19
      if constexpr (HC) {
        M::ag(acc_dv[g][1], tf[1], pf0[g]);
        SB();
        pf1[g] = A::pack(cs[g], 1);
        if (g == 0) tf[0] = RG::tr(smem, ct0, ct1, SC, 0, 0, 0);
      }
      SB();
    }
#pragma unroll
    for (int g = 0; g < KG; ++g) {   // slots 20, 21
      if constexpr (HC) {
        M::ag(acc_dv[g][0], tf[2], pf1[g]);
        SB();
        df0[g] = A::pack(cdp[g], 0);
        if (g == 0) tf[1] = RG::tr(smem, ct0, ct1, SC, 0, 1, 0);
      }
      SB();
    }
#pragma unroll
    for (int g = 0; g < KG; ++g) {   // slots 22, 23
      if constexpr (HC) {
        M::ag(acc_dv[g][1], tf[3], pf1[g]);
        SB();
#pragma unroll
        for (int i = 8; i < 12; ++i) mu(g, i);
        if (g == 0) tf[2] = RG::tr(smem, ct0, ct1, SC, 1, 0, 0);
      }
      SB();
    }
#pragma unroll
    for (int g = 0; g < KG; ++g) {   // slots 24, 25
      if constexpr (HC) {
        M::ag(acc_dk[g][0], tf[0], df0[g]);
        SB();
#pragma unroll
        for (int i = 12; i < 16; ++i) mu(g, i);
        if (g == 0) tf[3] = RG::tr(smem, ct0, ct1, SC, 1, 1, 0);
      }
      if (g == 1) {
        rq[0] = RG::row(smem, pr0, pr1, SP, 0, 0);
        rq[1] = RG::row(smem, pr0, pr1, SP, 1, 0);
      }
      SB();
    }
#pragma unroll
    for (int g = 0; g < KG; ++g) {   // slots 26, 27
      if constexpr (HC) {
        M::ag(acc_dk[g][1], tf[1], df0[g]);
        SB();
        df1[g] = A::pack(cdp[g], 1);
      }
      if (g == 0) {
        rq[2] = RG::row(smem, pr0, pr1, SP, 2, 0);
        rq[3] = RG::row(smem, pr0, pr1, SP, 3, 0);
      } else {
        rdo[0] = RG::row(smem, pr0, pr1, SP, 0, TB);
      }
      SB();
    }
#pragma unroll
    for (int g = 0; g < KG; ++g) {   // slots 28, 29
      if constexpr (HC) { M::ag(acc_dk[g][0], tf[2], df1[g]); SB(); }
      if (g == 0) ld_c(cS, ph16, 0, SP);
      else ld_c(cD, ph16, 4 * QS, SP);
      SB();
    }
#pragma unroll
    for (int g = 0; g < KG; ++g) {   // slots 30, 31
      if constexpr (HC) { M::ag(acc_dk[g][1], tf[3], df1[g]); SB(); }
    }
  };
  // A head's fragments go from their landing registers into AGPRs (K scaled on the way) and its accumulators are cleared there: for
  // the first head here, for every other one behind the stores of the head before it (its loads were requested in front of them).
  auto install = [&]() {
#pragma unroll
    for (int g = 0; g < KG; ++g)
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) {
        ka[g][kc] = M::to_agpr(EX ? kl[g][kc] : A::scale(kl[g][kc], c));
        va[g][kc] = M::to_agpr(vl[g][kc]);
      }
    const frag z = A::zero();
#pragma unroll
    for (int g = 0; g < KG; ++g)
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        M::ag_z(acc_dk[g][dt], z, z);
        M::ag_z(acc_dv[g][dt], z, z);
      }
  };
  // the first head: its stage 0 and its fragments (inside each copy of the sweep, and consumed at once: a landing register that
  // lives across the branch between the copies is spilled by hipcc)
  stage_dma(0, slot_of(0));
  load_kv();
  install();
  dma_wait_all();
  __syncthreads();
  auto T1 = ic<1>{};
  auto T0 = ic<0>{};
  const int st0 = 0;
  for (int t = 0; t < heads; ++t) {
  const int b0 = slot_of(st0);   // addresses of the current stage
  int cr0 = ra.b[0] + b0, cr1 = ra.b[1] + b0, ct0 = ta.b[0] + b0, ct1 = ta.b[1] + b0, ch16 = 16 * h + b0;
  // operands of sub-slice 0, then its S', dP' alone (the pipeline fills)
#pragma unroll
  for (int kc = 0; kc < 4; ++kc) rq[kc] = RG::row(smem, cr0, cr1, 0, kc, 0);
  ld_c(cS, ch16, 0, 0);
  ld_c(cD, ch16, 4 * QS, 0);
  rdo[0] = RG::row(smem, cr0, cr1, 0, 0, TB);
  SB();
  period(T0, ic<0>{}, ic<0>{}, ic<1>{}, cr0, cr1, ct0, ct1, cr0, cr1, ch16, sA, dpA, sB, dpB);
  for (int st = st0; st < nst; ++st) {
    const int nb = slot_of(st + 1);
    const int nr0 = ra.b[0] + nb, nr1 = ra.b[1] + nb, nh16 = 16 * h + nb;
    if (st + 1 < nst) stage_dma(st + 1, nb);
    else if (t + 1 < heads) {   // the next head's sweep: its stage 0 follows in the ring
      const size_t nbase = head_base(lay, bh + 1);
      qraw = make_raw_rsrc(q + nbase, mat_bytes);
      doraw = make_raw_rsrc(dout + nbase, mat_bytes);
      nlraw = make_raw_rsrc(nlv + (size_t)(bh + 1) * N, (uint32_t)N * 4u);
      ndraw = make_raw_rsrc(ndelta + (size_t)(bh + 1) * N, (uint32_t)N * 4u);
      stage_dma(0, nb);
    }
    period(T1, ic<1>{}, ic<0>{}, ic<2>{}, cr0, cr1, ct0, ct1, cr0, cr1, ch16, sB, dpB, sA, dpA);
    period(T1, ic<2>{}, ic<1>{}, ic<3>{}, cr0, cr1, ct0, ct1, cr0, cr1, ch16, sA, dpA, sB, dpB);
    dma_wait_all();   // this wave's pieces of the next stage have landed
    __syncthreads();
    // sub-slice 0 of the next stage is requested from here on (after the last stage: stale data, results unused)
    period(T1, ic<3>{}, ic<2>{}, ic<0>{}, cr0, cr1, ct0, ct1, nr0, nr1, nh16, sB, dpB, sA, dpA);
    period(T1, ic<0>{}, ic<3>{}, ic<1>{}, nr0, nr1, ct0, ct1, nr0, nr1, nh16, sA, dpA, sB, dpB);
    cr0 = nr0; cr1 = nr1; ch16 = nh16;
    ct0 = ta.b[0] + nb; ct1 = ta.b[1] + nb;
  }
  // hand over to the next head: its fragments are requested before this head's stores are issued
  float* dkrow = dk + base + (size_t)(kw0 + r) * ld;
  float* dvrow = dv + base + (size_t)(kw0 + r) * ld;
  if (t + 1 < heads) {
    ++bh;
    base = head_base(lay, bh);
    krs = make_rsrc(k + base, mat_bytes);
    vrs = make_rsrc(v + base, mat_bytes);
    load_kv();
    roff = (roff + nst) % 3;
  }
  M::mma_drain(acc_dk, acc_dv);
#pragma unroll
  for (int g2 = 0; g2 < KG; ++g2)
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      const f32x16 xk = acc_dk[g2][dt], xv = acc_dv[g2][dt];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 a = {xk[4 * g] * tau, xk[4 * g + 1] * tau, xk[4 * g + 2] * tau, xk[4 * g + 3] * tau};
        f32x4 b = {xv[4 * g], xv[4 * g + 1], xv[4 * g + 2], xv[4 * g + 3]};
        *reinterpret_cast<f32x4*>(dkrow + (size_t)32 * g2 * ld + 32 * dt + 8 * g + 4 * h) = a;
        *reinterpret_cast<f32x4*>(dvrow + (size_t)32 * g2 * ld + 32 * dt + 8 * g + 4 * h) = b;
      }
    }
  if (t + 1 < heads) install();
  }   // heads of this workgroup
  };
  if (exact) sweep(ic<1>{});
  else sweep(ic<0>{});
}

}  // namespace fa
