// The three kernels of fa_window.h, included by that file INSIDE namespace fa: plain text, not a header (no #pragma once), read
// once per build.  In scope: the FA_WIN_* hooks of fa_window.h, FA_WIN_NAME (the kernel's name in this build), FA_WIN_CAP (1: the
// soft-capping build), FA_WIN_CAP_PARAM (its extra argument) and FA_WIN_CAP_VALUE (the cap, 0.f in the other build); FA_WIN_LSINK
// (1: the forward ends its rows with a learned sink logit), FA_WIN_LSINK_PARAM (the forward's extra arguments) and
// FA_WIN_LSINK_LOGIT (the row's logit, 0.f in the other builds).
//
// The cap builds (CAP): k2 = cap_k2(tau, softcap) once per workgroup, r = cap_rcp(s, k2) and z = cap_z(r, softcap) per score, in
// front of the masks (a mask applied first would come out of the cap as -softcap, an admitted key).  From there the scores are the
// logits: the softmax constant is log2(e), lse = m_ref + ln l, and the backward's row constant is nlc = -lse (bwd_prep_kernel
// launched with 1 for 1 / tau).  The chain rule through the cap, dS = dZ * (1 - tanh^2) * tau, takes 1 - tanh^2 = 4 r (1 - r) from
// the same r (cap_slope): no further transcendental, 0 at both saturations, finite for every finite score.  The closing * tau on dQ
// and dK is the one every build has.  The split-operand rules (careful, the sink waves) are the same in both builds.
// ---------------------------------------------------------------------------------------------
// Forward, query-stationary: a workgroup = 4 waves = 128 query rows, as fwd_kernel.  P = exp2(c*s - c*m_ref) against a per-row
// reference that only moves when a lane's partial row sum would pass 2^6 (fa_fwd.h); a row has no reference until the first tile in
// which it admits a key (under a short window that is not the wave's first tile), and a tile in which some row of the wave still
// lacks one takes the classic step (tile maximum, reference moved, O and l rescaled).
// ---------------------------------------------------------------------------------------------
template <typename T, int D, int BN>
__global__ void __launch_bounds__(256)
FA_WIN_NAME(fwd)(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, float* __restrict__ o,
                   float* __restrict__ lse, FA_WIN_GEOM_PARAMS, Layout lay, float tau, FA_WIN_MASK_PARAMS FA_WIN_CAP_PARAM
                   FA_WIN_LSINK_PARAM) {
  using A = Atom<T>;
  typedef typename A::frag frag;
  constexpr int KC = D / 16, KT = BN / 32, DT = D / 32;
  constexpr int TB = A::template tile_bytes<D>(BN);
  __shared__ __attribute__((aligned(16))) char smem_raw[4 * TB];
  lds_char* smem = (lds_char*)smem_raw;

  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int bh, qb;
  FA_WIN_LOCATE(qb, nblk)
  const int q0 = qb * 128 + w * 32, qrow = q0 + r;
  const bool qvalid = qrow < N;
  const bool careful = A::SPLITS && (W + S < 64 || q0 < 64);   // wave-uniform: the wave's rows may admit fewer than 64 keys
  const int ld = lay.ld;
  const size_t base = head_base(lay, bh) + FA_WIN_ROW0 * ld;
  const uint32_t mat_bytes = ((uint32_t)(N - 1) * ld + D) * (uint32_t)sizeof(T);
  const rsrc_t qrs = make_rsrc(q + base, mat_bytes);
  const int ldk = lay.ldk;
  const size_t kvb = kv_base<D>(lay, bh, N) + FA_WIN_ROW0 * ldk;
  const uint32_t kv_bytes = ((uint32_t)(N - 1) * ldk + D) * (uint32_t)sizeof(T);
  const rsrc_t krs = make_rsrc(k + kvb, kv_bytes);
  const rsrc_t vrs = make_rsrc(v + kvb, kv_bytes);
  constexpr bool CAP = FA_WIN_CAP;
  const float cap = FA_WIN_CAP_VALUE, k2 = CAP ? cap_k2(tau, cap) : 0.f;   // (CAP builds only)
  const float c = CAP ? LOG2E : tau * LOG2E;                                // CAP: the capped scores are the logits

  frag qf[KC];
#pragma unroll
  for (int kc = 0; kc < KC; ++kc)
    qf[kc] = load_frag_buf<T>(qrs, (qrow * ld + 16 * kc + 8 * h) * (int)sizeof(T));

  f32x16 acc_o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc_o[dt] = zero16();
  float m_ref = -INFINITY, nmc = 0.f, l_run = 0.f;   // raw score units (CAP: capped logits); nmc = -m_ref * c; m_ref = -inf: the row has no reference yet

  const LaneAddr ra = A::template row_addr<D>(lane);
  const LaneAddr ta = A::template tr_addr<D>(lane);
  WinWalk walk;
  walk.template init<BN>(qb * 128, min(N, qb * 128 + 128) - 1, W, S);
  const int nt = walk.nt;
  TileStager<T, D, BN, 256> sk, sv;
  sk.init(tid, ldk);
  sv.init(tid, ldk);
  sk.load(krs, walk.tile(0) * BN);
  sv.load(vrs, walk.tile(0) * BN);
  sk.store(smem);
  sv.store(smem + 2 * TB);
  __syncthreads();

  auto tile = [&](auto par, int t) {
    constexpr int PAR = decltype(par)::value;
    const int kbase = walk.tile(t) * BN;
    const bool more = t + 1 < nt;
    if (more) {
      const int knext = walk.tile(t + 1) * BN;
      sk.load(krs, knext);
      sv.load(vrs, knext);
    }
    lds_char* tk = smem + PAR * TB;
    lds_char* tv = smem + (2 + PAR) * TB;
    bool active = false;   // wave-uniform: some row of the wave admits a key of this tile
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) active = active || win_any(q0, kbase + 32 * kt, W, S);
    if (active && q0 < N) {
      f32x16 s[KT];
      auto scores = [&]() {   // S^T tile of this wave (raw units), masked
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) {
          s[kt] = zero16();
#pragma unroll
          for (int kc = 0; kc < KC; ++kc) A::mma(s[kt], A::template row_frag<D>(tk, ra, 32 * kt, kc), qf[kc]);
          if constexpr (CAP) {   // the cap, in front of the masks
#pragma unroll
            for (int i = 0; i < 16; ++i) s[kt][i] = cap_z(cap_rcp(s[kt][i], k2), cap);
          }
          if (win_straddles(q0, kbase + 32 * kt, W, S)) {   // wave-uniform
#pragma unroll
            for (int i = 0; i < 16; ++i)
              if (!win_admits(qrow, kbase + 32 * kt + acc_row(i, h), W, S)) s[kt][i] = -INFINITY;
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
        if (__any(!(rowsum < WIN_DEFER_SUM))) {   // rare: some row outgrew its reference
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
  int t = 0;
  for (; t + 1 < nt; t += 2) {
    tile(ic<0>{}, t);
    tile(ic<1>{}, t + 1);
  }
  if (t < nt) tile(ic<0>{}, t);

  const float l_tot = xhalf_sum(l_run);   // > 0 for every real row: it admits its own position
  if (qvalid) {
    constexpr bool LSINK = FA_WIN_LSINK;   // (lsink build: the head's logit joins the row where its 1 / l is formed)
    float inv_s = 0.f, lse_s = 0.f;
    if constexpr (LSINK) lsink_finish(m_ref, l_tot, tau, FA_WIN_LSINK_LOGIT, inv_s, lse_s);
    const float inv = LSINK ? inv_s : 1.0f / l_tot;
    float* orow = o + base + (size_t)qrow * ld;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 val = {acc_o[dt][4 * g] * inv, acc_o[dt][4 * g + 1] * inv, acc_o[dt][4 * g + 2] * inv, acc_o[dt][4 * g + 3] * inv};
        *reinterpret_cast<f32x4*>(orow + 32 * dt + 8 * g + 4 * h) = val;
      }
    if (h == 0) lse[FA_WIN_ROWCONST0 + qrow] = LSINK ? lse_s : (CAP ? m_ref : m_ref * tau) + __logf(l_tot);
  }
}

// ---------------------------------------------------------------------------------------------
// Backward dQ, query-stationary: NWQ waves x 32 query rows, K / V tiles of 32 keys, the forward's walk over them.
// nlc = -L / tau and ndelta = -rowsum(dO * O) come from bwd_prep_kernel (fa_bwd_dkdv.h).
// ---------------------------------------------------------------------------------------------
template <typename T, int D, int NWQ>
__global__ void __launch_bounds__(64 * NWQ)
FA_WIN_NAME(dq)(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, const T* __restrict__ dout,
                  const float* __restrict__ nlc, const float* __restrict__ ndelta, float* __restrict__ dq, FA_WIN_GEOM_PARAMS,
                  Layout lay, float tau, FA_WIN_MASK_PARAMS FA_WIN_CAP_PARAM) {
  using A = Atom<T>;
  typedef typename A::frag frag;
  constexpr int BN = 32, KC = D / 16, DT = D / 32, QB = 32 * NWQ;
  constexpr int TB = A::template tile_bytes<D>(BN);
  __shared__ __attribute__((aligned(16))) char smem_raw[4 * TB];
  lds_char* smem = (lds_char*)smem_raw;

  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int bh, qb;
  FA_WIN_LOCATE(qb, nblk)
  const int q0 = qb * QB + w * 32, qrow = q0 + r;
  const bool qvalid = qrow < N;
  const bool careful = A::SPLITS && (W + S < 64 || q0 < 64);   // wave-uniform: see win_fwd_kernel
  const int ld = lay.ld;
  const size_t base = head_base(lay, bh) + FA_WIN_ROW0 * ld;
  const uint32_t mat_bytes = ((uint32_t)(N - 1) * ld + D) * (uint32_t)sizeof(T);
  const rsrc_t qrs = make_rsrc(q + base, mat_bytes);
  const rsrc_t dors = make_rsrc(dout + base, mat_bytes);
  const int ldk = lay.ldk;
  const size_t kvb = kv_base<D>(lay, bh, N) + FA_WIN_ROW0 * ldk;
  const uint32_t kv_bytes = ((uint32_t)(N - 1) * ldk + D) * (uint32_t)sizeof(T);
  const rsrc_t krs = make_rsrc(k + kvb, kv_bytes);
  const rsrc_t vrs = make_rsrc(v + kvb, kv_bytes);
  constexpr bool CAP = FA_WIN_CAP;
  const float cap = FA_WIN_CAP_VALUE, k2 = CAP ? cap_k2(tau, cap) : 0.f;   // (CAP builds only)
  const float c = CAP ? LOG2E : tau * LOG2E;                                // CAP: the capped scores are the logits

  frag qf[KC], dof[KC];
#pragma unroll
  for (int kc = 0; kc < KC; ++kc) {
    const int off = (qrow * ld + 16 * kc + 8 * h) * (int)sizeof(T);
    qf[kc] = load_frag_buf<T>(qrs, off);
    dof[kc] = load_frag_buf<T>(dors, off);
  }
  // this lane's row constants; -delta, in every register, is the accumulator input of the dP^T tiles
  const float nlq = qvalid ? nlc[FA_WIN_ROWCONST0 + qrow] * c : 0.f;   // -L * log2(e) (CAP: nlc = -L)
  const float ndq = qvalid ? ndelta[FA_WIN_ROWCONST0 + qrow] : 0.f;
  f32x16 nd16;
#pragma unroll
  for (int i = 0; i < 16; ++i) nd16[i] = ndq;

  f32x16 acc[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc[dt] = zero16();

  const LaneAddr ra = A::template row_addr<D>(lane);
  const LaneAddr ta = A::template tr_addr<D>(lane);
  WinWalk walk;
  walk.template init<BN>(qb * QB, min(N, qb * QB + QB) - 1, W, S);
  const int nt = walk.nt;
  TileStager<T, D, BN, 64 * NWQ> sk, sv;
  sk.init(tid, ldk);
  sv.init(tid, ldk);
  sk.load(krs, walk.tile(0) * BN);
  sv.load(vrs, walk.tile(0) * BN);
  sk.store(smem);
  sv.store(smem + 2 * TB);
  __syncthreads();

  auto tile = [&](auto par, int t) {
    constexpr int PAR = decltype(par)::value;
    const int kbase = walk.tile(t) * BN;
    const bool more = t + 1 < nt;
    if (more) {
      const int knext = walk.tile(t + 1) * BN;
      sk.load(krs, knext);
      sv.load(vrs, knext);
    }
    lds_char* tk = smem + PAR * TB;
    lds_char* tv = smem + (2 + PAR) * TB;
    if (q0 < N && win_any(q0, kbase, W, S)) {   // wave-uniform
      f32x16 s, dp;
      A::mma_c(s, A::template row_frag<D>(tk, ra, 0, 0), qf[0], zero16());
      A::mma_c(dp, A::template row_frag<D>(tv, ra, 0, 0), dof[0], nd16);
#pragma unroll
      for (int kc = 1; kc < KC; ++kc) {
        A::mma(s, A::template row_frag<D>(tk, ra, 0, kc), qf[kc]);
        A::mma(dp, A::template row_frag<D>(tv, ra, 0, kc), dof[kc]);
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if constexpr (CAP) {   // s <- P * (1 - tanh^2): dQ needs dS alone
          const float rc = cap_rcp(s[i], k2);
          s[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(cap_z(rc, cap), c, nlq)) * cap_slope(rc);
        } else {
          s[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[i], c, nlq));
        }
      }
      if (win_straddles(q0, kbase, W, S)) {   // the diagonal, a window edge, S (keys past N lie above every real row's diagonal)
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (!win_admits(qrow, kbase + acc_row(i, h), W, S)) s[i] = 0.f;
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
  int t = 0;
  for (; t + 1 < nt; t += 2) {
    tile(ic<0>{}, t);
    tile(ic<1>{}, t + 1);
  }
  if (t < nt) tile(ic<0>{}, t);

  if (qvalid) {
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
// Backward dK / dV, key-stationary: a workgroup = NW waves = NW * 32 keys of one (batch*head); each wave keeps the K, V fragments
// and the dK^T, dV^T accumulators of its 32 keys while the workgroup sweeps QS-query slices (Q, dO and their row constants staged in
// LDS, double buffered, as bwd_dkdv_kernel).  Key j is admitted by the queries j .. j + W - 1, and by every later one when j < S:
// the sweep runs from the block's own diagonal to the last query that admits its last key, and on to N when the block holds a sink.
// Stores one dK and one dV per QUERY head (a grouped call points dk, dv at the workspace; group_sum_kernel adds the groups).
// ---------------------------------------------------------------------------------------------
template <typename T, int D, int NW, int QS>
__global__ void __launch_bounds__(NW * 64)
FA_WIN_NAME(dkdv)(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, const T* __restrict__ dout,
                    const float* __restrict__ nlc, const float* __restrict__ ndelta, float* __restrict__ dk, float* __restrict__ dv,
                    FA_WIN_GEOM_PARAMS, Layout lay, float tau, FA_WIN_MASK_PARAMS FA_WIN_CAP_PARAM) {
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
  // (FA_WIN_LOCATE_KEYS of the window library:) With sinks, key block 0 of every head sweeps all N queries where the others sweep about BK + W: those blocks are dispatched first,
  // across all heads of an XCD, so the long sweeps run beside the short ones instead of behind them (measured, profiles/
  // window_train_bench.txt: dispatched head by head they were a tail of 0.8 ms on 2.5 at N = 8192, W = 1024, S = 4).
  FA_WIN_LOCATE_KEYS(kb, nblk)
  const int kb0 = kb * BK, kw0 = kb0 + w * 32, key = kw0 + r;
  const int ld = lay.ld;
  const size_t base = head_base(lay, bh) + FA_WIN_ROW0 * ld;
  const uint32_t mat_bytes = ((uint32_t)(N - 1) * ld + D) * (uint32_t)sizeof(T);
  const rsrc_t qrs = make_rsrc(q + base, mat_bytes);
  const rsrc_t dors = make_rsrc(dout + base, mat_bytes);
  const int ldk = lay.ldk;
  const size_t kvb = kv_base<D>(lay, bh, N) + FA_WIN_ROW0 * ldk;
  const uint32_t kv_bytes = ((uint32_t)(N - 1) * ldk + D) * (uint32_t)sizeof(T);
  const rsrc_t krs = make_rsrc(k + kvb, kv_bytes);
  const rsrc_t vrs = make_rsrc(v + kvb, kv_bytes);
  const float* nlg = nlc + FA_WIN_ROWCONST0;
  const float* deg = ndelta + FA_WIN_ROWCONST0;
  constexpr bool CAP = FA_WIN_CAP;
  const float cap = FA_WIN_CAP_VALUE, k2 = CAP ? cap_k2(tau, cap) : 0.f;   // (CAP builds only)
  const float c = CAP ? LOG2E : tau * LOG2E;                                // CAP: the capped scores are the logits

  frag kf[KC], vf[KC];
#pragma unroll
  for (int kc = 0; kc < KC; ++kc) {
    const int off = (key * ldk + 16 * kc + 8 * h) * (int)sizeof(T);   // rows >= N read as zero
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
  // the sweep: slices qi_begin .. nqi - 1
  const int q_last = kb0 < S ? N - 1 : min(N - 1, min(kb0 + BK, N) - 1 + W - 1);
  const int qi_begin = kb0 / QS, nqi = q_last / QS + 1;
  // Stage copies of Q and dO, as bwd_dkdv_kernel: LDS-DMA for bf16 at d >= 64, registers otherwise
  constexpr bool DMA = sizeof(T) == 2 && D >= 64;
  constexpr int PPG = D >= 128 ? 2 : 1;
  TileStager<T, D, QS, NT> sq, sdo;
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
        const int soff = (qi * QS + 8 * g) * ld * (int)sizeof(T);
        dma16(qraw, smem_addr + dst + 1024 * piece, dma_voff, soff);
        dma16(doraw, smem_addr + dst + TB + 1024 * piece, dma_voff, soff);
      }
    } else {
      sq.load(qrs, qi * QS);
      sdo.load(dors, qi * QS);
    }
    if (tid < QS) {
      const int row = qi * QS + tid;
      st_nl = row < N ? nlg[row] : 0.f;
      st_de = row < N ? deg[row] : 0.f;
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
  stage_load(qi_begin, 0);
  stage_store(smem);
  __syncthreads();

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
      if (kw0 < N && qi0 < N && win_any(qi0, kw0, W, S)) {   // wave-uniform
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
        // (CAP: the raw score is capped before L is subtracted: that accumulator starts at zero and nlc = -L comes in behind the cap)
        f32x16 s, dp;
        A::mma_c(s, A::template row_frag<D>(tq, ra, 32 * sub, 0), kf[0], CAP ? zero16() : nl16);
        A::mma_c(dp, A::template row_frag<D>(tdo, ra, 32 * sub, 0), vf[0], nd16);
#pragma unroll
        for (int kc = 1; kc < KC; ++kc) {
          A::mma(s, A::template row_frag<D>(tq, ra, 32 * sub, kc), kf[kc]);
          A::mma(dp, A::template row_frag<D>(tdo, ra, 32 * sub, kc), vf[kc]);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          if constexpr (CAP) {   // s <- P of the capped score (dV); dp <- dP' * (1 - tanh^2), so that dS = P * dp below
            const float rc = cap_rcp(s[i], k2);
            s[i] = __builtin_amdgcn_exp2f((cap_z(rc, cap) + nl16[i]) * c);
            dp[i] *= cap_slope(rc);
          } else {
            s[i] = __builtin_amdgcn_exp2f(s[i] * c);
          }
        }
        if (win_straddles(qi0, kw0, W, S)) {   // the unmasked path is taken only where every (query, key) pair is admitted
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (!win_admits(qi0 + acc_row(i, h), key, W, S)) s[i] = 0.f;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) dp[i] = s[i] * dp[i];
        frag pf[2], dsf[2];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          pf[s2] = A::pack(s, s2);
          dsf[s2] = A::pack(dp, s2);
        }
        // (the wave's keys hold a sink, kw0 < S: such a key collects P and dS of ALL later queries, G * N terms of order 1 / (W + S)
        // whose bf16 rounding adds up with sqrt(G * N), where a windowed key stops at G * W terms: the split operands there too)
        if (!(A::SPLITS && (W + S < 64 || qi0 < 64 || kw0 < S))) {
#pragma unroll
          for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
              A::mma(acc_dv[dt], A::template tr_frag<D>(tdo, ta, 32 * sub + 16 * s2, dt), pf[s2]);
              A::mma(acc_dk[dt], A::template tr_frag<D>(tq, ta, 32 * sub + 16 * s2, dt), dsf[s2]);
            }
        } else {   // queries with few admissible keys: both products also take what the bf16 rounding of P, dS dropped
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

  if (key < N) {
    float* dkrow = dk + base + (size_t)key * ld;
    float* dvrow = dv + base + (size_t)key * ld;
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
