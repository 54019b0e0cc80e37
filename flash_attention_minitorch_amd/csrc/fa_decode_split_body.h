// The body of decode_split_kernel and its _sink, _softcap and _lsink kernels (fa_decode.h), included INSIDE each: plain text, not a
// function.  A function template that both kernels call is inlined only after it has been simplified on its own, and every existing
// build of the kernel then comes out with other code than it had (compared per kernel: profiles/sink_isa_identity.txt); as text the
// existing kernel is the function it was.  In scope: T, D, GROUPED, PAGED, WINDOW, FP8, SINK, SOFTCAP, LSINK and the kernel's argument a.
  static_assert(!FP8 || (std::is_same<T, bf16_t>::value && GROUPED && !WINDOW), "fp8 caches: bf16 queries, the grouped form, no window");
  static_assert(!SINK || (WINDOW && GROUPED && !FP8), "sinks: beside a window, the grouped form, no fp8 cache");
  static_assert(!SOFTCAP || (GROUPED && !FP8 && !SINK), "soft-capping: the grouped form, no fp8 cache, no sinks");
  static_assert(!LSINK || (GROUPED && !FP8 && !SINK && !SOFTCAP), "learned sink logits: the grouped form, no fp8 cache, no sink tokens, no cap");
  using A = Atom<T>;
  typedef typename std::conditional<FP8, uint8_t, T>::type C;
  typedef typename A::frag frag;
  constexpr int KC = D / 16, DT = D / 32;
  constexpr int TB = A::template tile_bytes<D>(DEC_ROWS);
  constexpr int PW = (16 * DT + 2) * 64 * 4;   // one wave's partial: [lane][16*DT accumulator registers, m, l]
  static_assert(3 * PW <= 2 * TB, "the partials of waves 1-3 must fit the tile images");
  __shared__ __attribute__((aligned(16))) char smem_raw[2 * TB];
  lds_char* tk = (lds_char*)smem_raw;
  lds_char* tv = tk + TB;

  // workgroup -> (item = (b * Hkv + kv head) * nsplit + split, row block): the row blocks of one item are 8 workgroup ids apart, so
  // they share an XCD's L2 under round-robin dispatch and the chunk is fetched from HBM once (speed only)
  const int id = blockIdx.x, slot = id >> 3;
  const int qb = slot % a.nqb, item = (slot / a.nqb) * 8 + (id & 7);
  if (item >= a.items) return;
  const int bh = item / a.nsplit, split = item - bh * a.nsplit;
  const int b = bh / a.Hkv, hkv = bh - b * a.Hkv;
  const int len = __builtin_amdgcn_readfirstlane(clamp_len(a, b));
  int wedge = 0;   // (window builds) the block's window edge; the key range starts at the super tile that holds it
  if constexpr (WINDOW) wedge = max(len - a.Nq + (GROUPED ? row_query(a, qb * 32) : qb * 32) - a.window + 1, 0);
  // (sink builds) S; lo, the start of the window's range; vs, the end of the sink tiles below it; the split's bounds on that walk
  int S = 0, lo = 0, vs = 0, sc0 = 0, sc1 = 0;
  if constexpr (SINK) {
    S = a.sink;
    lo = wedge & ~(DEC_ROWS - 1);
    vs = min((S + DEC_ROWS - 1) & ~(DEC_ROWS - 1), lo);
    sink_chunk(split, a.chunk, len, vs, lo, sc0, sc1);
  }
  const int c0 = SINK ? sc0 : (WINDOW ? wedge & ~(DEC_ROWS - 1) : 0) + split * a.chunk, c1 = SINK ? sc1 : min(c0 + a.chunk, len);

  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the lane's row rho = qi * G + g: query qi of head hd = hkv * G + g
  const int G = GROUPED ? a.G : 1;
  const int q0 = qb * 32, rho = q0 + r, qi = GROUPED ? row_query(a, rho) : rho, hd = hkv * G + (rho - qi * G);
  const bool live = rho < G * a.Nq;
  // (a macro, as FA_NQ below: the other builds read a.tau where they always did)
  float tau8 = 0.f;
  if constexpr (FP8) tau8 = a.tau * scale_of(a.k_scale, hkv);
  // (softcap builds: the capped scores ARE the logits, so the softmax's tau is 1; k2 is cap_score's exp2 constant)
  float k2 = 0.f;
  if constexpr (SOFTCAP) k2 = cap_k2(a.tau, a.softcap);
#define FA_TAU (SOFTCAP ? 1.0f : FP8 ? tau8 : a.tau)
  const float c = FA_TAU * LOG2E;

  f32x16 acc_o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc_o[dt] = zero16();
  float m_run = -INFINITY, l_run = 0.f;

  if (c0 < c1) {   // (a chunk wholly past len_b loads nothing and leaves the empty partial m = -inf, l = 0)
    const size_t kvoff = (PAGED ? 0 : (size_t)b * a.kv_bstride) + (size_t)hkv * a.kv_hstride;   // (paged: inside a page)
    const uint32_t esz = sizeof(T);
    const uint32_t q_bytes = (uint32_t)a.q_bstride * esz;
    const rsrc_t qrs = make_rsrc(reinterpret_cast<const T*>(a.q) + (size_t)b * a.q_bstride, q_bytes);
    const uint32_t kv_bytes = ((uint32_t)(len - 1) * a.kv_ld + D) * (uint32_t)sizeof(C);
    const rsrc_t krs = make_rsrc(reinterpret_cast<const C*>(a.k) + kvoff, kv_bytes);   // (the slab's: unused by a paged build)
    const rsrc_t vrs = make_rsrc(reinterpret_cast<const C*>(a.v) + kvoff, kv_bytes);
    PageWalk pw;

    frag qf[KC];
    const int qoff = live ? (hd * (int)a.q_hstride + qi * a.q_ld + 8 * h) * (int)esz : (int)q_bytes;
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) qf[kc] = load_frag_buf<T>(qrs, qoff + 16 * kc * (int)esz);

    const LaneAddr ra = A::template row_addr<D>(lane);
    const LaneAddr ta = A::template tr_addr<D>(lane);
    typename std::conditional<FP8, Fp8Stager<D>, TileStager<T, D, DEC_ROWS, 256>>::type sk, sv;
    sk.init(tid, a.kv_ld);
    sv.init(tid, a.kv_ld);
    // causal: query i sits at position len - Nq + i and sees keys j <= len - Nq + i (bottom-right aligned); the block's rows span
    // the positions pos_lo .. pos_hi (wave-uniform; pos_hi may count rows past G * Nq, which only keeps a tile that masks to nothing)
    const int qpos = len - a.Nq + qi;
    const int pos_lo = len - a.Nq + (GROUPED ? row_query(a, q0) : q0), pos_hi = len - a.Nq + (GROUPED ? row_query(a, q0 + 31) : q0 + 31);
    if constexpr (PAGED) {
      pw.init(a, b, c0);
      if constexpr (SINK)
        sink_load<C, D>(pw, a, b, sk, sv, kvoff, len, c0, vs, lo, c1);
      else
        pw.template load<C, D>(a, sk, sv, kvoff, len, c0 + DEC_ROWS < c1);
    } else {
      load_rows(sk, krs, c0);
      load_rows(sv, vrs, c0);
    }
    if constexpr (WINDOW && !SINK) {
      if (c0 < wedge) {   // (split 0 of a block whose edge is inside a super tile)
        zero_below(sk, wedge - c0);
        zero_below(sv, wedge - c0);
      }
    }
    for (int t0 = c0; t0 < c1; t0 = SINK ? sink_next(t0, vs, lo) : t0 + DEC_ROWS) {
      __syncthreads();   // (the previous super tile's reads are done)
      if constexpr (SINK) {
        // the staged rows S <= j < wedge, which no row of the block admits: the tail of the last sink tile, the head of the first
        // tile of the window's range (the keys below S in that one stay)
        if (t0 < wedge && t0 + DEC_ROWS > S) {
          zero_rows(sk, S - t0, wedge - t0);
          zero_rows(sv, S - t0, wedge - t0);
        }
      }
      sk.store(tk);
      sv.store(tv);
      const int t1 = SINK ? sink_next(t0, vs, lo) : t0 + DEC_ROWS;   // the tile behind this one
      if (t1 < c1) {
        if constexpr (PAGED) {
          if constexpr (SINK)
            sink_load<C, D>(pw, a, b, sk, sv, kvoff, len, t1, vs, lo, c1);
          else
            pw.template load<C, D>(a, sk, sv, kvoff, len, t0 + 2 * DEC_ROWS < c1);
        } else {
          load_rows(sk, krs, t1);
          load_rows(sv, vrs, t1);
        }
      }
      __syncthreads();
      const int kbase = t0 + 32 * w;
      if (kbase >= c1 || (a.causal && kbase > pos_hi)) continue;   // wave-uniform: no admissible key in the wave's 32
      if constexpr (WINDOW) {
        // wave-uniform: the 32 keys are below every row's window (sink builds: and none of them is a sink)
        if (kbase + 31 <= pos_lo - a.window && (!SINK || kbase >= S)) continue;
      }
      f32x16 s = zero16();
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) A::mma(s, A::template row_frag<D>(tk, ra, 32 * w, kc), qf[kc]);
      if constexpr (SOFTCAP) {   // the cap, in front of the masks: a masked score must stay -inf, not become -softcap
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = cap_score(s[i], k2, a.softcap);
      }
      // (window: only the sub-tiles that hold a key at or below the highest row's edge - 1 mask for it; sink builds: and a key >= S)
      if (kbase + 32 > c1 || (a.causal && kbase + 31 > pos_lo) ||
          (WINDOW && kbase <= pos_hi - a.window && (!SINK || kbase + 31 >= S))) {   // wave-uniform
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int key = kbase + acc_row(i, h);
          if (key >= c1 || (a.causal && key > qpos) || (WINDOW && key <= qpos - a.window && (!SINK || key >= S))) s[i] = -INFINITY;
        }
      }
      float mx = s[0];
#pragma unroll
      for (int i = 1; i < 16; ++i) mx = fmaxf(mx, s[i]);
      const float m_new = fmaxf(m_run, xhalf_max(mx));
      const float nm = (m_new == -INFINITY) ? 0.f : -m_new * c;   // (every key so far masked: any finite reference, P = 0)
      const float alpha = __builtin_amdgcn_exp2f(__builtin_fmaf(m_run, c, nm));
      float rs = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        s[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[i], c, nm));
        rs += s[i];
      }
      if (__any(alpha != 1.0f)) {
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
          for (int i = 0; i < 16; ++i) acc_o[dt][i] *= alpha;
      }
      l_run = l_run * alpha + rs;
      m_run = m_new;
      // bf16: P goes in at 16 significant bits (pack + pack_lo): a row with few admissible keys holds P of order 1, whose 2^-9
      // rounding would not average out (the decode step's first tokens, causal rows near position 0)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const frag p_hi = A::pack(s, s2);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const frag vt = A::template tr_frag<D>(tv, ta, 32 * w + 16 * s2, dt);
          A::mma(acc_o[dt], vt, p_hi);
          if constexpr (A::SPLITS) A::mma(acc_o[dt], vt, A::pack_lo(s, s2, p_hi));
        }
      }
    }
  }
  const float l_w = xhalf_sum(l_run);

  // the partials of waves 1-3 meet in LDS (over the tile images), wave 0 adds them in wave order
  __syncthreads();
  if (w != 0) {
    lds_char* mine = tk + (w - 1) * PW + lane * (16 * DT + 2) * 4;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int i = 0; i < 16; ++i) *FA_LDS(float, mine + (16 * dt + i) * 4) = acc_o[dt][i];
    *FA_LDS(float, mine + 16 * DT * 4) = m_run;
    *FA_LDS(float, mine + (16 * DT + 1) * 4) = l_w;
  }
  __syncthreads();
  if (w != 0) return;
  float m_all = m_run;
#pragma unroll
  for (int u = 0; u < 3; ++u) m_all = fmaxf(m_all, *FA_LDS(float, tk + u * PW + (lane * (16 * DT + 2) + 16 * DT) * 4));
  float wgt = (m_run == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f((m_run - m_all) * c);
  float l_tot = l_w * wgt;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc_o[dt][i] *= wgt;
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    lds_char* pu = tk + u * PW + lane * (16 * DT + 2) * 4;
    const float mu = *FA_LDS(float, pu + 16 * DT * 4);
    wgt = (mu == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f((mu - m_all) * c);
    l_tot += *FA_LDS(float, pu + (16 * DT + 1) * 4) * wgt;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc_o[dt][i] += *FA_LDS(float, pu + (16 * dt + i) * 4) * wgt;
  }
  if (!live) return;
  const size_t bhq = (size_t)b * a.H + hd;
  if (a.nsplit == 1) {   // final: out = O / l, lse = m * tau + ln l; a row without an admissible key: out = 0, lse = -inf
    float inv = (l_tot > 0.f) ? 1.0f / l_tot : 0.f;
    if constexpr (FP8) inv *= scale_of(a.v_scale, hkv);   // (the scale of V: once per row, on 1 / l)
    float lse_s = 0.f;   // (lsink builds: the head's logit joins the row as one more column; a row without a key: out = 0, lse = a)
    if constexpr (LSINK) lsink_finish(m_all, l_tot, FA_TAU, a.sink_logits[hd], inv, lse_s);
    float* orow = a.out + (size_t)b * a.q_bstride + (size_t)hd * a.q_hstride + (size_t)qi * a.q_ld;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 val = {acc_o[dt][4 * g] * inv, acc_o[dt][4 * g + 1] * inv, acc_o[dt][4 * g + 2] * inv, acc_o[dt][4 * g + 3] * inv};
        *reinterpret_cast<f32x4*>(orow + 32 * dt + 8 * g + 4 * h) = val;
      }
    if constexpr (LSINK) {
      if (h == 0 && a.lse) a.lse[bhq * a.Nq + qi] = lse_s;
    } else {
      if (h == 0 && a.lse) a.lse[bhq * a.Nq + qi] = (l_tot > 0.f) ? m_all * FA_TAU + __logf(l_tot) : -INFINITY;
    }
  } else {
    const size_t pr = (bhq * a.nsplit + split) * a.Nq + qi;
    float* prow = a.part_o + pr * D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 val = {acc_o[dt][4 * g], acc_o[dt][4 * g + 1], acc_o[dt][4 * g + 2], acc_o[dt][4 * g + 3]};
        *reinterpret_cast<f32x4*>(prow + 32 * dt + 8 * g + 4 * h) = val;
      }
    if (h == 0) *reinterpret_cast<f32x2*>(a.part_ml + 2 * pr) = f32x2{m_all, l_tot};
  }
#undef FA_TAU
