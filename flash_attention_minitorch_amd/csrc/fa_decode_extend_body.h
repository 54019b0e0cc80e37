// The body of extend_split_kernel and its _sink, _softcap and _lsink kernels (fa_decode.h), included INSIDE each: plain text, not a
// function.  A function template that both kernels call is inlined only after it has been simplified on its own, and every existing
// build of the kernel then comes out with other code than it had (compared per kernel: profiles/sink_isa_identity.txt); as text the
// existing kernel is the function it was.  In scope: T, D, PAGED, RAGGED, WINDOW, FP8, SINK, SOFTCAP, LSINK and the kernel's argument a.
  static_assert(!FP8 || (std::is_same<T, bf16_t>::value && !RAGGED && !WINDOW), "fp8 caches: bf16 queries, no ragged form, no window");
  static_assert(!SINK || (WINDOW && !FP8), "sinks: beside a window, no fp8 cache");
  static_assert(!SOFTCAP || (!FP8 && !SINK), "soft-capping: no fp8 cache, no sinks");
  static_assert(!LSINK || (!FP8 && !SINK && !SOFTCAP), "learned sink logits: no fp8 cache, no sink tokens, no cap");
  using A = Atom<T>;
  typedef typename std::conditional<FP8, uint8_t, T>::type C;
  typedef typename A::frag frag;
  constexpr int KC = D / 16, DT = D / 32;
  constexpr int TB = A::template tile_bytes<D>(DEC_ROWS);
  __shared__ __attribute__((aligned(16))) char smem_raw[2 * TB];
  lds_char* tk = (lds_char*)smem_raw;
  lds_char* tv = tk + TB;

  // workgroup -> (item, row block) as in decode_split_kernel: the row blocks of one item share an XCD's L2
  const int id = blockIdx.x, slot = id >> 3;
  const int entry = slot % a.nqb, item = (slot / a.nqb) * 8 + (id & 7);
  if (item >= a.items) return;
  const int bh = item / a.nsplit, split = item - bh * a.nsplit;
  int b_ = bh / a.Hkv, hkv_ = bh - b_ * a.Hkv, qb_ = entry, row0_ = 0, nq_ = 0;
  if constexpr (RAGGED) {
    b_ = __builtin_amdgcn_readfirstlane(a.map[2 * entry]);
    if (b_ < 0) return;   // (an unused entry: the map is sized for the worst case)
    qb_ = __builtin_amdgcn_readfirstlane(a.map[2 * entry + 1]);
    hkv_ = bh;
    seq_rows(a.cu, a.ntok, b_, row0_, nq_);
    row0_ = __builtin_amdgcn_readfirstlane(row0_);
    nq_ = __builtin_amdgcn_readfirstlane(nq_);
  }
  const int b = b_, hkv = hkv_, qb = qb_, row0 = row0_;
  // The sequence's own count, or the call's.  A macro, not a local `const int Nq`: a local reads a.Nq once at the top of the uniform
  // build, which moved two of its fp32 builds from 58 to 59 SGPRs; with a.Nq read where it always was, the uniform builds compile to
  // the code they were (DESIGN.md "Ragged").  Do not fold it into a variable without comparing the resource report.
#define FA_NQ (RAGGED ? nq_ : a.Nq)
  const int len = __builtin_amdgcn_readfirstlane(clamp_len(a, b));
  int wedge = 0;   // (window builds) the block's window edge; the key range starts at the super tile that holds it
  if constexpr (WINDOW) wedge = max(len - FA_NQ + row_query(a, qb * EXT_BLOCK) - a.window + 1, 0);
  int S = 0, lo = 0, vs = 0, sc0 = 0, sc1 = 0;   // (sink builds) as in fa_decode_split_body.h
  if constexpr (SINK) {
    S = a.sink;
    lo = wedge & ~(DEC_ROWS - 1);
    vs = min((S + DEC_ROWS - 1) & ~(DEC_ROWS - 1), lo);
    sink_chunk(split, a.chunk, len, vs, lo, sc0, sc1);
  }
  const int c0 = SINK ? sc0 : (WINDOW ? wedge & ~(DEC_ROWS - 1) : 0) + split * a.chunk, c1 = SINK ? sc1 : min(c0 + a.chunk, len);

  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rows = a.G * FA_NQ;
  const int q0 = qb * EXT_BLOCK + 32 * w, rho = q0 + r, qi = row_query(a, rho), hd = hkv * a.G + (rho - qi * a.G);
  const bool live = rho < rows;
  const bool wave_live = q0 < rows;   // (wave-uniform)
  float tau8 = 0.f;
  if constexpr (FP8) tau8 = a.tau * scale_of(a.k_scale, hkv);
  // (softcap builds: the capped scores ARE the logits, so the softmax's tau is 1; k2 is cap_score's exp2 constant)
  float k2 = 0.f;
  if constexpr (SOFTCAP) k2 = cap_k2(a.tau, a.softcap);
#define FA_TAU (SOFTCAP ? 1.0f : FP8 ? tau8 : a.tau)
  const float c = FA_TAU * LOG2E;
  // causal: the last key any row of the block sees is the position of its last row (of its last REAL row: rows >= G * Nq see nothing)
  // (sink builds: blk_hi >= lo or the block has no sink tiles, so cend is never inside (vs, lo] either)
  const int blk_hi = len - FA_NQ + row_query(a, min(qb * EXT_BLOCK + EXT_BLOCK, rows) - 1);
  const int cend = a.causal ? min(c1, blk_hi + 1) : c1;

  f32x16 acc_o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc_o[dt] = zero16();
  float m_run = -INFINITY, l_run = 0.f;

  if (c0 < cend) {   // (a chunk past len_b, or past every position of the block, loads nothing and leaves m = -inf, l = 0)
    const size_t kvoff = (PAGED ? 0 : (size_t)b * a.kv_bstride) + (size_t)hkv * a.kv_hstride;   // (paged: inside a page)
    const uint32_t esz = sizeof(T);
    // (ragged: the resource of the sequence's own nq_b * H * D elements of the packed q)
    const uint32_t q_bytes = RAGGED ? (uint32_t)nq_ * (uint32_t)a.q_ld * esz : (uint32_t)a.q_bstride * esz;
    const rsrc_t qrs = make_rsrc(reinterpret_cast<const T*>(a.q) + (RAGGED ? (size_t)row0 * a.q_ld : (size_t)b * a.q_bstride), q_bytes);
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
    // the wave's rows span the positions pos_lo .. pos_hi (wave-uniform; rows past G * Nq may push pos_hi up, which only keeps a
    // sub-tile that masks to nothing for the real rows' lanes)
    const int qpos = len - FA_NQ + qi;
    const int pos_lo = len - FA_NQ + row_query(a, q0), pos_hi = len - FA_NQ + row_query(a, q0 + 31);
    if constexpr (PAGED) {
      pw.init(a, b, c0);
      if constexpr (SINK)
        sink_load<C, D>(pw, a, b, sk, sv, kvoff, len, c0, vs, lo, cend);
      else
        pw.template load<C, D>(a, sk, sv, kvoff, len, c0 + DEC_ROWS < cend);
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
    for (int t0 = c0; t0 < cend; t0 = SINK ? sink_next(t0, vs, lo) : t0 + DEC_ROWS) {
      __syncthreads();   // (the previous super tile's reads are done)
      if constexpr (SINK) {
        if (t0 < wedge && t0 + DEC_ROWS > S) {   // the staged rows S <= j < wedge, as in fa_decode_split_body.h
          zero_rows(sk, S - t0, wedge - t0);
          zero_rows(sv, S - t0, wedge - t0);
        }
      }
      sk.store(tk);
      sv.store(tv);
      const int t1 = SINK ? sink_next(t0, vs, lo) : t0 + DEC_ROWS;   // the tile behind this one
      if (t1 < cend) {
        if constexpr (PAGED) {
          if constexpr (SINK)
            sink_load<C, D>(pw, a, b, sk, sv, kvoff, len, t1, vs, lo, cend);
          else
            pw.template load<C, D>(a, sk, sv, kvoff, len, t0 + 2 * DEC_ROWS < cend);
        } else {
          load_rows(sk, krs, t1);
          load_rows(sv, vrs, t1);
        }
      }
      __syncthreads();
      if (!wave_live) continue;
#pragma unroll
      for (int st = 0; st < DEC_ROWS / 32; ++st) {
        const int kbase = t0 + 32 * st;
        if (kbase >= cend || (a.causal && kbase > pos_hi)) break;   // wave-uniform: no admissible key here or further on
        if constexpr (WINDOW) {
          // wave-uniform: the 32 keys are below every window of the wave's rows (sink builds: and none of them is a sink)
          if (kbase + 31 <= pos_lo - a.window && (!SINK || kbase >= S)) continue;
        }
        f32x16 s = zero16();
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) A::mma(s, A::template row_frag<D>(tk, ra, 32 * st, kc), qf[kc]);
        if constexpr (SOFTCAP) {   // the cap, in front of the masks: a masked score must stay -inf, not become -softcap
#pragma unroll
          for (int i = 0; i < 16; ++i) s[i] = cap_score(s[i], k2, a.softcap);
        }
        // (window: only the sub-tiles that hold a key at or below the wave's highest edge - 1 mask for it; sink builds: and a key >= S)
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
        // bf16: P at 16 significant bits (pack + pack_lo), as in decode_split_kernel
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const frag p_hi = A::pack(s, s2);
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            const frag vt = A::template tr_frag<D>(tv, ta, 32 * st + 16 * s2, dt);
            A::mma(acc_o[dt], vt, p_hi);
            if constexpr (A::SPLITS) A::mma(acc_o[dt], vt, A::pack_lo(s, s2, p_hi));
          }
        }
      }
    }
  }
  const float l_tot = xhalf_sum(l_run);
  if (!live) return;   // (no barrier follows)
  // (ragged: out, lse and the partials by packed row row0 + qi, as one batch element of a.Nq = ntok queries)
  const size_t bhq = RAGGED ? (size_t)hd : (size_t)b * a.H + hd;
  if (a.nsplit == 1) {   // final: out = O / l, lse = m * tau + ln l; a row without an admissible key: out = 0, lse = -inf
    float inv = (l_tot > 0.f) ? 1.0f / l_tot : 0.f;
    if constexpr (FP8) inv *= scale_of(a.v_scale, hkv);   // (the scale of V: once per row, on 1 / l)
    float lse_s = 0.f;   // (lsink builds: the head's logit joins the row as one more column; a row without a key: out = 0, lse = a)
    if constexpr (LSINK) lsink_finish(m_run, l_tot, FA_TAU, a.sink_logits[hd], inv, lse_s);
    float* orow = a.out + (RAGGED ? 0 : (size_t)b * a.q_bstride) + (size_t)hd * a.q_hstride + (size_t)(RAGGED ? row0 + qi : qi) * a.q_ld;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 val = {acc_o[dt][4 * g] * inv, acc_o[dt][4 * g + 1] * inv, acc_o[dt][4 * g + 2] * inv, acc_o[dt][4 * g + 3] * inv};
        *reinterpret_cast<f32x4*>(orow + 32 * dt + 8 * g + 4 * h) = val;
      }
    if constexpr (LSINK) {
      if (h == 0 && a.lse) a.lse[bhq * a.Nq + (RAGGED ? row0 + qi : qi)] = lse_s;
    } else {
      if (h == 0 && a.lse) a.lse[bhq * a.Nq + (RAGGED ? row0 + qi : qi)] = (l_tot > 0.f) ? m_run * FA_TAU + __logf(l_tot) : -INFINITY;
    }
  } else {
    const size_t pr = (bhq * a.nsplit + split) * a.Nq + (RAGGED ? row0 + qi : qi);
    float* prow = a.part_o + pr * D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 val = {acc_o[dt][4 * g], acc_o[dt][4 * g + 1], acc_o[dt][4 * g + 2], acc_o[dt][4 * g + 3]};
        *reinterpret_cast<f32x4*>(prow + 32 * dt + 8 * g + 4 * h) = val;
      }
    if (h == 0) *reinterpret_cast<f32x2*>(a.part_ml + 2 * pr) = f32x2{m_run, l_tot};
  }
#undef FA_NQ
#undef FA_TAU
