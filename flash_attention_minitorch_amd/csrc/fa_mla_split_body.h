// The body of mla_decode_split_kernel<PAGED> (fa_mla.h) and of mla_fp8_split_kernel<PAGED> (fa_mla_fp8.h), included as TEXT inside
// both for the reason fa_decode_split_body.h gives: as text the bf16 kernel is the function it was, under the name it had.  In
// scope: PAGED, FP8 and the argument a.  FP8 picks the stager that fills the tile image (MlaFp8Stager widens e4m3 codes to bf16 in
// front of LDS) and the bytes of a cache row; the argument's cache strides count 2-byte units in both (a 656-byte row is 328 of
// them).  Everything behind the image -- the fragments, the MFMAs, the softmax, the partials -- is one text.
  using T = bf16_t;
  using Stager = typename std::conditional<FP8, MlaFp8Stager, MlaStager>::type;
  constexpr int ROWB = FP8 ? MLA_FP8_ROW_BYTES : MLA_ROW_BYTES;
  using A = Atom<T>;
  typedef A::frag frag;
  constexpr int D = MLA_DQK, KC = D / 16, DT = MLA_DV / 32 / 4;   // KC: k-chunks of a score; DT: 32-column output tiles of a wave
  constexpr int TB = A::tile_bytes<D>(MLA_TILE);                  // 72 KB: the tile image
  constexpr int PB = 2 * 2 * 2 * 2 * 64 * 16;                     // 16 KB: P as [row half][key half][k-step][hi, lo][lane] fragments
  constexpr int RC = 768;                                         // row constants: [rh][kh][32] maxima (then sums), [64] alpha (then m)
  static_assert(TB + PB + RC <= 160 * 1024, "the tile image, P and the row constants must fit the CU's LDS");
  __shared__ __attribute__((aligned(16))) char smem_raw[TB + PB + RC];
  lds_char* tile = (lds_char*)smem_raw;
  lds_char* pbuf = tile + TB;
  lds_char* rc_x = pbuf + PB;    // [rh][kh][32] floats: a tile's maxima in the loop, the key halves' row sums behind it
  lds_char* rc_a = rc_x + 512;   // [64] floats: alpha in the loop, m behind it

  // workgroup -> (item, row block) as in decode_split_kernel
  const int id = blockIdx.x, slot = id >> 3;
  const int qb = slot % a.nqb, item = (slot / a.nqb) * 8 + (id & 7);
  if (item >= a.items) return;
  const int b = item / a.nsplit, split = item - b * a.nsplit;
  const int len = __builtin_amdgcn_readfirstlane(clamp_len(a, b));
  const int c0 = split * a.chunk, c1 = min(c0 + a.chunk, len);

  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6), kh = w & 1, rh = w >> 1;
  const int rows = a.G * a.Nq, q0 = qb * MLA_BLOCK;
  const bool half_live[2] = {true, q0 + 32 < rows};   // (wave-uniform; the first half of a block always has a live row)
  const float c = a.tau * LOG2E;

  f32x16 acc_o[2][DT];   // [row half][column tile]: O^T, the query row on the lane
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc_o[x][dt] = zero16();
  float m_run = -INFINITY, l_run = 0.f;

  if (c0 < c1) {   // (a chunk wholly past len_b loads nothing and leaves the empty partial m = -inf, l = 0; workgroup-uniform)
    const int rho = q0 + 32 * rh + r, qi = row_query(a, rho), hd = rho - qi * a.G;
    const uint32_t q_bytes = (uint32_t)a.q_bstride * 2;
    const rsrc_t qrs = make_rsrc(reinterpret_cast<const T*>(a.q) + (size_t)b * a.q_bstride, q_bytes);
    // (the slab's resource: ends at len_b; unused by a paged build)
    const rsrc_t krs = make_rsrc(reinterpret_cast<const T*>(a.k) + (PAGED ? 0 : (size_t)b * a.kv_bstride), (uint32_t)len * ROWB);
    PageWalk pw;   // (paged) stands on the page of the tile that is loaded next; stepped by 64-key tiles here

    // Q: the lane's row at the columns 16 kc + 8 h; rows >= H * Nq get the resource's size as their offset and read as zero
    frag qf[KC];
    const int qoff = rho < rows ? (hd * (int)a.q_hstride + qi * a.q_ld + 8 * h) * 2 : (int)q_bytes;
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) qf[kc] = load_frag_buf<T>(qrs, qoff + 32 * kc);

    const LaneAddr ra = A::row_addr<D>(lane);
    const LaneAddr ta = A::tr_addr<D>(lane);
    lds_char* tcol = tile + 512 * DT * w;   // the wave's 128 output columns of the image
    Stager st;
    st.init(tid);
    // causal: query i sits at position len - Nq + i; a row half's rows span pos_lo .. pos_hi (wave-uniform)
    const int qpos = len - a.Nq + qi;
    const int pos_lo = len - a.Nq + row_query(a, q0 + 32 * rh);
    const int pos_hi2[2] = {len - a.Nq + row_query(a, q0 + 31), len - a.Nq + row_query(a, q0 + 63)};
    const int pos_hi = pos_hi2[rh];
    // The tile at key t (a multiple of 64) into the staging registers.  Paged: through the resource of the tile's page, sized to the
    // page's valid rows; behind a page's last tile the walk steps, and fetches the next page id only if another tile follows.
#define FA_MLA_LOAD(t)                                                                                        \
  {                                                                                                           \
    const int t_ = (t);                                                                                       \
    if constexpr (PAGED) {                                                                                    \
      const int prow = min(a.page_size, len - pw.slot * a.page_size);                                         \
      st.load(make_rsrc(reinterpret_cast<const T*>(a.k) + (size_t)pw.next * a.page_stride, (uint32_t)prow * ROWB), pw.off); \
      pw.off += MLA_TILE;                                                                                     \
      if (pw.off == a.page_size) {                                                                            \
        pw.off = 0;                                                                                           \
        ++pw.slot;                                                                                            \
        if (t_ + MLA_TILE < c1) pw.next = pw.id(a);                                                           \
      }                                                                                                       \
    } else {                                                                                                  \
      st.load(krs, t_);                                                                                       \
    }                                                                                                         \
  }
    if constexpr (PAGED) pw.init(a, b, c0);
    FA_MLA_LOAD(c0)
    for (int t0 = c0; t0 < c1; t0 += MLA_TILE) {
      __syncthreads();   // (the previous tile's reads of the image, of P and of alpha are done)
      st.store(tile);
      if (t0 + MLA_TILE < c1) FA_MLA_LOAD(t0 + MLA_TILE)
      __syncthreads();
      // ---- S^T = K Q^T for (key half, row half), the row on the lane ----
      const int kbase = t0 + 32 * kh;
      f32x16 s;
      if (half_live[rh] && kbase < c1 && !(a.causal && kbase > pos_hi)) {   // wave-uniform
        s = zero16();
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) A::mma(s, A::row_frag<D>(tile, ra, 32 * kh, kc), qf[kc]);
        if (kbase + 32 > c1 || (a.causal && kbase + 31 > pos_lo)) {   // wave-uniform: the 32 keys straddle the end or a position
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int key = kbase + acc_row(i, h);
            if (key >= c1 || (a.causal && key > qpos)) s[i] = -INFINITY;
          }
        }
      } else {   // no admissible key in the wave's 32, or no live row: the tile joins as -inf and P = 0, no MFMA is issued
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = -INFINITY;
      }
      float mx = s[0];
#pragma unroll
      for (int i = 1; i < 16; ++i) mx = fmaxf(mx, s[i]);
      mx = xhalf_max(mx);
      if (h == 0) *FA_LDS(float, rc_x + ((2 * rh + kh) * 32 + r) * 4) = mx;
      __syncthreads();
      // both key halves of a row half form the same m_new and the same alpha
      const float m_new = fmaxf(m_run, fmaxf(mx, *FA_LDS(float, rc_x + ((2 * rh + (kh ^ 1)) * 32 + r) * 4)));
      const float nm = (m_new == -INFINITY) ? 0.f : -m_new * c;   // (every key so far masked: any finite reference, P = 0)
      const float alpha = __builtin_amdgcn_exp2f(__builtin_fmaf(m_run, c, nm));
      float rs = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        s[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[i], c, nm));
        rs += s[i];
      }
      l_run = l_run * alpha + rs;
      m_run = m_new;
      // P at 16 significant bits (pack + pack_lo), as in decode_split_kernel, in the lane's own fragment order
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const frag p_hi = A::pack(s, s2);
        const frag p_lo = A::pack_lo(s, s2, p_hi);
        lds_char* dst = pbuf + (((2 * rh + kh) * 2 + s2) * 2) * 1024 + lane * 16;
        *FA_LDS(frag, dst) = p_hi;
        *FA_LDS(frag, dst + 1024) = p_lo;
      }
      if (kh == 0 && h == 0) *FA_LDS(float, rc_a + (32 * rh + r) * 4) = alpha;
      __syncthreads();
      // ---- O^T += V^T P^T for the wave's 128 columns, all 64 rows, all 64 keys ----
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        if (!half_live[x]) continue;
        const float al = *FA_LDS(float, rc_a + (32 * x + r) * 4);
        if (__any(al != 1.0f)) {
#pragma unroll
          for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc_o[x][dt][i] *= al;
        }
      }
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {   // k-step: keys 16 ks .. 16 ks + 15 of the tile (key half ks >> 1)
        const int kb = t0 + 32 * (ks >> 1);
        if (kb >= c1) break;   // wave-uniform: past the end, and so is every later step
        // (a key half above every position of a row half holds P = 0 there: skipped, wave-uniform)
        const bool use0 = !(a.causal && kb > pos_hi2[0]), use1 = half_live[1] && !(a.causal && kb > pos_hi2[1]);
        frag p[2][2];
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
          for (int hl = 0; hl < 2; ++hl) p[x][hl] = *FA_LDS(frag, pbuf + ((2 * x * 2 + ks) * 2 + hl) * 1024 + lane * 16);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const frag vt = A::tr_frag<D>(tcol, ta, 16 * ks, dt);
          if (use0) {
            A::mma(acc_o[0][dt], vt, p[0][0]);
            A::mma(acc_o[0][dt], vt, p[0][1]);
          }
          if (use1) {
            A::mma(acc_o[1][dt], vt, p[1][0]);
            A::mma(acc_o[1][dt], vt, p[1][1]);
          }
        }
      }
    }
#undef FA_MLA_LOAD
  }

  // the two key halves' row sums meet in LDS and are added in half order; m is the same in both
  const float l_w = xhalf_sum(l_run);
  __syncthreads();
  if (h == 0) {
    *FA_LDS(float, rc_x + ((2 * rh + kh) * 32 + r) * 4) = l_w;
    if (kh == 0) *FA_LDS(float, rc_a + (32 * rh + r) * 4) = m_run;
  }
  __syncthreads();
  const bool final_row = a.nsplit == 1;   // final: out = O / l, lse = m * tau + ln l; a row without an admissible key: out = 0, lse = -inf
#pragma unroll
  for (int x = 0; x < 2; ++x) {
    const int rho = q0 + 32 * x + r;
    if (rho >= rows) continue;   // (no barrier follows)
    const int qi = row_query(a, rho), hd = rho - qi * a.G;
    const float m_all = *FA_LDS(float, rc_a + (32 * x + r) * 4);
    const float l_tot = *FA_LDS(float, rc_x + (2 * x * 32 + r) * 4) + *FA_LDS(float, rc_x + ((2 * x + 1) * 32 + r) * 4);
    const float inv = !final_row ? 1.0f : (l_tot > 0.f) ? 1.0f / l_tot : 0.f;
    const size_t bhq = (size_t)b * a.H + hd;
    const size_t pr = (bhq * a.nsplit + split) * a.Nq + qi;
    float* orow = final_row ? a.out + (((size_t)b * a.Nq + qi) * a.H + hd) * MLA_DV : a.part_o + pr * MLA_DV;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 val = {acc_o[x][dt][4 * g] * inv, acc_o[x][dt][4 * g + 1] * inv, acc_o[x][dt][4 * g + 2] * inv, acc_o[x][dt][4 * g + 3] * inv};
        *reinterpret_cast<f32x4*>(orow + 32 * DT * w + 32 * dt + 8 * g + 4 * h) = val;
      }
    if (w != 0 || h != 0) continue;   // (m and l: every wave holds the same values, the first one stores them)
    if (!final_row) *reinterpret_cast<f32x2*>(a.part_ml + 2 * pr) = f32x2{m_all, l_tot};
    else if (a.lse) a.lse[bhq * a.Nq + qi] = (l_tot > 0.f) ? m_all * a.tau + __logf(l_tot) : -INFINITY;
  }
