// The body of mla_sparse_split_kernel<PAGED> (fa_mla_sparse.h) and of mla_fp8_sparse_split_kernel<PAGED> (fa_mla_fp8.h), included
// as TEXT inside both, as fa_mla_split_body.h is.  In scope: PAGED, FP8 and the argument a.  FP8 picks the gather that fills the
// tile image (MlaFp8Gather widens e4m3 codes to bf16 in front of LDS) and the bytes of a cache row.
  using T = bf16_t;
  using Gather = typename std::conditional<FP8, MlaFp8Gather<PAGED>, MlaGather<PAGED>>::type;
  constexpr int ROWB = FP8 ? MLA_FP8_ROW_BYTES : MLA_ROW_BYTES;
  using A = Atom<T>;
  typedef A::frag frag;
  constexpr int D = MLA_DQK, KC = D / 16, DT = MLA_DV / 32 / 4;
  constexpr int TB = A::tile_bytes<D>(MLA_TILE);   // 72 KB: the tile image
  constexpr int PB = 2 * 2 * 2 * 2 * 64 * 16;      // 16 KB: P as [row half][key half][k-step][hi, lo][lane] fragments
  constexpr int RC = 768;                          // row constants, as mla_decode_split_kernel's
  static_assert(TB + PB + RC <= 160 * 1024, "the tile image, P and the row constants must fit the CU's LDS");
  __shared__ __attribute__((aligned(16))) char smem_raw[TB + PB + RC];
  lds_char* tile = (lds_char*)smem_raw;
  lds_char* pbuf = tile + TB;
  lds_char* rc_x = pbuf + PB;
  lds_char* rc_a = rc_x + 512;

  // workgroup -> (item, head block) as in mla_decode_split_kernel; item = ((b, i), split)
  const int id = blockIdx.x, slot = id >> 3;
  const int qb = slot % a.nqb, item = (slot / a.nqb) * 8 + (id & 7);
  if (item >= a.items) return;
  const int bi = item / a.nsplit, split = item - bi * a.nsplit;
  const int b = bi / a.Nq, qi = bi - b * a.Nq;
  const int len = __builtin_amdgcn_readfirstlane(clamp_len(a, b));
  // admitted: (unsigned)j < lim.  Query qi sits at position len - Nq + qi.
  const int lim = max(a.causal ? len - a.Nq + qi + 1 : len, 0);
  const int c0 = split * a.chunk, ntile = (min(c0 + a.chunk, a.topk) - c0) / MLA_TILE;

  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6), kh = w & 1, rh = w >> 1;
  const int q0 = qb * MLA_BLOCK;
  const bool half_live[2] = {true, q0 + 32 < a.H};   // (wave-uniform; the first half of a block always has a live head)
  const float c = a.tau * LOG2E;

  f32x16 acc_o[2][DT];   // [row half][column tile]: O^T, the head on the lane
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc_o[x][dt] = zero16();
  float m_run = -INFINITY, l_run = 0.f;

  if (lim > 0) {   // (no position can be admitted: nothing is read, the empty partial m = -inf, l = 0 is left; workgroup-uniform)
    const int hd = q0 + 32 * rh + r;
    const uint32_t q_bytes = (uint32_t)a.q_bstride * 2;
    const rsrc_t qrs = make_rsrc(reinterpret_cast<const T*>(a.q) + (size_t)b * a.q_bstride, q_bytes);
    // the slab's resource ends at len_b: its size is the offset of a row that is not admitted (unused by a paged build)
    const uint32_t k_bytes = (uint32_t)len * ROWB;
    const rsrc_t krs = make_rsrc(reinterpret_cast<const T*>(a.k) + (PAGED ? 0 : (size_t)b * a.kv_bstride), k_bytes);
    const char* pool = reinterpret_cast<const char*>(a.k);
    const int* trow = a.table + (PAGED ? (size_t)b * a.max_pages : 0);
    const int* idx = a.indices + ((size_t)bi * a.topk + c0) + lane;   // entry `lane` of the chunk's tile 0

    // Q: the lane's head at the columns 16 kc + 8 h; heads >= H get the resource's size as their offset and read as zero
    frag qf[KC];
    const int qoff = hd < a.H ? (hd * (int)a.q_hstride + qi * a.q_ld + 8 * h) * 2 : (int)q_bytes;
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) qf[kc] = load_frag_buf<T>(qrs, qoff + 32 * kc);

    const LaneAddr ra = A::row_addr<D>(lane);
    const LaneAddr ta = A::tr_addr<D>(lane);
    lds_char* tcol = tile + 512 * DT * w;   // the wave's 128 output columns of the image
    Gather st;
    st.init(tid);

    // The pipeline's three stages, each on the lane's own entry of a tile.
    // request: the raw entry.  resolve: the compare (-1 = not admitted), and (paged) the page id's load for an admitted entry, of
    // which the row inside its page is kept.  load: the ballot, and the rows through what MlaGather::load takes, from the resolved
    // entry and the page id that has arrived.
    int j_raw = 0, j_res = -1, page = 0;
    uint64_t mask_cur = 0, mask_nxt = 0;
#define FA_SP_REQUEST(t) j_raw = idx[(t) * MLA_TILE];
#define FA_SP_RESOLVE()                                                      \
  {                                                                          \
    j_res = (uint32_t)j_raw < (uint32_t)lim ? j_raw : -1;                    \
    if constexpr (PAGED) {                                                   \
      if (j_res >= 0) {                                                      \
        const int slot_ = j_res / a.page_size;                               \
        page = trow[slot_];                                                  \
        j_res -= slot_ * a.page_size;                                        \
      }                                                                      \
    }                                                                        \
  }
#define FA_SP_LOAD()                                                                                          \
  {                                                                                                           \
    mask_nxt = __ballot(j_res >= 0);                                                                          \
    if (mask_nxt != 0) { /* wave-uniform, and the same in every wave */                                       \
      int src;                                                                                                \
      if constexpr (PAGED)                                                                                    \
        src = j_res >= 0 ? min(max(page, 0), a.num_pages - 1) * a.page_size + j_res : 0;                      \
      else                                                                                                    \
        src = j_res >= 0 ? j_res * ROWB : (int)k_bytes;                                              \
      st.load(krs, pool, src);                                                                                \
    }                                                                                                         \
  }
    FA_SP_REQUEST(0)
    FA_SP_RESOLVE()
    if (ntile > 1) FA_SP_REQUEST(1)
    FA_SP_LOAD()   // rows of tile 0
    if (ntile > 1) FA_SP_RESOLVE()
    if (ntile > 2) FA_SP_REQUEST(2)
    for (int t = 0; t < ntile; ++t) {
      mask_cur = mask_nxt;
      if (mask_cur != 0) {
        __syncthreads();   // (the previous tile's reads of the image, of P and of alpha are done)
        st.store(tile, mask_cur);
      }
      if (t + 1 < ntile) FA_SP_LOAD() else mask_nxt = 0;
      if (t + 2 < ntile) FA_SP_RESOLVE()
      if (t + 3 < ntile) FA_SP_REQUEST(t + 3)
      if (mask_cur == 0) continue;   // no admitted entry in the tile: m, l, O and alpha stay (workgroup-uniform)
      __syncthreads();
      // ---- S^T = K Q^T for (key half, row half), the head on the lane ----
      const uint32_t mh = (uint32_t)(mask_cur >> (32 * kh));   // the key half's 32 validity bits (wave-uniform)
      f32x16 s;
      if (half_live[rh] && mh != 0) {
        s = zero16();
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) A::mma(s, A::row_frag<D>(tile, ra, 32 * kh, kc), qf[kc]);
        if (mh != 0xffffffffu) {
          const uint32_t ml = mh >> (4 * h);   // bit acc_row(i, 0) of it is key acc_row(i, h)
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (!((ml >> acc_row(i, 0)) & 1)) s[i] = -INFINITY;
        }
      } else {   // no admitted key in the wave's 32, or no live head: the half joins as -inf and P = 0, no MFMA is issued
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
      const float nm = (m_new == -INFINITY) ? 0.f : -m_new * c;   // (a dead head: any finite reference, P = 0)
      const float alpha = __builtin_amdgcn_exp2f(__builtin_fmaf(m_run, c, nm));
      float rs = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        s[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[i], c, nm));
        rs += s[i];
      }
      l_run = l_run * alpha + rs;
      m_run = m_new;
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
      // ---- O^T += V^T P^T for the wave's 128 columns, all 64 heads, the k-steps that hold an admitted key ----
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
      for (int ks = 0; ks < 4; ++ks) {   // k-step: entries 16 ks .. 16 ks + 15 of the tile
        if (((mask_cur >> (16 * ks)) & 0xffffu) == 0) continue;   // wave-uniform: P = 0 on all 16
        frag p[2][2];
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
          for (int hl = 0; hl < 2; ++hl) p[x][hl] = *FA_LDS(frag, pbuf + ((2 * x * 2 + ks) * 2 + hl) * 1024 + lane * 16);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const frag vt = A::tr_frag<D>(tcol, ta, 16 * ks, dt);
          A::mma(acc_o[0][dt], vt, p[0][0]);
          A::mma(acc_o[0][dt], vt, p[0][1]);
          if (half_live[1]) {
            A::mma(acc_o[1][dt], vt, p[1][0]);
            A::mma(acc_o[1][dt], vt, p[1][1]);
          }
        }
      }
    }
#undef FA_SP_REQUEST
#undef FA_SP_RESOLVE
#undef FA_SP_LOAD
  }

  // the two key halves' row sums meet in LDS and are added in half order; m is the same in both
  const float l_w = xhalf_sum(l_run);
  __syncthreads();
  if (h == 0) {
    *FA_LDS(float, rc_x + ((2 * rh + kh) * 32 + r) * 4) = l_w;
    if (kh == 0) *FA_LDS(float, rc_a + (32 * rh + r) * 4) = m_run;
  }
  __syncthreads();
  const bool final_row = a.nsplit == 1;   // final: out = O / l, lse = m * tau + ln l; no admitted entry: out = 0, lse = -inf
#pragma unroll
  for (int x = 0; x < 2; ++x) {
    const int hd = q0 + 32 * x + r;
    if (hd >= a.H) continue;   // (no barrier follows)
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
