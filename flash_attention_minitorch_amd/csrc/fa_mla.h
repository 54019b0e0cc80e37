// Multi-head latent attention (DeepSeek-V2 / V3 / R1, Kimi-K2) decode on a latent KV cache, for MI355X (gfx950): bf16, one cache row of
// 576 columns per token shared by ALL heads -- the compressed latent c_kv (512 columns) followed by the rotated k_pe (64).  With the
// up-projections absorbed into q a step is multi-query attention in which the score product runs over all 576 columns, the value is
// the first 512 columns of the SAME row, and the result is (H, 512) per token.  Declared in include/flash_attn_mi355x_mla.h,
// dispatched by fa_mla.hip; the atoms, make_rsrc, clamp_len, row_query and the page walk are fa_atoms.h's and fa_decode.h's, used as
// they are (this unit changes no shared definition: every other library's code object stays what it is).
//
// mla_decode_split_kernel<PAGED>: 256 threads, one wave per SIMD on the whole 512-entry register file; a workgroup = one (batch, key
// chunk, 64-row block).  Rows run in the decode kernels' order with G = H: rho = i * H + h for query i and head h; rows >= H * Nq read
// as zero and store nothing, and a 32-row half without a live row is skipped wave-uniformly in both products.
//   * The cache is walked in 64-key tiles of 576 columns (72 KB) in the image Atom<bf16_t>::off<576>, staged through registers
//     (MlaStager: 18 x 16 bytes per thread, the next tile's loads issued in front of this tile's MFMAs).  ONE image serves both
//     products: S reads row fragments over all 36 k-chunks, P.V reads transposed fragments of columns 0..511 of the same image, so a
//     cache row crosses HBM once and LDS once per workgroup.
//   * S: wave w = (key half kh = w & 1, row half rh = w >> 1) forms ONE 32 x 32 tile of S^T = K Q^T over the full 576 columns, 36 MFMAs
//     against its 32 rows of Q held as 144 registers of fragments (loaded once per workgroup).  The two key halves of a row half
//     exchange their tile maxima through LDS and form the same m_new and the same alpha; P = exp2(s c - m_new c) goes to LDS as the
//     bf16 pair pack + pack_lo (16 KB for 64 x 64, in the lanes' own fragment order: a reader's fragment is the writer's), alpha per
//     row beside it.  Each wave keeps the row sums of its own key half; the two halves are added once, at the end.
//   * P.V: every wave takes the output columns 128 w .. 128 w + 127 of all 64 rows over all 64 keys: 8 accumulator tiles (128
//     registers), per staged tile 4 k-steps x 8 tiles x 2 (hi, lo) = 64 MFMAs, rescaled by the alpha read from LDS.  So a tile costs
//     every wave 36 + 64 MFMAs and none of them is issued twice in the workgroup (decode_split_d256_kernel forms S once per column
//     half: free when the cache stream is the limit, not at H = 128 where the MFMAs are).
//   * One split stores out = O / l and lse = m tau + ln l; several splits store (o[512], m, l) partials, which
//     mla_decode_combine_kernel merges in split order (decode_combine_kernel's body text at 512 columns).  No atomics: a call repeats
//     bit for bit.  Chunks are whole multiples of 128 keys and a page a multiple of FA_PAGE_ROWS rows, so a tile lies inside one page
//     and a paged call returns the slab call's bits on the gathered cache.  Resources end at len_b or at the page.
// mla_append_kernel: token i of batch element b goes to row len_b - Nq + i, slab or paged, in 16-byte moves.
//
// Not built: window, sink tokens, soft cap, learned sink logits, fp8 latents, the ragged family, an extend kernel for long prefills,
// other latent widths, the training backward.  (Attention over per-query index lists, DeepSeek-V3.2's sparse attention, is a kernel
// of its own on this image and these products: fa_mla_sparse.h.)
#pragma once
#include "fa_atoms.h"
#include "fa_common.h"
#include "fa_decode.h"

namespace fa {

constexpr int MLA_DQK = 576, MLA_DV = 512;   // columns of a cache row (and of q); columns of it that are the value (and of out)
constexpr int MLA_TILE = 64;                 // keys per staged tile: 32 per key half
constexpr int MLA_BLOCK = 64;                // rows per workgroup: 32 per row half
constexpr int MLA_ROW_BYTES = MLA_DQK * 2;

// The register-staged copy of one 64 x 576 bf16 tile by 256 threads: 72 chunks of 16 bytes per row, which TileStager cannot tile
// (256 % 72 != 0).  Pass i = 2 * sp + rph of 18 moves, for lane group g = tid >> 3, the rows 2 * (g >> 1) + 32 * rph (+ 1 for the
// odd half of the group) at the four chunks of the 32-column subtile 2 * sp + (g & 1).  Eight consecutive lanes cover two adjacent
// rows x four chunks of one subtile (the image's ds_write_b128 rule, as TileStager), sixteen cover 128 contiguous bytes of each of
// two cache rows, and a row step of 32 keeps the swizzle phase: a thread's 18 global offsets and 18 LDS offsets are one register
// each plus compile-time constants.
struct MlaStager {
  static constexpr int CPR = MLA_DQK / 8, NCH = MLA_TILE * CPR, PER = NCH / 256;
  static_assert(NCH % 256 == 0 && PER == 18, "every thread moves 18 chunks");
  static constexpr int row_of(int tid, int i) { return 2 * (tid >> 4) + ((tid >> 2) & 1) + 32 * (i & 1); }
  static constexpr int chunk_of(int tid, int i) { return 4 * (2 * (i >> 1) + ((tid >> 3) & 1)) + (tid & 3); }
  static constexpr int src_step(int i) { return 32 * MLA_ROW_BYTES * (i & 1) + 128 * (i >> 1); }
  static constexpr int lds_step(int i) { return Atom<bf16_t>::off<MLA_DQK>(32 * (i & 1), 8 * (i >> 1)); }
  // every (row, chunk) of the tile exactly once, at the offsets init and the two steps form; eight lanes: two adjacent rows, one subtile
  static constexpr bool covers_image() {
    bool seen[NCH] = {};
    for (int tid = 0; tid < 256; ++tid)
      for (int i = 0; i < PER; ++i) {
        const int row = row_of(tid, i), ch = chunk_of(tid, i);
        if (row >= MLA_TILE || ch >= CPR || seen[row * CPR + ch]) return false;
        seen[row * CPR + ch] = true;
        if (Atom<bf16_t>::off<MLA_DQK>(row, ch) != Atom<bf16_t>::off<MLA_DQK>(row_of(tid, 0), chunk_of(tid, 0)) + lds_step(i)) return false;
        if (row * MLA_ROW_BYTES + ch * 16 != row_of(tid, 0) * MLA_ROW_BYTES + chunk_of(tid, 0) * 16 + src_step(i)) return false;
        const int t0 = tid & ~7;
        if ((row >> 1) != (row_of(t0, i) >> 1) || (ch >> 2) != (chunk_of(t0, i) >> 2)) return false;
      }
    return true;
  }
  u32x4 regs[PER];
  int voff, lds_off;
  FA_DEV void init(int tid) {
    voff = row_of(tid, 0) * MLA_ROW_BYTES + chunk_of(tid, 0) * 16;
    lds_off = Atom<bf16_t>::off<MLA_DQK>(row_of(tid, 0), chunk_of(tid, 0));
  }
  // The tile whose first row is row0 of the matrix the resource covers.  The row offset rides in the voffset, so the resource's
  // range check covers it: rows at or past the resource's end (len_b, or the page's valid rows) read as zero.
  FA_DEV void load(rsrc_t rs, int row0) {
#pragma unroll
    for (int i = 0; i < PER; ++i)
      regs[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff + row0 * MLA_ROW_BYTES + src_step(i), 0, 0));
  }
  FA_DEV void store(lds_char* tile) const {
#pragma unroll
    for (int i = 0; i < PER; ++i) *FA_LDS(u32x4, tile + lds_off + lds_step(i)) = regs[i];
  }
};
static_assert(MlaStager::covers_image(), "the stager's lane-to-chunk map must tile the 64 x 576 image once, by the image's write rule");

// The kernels' argument is fa_decode.h's DecodeArgs with Hkv = 1 and G = H (row_query, clamp_len and PageWalk read it as it is):
// q [B][Nq][H][576] (q_ld = H * 576, q_hstride = 576, q_bstride = Nq * H * 576), k = the latent cache (kv_ld = 576, kv_hstride = 0,
// kv_bstride = Ncap * 576, page_stride = page_size * 576; v is not read), items = B * nsplit, nqb = ceil(H * Nq / 64).
// out is [B][Nq][H][512], lse [B][H][Nq], the partials [B * H][nsplit][Nq][512] and [..][2] as decode_combine_kernel reads them.
template <bool PAGED>
__global__ void __launch_bounds__(256) mla_decode_split_kernel(DecodeArgs a) {
  using T = bf16_t;
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
    const rsrc_t krs = make_rsrc(reinterpret_cast<const T*>(a.k) + (PAGED ? 0 : (size_t)b * a.kv_bstride), (uint32_t)len * MLA_ROW_BYTES);
    PageWalk pw;   // (paged) stands on the page of the tile that is loaded next; stepped by 64-key tiles here

    // Q: the lane's row at the columns 16 kc + 8 h; rows >= H * Nq get the resource's size as their offset and read as zero
    frag qf[KC];
    const int qoff = rho < rows ? (hd * (int)a.q_hstride + qi * a.q_ld + 8 * h) * 2 : (int)q_bytes;
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) qf[kc] = load_frag_buf<T>(qrs, qoff + 32 * kc);

    const LaneAddr ra = A::row_addr<D>(lane);
    const LaneAddr ta = A::tr_addr<D>(lane);
    lds_char* tcol = tile + 512 * DT * w;   // the wave's 128 output columns of the image
    MlaStager st;
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
      st.load(make_rsrc(reinterpret_cast<const T*>(a.k) + (size_t)pw.next * a.page_stride, (uint32_t)prow * MLA_ROW_BYTES), pw.off); \
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
}

// The combine kernel at 512 columns: decode_combine_kernel's body text (thread (g, j): columns 4g .. 4g+3 of the splits j, j + 2,
// ...; the two partial sums of a column group added in the order j = 0, 1; in log2 units).  It addresses out through q's strides, so
// the host hands it the argument with OUT's strides in their place (q itself is not read here).
// (RAGGED is never true: it makes the argument's type depend on a template parameter, for the reason decode_split_sink_kernel gives.)
template <bool RAGGED>
__global__ void __launch_bounds__(256) mla_decode_combine_kernel(DecodeArgsOf<RAGGED> a) {
  constexpr int D = MLA_DV;
  constexpr bool FP8 = false, LSINK = false;
#include "fa_decode_combine_body.h"
}

// Append: kv_new [B][Nq][576] into the cache.  With L_b = len_b clamped to [0, Ncap] (the length COUNTS the new tokens), token i goes
// to row L_b - Nq + i, the position the causal mask gives query i; rows below 0 are not written and no row reaches Ncap.  A lane moves
// one 16-byte chunk; page ids are clamped to the pool as the split kernel's.
struct MlaAppendArgs {
  const void* kv_new;
  void* kv;
  const int* seqlens;   // [B] or null (= Ncap)
  const int* table;     // [B][max_pages] or null: slabs of Ncap rows
  long lanes;           // B * Nq * 72
  int Nq, Ncap, page_size, num_pages, max_pages;
};

__global__ void __launch_bounds__(256) mla_append_kernel(MlaAppendArgs a) {
  constexpr int CPR = MlaStager::CPR;
  const long lane = (long)blockIdx.x * 256 + threadIdx.x;
  if (lane >= a.lanes) return;
  const long row = lane / CPR;   // source row (b, i)
  const int ch = (int)(lane - row * CPR), b = (int)(row / a.Nq), i = (int)(row - (long)b * a.Nq);
  const int pos = clamp_len(a.seqlens, a.Ncap, b) - a.Nq + i;
  if (pos < 0) return;
  size_t dst_row;
  if (a.table) {
    const int slot = pos / a.page_size;
    const int page = min(max(a.table[(size_t)b * a.max_pages + slot], 0), a.num_pages - 1);
    dst_row = (size_t)page * a.page_size + (pos - slot * a.page_size);
  } else {
    dst_row = (size_t)b * a.Ncap + pos;
  }
  reinterpret_cast<u32x4*>(a.kv)[dst_row * CPR + ch] = reinterpret_cast<const u32x4*>(a.kv_new)[lane];
}

}  // namespace fa
