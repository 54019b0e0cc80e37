// Head dim 256 for the KV-cache calls (Gemma-2 2B / 9B, most of Gemma-3): bf16, d = 256 exactly, the decode and the extend family,
// slab or paged, windowed or not, soft-capped or not.  Declared in include/flash_attn_mi355x_decode_d256.h, dispatched by
// fa_decode.hip (launch_d256).  Kernels of their own, not the bodies of fa_decode.h at D = 256: two 128-key tile images of 64 KB each
// leave room for ONE four-wave workgroup per CU there, whose threads stage 2 x 64 registers beside 64 of Q and 128 of accumulators.
// What stays: the 128-key super tile (so FA_PAGE_ROWS, the page walk, the chunk rounding and policy() apply as they are), the row
// order rho = i * G + g, the resources that end at len_b or at the page, the partials' layout (decode_combine_kernel's), the cap in
// front of the masks.  The atoms are fa_atoms.h's: the tile image Atom<bf16_t>::off<256>, row_frag / tr_frag, pack + pack_lo.
//
// decode_split_d256_kernel: 512 threads, a workgroup = one (batch * kv head, key chunk, 32-row block).  All eight waves stage the
// 128 x 256 images of K and V (32 + 32 staging registers per thread).  Wave w = (key quarter kq = w & 3, column half ch = w >> 2)
// forms S for its 32 keys over the full d (16 MFMAs; the two column halves of a key quarter compute the same S, m and l, bit for
// bit: the same instructions on the same LDS image, free in a kernel bound by the cache stream) and the P.V product for the output
// columns 128 ch .. 128 ch + 127 alone: 64 accumulator registers.  Two waves per SIMD inside the one workgroup, so a wave has 256
// registers and no AGPRs to spare: the block's 32 rows of Q are a third LDS image (16 KB) read as row fragments beside K's, not
// 64 registers of fragments (the build is at 207 VGPRs without them: with them it does not fit; DESIGN.md "d = 256").  At the end the
// partials of the key quarters 1-3 of each column half meet in LDS over the tile images (6 x 16.5 KB) and the waves of key quarter 0
// add them in quarter order: no atomics, a call repeats bit for bit.
//
// extend_split_d256_kernel: 256 threads, a workgroup = one (batch * kv head, key chunk, 128-row block), wave w owns rows 32 w .. + 31
// and ALL 256 output columns (128 accumulator registers; with 64 of Q fragments the kernel runs at one wave per SIMD on the whole
// 512-entry file).  K and V are staged as the two 64-KEY HALVES of a super tile (HalfStager256): 32 + 32 staging registers per thread
// where a whole tile would take 64 + 64, and two 32 KB images.  No cross-wave merge.  A causal call loads no half above the block's last
// position, a windowed one none wholly below the block's edge.
//
// Both kernels are compiled without packed fp32 instructions (FA_NO_PK_F32), whatever the library's flags say.
#pragma once
#include "fa_decode.h"

namespace fa {

#if defined(__HIP_DEVICE_COMPILE__)
#define FA_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define FA_NO_PK_F32   // (the host pass knows no such feature)
#endif

constexpr int D256 = 256;
// The argument of every d256 build: DecodeArgs and the cap, which the SOFTCAP builds alone read.
using D256Args = SoftcapArgs;

template <bool PAGED, bool WINDOW, bool SOFTCAP>
__global__ void FA_NO_PK_F32 __launch_bounds__(512) decode_split_d256_kernel(D256Args a) {
  using T = bf16_t;
  using A = Atom<T>;
  typedef A::frag frag;
  constexpr int D = D256, KC = D / 16, DTH = D / 64;   // DTH: the 32-column tiles of a wave's column half
  constexpr int TB = A::tile_bytes<D>(DEC_ROWS);
  constexpr int PW = (16 * DTH + 2) * 64 * 4;   // one wave's partial: [lane][16*DTH accumulator registers, m, l]
  static_assert(6 * PW <= 2 * TB, "the partials of key quarters 1-3 of both column halves must fit the tile images");
  __shared__ __attribute__((aligned(16))) char smem_raw[2 * TB + A::tile_bytes<D>(32)];
  lds_char* tk = (lds_char*)smem_raw;
  lds_char* tv = tk + TB;
  lds_char* tq = tv + TB;   // the block's 32 rows of Q in the image of a 32-row tile

  // workgroup -> (item, row block) as in decode_split_kernel
  const int id = blockIdx.x, slot = id >> 3;
  const int qb = slot % a.nqb, item = (slot / a.nqb) * 8 + (id & 7);
  if (item >= a.items) return;
  const int bh = item / a.nsplit, split = item - bh * a.nsplit;
  const int b = bh / a.Hkv, hkv = bh - b * a.Hkv;
  const int len = __builtin_amdgcn_readfirstlane(clamp_len(a, b));
  int wedge = 0;   // (window builds) the block's window edge; the key range starts at the super tile that holds it
  if constexpr (WINDOW) wedge = max(len - a.Nq + row_query(a, qb * 32) - a.window + 1, 0);
  const int c0 = (WINDOW ? wedge & ~(DEC_ROWS - 1) : 0) + split * a.chunk, c1 = min(c0 + a.chunk, len);

  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6), kq = w & 3, ch = w >> 2;
  const int q0 = qb * 32, rho = q0 + r, qi = row_query(a, rho), hd = hkv * a.G + (rho - qi * a.G);
  const bool live = rho < a.G * a.Nq;
  // (softcap builds: the capped scores ARE the logits, so the softmax's tau is 1; k2 is cap_score's exp2 constant)
  float k2 = 0.f;
  if constexpr (SOFTCAP) k2 = cap_k2(a.tau, a.softcap);
  const float tau = SOFTCAP ? 1.0f : a.tau, c = tau * LOG2E;

  f32x16 acc_o[DTH];
#pragma unroll
  for (int dt = 0; dt < DTH; ++dt) acc_o[dt] = zero16();
  float m_run = -INFINITY, l_run = 0.f;

  if (c0 < c1) {   // (a chunk wholly past len_b loads nothing and leaves the empty partial m = -inf, l = 0)
    const size_t kvoff = (PAGED ? 0 : (size_t)b * a.kv_bstride) + (size_t)hkv * a.kv_hstride;   // (paged: inside a page)
    const uint32_t esz = sizeof(T);
    const uint32_t q_bytes = (uint32_t)a.q_bstride * esz;
    const rsrc_t qrs = make_rsrc(reinterpret_cast<const T*>(a.q) + (size_t)b * a.q_bstride, q_bytes);
    const uint32_t kv_bytes = ((uint32_t)(len - 1) * a.kv_ld + D) * esz;
    const rsrc_t krs = make_rsrc(reinterpret_cast<const T*>(a.k) + kvoff, kv_bytes);   // (the slab's: unused by a paged build)
    const rsrc_t vrs = make_rsrc(reinterpret_cast<const T*>(a.v) + kvoff, kv_bytes);
    PageWalk pw;

    // Q: thread t brings chunk t & 31 of the rows t >> 5 and 16 + (t >> 5) of the block; rows >= G * Nq get the resource's size as
    // their offset and read as zero
    u32x4 qreg[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int rr = q0 + (tid >> 5) + 16 * i, qr = row_query(a, rr), hr = hkv * a.G + (rr - qr * a.G);
      const int off = rr < a.G * a.Nq ? (hr * (int)a.q_hstride + qr * a.q_ld + 8 * (tid & 31)) * (int)esz : (int)q_bytes;
      qreg[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(qrs, off, 0, 0));
    }

    const LaneAddr ra = A::row_addr<D>(lane);
    const LaneAddr ta = A::tr_addr<D>(lane);
    TileStager<T, D, DEC_ROWS, 512> sk, sv;
    sk.init(tid, a.kv_ld);
    sv.init(tid, a.kv_ld);
    // causal: query i sits at position len - Nq + i; the block's rows span pos_lo .. pos_hi (wave-uniform)
    const int qpos = len - a.Nq + qi;
    const int pos_lo = len - a.Nq + row_query(a, q0), pos_hi = len - a.Nq + row_query(a, q0 + 31);
    if constexpr (PAGED) {
      pw.init(a, b, c0);
      pw.template load<T, D>(a, sk, sv, kvoff, len, c0 + DEC_ROWS < c1);
    } else {
      load_rows(sk, krs, c0);
      load_rows(sv, vrs, c0);
    }
    if constexpr (WINDOW) {
      if (c0 < wedge) {   // (split 0 of a block whose edge is inside a super tile: those rows may hold anything)
        zero_below(sk, wedge - c0);
        zero_below(sv, wedge - c0);
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) *FA_LDS(u32x4, tq + A::off<D>((tid >> 5) + 16 * i, tid & 31)) = qreg[i];   // (the loop's barriers publish it)
    for (int t0 = c0; t0 < c1; t0 += DEC_ROWS) {
      __syncthreads();   // (the previous super tile's reads are done)
      sk.store(tk);
      sv.store(tv);
      if (t0 + DEC_ROWS < c1) {
        if constexpr (PAGED) {
          pw.template load<T, D>(a, sk, sv, kvoff, len, t0 + 2 * DEC_ROWS < c1);
        } else {
          load_rows(sk, krs, t0 + DEC_ROWS);
          load_rows(sv, vrs, t0 + DEC_ROWS);
        }
      }
      __syncthreads();
      const int kbase = t0 + 32 * kq;
      if (kbase >= c1 || (a.causal && kbase > pos_hi)) continue;   // wave-uniform: no admissible key in the wave's 32
      if constexpr (WINDOW) {
        if (kbase + 31 <= pos_lo - a.window) continue;   // wave-uniform: the 32 keys are below every row's window
      }
      f32x16 s = zero16();
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) A::mma(s, A::row_frag<D>(tk, ra, 32 * kq, kc), A::row_frag<D>(tq, ra, 0, kc));
      if constexpr (SOFTCAP) {   // the cap, in front of the masks: a masked score must stay -inf, not become -softcap
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = cap_score(s[i], k2, a.softcap);
      }
      if (kbase + 32 > c1 || (a.causal && kbase + 31 > pos_lo) || (WINDOW && kbase <= pos_hi - a.window)) {   // wave-uniform
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int key = kbase + acc_row(i, h);
          if (key >= c1 || (a.causal && key > qpos) || (WINDOW && key <= qpos - a.window)) s[i] = -INFINITY;
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
        for (int dt = 0; dt < DTH; ++dt)
#pragma unroll
          for (int i = 0; i < 16; ++i) acc_o[dt][i] *= alpha;
      }
      l_run = l_run * alpha + rs;
      m_run = m_new;
      // P at 16 significant bits (pack + pack_lo), as in decode_split_kernel; the wave's own column half of V
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const frag p_hi = A::pack(s, s2);
        const frag p_lo = A::pack_lo(s, s2, p_hi);
#pragma unroll
        for (int dt = 0; dt < DTH; ++dt) {
          const frag vt = A::tr_frag<D>(tv + 512 * DTH * ch, ta, 32 * kq + 16 * s2, dt);
          A::mma(acc_o[dt], vt, p_hi);
          A::mma(acc_o[dt], vt, p_lo);
        }
      }
    }
  }
  const float l_w = xhalf_sum(l_run);

  // the partials of key quarters 1-3 meet in LDS (over the tile images), key quarter 0 of each column half adds them in quarter order
  constexpr int PL = (16 * DTH + 2) * 4;   // bytes of one lane's partial
  __syncthreads();
  if (kq != 0) {
    lds_char* mine = tk + (3 * ch + kq - 1) * PW + lane * PL;
#pragma unroll
    for (int dt = 0; dt < DTH; ++dt)
#pragma unroll
      for (int i = 0; i < 16; ++i) *FA_LDS(float, mine + (16 * dt + i) * 4) = acc_o[dt][i];
    *FA_LDS(float, mine + 16 * DTH * 4) = m_run;
    *FA_LDS(float, mine + (16 * DTH + 1) * 4) = l_w;
  }
  __syncthreads();
  if (kq != 0) return;
  lds_char* theirs = tk + 3 * ch * PW + lane * PL;
  float m_all = m_run;
#pragma unroll
  for (int u = 0; u < 3; ++u) m_all = fmaxf(m_all, *FA_LDS(float, theirs + u * PW + 16 * DTH * 4));
  float wgt = (m_run == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f((m_run - m_all) * c);
  float l_tot = l_w * wgt;
#pragma unroll
  for (int dt = 0; dt < DTH; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc_o[dt][i] *= wgt;
  // (one partial at a time: unrolled, the three partials' 192 LDS reads are all issued in front of the adds and 32 registers spill)
#pragma unroll 1
  for (int u = 0; u < 3; ++u) {
    lds_char* pu = theirs + u * PW;
    const float mu = *FA_LDS(float, pu + 16 * DTH * 4);
    wgt = (mu == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f((mu - m_all) * c);
    l_tot += *FA_LDS(float, pu + (16 * DTH + 1) * 4) * wgt;
#pragma unroll
    for (int dt = 0; dt < DTH; ++dt)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc_o[dt][i] += *FA_LDS(float, pu + (16 * dt + i) * 4) * wgt;
  }
  if (!live) return;
  const size_t bhq = (size_t)b * a.H + hd;
  const bool final_row = a.nsplit == 1;   // final: out = O / l, lse = m * tau + ln l; a row without an admissible key: out = 0, lse = -inf
  const float inv = !final_row ? 1.0f : (l_tot > 0.f) ? 1.0f / l_tot : 0.f;
  const size_t pr = (bhq * a.nsplit + split) * a.Nq + qi;
  float* orow = final_row ? a.out + (size_t)b * a.q_bstride + (size_t)hd * a.q_hstride + (size_t)qi * a.q_ld : a.part_o + pr * D;
#pragma unroll
  for (int dt = 0; dt < DTH; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x4 val = {acc_o[dt][4 * g] * inv, acc_o[dt][4 * g + 1] * inv, acc_o[dt][4 * g + 2] * inv, acc_o[dt][4 * g + 3] * inv};
      *reinterpret_cast<f32x4*>(orow + 128 * ch + 32 * dt + 8 * g + 4 * h) = val;
    }
  if (h != 0 || ch != 0) return;   // (m and l: the two column halves hold the same values, the first one stores them)
  if (!final_row) *reinterpret_cast<f32x2*>(a.part_ml + 2 * pr) = f32x2{m_all, l_tot};
  else if (a.lse) a.lse[bhq * a.Nq + qi] = (l_tot > 0.f) ? m_all * tau + __logf(l_tot) : -INFINITY;
}

// ---- extend ----
// The register-staged copy of a 64-KEY HALF of a super tile, 64 x 256 bf16, by 256 threads: TileStager's (row, chunk) map and LDS
// image with eight rows between a thread's consecutive chunks, where TileStager needs sixteen to keep the image's swizzle phase.
// Here the phase alternates with the chunk's parity, so a thread carries two LDS offsets.  load_rows, zero_below and a page's
// resource take it as they take TileStager.
struct HalfStager256 {
  static constexpr int ROWS = 64, NCH = ROWS * 32, PER = 8, RSTEP = 8;
  static constexpr bool live = true;
  u32x4 regs[PER];
  int voff, ldb, lds_off[2];
  FA_DEV void init(int tid, int ld) {
    ldb = ld * 2;
    const int g = tid >> 3, row = 2 * (g >> 3) + ((tid >> 2) & 1), ch = 4 * (g & 7) + (tid & 3);   // (TileStager's bf16 lane groups)
    voff = row * ldb + ch * 16;
    lds_off[0] = Atom<bf16_t>::off<D256>(row, ch);
    lds_off[1] = Atom<bf16_t>::off<D256>(row + 8, ch) - Atom<bf16_t>::off<D256>(8, 0);
  }
  FA_DEV void store(lds_char* tile) const {
#pragma unroll
    for (int i = 0; i < PER; ++i) *FA_LDS(u32x4, tile + lds_off[i & 1] + Atom<bf16_t>::off<D256>(8 * i, 0)) = regs[i];
  }
};
static_assert(Atom<bf16_t>::off<D256>(5 + 8 * 3, 6) == Atom<bf16_t>::off<D256>(5 + 8, 6) - Atom<bf16_t>::off<D256>(8, 0) + Atom<bf16_t>::off<D256>(24, 0) &&
                  Atom<bf16_t>::off<D256>(5 + 8 * 2, 6) == Atom<bf16_t>::off<D256>(5, 6) + Atom<bf16_t>::off<D256>(16, 0),
              "the image's swizzle phase follows the parity of the eight-row group");

template <bool PAGED, bool WINDOW, bool SOFTCAP>
__global__ void FA_NO_PK_F32 __launch_bounds__(256) extend_split_d256_kernel(D256Args a) {
  using T = bf16_t;
  using A = Atom<T>;
  typedef A::frag frag;
  constexpr int D = D256, KC = D / 16, DT = D / 32, HALF = HalfStager256::ROWS;
  constexpr int TB = A::tile_bytes<D>(HALF);
  __shared__ __attribute__((aligned(16))) char smem_raw[2 * TB];
  lds_char* tk = (lds_char*)smem_raw;
  lds_char* tv = tk + TB;

  const int id = blockIdx.x, slot = id >> 3;
  const int qb = slot % a.nqb, item = (slot / a.nqb) * 8 + (id & 7);
  if (item >= a.items) return;
  const int bh = item / a.nsplit, split = item - bh * a.nsplit;
  const int b = bh / a.Hkv, hkv = bh - b * a.Hkv;
  const int len = __builtin_amdgcn_readfirstlane(clamp_len(a, b));
  int wedge = 0;   // (window builds) the lowest key the 128-row block's first row admits
  if constexpr (WINDOW) wedge = max(len - a.Nq + row_query(a, qb * EXT_BLOCK) - a.window + 1, 0);
  const int c0 = (WINDOW ? wedge & ~(DEC_ROWS - 1) : 0) + split * a.chunk, c1 = min(c0 + a.chunk, len);
  // the first half that is staged: a chunk's first, or (split 0 of a windowed block) the half that holds the edge
  const int h0 = WINDOW ? max(c0, wedge & ~(HALF - 1)) : c0;

  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rows = a.G * a.Nq;
  const int q0 = qb * EXT_BLOCK + 32 * w, rho = q0 + r, qi = row_query(a, rho), hd = hkv * a.G + (rho - qi * a.G);
  const bool live = rho < rows;
  const bool wave_live = q0 < rows;   // (wave-uniform)
  float k2 = 0.f;
  if constexpr (SOFTCAP) k2 = cap_k2(a.tau, a.softcap);
  const float tau = SOFTCAP ? 1.0f : a.tau, c = tau * LOG2E;
  // causal: the last key any row of the block sees is the position of its last REAL row
  const int blk_hi = len - a.Nq + row_query(a, min(qb * EXT_BLOCK + EXT_BLOCK, rows) - 1);
  const int cend = a.causal ? min(c1, blk_hi + 1) : c1;

  f32x16 acc_o[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) acc_o[dt] = zero16();
  float m_run = -INFINITY, l_run = 0.f;

  if (h0 < cend) {   // (a chunk past len_b, or past every position of the block, loads nothing and leaves m = -inf, l = 0)
    const size_t kvoff = (PAGED ? 0 : (size_t)b * a.kv_bstride) + (size_t)hkv * a.kv_hstride;   // (paged: inside a page)
    const uint32_t esz = sizeof(T);
    const uint32_t q_bytes = (uint32_t)a.q_bstride * esz;
    const rsrc_t qrs = make_rsrc(reinterpret_cast<const T*>(a.q) + (size_t)b * a.q_bstride, q_bytes);
    const uint32_t kv_bytes = ((uint32_t)(len - 1) * a.kv_ld + D) * esz;
    const rsrc_t krs = make_rsrc(reinterpret_cast<const T*>(a.k) + kvoff, kv_bytes);   // (the slab's: unused by a paged build)
    const rsrc_t vrs = make_rsrc(reinterpret_cast<const T*>(a.v) + kvoff, kv_bytes);
    // (paged) the walk stands on the super tile of the half that is loaded next: PageWalk's fields, stepped after a tile's second half
    PageWalk pw;
    if constexpr (PAGED) pw.init(a, b, h0 & ~(DEC_ROWS - 1));

    frag qf[KC];
    const int qoff = live ? (hd * (int)a.q_hstride + qi * a.q_ld + 8 * h) * (int)esz : (int)q_bytes;
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) qf[kc] = load_frag_buf<T>(qrs, qoff + 16 * kc * (int)esz);

    const LaneAddr ra = A::row_addr<D>(lane);
    const LaneAddr ta = A::tr_addr<D>(lane);
    HalfStager256 sk, sv;
    sk.init(tid, a.kv_ld);
    sv.init(tid, a.kv_ld);
    const int qpos = len - a.Nq + qi;
    const int pos_lo = len - a.Nq + row_query(a, q0), pos_hi = len - a.Nq + row_query(a, q0 + 31);
    // The half at key t (a multiple of 64) into the staging registers.  Paged: through the resource of the tile's page, sized to
    // the page's valid rows, as PageWalk::load does; behind a tile's second half the walk steps, and fetches the next page id only
    // if another half follows.  Windowed: the rows below the block's edge become zeros (the first staged half alone has any).
#define FA_LOAD_HALF(t)                                                                                  \
  {                                                                                                      \
    const int t_ = (t);                                                                                  \
    if constexpr (PAGED) {                                                                               \
      const int prow = min(a.page_size, len - pw.slot * a.page_size);                                    \
      const uint32_t bytes = ((uint32_t)(prow - 1) * a.kv_ld + D) * esz;                                 \
      const size_t base = (size_t)pw.next * a.page_stride + kvoff;                                       \
      load_rows(sk, make_rsrc(reinterpret_cast<const T*>(a.k) + base, bytes), pw.off + (t_ & HALF));     \
      load_rows(sv, make_rsrc(reinterpret_cast<const T*>(a.v) + base, bytes), pw.off + (t_ & HALF));     \
      if (t_ & HALF) {                                                                                   \
        pw.off += DEC_ROWS;                                                                              \
        if (pw.off == a.page_size) {                                                                     \
          pw.off = 0;                                                                                    \
          ++pw.slot;                                                                                     \
        }                                                                                                \
        if (t_ + HALF < cend) pw.next = pw.id(a);                                                        \
      }                                                                                                  \
    } else {                                                                                             \
      load_rows(sk, krs, t_);                                                                            \
      load_rows(sv, vrs, t_);                                                                            \
    }                                                                                                    \
    if constexpr (WINDOW) {                                                                              \
      if (t_ < wedge) {                                                                                  \
        zero_below(sk, wedge - t_);                                                                      \
        zero_below(sv, wedge - t_);                                                                      \
      }                                                                                                  \
    }                                                                                                    \
  }
    FA_LOAD_HALF(h0)
    for (int t0 = h0; t0 < cend; t0 += HALF) {
      __syncthreads();   // (the previous half's reads are done)
      sk.store(tk);
      sv.store(tv);
      if (t0 + HALF < cend) FA_LOAD_HALF(t0 + HALF)
      __syncthreads();
      if (!wave_live) continue;
#pragma unroll
      for (int st = 0; st < HALF / 32; ++st) {
        const int kbase = t0 + 32 * st;
        if (kbase >= cend || (a.causal && kbase > pos_hi)) break;   // wave-uniform: no admissible key here or further on
        if constexpr (WINDOW) {
          if (kbase + 31 <= pos_lo - a.window) continue;   // wave-uniform: the 32 keys are below every window of the wave's rows
        }
        f32x16 s = zero16();
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) A::mma(s, A::row_frag<D>(tk, ra, 32 * st, kc), qf[kc]);
        if constexpr (SOFTCAP) {   // the cap, in front of the masks
#pragma unroll
          for (int i = 0; i < 16; ++i) s[i] = cap_score(s[i], k2, a.softcap);
        }
        if (kbase + 32 > c1 || (a.causal && kbase + 31 > pos_lo) || (WINDOW && kbase <= pos_hi - a.window)) {   // wave-uniform
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int key = kbase + acc_row(i, h);
            if (key >= c1 || (a.causal && key > qpos) || (WINDOW && key <= qpos - a.window)) s[i] = -INFINITY;
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
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {   // P at 16 significant bits (pack + pack_lo), as in decode_split_kernel
          const frag p_hi = A::pack(s, s2);
          const frag p_lo = A::pack_lo(s, s2, p_hi);
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) {
            const frag vt = A::tr_frag<D>(tv, ta, 32 * st + 16 * s2, dt);
            A::mma(acc_o[dt], vt, p_hi);
            A::mma(acc_o[dt], vt, p_lo);
          }
        }
      }
    }
#undef FA_LOAD_HALF
  }
  const float l_tot = xhalf_sum(l_run);
  if (!live) return;   // (no barrier follows)
  const size_t bhq = (size_t)b * a.H + hd;
  const bool final_row = a.nsplit == 1;   // final: out = O / l, lse = m * tau + ln l; a row without an admissible key: out = 0, lse = -inf
  const float inv = !final_row ? 1.0f : (l_tot > 0.f) ? 1.0f / l_tot : 0.f;
  const size_t pr = (bhq * a.nsplit + split) * a.Nq + qi;
  float* orow = final_row ? a.out + (size_t)b * a.q_bstride + (size_t)hd * a.q_hstride + (size_t)qi * a.q_ld : a.part_o + pr * D;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x4 val = {acc_o[dt][4 * g] * inv, acc_o[dt][4 * g + 1] * inv, acc_o[dt][4 * g + 2] * inv, acc_o[dt][4 * g + 3] * inv};
      *reinterpret_cast<f32x4*>(orow + 32 * dt + 8 * g + 4 * h) = val;
    }
  if (h != 0) return;
  if (!final_row) *reinterpret_cast<f32x2*>(a.part_ml + 2 * pr) = f32x2{m_run, l_tot};
  else if (a.lse) a.lse[bhq * a.Nq + qi] = (l_tot > 0.f) ? m_run * tau + __logf(l_tot) : -INFINITY;
}

// The combine kernel at 256 columns: decode_combine_kernel's body text (thread (g, j): columns 4g .. 4g+3 of the splits j, j + 4,
// ...; the four partial sums of a column group added in the order j = 0 .. 3), under FA_NO_PK_F32 like the kernels above.
// (RAGGED is never true: it makes the argument's type depend on a template parameter, for the reason decode_split_sink_kernel gives.)
template <bool RAGGED>
__global__ void FA_NO_PK_F32 __launch_bounds__(256) decode_combine_d256_kernel(DecodeArgsOf<RAGGED> a) {
  constexpr int D = D256;
  constexpr bool FP8 = false, LSINK = false;
#include "fa_decode_combine_body.h"
}

}  // namespace fa
