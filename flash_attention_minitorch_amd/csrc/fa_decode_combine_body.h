// The body of decode_combine_kernel and decode_combine_lsink_kernel (fa_decode.h), included INSIDE each: plain text, not a function,
// for the reason fa_decode_split_body.h gives (as text the existing kernel is the function it was).  In scope: D, RAGGED, FP8, LSINK
// and the kernel's argument a.
  static_assert(!LSINK || !FP8, "learned sink logits: no fp8 cache");
  constexpr int G = D / 4, S = 256 / G;
  __shared__ f32x4 red_o[256];
  __shared__ float red_m[256], red_l[256];
  const int tid = threadIdx.x, g = tid % G, j = tid / G;
  const int row = blockIdx.x % a.Nq, bh = blockIdx.x / a.Nq;
  if constexpr (RAGGED) {   // (workgroup-uniform: in front of the barriers)
    int s0, n0, sl, nl;
    seq_rows(a.cu, a.ntok, 0, s0, n0);
    seq_rows(a.cu, a.ntok, a.nseq - 1, sl, nl);
    if (row < s0 || row >= sl + nl) return;
  }
  const int b = bh / a.H, hd = bh - b * a.H;
  float tau8 = 0.f;
  if constexpr (FP8) tau8 = a.tau * scale_of(a.k_scale, hd / a.G);
#define FA_TAU (FP8 ? tau8 : a.tau)
  const float c = FA_TAU * LOG2E;
  const size_t p0 = (size_t)bh * a.nsplit * a.Nq + row;   // partial row of split s: p0 + s * Nq
  float m = -INFINITY;
  for (int s = j; s < a.nsplit; s += S) m = fmaxf(m, a.part_ml[2 * (p0 + (size_t)s * a.Nq)]);
  red_m[tid] = m;
  __syncthreads();
  float m_all = -INFINITY;
  for (int u = 0; u < S; ++u) m_all = fmaxf(m_all, red_m[u * G + g]);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float l = 0.f;
  if (m_all != -INFINITY) {
    for (int s = j; s < a.nsplit; s += S) {
      const size_t p = p0 + (size_t)s * a.Nq;
      const f32x2 ml = *reinterpret_cast<const f32x2*>(a.part_ml + 2 * p);
      if (ml[0] == -INFINITY) continue;
      const float wgt = __builtin_amdgcn_exp2f((ml[0] - m_all) * c);
      l += ml[1] * wgt;
      acc += *reinterpret_cast<const f32x4*>(a.part_o + p * D + 4 * g) * wgt;
    }
  }
  red_o[tid] = acc;
  red_l[tid] = l;
  __syncthreads();
  if (j != 0) return;
  for (int u = 1; u < S; ++u) {
    acc += red_o[u * G + g];
    l += red_l[u * G + g];
  }
  float inv = (l > 0.f) ? 1.0f / l : 0.f;
  if constexpr (FP8) inv *= scale_of(a.v_scale, hd / a.G);
  float lse_s = 0.f;
  if constexpr (LSINK) lsink_finish(m_all, l, FA_TAU, a.sink_logits[hd], inv, lse_s);   // (the sink column: once, behind the reduction)
  float* orow = a.out + (size_t)b * a.q_bstride + (size_t)hd * a.q_hstride + (size_t)row * a.q_ld;
  *reinterpret_cast<f32x4*>(orow + 4 * g) = acc * inv;
  if constexpr (LSINK) {
    if (g == 0 && a.lse) a.lse[(size_t)bh * a.Nq + row] = lse_s;
  } else {
    if (g == 0 && a.lse) a.lse[(size_t)bh * a.Nq + row] = (l > 0.f) ? m_all * FA_TAU + __logf(l) : -INFINITY;
  }
#undef FA_TAU
