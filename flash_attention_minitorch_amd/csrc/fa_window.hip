// C ABI of libflash_attn_mi355x_window.so (include/flash_attn_mi355x_window.h, _window_softcap.h): the sliding-window / attention-sink
// forward and backward on device pointers, with or without logit soft-capping.  This library's checks and the launches of the
// kernels of fa_window.h; what the training-side libraries share is in fa_side_host.h: the common checks, the layout, the tile
// shapes, the dispatch, and the backward's row constants (bwd_prep_kernel) and group sum (group_sum_kernel), as in fa_mi355x_bwd_gqa.
// A capped call (softcap > 0) takes the same path with the cap builds of the three kernels and 1 for 1 / tau in the row constants;
// softcap = 0 is the uncapped call, launch for launch.
#include "../../include/flash_attn_mi355x_window_softcap.h"
#define FA_WIN_SOFTCAP_KERNEL(stem) win_##stem##_softcap_kernel   // this library alone builds the cap kernels of fa_window.h
#include "fa_window.h"
#include "fa_side_host.h"

namespace {

struct Call : SideCall {
  int B, N, layout, W, S;
  float softcap;   // 0 for none
};

// The checks of both entry points, in one order, before any HIP call.  Completes the call: tau, W and S clamped to N, lay.
int validate(Call& c) {
  g_err[0] = 0;
  if (c.B <= 0 || c.H <= 0 || c.N <= 0 || c.d <= 0) return set_err(FA_ERR_BAD_ARG, "B, H, N and d must be positive");
  if (int rc = check_heads(c)) return rc;
  if (c.W < 1) return set_err(FA_ERR_BAD_ARG, "window must be at least 1");
  if (c.S < 0) return set_err(FA_ERR_BAD_ARG, "sink must not be negative");
  if (int rc = check_dtype(c)) return rc;
  if (c.layout != FA_LAYOUT_BHND && c.layout != FA_LAYOUT_BNHD) return set_err(FA_ERR_BAD_ARG, "unknown layout");
  if (int rc = check_d(c)) return rc;
  if (!c.q || !c.k || !c.v || !c.out || !c.lse || (c.bwd && (!c.dout || !c.dq || !c.dk || !c.dv || !c.ws)))
    return set_err(FA_ERR_BAD_ARG, "null pointer argument");
  if (int rc = check_scale(c)) return rc;
  if (!(c.softcap >= 0.f) || !std::isfinite(c.softcap))
    return set_err(FA_ERR_BAD_ARG, "softcap must be finite and not negative (0: no soft-capping)");
  if ((long)c.N * 128 * 4 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "N too large: one (batch*head) matrix must stay under 2 GiB");
  if ((long)c.N * c.H * c.d * 4 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "one batch element must stay under 2 GiB");
  if ((long)c.B * c.H * ((c.N + 31) / 32) >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "too many workgroups for one launch");
  if (c.bwd && c.Hkv < c.H)
    if (int rc = check_ws_aligned(c, "the workspace of a grouped backward must be 256-byte aligned")) return rc;
  c.tau = tau_of(c);
  c.W = std::min(c.W, c.N);   // W >= N or S >= N: every j <= i is admitted
  c.S = std::min(c.S, c.N);
  c.lay = side_layout(c.layout == FA_LAYOUT_BNHD, c.N, c.H, c.Hkv, c.d);
  return FA_OK;
}

// CAP: the soft-capping builds, in the tile shapes of the uncapped ones (SideTiles); the row constant is -lse (1 for 1 / tau), not
// -lse / tau.
template <typename T, int D, bool CAP>
int run(const Call& c) {
  using Ti = SideTiles<T, D>;
  constexpr int BN = Ti::BN, NWQ = Ti::NWQ, NW = Ti::NW, QS = Ti::QS;
  const int BH = c.B * c.H, N = c.N;
  const T *q = (const T*)c.q, *k = (const T*)c.k, *v = (const T*)c.v;
  if (!c.bwd) {
    const int nqb = (N + 127) / 128;
    if constexpr (CAP)
      FA_SIDE_LAUNCH("win_fwd_softcap_kernel", (fa::win_fwd_softcap_kernel<T, D, BN>), BH * nqb, 256, q, k, v, c.out, c.lse, N, nqb, BH,
                     c.lay, c.tau, c.W, c.S, c.softcap);
    else
      FA_SIDE_LAUNCH("win_fwd_kernel", (fa::win_fwd_kernel<T, D, BN>), BH * nqb, 256, q, k, v, c.out, c.lse, N, nqb, BH, c.lay, c.tau,
                     c.W, c.S);
    return FA_OK;
  }
  const long rows = (long)BH * N;
  const BwdScratch s(c, c.ws, rows, rows);
  const T* dout = (const T*)c.dout;
  if (int rc = launch_bwd_prep<T, D>(c, s, rows, N, CAP ? 1.0f : 1.0f / c.tau)) return rc;
  const int nkb = (N + NW * 32 - 1) / (NW * 32);
  if constexpr (CAP)
    FA_SIDE_LAUNCH("win_dkdv_softcap_kernel", (fa::win_dkdv_softcap_kernel<T, D, NW, QS>), BH * nkb, NW * 64, q, k, v, dout,
                   (const float*)s.nlc, (const float*)s.ndelta, s.dk, s.dv, N, nkb, BH, c.lay, c.tau, c.W, c.S, c.softcap);
  else
    FA_SIDE_LAUNCH("win_dkdv_kernel", (fa::win_dkdv_kernel<T, D, NW, QS>), BH * nkb, NW * 64, q, k, v, dout, (const float*)s.nlc,
                   (const float*)s.ndelta, s.dk, s.dv, N, nkb, BH, c.lay, c.tau, c.W, c.S);
  if (c.lay.G > 1)
    if (int rc = launch_group_sum(c, s, rows, c.layout == FA_LAYOUT_BNHD ? (long)(D / 4) : (long)N * (D / 4))) return rc;
  const int nqb = (N + 32 * NWQ - 1) / (32 * NWQ);
  if constexpr (CAP)
    FA_SIDE_LAUNCH("win_dq_softcap_kernel", (fa::win_dq_softcap_kernel<T, D, NWQ>), BH * nqb, 64 * NWQ, q, k, v, dout,
                   (const float*)s.nlc, (const float*)s.ndelta, c.dq, N, nqb, BH, c.lay, c.tau, c.W, c.S, c.softcap);
  else
    FA_SIDE_LAUNCH("win_dq_kernel", (fa::win_dq_kernel<T, D, NWQ>), BH * nqb, 64 * NWQ, q, k, v, dout, (const float*)s.nlc,
                   (const float*)s.ndelta, c.dq, N, nqb, BH, c.lay, c.tau, c.W, c.S);
  return FA_OK;
}

int dispatch(Call& c) {
  if (int rc = validate(c)) return rc;
  return side_dispatch(c, [&](auto t, auto d) {
    using T = typename decltype(t)::type;
    return c.softcap > 0.f ? run<T, decltype(d)::value, true>(c) : run<T, decltype(d)::value, false>(c);
  });
}

// The four entry points come here; the _window ones with softcap = 0.
int fwd(const void* q, const void* k, const void* v, float* out, float* lse, int B, int H, int Hkv, int N, int d, int layout,
        float softmax_scale, int window, float softcap, int sink, int dtype, void* stream) {
  Call c{side_call(q, k, v, out, lse, nullptr, H, Hkv, d, softmax_scale, dtype, stream), B, N, layout, window, sink, softcap};
  return dispatch(c);
}

int bwd(const void* q, const void* k, const void* v, const float* out, const void* out_grad, float* q_grad, float* k_grad,
        float* v_grad, const float* lse, void* workspace, int B, int H, int Hkv, int N, int d, int layout, float softmax_scale,
        int window, float softcap, int sink, int dtype, void* stream) {
  Call c{side_call(q, k, v, out, lse, workspace, H, Hkv, d, softmax_scale, dtype, stream), B, N, layout, window, sink, softcap};
  set_bwd(c, out_grad, q_grad, k_grad, v_grad);
  return dispatch(c);
}

}  // namespace

extern "C" {

const char* fa_mi355x_window_last_error(void) { return g_err; }

int fa_mi355x_fwd_window(const void* q, const void* k, const void* v, float* out, float* lse, int B, int H, int Hkv, int N, int d,
                         int layout, float softmax_scale, int window, int sink, int dtype, void* stream) {
  return fwd(q, k, v, out, lse, B, H, Hkv, N, d, layout, softmax_scale, window, 0.f, sink, dtype, stream);
}

int fa_mi355x_fwd_window_softcap(const void* q, const void* k, const void* v, float* out, float* lse, int B, int H, int Hkv, int N,
                                 int d, int layout, float softmax_scale, int window, float softcap, int sink, int dtype, void* stream) {
  return fwd(q, k, v, out, lse, B, H, Hkv, N, d, layout, softmax_scale, window, softcap, sink, dtype, stream);
}

size_t fa_mi355x_bwd_window_workspace_bytes(int B, int H, int Hkv, int N, int d) {
  if (B <= 0 || H <= 0 || Hkv <= 0 || H % Hkv != 0 || N <= 0 || d <= 0) return 0;
  return bwd_scratch_bytes((size_t)B * H * N, (size_t)B * H * N, d, Hkv < H);
}

int fa_mi355x_bwd_window(const void* q, const void* k, const void* v, const float* out, const void* out_grad, float* q_grad,
                         float* k_grad, float* v_grad, const float* lse, void* workspace, int B, int H, int Hkv, int N, int d,
                         int layout, float softmax_scale, int window, int sink, int dtype, void* stream) {
  return bwd(q, k, v, out, out_grad, q_grad, k_grad, v_grad, lse, workspace, B, H, Hkv, N, d, layout, softmax_scale, window, 0.f, sink,
             dtype, stream);
}

int fa_mi355x_bwd_window_softcap(const void* q, const void* k, const void* v, const float* out, const void* out_grad, float* q_grad,
                                 float* k_grad, float* v_grad, const float* lse, void* workspace, int B, int H, int Hkv, int N, int d,
                                 int layout, float softmax_scale, int window, float softcap, int sink, int dtype, void* stream) {
  return bwd(q, k, v, out, out_grad, q_grad, k_grad, v_grad, lse, workspace, B, H, Hkv, N, d, layout, softmax_scale, window, softcap,
             sink, dtype, stream);
}

}  // extern "C"
