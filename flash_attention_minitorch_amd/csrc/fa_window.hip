// C ABI of libflash_attn_mi355x_window.so (include/flash_attn_mi355x_window.h, _window_softcap.h): the sliding-window / attention-sink
// forward and backward on device pointers, with or without logit soft-capping.  Validation and dispatch for the kernels of
// fa_window.h; the row constants come from bwd_prep_kernel (fa_bwd_dkdv.h) and a grouped call's dK, dV from group_sum_kernel
// (fa_aux.h), as in fa_mi355x_bwd_gqa.  A capped call (softcap > 0) takes the same path with the cap builds of the three kernels
// and 1 for 1 / tau in the row constants; softcap = 0 is the uncapped call, launch for launch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <cmath>

#include "../../include/flash_attn_mi355x_window_softcap.h"
#define FA_WIN_SOFTCAP_KERNEL(stem) win_##stem##_softcap_kernel   // this library alone builds the cap kernels of fa_window.h
#include "fa_window.h"
#include "fa_bwd_dkdv.h"
#include "fa_aux.h"

namespace {

thread_local char g_err[512] = "";

int set_err(int code, const char* what, hipError_t e = hipSuccess) {
  if (e != hipSuccess)
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
  else
    snprintf(g_err, sizeof(g_err), "%s", what);
  return code;
}

constexpr int WS_VECS = 3;   // -L/tau, -delta, -L*log2(e): what bwd_prep_kernel writes (the third is unused here)
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline bool d_supported(int d) { return d == 32 || d == 64 || d == 128; }

struct Call {
  const void *q, *k, *v, *dout;
  float *out, *lse, *dq, *dk, *dv, *ws;
  int B, H, Hkv, N, d, layout, W, S, dtype;
  float scale, tau, softcap;   // softcap: 0 for none
  bool bwd;
  hipStream_t st;
  fa::Layout lay;
};

// The checks of both entry points, in one order, before any HIP call.  Completes the call: tau, W and S clamped to N, lay.
int validate(Call& c) {
  g_err[0] = 0;
  if (c.B <= 0 || c.H <= 0 || c.N <= 0 || c.d <= 0) return set_err(FA_ERR_BAD_ARG, "B, H, N and d must be positive");
  if (c.Hkv <= 0 || c.H % c.Hkv != 0) return set_err(FA_ERR_BAD_ARG, "Hkv must be positive and divide H");
  if (c.W < 1) return set_err(FA_ERR_BAD_ARG, "window must be at least 1");
  if (c.S < 0) return set_err(FA_ERR_BAD_ARG, "sink must not be negative");
  if (c.dtype != FA_DTYPE_F32 && c.dtype != FA_DTYPE_BF16) return set_err(FA_ERR_BAD_ARG, "unknown dtype");
  if (c.layout != FA_LAYOUT_BHND && c.layout != FA_LAYOUT_BNHD) return set_err(FA_ERR_BAD_ARG, "unknown layout");
  if (!d_supported(c.d)) return set_err(FA_ERR_BAD_ARG, "d must be 32, 64 or 128 (pad other head sizes with zero columns)");
  if (!c.q || !c.k || !c.v || !c.out || !c.lse || (c.bwd && (!c.dout || !c.dq || !c.dk || !c.dv || !c.ws)))
    return set_err(FA_ERR_BAD_ARG, "null pointer argument");
  if (c.scale != 0.f && (!(c.scale > 0.f) || !std::isfinite(c.scale)))
    return set_err(FA_ERR_BAD_ARG, "softmax_scale must be positive and finite (0: sqrt(1/d))");
  if (!(c.softcap >= 0.f) || !std::isfinite(c.softcap))
    return set_err(FA_ERR_BAD_ARG, "softcap must be finite and not negative (0: no soft-capping)");
  if ((long)c.N * 128 * 4 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "N too large: one (batch*head) matrix must stay under 2 GiB");
  if ((long)c.N * c.H * c.d * 4 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "one batch element must stay under 2 GiB");
  if ((long)c.B * c.H * ((c.N + 31) / 32) >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "too many workgroups for one launch");
  if (c.bwd && c.Hkv < c.H && (uintptr_t)c.ws % 256 != 0)
    return set_err(FA_ERR_BAD_ARG, "the workspace of a grouped backward must be 256-byte aligned");
  c.tau = c.scale > 0.f ? c.scale : sqrtf(1.0f / (float)c.d);
  c.W = std::min(c.W, c.N);   // W >= N or S >= N: every j <= i is admitted
  c.S = std::min(c.S, c.N);
  fa::Layout l{};   // no key mask, no dropout, no guard
  const bool rows_by_head = c.layout == FA_LAYOUT_BNHD;
  l.H = rows_by_head ? c.H : 1;
  l.ld = rows_by_head ? c.H * c.d : c.d;
  l.bstride = rows_by_head ? (long)c.N * c.H * c.d : (long)c.N * c.d;
  l.hstride = rows_by_head ? c.d : 0;
  l.mask_heads = 1;
  l.drop_scale = 1.0f;
  l.G = c.H / c.Hkv;
  if (l.G == 1) {
    l.kvH = l.H;
    l.ldk = l.ld;
  } else {
    l.kvH = rows_by_head ? c.Hkv : 1;
    l.ldk = rows_by_head ? c.Hkv * c.d : c.d;
  }
  c.lay = l;
  return FA_OK;
}

#define FA_WIN_LAUNCH(what, kern, grid, block, ...)                                       \
  do {                                                                                    \
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, c.st, __VA_ARGS__);              \
    const hipError_t e_ = hipGetLastError();                                              \
    if (e_ != hipSuccess) return set_err(FA_ERR_HIP, what " launch", e_);                 \
  } while (0)

// The per-(dtype, d) tile shapes are those of the phased kernels in fa_api.hip, in the builds that carry the split-operand path:
// forward key tile 64 (bf16) / 32 (fp32); dQ with 4 waves; dK/dV with 8 waves and 128-query slices for bf16 at d <= 64, 4 waves and
// 64-query slices at d = 128 (one wave per SIMD: the whole register file, no scratch), 4 waves and 32-query slices for fp32.
// CAP: the soft-capping builds, same shapes; the row constant is -lse (1 for 1 / tau), not -lse / tau.
template <typename T, int D, bool CAP>
int run(const Call& c) {
  constexpr bool BF = sizeof(T) == 2;
  constexpr int BN = BF ? 64 : 32, NWQ = 4, NW = (BF && D < 128) ? 8 : 4, QS = BF ? (D == 128 ? 64 : 128) : 32;
  const int BH = c.B * c.H, N = c.N;
  const T *q = (const T*)c.q, *k = (const T*)c.k, *v = (const T*)c.v;
  if (!c.bwd) {
    const int nqb = (N + 127) / 128;
    if constexpr (CAP)
      FA_WIN_LAUNCH("win_fwd_softcap_kernel", (fa::win_fwd_softcap_kernel<T, D, BN>), BH * nqb, 256, q, k, v, c.out, c.lse, N, nqb, BH,
                    c.lay, c.tau, c.W, c.S, c.softcap);
    else
      FA_WIN_LAUNCH("win_fwd_kernel", (fa::win_fwd_kernel<T, D, BN>), BH * nqb, 256, q, k, v, c.out, c.lse, N, nqb, BH, c.lay, c.tau,
                    c.W, c.S);
    return FA_OK;
  }
  const long rows = (long)BH * N;
  float *nlc = c.ws, *ndelta = c.ws + rows, *nl2 = c.ws + 2 * rows;
  float *dk = c.dk, *dv = c.dv;
  if (c.lay.G > 1) {   // per query head into the scratch behind the row constants
    dk = reinterpret_cast<float*>(reinterpret_cast<char*>(c.ws) + align256((size_t)WS_VECS * rows * sizeof(float)));
    dv = dk + (size_t)rows * D;
  }
  const T* dout = (const T*)c.dout;
  constexpr int RPB = 256 / (D / 8);
  FA_WIN_LAUNCH("bwd_prep_kernel", (fa::bwd_prep_kernel<T, D>), (int)((rows + RPB - 1) / RPB), 256, (const float*)c.out, dout,
                (const float*)c.lse, (const float*)nullptr, nlc, ndelta, nl2, rows, N, c.lay, fa::AUX_FA2, CAP ? 1.0f : 1.0f / c.tau);
  const int nkb = (N + NW * 32 - 1) / (NW * 32);
  if constexpr (CAP)
    FA_WIN_LAUNCH("win_dkdv_softcap_kernel", (fa::win_dkdv_softcap_kernel<T, D, NW, QS>), BH * nkb, NW * 64, q, k, v, dout,
                  (const float*)nlc, (const float*)ndelta, dk, dv, N, nkb, BH, c.lay, c.tau, c.W, c.S, c.softcap);
  else
    FA_WIN_LAUNCH("win_dkdv_kernel", (fa::win_dkdv_kernel<T, D, NW, QS>), BH * nkb, NW * 64, q, k, v, dout, (const float*)nlc,
                  (const float*)ndelta, dk, dv, N, nkb, BH, c.lay, c.tau, c.W, c.S);
  if (c.lay.G > 1)   // inner: 16-byte chunks between the heads of a group ([B][N][H][d]: d / 4; [B][H][N][d]: N * d / 4)
    FA_WIN_LAUNCH("group_sum_kernel", fa::group_sum_kernel, (int)((rows / c.lay.G * (D / 4) + 255) / 256), 256, (const float*)dk,
                  (const float*)dv, c.dk, c.dv, rows / c.lay.G * (D / 4),
                  c.layout == FA_LAYOUT_BNHD ? (long)(D / 4) : (long)N * (D / 4), c.lay.G);
  const int nqb = (N + 32 * NWQ - 1) / (32 * NWQ);
  if constexpr (CAP)
    FA_WIN_LAUNCH("win_dq_softcap_kernel", (fa::win_dq_softcap_kernel<T, D, NWQ>), BH * nqb, 64 * NWQ, q, k, v, dout,
                  (const float*)nlc, (const float*)ndelta, c.dq, N, nqb, BH, c.lay, c.tau, c.W, c.S, c.softcap);
  else
    FA_WIN_LAUNCH("win_dq_kernel", (fa::win_dq_kernel<T, D, NWQ>), BH * nqb, 64 * NWQ, q, k, v, dout, (const float*)nlc,
                  (const float*)ndelta, c.dq, N, nqb, BH, c.lay, c.tau, c.W, c.S);
  return FA_OK;
}

template <bool CAP>
int dispatch_cap(const Call& c) {
  if (c.dtype == FA_DTYPE_BF16) {
    if (c.d == 32) return run<fa::bf16_t, 32, CAP>(c);
    if (c.d == 64) return run<fa::bf16_t, 64, CAP>(c);
    return run<fa::bf16_t, 128, CAP>(c);
  }
  if (c.d == 32) return run<float, 32, CAP>(c);
  if (c.d == 64) return run<float, 64, CAP>(c);
  return run<float, 128, CAP>(c);
}

int dispatch(Call& c) {
  if (int rc = validate(c)) return rc;
  return c.softcap > 0.f ? dispatch_cap<true>(c) : dispatch_cap<false>(c);
}

// The four entry points fill one Call; the _window ones leave softcap at 0.
Call fwd_call(const void* q, const void* k, const void* v, float* out, float* lse, int B, int H, int Hkv, int N, int d, int layout,
              float softmax_scale, int window, float softcap, int sink, int dtype, void* stream) {
  Call c{};
  c.q = q; c.k = k; c.v = v; c.out = out; c.lse = lse;
  c.B = B; c.H = H; c.Hkv = Hkv; c.N = N; c.d = d; c.layout = layout; c.scale = softmax_scale; c.W = window; c.S = sink;
  c.softcap = softcap; c.dtype = dtype; c.st = (hipStream_t)stream; c.bwd = false;
  return c;
}

Call bwd_call(const void* q, const void* k, const void* v, const float* out, const void* out_grad, float* q_grad, float* k_grad,
              float* v_grad, const float* lse, void* workspace, int B, int H, int Hkv, int N, int d, int layout, float softmax_scale,
              int window, float softcap, int sink, int dtype, void* stream) {
  Call c = fwd_call(q, k, v, const_cast<float*>(out), const_cast<float*>(lse), B, H, Hkv, N, d, layout, softmax_scale, window, softcap,
                    sink, dtype, stream);
  c.dout = out_grad; c.dq = q_grad; c.dk = k_grad; c.dv = v_grad; c.ws = (float*)workspace; c.bwd = true;
  return c;
}

}  // namespace

extern "C" {

const char* fa_mi355x_window_last_error(void) { return g_err; }

int fa_mi355x_fwd_window(const void* q, const void* k, const void* v, float* out, float* lse, int B, int H, int Hkv, int N, int d,
                         int layout, float softmax_scale, int window, int sink, int dtype, void* stream) {
  Call c = fwd_call(q, k, v, out, lse, B, H, Hkv, N, d, layout, softmax_scale, window, 0.f, sink, dtype, stream);
  return dispatch(c);
}

int fa_mi355x_fwd_window_softcap(const void* q, const void* k, const void* v, float* out, float* lse, int B, int H, int Hkv, int N,
                                 int d, int layout, float softmax_scale, int window, float softcap, int sink, int dtype, void* stream) {
  Call c = fwd_call(q, k, v, out, lse, B, H, Hkv, N, d, layout, softmax_scale, window, softcap, sink, dtype, stream);
  return dispatch(c);
}

size_t fa_mi355x_bwd_window_workspace_bytes(int B, int H, int Hkv, int N, int d) {
  if (B <= 0 || H <= 0 || Hkv <= 0 || H % Hkv != 0 || N <= 0 || d <= 0) return 0;
  const size_t vecs = (size_t)WS_VECS * B * H * N * sizeof(float);
  if (Hkv == H) return vecs;
  return align256(vecs) + (size_t)2 * B * H * N * d * sizeof(float);
}

int fa_mi355x_bwd_window(const void* q, const void* k, const void* v, const float* out, const void* out_grad, float* q_grad,
                         float* k_grad, float* v_grad, const float* lse, void* workspace, int B, int H, int Hkv, int N, int d,
                         int layout, float softmax_scale, int window, int sink, int dtype, void* stream) {
  Call c = bwd_call(q, k, v, out, out_grad, q_grad, k_grad, v_grad, lse, workspace, B, H, Hkv, N, d, layout, softmax_scale, window,
                    0.f, sink, dtype, stream);
  return dispatch(c);
}

int fa_mi355x_bwd_window_softcap(const void* q, const void* k, const void* v, const float* out, const void* out_grad, float* q_grad,
                                 float* k_grad, float* v_grad, const float* lse, void* workspace, int B, int H, int Hkv, int N, int d,
                                 int layout, float softmax_scale, int window, float softcap, int sink, int dtype, void* stream) {
  Call c = bwd_call(q, k, v, out, out_grad, q_grad, k_grad, v_grad, lse, workspace, B, H, Hkv, N, d, layout, softmax_scale, window,
                    softcap, sink, dtype, stream);
  return dispatch(c);
}

}  // extern "C"
