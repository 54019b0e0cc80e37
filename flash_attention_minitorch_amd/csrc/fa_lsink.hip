// C ABI of libflash_attn_mi355x_lsink.so (include/flash_attn_mi355x_lsink.h): the training side of learned attention-sink logits.
// The forward is the lsink build of fa_window.h's forward kernel text (this library alone defines FA_WIN_LSINK_KERNEL); the
// backward for q, k and v is the window library's, on this forward's out and lse; the gradient of the logits is the two kernels
// below.  The checks, the layout, the tile shapes and the dispatch are fa_side_host.h's.
#include "../../include/flash_attn_mi355x_lsink.h"
#define FA_WIN_LSINK_KERNEL(stem) win_lsink_##stem##_kernel   // this library alone builds the lsink forward of fa_window.h
#include "fa_window.h"
#include "fa_side_host.h"

namespace fa {

// d a_h = - sum_{b,i} e^(a_h - lse_bhi) delta_bhi, delta = rowsum(dO o out).  Stage one: workgroup (h, s) = blockIdx.x takes the rows
// s * SLICE .. s * SLICE + SLICE - 1 of the B * N rows of head h (row r = b * N + i).  D / 8 threads share a row, eight columns each:
// two 16-byte loads of out (fp32) and one (bf16) or two (fp32) of out_grad; a thread adds its rows' weighted products in row order,
// the 256 thread sums meet in LDS and thread 0 adds them in thread order: ONE partial per workgroup, a fixed order, no atomics.
constexpr int LSINK_SLICE = FA_LSINK_SLICE_ROWS;

template <typename T, int D>
__global__ void __launch_bounds__(256) sink_grad_partial_kernel(const float* __restrict__ out, const T* __restrict__ dout,
                                                                const float* __restrict__ lse, const float* __restrict__ sink_logits,
                                                                float* __restrict__ partial, int B, int H, int N, int nslice, int bnhd) {
  constexpr int TPR = D / 8, RPP = 256 / TPR;   // threads per row, rows per pass
  static_assert(LSINK_SLICE % RPP == 0, "a slice is a whole number of passes");
  __shared__ float red[256];
  const int tid = threadIdx.x, col = (tid % TPR) * 8, sub = tid / TPR;
  const int h = blockIdx.x / nslice, s = blockIdx.x - h * nslice;
  const long rows = (long)B * N, r0 = (long)s * LSINK_SLICE;
  const float a2 = sink_logits[h] * LOG2E;
  float acc = 0.f;
  for (int p = 0; p < LSINK_SLICE / RPP; ++p) {
    const long r = r0 + (long)p * RPP + sub;
    if (r >= rows) break;   // (rows ascend with p: nothing further on either)
    const long b = r / N, i = r - b * N;
    const size_t row = bnhd ? ((size_t)r * H + h) : (((size_t)b * H + h) * N + i);   // the row's index among rows of D elements
    const float* o = out + row * D + col;
    const f32x4 o0 = *reinterpret_cast<const f32x4*>(o), o1 = *reinterpret_cast<const f32x4*>(o + 4);
    float g[8];
    if constexpr (sizeof(T) == 2) {
      const bf16x8 gv = *reinterpret_cast<const bf16x8*>(dout + row * D + col);
#pragma unroll
      for (int c = 0; c < 8; ++c) g[c] = (float)gv[c];
    } else {
      const f32x4 g0 = *reinterpret_cast<const f32x4*>(dout + row * D + col), g1 = *reinterpret_cast<const f32x4*>(dout + row * D + col + 4);
#pragma unroll
      for (int c = 0; c < 4; ++c) g[c] = g0[c], g[4 + c] = g1[c];
    }
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) dot += g[c] * o0[c];
#pragma unroll
    for (int c = 0; c < 4; ++c) dot += g[4 + c] * o1[c];
    const float w = __builtin_amdgcn_exp2f(__builtin_fmaf(-lse[((size_t)b * H + h) * N + i], LOG2E, a2));   // e^(a - lse) <= 1
    acc += w * dot;
  }
  red[tid] = acc;
  __syncthreads();
  if (tid != 0) return;
  float sum = 0.f;
  for (int t = 0; t < 256; ++t) sum += red[t];
  partial[(size_t)h * nslice + s] = -sum;
}

// Stage two: thread h adds its head's partials in slice order.
__global__ void __launch_bounds__(256) sink_grad_sum_kernel(const float* __restrict__ partial, float* __restrict__ sink_grad, int H,
                                                            int nslice) {
  const int h = blockIdx.x * 256 + threadIdx.x;
  if (h >= H) return;
  float sum = 0.f;
  for (int s = 0; s < nslice; ++s) sum += partial[(size_t)h * nslice + s];
  sink_grad[h] = sum;
}

}  // namespace fa

namespace {

struct Call : SideCall {
  int B, N, layout, W;
  const float* sink_logits;
};

long grad_slices(int B, int N) { return ((long)B * N + fa::LSINK_SLICE - 1) / fa::LSINK_SLICE; }

// The forward's checks, in one order, before any HIP call (the window library's, with the logits in the pointer check).
int validate(Call& c) {
  g_err[0] = 0;
  if (c.B <= 0 || c.H <= 0 || c.N <= 0 || c.d <= 0) return set_err(FA_ERR_BAD_ARG, "B, H, N and d must be positive");
  if (int rc = check_heads(c)) return rc;
  if (c.W < 1) return set_err(FA_ERR_BAD_ARG, "window must be at least 1 (a call without a window passes window = N)");
  if (int rc = check_dtype(c)) return rc;
  if (c.layout != FA_LAYOUT_BHND && c.layout != FA_LAYOUT_BNHD) return set_err(FA_ERR_BAD_ARG, "unknown layout");
  if (int rc = check_d(c)) return rc;
  if (!c.q || !c.k || !c.v || !c.out || !c.lse) return set_err(FA_ERR_BAD_ARG, "null pointer argument");
  if (!c.sink_logits) return set_err(FA_ERR_BAD_ARG, "null sink_logits: fa_mi355x_fwd_window is the call without the logits");
  if (int rc = check_scale(c)) return rc;
  if ((long)c.N * 128 * 4 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "N too large: one (batch*head) matrix must stay under 2 GiB");
  if ((long)c.N * c.H * c.d * 4 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "one batch element must stay under 2 GiB");
  if ((long)c.B * c.H * ((c.N + 31) / 32) >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "too many workgroups for one launch");
  c.tau = tau_of(c);
  c.W = std::min(c.W, c.N);
  c.lay = side_layout(c.layout == FA_LAYOUT_BNHD, c.N, c.H, c.Hkv, c.d);
  return FA_OK;
}

template <typename T, int D> int run_fwd(const Call& c) {
  constexpr int BN = SideTiles<T, D>::BN;
  const int BH = c.B * c.H, nqb = (c.N + 127) / 128;
  FA_SIDE_LAUNCH("win_lsink_fwd_kernel", (fa::win_lsink_fwd_kernel<T, D, BN>), BH * nqb, 256, (const T*)c.q, (const T*)c.k, (const T*)c.v,
                 c.out, c.lse, c.N, nqb, BH, c.lay, c.tau, c.W, 0, c.sink_logits, c.H);
  return FA_OK;
}

template <typename T, int D> int run_grad(const Call& c, float* sink_grad) {
  const int ns = (int)grad_slices(c.B, c.N);
  float* partial = (float*)c.ws;
  FA_SIDE_LAUNCH("sink_grad_partial_kernel", (fa::sink_grad_partial_kernel<T, D>), c.H * ns, 256, (const float*)c.out, (const T*)c.dout,
                 (const float*)c.lse, c.sink_logits, partial, c.B, c.H, c.N, ns, c.layout == FA_LAYOUT_BNHD ? 1 : 0);
  FA_SIDE_LAUNCH("sink_grad_sum_kernel", fa::sink_grad_sum_kernel, (c.H + 255) / 256, 256, (const float*)partial, sink_grad, c.H, ns);
  return FA_OK;
}

}  // namespace

extern "C" {

const char* fa_mi355x_lsink_last_error(void) { return g_err; }

int fa_mi355x_fwd_window_lsink(const void* q, const void* k, const void* v, float* out, float* lse, const float* sink_logits, int B, int H,
                               int Hkv, int N, int d, int layout, float softmax_scale, int window, int dtype, void* stream) {
  Call c{side_call(q, k, v, out, lse, nullptr, H, Hkv, d, softmax_scale, dtype, stream), B, N, layout, window, sink_logits};
  if (int rc = validate(c)) return rc;
  return side_dispatch(c, [&](auto t, auto dd) { return run_fwd<typename decltype(t)::type, decltype(dd)::value>(c); });
}

size_t fa_mi355x_sink_logits_grad_workspace_bytes(int B, int H, int N, int d) {
  if (B <= 0 || H <= 0 || N <= 0 || d <= 0) return 0;
  return (size_t)H * (size_t)grad_slices(B, N) * sizeof(float);
}

int fa_mi355x_sink_logits_grad(const float* out, const void* out_grad, const float* lse, const float* sink_logits, float* sink_grad,
                               void* workspace, int B, int H, int N, int d, int layout, int dtype, void* stream) {
  Call c{side_call(nullptr, nullptr, nullptr, out, lse, workspace, H, H, d, 0.f, dtype, stream), B, N, layout, 1, sink_logits};
  c.dout = out_grad;
  g_err[0] = 0;
  if (B <= 0 || H <= 0 || N <= 0 || d <= 0) return set_err(FA_ERR_BAD_ARG, "B, H, N and d must be positive");
  if (int rc = check_dtype(c)) return rc;
  if (layout != FA_LAYOUT_BHND && layout != FA_LAYOUT_BNHD) return set_err(FA_ERR_BAD_ARG, "unknown layout");
  if (int rc = check_d(c)) return rc;
  if (!out || !out_grad || !lse || !sink_grad || !workspace) return set_err(FA_ERR_BAD_ARG, "null pointer argument");
  if (!sink_logits) return set_err(FA_ERR_BAD_ARG, "null sink_logits");
  if (((uintptr_t)out | (uintptr_t)out_grad) % 16 != 0) return set_err(FA_ERR_BAD_ARG, "out and out_grad must be 16-byte aligned");
  if ((long)H * grad_slices(B, N) >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "too many workgroups for one launch");
  return side_dispatch(c, [&](auto t, auto dd) { return run_grad<typename decltype(t)::type, decltype(dd)::value>(c, sink_grad); });
}

}  // extern "C"
