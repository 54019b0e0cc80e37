// C ABI of libflash_attn_mi355x_varlen.so (include/flash_attn_mi355x_varlen.h): causal attention, windowed or not, forward and
// backward, on a packed batch of sequences of different lengths, and the rotary embedding that restarts at every sequence.
// Validation and dispatch for the kernels of fa_varlen.h; the row constants come from bwd_prep_kernel (fa_bwd_dkdv.h) and a grouped
// call's dK, dV from group_sum_kernel (fa_aux.h), both run over all T rows as one sequence, as fa_window.hip runs them.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <cmath>

#include "../../include/flash_attn_mi355x_varlen.h"
#include "fa_varlen.h"
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
inline long map_cap(int T, int nseq, int bs) { return (long)T / bs + nseq; }
inline size_t map_bytes(int T, int nseq) { return align256(sizeof(int4) * (size_t)map_cap(T, nseq, fa::VARLEN_QBLOCK)); }
inline bool sizes_ok(int nseq, int T, int H, int Hkv, int d) { return nseq >= 1 && T > 0 && H > 0 && d > 0 && Hkv > 0 && H % Hkv == 0; }

struct Call {
  const void *q, *k, *v, *dout;
  float *out, *lse, *dq, *dk, *dv;
  const int* cu;
  char* ws;
  int nseq, T, H, Hkv, d, W, S, dtype;
  float scale, tau;
  bool bwd;
  hipStream_t st;
  fa::Layout lay;
};

// The checks of both entry points, in one order, before any HIP call.  Completes the call: tau, W (no window: every j <= i), lay.
int validate(Call& c) {
  g_err[0] = 0;
  if (c.nseq < 1 || c.T <= 0 || c.H <= 0 || c.d <= 0) return set_err(FA_ERR_BAD_ARG, "nseq, T, H and d must be positive");
  if (c.Hkv <= 0 || c.H % c.Hkv != 0) return set_err(FA_ERR_BAD_ARG, "Hkv must be positive and divide H");
  if (c.W < 0) return set_err(FA_ERR_BAD_ARG, "window must not be negative (0: no window)");
  if (c.S < 0) return set_err(FA_ERR_BAD_ARG, "sink must not be negative");
  if (c.S > 0 && c.W == 0) return set_err(FA_ERR_BAD_ARG, "sink tokens need a window");
  if (c.dtype != FA_DTYPE_F32 && c.dtype != FA_DTYPE_BF16) return set_err(FA_ERR_BAD_ARG, "unknown dtype");
  if (!d_supported(c.d)) return set_err(FA_ERR_BAD_ARG, "d must be 32, 64 or 128 (pad other head sizes with zero columns)");
  if (!c.q || !c.k || !c.v || !c.out || !c.lse || !c.cu || !c.ws || (c.bwd && (!c.dout || !c.dq || !c.dk || !c.dv)))
    return set_err(FA_ERR_BAD_ARG, "null pointer argument");
  if (c.scale != 0.f && (!(c.scale > 0.f) || !std::isfinite(c.scale)))
    return set_err(FA_ERR_BAD_ARG, "softmax_scale must be positive and finite (0: sqrt(1/d))");
  // (T bounds every n_b: what holds for T holds for every sequence's buffer resource)
  if ((long)c.T * 128 * 4 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "T too large: one head's rows must stay under 2 GiB");
  if ((long)c.T * c.H * c.d * 4 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "the packed batch must stay under 2 GiB");
  if ((long)c.H * map_cap(c.T, c.nseq, fa::VARLEN_QBLOCK) >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "too many workgroups for one launch");
  if ((uintptr_t)c.ws % 256 != 0) return set_err(FA_ERR_BAD_ARG, "the workspace must be 256-byte aligned");
  c.tau = c.scale > 0.f ? c.scale : sqrtf(1.0f / (float)c.d);
  if (c.W == 0) c.W = INT_MAX;   // (the kernels clamp W and S to the sequence's length)
  fa::Layout l{};   // [1][T][H][d]: no key mask, no dropout, no guard
  l.H = c.H;
  l.ld = c.H * c.d;
  l.bstride = (long)c.T * c.H * c.d;
  l.hstride = c.d;
  l.mask_heads = 1;
  l.drop_scale = 1.0f;
  l.G = c.H / c.Hkv;
  l.kvH = c.Hkv;
  l.ldk = c.Hkv * c.d;
  c.lay = l;
  return FA_OK;
}

#define FA_VARLEN_LAUNCH(what, kern, grid, block, ...)                                    \
  do {                                                                                    \
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, c.st, __VA_ARGS__);              \
    const hipError_t e_ = hipGetLastError();                                              \
    if (e_ != hipSuccess) return set_err(FA_ERR_HIP, what " launch", e_);                 \
  } while (0)

// The tile shapes are those of fa_window.hip's run.  The workspace: the query-block map, (backward) the key-block map, the row
// constants, (grouped) the per-query-head dK and dV.
template <typename T, int D>
int run(const Call& c) {
  constexpr bool BF = sizeof(T) == 2;
  constexpr int BN = BF ? 64 : 32, NWQ = 4, NW = (BF && D < 128) ? 8 : 4, QS = BF ? (D == 128 ? 64 : 128) : 32, BK = NW * 32;
  static_assert(32 * NWQ == fa::VARLEN_QBLOCK, "the forward and dQ share one map");
  const int H = c.H, Tn = c.T;
  const T *q = (const T*)c.q, *k = (const T*)c.k, *v = (const T*)c.v;
  int4* map_q = reinterpret_cast<int4*>(c.ws);
  const int cap_q = (int)map_cap(Tn, c.nseq, fa::VARLEN_QBLOCK);
  fa::VarlenFill fill{};
  fill.H = H;
  if (!c.bwd) {
    fill.mat[0] = c.out;
    fill.ld[0] = c.lay.ld;
    fill.rowc = c.lse;
    FA_VARLEN_LAUNCH("varlen_schedule_kernel", fa::varlen_schedule_kernel, 1 + fa::VARLEN_FILL_BLOCKS, 256, c.cu, c.nseq, Tn, map_q,
                     cap_q, (int4*)nullptr, 0, 0, fill);
    FA_VARLEN_LAUNCH("varlen_fwd_kernel", (fa::varlen_fwd_kernel<T, D, BN>), H * cap_q, 256, q, k, v, c.out, c.lse,
                     (const int4*)map_q, Tn, cap_q, H, c.lay, c.tau, c.W, c.S);
    return FA_OK;
  }
  const size_t mb = map_bytes(Tn, c.nseq);
  int4* map_k = reinterpret_cast<int4*>(c.ws + mb);
  const int cap_k = (int)map_cap(Tn, c.nseq, BK);
  const long rows = (long)H * Tn;
  float *nlc = reinterpret_cast<float*>(c.ws + 2 * mb), *ndelta = nlc + rows, *nl2 = nlc + 2 * rows;
  float *dk = c.dk, *dv = c.dv;
  if (c.lay.G > 1) {   // per query head into the scratch behind the row constants
    dk = reinterpret_cast<float*>(c.ws + 2 * mb + align256((size_t)WS_VECS * rows * sizeof(float)));
    dv = dk + (size_t)rows * D;
  }
  // (the group sum reads all T rows of the per-query-head dK, dV: their unowned rows are zeroed, and its sums are then zeros)
  fill.mat[0] = c.dq;
  fill.mat[1] = dk;
  fill.mat[2] = dv;
  fill.ld[0] = fill.ld[1] = fill.ld[2] = c.lay.ld;
  FA_VARLEN_LAUNCH("varlen_schedule_kernel", fa::varlen_schedule_kernel, 1 + fa::VARLEN_FILL_BLOCKS, 256, c.cu, c.nseq, Tn, map_q, cap_q,
                   map_k, BK, cap_k, fill);
  const T* dout = (const T*)c.dout;
  constexpr int RPB = 256 / (D / 8);
  FA_VARLEN_LAUNCH("bwd_prep_kernel", (fa::bwd_prep_kernel<T, D>), (int)((rows + RPB - 1) / RPB), 256, (const float*)c.out, dout,
                   (const float*)c.lse, (const float*)nullptr, nlc, ndelta, nl2, rows, Tn, c.lay, fa::AUX_FA2, 1.0f / c.tau);
  FA_VARLEN_LAUNCH("varlen_dkdv_kernel", (fa::varlen_dkdv_kernel<T, D, NW, QS>), H * cap_k, NW * 64, q, k, v, dout, (const float*)nlc,
                   (const float*)ndelta, dk, dv, (const int4*)map_k, Tn, cap_k, H, c.lay, c.tau, c.W, c.S);
  if (c.lay.G > 1)
    FA_VARLEN_LAUNCH("group_sum_kernel", fa::group_sum_kernel, (int)((rows / c.lay.G * (D / 4) + 255) / 256), 256, (const float*)dk,
                     (const float*)dv, c.dk, c.dv, rows / c.lay.G * (D / 4), (long)(D / 4), c.lay.G);
  FA_VARLEN_LAUNCH("varlen_dq_kernel", (fa::varlen_dq_kernel<T, D, NWQ>), H * cap_q, 64 * NWQ, q, k, v, dout, (const float*)nlc,
                   (const float*)ndelta, c.dq, (const int4*)map_q, Tn, cap_q, H, c.lay, c.tau, c.W, c.S);
  return FA_OK;
}

int dispatch(Call& c) {
  if (int rc = validate(c)) return rc;
  if (c.dtype == FA_DTYPE_BF16) {
    if (c.d == 32) return run<fa::bf16_t, 32>(c);
    if (c.d == 64) return run<fa::bf16_t, 64>(c);
    return run<fa::bf16_t, 128>(c);
  }
  if (c.d == 32) return run<float, 32>(c);
  if (c.d == 64) return run<float, 64>(c);
  return run<float, 128>(c);
}

template <typename T, int E> int launch_rope(fa::RopeVarlenArgs a, bool il, hipStream_t st) {
  a.cpr = a.d / E;
  a.lanes *= a.cpr;   // (rows on entry)
  const long grid = (a.lanes + 255) / 256;
  if (il) hipLaunchKernelGGL((fa::rope_varlen_kernel<T, E, true>), dim3((unsigned)grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((fa::rope_varlen_kernel<T, E, false>), dim3((unsigned)grid), dim3(256), 0, st, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? FA_OK : set_err(FA_ERR_HIP, "rope_varlen_kernel launch", e);
}

}  // namespace

extern "C" {

const char* fa_mi355x_varlen_last_error(void) { return g_err; }

size_t fa_mi355x_fwd_varlen_workspace_bytes(int nseq, int T, int H, int Hkv, int d) {
  if (!sizes_ok(nseq, T, H, Hkv, d)) return 0;
  return map_bytes(T, nseq);
}

size_t fa_mi355x_bwd_varlen_workspace_bytes(int nseq, int T, int H, int Hkv, int d) {
  if (!sizes_ok(nseq, T, H, Hkv, d)) return 0;
  const long double est = 2.0L * H * T * d * 4 + 3.0L * H * T * 4 + 32.0L * ((long double)T + nseq) + 1024;
  if (est >= 4.0e18L) return 0;   // (past 2^62)
  const size_t vecs = (size_t)WS_VECS * H * T * sizeof(float);
  const size_t maps = 2 * map_bytes(T, nseq);
  if (Hkv == H) return maps + vecs;
  return maps + align256(vecs) + (size_t)2 * H * T * d * sizeof(float);
}

int fa_mi355x_fwd_varlen(const void* q, const void* k, const void* v, float* out, float* lse, const int* cu_seqlens, void* workspace,
                         int nseq, int T, int H, int Hkv, int d, float softmax_scale, int window, int sink, int dtype, void* stream) {
  Call c{};
  c.q = q; c.k = k; c.v = v; c.out = out; c.lse = lse; c.cu = cu_seqlens; c.ws = (char*)workspace;
  c.nseq = nseq; c.T = T; c.H = H; c.Hkv = Hkv; c.d = d; c.scale = softmax_scale; c.W = window; c.S = sink;
  c.dtype = dtype; c.st = (hipStream_t)stream; c.bwd = false;
  return dispatch(c);
}

int fa_mi355x_bwd_varlen(const void* q, const void* k, const void* v, const float* out, const void* out_grad, float* q_grad,
                         float* k_grad, float* v_grad, const float* lse, const int* cu_seqlens, void* workspace, int nseq, int T, int H,
                         int Hkv, int d, float softmax_scale, int window, int sink, int dtype, void* stream) {
  Call c{};
  c.q = q; c.k = k; c.v = v; c.out = const_cast<float*>(out); c.lse = const_cast<float*>(lse); c.dout = out_grad;
  c.dq = q_grad; c.dk = k_grad; c.dv = v_grad; c.cu = cu_seqlens; c.ws = (char*)workspace;
  c.nseq = nseq; c.T = T; c.H = H; c.Hkv = Hkv; c.d = d; c.scale = softmax_scale; c.W = window; c.S = sink;
  c.dtype = dtype; c.st = (hipStream_t)stream; c.bwd = true;
  return dispatch(c);
}

// (its own few checks, in fa_mi355x_rope's order, then the one launch)
int fa_mi355x_rope_varlen(const void* x, void* y, const float* cos, const float* sin, const int* cu_seqlens, int nseq, int T, int H, int d,
                          int rot, int max_pos, int interleaved, int inverse, int dtype, void* stream) {
  g_err[0] = 0;
  if (nseq < 1 || T <= 0 || H <= 0 || d <= 0) return set_err(FA_ERR_BAD_ARG, "nseq, T, H and d must be positive");
  if (dtype != FA_DTYPE_F32 && dtype != FA_DTYPE_BF16) return set_err(FA_ERR_BAD_ARG, "unknown dtype");
  if (!x || !y || !cu_seqlens) return set_err(FA_ERR_BAD_ARG, "null pointer argument (x, y and cu_seqlens)");
  if (!cos || !sin) return set_err(FA_ERR_BAD_ARG, "null cos or sin (the rotary tables, fp32 [max_pos][rot / 2])");
  if (interleaved != 0 && interleaved != 1) return set_err(FA_ERR_BAD_ARG, "interleaved must be 0 (NeoX pairs) or 1 (GPT-J pairs)");
  if (inverse != 0 && inverse != 1) return set_err(FA_ERR_BAD_ARG, "inverse must be 0 or 1");
  if (rot < 2 || rot % 2 != 0 || rot > d) {
    snprintf(g_err, sizeof(g_err), "rot = %d must be even and in 2 .. %d (d)", rot, d);
    return FA_ERR_BAD_ARG;
  }
  if (max_pos <= 0) return set_err(FA_ERR_BAD_ARG, "max_pos must be positive");
  if ((long)T * H * d / 256 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "too many elements for one rope launch");
  fa::RopeVarlenArgs a;
  a.x = x;
  a.y = y;
  a.cos = cos;
  a.sin = sin;
  a.cu = cu_seqlens;
  a.lanes = (long)T * H;
  a.nseq = nseq;
  a.T = T;
  a.H = H;
  a.d = d;
  a.rot = rot;
  a.max_pos = max_pos;
  a.inverse = inverse;
  // 16-byte lanes where the pairs' halves (NeoX) or the pairs (interleaved) fall on whole vectors and every pointer on 16 bytes
  const int esz = dtype == FA_DTYPE_BF16 ? 2 : 4, E = 16 / esz;
  const uintptr_t ptrs = (uintptr_t)x | (uintptr_t)y | (uintptr_t)cos | (uintptr_t)sin;
  const bool vec = (interleaved ? rot : rot / 2) % E == 0 && d % E == 0 && (ptrs & 15) == 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool il = interleaved != 0;
  if (dtype == FA_DTYPE_BF16) return vec ? launch_rope<fa::bf16_t, 8>(a, il, st) : launch_rope<fa::bf16_t, 1>(a, il, st);
  return vec ? launch_rope<float, 4>(a, il, st) : launch_rope<float, 1>(a, il, st);
}

}  // extern "C"
