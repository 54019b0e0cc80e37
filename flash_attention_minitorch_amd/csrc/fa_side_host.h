// Host core of the training-side libraries (fa_window.hip, fa_varlen.hip, fa_bidir.hip), included by each after its public header
// and its kernel header: the error buffer, the checks all of them make, the fa::Layout of their tensors, the per-(dtype, d) tile
// shapes and dispatch, the backward's workspace layout with the two launches that go with it (bwd_prep_kernel of fa_bwd_dkdv.h,
// group_sum_kernel of fa_aux.h) and the block-map sizing of the packed libraries.  Host code only; everything has internal linkage,
// so every library keeps an error buffer of its own behind its own *_last_error.  A library's .hip is left with its Call, its own
// checks, its attention-kernel launches and its entry points ("The host core of the training-side libraries").
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <cmath>

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

// What every call carries; a library's Call adds its geometry.  validate completes tau and lay.
struct SideCall {
  const void *q, *k, *v, *dout;
  float *out, *lse, *dq, *dk, *dv;
  char* ws;
  int H, Hkv, d, dtype;
  float scale, tau;
  bool bwd;
  hipStream_t st;
  fa::Layout lay;
};

// The fields every entry point fills; a backward adds its own (set_bwd).
inline SideCall side_call(const void* q, const void* k, const void* v, const float* out, const float* lse, void* ws, int H, int Hkv, int d,
                          float scale, int dtype, void* stream) {
  SideCall c{};
  c.q = q; c.k = k; c.v = v; c.out = const_cast<float*>(out); c.lse = const_cast<float*>(lse); c.ws = (char*)ws;
  c.H = H; c.Hkv = Hkv; c.d = d; c.scale = scale; c.dtype = dtype; c.st = (hipStream_t)stream;
  return c;
}
inline void set_bwd(SideCall& c, const void* dout, float* dq, float* dk, float* dv) {
  c.dout = dout; c.dq = dq; c.dk = dk; c.dv = dv; c.bwd = true;
}

// in a function that returns a status, with the call as c
#define FA_SIDE_LAUNCH(what, kern, grid, block, ...)                                      \
  do {                                                                                    \
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, c.st, __VA_ARGS__);              \
    const hipError_t e_ = hipGetLastError();                                              \
    if (e_ != hipSuccess) return set_err(FA_ERR_HIP, what " launch", e_);                 \
  } while (0)

// The checks of every library, each FA_OK or the error set; a library's validate calls them in its own order, between its own.
inline int check_heads(const SideCall& c) {
  return c.Hkv > 0 && c.H % c.Hkv == 0 ? FA_OK : set_err(FA_ERR_BAD_ARG, "Hkv must be positive and divide H");
}
inline int check_dtype(const SideCall& c) {
  return c.dtype == FA_DTYPE_F32 || c.dtype == FA_DTYPE_BF16 ? FA_OK : set_err(FA_ERR_BAD_ARG, "unknown dtype");
}
inline int check_d(const SideCall& c) {
  return d_supported(c.d) ? FA_OK : set_err(FA_ERR_BAD_ARG, "d must be 32, 64 or 128 (pad other head sizes with zero columns)");
}
inline int check_scale(const SideCall& c) {
  if (c.scale == 0.f || (c.scale > 0.f && std::isfinite(c.scale))) return FA_OK;
  return set_err(FA_ERR_BAD_ARG, "softmax_scale must be positive and finite (0: sqrt(1/d))");
}
inline int check_ws_aligned(const SideCall& c, const char* what) {
  return (uintptr_t)c.ws % 256 == 0 ? FA_OK : set_err(FA_ERR_BAD_ARG, what);
}
inline float tau_of(const SideCall& c) { return c.scale > 0.f ? c.scale : sqrtf(1.0f / (float)c.d); }

// q-side tensors [B][n][H][d] (rows_by_head; a packed batch is B = 1) or [B][H][n][d], the kv side with Hkv heads: no key mask, no
// dropout, no guard.  (G == 1: Hkv == H, and kvH, ldk are the q side's H, ld.)
inline fa::Layout side_layout(bool rows_by_head, long n, int H, int Hkv, int d) {
  fa::Layout l{};
  l.H = rows_by_head ? H : 1;
  l.ld = rows_by_head ? H * d : d;
  l.bstride = rows_by_head ? n * H * d : n * d;
  l.hstride = rows_by_head ? d : 0;
  l.mask_heads = 1;
  l.drop_scale = 1.0f;
  l.G = H / Hkv;
  l.kvH = rows_by_head ? Hkv : 1;
  l.ldk = rows_by_head ? Hkv * d : d;
  return l;
}

// The per-(dtype, d) tile shapes are those of the phased kernels in fa_api.hip, in the builds that carry the split-operand path:
// forward key tile BN 64 (bf16) / 32 (fp32); dQ with NWQ = 4 waves; dK/dV with NW = 8 waves and QS = 128-query slices for bf16 at
// d <= 64, 4 waves and 64-query slices at d = 128 (one wave per SIMD: the whole register file, no scratch), 4 waves and 32-query
// slices for fp32.  BK: the key rows of a dK/dV block.
template <typename T, int D> struct SideTiles {
  static constexpr bool BF = sizeof(T) == 2;
  static constexpr int BN = BF ? 64 : 32, NWQ = 4, NW = (BF && D < 128) ? 8 : 4, QS = BF ? (D == 128 ? 64 : 128) : 32, BK = NW * 32;
};

// f(type_tag<T>{}, fa::ic<D>{}) for the call's dtype and d (both checked): a library's dispatch passes a generic lambda that calls
// its run<T, D>
template <typename T> struct type_tag { using type = T; };
template <typename F> int side_dispatch(const SideCall& c, F&& f) {
  if (c.dtype == FA_DTYPE_BF16) {
    if (c.d == 32) return f(type_tag<fa::bf16_t>{}, fa::ic<32>{});
    if (c.d == 64) return f(type_tag<fa::bf16_t>{}, fa::ic<64>{});
    return f(type_tag<fa::bf16_t>{}, fa::ic<128>{});
  }
  if (c.d == 32) return f(type_tag<float>{}, fa::ic<32>{});
  if (c.d == 64) return f(type_tag<float>{}, fa::ic<64>{});
  return f(type_tag<float>{}, fa::ic<128>{});
}

// The backward's scratch: the three row-constant vectors of `rows` query rows and, behind them (256-byte aligned) when the heads are
// grouped, the dK and dV of every query head, `krows` rows of d floats each, which group_sum_kernel then adds into the caller's.
// bwd_scratch_bytes is what BwdScratch carves: the *_workspace_bytes functions and the run functions both go through here.
inline size_t bwd_scratch_bytes(size_t rows, size_t krows, int d, bool grouped) {
  const size_t vecs = (size_t)WS_VECS * rows * sizeof(float);
  return grouped ? align256(vecs) + 2 * krows * d * sizeof(float) : vecs;
}
struct BwdScratch {
  float *nlc, *ndelta, *nl2, *dk, *dv;   // dk, dv: where the dK/dV kernel stores (ungrouped: the caller's)
  BwdScratch(const SideCall& c, char* base, long rows, long krows)
      : nlc((float*)base), ndelta(nlc + rows), nl2(nlc + 2 * rows), dk(c.dk), dv(c.dv) {
    if (c.lay.G > 1) {
      dk = reinterpret_cast<float*>(base + bwd_scratch_bytes(rows, 0, c.d, true));
      dv = dk + (size_t)krows * c.d;
    }
  }
};

// The row constants of all `rows` query rows, n to a (batch element, head); factor: 1 / tau, or 1 under a logit cap.
template <typename T, int D> int launch_bwd_prep(const SideCall& c, const BwdScratch& s, long rows, int n, float factor) {
  constexpr int RPB = 256 / (D / 8);
  FA_SIDE_LAUNCH("bwd_prep_kernel", (fa::bwd_prep_kernel<T, D>), (int)((rows + RPB - 1) / RPB), 256, (const float*)c.out, (const T*)c.dout,
                 (const float*)c.lse, (const float*)nullptr, s.nlc, s.ndelta, s.nl2, rows, n, c.lay, fa::AUX_FA2, factor);
  return FA_OK;
}

// A grouped call's dK, dV from the per-query-head ones.  inner: 16-byte chunks between the heads of a group ([..][n][H][d]: d / 4;
// [B][H][n][d]: n * d / 4).
inline int launch_group_sum(const SideCall& c, const BwdScratch& s, long krows, long inner) {
  const long chunks = krows / c.lay.G * (c.d / 4);
  FA_SIDE_LAUNCH("group_sum_kernel", fa::group_sum_kernel, (int)((chunks + 255) / 256), 256, (const float*)s.dk, (const float*)s.dv, c.dk,
                 c.dv, chunks, inner, c.lay.G);
  return FA_OK;
}

// The packed libraries' block maps: at most T / qblock + nseq blocks of qblock rows, one entry each.
inline long map_cap(int T, int nseq, int bs) { return (long)T / bs + nseq; }
inline size_t map_bytes(int T, int nseq, int entry_bytes, int qblock) {
  return align256((size_t)entry_bytes * (size_t)map_cap(T, nseq, qblock));
}
inline bool packed_sizes_ok(int nseq, int Tq, int Tk, int H, int Hkv, int d) {
  return nseq >= 1 && Tq > 0 && Tk > 0 && H > 0 && d > 0 && Hkv > 0 && H % Hkv == 0;
}

}  // namespace
