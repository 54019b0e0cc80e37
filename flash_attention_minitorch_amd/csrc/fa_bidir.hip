// C ABI of libflash_attn_mi355x_bidir.so (include/flash_attn_mi355x_bidir.h): bidirectional attention, forward and backward, on a
// packed batch whose sequences have one length in the query buffers and another in the key buffers.  Validation and dispatch for the
// kernels of fa_bidir.h; the row constants come from bwd_prep_kernel (fa_bwd_dkdv.h), run over all Tq rows as one sequence, and a
// grouped call's dK, dV from group_sum_kernel (fa_aux.h), run over all Tk rows.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <cmath>

#include "../../include/flash_attn_mi355x_bidir.h"
#include "fa_bidir.h"
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
// (both maps are sized for blocks of 128 rows; the key blocks of some builds have 256 and need fewer entries)
inline size_t map_bytes(int T, int nseq) { return align256((size_t)fa::BIDIR_ENTRY_BYTES * (size_t)map_cap(T, nseq, fa::BIDIR_QBLOCK)); }
inline bool sizes_ok(int nseq, int Tq, int Tk, int H, int Hkv, int d) {
  return nseq >= 1 && Tq > 0 && Tk > 0 && H > 0 && d > 0 && Hkv > 0 && H % Hkv == 0;
}

struct Call {
  const void *q, *k, *v, *dout;
  float *out, *lse, *dq, *dk, *dv;
  const int *cu_q, *cu_k;
  char* ws;
  int nseq, Tq, Tk, H, Hkv, d, dtype;
  float scale, tau;
  bool bwd;
  hipStream_t st;
  fa::Layout lay;
};

// The checks of both entry points, in one order, before any HIP call.  Completes the call: tau, lay.
int validate(Call& c) {
  g_err[0] = 0;
  if (c.nseq < 1 || c.Tq <= 0 || c.Tk <= 0 || c.H <= 0 || c.d <= 0) return set_err(FA_ERR_BAD_ARG, "nseq, Tq, Tk, H and d must be positive");
  if (c.Hkv <= 0 || c.H % c.Hkv != 0) return set_err(FA_ERR_BAD_ARG, "Hkv must be positive and divide H");
  if (c.dtype != FA_DTYPE_F32 && c.dtype != FA_DTYPE_BF16) return set_err(FA_ERR_BAD_ARG, "unknown dtype");
  if (!d_supported(c.d)) return set_err(FA_ERR_BAD_ARG, "d must be 32, 64 or 128 (pad other head sizes with zero columns)");
  if (!c.q || !c.k || !c.v || !c.out || !c.lse || !c.cu_q || !c.cu_k || !c.ws || (c.bwd && (!c.dout || !c.dq || !c.dk || !c.dv)))
    return set_err(FA_ERR_BAD_ARG, "null pointer argument");
  if (c.scale != 0.f && (!(c.scale > 0.f) || !std::isfinite(c.scale)))
    return set_err(FA_ERR_BAD_ARG, "softmax_scale must be positive and finite (0: sqrt(1/d))");
  // (T bounds every n_b: what holds for T holds for every sequence's buffer resource; the per-query-head dK, dV have H * d columns)
  if ((long)c.Tq * 128 * 4 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "Tq too large: one head's rows must stay under 2 GiB");
  if ((long)c.Tk * 128 * 4 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "Tk too large: one head's rows must stay under 2 GiB");
  if ((long)c.Tq * c.H * c.d * 4 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "the packed queries must stay under 2 GiB");
  if ((long)c.Tk * c.H * c.d * 4 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "the packed keys must stay under 2 GiB (Tk * H * d * 4)");
  if ((long)c.H * map_cap(c.Tq, c.nseq, fa::BIDIR_QBLOCK) >= (1L << 31) || (long)c.H * map_cap(c.Tk, c.nseq, fa::BIDIR_QBLOCK) >= (1L << 31))
    return set_err(FA_ERR_BAD_ARG, "too many workgroups for one launch");
  if ((uintptr_t)c.ws % 256 != 0) return set_err(FA_ERR_BAD_ARG, "the workspace must be 256-byte aligned");
  c.tau = c.scale > 0.f ? c.scale : sqrtf(1.0f / (float)c.d);
  fa::Layout l{};   // q side [1][Tq][H][d], kv side [1][Tk][Hkv][d]: no key mask, no dropout, no guard
  l.H = c.H;
  l.ld = c.H * c.d;
  l.bstride = (long)c.Tq * c.H * c.d;
  l.hstride = c.d;
  l.mask_heads = 1;
  l.drop_scale = 1.0f;
  l.G = c.H / c.Hkv;
  l.kvH = c.Hkv;
  l.ldk = c.Hkv * c.d;
  c.lay = l;
  return FA_OK;
}

#define FA_BIDIR_LAUNCH(what, kern, grid, block, ...)                                     \
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
  static_assert(32 * NWQ == fa::BIDIR_QBLOCK, "the forward and dQ share one map");
  static_assert(BK >= fa::BIDIR_QBLOCK, "map_bytes sizes the key-block map for blocks of BIDIR_QBLOCK rows");
  const int H = c.H, Tq = c.Tq, Tk = c.Tk;
  const T *q = (const T*)c.q, *k = (const T*)c.k, *v = (const T*)c.v;
  int4* map_q = reinterpret_cast<int4*>(c.ws);
  const int cap_q = (int)map_cap(Tq, c.nseq, fa::BIDIR_QBLOCK);
  fa::BidirFill fill{};
  fill.H = H;
  fill.ldq = fill.ldk = c.lay.ld;
  if (!c.bwd) {
    fill.qmat = c.out;
    fill.rowc = c.lse;
    FA_BIDIR_LAUNCH("bidir_schedule_kernel", fa::bidir_schedule_kernel, 1 + fa::BIDIR_FILL_BLOCKS, 256, c.cu_q, c.cu_k, c.nseq, Tq, Tk,
                    map_q, cap_q, (int4*)nullptr, 0, 0, fill);
    FA_BIDIR_LAUNCH("bidir_fwd_kernel", (fa::bidir_fwd_kernel<T, D, BN>), H * cap_q, 256, q, k, v, c.out, c.lse, (const int4*)map_q, Tq,
                    Tk, cap_q, H, c.lay, c.tau);
    return FA_OK;
  }
  const size_t mbq = map_bytes(Tq, c.nseq), mbk = map_bytes(Tk, c.nseq);
  int4* map_k = reinterpret_cast<int4*>(c.ws + mbq);
  const int cap_k = (int)map_cap(Tk, c.nseq, BK);
  const long rows = (long)H * Tq, krows = (long)H * Tk;
  float *nlc = reinterpret_cast<float*>(c.ws + mbq + mbk), *ndelta = nlc + rows, *nl2 = nlc + 2 * rows;
  float *dk = c.dk, *dv = c.dv;
  if (c.lay.G > 1) {   // per query head into the scratch behind the row constants
    dk = reinterpret_cast<float*>(c.ws + mbq + mbk + align256((size_t)WS_VECS * rows * sizeof(float)));
    dv = dk + (size_t)krows * D;
  }   // (ungrouped: Hkv == H, k_grad and v_grad have the same H * d columns)
  // (the group sum reads all Tk rows of the per-query-head dK, dV: their unowned rows are zeroed, and its sums are then zeros)
  fill.qmat = c.dq;
  fill.kmat[0] = dk;
  fill.kmat[1] = dv;
  FA_BIDIR_LAUNCH("bidir_schedule_kernel", fa::bidir_schedule_kernel, 1 + fa::BIDIR_FILL_BLOCKS, 256, c.cu_q, c.cu_k, c.nseq, Tq, Tk, map_q,
                  cap_q, map_k, BK, cap_k, fill);
  const T* dout = (const T*)c.dout;
  constexpr int RPB = 256 / (D / 8);
  FA_BIDIR_LAUNCH("bwd_prep_kernel", (fa::bwd_prep_kernel<T, D>), (int)((rows + RPB - 1) / RPB), 256, (const float*)c.out, dout,
                  (const float*)c.lse, (const float*)nullptr, nlc, ndelta, nl2, rows, Tq, c.lay, fa::AUX_FA2, 1.0f / c.tau);
  FA_BIDIR_LAUNCH("bidir_dkdv_kernel", (fa::bidir_dkdv_kernel<T, D, NW, QS>), H * cap_k, NW * 64, q, k, v, dout, (const float*)nlc,
                  (const float*)ndelta, dk, dv, (const int4*)map_k, Tq, Tk, cap_k, H, c.lay, c.tau);
  if (c.lay.G > 1)
    FA_BIDIR_LAUNCH("group_sum_kernel", fa::group_sum_kernel, (int)((krows / c.lay.G * (D / 4) + 255) / 256), 256, (const float*)dk,
                    (const float*)dv, c.dk, c.dv, krows / c.lay.G * (D / 4), (long)(D / 4), c.lay.G);
  FA_BIDIR_LAUNCH("bidir_dq_kernel", (fa::bidir_dq_kernel<T, D, NWQ>), H * cap_q, 64 * NWQ, q, k, v, dout, (const float*)nlc,
                  (const float*)ndelta, c.dq, (const int4*)map_q, Tq, Tk, cap_q, H, c.lay, c.tau);
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

}  // namespace

extern "C" {

const char* fa_mi355x_bidir_last_error(void) { return g_err; }

size_t fa_mi355x_fwd_bidir_workspace_bytes(int nseq, int Tq, int Tk, int H, int Hkv, int d) {
  if (!sizes_ok(nseq, Tq, Tk, H, Hkv, d)) return 0;
  return map_bytes(Tq, nseq);
}

size_t fa_mi355x_bwd_bidir_workspace_bytes(int nseq, int Tq, int Tk, int H, int Hkv, int d) {
  if (!sizes_ok(nseq, Tq, Tk, H, Hkv, d)) return 0;
  const long double est = 2.0L * H * Tk * d * 4 + 3.0L * H * Tq * 4 + 32.0L * ((long double)Tq + Tk + 2.0L * nseq) + 1024;
  if (est >= 4.0e18L) return 0;   // (past 2^62)
  const size_t vecs = (size_t)WS_VECS * H * Tq * sizeof(float);
  const size_t maps = map_bytes(Tq, nseq) + map_bytes(Tk, nseq);
  if (Hkv == H) return maps + vecs;
  return maps + align256(vecs) + (size_t)2 * H * Tk * d * sizeof(float);
}

int fa_mi355x_fwd_bidir(const void* q, const void* k, const void* v, float* out, float* lse, const int* cu_seqlens_q,
                        const int* cu_seqlens_k, void* workspace, int nseq, int Tq, int Tk, int H, int Hkv, int d, float softmax_scale,
                        int dtype, void* stream) {
  Call c{};
  c.q = q; c.k = k; c.v = v; c.out = out; c.lse = lse; c.cu_q = cu_seqlens_q; c.cu_k = cu_seqlens_k; c.ws = (char*)workspace;
  c.nseq = nseq; c.Tq = Tq; c.Tk = Tk; c.H = H; c.Hkv = Hkv; c.d = d; c.scale = softmax_scale;
  c.dtype = dtype; c.st = (hipStream_t)stream; c.bwd = false;
  return dispatch(c);
}

int fa_mi355x_bwd_bidir(const void* q, const void* k, const void* v, const float* out, const void* out_grad, float* q_grad,
                        float* k_grad, float* v_grad, const float* lse, const int* cu_seqlens_q, const int* cu_seqlens_k, void* workspace,
                        int nseq, int Tq, int Tk, int H, int Hkv, int d, float softmax_scale, int dtype, void* stream) {
  Call c{};
  c.q = q; c.k = k; c.v = v; c.out = const_cast<float*>(out); c.lse = const_cast<float*>(lse); c.dout = out_grad;
  c.dq = q_grad; c.dk = k_grad; c.dv = v_grad; c.cu_q = cu_seqlens_q; c.cu_k = cu_seqlens_k; c.ws = (char*)workspace;
  c.nseq = nseq; c.Tq = Tq; c.Tk = Tk; c.H = H; c.Hkv = Hkv; c.d = d; c.scale = softmax_scale;
  c.dtype = dtype; c.st = (hipStream_t)stream; c.bwd = true;
  return dispatch(c);
}

}  // extern "C"
