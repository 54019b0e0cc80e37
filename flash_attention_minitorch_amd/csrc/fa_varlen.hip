// C ABI of libflash_attn_mi355x_varlen.so (include/flash_attn_mi355x_varlen.h): causal attention, windowed or not, forward and
// backward, on a packed batch of sequences of different lengths, and the rotary embedding that restarts at every sequence.
// This library's checks and the launches of the kernels of fa_varlen.h; what the training-side libraries share is in
// fa_side_host.h.  The row constants (bwd_prep_kernel) and a grouped call's dK, dV (group_sum_kernel) are run over all T rows as one
// sequence, as fa_window.hip runs them.
#include <limits.h>

#include "../../include/flash_attn_mi355x_varlen.h"
#include "fa_varlen.h"
#include "fa_side_host.h"

namespace {

inline size_t varlen_map_bytes(int T, int nseq) { return map_bytes(T, nseq, sizeof(int4), fa::VARLEN_QBLOCK); }

struct Call : SideCall {
  const int* cu;
  int nseq, T, W, S;
};

// The checks of both entry points, in one order, before any HIP call.  Completes the call: tau, W (no window: every j <= i), lay.
int validate(Call& c) {
  g_err[0] = 0;
  if (c.nseq < 1 || c.T <= 0 || c.H <= 0 || c.d <= 0) return set_err(FA_ERR_BAD_ARG, "nseq, T, H and d must be positive");
  if (int rc = check_heads(c)) return rc;
  if (c.W < 0) return set_err(FA_ERR_BAD_ARG, "window must not be negative (0: no window)");
  if (c.S < 0) return set_err(FA_ERR_BAD_ARG, "sink must not be negative");
  if (c.S > 0 && c.W == 0) return set_err(FA_ERR_BAD_ARG, "sink tokens need a window");
  if (int rc = check_dtype(c)) return rc;
  if (int rc = check_d(c)) return rc;
  if (!c.q || !c.k || !c.v || !c.out || !c.lse || !c.cu || !c.ws || (c.bwd && (!c.dout || !c.dq || !c.dk || !c.dv)))
    return set_err(FA_ERR_BAD_ARG, "null pointer argument");
  if (int rc = check_scale(c)) return rc;
  // (T bounds every n_b: what holds for T holds for every sequence's buffer resource)
  if ((long)c.T * 128 * 4 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "T too large: one head's rows must stay under 2 GiB");
  if ((long)c.T * c.H * c.d * 4 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "the packed batch must stay under 2 GiB");
  if ((long)c.H * map_cap(c.T, c.nseq, fa::VARLEN_QBLOCK) >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "too many workgroups for one launch");
  if (int rc = check_ws_aligned(c, "the workspace must be 256-byte aligned")) return rc;
  c.tau = tau_of(c);
  if (c.W == 0) c.W = INT_MAX;   // (the kernels clamp W and S to the sequence's length)
  c.lay = side_layout(true, c.T, c.H, c.Hkv, c.d);   // [1][T][H][d]
  return FA_OK;
}

// The workspace: the query-block map, (backward) the key-block map, the row constants, (grouped) the per-query-head dK and dV.
template <typename T, int D>
int run(const Call& c) {
  using Ti = SideTiles<T, D>;
  constexpr int BN = Ti::BN, NWQ = Ti::NWQ, NW = Ti::NW, QS = Ti::QS, BK = Ti::BK;
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
    FA_SIDE_LAUNCH("varlen_schedule_kernel", fa::varlen_schedule_kernel, 1 + fa::VARLEN_FILL_BLOCKS, 256, c.cu, c.nseq, Tn, map_q,
                   cap_q, (int4*)nullptr, 0, 0, fill);
    FA_SIDE_LAUNCH("varlen_fwd_kernel", (fa::varlen_fwd_kernel<T, D, BN>), H * cap_q, 256, q, k, v, c.out, c.lse,
                   (const int4*)map_q, Tn, cap_q, H, c.lay, c.tau, c.W, c.S);
    return FA_OK;
  }
  const size_t mb = varlen_map_bytes(Tn, c.nseq);
  int4* map_k = reinterpret_cast<int4*>(c.ws + mb);
  const int cap_k = (int)map_cap(Tn, c.nseq, BK);
  const long rows = (long)H * Tn;
  const BwdScratch s(c, c.ws + 2 * mb, rows, rows);
  // (the group sum reads all T rows of the per-query-head dK, dV: their unowned rows are zeroed, and its sums are then zeros)
  fill.mat[0] = c.dq;
  fill.mat[1] = s.dk;
  fill.mat[2] = s.dv;
  fill.ld[0] = fill.ld[1] = fill.ld[2] = c.lay.ld;
  FA_SIDE_LAUNCH("varlen_schedule_kernel", fa::varlen_schedule_kernel, 1 + fa::VARLEN_FILL_BLOCKS, 256, c.cu, c.nseq, Tn, map_q, cap_q,
                 map_k, BK, cap_k, fill);
  const T* dout = (const T*)c.dout;
  if (int rc = launch_bwd_prep<T, D>(c, s, rows, Tn, 1.0f / c.tau)) return rc;
  FA_SIDE_LAUNCH("varlen_dkdv_kernel", (fa::varlen_dkdv_kernel<T, D, NW, QS>), H * cap_k, NW * 64, q, k, v, dout, (const float*)s.nlc,
                 (const float*)s.ndelta, s.dk, s.dv, (const int4*)map_k, Tn, cap_k, H, c.lay, c.tau, c.W, c.S);
  if (c.lay.G > 1)
    if (int rc = launch_group_sum(c, s, rows, D / 4)) return rc;
  FA_SIDE_LAUNCH("varlen_dq_kernel", (fa::varlen_dq_kernel<T, D, NWQ>), H * cap_q, 64 * NWQ, q, k, v, dout, (const float*)s.nlc,
                 (const float*)s.ndelta, c.dq, (const int4*)map_q, Tn, cap_q, H, c.lay, c.tau, c.W, c.S);
  return FA_OK;
}

int dispatch(Call& c) {
  if (int rc = validate(c)) return rc;
  return side_dispatch(c, [&](auto t, auto d) { return run<typename decltype(t)::type, decltype(d)::value>(c); });
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
  if (!packed_sizes_ok(nseq, T, T, H, Hkv, d)) return 0;
  return varlen_map_bytes(T, nseq);
}

size_t fa_mi355x_bwd_varlen_workspace_bytes(int nseq, int T, int H, int Hkv, int d) {
  if (!packed_sizes_ok(nseq, T, T, H, Hkv, d)) return 0;
  const long double est = 2.0L * H * T * d * 4 + 3.0L * H * T * 4 + 32.0L * ((long double)T + nseq) + 1024;
  if (est >= 4.0e18L) return 0;   // (past 2^62)
  return 2 * varlen_map_bytes(T, nseq) + bwd_scratch_bytes((size_t)H * T, (size_t)H * T, d, Hkv < H);
}

int fa_mi355x_fwd_varlen(const void* q, const void* k, const void* v, float* out, float* lse, const int* cu_seqlens, void* workspace,
                         int nseq, int T, int H, int Hkv, int d, float softmax_scale, int window, int sink, int dtype, void* stream) {
  Call c{side_call(q, k, v, out, lse, workspace, H, Hkv, d, softmax_scale, dtype, stream), cu_seqlens, nseq, T, window, sink};
  return dispatch(c);
}

int fa_mi355x_bwd_varlen(const void* q, const void* k, const void* v, const float* out, const void* out_grad, float* q_grad,
                         float* k_grad, float* v_grad, const float* lse, const int* cu_seqlens, void* workspace, int nseq, int T, int H,
                         int Hkv, int d, float softmax_scale, int window, int sink, int dtype, void* stream) {
  Call c{side_call(q, k, v, out, lse, workspace, H, Hkv, d, softmax_scale, dtype, stream), cu_seqlens, nseq, T, window, sink};
  set_bwd(c, out_grad, q_grad, k_grad, v_grad);
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
