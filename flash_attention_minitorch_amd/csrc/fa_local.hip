// C ABI of libflash_attn_mi355x_local.so (include/flash_attn_mi355x_local.h): attention under a two-sided sliding window, forward and
// backward, on a packed batch whose sequences have one length in the query buffers and another in the key buffers (the queries are
// the last positions of the keys).  This library's checks (those of fa_bidir.hip, with its messages, and the window's) and the
// launches of the kernels of fa_local.h, behind fa_bidir.h's schedule kernel; what the training-side libraries share is in
// fa_side_host.h.  The row constants (bwd_prep_kernel) are run over all Tq rows as one sequence, a grouped call's dK, dV
// (group_sum_kernel) over all Tk rows.  The launches are fa_prefix.hip's: neither the grids nor the workspace know the window.
#include "../../include/flash_attn_mi355x_local.h"
#include "fa_local.h"
#include "fa_side_host.h"

namespace {

// (both maps are sized for blocks of 128 rows; the key blocks of some builds have 256 and need fewer entries)
inline size_t local_map_bytes(int T, int nseq) { return map_bytes(T, nseq, fa::BIDIR_ENTRY_BYTES, fa::BIDIR_QBLOCK); }

struct Call : SideCall {
  const int *cu_q, *cu_k;
  int nseq, Tq, Tk;
  int wl, wr;   // the caller's window; validate() turns an unbounded side into a bound no sequence reaches
};

// The checks of both entry points, in one order, before any HIP call.  Completes the call: tau, lay, the window's bounds.
int validate(Call& c) {
  g_err[0] = 0;
  if (c.nseq < 1 || c.Tq <= 0 || c.Tk <= 0 || c.H <= 0 || c.d <= 0) return set_err(FA_ERR_BAD_ARG, "nseq, Tq, Tk, H and d must be positive");
  if (int rc = check_heads(c)) return rc;
  if (int rc = check_dtype(c)) return rc;
  if (int rc = check_d(c)) return rc;
  if (!c.q || !c.k || !c.v || !c.out || !c.lse || !c.cu_q || !c.cu_k || !c.ws || (c.bwd && (!c.dout || !c.dq || !c.dk || !c.dv)))
    return set_err(FA_ERR_BAD_ARG, "null pointer argument");
  if (int rc = check_scale(c)) return rc;
  if (c.wl < -1) return set_err(FA_ERR_BAD_ARG, "window_left must be -1 (unbounded) or >= 0");
  if (c.wr < -1) return set_err(FA_ERR_BAD_ARG, "window_right must be -1 (unbounded) or >= 0");
  // (T bounds every n_b: what holds for T holds for every sequence's buffer resource; the per-query-head dK, dV have H * d columns)
  if ((long)c.Tq * 128 * 4 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "Tq too large: one head's rows must stay under 2 GiB");
  if ((long)c.Tk * 128 * 4 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "Tk too large: one head's rows must stay under 2 GiB");
  if ((long)c.Tq * c.H * c.d * 4 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "the packed queries must stay under 2 GiB");
  if ((long)c.Tk * c.H * c.d * 4 >= (1L << 31)) return set_err(FA_ERR_BAD_ARG, "the packed keys must stay under 2 GiB (Tk * H * d * 4)");
  if ((long)c.H * map_cap(c.Tq, c.nseq, fa::BIDIR_QBLOCK) >= (1L << 31) || (long)c.H * map_cap(c.Tk, c.nseq, fa::BIDIR_QBLOCK) >= (1L << 31))
    return set_err(FA_ERR_BAD_ARG, "too many workgroups for one launch");
  if (int rc = check_ws_aligned(c, "the workspace must be 256-byte aligned")) return rc;
  c.tau = tau_of(c);
  c.lay = side_layout(true, c.Tq, c.H, c.Hkv, c.d);   // q side [1][Tq][H][d], kv side [1][Tk][Hkv][d]
  // (positions stay under 2^22 by the bounds above: a side of LOCAL_UNBOUNDED or more is one no sequence reaches)
  c.wl = c.wl < 0 || c.wl > fa::LOCAL_UNBOUNDED ? fa::LOCAL_UNBOUNDED : c.wl;
  c.wr = c.wr < 0 || c.wr > fa::LOCAL_UNBOUNDED ? fa::LOCAL_UNBOUNDED : c.wr;
  return FA_OK;
}

// The workspace: the query-block map, (backward) the key-block map, the row constants, (grouped) the per-query-head dK and dV.
template <typename T, int D>
int run(const Call& c) {
  using Ti = SideTiles<T, D>;
  constexpr int BN = Ti::BN, NWQ = Ti::NWQ, NW = Ti::NW, QS = Ti::QS, BK = Ti::BK;
  static_assert(32 * NWQ == fa::BIDIR_QBLOCK, "the forward and dQ share one map");
  static_assert(BK >= fa::BIDIR_QBLOCK, "local_map_bytes sizes the key-block map for blocks of BIDIR_QBLOCK rows");
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
    FA_SIDE_LAUNCH("bidir_schedule_kernel", fa::bidir_schedule_kernel, 1 + fa::BIDIR_FILL_BLOCKS, 256, c.cu_q, c.cu_k, c.nseq, Tq, Tk,
                   map_q, cap_q, (int4*)nullptr, 0, 0, fill);
    FA_SIDE_LAUNCH("local_fwd_kernel", (fa::local_fwd_kernel<T, D, BN>), H * cap_q, 256, q, k, v, c.out, c.lse, (const int4*)map_q, Tq,
                   Tk, cap_q, H, c.lay, c.tau, c.wl, c.wr);
    return FA_OK;
  }
  const size_t mbq = local_map_bytes(Tq, c.nseq), mbk = local_map_bytes(Tk, c.nseq);
  int4* map_k = reinterpret_cast<int4*>(c.ws + mbq);
  const int cap_k = (int)map_cap(Tk, c.nseq, BK);
  const long rows = (long)H * Tq, krows = (long)H * Tk;
  const BwdScratch s(c, c.ws + mbq + mbk, rows, krows);   // (ungrouped: Hkv == H, k_grad and v_grad have the same H * d columns)
  // (the group sum reads all Tk rows of the per-query-head dK, dV: their unowned rows are zeroed, and its sums are then zeros)
  fill.qmat = c.dq;
  fill.kmat[0] = s.dk;
  fill.kmat[1] = s.dv;
  FA_SIDE_LAUNCH("bidir_schedule_kernel", fa::bidir_schedule_kernel, 1 + fa::BIDIR_FILL_BLOCKS, 256, c.cu_q, c.cu_k, c.nseq, Tq, Tk, map_q,
                 cap_q, map_k, BK, cap_k, fill);
  const T* dout = (const T*)c.dout;
  if (int rc = launch_bwd_prep<T, D>(c, s, rows, Tq, 1.0f / c.tau)) return rc;
  FA_SIDE_LAUNCH("local_dkdv_kernel", (fa::local_dkdv_kernel<T, D, NW, QS>), H * cap_k, NW * 64, q, k, v, dout, (const float*)s.nlc,
                 (const float*)s.ndelta, s.dk, s.dv, (const int4*)map_k, Tq, Tk, cap_k, H, c.lay, c.tau, c.wl, c.wr);
  if (c.lay.G > 1)
    if (int rc = launch_group_sum(c, s, krows, D / 4)) return rc;
  FA_SIDE_LAUNCH("local_dq_kernel", (fa::local_dq_kernel<T, D, NWQ>), H * cap_q, 64 * NWQ, q, k, v, dout, (const float*)s.nlc,
                 (const float*)s.ndelta, c.dq, (const int4*)map_q, Tq, Tk, cap_q, H, c.lay, c.tau, c.wl, c.wr);
  return FA_OK;
}

int dispatch(Call& c) {
  if (int rc = validate(c)) return rc;
  return side_dispatch(c, [&](auto t, auto d) { return run<typename decltype(t)::type, decltype(d)::value>(c); });
}

}  // namespace

extern "C" {

const char* fa_mi355x_local_last_error(void) { return g_err; }

size_t fa_mi355x_fwd_local_workspace_bytes(int nseq, int Tq, int Tk, int H, int Hkv, int d) {
  if (!packed_sizes_ok(nseq, Tq, Tk, H, Hkv, d)) return 0;
  return local_map_bytes(Tq, nseq);
}

size_t fa_mi355x_bwd_local_workspace_bytes(int nseq, int Tq, int Tk, int H, int Hkv, int d) {
  if (!packed_sizes_ok(nseq, Tq, Tk, H, Hkv, d)) return 0;
  const long double est = 2.0L * H * Tk * d * 4 + 3.0L * H * Tq * 4 + 32.0L * ((long double)Tq + Tk + 2.0L * nseq) + 1024;
  if (est >= 4.0e18L) return 0;   // (past 2^62)
  return local_map_bytes(Tq, nseq) + local_map_bytes(Tk, nseq) + bwd_scratch_bytes((size_t)H * Tq, (size_t)H * Tk, d, Hkv < H);
}

int fa_mi355x_fwd_local(const void* q, const void* k, const void* v, float* out, float* lse, const int* cu_seqlens_q,
                        const int* cu_seqlens_k, void* workspace, int nseq, int Tq, int Tk, int H, int Hkv, int d, float softmax_scale,
                        int window_left, int window_right, int dtype, void* stream) {
  Call c{side_call(q, k, v, out, lse, workspace, H, Hkv, d, softmax_scale, dtype, stream), cu_seqlens_q, cu_seqlens_k, nseq, Tq, Tk,
         window_left, window_right};
  return dispatch(c);
}

int fa_mi355x_bwd_local(const void* q, const void* k, const void* v, const float* out, const void* out_grad, float* q_grad,
                        float* k_grad, float* v_grad, const float* lse, const int* cu_seqlens_q, const int* cu_seqlens_k, void* workspace,
                        int nseq, int Tq, int Tk, int H, int Hkv, int d, float softmax_scale, int window_left, int window_right,
                        int dtype, void* stream) {
  Call c{side_call(q, k, v, out, lse, workspace, H, Hkv, d, softmax_scale, dtype, stream), cu_seqlens_q, cu_seqlens_k, nseq, Tq, Tk,
         window_left, window_right};
  set_bwd(c, out_grad, q_grad, k_grad, v_grad);
  return dispatch(c);
}

}  // extern "C"
